// plan_check.cpp -- stand-alone driver of the C ABI of include/wd_hip.h over tests/c/fake_hip_runtime.cpp.
//
// Compiled TOGETHER with warp_drive_amd/csrc/wd_runtime.cpp (not against libwdhip.so), so that a sanitizer build
// instruments the code under test.  Usage:
//     plan_check <absolute path of the fake> <scenario name> <op> <op> ...
// A scenario is a list of operations, each ONE argument of comma-separated words (tests/test_launch_plan_host.py holds
// the scenarios and every expectation; this program expects nothing).  Per operation it prints
//     > <op>
//     rc=<return code> err=<wd_last_error() when rc != 0> [further results]
//     | <each line the fake logged during the operation>
// and at the end the fake's live handles by kind.  It exits 0 unless it could not load the fake or parse an operation.
//
// Operations (numbers in C notation; FN is a number standing for a hipFunction_t; STREAM is `caller` or `null`;
// LAUNCH = FN,gx,gy,gz,bx,by,bz,lds ; BUF = n_bytes,seed -- byte i of an argument buffer is (seed + 7 * i) & 255):
//     init | init_path,PATH | malloc,BYTES | sync,STREAM | launch_packed,LAUNCH,STREAM,BUF | launch,LAUNCH,STREAM,N
//     plan | add,LAUNCH,BUF | size | add_cohort,ENTRY,COHORT,LAUNCH,BUF | cohorts | multi,LAUNCH,BUF,OFFSET,MAX_TICKS
//     run,REPEATS,STREAM | timing,ENTRY,STRIDE,MAX_SAMPLES | read | graph,REPS,STREAM | run_graph,LAUNCHES,STREAM
//     destroy | fail,CALL,NTH,ERROR | live
#include <dlfcn.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "wd_hip.h"

namespace {

struct Fake {
  void (*fail)(const char *, int, int);
  long (*log_size)(void);
  const char *(*log_line)(long);
  int (*live)(const char *);
  int (*errors)(void);
  void *(*caller_stream)(void);
} fake;

template <class T> void bind(void *lib, const char *name, T &fn) {
  fn = reinterpret_cast<T>(dlsym(lib, name));
  if (!fn) {
    fprintf(stderr, "plan_check: the fake lacks %s\n", name);
    exit(2);
  }
}

std::vector<std::string> words(const std::string &op) {
  std::vector<std::string> w(1);
  for (char c : op)
    if (c == ',') w.emplace_back(); else w.back() += c;
  return w;
}

struct Args {
  std::vector<std::string> w;
  size_t at = 1;
  const std::string &word() {
    if (at >= w.size()) {
      fprintf(stderr, "plan_check: `%s` needs more words\n", w[0].c_str());
      exit(2);
    }
    return w[at++];
  }
  long num() { return strtol(word().c_str(), nullptr, 0); }
  void *stream() {
    const std::string &s = word();
    if (s == "null") return nullptr;
    if (s == "caller") return fake.caller_stream();
    fprintf(stderr, "plan_check: stream `%s`\n", s.c_str());
    exit(2);
  }
  std::vector<unsigned char> buffer() {
    const long n = num(), seed = num();
    std::vector<unsigned char> b(n + 1);  // (never empty: a pointer to pass for 0 bytes too)
    for (long i = 0; i < n; ++i) b[i] = static_cast<unsigned char>(seed + 7 * i);
    b.resize(n);
    return b;
  }
};

struct Launch {
  void *fn;
  uint32_t g[3], b[3], lds;
};
Launch launch_of(Args &a) {
  Launch l;
  l.fn = reinterpret_cast<void *>(static_cast<uintptr_t>(a.num()));
  for (auto &v : l.g) v = static_cast<uint32_t>(a.num());
  for (auto &v : l.b) v = static_cast<uint32_t>(a.num());
  l.lds = static_cast<uint32_t>(a.num());
  return l;
}

long printed = 0;
void report(int rc, const std::string &more = "") {
  printf("rc=%d err=%s%s%s\n", rc, rc ? wd_last_error() : "", more.empty() ? "" : " ", more.c_str());
  for (const long n = fake.log_size(); printed < n; ++printed) printf("| %s\n", fake.log_line(printed));
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: plan_check <fake runtime> <scenario> <op> ...\n");
    return 2;
  }
  const char *path = argv[1];
  void *lib = dlopen(path, RTLD_NOW | RTLD_LOCAL);
  if (!lib) {
    fprintf(stderr, "plan_check: %s\n", dlerror());
    return 2;
  }
  bind(lib, "fake_fail", fake.fail);
  bind(lib, "fake_log_size", fake.log_size);
  bind(lib, "fake_log_line", fake.log_line);
  bind(lib, "fake_live", fake.live);
  bind(lib, "fake_errors", fake.errors);
  bind(lib, "fake_caller_stream", fake.caller_stream);
  printf("scenario %s\n", argv[2]);
  void *plan = nullptr;
  char text[256];
  for (int i = 3; i < argc; ++i) {
    Args a{words(argv[i])};
    const std::string &op = a.w[0];
    printf("> %s\n", argv[i]);
    if (op == "init") {
      report(wd_init_with_runtime(0, path));
    } else if (op == "init_path") {
      report(wd_init_with_runtime(0, a.word().c_str()));
    } else if (op == "malloc") {
      void *p = nullptr;
      report(wd_malloc(a.num(), &p));
    } else if (op == "sync") {
      report(wd_sync(a.stream()));
    } else if (op == "launch_packed") {
      Launch l = launch_of(a);
      void *s = a.stream();
      auto buf = a.buffer();
      report(wd_launch_packed(l.fn, l.g[0], l.g[1], l.g[2], l.b[0], l.b[1], l.b[2], l.lds, s, buf.data(), buf.size()));
    } else if (op == "launch") {
      Launch l = launch_of(a);
      void *s = a.stream();
      std::vector<int> values(a.num() + 1);
      std::vector<void *> params;
      for (auto &v : values) params.push_back(&v);
      const int rc = wd_launch(l.fn, l.g[0], l.g[1], l.g[2], l.b[0], l.b[1], l.b[2], l.lds, s, params.data());
      snprintf(text, sizeof(text), "params=%p", static_cast<void *>(params.data()));
      report(rc, text);
    } else if (op == "plan") {
      report(wd_plan_create(&plan));
    } else if (op == "add") {
      Launch l = launch_of(a);
      auto buf = a.buffer();
      report(wd_plan_add(plan, l.fn, l.g[0], l.g[1], l.g[2], l.b[0], l.b[1], l.b[2], l.lds, buf.data(), buf.size()));
    } else if (op == "size") {
      int n = -1;
      const int rc = wd_plan_size(plan, &n);
      report(rc, "n=" + std::to_string(n));
    } else if (op == "add_cohort") {
      const int entry = a.num(), cohort = a.num();
      Launch l = launch_of(a);
      auto buf = a.buffer();
      report(wd_plan_add_cohort(plan, entry, cohort, l.fn, l.g[0], l.g[1], l.g[2], l.b[0], l.b[1], l.b[2], l.lds,
                                buf.data(), buf.size()));
    } else if (op == "cohorts") {
      int n = -1;
      const int rc = wd_plan_cohorts(plan, &n);
      report(rc, "n=" + std::to_string(n));
    } else if (op == "multi") {
      Launch l = launch_of(a);
      auto buf = a.buffer();
      const size_t offset = a.num();
      const int max_ticks = a.num();
      report(wd_plan_set_multi_tick(plan, l.fn, l.g[0], l.g[1], l.g[2], l.b[0], l.b[1], l.b[2], l.lds, buf.data(),
                                    buf.size(), offset, max_ticks));
    } else if (op == "run") {
      const int repeats = a.num();
      report(wd_plan_run(plan, repeats, a.stream()));
    } else if (op == "timing") {
      const int entry = a.num(), stride = a.num(), max_samples = a.num();
      report(wd_plan_enable_timing(plan, entry, stride, max_samples));
    } else if (op == "read") {
      float ms = -1.f;
      int n = -1;
      const int rc = wd_plan_read_timing(plan, &ms, &n);
      snprintf(text, sizeof(text), "ms=%.1f n=%d", ms, n);
      report(rc, text);
    } else if (op == "graph") {
      const int reps = a.num();
      report(wd_plan_instantiate_graph(plan, reps, a.stream()));
    } else if (op == "run_graph") {
      const int launches = a.num();
      report(wd_plan_run_graph(plan, launches, a.stream()));
    } else if (op == "destroy") {
      const int rc = wd_plan_destroy(plan);
      plan = nullptr;
      report(rc);
    } else if (op == "fail") {
      const std::string call = a.word();
      const int nth = a.num(), error = a.num();
      fake.fail(call.c_str(), nth, error);
      report(0);
    } else if (op == "live") {
      snprintf(text, sizeof(text), "stream=%d event=%d graph=%d exec=%d module=%d alloc=%d errors=%d",
               fake.live("stream"), fake.live("event"), fake.live("graph"), fake.live("exec"), fake.live("module"),
               fake.live("alloc"), fake.errors());
      report(0, text);
    } else {
      fprintf(stderr, "plan_check: unknown operation `%s`\n", argv[i]);
      return 2;
    }
  }
  printf("end stream=%d event=%d graph=%d exec=%d module=%d alloc=%d errors=%d\n", fake.live("stream"),
         fake.live("event"), fake.live("graph"), fake.live("exec"), fake.live("module"), fake.live("alloc"),
         fake.errors());
  return 0;
}
