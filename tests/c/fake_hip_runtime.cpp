// fake_hip_runtime.cpp -- a recording stand-in for libamdhip64, for tests/test_launch_plan_host.py.
//
// It defines every entry point libwdhip.so binds with dlsym (WD_HIP_FUNCS in warp_drive_amd/csrc/wd_runtime.cpp), with
// the signatures of hip_runtime_api.h, opens no device and runs nothing.  What it does instead:
//   * one line per call in an in-memory log: the call, the handles involved and the result (`rc=`);
//   * streams, events, modules, graphs, graph execs and allocations are small heap objects named <kind>#<n> in order
//     of creation; a set of the live ones is kept, and a destroy / use of one that is not live is a FAKE_ERROR line;
//   * events remember the stream and the log position of their last record; hipEventElapsedTime on one never recorded
//     fails (and is a FAKE_ERROR), otherwise the milliseconds are the creation number of the START event, so a sum of
//     elapsed times tells which pairs were read;
//   * test controls (fake_*): fail the n-th call of a name with a given hipError_t, read / clear the log, count live
//     handles by kind, hand out the caller's stream.
// A runtime that lacks one symbol (dlsym decides what a runtime "has") is this file built with the symbol renamed on
// the command line, -D<name>=fake_without_<name>: header and definition then both carry the other name.
//
// The library is loaded by tests/c/plan_check.cpp only, in a process of its own.

#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

struct Handle {
  std::string kind;
  int id = 0;
  // events
  bool recorded = false;
  std::string on_stream;
  long position = -1;
  // streams
  bool capturing = false;
};

std::vector<std::string> g_log;
// The handle a caller holds is a one-byte heap block of its own; what the fake knows about it sits here under the
// COMPLEMENT of its address, so that a handle nobody destroys is unreachable at exit and LeakSanitizer reports it.
std::map<uintptr_t, Handle> g_live;
uintptr_t key(const void *p) { return ~reinterpret_cast<uintptr_t>(p); }
std::map<std::string, int> g_created;                  // kind -> handles made so far
std::map<std::string, std::pair<int, int>> g_fail;     // call -> (calls until the failing one, its error)
int g_errors = 0;
hipError_t g_last_error = hipSuccess;
Handle g_caller{"stream", 0};

void logf(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_log.emplace_back(buf);
}

void fake_error(const std::string &what) {
  ++g_errors;
  g_log.push_back("FAKE_ERROR " + what);
}

struct Made {
  void *token;
  int id;
};
Made make(const char *kind) {
  void *token = new char(0);
  Handle &h = g_live[key(token)];
  h.kind = kind;
  h.id = ++g_created[kind];
  return {token, h.id};
}

// name of a handle for the log; `kind` is what the call expects there
std::string name(const void *p, const char *kind) {
  if (!p) return std::string(kind) + "#null";
  if (p == &g_caller && !strcmp(kind, "stream")) return "stream#caller";
  auto it = g_live.find(key(p));
  char buf[64];
  if (it == g_live.end() || it->second.kind != kind) {
    snprintf(buf, sizeof(buf), "%s#dead:%p", kind, p);
    fake_error(std::string("use of a ") + kind + " that is not live: " + buf);
    return buf;
  }
  snprintf(buf, sizeof(buf), "%s#%d", kind, it->second.id);
  return buf;
}

Handle *live(const void *p, const char *kind) {
  if (p == &g_caller && !strcmp(kind, "stream")) return &g_caller;
  auto it = g_live.find(key(p));
  return it != g_live.end() && it->second.kind == kind ? &it->second : nullptr;
}

hipError_t destroy(const void *p, const char *kind, const char *call) {
  auto it = g_live.find(key(p));
  if (it == g_live.end() || it->second.kind != kind) {
    char buf[96];
    snprintf(buf, sizeof(buf), "%s of a %s that is not live: %p", call, kind, p);
    fake_error(buf);
    logf("%s %s=%s#dead rc=%d", call, kind, kind, static_cast<int>(hipErrorInvalidHandle));
    return hipErrorInvalidHandle;
  }
  logf("%s %s=%s#%d rc=0", call, kind, kind, it->second.id);
  g_live.erase(it);
  delete static_cast<const char *>(p);
  return hipSuccess;
}

// the injected failure of this call, if it is the one asked for
hipError_t injected(const char *call) {
  auto it = g_fail.find(call);
  if (it == g_fail.end()) return hipSuccess;
  if (--it->second.first > 0) return hipSuccess;
  hipError_t e = static_cast<hipError_t>(it->second.second);
  g_fail.erase(it);
  g_last_error = e;
  return e;
}

#define FAKE_ENTER(call, ...)                                     \
  if (hipError_t fail_ = injected(call)) {                        \
    logf(__VA_ARGS__);                                            \
    g_log.back() += " rc=" + std::to_string(static_cast<int>(fail_)); \
    return fail_;                                                 \
  }

std::string hex(const void *p, size_t n) {
  static const char *digits = "0123456789abcdef";
  std::string s;
  const unsigned char *b = static_cast<const unsigned char *>(p);
  for (size_t i = 0; i < n; ++i) {
    s += digits[b[i] >> 4];
    s += digits[b[i] & 15];
  }
  return s.empty() ? "-" : s;
}

}  // namespace

extern "C" {

// ---- test controls -----------------------------------------------------------------------------------------------
void fake_fail(const char *call, int nth, int error) { g_fail[call] = {nth, error}; }
long fake_log_size(void) { return static_cast<long>(g_log.size()); }
const char *fake_log_line(long i) { return i >= 0 && i < fake_log_size() ? g_log[i].c_str() : ""; }
void fake_log_clear(void) { g_log.clear(); }
int fake_live(const char *kind) {
  int n = 0;
  for (auto &kv : g_live) n += kv.second.kind == kind;
  return n;
}
int fake_errors(void) { return g_errors; }
void *fake_caller_stream(void) { return &g_caller; }

// ---- device ---------------------------------------------------------------------------------------------------------
hipError_t hipInit(unsigned int flags) {
  FAKE_ENTER("hipInit", "hipInit flags=%u", flags)
  logf("hipInit flags=%u rc=0", flags);
  return hipSuccess;
}
hipError_t hipSetDevice(int device) {
  FAKE_ENTER("hipSetDevice", "hipSetDevice device=%d", device)
  logf("hipSetDevice device=%d rc=0", device);
  return hipSuccess;
}
hipError_t hipGetDeviceCount(int *count) {
  FAKE_ENTER("hipGetDeviceCount", "hipGetDeviceCount")
  *count = 1;
  logf("hipGetDeviceCount count=1 rc=0");
  return hipSuccess;
}
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_t *prop, int device) {
  FAKE_ENTER("hipGetDevicePropertiesR0600", "hipGetDevicePropertiesR0600 device=%d", device)
  memset(prop, 0, sizeof(*prop));
  snprintf(prop->name, sizeof(prop->name), "fake device");
  snprintf(prop->gcnArchName, sizeof(prop->gcnArchName), "gfx950:fake");
  prop->multiProcessorCount = 256;
  prop->totalGlobalMem = size_t(1) << 30;
  logf("hipGetDevicePropertiesR0600 device=%d rc=0", device);
  return hipSuccess;
}
const char *hipGetErrorString(hipError_t e) {
  static char buf[48];  // (one caller thread)
  snprintf(buf, sizeof(buf), "fake error %d", static_cast<int>(e));
  logf("hipGetErrorString error=%d", static_cast<int>(e));
  return buf;
}
hipError_t hipGetLastError(void) {
  hipError_t e = g_last_error;
  g_last_error = hipSuccess;
  logf("hipGetLastError rc=%d", static_cast<int>(e));
  return e;
}
hipError_t hipDeviceSynchronize(void) {
  FAKE_ENTER("hipDeviceSynchronize", "hipDeviceSynchronize")
  logf("hipDeviceSynchronize rc=0");
  return hipSuccess;
}

// ---- memory ---------------------------------------------------------------------------------------------------------
hipError_t hipMalloc(void **ptr, size_t bytes) {
  FAKE_ENTER("hipMalloc", "hipMalloc bytes=%zu", bytes)
  const Made h = make("alloc");
  *ptr = h.token;
  logf("hipMalloc bytes=%zu out=alloc#%d rc=0", bytes, h.id);
  return hipSuccess;
}
hipError_t hipFree(void *ptr) {
  FAKE_ENTER("hipFree", "hipFree")
  return destroy(ptr, "alloc", "hipFree");
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t stream) {
  (void)dst;
  (void)src;
  FAKE_ENTER("hipMemcpyAsync", "hipMemcpyAsync bytes=%zu kind=%d", bytes, static_cast<int>(kind))
  logf("hipMemcpyAsync bytes=%zu kind=%d stream=%s rc=0", bytes, static_cast<int>(kind), name(stream, "stream").c_str());
  return hipSuccess;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t stream) {
  (void)dst;
  FAKE_ENTER("hipMemsetAsync", "hipMemsetAsync value=%d bytes=%zu", value, bytes)
  logf("hipMemsetAsync value=%d bytes=%zu stream=%s rc=0", value, bytes, name(stream, "stream").c_str());
  return hipSuccess;
}

// ---- code objects ---------------------------------------------------------------------------------------------------
hipError_t hipModuleLoad(hipModule_t *module, const char *path) {
  FAKE_ENTER("hipModuleLoad", "hipModuleLoad path=%s", path)
  const Made h = make("module");
  *module = reinterpret_cast<hipModule_t>(h.token);
  logf("hipModuleLoad path=%s out=module#%d rc=0", path, h.id);
  return hipSuccess;
}
hipError_t hipModuleLoadData(hipModule_t *module, const void *image) {
  (void)image;
  FAKE_ENTER("hipModuleLoadData", "hipModuleLoadData")
  const Made h = make("module");
  *module = reinterpret_cast<hipModule_t>(h.token);
  logf("hipModuleLoadData out=module#%d rc=0", h.id);
  return hipSuccess;
}
hipError_t hipModuleUnload(hipModule_t module) {
  FAKE_ENTER("hipModuleUnload", "hipModuleUnload")
  return destroy(module, "module", "hipModuleUnload");
}
// functions and globals belong to their module: plain numbers, nothing to free
hipError_t hipModuleGetFunction(hipFunction_t *function, hipModule_t module, const char *kname) {
  FAKE_ENTER("hipModuleGetFunction", "hipModuleGetFunction name=%s", kname)
  const int id = ++g_created["function"];
  *function = reinterpret_cast<hipFunction_t>(static_cast<uintptr_t>(0xf000 + id));
  logf("hipModuleGetFunction module=%s name=%s out=0x%x rc=0", name(module, "module").c_str(), kname, 0xf000 + id);
  return hipSuccess;
}
hipError_t hipModuleGetGlobal(hipDeviceptr_t *dptr, size_t *bytes, hipModule_t module, const char *gname) {
  FAKE_ENTER("hipModuleGetGlobal", "hipModuleGetGlobal name=%s", gname)
  *dptr = reinterpret_cast<hipDeviceptr_t>(static_cast<uintptr_t>(0xd000));
  *bytes = 64;
  logf("hipModuleGetGlobal module=%s name=%s rc=0", name(module, "module").c_str(), gname);
  return hipSuccess;
}
hipError_t hipFuncGetAttribute(int *value, hipFunction_attribute attrib, hipFunction_t function) {
  FAKE_ENTER("hipFuncGetAttribute", "hipFuncGetAttribute attribute=%d", static_cast<int>(attrib))
  *value = 100 + static_cast<int>(attrib);
  logf("hipFuncGetAttribute attribute=%d fn=%p rc=0", static_cast<int>(attrib), static_cast<void *>(function));
  return hipSuccess;
}

// ---- launch ---------------------------------------------------------------------------------------------------------
hipError_t hipModuleLaunchKernel(hipFunction_t f, unsigned int gx, unsigned int gy, unsigned int gz, unsigned int bx,
                                 unsigned int by, unsigned int bz, unsigned int lds, hipStream_t stream, void **params,
                                 void **extra) {
  std::string size = "-", bytes = "-";
  if (extra) {  // {HIP_LAUNCH_PARAM_BUFFER_POINTER, buffer, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END}
    const void *buffer = nullptr;
    const size_t *n = nullptr;
    for (int i = 0; extra[i] != HIP_LAUNCH_PARAM_END; i += 2) {
      if (extra[i] == HIP_LAUNCH_PARAM_BUFFER_POINTER) buffer = extra[i + 1];
      if (extra[i] == HIP_LAUNCH_PARAM_BUFFER_SIZE) n = static_cast<const size_t *>(extra[i + 1]);
    }
    if (!n || (*n && !buffer)) {
      fake_error("hipModuleLaunchKernel: `extra` without a buffer and its size");
    } else {
      size = std::to_string(*n);
      bytes = hex(buffer, *n);
    }
  }
  const std::string st = name(stream, "stream");
  Handle *s = live(stream, "stream");
  char head[256];
  snprintf(head, sizeof(head), "hipModuleLaunchKernel fn=%p grid=%u,%u,%u block=%u,%u,%u lds=%u stream=%s captured=%d params=%p",
           static_cast<void *>(f), gx, gy, gz, bx, by, bz, lds, st.c_str(), s && s->capturing ? 1 : 0,
           static_cast<void *>(params));
  std::string line = std::string(head) + " extra_size=" + size + " extra=" + bytes;
  if (hipError_t e = injected("hipModuleLaunchKernel")) {
    g_log.push_back(line + " rc=" + std::to_string(static_cast<int>(e)));
    return e;
  }
  g_log.push_back(line + " rc=0");
  return hipSuccess;
}

// ---- streams and events ---------------------------------------------------------------------------------------------
hipError_t hipStreamSynchronize(hipStream_t stream) {
  FAKE_ENTER("hipStreamSynchronize", "hipStreamSynchronize")
  logf("hipStreamSynchronize stream=%s rc=0", name(stream, "stream").c_str());
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *stream, unsigned int flags) {
  FAKE_ENTER("hipStreamCreateWithFlags", "hipStreamCreateWithFlags flags=%u", flags)
  const Made h = make("stream");
  *stream = reinterpret_cast<hipStream_t>(h.token);
  logf("hipStreamCreateWithFlags flags=%u out=stream#%d rc=0", flags, h.id);
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t stream) {
  FAKE_ENTER("hipStreamDestroy", "hipStreamDestroy")
  return destroy(stream, "stream", "hipStreamDestroy");
}
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned int flags) {
  FAKE_ENTER("hipStreamWaitEvent", "hipStreamWaitEvent stream=%s event=%s flags=%u", name(stream, "stream").c_str(),
             name(event, "event").c_str(), flags)
  Handle *e = live(event, "event");
  if (e && !e->recorded) fake_error("hipStreamWaitEvent on an event that was never recorded");
  logf("hipStreamWaitEvent stream=%s event=%s flags=%u rc=0", name(stream, "stream").c_str(),
       name(event, "event").c_str(), flags);
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *event, unsigned int flags) {
  FAKE_ENTER("hipEventCreateWithFlags", "hipEventCreateWithFlags flags=%u", flags)
  const Made h = make("event");
  *event = reinterpret_cast<hipEvent_t>(h.token);
  logf("hipEventCreateWithFlags flags=%u out=event#%d rc=0", flags, h.id);
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *event) {
  FAKE_ENTER("hipEventCreate", "hipEventCreate")
  const Made h = make("event");
  *event = reinterpret_cast<hipEvent_t>(h.token);
  logf("hipEventCreate out=event#%d rc=0", h.id);
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
  FAKE_ENTER("hipEventRecord", "hipEventRecord event=%s stream=%s", name(event, "event").c_str(),
             name(stream, "stream").c_str())
  const std::string st = name(stream, "stream");
  if (Handle *e = live(event, "event")) {
    e->recorded = true;
    e->on_stream = st;
    e->position = fake_log_size();
  }
  logf("hipEventRecord event=%s stream=%s rc=0", name(event, "event").c_str(), st.c_str());
  return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t event) {
  FAKE_ENTER("hipEventSynchronize", "hipEventSynchronize event=%s", name(event, "event").c_str())
  Handle *e = live(event, "event");
  if (e && !e->recorded) fake_error("hipEventSynchronize on an event that was never recorded");
  logf("hipEventSynchronize event=%s rc=0", name(event, "event").c_str());
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t start, hipEvent_t stop) {
  FAKE_ENTER("hipEventElapsedTime", "hipEventElapsedTime start=%s stop=%s", name(start, "event").c_str(),
             name(stop, "event").c_str())
  Handle *a = live(start, "event"), *b = live(stop, "event");
  if (!a || !b || !a->recorded || !b->recorded) {
    fake_error("hipEventElapsedTime on an event that was never recorded");
    logf("hipEventElapsedTime start=%s stop=%s rc=%d", name(start, "event").c_str(), name(stop, "event").c_str(),
         static_cast<int>(hipErrorInvalidHandle));
    g_last_error = hipErrorInvalidHandle;
    return hipErrorInvalidHandle;
  }
  *ms = static_cast<float>(a->id);
  logf("hipEventElapsedTime start=%s stop=%s start_stream=%s stop_stream=%s start_at=%ld stop_at=%ld ms=%d rc=0",
       name(start, "event").c_str(), name(stop, "event").c_str(), a->on_stream.c_str(), b->on_stream.c_str(),
       a->position, b->position, a->id);
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) {
  FAKE_ENTER("hipEventDestroy", "hipEventDestroy")
  return destroy(event, "event", "hipEventDestroy");
}

// ---- graphs ---------------------------------------------------------------------------------------------------------
hipError_t hipStreamBeginCapture(hipStream_t stream, hipStreamCaptureMode mode) {
  FAKE_ENTER("hipStreamBeginCapture", "hipStreamBeginCapture stream=%s mode=%d", name(stream, "stream").c_str(),
             static_cast<int>(mode))
  if (Handle *s = live(stream, "stream")) s->capturing = true;
  logf("hipStreamBeginCapture stream=%s mode=%d rc=0", name(stream, "stream").c_str(), static_cast<int>(mode));
  return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t stream, hipGraph_t *graph) {
  if (Handle *s = live(stream, "stream")) s->capturing = false;  // a failing call ends the capture too
  FAKE_ENTER("hipStreamEndCapture", "hipStreamEndCapture stream=%s", name(stream, "stream").c_str())
  const Made h = make("graph");
  *graph = reinterpret_cast<hipGraph_t>(h.token);
  logf("hipStreamEndCapture stream=%s out=graph#%d rc=0", name(stream, "stream").c_str(), h.id);
  return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t *exec, hipGraph_t graph, hipGraphNode_t *error_node, char *log_buffer,
                               size_t buffer_size) {
  (void)error_node;
  (void)log_buffer;
  (void)buffer_size;
  FAKE_ENTER("hipGraphInstantiate", "hipGraphInstantiate graph=%s", name(graph, "graph").c_str())
  const std::string g = name(graph, "graph");
  const Made h = make("exec");
  *exec = reinterpret_cast<hipGraphExec_t>(h.token);
  logf("hipGraphInstantiate graph=%s out=exec#%d rc=0", g.c_str(), h.id);
  return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t exec, hipStream_t stream) {
  FAKE_ENTER("hipGraphLaunch", "hipGraphLaunch exec=%s stream=%s", name(exec, "exec").c_str(),
             name(stream, "stream").c_str())
  logf("hipGraphLaunch exec=%s stream=%s rc=0", name(exec, "exec").c_str(), name(stream, "stream").c_str());
  return hipSuccess;
}
hipError_t hipGraphExecDestroy(hipGraphExec_t exec) {
  FAKE_ENTER("hipGraphExecDestroy", "hipGraphExecDestroy")
  return destroy(exec, "exec", "hipGraphExecDestroy");
}
hipError_t hipGraphDestroy(hipGraph_t graph) {
  FAKE_ENTER("hipGraphDestroy", "hipGraphDestroy")
  return destroy(graph, "graph", "hipGraphDestroy");
}

}  // extern "C"
