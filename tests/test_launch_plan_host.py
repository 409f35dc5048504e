"""The launch plans of warp_drive_amd/csrc/wd_runtime.cpp (libwdhip.so) against a recording fake of the HIP runtime.

tests/c/fake_hip_runtime.cpp defines every entry point the library binds with dlsym, opens no device and logs each call;
tests/c/plan_check.cpp is compiled together with wd_runtime.cpp itself and drives the C ABI of include/wd_hip.h through a
scenario (a list of operations given on its command line), printing every return code and what the fake logged.  The
scenarios and everything expected of them are in this file.  Both programs are built twice: plain -O2, and with
AddressSanitizer (leak detection on) + UndefinedBehaviorSanitizer; the sanitized build runs where no GPU is visible.
The fake is loaded by plan_check only, in a process of its own.

What is pinned: which stream every launch goes to and with which bytes, the fork / join events of the replica cohorts,
the tick counts the multi-tick form writes into its argument buffer, capture / instantiate / replay of the graph route,
the event brackets of the sampler bench.py reads (against a model of its counters, SamplerModel below), the error
paths of all of them, and that no stream, event, graph or graph exec outlives wd_plan_destroy."""
import os
import random
import re
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_RUNTIME, BAD_ARG = 100001, 100002  # include/wd_hip.h
LAUNCH_FAILURE, OUT_OF_MEMORY, INVALID_VALUE = 719, 2, 1  # hipError_t values the scenarios inject
HIDDEN = "hipStreamWaitEvent"  # the symbol the second fake lacks
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

ENTRY_FN, MULTI_FN = 0x100, 0x200  # the numbers that stand for kernels: entry i, the multi-tick form, ...


def cohort_fn(cohort, entry):
    return 0x1000 + 0x10 * cohort + entry


# ---- building and running plan_check --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    from warp_drive_amd import build as wd_build

    out = tmp_path_factory.mktemp("plan_check")
    common = ["-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-I{wd_build.ROCM}/include", f"-I{ROOT}/include"]
    fake = os.path.join(ROOT, "tests", "c", "fake_hip_runtime.cpp")
    srcs = [os.path.join(ROOT, "tests", "c", "plan_check.cpp"), os.path.join(wd_build.CSRC, "wd_runtime.cpp")]
    built = {}
    for tag, flags in (("plain", ["-O2"]), ("sanitized", SANITIZE)):
        paths = {k: str(out / f"{k}_{tag}") for k in ("plan_check", "libfake.so", "libfake_without.so")}
        subprocess.run(["g++", *flags, *common, "-Wall", "-Werror", "-fPIC", "-shared", fake, "-o", paths["libfake.so"]],
                       check=True)
        subprocess.run(["g++", *flags, *common, "-fPIC", "-shared", f"-D{HIDDEN}=fake_without_{HIDDEN}", fake, "-o",
                        paths["libfake_without.so"]], check=True)
        subprocess.run(["g++", *flags, *common, "-Wall", "-Wno-unused-result", "-Wno-format-truncation", *srcs, "-o",
                        paths["plan_check"], "-ldl"], check=True)
        built[tag] = paths
    return built


class Line:
    """one line of the fake's log: `call key=value ...`; `at` is its position in the log of the process"""

    def __init__(self, raw, at):
        self.raw, self.at = raw, at
        self.call, _, rest = raw.partition(" ")
        self.f = dict(w.split("=", 1) for w in rest.split() if "=" in w) if self.call != "FAKE_ERROR" else {}

    def __getitem__(self, key):
        return self.f[key]

    @property
    def rc(self):
        return int(self.f.get("rc", 0))

    @property
    def bytes(self):
        return b"" if self["extra"] == "-" else bytes.fromhex(self["extra"])

    def __repr__(self):
        return self.raw


class Op:
    def __init__(self, text):
        self.text, self.rc, self.err, self.out, self.log = text, None, "", {}, []

    def calls(self, *names):
        return [l for l in self.log if l.call in names]

    @property
    def launches(self):
        return self.calls("hipModuleLaunchKernel")

    def __repr__(self):
        return f"<{self.text}: rc={self.rc} {self.err} {self.out} {self.log}>"


class Result(list):
    """the operations of one plan_check run, in order; `end` is the fake's live-handle count when the program ended"""

    def op(self, prefix, nth=0):
        return [o for o in self if o.text.startswith(prefix)][nth]

    @property
    def lines(self):
        return [l for o in self for l in o.log]


def parse(stdout):
    res, at = Result(), 0
    for raw in stdout.splitlines():
        if raw.startswith("> "):
            res.append(Op(raw[2:]))
        elif raw.startswith("| "):
            res[-1].log.append(Line(raw[2:], at))
            at += 1
        elif raw.startswith("rc="):
            m = re.match(r"rc=(-?\d+) err=(.*)", raw)
            res[-1].rc = int(m.group(1))
            if res[-1].rc:
                res[-1].err = m.group(2)
            else:
                res[-1].out = dict(w.split("=", 1) for w in m.group(2).split())
        elif raw.startswith("end "):
            res.end = {k: int(v) for k, v in (w.split("=") for w in raw[4:].split())}
    return res


@pytest.fixture(params=["plain", "sanitized"])
def check(request, programs):
    """-> check(scenario, ops, fake="libfake.so"): runs plan_check, and asserts what holds after EVERY scenario: exit 0,
    nothing on stderr (a sanitizer report is there), nothing live in the fake, nothing destroyed twice or used dead"""
    if request.param == "sanitized":
        import torch

        if torch.cuda.is_available():
            pytest.skip("a GPU is visible")  # sanitizers are for CPU runs
    paths = programs[request.param]

    def run(scenario, ops, fake="libfake.so", expect_clean=True):
        ops = [o if isinstance(o, str) else ",".join(str(w) for w in o) for o in ops]
        env = dict(os.environ)
        if request.param == "sanitized":
            env["ASAN_OPTIONS"] = "detect_leaks=1"
        p = subprocess.run([paths["plan_check"], paths[fake], scenario, *ops], capture_output=True, text=True, env=env)
        dump = os.environ.get("WD_PLAN_CHECK_LOGS")  # keep every scenario's output (docs/rounds/r20.md compares them)
        if dump:
            with open(os.path.join(dump, f"{request.param}__{scenario}.txt"), "w") as f:
                f.write(p.stdout + p.stderr)
        res = parse(p.stdout)
        res.returncode, res.stderr = p.returncode, p.stderr
        if expect_clean:
            assert p.returncode == 0 and p.stderr == "", f"{scenario}: exit {p.returncode}\n{p.stderr[-3000:]}"
            assert res.end == dict.fromkeys(res.end, 0), f"{scenario}: {res.end}"
            assert not [l for l in res.lines if l.call == "FAKE_ERROR"]
        return res

    run.paths = paths
    return run


def launch(fn, grid=(1, 1, 1), block=(64, 1, 1), lds=0):
    return [hex(fn), *grid, *block, lds]


def buffer(n, seed):
    """the bytes plan_check makes of `n,seed`"""
    return bytes((seed + 7 * i) & 255 for i in range(n))


def brief(line):
    if line.call == "hipModuleLaunchKernel":
        return ("launch", int(line["fn"], 16), line["stream"])
    if line.call == "hipEventRecord":
        return ("record", line["event"], line["stream"])
    if line.call == "hipStreamWaitEvent":
        return ("wait", line["stream"], line["event"])
    if line.call in ("hipEventCreateWithFlags", "hipStreamCreateWithFlags", "hipEventCreate"):
        return (line.call, int(line.f.get("flags", 0)), line["out"])
    return (line.call,)


EVENT_CALLS = ("hipEventCreate", "hipEventCreateWithFlags", "hipEventRecord", "hipEventSynchronize", "hipEventElapsedTime",
               "hipEventDestroy", "hipStreamWaitEvent", "hipStreamCreateWithFlags")


# ---- binding ------------------------------------------------------------------------------------------------------------
def test_runtime_that_lacks_a_symbol(check):
    res = check("lacks_symbol", ["init", "plan", ["add", *launch(ENTRY_FN), 4, 1], "run,1,caller", "malloc,16", "destroy"],
                fake="libfake_without.so")
    init = res.op("init")
    assert init.rc == NO_RUNTIME and HIDDEN in init.err
    assert res.op("run").rc == NO_RUNTIME and res.op("malloc").rc == NO_RUNTIME
    assert res.lines == []  # not one call reached the half-bound runtime


def test_calls_before_init_fail(check):
    ops = ["malloc,16", ["launch_packed", *launch(ENTRY_FN), "caller", 4, 1], "sync,caller", "plan",
           ["add", *launch(ENTRY_FN), 4, 1], "size", "run,1,caller", "run,3,caller", "timing,0,1,4", "read", "graph,2,caller",
           "run_graph,1,caller", "destroy"]
    res = check("before_init", ops)
    for o in res:
        want = 0 if o.text.split(",")[0] in ("plan", "add", "size", "destroy") else NO_RUNTIME
        assert o.rc == want, o
        assert o.rc == 0 or "wd_init" in o.err
    assert res.op("size").out == {"n": "1"} and res.lines == []


def test_second_init_rebinds_nothing(check):
    ops = ["init", "init_path,/nonexistent/libamdhip64.so", f"init_path,{check.paths['libfake_without.so']}",
           ["launch_packed", *launch(ENTRY_FN), "caller", 4, 1]]
    res = check("second_init", ops)
    for o in res[:3]:  # every init is hipInit + hipSetDevice on the runtime bound first
        assert o.rc == 0 and [l.call for l in o.log] == ["hipInit", "hipSetDevice"], o
    assert len(res[3].launches) == 1  # ... and the launch still lands in its log


# ---- plain launches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream", ["caller", "null"])
def test_launches_arrive_unchanged(check, stream):
    geo = dict(grid=(7, 2, 3), block=(128, 2, 1), lds=4096)
    sizes = (0, 4, 12, 260)
    ops = ["init"] + [["launch_packed", *launch(0xabc0 + n, **geo), stream, n, 3 + n] for n in sizes]
    ops += [["launch", *launch(0xdef0, **geo), stream, 3]]
    res = check(f"launch_{stream}", ops)
    for o, n in zip(res[1:], sizes):
        (l,) = o.log
        assert o.rc == 0 and l.call == "hipModuleLaunchKernel" and int(l["fn"], 16) == 0xabc0 + n
        assert (l["grid"], l["block"], l["lds"], l["stream"]) == ("7,2,3", "128,2,1", "4096", f"stream#{stream}")
        assert l["params"] == "(nil)" and int(l["extra_size"]) == n and l.bytes == buffer(n, 3 + n)
    (l,) = res[-1].log  # wd_launch: the caller's array of argument pointers, no packed buffer
    assert (l["grid"], l["block"], l["lds"], l["stream"]) == ("7,2,3", "128,2,1", "4096", f"stream#{stream}")
    assert l["params"] == res[-1].out["params"] != "(nil)" and l["extra_size"] == "-"


# ---- a plan on one stream -------------------------------------------------------------------------------------------------
THREE = [(ENTRY_FN, dict(grid=(8, 1, 1), block=(256, 1, 1), lds=0), 24, 11),
         (ENTRY_FN + 1, dict(grid=(2000, 1, 1), block=(128, 1, 1), lds=33792), 260, 5),
         (ENTRY_FN + 2, dict(grid=(3, 4, 1), block=(64, 2, 2), lds=16), 0, 0)]


def three_entry_plan():
    return ["init", "plan"] + [["add", *launch(fn, **geo), n, seed] for fn, geo, n, seed in THREE]


def assert_is_entries(lines, reps, stream, entries=THREE):
    assert len(lines) == reps * len(entries)
    for k, l in enumerate(lines):
        fn, geo, n, seed = entries[k % len(entries)]
        assert l.call == "hipModuleLaunchKernel" and l.rc == 0 and int(l["fn"], 16) == fn and l["stream"] == stream
        assert l["grid"] == ",".join(map(str, geo["grid"])) and l["block"] == ",".join(map(str, geo["block"]))
        assert int(l["lds"]) == geo["lds"] and l.bytes == buffer(n, seed) and l["params"] == "(nil)"


def test_plan_replays_its_entries_in_order(check):
    res = check("plan_one_stream", three_entry_plan() + ["size", "cohorts", "run,1,caller", "run,4,caller", "run,2,null",
                                                         "run,0,caller", "destroy"])
    assert res.op("size").out == {"n": "3"} and res.op("cohorts").out == {"n": "1"}
    for o, reps, stream in zip(res[-5:-1], (1, 4, 2, 0), ("caller", "caller", "null", "caller")):
        assert o.rc == 0
        assert_is_entries(o.log, reps, f"stream#{stream}")  # launches only: no event call with timing off
    assert res.op("destroy").log == []


# ---- the sampler: a model of its counters -----------------------------------------------------------------------------------
class SamplerModel:
    """What wd_plan_enable_timing / wd_plan_run / wd_plan_read_timing do with their counters, as plain Python.

    `trace` is what the caller's stream sees: ("start", i) / ("end", i) for the records of event pair i, and
    ("launch", fn, ticks) (ticks: the count the multi-tick form carries, else None).  A plan of ONE entry is bracketed
    over group = min(stride, 8) repetitions; a multi-entry plan around the timed entry of every stride-th repetition;
    a cohort or multi-tick run as a whole, counted as `repeats` launches.  A bracket stays open across run() calls.
    The two `mutate` values are planted defects (test_model_has_teeth)."""

    def __init__(self, entries=1, cohorts=1, max_ticks=0, mutate=None):
        self.entries, self.cohorts, self.max_ticks, self.mutate = entries, cohorts, max_ticks, mutate
        self.trace = []
        self.enable(-1, 1, 1)

    def enable(self, entry, stride, max_samples):
        self.used = self.run_counter = self.pending = 0
        self.open, self.launches, self.group, self.timed_entry = False, [], 1, -1
        if entry < 0:
            return
        self.timed_entry, self.stride, self.max_samples = entry, stride, max_samples
        if self.entries == 1:
            self.group = stride if self.mutate == "group_is_stride" else min(stride, 8)

    def _sampling(self):
        return self.timed_entry >= 0 and (self.open or self.used < self.max_samples)

    def _close(self):
        self.trace.append(("end", self.used))
        self.launches.append(self.pending)
        self.pending, self.open = 0, False
        self.used += 1

    def run(self, repeats):
        if repeats >= 2 and (self.max_ticks or self.cohorts >= 2):
            timed = self._sampling()
            if timed and not self.open:
                self.trace.append(("start", self.used))
                self.open = True
            if self.max_ticks:
                left = repeats
                while left > 0:
                    n = min(left, self.max_ticks)
                    self.trace.append(("launch", MULTI_FN, n))
                    left -= n
            else:  # of the cohorts, the caller's stream sees cohort 0
                self.trace += [("launch", cohort_fn(0, i), None) for _ in range(repeats) for i in range(self.entries)]
            self.run_counter += repeats
            if timed:
                self.pending += 1 if (self.mutate == "cohort_run_counts_one" and not self.max_ticks) else repeats
                self._close()
            return
        for _ in range(repeats):
            phase = self.run_counter % self.stride if self.timed_entry >= 0 else 0
            sampling = self._sampling()
            for i in range(self.entries):
                timed = sampling and i == self.timed_entry
                if timed and phase == 0 and not self.open:
                    self.trace.append(("start", self.used))
                    self.open = True
                self.trace.append(("launch", ENTRY_FN + i, None))
                if timed and self.open:
                    self.pending += 1
                    if phase == self.group - 1:
                        self._close()
            self.run_counter += 1

    def read(self):
        """-> (launches covered, the event pairs summed); starts over"""
        out = (sum(self.launches), list(range(self.used)))
        self.used, self.open, self.pending, self.launches = 0, False, 0, []
        return out


def timed_plan(kind, entries=1, max_ticks=16):
    """operations that build a plan of `entries` launches: plain, with two complete cohorts, or with the multi-tick form"""
    ops = ["plan"] + [["add", *launch(ENTRY_FN + i), 8, i] for i in range(entries)]
    if kind == "cohorts":
        ops += [["add_cohort", i, c, *launch(cohort_fn(c, i)), 8, 16 * c + i] for c in range(2) for i in range(entries)]
    if kind == "multi":
        ops += [["multi", *launch(MULTI_FN), 12, 0, 8, max_ticks]]
    return ops


def model_for(kind, entries=1, max_ticks=16, mutate=None):
    return SamplerModel(entries, cohorts=2 if kind == "cohorts" else 1, max_ticks=max_ticks if kind == "multi" else 0,
                        mutate=mutate)


def sampler_ops(steps):
    """steps: ("timing", entry, stride, max) / ("run", k) / ("read",) -> plan_check operations"""
    return [["run", s[1], "caller"] if s[0] == "run" else list(s) for s in steps]


def disagreements(ops_of_plan, steps, model, ticks_offset=8):
    """Replay `steps` on `model` and compare with the log of the same steps (`ops_of_plan`: their operations, in order).
    Also checks, from the log alone, what must hold of every bracket read.  -> list of differences (empty: agreement)"""
    diffs, ev, trace, launches_at = [], [], [], {}
    for o, s in zip(ops_of_plan, steps):
        assert o.rc == 0, o
        if s[0] == "timing":
            ev = [l["out"] for l in o.calls("hipEventCreate")]
            assert len(ev) == (2 * s[3] if s[1] >= 0 else 0)
            model.enable(*s[1:])
        elif s[0] == "run":
            for l in o.log:
                if l.call == "hipEventRecord" and l["event"] in ev:
                    assert l["stream"] == "stream#caller"
                    k = ev.index(l["event"])
                    trace.append(("end" if k % 2 else "start", k // 2))
                elif l.call == "hipModuleLaunchKernel" and l["stream"] == "stream#caller":
                    fn = int(l["fn"], 16)
                    ticks = struct.unpack_from("<i", l.bytes, ticks_offset)[0] if fn == MULTI_FN else None
                    trace.append(("launch", fn, ticks))
                    launches_at[l.at] = 1 if ticks is None else ticks
            model.run(s[1])
        else:
            n, pairs = model.read()
            reads = o.calls("hipEventElapsedTime")
            got = [(l["start"], l["stop"]) for l in reads]
            if got != [(ev[2 * i], ev[2 * i + 1]) for i in pairs]:
                diffs.append(f"{o.text}: pairs read {got}, model {pairs}")
            if int(o.out["n"]) != n:
                diffs.append(f"{o.text}: {o.out['n']} launches covered, model {n}")
            want_ms = sum(int(ev[2 * i].split("#")[1]) for i in pairs)
            if float(o.out["ms"]) != want_ms:
                diffs.append(f"{o.text}: total {o.out['ms']}, model {want_ms}")
            # from the log alone: every pair read was recorded start-before-end on the caller's stream, and the launches
            # (ticks) issued on that stream between the two records are what read_timing says the total covers
            covered = 0
            for l in reads:
                assert l.rc == 0 and l["start_stream"] == l["stop_stream"] == "stream#caller", l
                a, b = int(l["start_at"]), int(l["stop_at"])
                inside = [n_ for at, n_ in launches_at.items() if a < at < b]
                assert a < b and inside, l
                covered += sum(inside)
            assert covered == int(o.out["n"]), (o, covered)
            assert [l["event"] for l in o.calls("hipEventSynchronize")] == [l["stop"] for l in reads]
    if trace != model.trace:
        k = next((i for i, (a, b) in enumerate(zip(trace, model.trace)) if a != b), min(len(trace), len(model.trace)))
        diffs.append(f"caller's stream differs at item {k}: log {trace[k:k + 3]}, model {model.trace[k:k + 3]}")
    return diffs


def run_sampler_case(check, name, kind, steps, entries=1, max_ticks=16, mutate=None):
    ops = ["init"] + timed_plan(kind, entries, max_ticks)
    first = len(ops)
    res = check(name, ops + sampler_ops(steps) + ["destroy"])
    return res, disagreements(res[first:first + len(steps)], steps, model_for(kind, entries, max_ticks, mutate))


# sequences of run(k) that mix single ticks with multi-tick runs; tests/test_gpu_launch_plan.py replays them on the device
MIXED_SEQUENCES = {"mixed_a": (1, 7, 2, 1, 5, 16, 3), "mixed_b": (3, 1, 1, 8, 1, 9, 2, 1, 1, 1, 1, 1, 1, 1, 4),
                   "mixed_c": (1, 1, 1, 1, 1, 12, 1, 1, 4, 1, 1, 1, 1, 1, 1, 1, 1, 2)}
KINDS = ("single", "cohorts", "multi")


def mixed_runs(name, total=48):
    """a mixed sequence, with one more run that brings it to `total` ticks"""
    seq = MIXED_SEQUENCES[name]
    return seq + (total - sum(seq),)


def test_timing_of_a_multi_entry_plan_with_the_benchmark_arguments(check):
    """bench.py's time_episode on the unfused tick: enable_timing(step_entry, 8, launches // 8), run(launches), read,
    enable_timing(-1, 1, 1) -- on a three-entry plan whose second entry is the step"""
    launches = 44
    steps = [("timing", 1, 8, launches // 8), ("run", launches), ("read",), ("run", 7), ("run", 13), ("read",),
             ("timing", -1, 1, 1), ("run", 9), ("read",)]
    ops = three_entry_plan()
    first = len(ops)
    res = check("timing_three_entries", ops + sampler_ops(steps) + ["live", "destroy"])
    got = res[first:first + len(steps)]
    # every 8th repetition: record, the step launch, record -- distinct events, on the launch stream, 5 = max_samples
    # brackets although repetition 40 is a sixth multiple of 8
    run = [brief(l) for l in got[1].log]
    ev = [l["out"] for l in got[0].calls("hipEventCreate")]
    assert len(ev) == 10 and len(set(ev)) == 10
    want = []
    for rep in range(launches):
        for i in range(3):
            bracket = i == 1 and rep % 8 == 0 and rep // 8 < 5
            want += [("record", ev[2 * (rep // 8)], "stream#caller")] if bracket else []
            want += [("launch", ENTRY_FN + i, "stream#caller")]
            want += [("record", ev[2 * (rep // 8) + 1], "stream#caller")] if bracket else []
    assert run == want
    assert got[2].out == {"ms": f"{sum(int(e.split('#')[1]) for e in ev[0::2]):.1f}", "n": "5"}
    # the counter of repetitions goes on (44 .. 63: multiples of 8 at 48 and 56), the pairs start over
    assert [b for o in got[3:5] for b in map(brief, o.log) if b[0] == "record"] == \
        [("record", e, "stream#caller") for e in ev[:4]]
    assert got[5].out == {"ms": f"{sum(int(e.split('#')[1]) for e in ev[0:4:2]):.1f}", "n": "2"}
    # disabled: every event destroyed, runs are launches only, nothing to read
    assert [l["event"] for l in got[6].calls("hipEventDestroy")] == ev
    assert not got[7].calls(*EVENT_CALLS) and got[8].out == {"ms": "0.0", "n": "0"} and not got[8].log
    assert res.op("live").out["event"] == "0"
    # ... and the model says the same of the whole sequence
    assert disagreements(got, steps, SamplerModel(entries=3)) == []


@pytest.mark.parametrize("stride", [1, 3, 8, 16])
def test_timing_of_a_one_entry_plan(check, stride):
    """48 ticks as run(1) only, run(6) only (a plain plan: six repetitions on one stream) and mixed with cohort and
    multi-tick runs.  run(1) / run(k) only: every window of `stride` ticks has one bracket over its first
    min(stride, 8) launches, so a read covers 48 launches at strides 1, 3, 8 and 24 at stride 16."""
    closed_form = {1: 48, 3: 48, 8: 48, 16: 24}[stride]
    for tag, kind, runs in [("ones", "single", (1,) * 48), ("sixes", "single", (6,) * 8), ("one_run", "single", (48,)),
                            ("ones_cohort_plan", "cohorts", (1,) * 48), ("ones_multi_plan", "multi", (1,) * 48)] + \
            [(f"{name}_{kind}", kind, mixed_runs(name)) for name in MIXED_SEQUENCES for kind in KINDS]:
        assert sum(runs) == 48
        steps = [("timing", 0, stride, 64)] + [("run", k) for k in runs] + [("read",), ("run", 5), ("read",)]
        res, diffs = run_sampler_case(check, f"timing_s{stride}_{tag}", kind, steps)
        assert diffs == [], (tag, diffs)
        read = res.op("read")
        if all(k == 1 for k in runs) or kind == "single":
            assert int(read.out["n"]) == closed_form and len(read.calls("hipEventElapsedTime")) == closed_form // min(stride, 8)
        if tag.startswith("ones_"):  # run(1) on a plan with cohorts / the multi-tick form: the one-tick entry, no fork
            assert {brief(l) for l in res.op("run").log if l.call == "hipModuleLaunchKernel"} == {("launch", ENTRY_FN, "stream#caller")}
            assert not [l for o in res[:-4] for l in o.calls("hipStreamCreateWithFlags", "hipStreamWaitEvent")]


def test_max_samples_and_brackets_that_span_runs(check):
    """at most max_samples pairs; a bracket opened by one run(1) is closed by a later one, or by a cohort run that
    arrives in the middle of it, and is then counted with everything in between"""
    steps = [("timing", 0, 8, 2), ("run", 1), ("run", 1), ("run", 3), ("run", 1), ("run", 1), ("run", 1), ("run", 1),
             ("run", 9), ("run", 8), ("read",), ("run", 3), ("read",)]
    res, diffs = run_sampler_case(check, "span_runs", "cohorts", steps)
    assert diffs == []
    # bracket 0: ticks 0 and 1 and the cohort run of 3 that closes it: 5 launches; bracket 1 opens at tick 8 (the fourth
    # run(1) after it) and is closed by the cohort run of 9: 10; max_samples = 2 is used up, run(8) is not sampled
    assert res.op("read").out == {"ms": "4.0", "n": "15"}
    assert res.op("read", 1).out["n"] == "3"


def random_steps(seed):
    rng = random.Random(seed)
    kind, stride = rng.choice(KINDS), rng.choice((1, 3, 8, 16))
    max_ticks = rng.choice((1, 4, 16))
    steps = [("timing", 0, stride, rng.choice((1, 2, 3, 50)))]
    for _ in range(rng.randint(4, 16)):
        u = rng.random()
        if u < 0.12:
            steps.append(("read",))
        elif u < 0.16:
            steps.append(("timing", 0, rng.choice((1, 3, 8, 16)), rng.choice((1, 4, 50))))
        else:
            steps.append(("run", rng.choice((1, 1, 1, 1, 2, 3, 5, 7, 8, 9, 16, 17, 23))))
    return kind, max_ticks, steps + [("read",)]


def test_random_sequences_agree_with_the_model(check):
    """240 seeded sequences of run(k) / read / re-enable on the three kinds of one-entry plan, 40 plans per process"""
    routes = set()
    for batch in range(6):
        cases = [random_steps(seed) for seed in range(40 * batch, 40 * batch + 40)]
        ops, spans = ["init"], []
        for kind, max_ticks, steps in cases:
            ops += timed_plan(kind, 1, max_ticks)
            spans.append(len(ops))
            ops += sampler_ops(steps) + ["destroy"]
        res = check(f"random_{batch}", ops)
        for seed, (first, (kind, max_ticks, steps)) in enumerate(zip(spans, cases), 40 * batch):
            diffs = disagreements(res[first:first + len(steps)], steps, model_for(kind, 1, max_ticks))
            assert diffs == [], (seed, kind, steps, diffs)
            routes.add(kind)
    assert routes == set(KINDS)


def test_model_has_teeth(check):
    """the model is the yardstick of the tests above: with either planted defect it must disagree with the log"""
    s16 = [("timing", 0, 16, 8)] + [("run", 1)] * 20 + [("read",)]
    coh = [("timing", 0, 8, 8), ("run", 1), ("run", 5), ("run", 3), ("read",)]
    for name, kind, steps, mutate in (("teeth_group", "single", s16, "group_is_stride"),
                                      ("teeth_cohort", "cohorts", coh, "cohort_run_counts_one")):
        _, diffs = run_sampler_case(check, name, kind, steps)
        assert diffs == []
        _, diffs = run_sampler_case(check, name, kind, steps, mutate=mutate)
        assert diffs, f"the model with `{mutate}` still agrees with the log"


def test_mixed_sequences_are_sampled_at_stride_8():
    """the device test replays MIXED_SEQUENCES at stride 8 and asks for a total above 0: the model must cover launches"""
    for kind in KINDS:
        for name in MIXED_SEQUENCES:
            m = model_for(kind, max_ticks=2048)
            m.enable(0, 8, 64)
            for k in mixed_runs(name):
                m.run(k)
            assert m.read()[0] >= 8


# ---- replica cohorts --------------------------------------------------------------------------------------------------------
def cohort_plan(C, entries=2, skip=()):
    ops = ["init", "plan"] + [["add", *launch(ENTRY_FN + i, grid=(2000, 1, 1)), 16, i] for i in range(entries)]
    ops += [["add_cohort", i, c, *launch(cohort_fn(c, i), grid=(2000 // C, 1, 1)), 16, 32 * c + i]
            for c in range(C) for i in range(entries) if (c, i) not in skip]
    return ops


def assert_forked_and_joined(op, caller="stream#caller"):
    """of one cohort run, failed or not: the fork is recorded on the caller's stream before any side stream waits for it;
    a side stream launches only after its wait; its join is recorded after its last launch; the caller's stream waits
    for every join.  -> {side stream: its launches}"""
    lines = [l for l in op.log if l.rc == 0]
    forks = [l for l in lines if l.call == "hipEventRecord" and l["stream"] == caller]
    side = {}
    for l in lines:
        if l.call == "hipStreamWaitEvent" and l["stream"] != caller:
            fork = [f for f in forks if f["event"] == l["event"] and f.at < l.at]
            assert fork and l["stream"] not in side, l  # one wait per side stream, for the fork recorded before it
            side[l["stream"]] = l.at
    out = {}
    for st, waited_at in side.items():
        mine = [l for l in op.launches if l["stream"] == st]
        assert all(l.at > waited_at for l in mine)
        last = max([l.at for l in mine] + [waited_at])
        joins = [l for l in lines if l.call == "hipEventRecord" and l["stream"] == st and l.at > last]
        assert len(joins) == 1, (st, op)
        waits = [l for l in lines if l.call == "hipStreamWaitEvent" and l["stream"] == caller
                 and l["event"] == joins[0]["event"] and l.at > joins[0].at]
        assert len(waits) == 1, (st, op)
        out[st] = mine
    strays = {l["stream"] for l in op.launches} - set(out) - {caller}
    assert not strays, f"launches on streams that never waited for the fork: {strays}"
    return out


@pytest.mark.parametrize("C", [2, 3, 4])
def test_cohorts_fork_and_join(check, C):
    ops = cohort_plan(C) + ["cohorts", "run,1,caller", "run,3,caller", "run,2,caller", "run,1,caller",
                            ["add_cohort", 0, 0, *launch(cohort_fn(0, 0)), 16, 0], "destroy"]
    res = check(f"cohorts_{C}", ops)
    assert res.op("cohorts").out == {"n": str(C)}
    runs = [o for o in res if o.text.startswith("run")]
    whole = [(ENTRY_FN + i, dict(grid=(2000, 1, 1), block=(64, 1, 1), lds=0), 16, i) for i in range(2)]
    for o in (runs[0], runs[3]):  # run(1): the whole-range entries on the caller's stream, no event
        assert_is_entries(o.log, 1, "stream#caller", whole)
    # the first cohort run creates the fork event, then a non-blocking stream and its join event per side cohort
    ev = [f"event#{k}" for k in range(1, C + 1)]
    st = ["stream#caller"] + [f"stream#{k}" for k in range(1, C)]
    want = [("hipEventCreateWithFlags", 2, ev[0])]  # hipEventDisableTiming
    for c in range(1, C):
        want += [("hipStreamCreateWithFlags", 1, st[c]), ("hipEventCreateWithFlags", 2, ev[c])]  # hipStreamNonBlocking
    body = lambda reps: ([("record", ev[0], st[0])] + [("wait", st[c], ev[0]) for c in range(1, C)]
                         + [("launch", cohort_fn(c, i), st[c]) for _ in range(reps) for c in range(C) for i in range(2)]
                         + [x for c in range(1, C) for x in (("record", ev[c], st[c]), ("wait", st[0], ev[c]))])
    assert [brief(l) for l in runs[1].log] == want + body(3)  # tick-major, each launch on its cohort's own stream
    assert [brief(l) for l in runs[2].log] == body(2)  # streams and events are reused
    for o, reps in ((runs[1], 3), (runs[2], 2)):
        assert o.rc == 0
        sides = assert_forked_and_joined(o)
        assert len(sides) == C - 1 and all(len(v) == 2 * reps for v in sides.values())
        for l in o.launches:  # geometry and bytes of the cohort's own entry
            c, i = (int(l["fn"], 16) - 0x1000) // 16, int(l["fn"], 16) % 16
            assert l["grid"] == f"{2000 // C},1,1" and l.bytes == buffer(16, 32 * c + i)
    refused = res.op("add_cohort", 2 * C)
    assert refused.rc == BAD_ARG and "wd_plan_add_cohort" in refused.err
    assert len(res.op("destroy").calls("hipStreamDestroy")) == C - 1 and len(res.op("destroy").calls("hipEventDestroy")) == C


def test_incomplete_cohorts_run_as_one_stream(check):
    res = check("cohorts_incomplete", cohort_plan(3, skip={(2, 1)}) + ["cohorts", "run,4,caller", "destroy"])
    assert res.op("cohorts").out == {"n": "1"}
    whole = [(ENTRY_FN + i, dict(grid=(2000, 1, 1), block=(64, 1, 1), lds=0), 16, i) for i in range(2)]
    assert_is_entries(res.op("run").log, 4, "stream#caller", whole)


def test_cohort_arguments_out_of_range_are_refused(check):
    ops = cohort_plan(2) + [["add_cohort", 0, 4, *launch(cohort_fn(4, 0)), 16, 0],
                            ["add_cohort", 2, 1, *launch(cohort_fn(1, 2)), 16, 0],
                            ["add_cohort", -1, 1, *launch(cohort_fn(1, 0)), 16, 0],
                            ["add_cohort", 0, -1, *launch(cohort_fn(0, 0)), 16, 0], "cohorts", "destroy"]
    res = check("cohorts_bad_arg", ops)
    for o in res[-6:-2]:
        assert o.rc == BAD_ARG and "wd_plan_add_cohort" in o.err, o
    assert res.op("cohorts").out == {"n": "2"} and res.lines[2:] == []


# ---- the multi-tick form ------------------------------------------------------------------------------------------------------
def test_multi_tick_runs_are_split_and_carry_their_tick_count(check):
    given = buffer(28, 9)
    for max_ticks, want in ((16, (16, 16, 5)), (1, (1,) * 37), (2048, (37,))):
        ops = ["init", "plan", ["add", *launch(ENTRY_FN, grid=(2000, 1, 1)), 24, 3],
               ["multi", *launch(MULTI_FN, grid=(2000, 1, 1), block=(128, 1, 1), lds=512), 28, 9, 20, max_ticks],
               "run,37,caller", "run,1,caller", "run,2,null", "destroy"]
        res = check(f"multi_tick_{max_ticks}", ops)
        first, one, two = [o for o in res if o.text.startswith("run")]
        assert first.rc == 0 and [brief(l) for l in first.log] == [("launch", MULTI_FN, "stream#caller")] * len(want)
        for l, n in zip(first.log, want):  # the count at byte 20, every other byte as given
            assert l.bytes == given[:20] + struct.pack("<i", n) + given[24:]
            assert (l["grid"], l["block"], l["lds"]) == ("2000,1,1", "128,1,1", "512")
        (l,) = one.log  # run(1) is the one-tick entry, its own buffer untouched
        assert brief(l) == ("launch", ENTRY_FN, "stream#caller") and l.bytes == buffer(24, 3)
        assert [brief(l) for l in two.log] == [("launch", MULTI_FN, "stream#null")] * (2 if max_ticks == 1 else 1)
        assert not [l for l in res.lines if l.call in EVENT_CALLS]  # no fork, no join


def test_multi_tick_bad_arguments_are_refused(check):
    one = ["init", "plan", ["add", *launch(ENTRY_FN), 24, 3]]
    m = lambda n, offset, max_ticks: ["multi", *launch(MULTI_FN), n, 9, offset, max_ticks]
    res = check("multi_tick_bad_arg", one + [m(28, 18, 16), m(28, 28, 16), m(30, 28, 16), m(2, 0, 16), m(28, 24, 0),
                                             m(28, 24, -1), "run,5,caller", m(28, 24, 16), "run,5,caller", "destroy"])
    for o in res[3:9]:  # unaligned; past the end; the four bytes end past the buffer; max_ticks < 1
        assert o.rc == BAD_ARG and "wd_plan_set_multi_tick" in o.err, o
    assert [brief(l)[1] for l in res.op("run").log] == [ENTRY_FN] * 5  # refused: the plan is as it was
    assert [brief(l)[1] for l in res.op("run", 1).log] == [MULTI_FN]  # the last four bytes are a valid place
    res = check("multi_tick_two_entries", one + [["add", *launch(ENTRY_FN + 1), 24, 3], m(28, 24, 16), "destroy"])
    assert res.op("multi").rc == BAD_ARG


# ---- the graph route ------------------------------------------------------------------------------------------------------------
def test_graph_capture_instantiate_and_replay(check):
    ops = three_entry_plan() + ["run_graph,1,caller", "graph,4,caller", "run_graph,3,caller", "run_graph,2,null",
                                "graph,2,caller", "run_graph,1,caller", "graph,0,caller", "destroy"]
    res = check("graph", ops)
    refused = res.op("run_graph")
    assert refused.rc == BAD_ARG and "not instantiated" in refused.err and not refused.log
    for nth, (reps, graph, exec_) in enumerate(((4, "graph#1", "exec#1"), (2, "graph#2", "exec#2"))):
        o = res.op("graph", nth)
        head = o.log[:1] if nth == 0 else o.log[:2]
        if nth:  # a second instantiate destroys the first exec
            assert (head[0].call, head[0]["exec"]) == ("hipGraphExecDestroy", "exec#1")
        assert o.rc == 0 and (head[-1].call, head[-1]["stream"], head[-1]["mode"]) == ("hipStreamBeginCapture", "stream#caller", "1")
        body = o.log[len(head):-3]
        assert_is_entries(body, reps, "stream#caller")
        assert all(l["captured"] == "1" for l in body)
        end, inst, gone = o.log[-3:]
        assert (end.call, end["stream"], end["out"]) == ("hipStreamEndCapture", "stream#caller", graph)
        assert (inst.call, inst["graph"], inst["out"]) == ("hipGraphInstantiate", graph, exec_)
        assert (gone.call, gone["graph"]) == ("hipGraphDestroy", graph)  # the captured graph is not kept
    for o, n, stream, exec_ in ((res.op("run_graph", 1), 3, "caller", "exec#1"), (res.op("run_graph", 2), 2, "null", "exec#1"),
                                (res.op("run_graph", 3), 1, "caller", "exec#2")):
        assert o.rc == 0 and [(l.call, l["exec"], l["stream"]) for l in o.log] == [("hipGraphLaunch", exec_, f"stream#{stream}")] * n
    assert res.op("graph", 2).rc == BAD_ARG and not res.op("graph", 2).log
    assert [l["exec"] for l in res.op("destroy").calls("hipGraphExecDestroy")] == ["exec#2"]


# ---- failures ---------------------------------------------------------------------------------------------------------------------
def assert_failed(op, call, error, launches=None):
    """the HIP code is returned, wd_last_error names the call, the runtime's sticky error is consumed exactly once, and
    nothing is launched after the failing call"""
    assert op.rc == error and call in op.err and str(error) in op.err, op
    assert len(op.calls("hipGetLastError")) == 1 and op.calls("hipGetLastError")[0].rc == error
    failed = [l for l in op.log if l.rc != 0 and l.call != "hipGetLastError"]
    assert len(failed) == 1 and failed[0].call == call.split("(")[0]
    assert not [l for l in op.launches if l.at > failed[0].at]
    if launches is not None:
        assert len(op.launches) == launches
    return failed[0]


ROUTES = {"single": (three_entry_plan(), "run,4,caller", (1, 2, 12)),
          "single_of_cohort_plan": (cohort_plan(3), "run,1,caller", (1, 2)),
          "cohorts": (cohort_plan(3), "run,3,caller", (1, 2, 3, 7, 18)),
          "multi": (["init"] + timed_plan("multi", 1, 4), "run,11,caller", (1, 2, 3)),
          "graph": (three_entry_plan(), "graph,4,caller", (1, 5, 12))}


@pytest.mark.parametrize("route", list(ROUTES))
def test_kth_launch_fails(check, route):
    setup, run, ks = ROUTES[route]
    for k in ks:
        res = check(f"launch_{k}_fails_{route}", setup + [f"fail,hipModuleLaunchKernel,{k},{LAUNCH_FAILURE}", run, run, "destroy"])
        o = res.op(run)
        assert_failed(o, "hipModuleLaunchKernel", LAUNCH_FAILURE, launches=k)
        if route == "cohorts":  # every side stream that waited for the fork is joined back before the error returns
            assert len(assert_forked_and_joined(o)) == 2
        if route == "graph":  # the capture is still ended, and its graph destroyed (nothing live: `check` itself)
            assert [l.call for l in o.log[-2:]] == ["hipStreamEndCapture", "hipGraphDestroy"]
            assert not o.calls("hipGraphInstantiate")
        again = res.op(run, 1)  # the plan is usable afterwards
        assert again.rc == 0 and len(again.launches) == {"single": 12, "single_of_cohort_plan": 2, "cohorts": 18, "multi": 3,
                                                         "graph": 12}[route]
        if route == "cohorts":
            assert len(assert_forked_and_joined(again)) == 2


def test_capture_and_instantiate_failures_leave_nothing_behind(check):
    plan = three_entry_plan()
    res = check("begin_capture_fails", plan + [f"fail,hipStreamBeginCapture,1,{INVALID_VALUE}", "graph,2,caller",
                                               "run_graph,1,caller", "destroy"])
    assert_failed(res.op("graph"), "hipStreamBeginCapture", INVALID_VALUE, launches=0)
    assert res.op("run_graph").rc == BAD_ARG
    res = check("end_capture_fails", plan + [f"fail,hipStreamEndCapture,1,{INVALID_VALUE}", "graph,2,caller",
                                             "run_graph,1,caller", "destroy"])
    assert_failed(res.op("graph"), "hipStreamEndCapture", INVALID_VALUE, launches=6)
    assert res.op("run_graph").rc == BAD_ARG and not res.op("graph").calls("hipGraphInstantiate")
    res = check("instantiate_fails", plan + ["graph,1,caller", f"fail,hipGraphInstantiate,1,{OUT_OF_MEMORY}", "graph,2,caller",
                                             "run_graph,1,caller", "graph,2,caller", "run_graph,1,caller", "destroy"])
    o = res.op("graph", 1)
    assert_failed(o, "hipGraphInstantiate", OUT_OF_MEMORY, launches=6)
    assert o.log[-1].call == "hipGraphDestroy"
    assert res.op("run_graph").rc == BAD_ARG  # the first exec is gone, the second never came to be
    assert res.op("run_graph", 1).rc == 0
    res = check("graph_launch_fails", plan + ["graph,1,caller", f"fail,hipGraphLaunch,2,{LAUNCH_FAILURE}", "run_graph,4,caller",
                                              "destroy"])
    assert_failed(res.op("run_graph"), "hipGraphLaunch", LAUNCH_FAILURE)
    assert len(res.op("run_graph").calls("hipGraphLaunch")) == 2


def test_event_record_failures(check):
    # a bracket's start on the single route: the launch it would have preceded is not issued
    res = check("record_fails_single", three_entry_plan() + ["timing,1,1,4", f"fail,hipEventRecord,3,{INVALID_VALUE}",
                                                             "run,4,caller", "destroy"])
    assert_failed(res.op("run"), "hipEventRecord", INVALID_VALUE, launches=4)
    # the fork: nothing is forked, nothing launched
    res = check("fork_record_fails", cohort_plan(3) + [f"fail,hipEventRecord,1,{INVALID_VALUE}", "run,3,caller", "run,3,caller",
                                                       "destroy"])
    o = res.op("run")
    assert_failed(o, "hipEventRecord(fork)", INVALID_VALUE, launches=0)
    assert not o.calls("hipStreamWaitEvent")
    assert res.op("run", 1).rc == 0 and len(assert_forked_and_joined(res.op("run", 1))) == 2
    # a side stream's wait for the fork: the side streams that do wait are joined back, the other one gets no launch
    res = check("fork_wait_fails", cohort_plan(3) + [f"fail,hipStreamWaitEvent,2,{INVALID_VALUE}", "run,3,caller", "destroy"])
    o = res.op("run")
    assert_failed(o, "hipStreamWaitEvent(fork)", INVALID_VALUE, launches=0)
    assert list(assert_forked_and_joined(o)) == ["stream#1"]
    # the first join: the error is returned, and the other side stream is still joined
    res = check("join_record_fails", cohort_plan(3) + [f"fail,hipEventRecord,2,{INVALID_VALUE}", "run,3,caller", "destroy"])
    o = res.op("run")
    assert_failed(o, "hipEventRecord(join)", INVALID_VALUE, launches=18)
    tail = [brief(l) for l in o.log if l.rc == 0 and l.call in ("hipEventRecord", "hipStreamWaitEvent")][-2:]
    assert tail == [("record", "event#3", "stream#2"), ("wait", "stream#caller", "event#3")]
    # the end of the bracket around a timed cohort run: after the joins
    res = check("bracket_end_fails", cohort_plan(2, entries=1) + ["timing,0,8,4", f"fail,hipEventRecord,4,{INVALID_VALUE}",
                                                                  "run,3,caller", "destroy"])
    o = res.op("run")
    assert_failed(o, "hipEventRecord", INVALID_VALUE, launches=6)
    assert len(assert_forked_and_joined(o)) == 1


@pytest.mark.parametrize("call,nth", [("hipStreamCreateWithFlags", 1), ("hipStreamCreateWithFlags", 2),
                                      ("hipStreamCreateWithFlags", 3), ("hipEventCreateWithFlags", 1),
                                      ("hipEventCreateWithFlags", 2), ("hipEventCreateWithFlags", 4)])
def test_side_stream_creation_fails(check, call, nth):
    """the first cohort run cannot make one of its streams or events: the error is returned with nothing forked or
    launched, and the next run makes what is missing -- each side stream with its own join event"""
    res = check(f"{call}_{nth}_fails", cohort_plan(4) + [f"fail,{call},{nth},{OUT_OF_MEMORY}", "run,2,caller", "run,2,caller",
                                                         "run,2,caller", "destroy"])
    o = res.op("run")
    assert_failed(o, call, OUT_OF_MEMORY, launches=0)
    assert not o.calls("hipEventRecord", "hipStreamWaitEvent")
    for again in (res.op("run", 1), res.op("run", 2)):
        assert again.rc == 0 and len(again.launches) == 16
        sides = assert_forked_and_joined(again)
        assert sorted(len(v) for v in sides.values()) == [4, 4, 4]
    assert not res.op("run", 2).calls("hipStreamCreateWithFlags", "hipEventCreateWithFlags")
    made = [l for l in res.lines if l.call in ("hipStreamCreateWithFlags", "hipEventCreateWithFlags") and l.rc == 0]
    gone = res.op("destroy").calls("hipStreamDestroy", "hipEventDestroy") + res.op("run").calls("hipStreamDestroy")
    assert len(made) == len(gone)


def test_timing_calls_fail_cleanly(check):
    ops = ["init"] + timed_plan("single") + [f"fail,hipEventCreate,3,{OUT_OF_MEMORY}", "timing,0,1,4", "run,2,caller", "read",
                                             "timing,0,1,2", "run,2,caller", f"fail,hipEventElapsedTime,2,{INVALID_VALUE}", "read",
                                             "read", "timing,5,1,2", "timing,0,0,2", "timing,0,1,0", "destroy"]
    res = check("timing_failures", ops)
    assert_failed(res.op("timing"), "hipEventCreate", OUT_OF_MEMORY)
    assert not res.op("run").calls(*EVENT_CALLS) and res.op("read").out == {"ms": "0.0", "n": "0"}  # timing stayed off
    assert_failed(res.op("read", 1), "hipEventElapsedTime", INVALID_VALUE)
    assert res.op("read", 2).out["n"] == "2"  # the failed read dropped nothing
    for nth in (2, 3, 4):
        assert res.op("timing", nth).rc == BAD_ARG
