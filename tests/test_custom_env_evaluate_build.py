"""The one-launch evaluation of a custom environment without a GPU (include/wd_env_evaluate.h;
utils/custom_tick.py::FusedEvaluateMixin): the host-buildable half of the header computes the probabilities the numpy model
computes, running sums that equal wd_env_rollout.h's bit for bit, and the first-maximum scan on crafted rows; the worked
example and the probe compile to the expected entries without scratch memory or spills and with the launch bounds the host
admits blocks by; the four existing examples and the in-tree code objects are what they were; the mixin packs exactly the
kernarg layout the compiled Evaluate entries declare and refuses by name whatever the kit does not serve; and the cases of
tests/test_gpu_custom_env_evaluate.py -- replayed here on the host alone -- have the coverage they are meant to have.  hipcc
cross-compiles gfx950, so no GPU is needed."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from tests import custom_crafted_policies as crafted
from tests import custom_evaluate_model as model
from tests import custom_tick_model as tick_model
from tests.test_custom_env_rollout_build import (_DeviceTensor, _metadata, _sha, _StubData, _StubFunctions, _StubResetter,
                                                 _StubSampler)
from warp_drive_amd import build as wd_build

ROOT = model.ROOT
UNITS = {"RendezvousEvaluate": (model.EXAMPLE_SOURCE, model.EXAMPLE_KERNELS, "HipRendezvousEvaluate"),
         "EvaluateProbe": (model.PROBE_SOURCE, model.PROBE_KERNELS, "HipEvaluateProbe")}
SHA_LIST = os.path.join(ROOT, "profiles", "r42_code_object_sha256.txt")
TRAILING = 12   # WD_EVALUATE_PARAMS
f32 = np.float32

_CACHE = []


@pytest.fixture(autouse=True)
def cache(tmp_path_factory, monkeypatch):
    """one cache directory for the module: each unit compiles once"""
    if not _CACHE:
        _CACHE.append(str(tmp_path_factory.mktemp("env_cache")))
    monkeypatch.setenv("WD_ENV_CACHE", _CACHE[0])
    return _CACHE[0]


# ------------------------------------------------------------------------------------------------ the host program
@pytest.fixture(scope="module")
def pick_check(tmp_path_factory):
    """tests/c/evaluate_pick_check.cpp built with the host compiler alone: no HIP include path, no HIP define"""
    exe = str(tmp_path_factory.mktemp("evaluate_pick_check") / "evaluate_pick_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c", "evaluate_pick_check.cpp"), "-o", exe], check=True)

    def run(kind, A, rows):
        """rows [R, 8] float32 -> kind 0: (p [R, 8], cum [R, 8], rollout cum [R, 8], pick [R]); kind 1: pick [R]"""
        rows = np.ascontiguousarray(rows, dtype=f32).reshape(-1, 8)
        lines = [str(len(rows))] + [f"{kind} {A} " + " ".join(str(int(b)) for b in r.view(np.uint32)) for r in rows]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        got = [line.split() for line in out.splitlines()]
        assert len(got) == len(rows)
        if kind == 1:
            assert all(g[0] == "S" and len(g) == 2 for g in got)
            return np.array([int(g[1]) for g in got], dtype=np.int32)
        assert all(g[0] == "L" and len(g) == 26 for g in got)
        table = np.array([[int(v) for v in g[1:]] for g in got], dtype=np.int64)
        as_f = lambda t: t.astype(np.uint32).view(f32)  # noqa: E731
        return as_f(table[:, :8]), as_f(table[:, 8:16]), as_f(table[:, 16:24]), table[:, 24].astype(np.int32)

    return run


def _softmax(logits):
    """the model's probabilities of rows of logits (tests/classic_control_policy.py::policy_probabilities' last lines)"""
    x = np.asarray(logits, dtype=f32)
    e = np.exp((x - x.max(axis=1, keepdims=True)).astype(f32)).astype(f32)
    s = np.zeros(len(x), f32)
    for a in range(x.shape[1]):
        s = (s + e[:, a]).astype(f32)
    return (e / s[:, None]).astype(f32)


@pytest.mark.parametrize("A", [1, 2, 5, 8])
def test_the_host_build_computes_the_probabilities_and_the_rollouts_running_sums(pick_check, A):
    """300 seeded rows of logits in [-6, 6] and crafted rows whose probabilities are exact (equal logits; gaps of 128).
    The running sums built from the probabilities equal wd_rollout_running_sums' bit for bit on EVERY row; the
    probabilities are the model's within NEAR_WINDOW (two expf), bit for bit on the crafted rows; slots at and past A are
    0; the pick is the first maximum of the program's own probabilities."""
    rng = np.random.RandomState(40 + A)
    rows = np.zeros((300, 8), f32)
    rows[:, :A] = rng.uniform(-6, 6, size=(300, A)).astype(f32)
    exact = np.zeros((4, 8), f32)                   # all equal: 1 / A each
    exact[1, :A] = 3.5                              # all equal, another value
    exact[2, :A], exact[2, A - 1] = -128.0, 0.0     # the last slot wins alone
    exact[3, :A], exact[3, 0] = -128.0, 0.0         # ... the first
    if A >= 3:
        exact[2, 0] = 0.0                           # a tie of the first and the last slot
    rows = np.concatenate([rows, exact])
    rows[:, A:] = 77.0                              # behind A: ignored, whatever stands there
    p, cum, rollout_cum, pick = pick_check(0, A, rows)
    assert cum.tobytes() == rollout_cum.tobytes()
    assert (p[:, A:] == 0).all() and (cum[:, A:] == cum[:, A - 1:A]).all()
    want = _softmax(rows[:, :A])
    worst = float(np.abs(p[:, :A].astype(np.float64) - want.astype(np.float64)).max())
    print(f"A {A}: largest difference of a probability {worst:.3g}")
    assert worst < model.NEAR_WINDOW
    assert p[-4:, :A].tobytes() == want[-4:].tobytes()
    assert set(p[-4:-2, :A].reshape(-1).tolist()) == {float(f32(1.0) / f32(A))}
    assert pick.tolist() == model.first_maximum(p[:, :A]).tolist()
    assert pick[-4] == 0 and pick[-3] == 0 and pick[-1] == 0 and pick[-2] == (0 if A >= 3 or A == 1 else A - 1)
    assert (model.running_sums(p[:, :A]) == cum[:, :A]).all()
    if A > 1:
        assert len(set(pick[:300].tolist())) == A


def test_the_first_maximum_scan_on_crafted_rows(pick_check):
    """exact ties (the lower index wins), one-ulp gaps, A = 1, the maximum in the last slot at A = 8, slots at and past
    n_actions never picked"""
    up = lambda v: np.nextafter(f32(v), f32(2))    # noqa: E731
    down = lambda v: np.nextafter(f32(v), f32(-1))  # noqa: E731
    cases = [
        # (A, probabilities, expected)
        (5, [0.2, 0.2, 0.2, 0.2, 0.2, 0, 0, 0], 0),                    # all tied
        (5, [0.0, 0.5, 0.0, 0.5, 0.0, 0, 0, 0], 1),                    # two tied winners behind a zero
        (8, [0.125] * 8, 0),
        (3, [0.25, up(0.25), 0.25, 0, 0, 0, 0, 0], 1),                 # one ulp above: it wins
        (3, [0.25, down(0.25), 0.25, 0, 0, 0, 0, 0], 0),               # one ulp below: it does not
        (4, [down(0.25), 0.25, up(0.25), up(0.25), 0, 0, 0, 0], 2),    # rising by one ulp, then a tie
        (8, [0.1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1, up(0.1)], 7),          # the maximum in the last slot
        (8, [0, 0, 0, 0, 0, 0, 0, 1.0], 7),
        (1, [1.0, 0, 0, 0, 0, 0, 0, 0], 0),                            # A = 1
        (1, [1.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0, 5.0], 0),              # larger values behind n_actions: never picked
        (2, [0.5, 0.5, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0], 0),
        (5, [0.1, 0.3, 0.2, 0.3, 0.1, 0.9, 0.9, 0.9], 1),
        (7, [0, 0, 0, 0, 0, 0, 1e-30, 1.0], 6),
        (2, [0.0, 0.0, 1.0, 0, 0, 0, 0, 0], 0),                        # all zeros in front: action 0
    ]
    for A in sorted({c[0] for c in cases}):
        rows = [c for c in cases if c[0] == A]
        got = pick_check(1, A, np.array([r[1] for r in rows], dtype=f32))
        assert got.tolist() == [r[2] for r in rows], (A, got.tolist())
        assert got.tolist() == model.first_maximum(np.array([r[1][:A] for r in rows], dtype=f32)).tolist()


def test_the_header_is_self_contained_and_leaves_its_parents_alone():
    text = open(model.HEADER).read()
    assert set(re.findall(r"^\s*#include\s+(\S+)", text, re.M)) == {"<hip/hip_runtime.h>", "<stdint.h>", "<math.h>",
                                                                    '"wd_env_rollout.h"'}
    code = re.sub(r"//.*", "", text)
    assert "asm" not in code and "atomic" not in code.lower() and "shfl" not in code and "csrc" not in code
    assert code.count("wd_rollout_logits<H, F>") == 1 and "wd_rollout_pick(" in code and "wd_tick_block(" in code
    assert "fmaf" not in code                                         # no network arithmetic of its own
    assert code.count("for (") == code.count("WD_ROLLOUT_UNROLL") + 3  # all unrolled but the stage and the two restore loops
    for name in ("wd_env.h", "wd_env_tick.h", "wd_env_rollout.h", "wd_env_update.h"):
        assert "wd_evaluate" not in open(os.path.join(ROOT, "include", name)).read().lower(), name
    trainer = open(os.path.join(ROOT, "warp_drive_amd", "training", "trainer.py")).read()
    assert "FusedEvaluateMixin" not in trainer and "custom_evaluate_launch" not in trainer


# ------------------------------------------------------------------------------------------------------ the build
def _env_class(unit):
    if unit == "RendezvousEvaluate":
        return model.example_module().RendezvousEvaluate
    from tests.custom_envs.evaluate_probe import EvaluateProbe

    return EvaluateProbe


def _bounds(cls):
    return cls.ROLLOUT_MAX_THREADS if cls.EVALUATE_MAX_THREADS is None else cls.EVALUATE_MAX_THREADS


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_the_units_build_to_the_expected_entries_without_scratch_or_spills(cache, unit):
    source, kernels, prefix = UNITS[unit]
    manifest_before = _sha(wd_build.MANIFEST)
    in_tree_before = sorted(os.listdir(wd_build.CSRC))
    path = wd_build.build_env_unit(unit, source)
    assert os.path.dirname(path) == cache and wd_build.kernels_in(path) == kernels
    assert _sha(wd_build.MANIFEST) == manifest_before and sorted(os.listdir(wd_build.CSRC)) == in_tree_before
    sources = wd_build.unit_sources(source, [f[2:] for f in wd_build.env_unit_flags(source) if f.startswith("-I")])
    for header in ("wd_env_evaluate.h", "wd_env_rollout.h", "wd_env_tick.h", "wd_env.h"):
        assert os.path.join(ROOT, "include", header) in sources
    meta = _metadata(path)
    assert sorted(meta) == kernels
    cls = _env_class(unit)
    assert cls.EVALUATE_KERNEL == prefix + "Evaluate_H{width}" and cls.EVALUATE_POLICY_OPT_IN is True
    for width in (32, 64):
        for pattern, bounds in ((cls.EVALUATE_KERNEL, _bounds(cls)), (cls.ROLLOUT_KERNEL, cls.ROLLOUT_MAX_THREADS)):
            name = pattern.format(width=width)
            m = meta[name]
            print(f"{name}: {m['vgprs']} VGPRs, private {m['private']}, spills {m['vgpr_spills']} / {m['sgpr_spills']}, "
                  f"static LDS {m['lds']}, at most {m['max_threads']} threads")
            assert (m["private"], m["vgpr_spills"], m["sgpr_spills"]) == (0, 0, 0), name
            assert m["max_threads"] == bounds[width] == {32: 1024, 64: 512}[width]
            assert 0 < m["vgprs"] <= 512 // (bounds[width] // 256), name  # the lanes' share of a SIMD's 512
        explicit = [a for a in meta[cls.EVALUATE_KERNEL.format(width=width)]["args"] if not a[2].startswith("hidden_")]
        assert len(explicit) == len(cls.TICK_STEP_ARGS) + TRAILING
        assert explicit[-1][1] == 4 and explicit[-1][2] == "by_value"           # `int ticks` LAST
    for name in (prefix + "Step", prefix + "Tick"):
        assert (meta[name]["private"], meta[name]["vgpr_spills"], meta[name]["sgpr_spills"]) == (0, 0, 0), name


def test_the_example_is_one_class_for_the_whole_cycle():
    from warp_drive_amd.utils.custom_tick import FusedEvaluateMixin, FusedRolloutMixin, FusedUpdateMixin

    cls = _env_class("RendezvousEvaluate")
    assert issubclass(cls, FusedEvaluateMixin) and issubclass(cls, FusedUpdateMixin) and issubclass(cls, FusedRolloutMixin)
    assert cls.__mro__[1] is FusedEvaluateMixin and cls.__mro__[2] is FusedUpdateMixin
    assert cls.UPDATE_KERNEL_PREFIX == "HipRendezvousEvaluatePg" and cls.UPDATE_OBS_SIZE == 5
    assert FusedEvaluateMixin.EVALUATE_MAX_THREADS is None and FusedEvaluateMixin.EVALUATE_KERNEL is None
    here = os.path.dirname(model.EXAMPLE_SOURCE)
    assert sorted(f for f in os.listdir(here) if f != "__pycache__") == ["rendezvous_evaluate.hip", "rendezvous_evaluate.py"]
    source = re.sub(r"//.*", "", open(model.EXAMPLE_SOURCE).read())
    assert "WD_PG_UPDATE_ENTRIES(RendezvousEvaluate, 5)" in source and source.count("rdve_step(") == 5
    assert "rendezvous_update" not in source and "rendezvous_policy" not in source
    assert not any("rendezvous" in unit.lower() or "probe" in unit.lower() for unit, _ in wd_build.UNITS.values())
    owners = wd_build.in_tree_kernel_owners()
    assert not [k for k in model.EXAMPLE_KERNELS + model.PROBE_KERNELS if k in owners]


# -------------------------------------------------------------------------------- what was there is what it was
def _sha_record():
    """(in-tree objects {name: (parent, tree)}, example sources {(example, file): (parent, tree)}) of the round's record"""
    objects, sources = {}, {}
    for line in open(SHA_LIST):
        if line.startswith("#") or line.startswith("object ") or line.startswith("example: file") or not line.strip():
            continue
        parts = line.split()
        if parts[0].endswith(":"):
            sources[(parts[0][:-1], parts[1])] = (parts[2], parts[3])
            assert parts[4] == "yes"
        else:
            objects[parts[0]] = (parts[1], parts[2])
            assert parts[3] == "yes"
    return objects, sources


def test_the_existing_examples_resolve_to_the_parents_cache_names():
    """a unit's cache file name hashes the contents of its sources, the flags and the compiler's version
    (build.env_unit_path): every file the four existing examples are compiled from has the parent commit's bytes, and none
    of them reads the new header -- so the names, and the objects behind them, are the parent's"""
    _, sources = _sha_record()
    examples = {"rendezvous": "rendezvous_step.hip", "rendezvous_fused": "rendezvous_fused.hip",
                "rendezvous_policy": "rendezvous_policy.hip", "rendezvous_update": "rendezvous_update.hip"}
    seen = set()
    for folder, name in examples.items():
        src = os.path.join(ROOT, "examples", folder, name)
        files = wd_build.unit_sources(src, [f[2:] for f in wd_build.env_unit_flags(src) if f.startswith("-I")])
        assert model.HEADER not in files
        for path in files:
            key = (folder, os.path.relpath(path, ROOT))
            parent, tree = sources[key]
            assert parent == tree == hashlib.sha256(open(path, "rb").read()).hexdigest(), key
            seen.add(key)
    assert seen == set(sources)


def test_no_in_tree_code_object_changed():
    objects, _ = _sha_record()
    assert set(objects) == set(wd_build.UNITS) and all(parent == tree for parent, tree in objects.values())
    built = {n: os.path.join(wd_build.CSRC, n) for n in objects if os.path.exists(os.path.join(wd_build.CSRC, n))}
    differ = [n for n, path in built.items() if _sha(path) != objects[n][0]]
    assert differ == [], differ


# ------------------------------------------------------------------------------------- the mixin against the header
def _stubbed(unit, num_agents=5, pools=None, missing=(), **config):
    """the env with the device side stubbed (no code object is loaded, nothing is launched)"""
    from warp_drive_amd.managers.function_manager import CUDAFunctionFeed

    if unit == "RendezvousEvaluate":
        env = _env_class(unit)(**dict(dict(num_agents=num_agents, grid_length=4, episode_length=4), **config))
        scalars, F = {"wall_penalty": np.float32(0.125), "spread_limit": np.int32(-1), "grid_length": np.int32(4)}, 5
    else:
        env = _env_class(unit)(**dict(dict(num_agents=num_agents, episode_length=4), **config))
        scalars, F = {}, 2
    env.cuda_function_manager = _StubFunctions(missing)
    env.cuda_data_manager = _StubData(scalars, num_agents, F, pools)
    env.cuda_step_function_feed = CUDAFunctionFeed(env.cuda_data_manager)
    env.cuda_env_resetter = _StubResetter()
    return env, F


def _outputs(E, N, **other):
    import torch

    out = {"reward_sum": _DeviceTensor((E, N), torch.float32, 0xA0000), "steps": _DeviceTensor((E,), torch.int32, 0xB0000),
           "done": _DeviceTensor((E,), torch.int32, 0xC0000)}
    out.update(other)
    return out


def _trace(rows, E, N, **kw):
    import torch

    return _DeviceTensor((rows, E, N), kw.pop("dtype", torch.int32), 0xD0000, **kw)


def _packed(F, H, A, **kw):
    import torch

    return _DeviceTensor((model.policy_floats(F, H, A),), kw.pop("dtype", torch.float32), 0xE0000, **kw)


@pytest.mark.parametrize("unit,A,width,ticks,greedy,traced",
                         [("RendezvousEvaluate", 5, 32, 4, True, True), ("RendezvousEvaluate", 5, 64, 7, False, False),
                          ("EvaluateProbe", 1, 32, 3, False, True), ("EvaluateProbe", 8, 64, 1, True, False)])
def test_the_mixin_packs_the_kernarg_layout_of_the_compiled_evaluate_entry(unit, A, width, ticks, greedy, traced):
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.utils.custom_tick import custom_evaluate_launch

    env, F = _stubbed(unit, **({"n_actions": A} if unit == "EvaluateProbe" else {}))
    entry = env.EVALUATE_KERNEL.format(width=width)
    explicit = [a for a in _metadata(wd_build.build_env_unit(unit, UNITS[unit][0]))[entry]["args"]
                if not a[2].startswith("hidden_")]
    assert env.has_live_policy_evaluate(width, A)
    sampler, outputs, packed = _StubSampler(), _outputs(3, 5), _packed(F, width, A)
    trace = _trace(ticks + 1, 3, 5) if traced else None
    fn, args, block, grid, shared = env.evaluate_launch(sampler, policy=(packed, width), use_argmax=greedy, outputs=outputs,
                                                        action_trace=trace, ticks=ticks)
    n_w = model.policy_floats(F, width, A)
    assert fn.name == entry and block == (64, 1, 1) and grid == (3, 1)
    assert shared == (4 * n_w + 15) // 16 * 16 and shared % 16 == 0 and 0 <= shared - 4 * n_w < 16
    assert isinstance(args[-1], np.int32) and int(args[-1]) == ticks
    blob = drv._pack_args(args)
    assert len(blob) == max(o + s for o, s, _ in explicit) and blob[-4:] == np.int32(ticks).tobytes()
    # argument by argument: an 8-byte pointer where the entry declares a buffer, 4 bytes where it takes a value
    offset, layout = 0, []
    for a in args:
        size = 8 if isinstance(a, (drv.DevicePtr, np.uint64)) or hasattr(a, "data_ptr") else a.dtype.itemsize
        offset += (-offset) % size
        layout.append((offset, size))
        offset += size
    assert layout == [(o, s) for o, s, _ in explicit]
    assert ["global_buffer" if s == 8 else "by_value" for _, s in layout] == [k for _, _, k in explicit]
    assert env.cuda_function_manager.initialized == [entry] and env.cuda_env_resetter.calls == [(0, 0)]
    # the kit's trailing arguments, in the header's order, type by type
    tail = args[len(env.TICK_STEP_ARGS):]
    assert len(tail) == TRAILING
    assert int(tail[0]) == 0x7000 and tail[1] is packed
    assert isinstance(tail[2], np.int32) and int(tail[2]) == A
    assert int(tail[3]) == 0x9000 and isinstance(tail[4], np.int32) and int(tail[4]) == 3
    assert int(tail[5]) == model.TICK_TAG and np.dtype(type(tail[5])).itemsize == 4
    assert isinstance(tail[6], np.int32) and int(tail[6]) == (1 if greedy else 0)
    assert [t.data_ptr() for t in tail[7:10]] == [0xA0000, 0xB0000, 0xC0000]
    if traced:
        assert tail[10] is trace
    else:
        assert isinstance(tail[10], np.uint64) and int(tail[10]) == 0
    # the default tick count is the episode's; the function underneath gives the same launch
    assert int(env.evaluate_launch(sampler, (packed, width), greedy, outputs, action_trace=None)[1][-1]) == 4
    again = custom_evaluate_launch(env, entry, env.TICK_STEP_ARGS, sampler, A, packed, width, env.cuda_env_resetter, greedy,
                                   outputs, trace, ticks)
    assert drv._pack_args(again[1]) == blob and again[2:] == (block, grid, shared)


def test_the_host_admits_only_what_the_entries_serve():
    from warp_drive_amd.utils import spaces

    env, _ = _stubbed("RendezvousEvaluate")
    assert env.has_live_policy_evaluate(32, 5) and env.has_live_policy_evaluate(64, 5)
    assert env.has_live_policy_rollout(32, 5) and env.has_live_policy_rollout(64, 5)
    assert not env.has_live_policy_evaluate(48, 5) and not env.has_live_policy_evaluate(128, 5)
    assert not env.has_live_policy_evaluate(32, 0) and not env.has_live_policy_evaluate(32, 9)
    assert env.has_live_policy_evaluate(32, 1) and env.has_live_policy_evaluate(32, 8)
    multi, _ = _stubbed("RendezvousEvaluate")
    multi.action_space = {a: spaces.MultiDiscrete((5, 5)) for a in range(5)}
    assert not multi.has_live_policy_evaluate(32, 5)
    box, _ = _stubbed("RendezvousEvaluate")
    box.action_space = {a: spaces.Box(low=-1.0, high=1.0, shape=(1,), dtype=np.float32) for a in range(5)}
    assert not box.has_live_policy_evaluate(32, 1)
    wide, _ = _stubbed("RendezvousEvaluate", num_agents=520)   # a block of 576 threads
    assert wide.has_live_policy_evaluate(32, 5) and not wide.has_live_policy_evaluate(64, 5)
    edge, _ = _stubbed("RendezvousEvaluate", num_agents=512)
    assert edge.has_live_policy_evaluate(64, 5)
    pooled, _ = _stubbed("RendezvousEvaluate", pools={"mood": "mood_reset_pool"})
    assert not pooled.has_live_policy_evaluate(32, 5)
    absent, _ = _stubbed("RendezvousEvaluate", missing=["HipRendezvousEvaluateEvaluate_H64"])
    assert absent.has_live_policy_evaluate(32, 5) and not absent.has_live_policy_evaluate(64, 5)
    assert absent.has_live_policy_rollout(64, 5)               # the Rollout entry is there: the two answers are separate
    # the evaluate entries' own bound, where the class states one
    own, _ = _stubbed("RendezvousEvaluate", num_agents=300)    # a block of 320 threads
    own.EVALUATE_MAX_THREADS = {32: 256, 64: 256}
    assert not own.has_live_policy_evaluate(32, 5) and own.has_live_policy_rollout(32, 5)
    # the probe states none: the Rollout entries' bounds hold
    probe, _ = _stubbed("EvaluateProbe", num_agents=520)
    assert probe.EVALUATE_MAX_THREADS is None
    assert probe.has_live_policy_evaluate(32, 2) and not probe.has_live_policy_evaluate(64, 2)


def test_every_request_the_evaluation_does_not_serve_is_refused_by_name():
    import torch

    from warp_drive_amd.rollout import UnsupportedRolloutShape
    from warp_drive_amd.utils import spaces
    from warp_drive_amd.utils.custom_tick import custom_evaluate_launch

    env, F = _stubbed("RendezvousEvaluate")
    sampler, E, N = _StubSampler(), 3, 5
    packed, outputs = _packed(F, 32, 5), _outputs(E, N)
    ok = dict(policy=(packed, 32), use_argmax=True, outputs=outputs, ticks=4)

    def wrong(shape, dtype, short):
        """a tensor wrong in every way: not CUDA, non-contiguous, wrong dtype, one element short, None"""
        other = torch.int32 if dtype == torch.float32 else torch.float32
        return [_DeviceTensor(shape, dtype, 1, cuda=False), _DeviceTensor(shape, dtype, 1, contiguous=False),
                _DeviceTensor(shape, other, 1), _DeviceTensor(short, dtype, 1), None]

    n_w = model.policy_floats(F, 32, 5)
    cases = [(dict(ok, policy=packed), "policy = "), (dict(ok, policy=(packed, 48)), "hidden width of 48"),
             (dict(ok, policy=(_packed(F, 64, 5), 32)), "packed policy must be"), (dict(ok, ticks=0), "0 ticks"),
             (dict(ok, ticks=-3), "-3 ticks"), (dict(ok, outputs=None), "outputs = "),
             (dict(ok, outputs={"reward_sum": outputs["reward_sum"]}), "outputs = "),
             (dict(ok, action_trace=_trace(3, E, N)), "action_trace must be"),          # fewer rows than ticks
             (dict(ok, action_trace=_trace(4, E, N + 1)), "action_trace must be"),
             (dict(ok, action_trace=_trace(4, E * N, 1)), "action_trace must be")]
    cases += [(dict(ok, policy=(t, 32)), "packed policy must be") for t in wrong((n_w,), torch.float32, (n_w - 1,))]
    cases += [(dict(ok, outputs=_outputs(E, N, reward_sum=t)), r"outputs\['reward_sum'\]")
              for t in wrong((E, N), torch.float32, (E * N - 1,))]
    cases += [(dict(ok, outputs=_outputs(E, N, steps=t)), r"outputs\['steps'\]") for t in wrong((E,), torch.int32, (E - 1,))]
    cases += [(dict(ok, outputs=_outputs(E, N, done=t)), r"outputs\['done'\]") for t in wrong((E,), torch.int32, (E - 1,))]
    cases += [(dict(ok, action_trace=t), "action_trace must be") for t in wrong((4, E, N), torch.int32, (4, E, N - 1))[:-1]]
    for extra, what in cases:
        with pytest.raises(UnsupportedRolloutShape, match=what):
            env.evaluate_launch(sampler, **extra)
    # shapes the entries do not serve, each with its reason, stated against the evaluate names
    wide, _ = _stubbed("RendezvousEvaluate", num_agents=520)
    with pytest.raises(UnsupportedRolloutShape, match="576 threads.*wd_env_evaluate.h"):
        wide.evaluate_launch(sampler, (_packed(F, 64, 5), 64), True, _outputs(E, 520), ticks=4)
    pooled, _ = _stubbed("RendezvousEvaluate", pools={"mood": "mood_reset_pool"})
    with pytest.raises(UnsupportedRolloutShape, match="reset pool"):
        pooled.evaluate_launch(sampler, **ok)
    absent, _ = _stubbed("RendezvousEvaluate", missing=["HipRendezvousEvaluateEvaluate_H32"])
    with pytest.raises(UnsupportedRolloutShape, match="HipRendezvousEvaluateEvaluate_H32"):
        absent.evaluate_launch(sampler, **ok)
    multi, _ = _stubbed("RendezvousEvaluate")
    multi.action_space = {a: spaces.MultiDiscrete((5, 5)) for a in range(5)}
    with pytest.raises(UnsupportedRolloutShape, match="MultiDiscrete"):
        multi.evaluate_launch(sampler, **ok)
    unnamed, _ = _stubbed("RendezvousEvaluate")
    unnamed.EVALUATE_KERNEL = None
    assert not unnamed.has_live_policy_evaluate(32, 5)
    with pytest.raises(UnsupportedRolloutShape, match="EVALUATE_KERNEL"):
        unnamed.evaluate_launch(sampler, **ok)
    bare, _ = _stubbed("RendezvousEvaluate")
    bare.cuda_env_resetter = None
    with pytest.raises(UnsupportedRolloutShape, match="resetter"):
        bare.evaluate_launch(sampler, **ok)
    for A in (0, 9):
        with pytest.raises(UnsupportedRolloutShape, match=f"{A} actions"):
            custom_evaluate_launch(env, "HipRendezvousEvaluateEvaluate_H32", env.TICK_STEP_ARGS, sampler, A, packed, 32,
                                   env.cuda_env_resetter, True, outputs, None, 4)
    # nothing was looked up or launched for a refused request ... and a served one still goes through
    for e in (env, wide, pooled, absent, multi, unnamed, bare):
        assert e.cuda_function_manager.initialized == []
        assert e.cuda_env_resetter is None or e.cuda_env_resetter.calls == []
    assert env.evaluate_launch(sampler, **ok)[0].name == "HipRendezvousEvaluateEvaluate_H32"
    assert env.evaluate_launch(sampler, **dict(ok, action_trace=_trace(4, E, N)))[0].name == "HipRendezvousEvaluateEvaluate_H32"


# --------------------------------------------------------------------------------- the GPU cases, on the host alone
def test_the_gpu_cases_cannot_pass_vacuously():
    """every case of tests/test_gpu_custom_env_evaluate.py replayed with the host step, the model and the Philox replay
    alone.  Per case: the flagged decisions within the project's cap; Rendezvous with more than one agent: at least one
    early and one timed finish and two distinct step counts; a sampled case with 50 decisions per action: every action.
    Per kind, action count and mode, all cases together: every action."""
    seen = {}
    for case in model.RENDEZVOUS_CASES + model.PROBE_CASES:
        got = model.simulate(case)
        print(f"{case}: seeds {case.seed} / {case.policy_seed}, spread limit {case.config().get('spread_limit')}, actions "
              f"{got['actions'].tolist()}, steps {got['steps'].tolist()}, {got['early']} early and {got['timed']} timed, "
              f"{got['near']} flagged of {got['decisions']} (cap {case.near_cap(got['decisions'])})")
        assert got["actions"].sum() == got["decisions"] == int(got["steps"].sum()) * case.N
        assert got["near"] <= case.near_cap(got["decisions"]), case
        assert (got["done"] == 1).all() and got["early"] + got["timed"] == case.E, case
        if case.kind == "rendezvous" and case.N > 1:
            assert got["early"] >= 1 and got["timed"] >= 1 and len(set(got["steps"].tolist())) >= 2, case
        if case.kind == "probe":
            assert (got["steps"] == case.L).all() and case.ticks == case.L + 1    # the launch stops at the first done
        if not case.greedy and got["decisions"] >= 50 * case.A:
            assert (got["actions"] > 0).all(), case
        key = (case.kind, case.A, case.mode)
        seen[key] = seen.get(key, 0) + got["actions"]
    for key, counts in seen.items():
        assert (counts > 0).all(), (key, counts.tolist())
    for case in model.SHORT_CASES:                       # `ticks` shorter than the episode: somebody is still running
        got = model.simulate(case)
        assert (got["done"] == 0).any() and (got["steps"][got["done"] == 0] == case.ticks).all(), case
    # the shapes the issue lists, both widths and both modes; the wide one at width 32 only
    shapes = {(c.E, c.N, c.L, c.T, c.hidden, c.mode) for c in model.RENDEZVOUS_CASES}
    assert shapes == {s + (H, m) for s in model.RENDEZVOUS_SHAPES for H in (32, 64) for m in model.MODES} | \
        {model.WIDE_SHAPE + (32, m) for m in model.MODES}
    assert {(c.A, c.N, c.hidden, c.mode) for c in model.PROBE_CASES} == \
        {(A, N, H, m) for A in (1, 2, 8) for N in (1, 5, 70) for H in (32, 64) for m in model.MODES}


def test_the_crafted_policies_are_exact_and_the_preset_epochs_hit_the_ends():
    """the model's probabilities of every crafted policy are exactly 0, 1 / m or 1 / A on observations of both envs' kind,
    the switched policy's winner is the one the helper states, and the listed (row, epoch) pairs draw u == 1.0 and
    u == 2^-24"""
    rng = np.random.RandomState(3)
    for F, A in ((5, 5), (2, 2), (2, 8)):
        obs = (rng.randint(0, 9, size=(64, F)).astype(f32) / f32(8))
        obs[:8, 0] = 0.5
        for H in model.WIDTHS:
            p = model.policy_probabilities(crafted.uniform(F, H, A), H, obs, A)
            assert set(p.reshape(-1).tolist()) == {float(f32(1.0) / f32(A))} and (model.first_maximum(p) == 0).all()
            if A >= 5:
                p = model.policy_probabilities(crafted.constant(F, H, A, (1, 3)), H, obs, A)
                assert set(p.reshape(-1).tolist()) == {0.0, 0.5} and (model.first_maximum(p) == 1).all()
                assert (p[:, [1, 3]] == 0.5).all()
            above, below = (2, 1) if A >= 3 else (0, 1)
            p = model.policy_probabilities(crafted.switched(F, H, A, 0, 0.5, above, below), H, obs, A)
            assert set(p.reshape(-1).tolist()) == {0.0, 0.5, 1.0}
            want = crafted.switched_winner(obs[:, 0], 0.5, above, below)
            assert (model.first_maximum(p) == want).all() and {above, below} == set(want.tolist())
            assert (p[:8, [above, below]] == 0.5).all()
            assert not model.near_top_two(p)[8:][obs[8:, 0] != 0.5].any()
    k0, k1 = tick_model.seed_words(crafted.END_SEED)
    for kind, value in (("hi", 1.0), ("lo", 2.0 ** -24)):
        rows, epochs = (np.array(v, dtype=np.uint32) for v in zip(*crafted.END_DRAWS[kind]))
        u = tick_model.uniform_of(tick_model.tick_bits(rows, epochs, k0, k1, model.TICK_TAG)[:, 0])
        assert (u == f32(value)).all(), (kind, u)
    epochs, roles = crafted.preset_epochs(260, 7)
    assert len(roles) == 7 and {k for k, _ in roles.values()} == {"hi", "lo"} and len({t for _, t in roles.values()}) == 7
    for row, (kind, tick) in roles.items():
        assert model.uniforms_at(crafted.END_SEED, [row], [int(epochs[row]) + tick])[0] == \
            f32(1.0 if kind == "hi" else 2.0 ** -24)
