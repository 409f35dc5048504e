"""The fused tick of a custom environment without a GPU: include/wd_env_tick.h builds with the host compiler and draws
what the numpy model draws, the worked example and the several-heads probe compile to the expected entries without
scratch memory, the host helper packs exactly the kernarg layout the compiled Tick entries declare, and every request
the kit does not serve is refused by name.  hipcc cross-compiles gfx950, so no GPU is needed."""
import hashlib
import os
import re
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from oracle.core_np import seed_words
from tests import custom_tick_model as model
from tests.rendezvous_helpers import EXAMPLE_DIR, ROOT
from warp_drive_amd import build as wd_build

FUSED_DIR = os.path.join(ROOT, "examples", "rendezvous_fused")
FUSED_SOURCE = os.path.join(FUSED_DIR, "rendezvous_fused.hip")
PROBE_SOURCE = os.path.join(ROOT, "tests", "custom_envs", "heads_probe.hip")
FUSED_KERNELS = ["HipRendezvousFusedReset", "HipRendezvousFusedStep", "HipRendezvousFusedTick"]
PROBE_KERNELS = ["HipHeadsProbeStep", "HipHeadsProbeTick"]
TICK_TAG = zlib.crc32(b"tick") & 0x7FFFFFFF


@pytest.fixture(autouse=True)
def cache(tmp_path_factory, monkeypatch):
    path = _cache_dir(tmp_path_factory)
    monkeypatch.setenv("WD_ENV_CACHE", path)
    return path


_CACHE = []


def _cache_dir(tmp_path_factory):
    """one cache directory for the module: each unit compiles once"""
    if not _CACHE:
        _CACHE.append(str(tmp_path_factory.mktemp("env_cache")))
    return _CACHE[0]


def fused_module():
    import importlib.util
    import sys

    name = "rendezvous_fused_example"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(FUSED_DIR, "rendezvous_fused.py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


# ------------------------------------------------------------------------------------------------ the host program
@pytest.fixture(scope="module")
def draw_check(tmp_path_factory):
    """tests/c/tick_draw_check.cpp built with the host compiler alone: no HIP include path, no HIP define"""
    exe = str(tmp_path_factory.mktemp("tick_draw_check") / "tick_draw_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c", "tick_draw_check.cpp"), "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        return [line.split() for line in out.splitlines()]

    return run


SEEDS = (0, 1, 12345, 0x7FFFFFFF)
ROWS = (0, 1, 69, 199999, 2 ** 31 + 5, 2 ** 32 - 1)
# 0, inside and at the end of a group of four, the first of the next, the last epoch and the one after it (it wraps)
EPOCHS = (0, 3, 4, 2 ** 32 - 1, (2 ** 32 - 1 + 1) % 2 ** 32)
TAGS = (0, TICK_TAG, 0x7FFFFFFF)


def test_the_host_build_draws_the_models_uniforms(draw_check):
    grid = [(s, r, e, t) for s in SEEDS for r in ROWS for e in EPOCHS for t in TAGS]
    lines = []
    for seed, row, epoch, tag in grid:
        k0, k1 = seed_words(seed)
        lines.append(f"D {k0} {k1} {row} {epoch} {tag}")
    got = draw_check(lines)
    assert len(got) == len(grid)
    for (seed, row, epoch, tag), out in zip(grid, got):
        k0, k1 = seed_words(seed)
        bits = model.tick_bits([row], [epoch], k0, k1, tag)[0]
        want = [int(b) for b in bits] + [int(b) for b in model.uniform_of(bits).view(np.uint32)]
        assert out[0] == "D" and [int(v) for v in out[1:]] == want, (seed, row, epoch, tag)
    # the uniforms lie in (0, 1]; the epoch after the last one is epoch 0 again, as uint32 arithmetic says
    u = model.uniform_of(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint32))
    assert u.tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]
    draws = model.TickDraws(12345, 1, 1, TICK_TAG)
    draws.epochs[:] = 2 ** 32 - 1
    p = [np.full((1, 1, 5), 0.2, dtype=np.float32)]
    first, second = draws.draw(p), draws.draw(p)
    assert draws.epochs.tolist() == [1]
    k0, k1 = seed_words(12345)
    row_bits = " ".join(str(int(b)) for b in p[0].reshape(-1).view(np.uint32))
    got = draw_check([f"P 0 {k0} {k1} 0 {e} {TICK_TAG} 5 {row_bits}" for e in (2 ** 32 - 1, 0)])
    assert [int(g[1]) for g in got] == [int(first[0, 0, 0]), int(second[0, 0, 0])]


def _pick_rows():
    rng = np.random.RandomState(7)
    f = np.float32
    rows = {"single action": np.ones(1, dtype=f), "uniform": np.full(5, 0.2, dtype=f),
            "71 actions": rng.dirichlet(np.ones(71)).astype(f),
            "leading zeros": np.array([0, 0, 0.25, 0.5, 0.25], dtype=f),
            "trailing zeros": np.array([0.5, 0.25, 0.25, 0, 0, 0], dtype=f),
            "zeros at both ends": np.array([0, 0.75, 0, 0.25, 0], dtype=f),
            "short of one": np.array([0.25, 0.25, 0.25], dtype=f)}  # the clamp: u may lie above every prefix sum
    for hot in (0, 3, 6):
        rows[f"one-hot at {hot}"] = np.eye(7, dtype=f)[hot]
    return rows


def test_the_host_build_picks_the_models_actions(draw_check):
    rows = _pick_rows()
    cases = [(name, head, seed, row, epoch, tag) for name in rows for head in range(4) for seed in (0, 12345)
             for row in (0, 69, 2 ** 31 + 5) for epoch in EPOCHS for tag in (TICK_TAG,)]
    lines = []
    for name, head, seed, row, epoch, tag in cases:
        k0, k1 = seed_words(seed)
        p = rows[name]
        lines.append(f"P {head} {k0} {k1} {row} {epoch} {tag} {len(p)} " + " ".join(str(int(b)) for b in p.view(np.uint32)))
    got = draw_check(lines)
    assert len(got) == len(cases)
    seen = {name: set() for name in rows}
    for (name, head, seed, row, epoch, tag), out in zip(cases, got):
        k0, k1 = seed_words(seed)
        u = model.uniform_of(model.tick_bits([row], [epoch], k0, k1, tag)[0, head])
        want = int(model.pick(rows[name], u))
        assert out[0] == "P" and int(out[1]) == want, (name, head, seed, row, epoch)
        seen[name].add(want)
    # the rows do what they are there for
    assert seen["single action"] == {0} and all(seen[f"one-hot at {h}"] == {h} for h in (0, 3, 6))
    assert seen["leading zeros"] <= {2, 3, 4} and seen["trailing zeros"] <= {0, 1, 2}
    assert seen["zeros at both ends"] <= {1, 3} and len(seen["zeros at both ends"]) == 2
    assert 2 in seen["short of one"] and len(seen["71 actions"]) > 20


def test_reset_entry_layout_is_the_hosts(draw_check):
    """24 bytes, fields at 0 / 8 / 16: what HIPEnvironmentReset._build_table writes"""
    from warp_drive_amd.managers.function_manager import HIPEnvironmentReset

    assert draw_check(["L"]) == [["L", "24", "0", "8", "16"]]
    source = open(os.path.join(ROOT, "warp_drive_amd", "managers", "function_manager.py")).read()
    assert '[("data", "<u8"), ("ref", "<u8"), ("row", "<i4"), ("pad", "<i4")]' in source
    dtype = np.dtype([("data", "<u8"), ("ref", "<u8"), ("row", "<i4"), ("pad", "<i4")])
    assert dtype.itemsize == 24 and [dtype.fields[k][1] for k in ("data", "ref", "row")] == [0, 8, 16]
    assert hasattr(HIPEnvironmentReset, "_build_table")


def test_the_header_is_self_contained():
    text = open(os.path.join(ROOT, "include", "wd_env_tick.h")).read()
    assert set(re.findall(r"^\s*#include\s+(\S+)", text, re.M)) == {"<hip/hip_runtime.h>", "<stdint.h>", '"wd_env.h"'}
    assert "asm" not in re.sub(r"//.*", "", text) and "atomic" not in re.sub(r"//.*", "", text).lower()


# ------------------------------------------------------------------------------------------------------ the build
def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest() if os.path.exists(path) else None


def _metadata(hsaco):
    """{kernel: {"private", "vgpr_spills", "sgpr_spills", "lds", "vgprs", "args": [(offset, size, kind), ...]}} from the
    code object's notes"""
    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "env.elf")
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={hsaco}", f"--output={elf}"],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                               text=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        name = re.search(r"^\s{4}\.name:\s+(\S+)$", block, re.M)
        if name is None:
            continue
        field = lambda key: int(re.search(r"^\s{4}\." + key + r":\s+(\d+)$", block, re.M).group(1))  # noqa: E731
        args = [(int(o), int(s), k) for o, s, k in
                re.findall(r"\.offset:\s+(\d+)\s+\.size:\s+(\d+)\s+\.value_kind:\s+(\S+)", block)]
        out[name.group(1)] = {"private": field("private_segment_fixed_size"), "vgpr_spills": field("vgpr_spill_count"),
                              "sgpr_spills": field("sgpr_spill_count"), "lds": field("group_segment_fixed_size"),
                              "vgprs": field("vgpr_count"), "args": args}
    return out


@pytest.mark.parametrize("name,source,kernels,tick", [("RendezvousFused", FUSED_SOURCE, FUSED_KERNELS, "HipRendezvousFusedTick"),
                                                      ("HeadsProbe", PROBE_SOURCE, PROBE_KERNELS, "HipHeadsProbeTick")])
def test_the_units_build_to_the_expected_entries_without_scratch(cache, name, source, kernels, tick):
    manifest_before = _sha(wd_build.MANIFEST)
    in_tree_before = sorted(os.listdir(wd_build.CSRC))
    path = wd_build.build_env_unit(name, source)
    assert os.path.dirname(path) == cache and wd_build.kernels_in(path) == kernels
    assert _sha(wd_build.MANIFEST) == manifest_before and sorted(os.listdir(wd_build.CSRC)) == in_tree_before
    # the header is one of the unit's sources: an edit of it gives another object
    assert os.path.join(ROOT, "include", "wd_env_tick.h") in wd_build.unit_sources(source, [os.path.join(ROOT, "include")])
    meta = _metadata(path)
    assert sorted(meta) == kernels
    for kernel, m in meta.items():
        print(f"{kernel}: {m['vgprs']} VGPRs, private {m['private']}, spills {m['vgpr_spills']} / {m['sgpr_spills']}, "
              f"static LDS {m['lds']}")
        assert (m["private"], m["vgpr_spills"], m["sgpr_spills"]) == (0, 0, 0), kernel
        assert m["vgprs"] <= 64  # a block of 1024 threads: 16 wavefronts on 4 SIMDs
    assert tick in meta


def test_the_fused_example_is_not_part_of_the_in_tree_build_and_the_old_example_is_as_it_was():
    assert not any("rendezvous" in unit.lower() or "heads_probe" in unit.lower() for unit, _ in wd_build.UNITS.values())
    owners = wd_build.in_tree_kernel_owners()
    assert not [k for k in FUSED_KERNELS + PROBE_KERNELS if k in owners]
    # examples/rendezvous/ is what the parent commit has: two kernels, no Tick entry
    old = wd_build.build_env_unit("Rendezvous", os.path.join(EXAMPLE_DIR, "rendezvous_step.hip"))
    assert wd_build.kernels_in(old) == ["HipRendezvousReset", "HipRendezvousStep"]
    assert sorted(f for f in os.listdir(EXAMPLE_DIR) if f != "__pycache__") == ["rendezvous.py", "rendezvous_step.hip"]
    assert "wd_env_tick.h" not in open(os.path.join(EXAMPLE_DIR, "rendezvous_step.hip")).read()


# ------------------------------------------------------------------------------------- the helper against the header
class _Fn:
    def __init__(self, name):
        self.name = name


class _StubFunctions:
    grid = (3, 1)

    def __init__(self):
        self.initialized = []

    def initialize_functions(self, names):
        self.initialized += list(names)

    def get_function(self, name):
        return _Fn(name)


class _StubData:
    """device arrays are addresses, scalars numpy scalars of their own width, as the data manager hands them out"""

    def __init__(self, scalars):
        self.scalars = scalars
        self.next = 0x10000

    def device_data(self, name):
        from warp_drive_amd.managers import hip_driver as drv

        if name in self.scalars:
            return self.scalars[name]
        self.next += 0x1000
        return drv.DevicePtr(self.next)

    def meta_info(self, name):
        return np.int32({"n_agents": 5, "episode_length": 4, "n_envs": 3}[name])


class _StubSampler:
    def __init__(self):
        from warp_drive_amd.managers import hip_driver as drv

        self.rng_state = drv.DevicePtr(0x7000)


class _StubResetter:
    def __init__(self):
        self.calls = []

    def fused_launch(self, dm, force_reset, undo):
        from warp_drive_amd.managers import hip_driver as drv

        self.calls.append((force_reset, undo))
        return _Fn("reset_when_done_fused"), (drv.DevicePtr(0x9000), np.int32(3)), (256, 1, 1), (3, 1)


def _stubbed(env, scalars):
    """the env with the device side stubbed (no code object is loaded, nothing is launched)"""
    from warp_drive_amd.managers.function_manager import CUDAFunctionFeed

    env.cuda_function_manager = _StubFunctions()
    env.cuda_data_manager = _StubData(scalars)
    env.cuda_step_function_feed = CUDAFunctionFeed(env.cuda_data_manager)
    return env


def _probabilities(E, N, sizes):
    import torch

    return [torch.full((E, N, a), 1.0 / a, dtype=torch.float32) for a in sizes]


def _stubbed_fused(**config):
    env = fused_module().RendezvousFused(**dict(dict(num_agents=5, grid_length=4, episode_length=4), **config))
    return _stubbed(env, {"wall_penalty": np.float32(0.125), "spread_limit": np.int32(-1), "grid_length": np.int32(4)})


def _stubbed_probe(head_sizes):
    from tests.custom_envs.heads_probe import HeadsProbe

    return _stubbed(HeadsProbe(num_agents=5, episode_length=4, head_sizes=head_sizes), {"n_heads": np.int32(len(head_sizes))})


@pytest.mark.parametrize("which,head_sizes", [("fused", (5,)), ("probe", (3,)), ("probe", (2, 7)), ("probe", (4, 1, 9, 71))])
def test_the_helper_packs_the_kernarg_layout_of_the_compiled_tick_entry(which, head_sizes):
    from warp_drive_amd.managers import hip_driver as drv

    if which == "fused":
        env, source, unit, tick = _stubbed_fused(), FUSED_SOURCE, "RendezvousFused", "HipRendezvousFusedTick"
    else:
        env, source, unit, tick = _stubbed_probe(head_sizes), PROBE_SOURCE, "HeadsProbe", "HipHeadsProbeTick"
    assert env.TICK_HEADS == len(head_sizes)
    explicit = [a for a in _metadata(wd_build.build_env_unit(unit, source))[tick]["args"] if not a[2].startswith("hidden_")]
    kernarg_bytes = max(o + s for o, s, _ in explicit)
    resetter = _StubResetter()
    for launch, ticks in ((env.tick_launch, 1), (env.rollout_launch, 1)):
        fn, args, block, grid, shared = launch(_StubSampler(), _probabilities(3, 5, head_sizes), resetter)
        assert fn.name == tick and block == (64, 1, 1) and grid == (3, 1) and shared == 0
        assert isinstance(args[-1], np.int32) and int(args[-1]) == ticks
        packed = drv._pack_args(args)
        assert len(packed) == kernarg_bytes, (len(packed), kernarg_bytes)
        assert packed[-4:] == np.int32(ticks).tobytes()
        # argument by argument: an 8-byte pointer where the entry declares a buffer, 4 bytes where it takes a value
        offset, layout = 0, []
        for a in args:
            size = 8 if isinstance(a, drv.DevicePtr) or hasattr(a, "data_ptr") else a.dtype.itemsize
            offset += (-offset) % size
            layout.append((offset, size))
            offset += size
        assert layout == [(o, s) for o, s, _ in explicit]
        kinds = ["global_buffer" if s == 8 else "by_value" for _, s in layout]
        assert kinds == [k for _, _, k in explicit]
    assert env.cuda_function_manager.initialized == [tick, tick] and resetter.calls == [(0, 0), (0, 0)]
    # the kit's trailing arguments, in the header's order
    from warp_drive_amd.utils.custom_tick import custom_tick_launch

    probs = _probabilities(3, 5, head_sizes)
    _, args, _, _, _ = custom_tick_launch(env, tick, env.TICK_STEP_ARGS, _StubSampler(), probs, resetter, ticks=7)
    tail = args[len(env.TICK_STEP_ARGS):]
    H = len(head_sizes)
    assert int(tail[0]) == 0x7000 and int(tail[1]) == H
    assert [t.data_ptr() for t in tail[2:2 + H]] == [p.data_ptr() for p in probs]
    assert all(isinstance(t, np.uint64) and int(t) == 0 for t in tail[2 + H:6])
    assert [int(v) for v in tail[6:10]] == list(head_sizes) + [0] * (4 - H)
    assert int(tail[10]) == 0x9000 and int(tail[11]) == 3 and int(tail[12]) == TICK_TAG and int(tail[13]) == 7
    assert len(tail) == 14 and isinstance(tail[13], np.int32)


# ------------------------------------------------------------------------------------------------------ refusals
def test_every_request_the_kit_does_not_serve_is_refused_by_name():
    from tests.custom_envs.heads_probe import HeadsProbe
    from warp_drive_amd.rollout import UnsupportedRolloutShape
    from warp_drive_amd.utils import spaces

    env, sampler, resetter = _stubbed_fused(), _StubSampler(), _StubResetter()
    probs = _probabilities(3, 5, (5,))
    cases = [(dict(env_range=(0, 2)), "replica range"), (dict(batch={"obs": None}), "batch"),
             (dict(policy=(None, 32)), "in-kernel policy"), (dict(actor=(None, 32, 1.0, 0.0)), "in-kernel actor"),
             (dict(ou_params=(0.15, 0.2, 1.0)), "Box action space")]
    for extra, what in cases:
        with pytest.raises(UnsupportedRolloutShape, match=what):
            env.tick_launch(sampler, probs, resetter, **extra)
    with pytest.raises(UnsupportedRolloutShape, match="presampled actions"):
        env.tick_launch(sampler, None, resetter)
    assert env.has_presampled_tick() is False
    box = _stubbed_fused()
    box.action_space = {a: spaces.Box(low=-1.0, high=1.0, shape=(1,), dtype=np.float32) for a in range(5)}
    with pytest.raises(UnsupportedRolloutShape, match="Box action space"):
        box.tick_launch(sampler, _probabilities(3, 5, (1,)), resetter)
    five = _stubbed(HeadsProbe(num_agents=5, episode_length=4, head_sizes=(2, 2, 2, 2, 2)), {"n_heads": np.int32(5)})
    assert five.TICK_HEADS == 5
    with pytest.raises(UnsupportedRolloutShape, match="5 action heads"):
        five.tick_launch(sampler, _probabilities(3, 5, (2, 2, 2, 2, 2)), resetter)
    # nothing was looked up or launched for a refused request ... and a served one still goes through
    assert env.cuda_function_manager.initialized == [] and resetter.calls == []
    assert env.tick_launch(sampler, probs, resetter)[0].name == "HipRendezvousFusedTick"
    # the kit does not claim reset pools: RolloutEngine keeps the per-tick plan for an env that has one
    assert not getattr(env, "TICK_POOL_RESET", False) and not getattr(env, "TICK_ENV_RANGES", False)
