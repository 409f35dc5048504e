"""The one-launch rollout of a custom environment without a GPU: the host-buildable half of include/wd_env_rollout.h
computes what the numpy model computes, the worked example and the probe compile to the expected entries without scratch
memory and with the launch bounds the host admits blocks by, the host helper packs exactly the kernarg layout the compiled
Rollout entries declare, every request the kit does not serve is refused by name, and the cases of the GPU test -- replayed
here on the host alone -- have the coverage they are meant to have.  hipcc cross-compiles gfx950, so no GPU is needed."""
import hashlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import custom_rollout_model as model
from tests.classic_control_cases import NEAR_WINDOW, near_threshold
from tests.classic_control_policy import count_below
from tests.rendezvous_helpers import ROOT
from warp_drive_amd import build as wd_build

POLICY_KERNELS = ["HipRendezvousPolicyRollout_H32", "HipRendezvousPolicyRollout_H64", "HipRendezvousPolicyStep",
                  "HipRendezvousPolicyTick"]
PROBE_KERNELS = ["HipPolicyProbeRollout_H32", "HipPolicyProbeRollout_H64", "HipPolicyProbeStep", "HipPolicyProbeTick"]
UNITS = {"RendezvousPolicy": (model.POLICY_SOURCE, POLICY_KERNELS, "HipRendezvousPolicy"),
         "PolicyProbe": (model.PROBE_SOURCE, PROBE_KERNELS, "HipPolicyProbe")}
HEADER = os.path.join(ROOT, "include", "wd_env_rollout.h")

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
def policy_check(tmp_path_factory):
    """tests/c/rollout_policy_check.cpp built with the host compiler alone: no HIP include path, no HIP define"""
    exe = str(tmp_path_factory.mktemp("rollout_policy_check") / "rollout_policy_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "c", "rollout_policy_check.cpp"), "-o", exe], check=True)

    def run(H, F, A, packed, obs, u):
        words = lambda v: " ".join(str(int(b)) for b in np.ascontiguousarray(v, dtype=np.float32).reshape(-1).view(np.uint32))  # noqa: E731
        lines = [f"{H} {F} {A} {len(obs)}", words(packed)] + [f"{words(o)} {words(x)}" for o, x in zip(obs, u)]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
        rows = [line.split() for line in out.splitlines()]
        assert len(rows) == len(obs) and all(r[0] == "R" and len(r) == 2 + 2 * A for r in rows)
        table = np.array([[int(v) for v in r[1:]] for r in rows], dtype=np.int64)
        return (table[:, :A].astype(np.uint32).view(np.float32), table[:, A:2 * A].astype(np.uint32).view(np.float32),
                table[:, 2 * A].astype(np.int32))

    return run


@pytest.mark.parametrize("H,F,A", [(32, 5, 5), (64, 5, 5), (32, 2, 1), (32, 2, 8), (64, 2, 2)])
def test_the_host_build_computes_the_models_policy(policy_check, H, F, A):
    """300 seeded rows: observations in [0, 1] (what both envs produce), uniforms in (0, 1], the last row's exactly 1.0
    (the clamp).  Logits bit for bit; running sums within NEAR_WINDOW (the two sides call different expf); picks equal
    wherever near_threshold does not flag the row, the flagged rows under near_cap's rule."""
    R = 300
    _, packed = model.make_policy(F, A, H)
    assert packed.size == model.policy_floats(F, H, A)
    rng = np.random.RandomState(1000 * H + 10 * F + A)
    obs = rng.randint(0, 13, size=(R, F)).astype(np.float32) / np.float32(12)
    u = ((rng.randint(0, 2 ** 24, size=R).astype(np.uint32) + np.uint32(1)).astype(np.float32) * np.float32(2.0 ** -24))
    u[-1] = 1.0
    logits, cum, picks = policy_check(H, F, A, packed, obs, u)
    want_logits = model.policy_logits(packed, H, obs, A)
    assert logits.tobytes() == want_logits.tobytes(), np.argwhere(logits != want_logits)[:5].tolist()
    want_cum = model.model_sums(packed, H, obs, A)
    worst = float(np.abs(cum.astype(np.float64) - want_cum.astype(np.float64)).max())
    print(f"H {H} F {F} A {A}: largest difference of a running sum {worst:.3g}")
    assert worst < NEAR_WINDOW
    near = near_threshold(want_cum, u)
    want_picks = count_below(want_cum, u)
    assert (picks[~near] == want_picks[~near]).all()
    assert int(near.sum()) <= model.near_cap(R, A)
    assert picks.min() >= 0 and picks.max() <= A - 1 and picks[-1] == want_picks[-1]
    if A > 1:
        assert len(set(picks.tolist())) > 1


def test_the_header_is_self_contained_and_holds_its_limits():
    text = open(HEADER).read()
    assert set(re.findall(r"^\s*#include\s+(\S+)", text, re.M)) == {"<hip/hip_runtime.h>", "<stdint.h>", "<math.h>",
                                                                    '"wd_env_tick.h"'}
    code = re.sub(r"//.*", "", text)
    assert "asm" not in code and "atomic" not in code.lower() and "shfl" not in code and "csrc" not in code
    # the packed layout's size, as the host helper and the model state it
    from warp_drive_amd.utils.custom_tick import rollout_policy_floats

    for F, H, A in ((5, 32, 5), (2, 64, 8), (6, 32, 1)):
        assert rollout_policy_floats(F, H, A) == model.policy_floats(F, H, A) == F * H + H + H * H + H + A * H + A


# ------------------------------------------------------------------------------------------------------ the build
def _sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest() if os.path.exists(path) else None


def _metadata(hsaco):
    """{kernel: {"private", "vgpr_spills", "sgpr_spills", "lds", "vgprs", "max_threads", "args": [(offset, size, kind)]}}
    from the code object's notes"""
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
                              "vgprs": field("vgpr_count"), "max_threads": field("max_flat_workgroup_size"), "args": args}
    return out


def _env_class(unit):
    if unit == "RendezvousPolicy":
        return model.policy_module().RendezvousPolicy
    from tests.custom_envs.policy_probe import PolicyProbe

    return PolicyProbe


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_the_units_build_to_the_expected_entries_without_scratch(cache, unit):
    source, kernels, prefix = UNITS[unit]
    manifest_before = _sha(wd_build.MANIFEST)
    in_tree_before = sorted(os.listdir(wd_build.CSRC))
    path = wd_build.build_env_unit(unit, source)
    assert os.path.dirname(path) == cache and wd_build.kernels_in(path) == kernels
    assert _sha(wd_build.MANIFEST) == manifest_before and sorted(os.listdir(wd_build.CSRC)) == in_tree_before
    sources = wd_build.unit_sources(source, [os.path.join(ROOT, "include")])
    assert HEADER in sources and os.path.join(ROOT, "include", "wd_env_tick.h") in sources
    meta = _metadata(path)
    assert sorted(meta) == kernels
    cls = _env_class(unit)
    for kernel, m in meta.items():
        print(f"{kernel}: {m['vgprs']} VGPRs, private {m['private']}, spills {m['vgpr_spills']} / {m['sgpr_spills']}, "
              f"static LDS {m['lds']}, at most {m['max_threads']} threads")
        assert (m["private"], m["vgpr_spills"], m["sgpr_spills"]) == (0, 0, 0), kernel
    for width in (32, 64):
        entry = meta[cls.ROLLOUT_KERNEL.format(width=width)]
        assert entry["max_threads"] == cls.ROLLOUT_MAX_THREADS[width]
        assert entry["vgprs"] <= 512 // (cls.ROLLOUT_MAX_THREADS[width] // 256)  # the lanes' share of a SIMD's 512
    assert cls.TICK_KERNEL == prefix + "Tick" and cls.ROLLOUT_POLICY_WIDTHS == (32, 64)
    # the Tick entry is round 34's kit, unchanged: the step's arguments + 14 trailing ones
    explicit = [a for a in meta[cls.TICK_KERNEL]["args"] if not a[2].startswith("hidden_")]
    assert len(explicit) == len(cls.TICK_STEP_ARGS) + 14


def test_the_new_units_are_not_part_of_the_in_tree_build_and_the_old_examples_are_as_they_were():
    assert not any("rendezvous" in unit.lower() or "probe" in unit.lower() for unit, _ in wd_build.UNITS.values())
    owners = wd_build.in_tree_kernel_owners()
    assert not [k for k in POLICY_KERNELS + PROBE_KERNELS if k in owners]
    for folder, files in (("rendezvous", ["rendezvous.py", "rendezvous_step.hip"]),
                          ("rendezvous_fused", ["rendezvous_fused.hip", "rendezvous_fused.py"]),
                          ("rendezvous_policy", ["rendezvous_policy.hip", "rendezvous_policy.py"])):
        here = os.path.join(ROOT, "examples", folder)
        assert sorted(f for f in os.listdir(here) if f != "__pycache__") == files
    for name in ("rendezvous/rendezvous_step.hip", "rendezvous_fused/rendezvous_fused.hip"):
        assert "wd_env_rollout.h" not in open(os.path.join(ROOT, "examples", name)).read()
    for name in ("wd_env.h", "wd_env_tick.h"):
        assert "rollout.h" not in open(os.path.join(ROOT, "include", name)).read()


# ------------------------------------------------------------------------------------- the helper against the header
class _Fn:
    def __init__(self, name):
        self.name = name


class _StubFunctions:
    grid = (3, 1)

    def __init__(self, missing=()):
        self.initialized, self.missing = [], set(missing)

    def initialize_functions(self, names):
        self.initialized += list(names)

    def get_function(self, name):
        return _Fn(name)

    def has_function(self, name):
        return name not in self.missing


class _StubData:
    """device arrays are addresses, scalars numpy scalars of their own width, as the data manager hands them out"""

    def __init__(self, scalars, n_agents, obs_size, pools=None):
        self.scalars, self.n_agents, self.obs_size = scalars, n_agents, obs_size
        self.reset_target_to_pool = dict(pools or {})
        self.next = 0x10000

    def device_data(self, name):
        from warp_drive_amd.managers import hip_driver as drv

        if name in self.scalars:
            return self.scalars[name]
        self.next += 0x1000
        return drv.DevicePtr(self.next)

    def meta_info(self, name):
        return np.int32({"n_agents": self.n_agents, "episode_length": 4, "n_envs": 3}[name])

    def get_shape(self, name):
        assert name == "observations"
        return (3, self.n_agents, self.obs_size)


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


class _DeviceTensor:
    """what the helper asks of a CUDA tensor, without a device"""
    is_cuda = True

    def __init__(self, shape, dtype, ptr, contiguous=True, cuda=True):
        self.shape, self.dtype, self.ptr, self.contiguous, self.is_cuda = tuple(shape), dtype, ptr, contiguous, cuda

    def numel(self):
        return int(np.prod(self.shape))

    def is_contiguous(self):
        return self.contiguous

    def data_ptr(self):
        return self.ptr


def _stubbed(unit, num_agents=5, pools=None, missing=(), **config):
    """the env with the device side stubbed (no code object is loaded, nothing is launched)"""
    from warp_drive_amd.managers.function_manager import CUDAFunctionFeed

    if unit == "RendezvousPolicy":
        env = _env_class(unit)(**dict(dict(num_agents=num_agents, grid_length=4, episode_length=4), **config))
        scalars, F = {"wall_penalty": np.float32(0.125), "spread_limit": np.int32(-1), "grid_length": np.int32(4)}, 5
    else:
        env = _env_class(unit)(**dict(dict(num_agents=num_agents, episode_length=4), **config))
        scalars, F = {}, 2
    env.cuda_function_manager = _StubFunctions(missing)
    env.cuda_data_manager = _StubData(scalars, num_agents, F, pools)
    env.cuda_step_function_feed = CUDAFunctionFeed(env.cuda_data_manager)
    return env, F


def _batch(E, N, F, rows, **other):
    import torch

    spec = {"obs": ((rows, E, N, F), torch.float32, 0xA0000), "actions": ((rows, E, N, 1), torch.int32, 0xB0000),
            "rewards": ((rows, E, N), torch.float32, 0xC0000), "done": ((rows, E), torch.int32, 0xD0000)}
    batch = {k: _DeviceTensor(*v) for k, v in spec.items()}
    batch.update(other)
    return batch


def _packed(F, H, A, **kw):
    import torch

    return _DeviceTensor((model.policy_floats(F, H, A),), torch.float32, 0xE0000, **kw)


@pytest.mark.parametrize("unit,A,width,ticks", [("RendezvousPolicy", 5, 32, 1), ("RendezvousPolicy", 5, 64, 7),
                                                ("PolicyProbe", 1, 32, 3), ("PolicyProbe", 8, 64, 5)])
def test_the_helper_packs_the_kernarg_layout_of_the_compiled_rollout_entry(unit, A, width, ticks):
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.utils.custom_tick import custom_rollout_launch

    env, F = _stubbed(unit, **({"n_actions": A} if unit == "PolicyProbe" else {}))
    entry = env.ROLLOUT_KERNEL.format(width=width)
    explicit = [a for a in _metadata(wd_build.build_env_unit(unit, UNITS[unit][0]))[entry]["args"]
                if not a[2].startswith("hidden_")]
    kernarg_bytes = max(o + s for o, s, _ in explicit)
    assert env.has_live_policy_rollout(width, A)
    resetter, sampler = _StubResetter(), _StubSampler()
    batch, packed = _batch(3, 5, F, ticks + 1), _packed(F, width, A)
    env.ticks_per_launch = ticks   # (what RolloutEngine sets around the call)
    fn, args, block, grid, shared = env.tick_launch(sampler, [None], resetter, batch=batch, policy=(packed, width))
    n_w = model.policy_floats(F, width, A)
    assert fn.name == entry and block == (64, 1, 1) and grid == (3, 1)
    assert shared == (4 * n_w + 15) // 16 * 16 and shared % 16 == 0 and 0 <= shared - 4 * n_w < 16
    assert isinstance(args[-1], np.int32) and int(args[-1]) == ticks
    blob = drv._pack_args(args)
    assert len(blob) == kernarg_bytes, (len(blob), kernarg_bytes)
    assert blob[-4:] == np.int32(ticks).tobytes()
    # argument by argument: an 8-byte pointer where the entry declares a buffer, 4 bytes where it takes a value
    offset, layout = 0, []
    for a in args:
        size = 8 if isinstance(a, drv.DevicePtr) or hasattr(a, "data_ptr") else a.dtype.itemsize
        offset += (-offset) % size
        layout.append((offset, size))
        offset += size
    assert layout == [(o, s) for o, s, _ in explicit]
    assert ["global_buffer" if s == 8 else "by_value" for _, s in layout] == [k for _, _, k in explicit]
    assert env.cuda_function_manager.initialized == [entry] and resetter.calls == [(0, 0)]
    # the kit's trailing arguments, in the header's order
    tail = args[len(env.TICK_STEP_ARGS):]
    assert len(tail) == 11 and int(tail[0]) == 0x7000 and tail[1] is packed and int(tail[2]) == A
    assert int(tail[3]) == 0x9000 and int(tail[4]) == 3 and int(tail[5]) == model.TICK_TAG
    assert [t.data_ptr() for t in tail[6:10]] == [0xA0000, 0xB0000, 0xC0000, 0xD0000] and int(tail[10]) == ticks
    # the function underneath gives the same launch
    again = custom_rollout_launch(env, entry, env.TICK_STEP_ARGS, sampler, A, packed, width, resetter, batch, ticks)
    assert drv._pack_args(again[1]) == blob and again[2:] == (block, grid, shared)
    # with neither batch nor policy it is the parent's tick, on the Tick entry
    import torch

    probs = [torch.full((3, 5, A), 1.0 / A, dtype=torch.float32)]
    assert env.tick_launch(sampler, probs, resetter)[0].name == env.TICK_KERNEL
    assert env.rollout_launch(sampler, probs, resetter)[0].name == env.TICK_KERNEL


# ------------------------------------------------------------------------------------------------------ admission
def test_the_host_admits_only_what_the_entries_serve():
    from warp_drive_amd.utils import spaces

    env, _ = _stubbed("RendezvousPolicy")
    assert env.has_live_policy_rollout(32, 5) and env.has_live_policy_rollout(64, 5)
    assert env.ROLLOUT_POLICY_OPT_IN is True and env.ticks_per_launch == 1 and env.ROLLOUT_POLICY_WIDTHS == (32, 64)
    assert not env.has_live_policy_rollout(48, 5) and not env.has_live_policy_rollout(128, 5)
    assert not env.has_live_policy_rollout(32, 0) and not env.has_live_policy_rollout(32, 9)
    assert env.has_live_policy_rollout(32, 1) and env.has_live_policy_rollout(32, 8)
    multi, _ = _stubbed("RendezvousPolicy")
    multi.action_space = {a: spaces.MultiDiscrete((5, 5)) for a in range(5)}
    assert not multi.has_live_policy_rollout(32, 5)
    box, _ = _stubbed("RendezvousPolicy")
    box.action_space = {a: spaces.Box(low=-1.0, high=1.0, shape=(1,), dtype=np.float32) for a in range(5)}
    assert not box.has_live_policy_rollout(32, 1)
    wide, _ = _stubbed("RendezvousPolicy", num_agents=520)   # a block of 576 threads
    assert wide.has_live_policy_rollout(32, 5) and not wide.has_live_policy_rollout(64, 5)
    edge, _ = _stubbed("RendezvousPolicy", num_agents=512)
    assert edge.has_live_policy_rollout(64, 5)
    pooled, _ = _stubbed("RendezvousPolicy", pools={"mood": "mood_reset_pool"})
    assert not pooled.has_live_policy_rollout(32, 5)
    absent, _ = _stubbed("RendezvousPolicy", missing=["HipRendezvousPolicyRollout_H64"])
    assert absent.has_live_policy_rollout(32, 5) and not absent.has_live_policy_rollout(64, 5)


def test_every_request_the_rollout_does_not_serve_is_refused_by_name():
    import torch

    from warp_drive_amd.rollout import UnsupportedRolloutShape
    from warp_drive_amd.utils.custom_tick import custom_rollout_launch

    env, F = _stubbed("RendezvousPolicy")
    sampler, resetter = _StubSampler(), _StubResetter()
    batch, packed = _batch(3, 5, F, 4), _packed(F, 32, 5)
    env.ticks_per_launch = 4
    ok = dict(batch=batch, policy=(packed, 32))
    cases = [(dict(ok, env_range=(0, 2)), "replica range"), (dict(batch=batch), "without an in-kernel policy"),
             (dict(policy=(packed, 32)), "without the batch tensors"),
             (dict(ok, actor=(None, 32, 1.0, 0.0)), "in-kernel actor"), (dict(ok, mean_batch=None), "record of means"),
             (dict(ok, ou_params=(0.15, 0.2, 1.0)), "Box action space"), (dict(ok, cohort=3), "'cohort'"),
             (dict(batch=batch, policy=packed), "policy = "), (dict(batch=batch, policy=(packed, 48)), "hidden width of 48"),
             (dict(batch=batch, policy=(_packed(F, 64, 5), 32)), "packed policy must be"),
             (dict(batch=batch, policy=(_packed(F, 32, 5, contiguous=False), 32)), "packed policy must be"),
             (dict(batch=batch, policy=(_packed(F, 32, 5, cuda=False), 32)), "packed policy must be"),
             (dict(batch=_batch(3, 5, F, 3), policy=(packed, 32)), r"batch\['obs'\]"),
             (dict(batch=_batch(3, 5, F, 4, rewards=_DeviceTensor((4, 3, 5, 1), torch.float32, 1)), policy=(packed, 32)),
              r"batch\['rewards'\]"),
             (dict(batch=_batch(3, 5, F, 4, actions=_DeviceTensor((4, 3, 5, 1), torch.float32, 1)), policy=(packed, 32)),
              r"batch\['actions'\]"),
             (dict(batch=_batch(3, 5, F, 4, done=_DeviceTensor((4, 3), torch.int32, 1, contiguous=False)),
                   policy=(packed, 32)), r"batch\['done'\]"),
             (dict(batch=_batch(3, 5, F, 4, obs=_DeviceTensor((4, 3, 5, 6), torch.float32, 1)), policy=(packed, 32)),
              r"batch\['obs'\]")]
    for extra, what in cases:
        with pytest.raises(UnsupportedRolloutShape, match=what):
            env.tick_launch(sampler, [None], resetter, **extra)
    # the parent's refusals are the parent's
    probs = [torch.full((3, 5, 5), 0.2, dtype=torch.float32)]
    for extra, what in ((dict(env_range=(0, 2)), "replica range"), (dict(actor=(None, 32, 1.0, 0.0)), "in-kernel actor"),
                        (dict(ou_params=(0.15, 0.2, 1.0)), "Box action space"), (dict(mean_batch=None), "record of means")):
        with pytest.raises(UnsupportedRolloutShape, match=what):
            env.tick_launch(sampler, probs, resetter, **extra)
    with pytest.raises(UnsupportedRolloutShape, match="presampled actions"):
        env.tick_launch(sampler, None, resetter)
    # shapes the entries do not serve
    wide, _ = _stubbed("RendezvousPolicy", num_agents=520)
    wide.ticks_per_launch = 4
    with pytest.raises(UnsupportedRolloutShape, match="576 threads"):
        wide.tick_launch(sampler, [None], resetter, batch=_batch(3, 520, F, 4), policy=(_packed(F, 64, 5), 64))
    pooled, _ = _stubbed("RendezvousPolicy", pools={"mood": "mood_reset_pool"})
    with pytest.raises(UnsupportedRolloutShape, match="reset pool"):
        pooled.tick_launch(sampler, [None], resetter, **ok)
    absent, _ = _stubbed("RendezvousPolicy", missing=["HipRendezvousPolicyRollout_H32"])
    with pytest.raises(UnsupportedRolloutShape, match="HipRendezvousPolicyRollout_H32"):
        absent.tick_launch(sampler, [None], resetter, **ok)
    for A in (0, 9):
        with pytest.raises(UnsupportedRolloutShape, match=f"{A} actions"):
            custom_rollout_launch(env, "HipRendezvousPolicyRollout_H32", env.TICK_STEP_ARGS, sampler, A, packed, 32,
                                  resetter, batch, 4)
    # nothing was looked up or launched for a refused request ... and a served one still goes through
    assert env.cuda_function_manager.initialized == [] and resetter.calls == []
    assert env.tick_launch(sampler, [None], resetter, **ok)[0].name == "HipRendezvousPolicyRollout_H32"
    assert not getattr(env, "TICK_POOL_RESET", False) and not getattr(env, "TICK_ENV_RANGES", False)
    assert not getattr(env, "ROLLOUT_POOL_RESET", False)


# --------------------------------------------------------------------------------- the GPU cases, on the host alone
def test_the_gpu_cases_cannot_pass_vacuously():
    """every case of tests/test_gpu_custom_env_rollout.py replayed with the host step, the model and the Philox replay
    alone: every action occurs wherever there is more than one, the near-threshold draws stay within near_cap's rule (a
    condition on the cases, not a measurement of the device), and replicas finish both early and at the time limit"""
    early = timed = 0
    for case in model.RENDEZVOUS_CASES + model.PROBE_CASES:
        got = model.simulate(case)
        print(f"{case}: seed {case.seed}, actions {got['actions'].tolist()}, {got['early']} early and {got['timed']} timed "
              f"finishes, {got['near']} near-threshold draws of {case.draws} (cap {case.near_cap()})")
        assert got["actions"].sum() == case.draws
        if case.A > 1:
            assert (got["actions"] > 0).all(), case
        assert got["near"] <= case.near_cap(), case
        assert got["timed"] >= 1, case
        if case.kind == "rendezvous":
            early, timed = early + got["early"], timed + got["timed"]
            if case.N > 1:
                assert got["early"] >= 1, case
    assert early >= 1 and timed >= 1
    # the shapes the issue lists, both widths; the wide one at width 32 only
    shapes = {(c.E, c.N, c.L, c.T, c.hidden) for c in model.RENDEZVOUS_CASES}
    assert shapes == {s + (H,) for s in model.RENDEZVOUS_SHAPES for H in (32, 64)} | {model.WIDE_SHAPE + (32,)}
    assert {(c.A, c.N, c.hidden) for c in model.PROBE_CASES} == {(A, N, H) for A in (1, 2, 8) for N in (1, 5, 70)
                                                                 for H in (32, 64)}
