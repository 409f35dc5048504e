"""The in-kernel policy of the ClassicControl Acrobot / MountainCar rollouts, on the host: the restatement of its
arithmetic (tests/classic_control_policy.py) against the float64 PyTorch network, the code object of the four
HipClassicControl<X>EnvRollout_H<width> entries, which env classes admit them, the launch `tick_launch` builds with and
without a policy (fakes for the managers, as tests/test_gridworld_shapes_logic.py), and the sizing of the GPU parity test."""
import copy
import json
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import classic_control_policy as ccp

ROLLOUT_KERNELS = [f"HipClassicControl{x}EnvRollout_H{h}" for x in ("Acrobot", "MountainCar") for h in (32, 64)]


@pytest.mark.parametrize("O", [6, 2])
@pytest.mark.parametrize("hidden", [32, 64])
def test_policy_restatement_matches_float64_network(O, hidden):
    """probabilities within the project's 2e-6 gate of the float64 forward of FullyConnected(O, [3], [H, H]) with the head
    weights scaled by 6, over 20 000 observations (measured on the CPU: at most 6.8e-7)"""
    import torch
    from warp_drive_amd.training.models import FullyConnected
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy, rollout_policy_width

    torch.manual_seed(5)
    model = FullyConnected(O, [3], [hidden, hidden])
    with torch.no_grad():
        model.policy_head[0].weight.mul_(6.0)
    assert rollout_policy_width(model, O) == hidden
    packed = pack_rollout_policy(model)
    assert packed.numel() == ccp.policy_weight_count(O, hidden, 3) == O * hidden + hidden + hidden * hidden + hidden + 3 * hidden + 3
    rng = np.random.RandomState(O * 100 + hidden)
    scale = np.array([1, 1, 1, 1, 12.6, 28.3], np.float32) if O == 6 else np.array([1.2, 0.07], np.float32)
    obs = (rng.uniform(-1, 1, size=(20000, O)) * scale).astype(np.float32)
    got = ccp.policy_probabilities(packed.numpy(), hidden, obs, 3)
    with torch.no_grad():
        want = copy.deepcopy(model).double()(torch.from_numpy(obs).double())[0][0].numpy()
    assert got.dtype == np.float32 and got.shape == (20000, 3)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"O={O} H={hidden}: largest probability difference {err:.2e}")
    assert err <= 2e-6, err
    assert np.ptp(want, axis=0).max() > 0.1  # the probabilities vary with the observation: not one constant row
    # the four-float case is the oracle's own restatement, bit for bit
    if O == 2:
        from oracle.cartpole_np import policy_probabilities as cartpole_probabilities

        torch.manual_seed(6)
        m4 = FullyConnected(4, [2], [hidden, hidden])
        p4 = pack_rollout_policy(m4).numpy()
        o4 = rng.uniform(-2, 2, size=(500, 4)).astype(np.float32)
        np.testing.assert_array_equal(ccp.policy_probabilities(p4, hidden, o4, 2), cartpole_probabilities(p4, hidden, o4))


def test_sampler_helpers():
    p = np.array([[0.25, 0.25, 0.5], [0.0, 1.0, 0.0]], np.float32)
    cum = ccp.running_sums(p)
    np.testing.assert_array_equal(cum, np.array([[0.25, 0.5, 1.0], [0.0, 1.0, 1.0]], np.float32))
    np.testing.assert_array_equal(ccp.count_below(cum, np.array([0.25, 1.0], np.float32)), [0, 1])
    np.testing.assert_array_equal(ccp.count_below(cum, np.array([0.26, 0.5], np.float32)), [1, 1])
    np.testing.assert_array_equal(ccp.count_below(np.array([[0.2, 0.4, 0.9]], np.float32), np.array([1.0], np.float32)), [2])


def _manifest():
    from warp_drive_amd import build as wd_build

    wd_build.build_kernels_locked()
    return json.load(open(wd_build.MANIFEST))


def test_rollout_kernels_in_the_code_object_without_scratch_or_spills():
    """all four entries are in wd_kernels_cc.hsaco, and none has a private segment or a spilled VGPR"""
    from warp_drive_amd import build as wd_build

    manifest = _manifest()
    for k in ROLLOUT_KERNELS:
        assert manifest.get(k) == "wd_kernels_cc.hsaco", k
    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "cc.elf")
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={os.path.join(wd_build.CSRC, 'wd_kernels_cc.hsaco')}", f"--output={elf}"],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                               text=True).stdout
    found = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?"
                       r"\s+\.vgpr_spill_count:\s+(\d+)", notes)
    found = {n: (int(p), int(v)) for n, p, v in found if n in ROLLOUT_KERNELS}
    assert set(found) == set(ROLLOUT_KERNELS)
    for name, (private, spills) in found.items():
        assert private == 0 and spills == 0, (name, private, spills)


# ----------------------------------------------------------------------------------- fakes for the managers
class _FakeFn:
    def __init__(self, name):
        self.name = name


class _FakeFM:
    def __init__(self, manifest):
        self.manifest, self.initialized = manifest, []

    def initialize_functions(self, names):
        self.initialized += list(names)

    def has_function(self, name):
        return name in self.manifest

    def get_function(self, name):
        return _FakeFn(name)


class _FakeDM:
    reset_target_to_pool = {}

    def __init__(self, E, O):
        self.E, self.O = E, O

    def meta_info(self, key):
        return {"n_envs": self.E}[key]

    def get_shape(self, name):
        return {"observations": (self.E, 1, self.O)}[name]


class _FakeResetter:
    def fused_launch(self, dm, force, undo):
        return None, ["table", 2], None, None


def _classes():
    from warp_drive_amd.envs import classic_control as cc

    return {"acrobot": (cc.CUDAClassicControlAcrobotEnv, 6, "Acrobot"),
            "mountain_car": (cc.CUDAClassicControlMountainCarEnv, 2, "MountainCar"),
            "continuous_mountain_car": (cc.CUDAClassicControlContinuousMountainCarEnv, 2, "ContinuousMountainCar"),
            "pendulum": (cc.CUDAClassicControlPendulumEnv, 3, "Pendulum")}


def _fake_managed(env_name, E, manifest):
    cls, O, x = _classes()[env_name]
    env = cls(episode_length=20, seed=5)
    env.cuda_function_manager, env.cuda_data_manager = _FakeFM(manifest), _FakeDM(E, O)
    env.cuda_step = _FakeFn(f"HipClassicControl{x}EnvStep")
    env.cuda_step_function_feed = lambda names: [("arg", n) for n in names]
    return env


def _tensor(shape, dtype, cuda=True, contiguous=True):
    n = int(np.prod(shape))
    return types.SimpleNamespace(is_cuda=cuda, is_contiguous=lambda: contiguous, dtype=dtype, shape=tuple(shape),
                                 numel=lambda: n)


def test_which_envs_admit_a_live_policy():
    """true exactly for (Acrobot | MountainCar) x {32, 64} x n_actions <= 8 with the entry in the manifest"""
    manifest = _manifest()
    for name, (cls, _, x) in _classes().items():
        discrete = name in ("acrobot", "mountain_car")
        assert getattr(cls, "ROLLOUT_POLICY_WIDTHS", None) == ((32, 64) if discrete else None), name
        assert cls.ROLLOUT_POLICY_OPT_IN is True
        env = _fake_managed(name, 1000, manifest)
        for width in (8, 16, 31, 32, 33, 48, 64, 128, 256):
            for n_actions in (1, 2, 3, 8, 9, 21):
                want = discrete and width in (32, 64) and n_actions <= 8
                assert env.has_live_policy_rollout(width, n_actions) is want, (name, width, n_actions)
        # ... and only while the code object has the entry
        env.cuda_function_manager = _FakeFM({k: v for k, v in manifest.items() if "Rollout_H32" not in k})
        assert not env.has_live_policy_rollout(32, 3) and env.has_live_policy_rollout(64, 3) is discrete


@pytest.mark.parametrize("env_name", ["acrobot", "mountain_car", "continuous_mountain_car", "pendulum"])
def test_tick_launch_without_a_policy_is_the_fixed_probability_launch(env_name):
    """name, arguments, block, grid and `shared == 0` of the launch the fused tick had before the rollout entries"""
    import torch
    from warp_drive_amd.managers.function_manager import _stream_tag

    E, T = 70001, 7
    cls, O, x = _classes()[env_name]
    env = _fake_managed(env_name, E, _manifest())
    env.ticks_per_launch = T
    cont = env_name in ("continuous_mountain_car", "pendulum")
    probs = _tensor((E, 1, 1) if cont else (E, 1, 3), torch.float32)
    sampler = types.SimpleNamespace(rng_state="rng")
    if cont:
        env.cuda_data_manager.device_data = lambda name: ("device", name)
    fn, args, block, grid, shared = env.tick_launch(sampler, [probs], _FakeResetter())
    assert fn.name == f"HipClassicControl{x}EnvTick" and env.cuda_function_manager.initialized == [fn.name]
    assert block == (256, 1, 1) and grid == (min(4096, (E + 255) // 256), 1) and shared == 0
    null = np.uint64(0)
    step_args = [("arg", n) for n in env._step_args()]
    ou = ([("device", "sampled_actions_ou_state"), np.float32(0.15), np.float32(0.2), np.float32(1.0)] if cont
          else [null, np.float32(0), np.float32(0), np.float32(0)])
    want = step_args + ["rng", probs, np.int32(1 if cont else 3), "table", 2, _stream_tag("tick"), np.int32(T)] + \
        [null] * 4 + [null, null, np.int32(0)] + ou
    assert len(args) == len(want)
    for i, (g, w) in enumerate(zip(args, want)):
        assert type(g) is type(w) and g == w, (i, g, w)


@pytest.mark.parametrize("env_name,O", [("acrobot", 6), ("mountain_car", 2)])
@pytest.mark.parametrize("width", [32, 64])
def test_tick_launch_with_a_policy(env_name, O, width):
    """the Rollout_H<width> entry, the tick's arguments followed by (packed, width), 4 n_w bytes of LDS; anything else is
    UnsupportedRolloutShape"""
    import torch
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    E, T = 1000, 5
    x = _classes()[env_name][2]
    env = _fake_managed(env_name, E, _manifest())
    env.ticks_per_launch = T
    probs = _tensor((E, 1, 3), torch.float32)
    sampler = types.SimpleNamespace(rng_state="rng")
    n_w = ccp.policy_weight_count(O, width, 3)
    packed = _tensor((n_w,), torch.float32)
    plain = env.tick_launch(sampler, [probs], _FakeResetter())
    fn, args, block, grid, shared = env.tick_launch(sampler, [probs], _FakeResetter(), policy=(packed, width))
    assert fn.name == f"HipClassicControl{x}EnvRollout_H{width}" and shared == 4 * n_w <= 65536
    assert (block, grid) == (plain[2], plain[3])
    assert len(args) == len(plain[1]) + 2 and args[-2] is packed and type(args[-1]) is np.int32 and args[-1] == width
    for g, w in zip(args[:-2], plain[1]):
        assert type(g) is type(w) and g == w
    bad = [(_tensor((n_w + 1,), torch.float32), width), (_tensor((n_w,), torch.float64), width),
           (_tensor((n_w,), torch.float32, cuda=False), width), (_tensor((n_w,), torch.float32, contiguous=False), width),
           (packed, 48), (packed, 96 - width), packed]
    for policy in bad:
        with pytest.raises(UnsupportedRolloutShape):
            env.tick_launch(sampler, [probs], _FakeResetter(), policy=policy)
    with pytest.raises(UnsupportedRolloutShape):  # nine actions do not fit the kernel's registers
        env.tick_launch(sampler, [_tensor((E, 1, 9), torch.float32)], _FakeResetter(),
                        policy=(_tensor((ccp.policy_weight_count(O, width, 9),), torch.float32), width))


@pytest.mark.parametrize("env_name", ["continuous_mountain_car", "pendulum"])
def test_box_envs_refuse_a_policy(env_name):
    import torch
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    env = _fake_managed(env_name, 1000, _manifest())
    probs = _tensor((1000, 1, 1), torch.float32)
    with pytest.raises(UnsupportedRolloutShape):
        env.tick_launch(types.SimpleNamespace(rng_state="rng"), [probs], _FakeResetter(),
                        policy=(_tensor((100,), torch.float32), 32))


@pytest.mark.parametrize("env_name", ["acrobot", "mountain_car"])
@pytest.mark.parametrize("hidden", [32, 64])
@pytest.mark.parametrize("pool", [0, 16])
def test_parity_case_is_not_vacuous_on_the_host(env_name, hidden, pool):
    """the GPU parity test's policy, seeds and sizes, replayed on the host alone: at least 2 E finished episodes, each
    action at least 5 % of the draws, at least 8 of the 16 pool rows drawn"""
    from warp_drive_amd.managers.function_manager import _stream_tag

    r = ccp.host_rollout(env_name, hidden, pool, _stream_tag("tick"))
    E = ccp.PARITY["E"]
    draws = E * ccp.PARITY["ticks"] * ccp.PARITY["launches"]
    assert draws == 90060 and r["action_counts"].sum() == draws
    assert r["finished"] >= 2 * E
    assert (r["action_counts"] >= 0.05 * draws).all(), r["action_counts"]
    assert not pool or len(r["pool_rows"]) >= 8


def test_opt_in_switch_is_documented_next_to_the_key():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "warp_drive_amd", "training", "run_configs", "default_configs.yaml")).read()
    at = text.index("fused_rollout_policy:")
    assert '"all"' in text[at:at + 1200]
