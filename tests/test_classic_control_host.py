"""ClassicControl Acrobot / MountainCar / ContinuousMountainCar / Pendulum on the host: the numpy steps of
warp_drive_amd/envs/classic_control.py against the reference's kernel sources (tests/golden/cc_<env>_traj.npz,
scripts/gen_classic_control_golden.py), the env API, the run configs, and the code object of the device kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENVS = ("acrobot", "mountain_car", "continuous_mountain_car", "pendulum")


def _step_fn(env):
    from warp_drive_amd.envs import classic_control as cc

    return {"acrobot": cc.acrobot_step, "mountain_car": cc.mountain_car_step,
            "continuous_mountain_car": cc.continuous_mountain_car_step, "pendulum": cc.pendulum_step}[env]


@pytest.mark.parametrize("env", ENVS)
def test_numpy_step_replays_reference_kernel_source(env):
    """tick by tick: each tick starts from the fixture's recorded inputs; floats within 1e-5 abs, discrete exact
    (MountainCar's done == 2 on the goal included)"""
    from warp_drive_amd.envs.classic_control import apply_done

    g = np.load(os.path.join(GOLDEN, f"cc_{env}_traj.npz"))
    T = int(g["episode_length"])
    step = _step_fn(env)
    for t in range(g["actions"].shape[0]):
        state, obs, rew, term = step(g["state_in"][t], g["actions"][t])
        ts = g["timestep_in"][t] + 1
        np.testing.assert_array_equal(ts, g["timestep"][t])
        np.testing.assert_allclose(state, g["state"][t], rtol=0, atol=1e-5, err_msg=f"{env} t={t}")
        np.testing.assert_allclose(obs, g["obs"][t], rtol=0, atol=1e-5, err_msg=f"{env} t={t}")
        np.testing.assert_allclose(rew, g["rewards"][t], rtol=0, atol=1e-5, err_msg=f"{env} t={t}")
        np.testing.assert_array_equal(apply_done(term, ts, T), g["done"][t], err_msg=f"{env} t={t}")
    if env == "mountain_car":
        assert (g["done"] == 2).any()


def _classes():
    from warp_drive_amd.envs import classic_control as cc

    return {"acrobot": (cc.ClassicControlAcrobotEnv, cc.CUDAClassicControlAcrobotEnv, 4, 6, 3),
            "mountain_car": (cc.ClassicControlMountainCarEnv, cc.CUDAClassicControlMountainCarEnv, 2, 2, 3),
            "continuous_mountain_car": (cc.ClassicControlContinuousMountainCarEnv,
                                        cc.CUDAClassicControlContinuousMountainCarEnv, 2, 2, None),
            "pendulum": (cc.ClassicControlPendulumEnv, cc.CUDAClassicControlPendulumEnv, 2, 3, None)}


@pytest.mark.parametrize("env", ENVS)
def test_spaces_fixed_start_and_reset_pool(env):
    from warp_drive_amd.training.data_loader import reset_is_deterministic
    from warp_drive_amd.utils import spaces

    cpu_cls, dev_cls, S, O, n_act = _classes()[env]
    e = cpu_cls(episode_length=20, seed=11)
    if n_act is None:
        assert isinstance(e.action_space[0], spaces.Box) and tuple(e.action_space[0].shape) == (1,)
    else:
        assert isinstance(e.action_space[0], spaces.Discrete) and e.action_space[0].n == n_act
    assert tuple(e.observation_space[0].shape) == (O,)
    o1, o2 = e.reset()[0], e.reset()[0]
    assert o1.shape == (O,) and o1.dtype == np.float32
    np.testing.assert_array_equal(o1, o2)  # seeded fixed start
    np.testing.assert_array_equal(cpu_cls(episode_length=20, seed=11).reset()[0], o1)
    assert reset_is_deterministic(e)
    pooled = cpu_cls(episode_length=20, seed=11, reset_pool_size=16)
    assert not reset_is_deterministic(pooled)
    assert not np.array_equal(pooled.reset()[0], pooled.reset()[0])
    d = dev_cls(episode_length=20, seed=11, reset_pool_size=16)
    feed = d.get_data_dictionary()
    assert feed["state"]["data"].shape == (1, S) and not feed["state"]["attributes"]["save_copy_and_apply_at_reset"]
    pool = d.get_reset_pool_dictionary()
    assert pool["state_reset_pool"]["data"].shape == (16, 1, S)
    assert pool["state_reset_pool"]["attributes"]["reset_target"] == "state"
    assert len(dev_cls(episode_length=20, seed=11).get_reset_pool_dictionary()) == 0
    assert dev_cls.TICK_HEADS == 1 and dev_cls.TICK_POOL_RESET and dev_cls.ticks_per_launch == 1


@pytest.mark.parametrize("env", ENVS)
def test_env_wrapper_cpu_episode(env):
    from warp_drive_amd.env_wrapper import EnvWrapper

    cpu_cls, _, S, O, n_act = _classes()[env]
    w = EnvWrapper(env_obj=cpu_cls(episode_length=25, seed=3), env_backend="cpu")
    obs = w.reset()
    assert obs[0].shape == (O,)
    rng = np.random.RandomState(0)
    for t in range(25):
        a = rng.randint(0, n_act) if n_act else np.float32(rng.uniform(-2, 2))
        obs, rew, done, _ = w.step({0: a})
        assert obs[0].shape == (O,) and np.isfinite(rew[0])
        if done["__all__"]:
            break
    assert done["__all__"]


def test_train_script_knows_the_new_configs():
    from warp_drive_amd.training.scripts import train

    for name in ("single_acrobot", "single_mountain_car"):
        assert name in train._ENVS
        import yaml

        cfg = yaml.safe_load(open(os.path.join(train._CONFIGS, f"{name}.yaml")))
        assert cfg["name"] == name and cfg["env"]["reset_pool_size"] > 1
        assert "neg_pos_env_ratio" not in cfg["trainer"]


KERNELS = [f"HipClassicControl{x}Env{k}" for x in ("Acrobot", "MountainCar", "ContinuousMountainCar", "Pendulum")
           for k in ("Step", "Tick")]


def test_kernels_in_their_own_code_object_without_scratch():
    from warp_drive_amd import build as wd_build

    wd_build.build_kernels_locked()
    import json

    manifest = json.load(open(wd_build.MANIFEST))
    for k in KERNELS:
        assert manifest.get(k) == "wd_kernels_cc.hsaco", k
    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    import tempfile

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
    found = {n: (int(p), int(v)) for n, p, v in found if n in KERNELS}
    assert set(found) == set(KERNELS)
    for name, (private, spills) in found.items():
        assert private == 0 and spills == 0, (name, private, spills)
