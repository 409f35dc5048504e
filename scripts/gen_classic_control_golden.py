#!/usr/bin/env python3
"""Record tests/golden/cc_<env>_traj.npz: the reference's own device kernels for Acrobot, MountainCar,
ContinuousMountainCar and Pendulum (example_envs/single_agent/classic_control/*/*_step_numba.py) executed on the host
under a minimal `numba.cuda` stand-in (jit = identity, blockIdx / threadIdx set per replica, const.array_like and
local.array as numpy arrays) -- the recipe of oracle/gen_golden.py::gen_cartpole_traj.

    python scripts/gen_classic_control_golden.py [--reference DIR]

Every tick of every replica is recorded with its inputs: the state and timestep it starts from, the action, and what
the kernel wrote (state, observation, reward, done, timestep).  Finished replicas restart from a fresh draw, so a
fixture is replayed TICK BY TICK (the tests load each tick's inputs): Acrobot is chaotic, and the stand-in evaluates
with Python / numpy types rather than Numba's (math.cos of a float32 in float64, ...), so the fixtures pin the
arithmetic to ~1e-5, not bit for bit.  Nothing of the reference is copied: the script reads its sources when it runs.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")
KDIR = "example_envs/single_agent/classic_control"


class _Idx:
    x = 0


def load_kernel_module(reference, rel, modname):
    stub_cuda = types.ModuleType("numba.cuda")
    stub_cuda.jit = lambda f=None, **kw: f if f is not None else (lambda g: g)
    stub_cuda.blockIdx, stub_cuda.threadIdx = _Idx(), _Idx()
    stub_cuda.const = types.SimpleNamespace(array_like=lambda a: np.asarray(a))
    stub_cuda.local = types.SimpleNamespace(array=lambda shape, dtype: np.zeros(shape, dtype=dtype))
    stub = types.ModuleType("numba")
    stub.cuda = stub_cuda
    stub.float32 = np.float32
    saved = {k: sys.modules.get(k) for k in ("numba", "numba.cuda")}
    sys.modules["numba"], sys.modules["numba.cuda"] = stub, stub_cuda
    try:
        spec = importlib.util.spec_from_file_location(modname, os.path.join(reference, KDIR, rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod, stub_cuda


# per env: kernel file, kernel name, state dim, obs dim, continuous, episode length, float32 constants (in argument
# order, the values of envs/classic_control.py), initial-state sampler
SPECS = {
    "acrobot": ("acrobot/acrobot_step_numba.py", "NumbaClassicControlAcrobotEnvStep", 4, 6, False, 40, [],
                lambda rng, n: rng.uniform(-0.1, 0.1, size=(n, 4)) * np.array([20.0, 20.0, 40.0, 60.0])),
    "mountain_car": ("mountain_car/mountain_car_step_numba.py", "NumbaClassicControlMountainCarEnvStep", 2, 2, False, 40,
                     [-1.2, 0.6, 0.07, 0.5, 0.0, 0.001, 0.0025],
                     lambda rng, n: np.stack([rng.uniform(-1.2, 0.58, n), rng.uniform(-0.07, 0.07, n)], axis=1)),
    "continuous_mountain_car": ("continuous_mountain_car/continuous_mountain_car_step_numba.py",
                                "NumbaClassicControlContinuousMountainCarEnvStep", 2, 2, True, 40,
                                [-1.0, 1.0, -1.2, 0.6, 0.07, 0.45, 0.0, 0.0015],
                                lambda rng, n: np.stack([rng.uniform(-1.2, 0.5, n), rng.uniform(-0.07, 0.07, n)], axis=1)),
    "pendulum": ("pendulum/pendulum_step_numba.py", "NumbaClassicControlPendulumEnvStep", 2, 3, True, 40, [],
                 lambda rng, n: rng.uniform(-1.0, 1.0, size=(n, 2)) * np.array([np.pi, 8.0])),
}


def gen(reference, env, num_envs=32, num_ticks=100, seed=7000):
    rel, kname, S, O, cont, T, consts, draw = SPECS[env]
    mod, cuda = load_kernel_module(reference, rel, f"ref_{env}_step_numba")
    step = getattr(mod, kname)
    f32 = np.float32
    consts = [f32(c) for c in consts]
    E = num_envs
    rng = np.random.RandomState(seed)
    state = draw(rng, E).astype(f32).reshape(E, 1, S)
    timestep = rng.randint(0, T, size=E).astype(np.int32)  # replicas at every phase of an episode
    action = np.zeros((E, 1, 1), f32 if cont else np.int32)
    done = np.zeros(E, np.int32)
    reward = np.zeros((E, 1), f32)
    obs = np.zeros((E, 1, O), f32)
    rec = {k: [] for k in ("state_in", "timestep_in", "actions", "state", "obs", "rewards", "done", "timestep")}
    for _ in range(num_ticks):
        if cont:  # values outside the clip range included
            action[:] = rng.uniform(-3.0, 3.0, size=(E, 1, 1)).astype(f32)
        else:
            action[:] = rng.randint(0, 3, size=(E, 1, 1))
        rec["state_in"].append(state[:, 0].copy())
        rec["timestep_in"].append(timestep.copy())
        done[:] = 0
        for e in range(E):  # grid = (E,), block = (1,)
            cuda.blockIdx.x, cuda.threadIdx.x = e, 0
            step(state, action, done, reward, obs, *consts, timestep, T)
        for k, v in (("actions", action[:, 0, 0]), ("state", state[:, 0]), ("obs", obs[:, 0]),
                     ("rewards", reward[:, 0]), ("done", done), ("timestep", timestep)):
            rec[k].append(v.copy())
        m = done > 0  # finished replicas restart from a fresh draw
        state[m, 0] = draw(rng, int(m.sum())).astype(f32)
        timestep[m] = 0
    out = {k: np.stack(v) for k, v in rec.items()}
    out["episode_length"] = np.int32(T)
    np.savez_compressed(os.path.join(OUT, f"cc_{env}_traj.npz"), **out)
    print(f"cc_{env}_traj.npz: E={E} ticks={num_ticks} done values {np.unique(out['done']).tolist()} "
          f"(timeouts {int((out['timestep'] == T).sum())}, terminal {int(((out['done'] > 0) & (out['timestep'] < T)).sum())})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("WD_REFERENCE", "../reference"))
    args = ap.parse_args()
    for name in SPECS:
        gen(args.reference, name)
