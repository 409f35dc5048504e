#!/usr/bin/env python3
"""Env-steps/s of Acrobot, MountainCar, ContinuousMountainCar and Pendulum at E = 100 000 replicas for three rollout
paths: the unfused plan (sampler, step kernel, reset kernel), the fused tick at T = 1 tick per launch and at T = 50.
One JSON line per (env, path): wall time per tick over a timed loop of launches (events around the loop), env-steps/s,
and the step's algorithmic bytes per env-step (state read + write, action, observation, reward, done, timestep read +
write -- the unfused step kernel's own traffic; the fused tick moves less per step: the state stays in registers)
over the measured time as a fraction of the HBM peak.  Kernel times: run it a second time under
`rocprofv3 --kernel-trace --stats` (the kernel-only times then come from the profiler, not from this loop).

    python scripts/classic_control_timing.py [--envs 100000] [--ticks 200]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # MI355X HBM3E, bytes/s
BYTES = {"acrobot": 76, "mountain_car": 44, "continuous_mountain_car": 44, "pendulum": 48}


def _env(name, T):
    from warp_drive_amd.envs import classic_control as cc

    cls = {"acrobot": cc.CUDAClassicControlAcrobotEnv, "mountain_car": cc.CUDAClassicControlMountainCarEnv,
           "continuous_mountain_car": cc.CUDAClassicControlContinuousMountainCarEnv,
           "pendulum": cc.CUDAClassicControlPendulumEnv}[name]
    return cls(episode_length=T, seed=5)


def measure(name, E, ticks, path):
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.rollout import RolloutEngine
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

    w = EnvWrapper(env_obj=_env(name, 200), num_envs=E, env_backend="hip")
    w.reset_all_envs()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=1)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    tpl = {"unfused": 1, "fused T=1": 1, "fused T=50": 50}[path]
    engine = RolloutEngine(w, sampler, fused=path != "unfused", ticks_per_launch=tpl)
    launches = max(1, ticks // engine.ticks_per_launch)
    engine.run(max(1, launches // 4))
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    engine.run(launches)
    t1.record()
    torch.cuda.synchronize()
    per_tick = t0.elapsed_time(t1) * 1e-3 / (launches * engine.ticks_per_launch)
    return {"env": name, "path": path, "n_envs": E, "ticks_per_launch": engine.ticks_per_launch,
            "entries": engine.entry_names, "wall_us_per_tick": round(per_tick * 1e6, 3),
            "env_steps_per_s": round(E / per_tick), "alg_bytes_per_step": BYTES[name],
            "alg_bytes_over_wall_frac_hbm": round(BYTES[name] * E / per_tick / HBM_PEAK, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=100000)
    ap.add_argument("--ticks", type=int, default=200)
    args = ap.parse_args()
    for name in BYTES:
        for path in ("unfused", "fused T=1", "fused T=50"):
            print(json.dumps(measure(name, args.envs, args.ticks, path)), flush=True)


if __name__ == "__main__":
    main()
