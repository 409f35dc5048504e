#!/usr/bin/env python3
"""Env-steps/s of Acrobot, MountainCar, ContinuousMountainCar and Pendulum at E = 100 000 replicas for three rollout
paths: the unfused plan (sampler, step kernel, reset kernel), the fused tick at T = 1 tick per launch and at T = 50.
The two discrete envs have a fourth: the live-policy rollout at T = 50 (HipClassicControl<X>EnvRollout_H32 / _H64: the
policy network evaluated by the kernel on every tick, every tick recorded in the batch tensors), beside the
fixed-probability T = 50 tick recording the same rows -- the difference is the cost of the in-kernel forward.
One JSON line per (env, path): wall time per tick over a timed loop of launches (events around the loop), env-steps/s,
and the step's algorithmic bytes per env-step (state read + write, action, observation, reward, done, timestep read +
write -- the unfused step kernel's own traffic; the fused tick moves less per step: the state stays in registers)
over the measured time as a fraction of the HBM peak.  Kernel times: run it a second time under
`rocprofv3 --kernel-trace --stats` (the kernel-only times then come from the profiler, not from this loop).

`--trainer`: instead, the trainer's rollout of one 50-tick batch (`Trainer._generate_rollout_batch`, host time between
two synchronisations) on single_acrobot / single_mountain_car with a [H, H] policy, per-tick path against one-launch
path (`trainer.fused_rollout_policy: "all"`), in one process.

    python scripts/classic_control_timing.py [--envs 100000] [--ticks 200] [--only acrobot mountain_car]
    python scripts/classic_control_timing.py --trainer [--envs 1000] [--batches 20]
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
    tpl = {"unfused": 1, "fused T=1": 1}.get(path, 50)
    extra = {}
    if path.startswith("live policy") or path.endswith("recorded"):
        O = int(w.env.observation_space[0].shape[0])
        dev = torch.device("cuda", torch.cuda.current_device())
        extra["rollout_batch"] = {"obs": torch.zeros((tpl, E, 1, O), device=dev),
                                  "actions": torch.zeros((tpl, E, 1, 1), dtype=torch.int32, device=dev),
                                  "rewards": torch.zeros((tpl, E, 1), device=dev),
                                  "done": torch.zeros((tpl, E), dtype=torch.int32, device=dev)}
    if path.startswith("live policy"):
        from warp_drive_amd.training.models import FullyConnected
        from warp_drive_amd.training.policy_kernel import pack_rollout_policy

        H = int(path.rsplit("H=", 1)[1])
        torch.manual_seed(5)
        extra["rollout_policy"] = (pack_rollout_policy(FullyConnected(O, [3], [H, H])).to(dev), H)
    engine = RolloutEngine(w, sampler, fused=path != "unfused", ticks_per_launch=tpl, **extra)
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


def measure_trainer(config, E, hidden, one_launch, batches):
    """host time of the trainer's rollout of one 50-tick batch"""
    import tempfile
    import time

    from warp_drive_amd.training.scripts.train import setup_trainer

    ov = {"trainer": {"num_envs": E, "train_batch_size": E * 50, "num_episodes": 10 ** 7, "seed": 7},
          "env": {"episode_length": 200}, "saving": {"metrics_log_freq": 10 ** 6, "model_params_save_freq": 0},
          "policy": {"shared": {"model": {"type": "fully_connected", "fc_dims": [hidden, hidden],
                                          "model_ckpt_filepath": ""}}}}
    if one_launch:
        ov["trainer"]["fused_rollout_policy"] = "all"
    import yaml

    base = yaml.safe_load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "warp_drive_amd",
                                            "training", "run_configs", f"{config}.yaml")))
    ov["policy"]["shared"] = {**base["policy"]["shared"], **ov["policy"]["shared"]}
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as d:
        tr = setup_trainer(config, ov, results_dir=d, verbose=False)
        assert (tr._batch_rollout is not None) == one_launch
        for _ in range(3):
            tr._generate_rollout_batch()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(batches):
            tr._generate_rollout_batch()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / batches
        kernel = tr.engine.step_kernel_name
        tr.graceful_close()
    return {"config": config, "n_envs": E, "hidden": hidden, "path": "one launch per batch" if one_launch else "per tick",
            "kernel": kernel, "ms_per_50_tick_batch": round(dt * 1e3, 3), "env_steps_per_s": round(E * 50 / dt)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=100000)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--only", nargs="*", default=list(BYTES), choices=list(BYTES))
    ap.add_argument("--trainer", action="store_true", help="time the trainer's rollout of a 50-tick batch instead")
    ap.add_argument("--batches", type=int, default=20)
    args = ap.parse_args()
    if args.trainer:
        for config in ("single_acrobot", "single_mountain_car"):
            for hidden in (32, 64):
                for one_launch in (False, True):
                    print(json.dumps(measure_trainer(config, args.envs, hidden, one_launch, args.batches)), flush=True)
        return
    for name in args.only:
        paths = ["unfused", "fused T=1", "fused T=50"]
        if name in ("acrobot", "mountain_car"):
            paths += ["fused T=50 recorded", "live policy T=50 H=32", "live policy T=50 H=64"]
        for path in paths:
            print(json.dumps(measure(name, args.envs, args.ticks, path)), flush=True)


if __name__ == "__main__":
    main()
