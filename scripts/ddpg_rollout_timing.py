#!/usr/bin/env python3
"""TrainerDDPG on single_pendulum and single_continuous_mountain_car at E = 10 000 replicas, T = 5 ticks per iteration:
host time of the rollout (`_generate_rollout_batch`) and of the update (`_update_model_params`) between two
synchronisations, on the per-tick path and on the one-launch path (`trainer.fused_rollout_policy: "all"`:
HipClassicControl<X>EnvRollout_A64).  Both trainers live in one process and are called alternately: two warm-up calls
and seven timed calls each.  One JSON line per (env, path) with the median and the spread.

    python scripts/ddpg_rollout_timing.py [--envs 10000] [--ticks 5] [--calls 7]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(env_name, E, T, path, results_dir):
    from warp_drive_amd.training.scripts.train import setup_trainer

    ov = {"trainer": {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": 1,
                      "fused_rollout_policy": "all" if path == "one launch" else False},
          "saving": {"metrics_log_freq": 10 ** 9, "model_params_save_freq": 0}}
    torch.manual_seed(1)
    tr = setup_trainer(env_name, ov, results_dir=results_dir, verbose=False)
    assert tr.rollout_path == path, (tr.rollout_path, path)
    return tr


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=10000)
    ap.add_argument("--ticks", type=int, default=5)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    paths = ("per tick", "one launch")
    for env_name in ("single_pendulum", "single_continuous_mountain_car"):
        with tempfile.TemporaryDirectory() as tmp:
            trainers = {p: build(env_name, args.envs, args.ticks, p, os.path.join(tmp, p.replace(" ", "_"))) for p in paths}
            times = {p: {"rollout": [], "update": []} for p in paths}
            for call in range(args.warmup + args.calls):
                for p in paths:   # alternating: both paths see the same drift of the clocks
                    tr = trainers[p]
                    r = timed(tr._generate_rollout_batch)
                    u = timed(lambda: tr._update_model_params(call, False))
                    if call >= args.warmup:
                        times[p]["rollout"].append(r)
                        times[p]["update"].append(u)
            for p in paths:
                rec = {"env": env_name, "path": p, "envs": args.envs, "ticks": args.ticks, "calls": args.calls}
                for k, v in times[p].items():
                    rec[f"{k}_us_median"] = round(float(np.median(v)), 1)
                    rec[f"{k}_us_min"] = round(float(np.min(v)), 1)
                    rec[f"{k}_us_max"] = round(float(np.max(v)), 1)
                print(json.dumps(rec), flush=True)
            for tr in trainers.values():
                tr.graceful_close()


if __name__ == "__main__":
    main()
