#!/usr/bin/env python3
"""TrainerDDPG.evaluate_episodes(use_argmax=True) on single_pendulum and single_continuous_mountain_car at E = 10 000
replicas: host time of one greedy evaluation between two synchronisations, on the per-tick path (actor forward, fused
tick and HipEvaluateAccumulate per tick) and on the one-launch path (`trainer.fused_evaluation: true`:
HipClassicControl<X>EnvEvaluate_A64).  Both trainers live in one process and are called alternately: two warm-up calls
and seven timed calls each.  One JSON line per (env, path) with the median and the spread.

    python scripts/ddpg_evaluate_timing.py [--envs 10000] [--calls 7]
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


def build(env_name, E, path, results_dir):
    from warp_drive_amd.training.scripts.train import setup_trainer

    ov = {"trainer": {"num_envs": E, "train_batch_size": E * 5, "num_episodes": 10 ** 6, "seed": 1,
                      "fused_rollout_policy": "all", "fused_evaluation": path == "one launch"},
          "saving": {"metrics_log_freq": 10 ** 9, "model_params_save_freq": 0}}
    torch.manual_seed(1)
    tr = setup_trainer(env_name, ov, results_dir=results_dir, verbose=False)
    assert tr.rollout_path == "one launch"
    return tr


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=10000)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    paths = ("per tick", "one launch")
    for env_name in ("single_pendulum", "single_continuous_mountain_car"):
        with tempfile.TemporaryDirectory() as tmp:
            trainers = {p: build(env_name, args.envs, p, os.path.join(tmp, p.replace(" ", "_"))) for p in paths}
            times, last = {p: [] for p in paths}, {}
            for call in range(args.warmup + args.calls):
                for p in paths:   # alternating: both paths see the same drift of the clocks
                    tr = trainers[p]
                    t, last[p] = timed(lambda: tr.evaluate_episodes(use_argmax=True))
                    assert tr.evaluation_path == p, (tr.evaluation_path, p)
                    if call >= args.warmup:
                        times[p].append(t)
            for p in paths:
                rewards, steps = last[p]
                rec = {"env": env_name, "path": p, "envs": args.envs, "calls": args.calls,
                       "episode_length": int(trainers[p].w.episode_length),
                       "evaluate_us_median": round(float(np.median(times[p])), 1),
                       "evaluate_us_min": round(float(np.min(times[p])), 1),
                       "evaluate_us_max": round(float(np.max(times[p])), 1),
                       "mean_steps": round(float(steps["shared"].mean()), 2),
                       "mean_reward": round(float(rewards["shared"].mean()), 3)}
                print(json.dumps(rec), flush=True)
            for tr in trainers.values():
                tr.graceful_close()


if __name__ == "__main__":
    main()
