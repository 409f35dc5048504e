#!/usr/bin/env python3
"""Trainer's A2C update of a policy with `normalize_return` AND `normalize_advantage` on its two paths -- "framework"
(what `trainer.fused_update: "all"` alone leaves such a policy on) and "kernels" (with
`trainer.fused_update_normalize: true`: eight launches, training/pg_update_kernels.py) -- in ONE process on the
one-launch rollout, by scripts/pg_update_timing.py's method (its `run` and `summary`: device events around
`_update_model_params`, the paths alternating inside a repeat), at Cartpole E = 100 000, T = 10 and at
tag_gridworld_with_reset_pool's shape (E = 2000, T = 100, one policy of five agents).  One JSON line per (shape, path),
for the kernels path with the device time of the two or three normalising launches alone per switch pair, and a last line
per shape: whether every repeat of one path is below every repeat of the other.

    python scripts/pg_normalize_timing.py [--iterations 100] [--warmup 10] [--repeats 5] [--shapes 0,1]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.pg_update_timing import run, summary  # noqa: E402

SHAPES = (("single_cartpole", 100000, 10), ("tag_gridworld_with_reset_pool", 2000, 100))   # (run config, replicas, ticks)


def build(name, E, T, path, results_dir):
    from warp_drive_amd.training import trainer as trainer_module
    from warp_drive_amd.training.scripts.train import setup_trainer

    shipped = yaml.safe_load(open(os.path.join(os.path.dirname(trainer_module._DEFAULT_CONFIG), f"{name}.yaml")))
    policy = {**shipped["policy"]["shared"], "normalize_return": True, "normalize_advantage": True}
    trainer = {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": 1, "fused_rollout_policy": "all",
               "fused_update": "all", "fused_update_normalize": path == "kernels"}
    ov = {"trainer": trainer, "policy": {"shared": policy}, "saving": {"metrics_log_freq": 10 ** 9, "model_params_save_freq": 0}}
    torch.manual_seed(1)
    tr = setup_trainer(name, ov, results_dir=results_dir, verbose=False)
    assert tr._batch_rollout is not None and tr.update_path == {"shared": path}, (tr.rollout_path, tr.update_path)
    return tr


def normalising_launches(tr, count):
    """device microseconds (medians) of `normalize` alone per switch pair, on what the last update left behind"""
    k, out = tr._pg_kernels["shared"], {}
    for name, switches in (("return", (True, False)), ("advantage", (False, True)), ("both", (True, True))):
        times = []
        for _ in range(count):
            torch.cuda.synchronize()
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            k.normalize(*switches)
            e.record()
            torch.cuda.synchronize()
            times.append(1e3 * a.elapsed_time(e))
        out[name] = {"median_us": round(float(np.median(times)), 1), "min_us": round(min(times), 1), "max_us": round(max(times), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="0,1")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    paths = ("framework", "kernels")
    for name, E, T in [SHAPES[int(i)] for i in args.shapes.split(",")]:
        with tempfile.TemporaryDirectory() as tmp:
            trainers = {p: build(name, E, T, p, os.path.join(tmp, p)) for p in paths}
            update, it = {p: [] for p in paths}, 0
            for _ in range(args.repeats):
                for p in paths:
                    run(trainers[p], it, args.warmup)
                    update[p].append(run(trainers[p], it + args.warmup, args.iterations)[0])
                it += args.warmup + args.iterations
            records = {}
            for p in paths:
                k = trainers["kernels"]._pg_kernels["shared"]
                records[p] = {"config": name, "envs": E, "ticks": T, "rows": k.rows, "columns": k.columns, "path": p,
                              "iterations": args.iterations, "warmup": args.warmup, "repeats": args.repeats,
                              "update": summary(update[p])}
                if p == "kernels":
                    records[p]["normalize_us"] = normalising_launches(trainers[p], 100)
                print(json.dumps(records[p]), flush=True)
            k, f = records["kernels"]["update"], records["framework"]["update"]
            print(json.dumps({"config": name, "envs": E, "ticks": T, "kernels_slowest_repeat_us": k["max_us"],
                              "framework_fastest_repeat_us": f["min_us"], "kernels_below_in_every_repeat": k["max_us"] < f["min_us"],
                              "framework_below_in_every_repeat": f["max_us"] < k["min_us"],
                              "ratio_of_medians": round(f["median_us"] / k["median_us"], 2)}), flush=True)
            for tr in trainers.values():
                tr.graceful_close()


if __name__ == "__main__":
    main()
