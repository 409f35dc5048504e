#!/usr/bin/env python3
"""Trainer's A2C update under `trainer.neg_pos_env_ratio` on its two paths -- "framework" (what `trainer.fused_update: "all"`
alone leaves such a trainer on: two nonzero().tolist() round trips, a host np.random.choice, five fancy-index gathers) and
"kernels" (with `trainer.fused_update_downsample: true`: three launches of csrc/kernels/pg_downsample.hip, one read-back of
three integers, then the five update launches on the kept columns) -- in ONE process on MountainCar's one-launch rollout,
E = 1000, T = 500, [32, 32], neg_pos_env_ratio 10, by scripts/pg_update_timing.py's method (device events around
`_update_model_params`, the paths alternating inside a repeat).  Nobody has measured how many MountainCar replicas reach
the goal early in training: after every rollout `--positives` (default 20 = 2 %) seeded replicas are given done == 2 on
the last tick, so both paths keep 20 + 200 of the 1000 columns.  One JSON line per path, for the kernels path with the
device time of the three new launches alone, and a last line: whether every repeat of one path is below every repeat of
the other.

    python scripts/pg_downsample_timing.py [--iterations 200] [--warmup 20] [--repeats 5] [--positives 20]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.pg_update_timing import summary  # noqa: E402

ENV, E, T, RATIO = "single_mountain_car", 1000, 500, 10


def build(path, results_dir):
    from warp_drive_amd.training.scripts.train import setup_trainer

    trainer = {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": 1, "fused_rollout_policy": "all",
               "fused_update": "all", "neg_pos_env_ratio": RATIO, "fused_update_downsample": path == "kernels"}
    ov = {"trainer": trainer, "saving": {"metrics_log_freq": 10 ** 9, "model_params_save_freq": 0}}
    torch.manual_seed(1)   # (the shipped policy: A2C, [32, 32], no normalisation)
    tr = setup_trainer(ENV, ov, results_dir=results_dir, verbose=False)
    assert tr._batch_rollout is not None and tr.update_path == {"shared": path}, (tr.rollout_path, tr.update_path)
    return tr


def run(tr, first, count, positives):
    """`count` iterations, each a rollout, the positives written into its done flags, then the timed update -> microseconds"""
    events = []
    for it in range(first, first + count):
        tr._generate_rollout_batch()
        tr.done_batch[T - 1, positives] = 2
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr._update_model_params(it, False)
        b.record()
        torch.cuda.synchronize()
        events.append(1e3 * a.elapsed_time(b))
    return events


def new_launches(tr, count):
    """device microseconds (median / min / max) of scan + keep and of the gather alone, on the trainer's last batch"""
    k, b, done = tr._pg_kernels["shared"], tr.batch["shared"], tr.done_batch[:T]
    k.downsample(done, RATIO, 0, b["obs"][:T], b["actions"][:T], b["rewards"][:T], seed_words=tr._seed_words)
    K = k.E
    pairs = [(b["obs"][:T], k._kept["obs"][:T * K * 2]), (b["actions"][:T], k._kept["actions"][:T * K]),
             (b["rewards"][:T], k._kept["rewards"][:T * K]), (done, k._kept["done"][:T * K])]
    stages = {"scan": lambda: k.select_scan(done, 0, tr._seed_words), "keep": lambda: k.select_keep(RATIO),
              "gather": lambda: k.gather_columns(K, pairs)}
    out = {"kept_columns": K}
    for name, launch in stages.items():
        times = []
        for _ in range(count):
            torch.cuda.synchronize()
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch()
            e.record()
            torch.cuda.synchronize()
            times.append(1e3 * a.elapsed_time(e))
        out[name] = {"median_us": round(float(np.median(times)), 1), "min_us": round(min(times), 1), "max_us": round(max(times), 1)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--positives", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    paths = ("framework", "kernels")
    positives = torch.from_numpy(np.sort(np.random.default_rng(53).choice(E, args.positives, replace=False))).cuda()
    with tempfile.TemporaryDirectory() as tmp:
        trainers = {p: build(p, os.path.join(tmp, p)) for p in paths}
        update, it = {p: [] for p in paths}, 0
        for _ in range(args.repeats):
            for p in paths:   # alternating: both paths see the same drift of the clocks
                run(trainers[p], it, args.warmup, positives)
                update[p].append(run(trainers[p], it + args.warmup, args.iterations, positives))
            it += args.warmup + args.iterations
        records = {}
        for p in paths:
            records[p] = {"config": ENV, "envs": E, "ticks": T, "neg_pos_env_ratio": RATIO, "positives": args.positives,
                          "positive_share": args.positives / E, "path": p, "iterations": args.iterations,
                          "warmup": args.warmup, "repeats": args.repeats, "update": summary(update[p])}
            if p == "kernels":
                records[p]["sampled"] = trainers[p]._pg_kernels["shared"].sampled
                records[p]["new_launches_us"] = new_launches(trainers[p], 100)
            print(json.dumps(records[p]), flush=True)
        k, f = records["kernels"]["update"], records["framework"]["update"]
        print(json.dumps({"config": ENV, "envs": E, "ticks": T, "kernels_slowest_repeat_us": k["max_us"],
                          "framework_fastest_repeat_us": f["min_us"], "kernels_below_in_every_repeat": k["max_us"] < f["min_us"],
                          "framework_below_in_every_repeat": f["max_us"] < k["min_us"],
                          "ratio_of_medians": round(f["median_us"] / k["median_us"], 2)}), flush=True)
        for tr in trainers.values():
            tr.graceful_close()


if __name__ == "__main__":
    main()
