#!/usr/bin/env python3
"""TrainerDDPG's update on its three paths -- "framework" (autograd, clip_grad_norm_, two Adams, soft_update), "kernels"
(`trainer.fused_update: true`: four launches, training/ddpg_update_kernels.py) and "matrix" (the same with
`trainer.fused_update_gradients: "matrix"`: the gradient launch on the float32 matrix cores) -- in ONE process, at shapes
of single_pendulum on the one-launch rollout: E = 10 000 with T = 5, the shipped config's E = 1000 with T = 10, and
E = 100 000 with T = 5; `--width 32` measures [32, 32] networks.

Per shape: three trainers, same seed.  Per repeat and path: `--warmup` iterations, then `--iterations` iterations; every
iteration is rollout, synchronise, device event, `_update_model_params(it, False)`, device event.  The paths alternate
inside a repeat.  One JSON line per (shape, path): the median of every repeat, and the median / min / max over the
repeats, of the update and of the whole iteration (rollout + update, host clock between two synchronisations); for the
kernels and matrix paths also the device time of each of the four launches.  The last lines per shape say whether the
slowest repeat of the kernels path is faster than the fastest repeat of the framework path, and whether the slowest repeat
of the matrix path is faster than the fastest repeat of the kernels path.

    python scripts/ddpg_update_timing.py [--iterations 200] [--warmup 20] [--repeats 5] [--width 64] [--shapes 0 1 2]
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

SHAPES = ((10000, 5), (1000, 10), (100000, 5))
PATHS = ("framework", "kernels", "matrix")


def build(E, T, path, results_dir, width=64):
    from warp_drive_amd.training.scripts.train import setup_trainer

    trainer = {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": 1, "fused_rollout_policy": "all"}
    fused = path != "framework"
    if fused:
        trainer["fused_update"] = True
    if path == "matrix":
        trainer["fused_update_gradients"] = "matrix"
    ov = {"trainer": trainer, "saving": {"metrics_log_freq": 10 ** 9, "model_params_save_freq": 0}}
    if width != 64:
        # (an override replaces the policy's entry: single_pendulum.yaml's, with the other width)
        net = lambda kind: {"type": kind, "fc_dims": [width, width], "model_ckpt_filepath": ""}  # noqa: E731
        ov["policy"] = {"shared": {"to_train": True, "algorithm": "DDPG", "clip_grad_norm": True, "max_grad_norm": 3,
                                   "normalize_advantage": False, "normalize_return": False, "gamma": 0.99, "tau": 0.05,
                                   "lr": {"actor": 0.001, "critic": 0.001},
                                   "model": {"actor": net("fully_connected_actor"),
                                             "critic": net("fully_connected_action_value_critic")}}}
    torch.manual_seed(1)
    tr = setup_trainer("single_pendulum", ov, results_dir=results_dir, verbose=False)
    assert tr.rollout_path == "one launch" and tr.update_path == ("kernels" if fused else "framework")
    assert tr.update_gradients_path == {"framework": None, "kernels": "lanes", "matrix": "matrix"}[path]
    return tr


def run(tr, first, count):
    """`count` iterations -> (update microseconds by device events, whole-iteration microseconds by the host clock)"""
    events, whole = [], []
    for it in range(first, first + count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr._generate_rollout_batch()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr._update_model_params(it, False)
        b.record()
        torch.cuda.synchronize()
        whole.append(1e6 * (time.perf_counter() - t0))
        events.append((a, b))
    return [1e3 * a.elapsed_time(b) for a, b in events], whole


def per_launch(tr, count):
    """device microseconds of each of the four launches (medians), on the trainer's current batch"""
    pol = tr.policies[0]
    k, T, pcfg = tr._update_kernels, tr.batch_len, tr.config["policy"][pol]
    b = tr.batch[pol]
    scale, bias = tr._actor_range
    packed = tr._batch_rollout["packed"][pol]
    stages = {
        "targets": lambda: k.targets(b["obs"][:T], tr._flat_target.flat, scale, bias),
        "gradients": lambda: k.gradients(b["obs"][:T], b["actions"][:T], b["rewards"][:T], tr.done_batch[:T], k.next_values,
                                         tr._flat.flat, pcfg["gamma"], scale, bias),
        "reduce": k.reduce,
        "apply": lambda: k.apply(tr._flat.flat, tr._flat_target.flat, tr._adam["exp_avg"], tr._adam["exp_avg_sq"],
                                 tr._adam["step"] + 1, 1e-3, 1e-3, tr.tau, max_norm=pcfg["max_grad_norm"], packed=packed)}
    out = {}
    for name, fn in stages.items():
        times = []
        for _ in range(count):
            torch.cuda.synchronize()
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            times.append(1e3 * a.elapsed_time(e))
        out[name] = round(float(np.median(times)), 1)
    return out


def summary(per_repeat):
    med = [float(np.median(r)) for r in per_repeat]
    return {"repeat_medians_us": [round(m, 1) for m in med], "median_us": round(float(np.median(med)), 1),
            "min_us": round(min(med), 1), "max_us": round(max(med), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--shapes", type=int, nargs="*", default=list(range(len(SHAPES))))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    paths = PATHS
    for E, T in (SHAPES[i] for i in args.shapes):
        with tempfile.TemporaryDirectory() as tmp:
            trainers = {p: build(E, T, p, os.path.join(tmp, p), args.width) for p in paths}
            update = {p: [] for p in paths}
            whole = {p: [] for p in paths}
            it = 0
            for _ in range(args.repeats):
                for p in paths:   # alternating: both paths see the same drift of the clocks
                    run(trainers[p], it, args.warmup)
                    u, w = run(trainers[p], it + args.warmup, args.iterations)
                    update[p].append(u)
                    whole[p].append(w)
                it += args.warmup + args.iterations
            records = {}
            for p in paths:
                records[p] = {"envs": E, "ticks": T, "n_step": trainers[p].n_step, "width": args.width, "path": p, "iterations": args.iterations,
                              "warmup": args.warmup, "repeats": args.repeats, "update": summary(update[p]),
                              "iteration": summary(whole[p])}
                if p != "framework":
                    records[p]["launch_us"] = per_launch(trainers[p], 50)
                print(json.dumps(records[p]), flush=True)
            k, f = records["kernels"]["update"], records["framework"]["update"]
            print(json.dumps({"envs": E, "ticks": T, "kernels_slowest_repeat_us": k["max_us"],
                              "framework_fastest_repeat_us": f["min_us"], "kernels_faster": k["max_us"] < f["min_us"],
                              "ratio_of_medians": round(f["median_us"] / k["median_us"], 2)}), flush=True)
            m = records["matrix"]["update"]
            print(json.dumps({"envs": E, "ticks": T, "width": args.width, "matrix_slowest_repeat_us": m["max_us"],
                              "kernels_fastest_repeat_us": k["min_us"], "matrix_faster": m["max_us"] < k["min_us"],
                              "ratio_of_medians": round(k["median_us"] / m["median_us"], 2)}), flush=True)
            for tr in trainers.values():
                tr.graceful_close()


if __name__ == "__main__":
    main()
