#!/usr/bin/env python3
"""Trainer's A2C update on its two paths -- "framework" (framework GEMMs, FusedObjective, autograd, clip_grad_norm_,
torch.optim.Adam, the repack) and "kernels" (`trainer.fused_update: "all"`: five launches,
training/pg_update_kernels.py) -- in ONE process on the one-launch rollout, at seven shapes: Cartpole E = 100 000 with
T = 10 (the shipped shape) and T = 50, single_acrobot as shipped (E = 100, T = 500), the learning test's Acrobot
E = 1000, T = 50, and TagGridWorld (training/pg_update_gridworld_kernels.py: five launches PER trained policy) at
tag_gridworld.yaml's E = 1000, T = 100 with [32, 32] and with [64, 64] policies, both trained, and at the learning test's
E = 600, T = 100 on a 20 x 20 grid with the taggers alone trained.

Per shape: two trainers, same seed.  Per repeat and path: `--warmup` iterations, then `--iterations` iterations; every
iteration is rollout, synchronise, device event, `_update_model_params(it, False)`, device event.  The paths alternate
inside a repeat.  One JSON line per (shape, path): the median of every repeat, and the median / min / max over the
repeats, of the update and of the whole iteration (rollout + update, host clock between two synchronisations); for the
kernels path also the device time of each of the five launches.  A last line per shape says whether the slowest repeat
of the kernels path is faster than the fastest repeat of the framework path.

    python scripts/pg_update_timing.py [--iterations 200] [--warmup 20] [--repeats 5] [--shapes 0,1,2,3,4,5,6]
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

# (env, replicas, ticks[, TagGridWorld: hidden width, trained policies, grid length])
SHAPES = (("cartpole", 100000, 10), ("cartpole", 100000, 50), ("acrobot", 100, 500), ("acrobot", 1000, 50),
          ("tag_gridworld", 1000, 100, 32, ("tagger", "runner"), 10), ("tag_gridworld", 1000, 100, 64, ("tagger", "runner"), 10),
          ("tag_gridworld", 600, 100, 32, ("tagger",), 20))


def build(env, E, T, fused, results_dir, width=None, trained=("shared",), grid_length=None):
    from warp_drive_amd.training.scripts.train import setup_trainer

    trainer = {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": 1, "fused_rollout_policy": "all"}
    if fused:
        trainer["fused_update"] = "all"
    ov = {"trainer": trainer, "saving": {"metrics_log_freq": 10 ** 9, "model_params_save_freq": 0}}
    name = f"single_{env}"
    if env == "tag_gridworld":
        name = env
        ov["env"] = {"grid_length": grid_length}
        ov["policy"] = {p: {"to_train": p in trained, "algorithm": "A2C", "vf_loss_coeff": 1, "entropy_coeff": 0.05, "gamma": 0.98,
                            "lr": 0.001, "model": {"type": "fully_connected", "fc_dims": [width, width], "model_ckpt_filepath": ""}}
                        for p in ("runner", "tagger")}
    torch.manual_seed(1)
    tr = setup_trainer(name, ov, results_dir=results_dir, verbose=False)
    assert tr._batch_rollout is not None
    assert all(tr.update_path[p] == ("kernels" if fused else "framework") for p in trained), tr.update_path
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


def per_launch(tr, count, pol):
    """device microseconds of each of the five launches of `pol` (medians), on the trainer's current batch"""
    k, T, pcfg = tr._pg_kernels[pol], tr.batch_len, tr.config["policy"][pol]
    b, flat, adam = tr.batch[pol], tr._pg_flat[pol], tr._pg_adam[pol]
    packed = tr._batch_rollout["packed"][pol]
    stages = {
        "values": lambda: k.compute_values(b["obs"][:T], flat.flat),
        "returns": lambda: k.discounted_returns(b["rewards"][:T], tr.done_batch[:T], pcfg["gamma"]),
        "gradients": lambda: k.gradients(b["obs"][:T], b["actions"][:T], flat.flat, pcfg["entropy_coeff"], pcfg["vf_loss_coeff"]),
        "reduce": k.reduce,
        "apply": lambda: k.apply(flat.flat, adam["exp_avg"], adam["exp_avg_sq"], adam["step"] + 1, pcfg["lr"],
                                 max_norm=pcfg["max_grad_norm"] if pcfg["clip_grad_norm"] else None, packed=packed)}
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
    ap.add_argument("--shapes", default=",".join(str(i) for i in range(len(SHAPES))))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    paths = ("framework", "kernels")
    for env, E, T, *more in [SHAPES[int(i)] for i in args.shapes.split(",")]:
        trained = more[1] if more else ("shared",)
        with tempfile.TemporaryDirectory() as tmp:
            trainers = {p: build(env, E, T, p == "kernels", os.path.join(tmp, p), *more) for p in paths}
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
                rows = {pol: E * T * len(trainers[p].policy_map[pol]) for pol in trained}
                records[p] = {"env": env, "envs": E, "ticks": T, "rows": sum(rows.values()), "path": p, "iterations": args.iterations,
                              "warmup": args.warmup, "repeats": args.repeats, "update": summary(update[p]),
                              "iteration": summary(whole[p])}
                if more:
                    records[p].update({"hidden": more[0], "trained": {pol: rows[pol] for pol in trained}})
                if p == "kernels":
                    launches = {pol: per_launch(trainers[p], 50, pol) for pol in trained}
                    records[p]["launch_us"] = launches if more else launches["shared"]
                print(json.dumps(records[p]), flush=True)
            k, f = records["kernels"]["update"], records["framework"]["update"]
            print(json.dumps({"env": env, "envs": E, "ticks": T, **({"hidden": more[0]} if more else {}), "kernels_slowest_repeat_us": k["max_us"],
                              "framework_fastest_repeat_us": f["min_us"], "kernels_faster": k["max_us"] < f["min_us"],
                              "ratio_of_medians": round(f["median_us"] / k["median_us"], 2)}), flush=True)
            for tr in trainers.values():
                tr.graceful_close()


if __name__ == "__main__":
    main()
