#!/usr/bin/env python3
"""`tag_gridworld_with_reset_pool` at its run config's shape (E = 2000, T = 100, one shared [32, 32] policy, grid 100) on
three settings in ONE process: "per tick" (no fused key: framework forward, sample, step, table reset, two pool
launches, undo per tick; the framework's update), "one launch" (`fused_rollout_policy: "all"`:
HipTagGridWorldRollout_N5P_H32, the framework's update) and "all keys" (+ `fused_update: "all"`, `fused_evaluation`).

Per repeat and setting: `--warmup` iterations, then `--iterations` iterations; every iteration is a device event, the
rollout, a device event, the update, a synchronisation.  The settings alternate inside a repeat.  One JSON line per
setting: the median of every repeat, and the median / min / max over the repeats, of the rollout per tick (device events)
and of the whole iteration (host clock between two synchronisations).  A last line says whether every repeat of the
one-launch rollout is below every repeat of the per-tick path.

Then the kernels alone, launched directly, T = 100 ticks per launch: HipTagGridWorldRollout_N5_H32 on `CUDATagGridWorld`
and HipTagGridWorldRollout_N5P_H32 on the env with the pool, both at grid 63, same E, same policy -- the cost of the
256-entry table and the pooled restart.

    python scripts/gridworld_pool_timing.py [--iterations 200] [--warmup 20] [--repeats 5]
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

SETTINGS = {"per tick": {}, "one launch": {"fused_rollout_policy": "all"},
            "all keys": {"fused_rollout_policy": "all", "fused_update": "all", "fused_evaluation": True}}


def build(keys, results_dir):
    from warp_drive_amd.training.scripts.train import setup_trainer

    ov = {"trainer": {"num_episodes": 10 ** 6, "seed": 1, **keys},
          "saving": {"metrics_log_freq": 10 ** 9, "model_params_save_freq": 0}}
    torch.manual_seed(1)
    return setup_trainer("tag_gridworld_with_reset_pool", ov, results_dir=results_dir, verbose=False)


def run(tr, first, count):
    """`count` iterations -> (rollout microseconds by device events, whole-iteration microseconds by the host clock)"""
    events, whole = [], []
    for it in range(first, first + count):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        tr._generate_rollout_batch()
        b.record()
        tr._update_model_params(it, False)
        torch.cuda.synchronize()
        whole.append(1e6 * (time.perf_counter() - t0))
        events.append((a, b))
    return [1e3 * a.elapsed_time(b) for a, b in events], whole


def summary(per_repeat, scale=1.0):
    med = [float(np.median(r)) * scale for r in per_repeat]
    return {"repeat_medians_us": [round(m, 2) for m in med], "median_us": round(float(np.median(med)), 2),
            "min_us": round(min(med), 2), "max_us": round(max(med), 2)}


def trainer_settings(args):
    with tempfile.TemporaryDirectory() as tmp:
        trainers = {name: build(keys, os.path.join(tmp, name.replace(" ", "_"))) for name, keys in SETTINGS.items()}
        assert trainers["per tick"]._batch_rollout is None and trainers["per tick"].update_path == {"shared": "framework"}
        for name in ("one launch", "all keys"):
            assert trainers[name].engine.step_kernel_name == "HipTagGridWorldRollout_N5P_H32"
        assert trainers["one launch"].update_path == {"shared": "framework"}
        assert trainers["all keys"].update_path == {"shared": "kernels"}
        T = trainers["per tick"].batch_len
        rollout = {name: [] for name in SETTINGS}
        whole = {name: [] for name in SETTINGS}
        it = 0
        for _ in range(args.repeats):
            for name, tr in trainers.items():   # alternating: every setting sees the same drift of the clocks
                run(tr, it, args.warmup)
                r, w = run(tr, it + args.warmup, args.iterations)
                rollout[name].append(r)
                whole[name].append(w)
            it += args.warmup + args.iterations
        records = {}
        for name, tr in trainers.items():
            records[name] = {"env": "tag_gridworld_with_reset_pool", "envs": tr.num_envs, "ticks": T, "setting": name,
                             "iterations": args.iterations, "warmup": args.warmup, "repeats": args.repeats,
                             "rollout_per_tick": summary(rollout[name], 1.0 / T), "iteration": summary(whole[name])}
            print(json.dumps(records[name]), flush=True)
        slow, fast = records["per tick"]["rollout_per_tick"], records["one launch"]["rollout_per_tick"]
        print(json.dumps({"one_launch_slowest_repeat_us_per_tick": fast["max_us"],
                          "per_tick_fastest_repeat_us_per_tick": slow["min_us"], "delivered": fast["max_us"] < slow["min_us"],
                          "ratio_of_medians": round(slow["median_us"] / fast["median_us"], 1)}), flush=True)
        for tr in trainers.values():
            tr.graceful_close()


def kernels_alone(args, E=2000, T=100, L=63):
    from tests.hip_harness import make_wrapper
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorld, CUDATagGridWorldWithResetPool
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.models import FullyConnected
    from warp_drive_amd.training.policy_kernel import pack_gridworld_policy

    torch.manual_seed(1)
    packed = pack_gridworld_policy(FullyConnected(21, [5], [32, 32])).cuda()
    cfg = dict(num_taggers=4, grid_length=L, episode_length=100, seed=20)
    launches = {}
    for cls in (CUDATagGridWorld, CUDATagGridWorldWithResetPool):
        w = make_wrapper(cls(**cfg), E)
        if cls is CUDATagGridWorldWithResetPool:
            w.init_reset_pool(seed=1)
        sampler = HIPSampler(w.cuda_function_manager)
        sampler.init_random(seed=2)
        w.env.ticks_per_launch = T
        batch = {"obs": torch.zeros((T, E, 5, 21), device="cuda"), "actions": torch.zeros((T, E, 5, 1), dtype=torch.int32, device="cuda"),
                 "rewards": torch.zeros((T, E, 5), device="cuda"), "done": torch.zeros((T, E), dtype=torch.int32, device="cuda")}
        probs = torch.full((E, 5, 5), 0.2, device="cuda")
        launches[cls.__name__] = (w, sampler, batch, w.env.tick_launch(sampler, [probs], w.env_resetter, batch=batch,
                                                                       policy=([packed, packed], 32)))
    times = {name: [] for name in launches}
    for _ in range(args.repeats):
        for name, (w, sampler, batch, (fn, a, block, grid, shared)) in launches.items():
            per = []
            for i in range(args.warmup + args.iterations):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                fn(*a, block=block, grid=grid, shared=shared)
                e.record()
                torch.cuda.synchronize()
                if i >= args.warmup:
                    per.append(1e3 * s.elapsed_time(e))
            times[name].append(per)
    for name, (w, sampler, batch, (fn, a, block, grid, shared)) in launches.items():
        print(json.dumps({"kernel": fn.name, "env": name, "envs": E, "ticks": T, "grid_length": L, "lds_bytes": shared,
                          "blocks": grid[0], "finished_per_launch": int((batch["done"] > 0).sum()),
                          "per_tick": summary(times[name], 1.0 / T)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    trainer_settings(args)
    kernels_alone(args)


if __name__ == "__main__":
    main()
