#!/usr/bin/env python3
"""Cartpole with a reset pool (`single_cartpole_with_reset_pool`): what the one-launch rollout costs against the per-tick
plan, and what the pooled restart costs over the unpooled rollout.

Trainer settings, ONE setting per process (`--setting`), or -- without `--setting` -- `--repeats` fresh child processes
of every setting, alternating (the parent never touches the GPU):
  "per tick"    no fused key: framework forward, sample, step, table reset, pool launch, undo per tick; the framework's
                update (what a pooled Cartpole ran before the ..._P entries existed)
  "one launch"  `fused_rollout_policy: "all"`: HipClassicControlCartPoleEnvRollout_P_H32, the framework's update
  "all keys"    + `fused_update: "all"`, `fused_evaluation`
  "unpooled"    `single_cartpole` at the same shape on its default one launch (..._Rollout_H32): the floor
at `--shape config` (E = 100 000, T = 10, the run config's) or `--shape long` (E = 1000, T = 50, episode length 200).
Per process: `--warmup` iterations, then `--iterations`; every iteration is a device event, the rollout, a device event,
the update, a synchronisation.  One JSON line: the median rollout per tick (device events) and the median iteration
(host clock between two synchronisations).  The parent prints every child's line, a summary per setting, and whether
EVERY repeat of the one launch lies below EVERY repeat of the per-tick plan.

`--kernels`: the entries alone, launched directly at both shapes with the same [32, 32] policy: the unpooled
..._Rollout_H32, ..._P_H32 with the 1000-row pool staged in LDS and with the pool in global memory; "steady" = launch
after launch of a random policy (episodes of about 20 ticks: a restart in nearly every wavefront and tick), "from rest" =
every timed launch starts all replicas from pool rows at time step 0 (restarts are rare within the first ticks: what a
trained policy's launches look like).

    python scripts/cartpole_pool_timing.py [--shape config] [--iterations 50] [--warmup 10] [--repeats 5]
    python scripts/cartpole_pool_timing.py --kernels
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {"per tick": {}, "one launch": {"fused_rollout_policy": "all"},
            "all keys": {"fused_rollout_policy": "all", "fused_update": "all", "fused_evaluation": True},
            "unpooled": {}}
SHAPES = {"config": {"trainer": {}, "env": {}},
          "long": {"trainer": {"num_envs": 1000, "train_batch_size": 1000 * 50}, "env": {"episode_length": 200}}}


def one_setting(args):
    import torch
    from warp_drive_amd.training.scripts.train import setup_trainer

    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    shape = SHAPES[args.shape]
    ov = {"trainer": {"num_episodes": 10 ** 6, "seed": 1, **shape["trainer"], **SETTINGS[args.setting]},
          "env": dict(shape["env"]), "saving": {"metrics_log_freq": 10 ** 9, "model_params_save_freq": 0}}
    torch.manual_seed(1)
    with tempfile.TemporaryDirectory() as tmp:
        name = "single_cartpole" if args.setting == "unpooled" else "single_cartpole_with_reset_pool"
        tr = setup_trainer(name, ov, results_dir=tmp, verbose=False)
        want = {"per tick": "HipClassicControlCartPoleEnvStep", "unpooled": "HipClassicControlCartPoleEnvRollout_H32"}
        assert tr.engine.step_kernel_name == want.get(args.setting, "HipClassicControlCartPoleEnvRollout_P_H32")
        assert tr.update_path == {"shared": "kernels" if args.setting == "all keys" else "framework"}
        events, whole = [], []
        for it in range(args.warmup + args.iterations):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            tr._generate_rollout_batch()
            b.record()
            tr._update_model_params(it, False)
            torch.cuda.synchronize()
            if it >= args.warmup:
                whole.append(1e6 * (time.perf_counter() - t0))
                events.append(1e3 * a.elapsed_time(b))
        T = tr.batch_len
        print(json.dumps({"setting": args.setting, "shape": args.shape, "envs": tr.num_envs, "ticks": T,
                          "kernel": tr.engine.step_kernel_name, "iterations": args.iterations, "warmup": args.warmup,
                          "rollout_us_per_tick": round(float(np.median(events)) / T, 3),
                          "iteration_us": round(float(np.median(whole)), 1),
                          "restarts_per_tick_and_replica": round(float((tr.done_batch[:T] > 0).float().mean()), 4)}), flush=True)
        tr.graceful_close()


def all_settings(args):
    results = {name: [] for name in SETTINGS}
    for _ in range(args.repeats):
        for name in SETTINGS:   # alternating: every setting sees the same drift of the clocks
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--setting", name, "--shape", args.shape,
                                  "--iterations", str(args.iterations), "--warmup", str(args.warmup)],
                                 check=True, capture_output=True, text=True, timeout=args.child_timeout).stdout
            line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
            print(line, flush=True)
            results[name].append(json.loads(line))
    for name, recs in results.items():
        r, w = [x["rollout_us_per_tick"] for x in recs], [x["iteration_us"] for x in recs]
        print(json.dumps({"summary": name, "shape": args.shape, "repeats": args.repeats,
                          "rollout_us_per_tick": {"median": float(np.median(r)), "min": min(r), "max": max(r)},
                          "iteration_us": {"median": float(np.median(w)), "min": min(w), "max": max(w)}}), flush=True)
    for key in ("rollout_us_per_tick", "iteration_us"):
        slow = [x[key] for x in results["per tick"]]
        for name in ("one launch", "all keys"):
            fast = [x[key] for x in results[name]]
            print(json.dumps({"claim": f"{name} below per tick, every repeat, {key}", "shape": args.shape,
                              "slowest_" + name.replace(" ", "_"): max(fast), "fastest_per_tick": min(slow),
                              "holds": max(fast) < min(slow),
                              "ratio_of_medians": round(float(np.median(slow) / np.median(fast)), 2)}), flush=True)


def kernels_alone(args):
    import torch
    from tests.hip_harness import make_wrapper
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.models import FullyConnected
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    torch.manual_seed(1)
    packed = pack_rollout_policy(FullyConnected(4, [2], [32, 32])).cuda()
    for E, T, length in ((100000, 10, 500), (1000, 50, 200)):
        launches = {}
        for name, pool, placement in (("unpooled", 0, None), ("pool staged in LDS", 1000, "lds"),
                                      ("pool in global memory", 1000, "global")):
            w = make_wrapper(CUDAClassicControlCartPoleEnv(episode_length=length, seed=5, reset_pool_size=pool), E)
            if pool:
                w.init_reset_pool(seed=1)
                w.env.pool_placement = placement
            sampler = HIPSampler(w.cuda_function_manager)
            sampler.init_random(seed=2)
            w.env.ticks_per_launch = T
            batch = {"obs": torch.zeros((T, E, 1, 4), device="cuda"),
                     "actions": torch.zeros((T, E, 1, 1), dtype=torch.int32, device="cuda"),
                     "rewards": torch.zeros((T, E, 1), device="cuda"), "done": torch.zeros((T, E), dtype=torch.int32, device="cuda")}
            probs = torch.full((E, 1, 2), 0.5, device="cuda")
            dm = w.cuda_data_manager
            rest = {n: np.ascontiguousarray(dm.pull_data_from_device(n)).copy() for n in ("state", "observations", "_timestep_")}
            # (the sampler is kept: its RNG words are freed with it)
            launches[name] = (w, sampler, batch, rest, w.env.tick_launch(sampler, [probs], w.env_resetter, batch=batch, policy=(packed, 32)))
        for mode in ("steady", "from rest"):
            times = {name: [] for name in launches}
            finished = {}
            for _ in range(args.repeats):
                for name, (w, sampler, batch, rest, (fn, a, block, grid, shared)) in launches.items():
                    per = []
                    for i in range(args.warmup + args.iterations):
                        if mode == "from rest":
                            for n, t in rest.items():
                                drv.memcpy_htod(w.cuda_data_manager.device_data(n), t)
                            torch.cuda.synchronize()
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        fn(*a, block=block, grid=grid, shared=shared)
                        e.record()
                        torch.cuda.synchronize()
                        if i >= args.warmup:
                            per.append(1e3 * s.elapsed_time(e))
                    times[name].append(float(np.median(per)) / T)
                    finished[name] = float((batch["done"] > 0).float().mean())
            for name, (w, sampler, batch, rest, (fn, a, block, grid, shared)) in launches.items():
                t = times[name]
                print(json.dumps({"kernel": fn.name, "pool": name, "mode": mode, "envs": E, "ticks": T, "lds_bytes": shared,
                                  "restarts_per_tick_and_replica": round(finished[name], 4),
                                  "us_per_tick": {"repeat_medians": [round(x, 3) for x in t],
                                                  "median": round(float(np.median(t)), 3), "min": round(min(t), 3),
                                                  "max": round(max(t), 3)}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--setting", choices=sorted(SETTINGS), default=None)
    ap.add_argument("--shape", choices=sorted(SHAPES), default="config")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.kernels:
        kernels_alone(args)
    elif args.setting is not None:
        one_setting(args)
    else:
        all_settings(args)


if __name__ == "__main__":
    main()
