#!/usr/bin/env python3
"""The fused tick of a custom environment (include/wd_env_tick.h) against the per-tick launch plan, on
examples/rendezvous_fused/ at E = 2000 replicas of N = 100 agents, three plans in ONE process:

    "per tick"    sample_actions -> HipRendezvousFusedStep -> reset_when_done_fused, three launches per tick: what a
                  custom env without a Tick entry gets (docs/rounds/r33.md section 3 measured it at 13.9 us per tick)
    "one launch"  HipRendezvousFusedTick, one launch per tick (the multi-tick form switched off)
    "multi tick"  HipRendezvousFusedTick, ONE launch whose blocks loop over all ticks of the window

Method (r33's): device events around `--ticks` ticks replayed from C (`RolloutEngine.run`), after `--warmup` ticks, six
windows per plan, the plans alternating inside every round so that each sees the same drift of the clocks.  One JSON
line per plan with every window, then one line that says whether EVERY window of "one launch" lies below EVERY window of
"per tick".

    python scripts/custom_env_timing.py [--envs 2000] [--agents 100] [--ticks 2000] [--warmup 200] [--windows 6]
"""
import argparse
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANS = ("per tick", "one launch", "multi tick")


def fused_example():
    spec = importlib.util.spec_from_file_location(
        "rendezvous_fused_example", os.path.join(ROOT, "examples", "rendezvous_fused", "rendezvous_fused.py"))
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    return module


def build(plan, args, module):
    from warp_drive_amd import rollout
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders
    from warp_drive_amd.utils.env_registrar import EnvironmentRegistrar

    registrar = EnvironmentRegistrar()
    registrar.add(env_backend=["cpu", "hip"], cuda_env_src_path=module.SOURCE)(module.RendezvousFused)
    config = dict(num_agents=args.agents, grid_length=10, episode_length=20, seed=1, wall_penalty=0.125, spread_limit=-1)
    w = EnvWrapper(env_name="RendezvousFused", env_config=config, num_envs=args.envs, env_backend="hip",
                   env_registrar=registrar)
    w.reset_all_envs()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=3)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    saved = rollout.TICK_ROLLOUT
    rollout.TICK_ROLLOUT = 1 if plan == "multi tick" else 0
    try:
        engine = rollout.RolloutEngine(w, sampler, fused=plan != "per tick")
    finally:
        rollout.TICK_ROLLOUT = saved
    want = {"per tick": (["sample_actions[0]", "HipRendezvousFusedStep", "reset_when_done_fused"], None),
            "one launch": (["HipRendezvousFusedTick"], None),
            "multi tick": (["HipRendezvousFusedTick"], "HipRendezvousFusedTick")}[plan]
    assert (engine.entry_names, engine.rollout_kernel_name) == want, (plan, engine.entry_names, engine.rollout_kernel_name)
    return w, sampler, engine


def window(engine, ticks):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    engine.run(ticks)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / ticks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2000)
    ap.add_argument("--agents", type=int, default=100)
    ap.add_argument("--ticks", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--windows", type=int, default=6)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    module = fused_example()
    built = {plan: build(plan, args, module) for plan in PLANS}
    times = {plan: [] for plan in PLANS}
    for _ in range(args.windows):
        for plan in PLANS:  # alternating
            engine = built[plan][2]
            engine.run(args.warmup)
            torch.cuda.synchronize()
            times[plan].append(window(engine, args.ticks))
    for plan in PLANS:
        w, _, engine = built[plan]
        us = times[plan]
        print(json.dumps({"plan": plan, "entries": engine.entry_names, "multi_tick_entry": engine.rollout_kernel_name,
                          "envs": args.envs, "agents": args.agents, "ticks": args.ticks, "warmup": args.warmup,
                          "windows_us_per_tick": [round(v, 2) for v in us], "median_us_per_tick": round(float(np.median(us)), 2),
                          "min_us_per_tick": round(min(us), 2), "max_us_per_tick": round(max(us), 2),
                          "timestep_max": int(w.cuda_data_manager.pull_data_from_device("_timestep_").max())}), flush=True)
    med = {plan: float(np.median(times[plan])) for plan in PLANS}
    print(json.dumps({"every_one_launch_window_below_every_per_tick_window": max(times["one launch"]) < min(times["per tick"]),
                      "every_multi_tick_window_below_every_one_launch_window": max(times["multi tick"]) < min(times["one launch"]),
                      "per_tick_over_one_launch": round(med["per tick"] / med["one launch"], 2),
                      "per_tick_over_multi_tick": round(med["per tick"] / med["multi tick"], 2)}), flush=True)


if __name__ == "__main__":
    main()
