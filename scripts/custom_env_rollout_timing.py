#!/usr/bin/env python3
"""The one-launch rollout of a custom environment with the policy inside the kernel (include/wd_env_rollout.h) against the
per-tick path, on examples/rendezvous_policy/ at E = 2000 replicas of N = 100 agents, `Trainer`'s rollout generation of a
batch of 20 ticks, per hidden width two plans in ONE process:

    "per tick"    `trainer.fused_rollout_policy` unset: the framework's policy forward, then HipRendezvousPolicyTick,
                  per tick -- what the class gets without the Rollout entries (the path RendezvousFused takes)
    "one launch"  `trainer.fused_rollout_policy: "all"`: HipRendezvousPolicyRollout_H<width>, ONE launch per batch; the
                  time includes the repack of the policy and the episodic bookkeeping over the recorded rows

Method (scripts/custom_env_timing.py's): device events around `--batches` calls of `Trainer._generate_rollout_batch`,
after `--warmup` calls, six windows per plan, the plans alternating inside every round so that each sees the same drift
of the clocks.  One JSON line per plan with every window (us per tick) and the time of a whole training iteration
(rollout + update, host time between two synchronisations), then one line per width that says whether EVERY window of
"one launch" lies below EVERY window of "per tick".

    python scripts/custom_env_rollout_timing.py [--envs 2000] [--agents 100] [--batch 20] [--batches 200] [--warmup 10]
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANS = ("per tick", "one launch")


def policy_example():
    spec = importlib.util.spec_from_file_location(
        "rendezvous_policy_example", os.path.join(ROOT, "examples", "rendezvous_policy", "rendezvous_policy.py"))
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    return module


def build(plan, width, args, module, results_dir):
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.training.trainer import Trainer
    from warp_drive_amd.utils.env_registrar import EnvironmentRegistrar

    registrar = EnvironmentRegistrar()
    registrar.add(env_backend=["cpu", "hip"], cuda_env_src_path=module.SOURCE)(module.RendezvousPolicy)
    env_config = dict(num_agents=args.agents, grid_length=10, episode_length=20, seed=1, wall_penalty=0.125,
                      spread_limit=-1)
    w = EnvWrapper(env_name="RendezvousPolicy", env_config=env_config, num_envs=args.envs, env_backend="hip",
                   env_registrar=registrar)
    trainer_config = {"num_envs": args.envs, "train_batch_size": args.envs * args.batch, "num_episodes": 10 ** 7, "seed": 7}
    if plan == "one launch":
        trainer_config["fused_rollout_policy"] = "all"
    config = {"name": "rendezvous_policy", "trainer": trainer_config,
              "policy": {"shared": {"to_train": True, "algorithm": "A2C", "lr": 0.001, "vf_loss_coeff": 1, "gamma": 0.98,
                                    "model": {"type": "fully_connected", "fc_dims": [width, width]}}},
              "saving": {"metrics_log_freq": 10 ** 6, "model_params_save_freq": 0, "basedir": results_dir,
                         "name": "rendezvous_policy", "tag": f"{plan.replace(' ', '_')}_{width}"}}
    torch.manual_seed(0)
    trainer = Trainer(env_wrapper=w, config=config, policy_tag_to_agent_id_map={"shared": list(range(args.agents))},
                      results_dir=results_dir, verbose=False)
    want = {"per tick": ("per tick", ["HipRendezvousPolicyTick"]),
            "one launch": ("one launch", [f"HipRendezvousPolicyRollout_H{width}"])}[plan]
    assert (trainer.rollout_path, trainer.engine.entry_names) == want, (plan, trainer.rollout_path, trainer.engine.entry_names)
    return trainer


def window(trainer, batches, ticks_per_batch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(batches):
        trainer._generate_rollout_batch()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / (batches * ticks_per_batch)


def iteration_ms(trainer, iterations):
    trainer.train(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.train(iterations)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iterations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2000)
    ap.add_argument("--agents", type=int, default=100)
    ap.add_argument("--batch", type=int, default=20, help="ticks of a training batch")
    ap.add_argument("--batches", type=int, default=200, help="batches per window")
    ap.add_argument("--warmup", type=int, default=10, help="batches before every window")
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--iterations", type=int, default=5, help="training iterations of the whole-iteration time")
    ap.add_argument("--widths", type=int, nargs="+", default=[32, 64])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    module = policy_example()
    with tempfile.TemporaryDirectory() as results_dir:
        for width in args.widths:
            built = {plan: build(plan, width, args, module, results_dir) for plan in PLANS}
            times = {plan: [] for plan in PLANS}
            for _ in range(args.windows):
                for plan in PLANS:  # alternating
                    for _ in range(args.warmup):
                        built[plan]._generate_rollout_batch()
                    torch.cuda.synchronize()
                    times[plan].append(window(built[plan], args.batches, args.batch))
            whole = {plan: iteration_ms(built[plan], args.iterations) for plan in PLANS}
            for plan in PLANS:
                us = times[plan]
                print(json.dumps({"plan": plan, "width": width, "entries": built[plan].engine.entry_names,
                                  "envs": args.envs, "agents": args.agents, "batch_ticks": args.batch,
                                  "batches_per_window": args.batches, "warmup_batches": args.warmup,
                                  "windows_us_per_tick": [round(v, 2) for v in us],
                                  "median_us_per_tick": round(float(np.median(us)), 2), "min_us_per_tick": round(min(us), 2),
                                  "max_us_per_tick": round(max(us), 2), "iteration_ms": round(whole[plan], 2)}), flush=True)
            med = {plan: float(np.median(times[plan])) for plan in PLANS}
            print(json.dumps({"width": width,
                              "every_one_launch_window_below_every_per_tick_window":
                                  max(times["one launch"]) < min(times["per tick"]),
                              "per_tick_over_one_launch": round(med["per tick"] / med["one launch"], 2),
                              "iteration_per_tick_over_one_launch": round(whole["per tick"] / whole["one launch"], 2)}),
                  flush=True)
            for trainer in built.values():
                trainer.graceful_close()


if __name__ == "__main__":
    main()
