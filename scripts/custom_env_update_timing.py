#!/usr/bin/env python3
"""The A2C / PPO update of a custom environment as kernels (include/wd_env_update.h) against the framework's update, on
examples/rendezvous_update/ at N = 100 agents and a batch of 20 ticks: E = 2000 replicas (4 M rows) and E = 200 (400 k
rows), per hidden width three plans in ONE process, all on the one-launch rollout:

    "framework"    `trainer.fused_update` unset: the update in framework ops -- the parent commit's path, the yardstick
    "kernels x1"   `trainer.fused_update: "all"`: five launches, the gradient launch on ONE block per compute unit
    "kernels x2"   the same with TWO blocks per compute unit (PgCustomUpdateKernels' `blocks_per_cu`)

Method (scripts/custom_env_rollout_timing.py's): device events around `--updates` calls of `Trainer._update_model_params`
(non-logging) on a rolled-out batch, after `--warmup` calls, six windows per plan, the plans alternating inside every round
so that each sees the same drift of the clocks.  One JSON line per plan with every window (ms per update) and the time of
a whole training iteration (rollout + update, host time between two synchronisations), then one line per shape and width
that says, for each kernel plan, whether EVERY window of it lies below EVERY window of the framework's, and whether every
window of "kernels x2" lies below every window of "kernels x1".  Nothing gates on the times.

    python scripts/custom_env_update_timing.py [--envs 2000 200] [--agents 100] [--batch 20] [--updates 20] [--warmup 3]
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

PLANS = ("framework", "kernels x1", "kernels x2")
BLOCKS_PER_CU = {"kernels x1": 1, "kernels x2": 2}
POLICY = "shared"


def update_example():
    spec = importlib.util.spec_from_file_location(
        "rendezvous_update_example", os.path.join(ROOT, "examples", "rendezvous_update", "rendezvous_update.py"))
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    return module


def build(plan, width, envs, args, module, results_dir):
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.training.trainer import Trainer
    from warp_drive_amd.utils.env_registrar import EnvironmentRegistrar

    registrar = EnvironmentRegistrar()
    registrar.add(env_backend=["cpu", "hip"], cuda_env_src_path=module.SOURCE)(module.RendezvousUpdate)
    env_config = dict(num_agents=args.agents, grid_length=10, episode_length=20, seed=1, wall_penalty=0.125,
                      spread_limit=-1)
    w = EnvWrapper(env_name="RendezvousUpdate", env_config=env_config, num_envs=envs, env_backend="hip",
                   env_registrar=registrar)
    trainer_config = {"num_envs": envs, "train_batch_size": envs * args.batch, "num_episodes": 10 ** 7, "seed": 7,
                      "fused_rollout_policy": "all"}
    if plan != "framework":
        trainer_config["fused_update"] = "all"
    config = {"name": "rendezvous_update", "trainer": trainer_config,
              "policy": {POLICY: {"to_train": True, "algorithm": "A2C", "lr": 0.001, "vf_loss_coeff": 1, "gamma": 0.98,
                                  "entropy_coeff": 0.05, "clip_grad_norm": True, "max_grad_norm": 3,
                                  "normalize_advantage": False, "normalize_return": False,
                                  "model": {"type": "fully_connected", "fc_dims": [width, width]}}},
              "saving": {"metrics_log_freq": 10 ** 6, "model_params_save_freq": 0, "basedir": results_dir,
                         "name": "rendezvous_update", "tag": f"{plan.replace(' ', '_')}_{width}_{envs}"}}
    torch.manual_seed(0)
    trainer = Trainer(env_wrapper=w, config=config, policy_tag_to_agent_id_map={POLICY: list(range(args.agents))},
                      results_dir=results_dir, verbose=False)
    assert trainer.rollout_path == "one launch", trainer.rollout_path
    want = "framework" if plan == "framework" else "kernels"
    assert trainer.update_path == {POLICY: want}, (plan, trainer.update_path)
    if plan != "framework":
        k = trainer._pg_kernels[POLICY]
        trainer._pg_kernels[POLICY] = w.env.update_kernels(envs, args.batch, args.agents, k.H, k.O, k.A, trainer.device,
                                                           blocks_per_cu=BLOCKS_PER_CU[plan])
    return trainer


def run_updates(trainer, n):
    for i in range(n):
        trainer._update_model_params(i, False)


def window(trainer, updates):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run_updates(trainer, updates)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / updates


def iteration_ms(trainer, iterations):
    trainer.train(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    trainer.train(iterations)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iterations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[2000, 200])
    ap.add_argument("--agents", type=int, default=100)
    ap.add_argument("--batch", type=int, default=20, help="ticks of a training batch")
    ap.add_argument("--updates", type=int, default=20, help="updates per window")
    ap.add_argument("--warmup", type=int, default=3, help="updates before every window")
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--iterations", type=int, default=5, help="training iterations of the whole-iteration time")
    ap.add_argument("--widths", type=int, nargs="+", default=[32, 64])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    module = update_example()
    with tempfile.TemporaryDirectory() as results_dir:
        for envs in args.envs:
            for width in args.widths:
                built = {plan: build(plan, width, envs, args, module, results_dir) for plan in PLANS}
                for trainer in built.values():
                    trainer._generate_rollout_batch()
                torch.cuda.synchronize()
                times = {plan: [] for plan in PLANS}
                for _ in range(args.windows):
                    for plan in PLANS:  # alternating
                        run_updates(built[plan], args.warmup)
                        torch.cuda.synchronize()
                        times[plan].append(window(built[plan], args.updates))
                whole = {plan: iteration_ms(built[plan], args.iterations) for plan in PLANS}
                rows = envs * args.agents * args.batch
                for plan in PLANS:
                    ms = times[plan]
                    k = built[plan]._pg_kernels.get(POLICY)
                    print(json.dumps({"plan": plan, "width": width, "envs": envs, "agents": args.agents,
                                      "batch_ticks": args.batch, "rows": rows,
                                      "gradient_blocks": None if k is None else k.gradients_grid,
                                      "updates_per_window": args.updates, "warmup_updates": args.warmup,
                                      "windows_ms_per_update": [round(v, 3) for v in ms],
                                      "median_ms_per_update": round(float(np.median(ms)), 3), "min_ms_per_update": round(min(ms), 3),
                                      "max_ms_per_update": round(max(ms), 3), "iteration_ms": round(whole[plan], 2)}), flush=True)
                med = {plan: float(np.median(times[plan])) for plan in PLANS}
                below = lambda a, b: max(times[a]) < min(times[b])   # noqa: E731
                print(json.dumps({"width": width, "envs": envs, "rows": rows,
                                  "every_x1_window_below_every_framework_window": below("kernels x1", "framework"),
                                  "every_x2_window_below_every_framework_window": below("kernels x2", "framework"),
                                  "every_x2_window_below_every_x1_window": below("kernels x2", "kernels x1"),
                                  "framework_over_x1": round(med["framework"] / med["kernels x1"], 2),
                                  "framework_over_x2": round(med["framework"] / med["kernels x2"], 2),
                                  "iteration_framework_over_x1": round(whole["framework"] / whole["kernels x1"], 2),
                                  "iteration_framework_over_x2": round(whole["framework"] / whole["kernels x2"], 2)}),
                      flush=True)
                for trainer in built.values():
                    trainer.graceful_close()
                del built
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
