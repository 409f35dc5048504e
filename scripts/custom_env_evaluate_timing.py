#!/usr/bin/env python3
"""`Trainer.evaluate_episodes` of a custom environment in ONE launch (include/wd_env_evaluate.h) against the per-tick path,
at E = 2000 replicas of N = 100 agents, grid 10, episodes of 20 ticks (scripts/custom_env_rollout_timing.py's config), greedy
and sampled, per hidden width two plans in ONE process, both under `trainer.fused_rollout_policy: "all"`:

    "per tick"    examples/rendezvous_update/: the class trains in kernels and has no Evaluate entries, so an evaluation is
                  `episode_length` times policy forward + HipRendezvousUpdateTick + HipEvaluateAccumulate
    "one launch"  examples/rendezvous_evaluate/: HipRendezvousEvaluateEvaluate_H<width>, one launch per evaluation; the time
                  includes the repack of the policy

Method: a host clock around `--calls` calls of `evaluate_episodes` (every call ends in a device synchronise: it pulls its
results), after `--warmup` calls of both plans, six windows per plan and mode, the plans alternating inside every round so
that each sees the same drift of the clocks.  One JSON line per plan and mode with every window (ms per evaluation), then
one line per width and mode that says whether EVERY window of "one launch" lies below EVERY window of "per tick".
`--plans "per tick"` measures that plan alone (a checkout without the Evaluate example has nothing else).

    python scripts/custom_env_evaluate_timing.py [--envs 2000] [--agents 100] [--calls 20] [--warmup 3] [--widths 32 64]
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

EXAMPLES = {"per tick": ("rendezvous_update", "RendezvousUpdate"), "one launch": ("rendezvous_evaluate", "RendezvousEvaluate")}
MODES = ("greedy", "sampled")


def example(plan):
    folder, name = EXAMPLES[plan]
    spec = importlib.util.spec_from_file_location(f"{folder}_example", os.path.join(ROOT, "examples", folder, f"{folder}.py"))
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    return module, getattr(module, name)


def build(plan, width, args, results_dir):
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.training.trainer import Trainer
    from warp_drive_amd.utils.env_registrar import EnvironmentRegistrar

    module, cls = example(plan)
    registrar = EnvironmentRegistrar()
    registrar.add(env_backend=["cpu", "hip"], cuda_env_src_path=module.SOURCE)(cls)
    env_config = dict(num_agents=args.agents, grid_length=10, episode_length=20, seed=1, wall_penalty=0.125, spread_limit=-1)
    w = EnvWrapper(env_name=cls.name, env_config=env_config, num_envs=args.envs, env_backend="hip", env_registrar=registrar)
    config = {"name": cls.name, "trainer": {"num_envs": args.envs, "train_batch_size": args.envs * 20, "num_episodes": 10 ** 7,
                                            "seed": 7, "fused_rollout_policy": "all"},
              "policy": {"shared": {"to_train": True, "algorithm": "A2C", "lr": 0.001, "vf_loss_coeff": 1, "gamma": 0.98,
                                    "model": {"type": "fully_connected", "fc_dims": [width, width]}}},
              "saving": {"metrics_log_freq": 10 ** 6, "model_params_save_freq": 0, "basedir": results_dir,
                         "name": cls.name, "tag": f"{plan.replace(' ', '_')}_{width}"}}
    torch.manual_seed(0)
    trainer = Trainer(env_wrapper=w, config=config, policy_tag_to_agent_id_map={"shared": list(range(args.agents))},
                      results_dir=results_dir, verbose=False)
    assert trainer.rollout_path == "one launch", trainer.rollout_path
    return trainer


def window(trainer, calls, greedy):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        trainer.evaluate_episodes(use_argmax=greedy)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=2000)
    ap.add_argument("--agents", type=int, default=100)
    ap.add_argument("--calls", type=int, default=20, help="evaluations per window")
    ap.add_argument("--warmup", type=int, default=3, help="evaluations of every plan and mode before the first window")
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--widths", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--plans", nargs="+", default=list(EXAMPLES), choices=list(EXAMPLES))
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    with tempfile.TemporaryDirectory() as results_dir:
        for width in args.widths:
            built = {plan: build(plan, width, args, results_dir) for plan in args.plans}
            for mode in MODES:
                for plan in args.plans:
                    for _ in range(args.warmup):
                        built[plan].evaluate_episodes(use_argmax=mode == "greedy")
                    assert built[plan].evaluation_path == plan, (plan, built[plan].evaluation_path)
            for mode in MODES:
                times = {plan: [] for plan in args.plans}
                for _ in range(args.windows):
                    for plan in args.plans:  # alternating
                        times[plan].append(window(built[plan], args.calls, mode == "greedy"))
                for plan in args.plans:
                    ms = times[plan]
                    print(json.dumps({"tree": args.label, "plan": plan, "mode": mode, "width": width, "envs": args.envs,
                                      "agents": args.agents, "episode_ticks": 20, "calls_per_window": args.calls,
                                      "warmup_calls": args.warmup, "windows_ms_per_evaluation": [round(v, 3) for v in ms],
                                      "median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3),
                                      "max_ms": round(max(ms), 3)}), flush=True)
                if len(args.plans) == 2:
                    med = {plan: float(np.median(times[plan])) for plan in args.plans}
                    print(json.dumps({"tree": args.label, "width": width, "mode": mode,
                                      "every_one_launch_window_below_every_per_tick_window":
                                          max(times["one launch"]) < min(times["per tick"]),
                                      "per_tick_over_one_launch": round(med["per tick"] / med["one launch"], 2)}), flush=True)
            for trainer in built.values():
                trainer.graceful_close()


if __name__ == "__main__":
    main()
