#!/usr/bin/env python3
"""The returns launch of `trainer.fused_update: "all"` with and without the policy key `gae_lambda`, by
scripts/pg_update_timing.py's method (device events, the sides alternating inside a repeat), in ONE process per shape:

  * the launch alone on the trainer's last batch: HipDiscountedReturns (today's estimator), HipPgGaeReturns
    (csrc/kernels/pg_gae.hip) at the host's S (`pg_update_kernels.gae_wavefronts`) and at S = 1;
  * the whole update (`_update_model_params`, five launches) of three trainers: without the key, with `gae_lambda: 0.95`,
    and with the key and S forced to 1.

Shapes: single_acrobot as shipped (E = 100, T = 500: two tiles of columns, the scan's case) and single_cartpole at
E = 100 000, T = 10 (1563 tiles: the host picks S = 1 and the entry reads one array more than HipDiscountedReturns).  One
JSON line per side and one per comparison: whether every repeat of one side is below every repeat of the other.

    python scripts/pg_gae_timing.py [--launches 200] [--iterations 100] [--warmup 20] [--repeats 5]
"""
import argparse
import functools
import json
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts.pg_update_timing import summary  # noqa: E402

SHAPES = (("single_acrobot", 100, 500), ("single_cartpole", 100000, 10))
LAMBDA = 0.95


def build(env, E, T, results_dir, gae):
    import yaml
    from warp_drive_amd.training.scripts.train import _CONFIGS, setup_trainer

    shipped = yaml.safe_load(open(os.path.join(_CONFIGS, f"{env}.yaml")))["policy"]["shared"]   # (an override replaces it whole)
    ov = {"trainer": {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": 1,
                      "fused_rollout_policy": "all", "fused_update": "all"},
          "policy": {"shared": {**shipped, "gae_lambda": LAMBDA if gae else None}},
          "saving": {"metrics_log_freq": 10 ** 9, "model_params_save_freq": 0}}
    torch.manual_seed(1)
    tr = setup_trainer(env, ov, results_dir=results_dir, verbose=False)
    assert tr._batch_rollout is not None and tr.update_path == {"shared": "kernels"}, (tr.rollout_path, tr.update_path)
    return tr


def timed(call, count):
    """device microseconds of `count` single calls, an event pair around each"""
    out = []
    for _ in range(count):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        out.append(1e3 * a.elapsed_time(b))
    return out


def update(tr, it):
    tr._generate_rollout_batch()
    return lambda: tr._update_model_params(it, False)


def compare(tag, records, a, b):
    x, y = records[a], records[b]
    print(json.dumps({**tag, "compared": [a, b], f"{a}_below_in_every_repeat": x["max_us"] < y["min_us"],
                      f"{b}_below_in_every_repeat": y["max_us"] < x["min_us"],
                      "ratio_of_medians": round(y["median_us"] / x["median_us"], 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measures the device: no GPU, no number"
    from warp_drive_amd.training.pg_update_kernels import gae_wavefronts

    for env, E, T in SHAPES:
        with tempfile.TemporaryDirectory() as tmp:
            trainers = {"today": build(env, E, T, os.path.join(tmp, "a"), False), "gae": build(env, E, T, os.path.join(tmp, "b"), True),
                        "gae_S1": build(env, E, T, os.path.join(tmp, "c"), True)}
            k1 = trainers["gae_S1"]._pg_kernels["shared"]
            k1.gae_returns = functools.partial(k1.gae_returns, wavefronts=1)
            tr = trainers["gae"]
            k, S = tr._pg_kernels["shared"], gae_wavefronts(E, T, tr._pg_kernels["shared"].compute_units)
            tag = {"config": env, "envs": E, "ticks": T, "host_S": S}
            tr._generate_rollout_batch()
            rewards, done, gamma = tr.batch["shared"]["rewards"][:T], tr.done_batch[:T], tr.trainers["shared"].discount_factor_gamma
            k.compute_values(tr.batch["shared"]["obs"][:T], tr._pg_flat["shared"].flat)
            launches = {"HipDiscountedReturns": lambda: k.discounted_returns(rewards, done, gamma),
                        f"HipPgGaeReturns_S{S}": lambda: k.gae_returns(rewards, done, gamma, LAMBDA, wavefronts=S),
                        "HipPgGaeReturns_S1": lambda: k.gae_returns(rewards, done, gamma, LAMBDA, wavefronts=1)}
            alone, whole, it = {n: [] for n in launches}, {n: [] for n in trainers}, 0
            for _ in range(args.repeats):
                for name, call in launches.items():   # alternating: every side sees the same drift of the clocks
                    timed(call, args.warmup)
                    alone[name].append(timed(call, args.launches))
                for name, t in trainers.items():
                    for count in (args.warmup, args.iterations):   # (the second list is the timed one)
                        times = [timed(update(t, it + i), 1)[0] for i in range(count)]
                    whole[name].append(times)
                it += args.warmup + args.iterations
            records = {}
            for kind, sides in (("launch", alone), ("update", whole)):
                for name, per_repeat in sides.items():
                    records[name] = summary(per_repeat)
                    print(json.dumps({**tag, "timed": kind, "side": name, **records[name]}), flush=True)
            compare(tag, records, f"HipPgGaeReturns_S{S}", "HipDiscountedReturns")
            if S != 1:
                compare(tag, records, f"HipPgGaeReturns_S{S}", "HipPgGaeReturns_S1")
            compare(tag, records, "gae", "today")
            compare(tag, records, "gae", "gae_S1")
            for t in trainers.values():
                t.graceful_close()


if __name__ == "__main__":
    main()
