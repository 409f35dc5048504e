"""Trainer.evaluate_episodes for TagGridWorld at 1000 replicas x 100-tick episodes ("tagger" + "runner" policies of
[32, 32] and [64, 64]): the one-launch path (`trainer.fused_rollout_policy: "all"`: HipTagGridWorldEvaluate_N5_H<width>)
against the per-tick path (the default), greedy and sampled.  Host clock around calls that end in the result pull: two
warm-up calls, seven timed calls per path, the two paths alternating.  Run on the GPU box."""
import os, statistics, sys, tempfile, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from warp_drive_amd.training.scripts.train import setup_trainer

E, T, WARMUP, CALLS = 1000, 100, 2, 7


def policies(h):
    pol = {"to_train": True, "algorithm": "A2C", "vf_loss_coeff": 1, "entropy_coeff": 0.05, "gamma": 0.98, "lr": 0.002,
           "model": {"type": "fully_connected", "fc_dims": [h, h], "model_ckpt_filepath": ""}}
    return {"runner": dict(pol), "tagger": dict(pol)}


def trainer(h, trainer_ov):
    ov = {"trainer": dict({"num_envs": E, "train_batch_size": E * T}, **trainer_ov), "env": {"episode_length": T},
          "policy": policies(h)}
    torch.manual_seed(0)
    return setup_trainer("tag_gridworld", ov, results_dir=tempfile.mkdtemp(prefix="gw_eval_"), verbose=False)


def timed(tr, greedy):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rewards, steps = tr.evaluate_episodes(use_argmax=greedy)   # (ends in the pull of the two result arrays)
    return time.perf_counter() - t0, float(steps["tagger"].mean())


for h in (32, 64):
    paths = {"one launch": trainer(h, {"fused_rollout_policy": "all"}), "per tick": trainer(h, {})}
    for tr in paths.values():
        tr.train(1)
    for greedy in (True, False):
        times, mean_steps = {p: [] for p in paths}, {}
        for call in range(WARMUP + CALLS):
            for path, tr in paths.items():
                dt, mean_steps[path] = timed(tr, greedy)
                assert tr.evaluation_path == path, (tr.evaluation_path, path)
                if call >= WARMUP:
                    times[path].append(dt)
        for path, ts in times.items():
            ts_ms = sorted(t * 1e3 for t in ts)
            print(f"[{h}, {h}] {'greedy' if greedy else 'sampled'} {path}: median {statistics.median(ts_ms):.3f} ms, min "
                  f"{ts_ms[0]:.3f}, max {ts_ms[-1]:.3f} over {CALLS} calls ({E} replicas, episodes of at most {T} ticks, "
                  f"mean steps {mean_steps[path]:.1f}); all: {' '.join(f'{t:.3f}' for t in ts_ms)}", flush=True)
        a, b = statistics.median(times["per tick"]), statistics.median(times["one launch"])
        print(f"[{h}, {h}] {'greedy' if greedy else 'sampled'}: per tick / one launch = {a / b:.1f}", flush=True)
    for tr in paths.values():
        tr.graceful_close()
