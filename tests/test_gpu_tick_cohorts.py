"""Replica cohorts of the fused TagContinuous tick (RolloutEngine + LaunchPlan.add_cohort): a multi-tick run() forks the
replicas into C ranges on their own streams and joins them back into the caller's stream.  Replicas are independent and the tick's random draws are keyed by (agent, epoch), not by block or launch, so
every array must be BIT-identical to one whole-range launch per tick -- resets included (15-tick episodes)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_tag_continuous import BENCH_CFG, _fused_ticks_vs_c_oracle

pytestmark = pytest.mark.gpu

CFG = dict(BENCH_CFG, episode_length=15)  # BASELINE configs[2] (5 taggers x 100 runners, K = 10), short episodes
ARRAYS = ("observations", "rewards", "_done_", "sampled_actions", "nearest_neighbor_ids", "loc_x", "loc_y", "speed",
          "direction", "acceleration", "still_in_the_game", "num_runners", "_timestep_")


def _engine(monkeypatch, E, cohorts, seed=4242):
    from tests.hip_harness import require_gpu
    from warp_drive_amd import rollout
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.envs.tag_continuous import TagContinuous
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

    require_gpu()
    monkeypatch.setattr(rollout, "TICK_COHORTS", cohorts)
    w = EnvWrapper(env_obj=TagContinuous(**CFG), num_envs=E, env_backend="hip")
    w.reset_all_envs()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=seed)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    engine = rollout.RolloutEngine(w, sampler)
    assert engine.step_kernel_name == "HipTagContinuousTick_K10_N105A21"
    assert len(engine.entry_names) == 1
    return w, sampler, engine


def _state(w, sampler):
    from tests.hip_harness import pull
    from warp_drive_amd.managers import hip_driver as drv

    torch.cuda.synchronize()
    out = {k: pull(w, k) for k in ARRAYS}
    rng = np.zeros(4 + w.n_envs * w.n_agents, dtype=np.uint32)
    drv.memcpy_dtoh(rng, sampler.rng_state)
    out["rng_state"] = rng
    return out


def _assert_same(a, b, tag):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{k} {tag}")


@pytest.mark.parametrize("E,cohorts", [(2000, 2), (2000, 3), (2000, 4), (1000, 3)])
def test_cohorts_equal_one_launch_per_tick(monkeypatch, E, cohorts):
    """C in {2, 3, 4} (E = 2000 and 1000 are not multiples of 32 * C: the last cohort is the odd one) against C = 1
    stepped one tick at a time: run(1) / run(n) sequences over 35 ticks, two restarts of every replica"""
    w1, s1, ref = _engine(monkeypatch, E, 1)
    assert ref.cohorts == 1
    wc, sc, eng = _engine(monkeypatch, E, cohorts)
    assert eng.cohorts == cohorts
    done = 0
    for chunk in (1, 7, 2, 1, 5, 16, 3):
        for _ in range(chunk):
            ref.run(1)
        eng.run(chunk)
        done += chunk
        _assert_same(_state(wc, sc), _state(w1, s1), f"after {done} ticks (last run({chunk}))")
    assert done >= 30


def test_small_E_keeps_one_cohort(monkeypatch):
    """cohorts that would not cover half of the CUs each: the engine keeps one launch per tick"""
    _, _, eng = _engine(monkeypatch, 200, 2)
    assert eng.cohorts == 1 and eng.plan.cohorts == 1


def test_caller_stream_is_ordered_after_every_cohort(monkeypatch):
    """a torch read on the caller's stream right after run(n), with no synchronisation, sees the final state of
    every cohort (the join events)"""
    w1, s1, ref = _engine(monkeypatch, 2000, 1)
    wc, sc, eng = _engine(monkeypatch, 2000, 3)
    ref.run(24)
    dm = wc.cuda_data_manager
    eng.run(24)
    snap = {k: dm.data_on_device_via_torch(k).clone() for k in ("observations", "rewards", "sampled_actions")}
    torch.cuda.synchronize()
    for k, v in snap.items():
        np.testing.assert_array_equal(v.cpu().numpy(), w1.cuda_data_manager.pull_data_from_device(k), err_msg=k)


def test_cohort_plan_vs_c_oracle(monkeypatch):
    """an engine built with cohorts, stepped one tick at a time (the whole-range entry), every replica against the
    C oracle; with the tests above (cohort runs bit-identical to one launch per tick) this ties the cohort runs to
    the oracle too"""
    from warp_drive_amd import rollout

    monkeypatch.setattr(rollout, "TICK_COHORTS", 2)
    _fused_ticks_vs_c_oracle(dict(CFG), 2000, 32, 4242)
