"""Multi-tick form of the fused TagContinuous tick (HipTagContinuousRollout_K10_N105A21, LaunchPlan.set_multi_tick): a
run(n >= 2) is ONE launch whose blocks take their replica through n ticks.  Every tick of the loop is the whole one-tick
kernel and the draws are keyed by (agent, epoch), so every array and the RNG state must be BIT-identical to an engine
stepped with run(1) -- restarts at the start, in the middle and on the last tick of a launch included (15-tick episodes).
With the switch off the engine is the cohort engine of tests/test_gpu_tick_cohorts.py, whose comparisons are repeated
here (that file exercises the default, which is the multi-tick form from now on)."""
import numpy as np
import pytest
import torch

from tests.test_gpu_tag_continuous import _fused_ticks_vs_c_oracle
from tests.test_gpu_tick_cohorts import ARRAYS, CFG, _assert_same, _state

pytestmark = pytest.mark.gpu

ROLLOUT = "HipTagContinuousRollout_K10_N105A21"
# 35 ticks in uneven launches (launches end after ticks 1, 8, 10, 11, 16, 32, 35; episodes of 15 ticks restart on ticks 15
# and 30: in the middle of the 5-tick and of the 16-tick launch), and one launch of 40 ticks with two restarts inside it
CHUNKS = ((1, 7, 2, 1, 5, 16, 3), (40,))
# launches that end exactly ON a restart (ticks 15 and 30), so the next one starts on a fresh episode
CHUNKS_ON_RESTART = (15, 15, 5)
SIZES = (2000, 1000, 33, 2500)  # 2500: more blocks than the device holds at once -- blocks start after others have finished


def _engine(monkeypatch, E, rollout_on, cohorts=2, cfg=CFG, seed=4242):
    from tests.hip_harness import require_gpu
    from warp_drive_amd import rollout
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.envs.tag_continuous import TagContinuous
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

    require_gpu()
    monkeypatch.setattr(rollout, "TICK_COHORTS", cohorts)
    monkeypatch.setattr(rollout, "TICK_ROLLOUT", 1 if rollout_on else 0)
    w = EnvWrapper(env_obj=TagContinuous(**cfg), num_envs=E, env_backend="hip")
    w.reset_all_envs()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=seed)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    engine = rollout.RolloutEngine(w, sampler)
    assert engine.step_kernel_name == "HipTagContinuousTick_K10_N105A21"
    assert engine.ticks_per_launch == 1 and len(engine.entry_names) == 1
    assert engine.rollout_kernel_name == (ROLLOUT if rollout_on else None)
    return w, sampler, engine


def _compare_chunks(monkeypatch, E, cfg, chunks):
    """an engine on the multi-tick path, run(chunk) per chunk, against a second engine stepped with run(1); tolerance 0"""
    w1, s1, ref = _engine(monkeypatch, E, False, cohorts=1, cfg=cfg)
    wr, sr, eng = _engine(monkeypatch, E, True, cfg=cfg)
    done = 0
    for chunk in chunks:
        for _ in range(chunk):
            ref.run(1)
        eng.run(chunk)
        done += chunk
        _assert_same(_state(wr, sr), _state(w1, s1), f"after {done} ticks (last run({chunk}))")
    assert done >= 35
    return w1


@pytest.mark.parametrize("chunks", CHUNKS + (CHUNKS_ON_RESTART,), ids=lambda c: "+".join(map(str, c)))
@pytest.mark.parametrize("E", SIZES)
def test_rollout_equals_one_launch_per_tick(monkeypatch, E, chunks):
    _compare_chunks(monkeypatch, E, CFG, chunks)


@pytest.mark.parametrize("chunks", CHUNKS, ids=lambda c: "+".join(map(str, c)))
@pytest.mark.parametrize("E", SIZES)
def test_rollout_with_the_arena_emptying(monkeypatch, E, chunks):
    """the largest tagging distance the env takes: the arena falls below K agents in the game inside a launch, and episodes end early on
    `no runners left`, at ticks that differ from replica to replica"""
    _compare_chunks(monkeypatch, E, dict(CFG, tagging_distance=1.0), chunks)


@pytest.mark.parametrize("chunks", CHUNKS, ids=lambda c: "+".join(map(str, c)))
@pytest.mark.parametrize("E", SIZES)
def test_rollout_with_nobody_leaving(monkeypatch, E, chunks):
    """tagging distance 0: every agent stays in the game for the whole episode"""
    w1 = _compare_chunks(monkeypatch, E, dict(CFG, tagging_distance=0.0), chunks)
    assert (w1.cuda_data_manager.pull_data_from_device("still_in_the_game") == 1).all()


def test_rollout_plan_vs_c_oracle(monkeypatch):
    """an engine that carries the multi-tick form, stepped one tick at a time, every replica against the C oracle; with
    the tests above (multi-tick runs bit-identical to one launch per tick) this ties the loop to the oracle too"""
    from warp_drive_amd import rollout

    monkeypatch.setattr(rollout, "TICK_COHORTS", 2)
    monkeypatch.setattr(rollout, "TICK_ROLLOUT", 1)
    _fused_ticks_vs_c_oracle(dict(CFG), 2000, 32, 4242)


def test_caller_stream_sees_the_final_tick(monkeypatch):
    """a torch read on the caller's stream right after run(24), with no synchronisation, sees tick 24"""
    w1, s1, ref = _engine(monkeypatch, 2000, False, cohorts=1)
    wr, sr, eng = _engine(monkeypatch, 2000, True)
    ref.run(24)
    dm = wr.cuda_data_manager
    eng.run(24)
    snap = {k: dm.data_on_device_via_torch(k).clone() for k in ("observations", "rewards", "sampled_actions")}
    torch.cuda.synchronize()
    for k, v in snap.items():
        np.testing.assert_array_equal(v.cpu().numpy(), w1.cuda_data_manager.pull_data_from_device(k), err_msg=k)


def test_long_runs_are_split(monkeypatch):
    """a run longer than the cap on ticks per launch is several launches: same state as the same ticks in smaller runs"""
    from warp_drive_amd import rollout

    monkeypatch.setattr(rollout, "ROLLOUT_MAX_TICKS", 16)
    w1, s1, a = _engine(monkeypatch, 256, True)
    w2, s2, b = _engine(monkeypatch, 256, True)
    a.run(37)  # 16 + 16 + 5
    for n in (10, 10, 10, 7):
        b.run(n)
    _assert_same(_state(w1, s1), _state(w2, s2), "run(37) split at 16 ticks per launch")


@pytest.mark.parametrize("E,cohorts", [(2000, 2), (2000, 3), (2000, 4), (1000, 3)])
def test_switch_off_is_the_cohort_plan(monkeypatch, E, cohorts):
    """WD_TICK_ROLLOUT=0: no multi-tick form, the cohort plan as before, bit-identical to one launch per tick"""
    w1, s1, ref = _engine(monkeypatch, E, False, cohorts=1)
    wc, sc, eng = _engine(monkeypatch, E, False, cohorts=cohorts)
    assert ref.cohorts == 1 and eng.cohorts == cohorts and eng.plan.cohorts == cohorts
    done = 0
    for chunk in CHUNKS[0]:
        for _ in range(chunk):
            ref.run(1)
        eng.run(chunk)
        done += chunk
        _assert_same(_state(wc, sc), _state(w1, s1), f"after {done} ticks (last run({chunk}))")
    assert done >= 30 and set(ARRAYS) < set(_state(wc, sc))
