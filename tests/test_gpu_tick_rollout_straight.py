"""The multi-tick TagContinuous entry issues its probability slabs as straight-line code (tc_fetch_slabs_straight: one
global address and one LDS base per slab and per four pieces, the pieces told apart by the instruction's immediate
offset, which must advance the global and the LDS address alike).  It must leave what the one-tick kernel leaves: every
array of tests/test_gpu_tick_rollout.py plus the RNG words, tolerance 0, against a second engine stepped with run(1).

Both engines sample from seeded random probability rows, different for every row and head.  With the uniform rows of
the default a row that lands in the wrong LDS place samples the same action, and a misplaced slab piece goes unseen.

Replica e's slab starts at 8820 * e bytes and its observation rows at 3 * e dwords modulo 4, so four consecutive
replicas cover every 16-byte phase of both; E = 1 .. 5 put each phase into the last block of a launch once."""
import numpy as np
import pytest
import torch

from tests.test_gpu_tick_cohorts import ARRAYS, CFG, _assert_same, _state
from tests.test_gpu_tick_rollout import ROLLOUT

pytestmark = pytest.mark.gpu


def _random_rows(E, N, heads, seed):
    """one [E, N, a] float32 tensor per head: every row a distribution of its own"""
    rng = np.random.default_rng(seed)
    out = []
    for a in heads:
        p = rng.random((E, N, a), dtype=np.float32) + np.float32(0.05)
        p /= p.sum(axis=2, keepdims=True, dtype=np.float32)
        out.append(torch.from_numpy(np.ascontiguousarray(p)).cuda())
    return out


def _engine(monkeypatch, E, rollout_on, cfg, seed=4242, prob_seed=77):
    from tests.hip_harness import require_gpu
    from warp_drive_amd import rollout
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.envs.tag_continuous import TagContinuous
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

    require_gpu()
    monkeypatch.setattr(rollout, "TICK_COHORTS", 2 if rollout_on else 1)
    monkeypatch.setattr(rollout, "TICK_ROLLOUT", 1 if rollout_on else 0)
    env = TagContinuous(**cfg)
    w = EnvWrapper(env_obj=env, num_envs=E, env_backend="hip")
    w.reset_all_envs()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=seed)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    heads = [int(n) for n in env.action_space[0].nvec]
    assert heads == [21, 21] and w.n_agents == 105
    probs = _random_rows(E, w.n_agents, heads, prob_seed)
    engine = rollout.RolloutEngine(w, sampler, probabilities=probs)
    assert engine.step_kernel_name == "HipTagContinuousTick_K10_N105A21"
    assert engine.rollout_kernel_name == (ROLLOUT if rollout_on else None)
    return w, sampler, engine, probs


def _compare(monkeypatch, E, cfg, chunks):
    w1, s1, ref, p1 = _engine(monkeypatch, E, False, cfg)
    wr, sr, eng, pr = _engine(monkeypatch, E, True, cfg)
    for a, b in zip(p1, pr):
        assert torch.equal(a, b) and float((a[0, 0] - a[0, 1]).abs().max()) > 0
    done = 0
    for chunk in chunks:
        for _ in range(chunk):
            ref.run(1)
        eng.run(chunk)
        done += chunk
        got, want = _state(wr, sr), _state(w1, s1)
        assert set(ARRAYS) < set(got) and "rng_state" in got
        _assert_same(got, want, f"after {done} ticks (last run({chunk}))")
    return w1, want


@pytest.mark.parametrize("E", [1, 2, 3, 4, 5])
def test_every_alignment_with_everybody_in_the_game(monkeypatch, E):
    """tagging distance 0, run(6) from a fresh episode: every agent stays in the game, so both wavefronts use the dense form
    on every chunk, the two full ones and the short last one"""
    w1, want = _compare(monkeypatch, E, dict(CFG, tagging_distance=0.0), (6,))
    assert (want["still_in_the_game"] == 1).all()
    # the draws are not the uniform rows' draws by accident: both heads use their whole range
    acts = want["sampled_actions"]
    assert acts.min() == 0 and acts.max() == 20


@pytest.mark.parametrize("tagging_distance", [None, 1.0], ids=["default_distance", "distance_1"])
def test_wavefronts_in_different_forms(monkeypatch, tagging_distance):
    """E = 9, run(40): agents leave the game at their own ticks, so there are trips on which one wavefront of a block writes
    its rows in the dense form and the other in the sparse one, and restores inside the launch"""
    cfg = dict(CFG) if tagging_distance is None else dict(CFG, tagging_distance=tagging_distance)
    _compare(monkeypatch, 9, cfg, (40,))


def test_reload_trips_and_the_trip_after_a_restore(monkeypatch):
    """E = 9, three-tick episodes: every third trip restores, launches of one tick among them"""
    _compare(monkeypatch, 9, dict(CFG, episode_length=3), (1, 2, 3, 5, 1, 8))
