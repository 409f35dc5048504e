"""The loop of the multi-tick TagContinuous entry reads its pointer arguments from the kernel-argument segment through
phase-scoped views (tc_kernarg.h: TcRolloutKernarg mirrors the segment field for field; tc_fast.h takes a TcPhase at the
top of every phase).  A wrong field in the mirror struct reads ANOTHER array's pointer, so the cases here are built to show
exactly that: every registered array is an allocation of its own and holds contents that no other array of its size holds
(asserted on the host before the first launch), and the multi-tick entry must leave the bytes the one-tick entry leaves --
two engines start from the same state, one is stepped with run(1) and one with run(n); the thirteen arrays and the RNG
words are compared at tolerance 0 (the method and the helpers of tests/test_gpu_tick_rollout_rows.py and
tests/test_gpu_tick_rollout_search.py).  A store or a load through a neighbour's pointer changes two arrays.

The one built shape (5 taggers + 100 runners, K = 10) at E = 1, 2 and 9.  Three-tick episodes in launches of (1, 2, 3, 5, 1,
8) take the views of the reload (trip 0 of a launch, the trip after a restore) and of the restore through every kind of
trip; one run(40) with tags at tagging distance 0.15 takes the steady-state views through the dense and the sparse row
form and all three regimes of the search."""
import numpy as np
import pytest

from tests.test_gpu_tick_cohorts import ARRAYS, CFG
from tests.test_gpu_tick_rollout_rows import N, SENTINEL, _host_write, _pair, _run_chunks

pytestmark = pytest.mark.gpu

f32 = np.float32
# every array the entries take a pointer to (envs/tag_continuous.py _STEP_ARGS and the fused tick's own), by registered name
POINTER_ARGS = ("loc_x", "loc_y", "speed", "direction", "acceleration", "agent_types", "edge_hit_reward_penalty",
                "acceleration_actions", "turn_actions", "skill_levels", "still_in_the_game", "observations",
                "sampled_actions", "nearest_neighbor_ids", "rewards", "step_rewards", "num_runners", "_done_", "_timestep_",
                "obs_rows_cleared")
assert set(ARRAYS) <= set(POINTER_ARGS)


def _craft(E, seed):
    """contents of their own for the arrays that a fresh reset leaves alike (zeros): valid state, the same in both
    engines"""
    rng = np.random.default_rng(seed)
    live = np.ones((E, N), dtype=bool)
    for e in range(E):
        live[e, rng.choice(np.arange(5, N), size=7 + e, replace=False)] = False   # runners only: the taggers stay
    return {
        "still_in_the_game": live,
        "speed": rng.uniform(0.0, 0.1, size=(E, N)).astype(f32),
        "acceleration": rng.uniform(-0.05, 0.05, size=(E, N)).astype(f32),
        "direction": rng.uniform(0.0, 6.0, size=(E, N)).astype(f32),
        "edge_hit_reward_penalty": np.full((E, N), -0.25, dtype=f32),
        "rewards": np.full((E, N), 0.5, dtype=f32),
        # (zeros in this configuration, as obs_rows_cleared is; every replica is one tick into its episode: `_done_` is zeros)
        "step_rewards": (0.001 * (1 + np.arange(N))).astype(f32),
        "_timestep_": np.ones(E, dtype=np.int32),
    }


def _crafted_pair(monkeypatch, E, cfg, seed=11):
    want = _craft(E, seed)
    one, multi = _pair(monkeypatch, E, cfg, want["still_in_the_game"])
    for w in (one[0], multi[0]):
        for name, val in want.items():
            if name == "still_in_the_game":
                continue

            def put(a, val=val):
                assert a.shape == val.shape and a.dtype == val.dtype, (a.shape, a.dtype)
                a[:] = val

            _host_write(w, name, put)
        _assert_every_array_is_its_own(w)
    return one, multi


def _assert_every_array_is_its_own(w):
    """no two pointer arguments share an allocation, and no two of the same size in bytes hold the same bytes"""
    dm = w.cuda_data_manager
    host = {k: np.ascontiguousarray(dm.pull_data_from_device(k)) for k in POINTER_ARGS}
    address = lambda p: int(getattr(p, "value", p))
    spans = sorted((address(dm.device_data(k)), host[k].nbytes, k) for k in POINTER_ARGS)
    for (p0, n0, k0), (p1, _, k1) in zip(spans, spans[1:]):
        assert p0 + n0 <= p1, (k0, k1)
    names = list(POINTER_ARGS)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if host[a].nbytes == host[b].nbytes:
                assert host[a].tobytes() != host[b].tobytes(), (a, b)


@pytest.mark.parametrize("E", [1, 2, 9])
def test_run_n_equals_run_1_with_every_array_its_own(monkeypatch, E):
    """run(2), run(1), run(4): trips that start a launch and trips inside one, agents out of the game from the start"""
    one, multi = _crafted_pair(monkeypatch, E, dict(CFG, tagging_distance=0.0))
    want = _run_chunks(one, multi, (2, 1, 4))
    assert not (want["observations"] == SENTINEL).any()
    assert (want["_timestep_"] == 1 + 7).all()


@pytest.mark.parametrize("E", [1, 2, 9])
def test_three_tick_episodes(monkeypatch, E):
    """episodes of three ticks in launches of (1, 2, 3, 5, 1, 8): the reload and the restore views on every kind of trip --
    first of a launch, after a restore, both, neither"""
    one, multi = _crafted_pair(monkeypatch, E, dict(CFG, episode_length=3, tagging_distance=1.0))
    want = _run_chunks(one, multi, (1, 2, 3, 5, 1, 8))
    assert not (want["observations"] == SENTINEL).any()
    assert (want["_timestep_"] == (1 + 20) % 3).all()


def test_forty_ticks_with_tags(monkeypatch):
    """E = 9, one run(40) at tagging distance 0.15 (no restart inside the launch): agents leave the game tick by tick"""
    cfg = dict(CFG, episode_length=500, tagging_distance=0.15)
    one, multi = _crafted_pair(monkeypatch, 9, cfg)
    before = _craft(9, 11)["still_in_the_game"].sum(axis=1)
    want = _run_chunks(one, multi, (40,))
    after = (want["still_in_the_game"] & 1).sum(axis=1)
    print("agents in the game before / after run(40), per replica:", list(before), list(after))
    assert (after < before).all()
    assert not (want["observations"] == SENTINEL).any()
