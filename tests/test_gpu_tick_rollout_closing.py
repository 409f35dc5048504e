"""The multi-tick TagContinuous entry (HipTagContinuousRollout_K10_N105A21) stores the state a thread carries in registers
-- position, speed, heading, acceleration, the edge penalty, the RNG epoch word, the time step and the runner count -- on
CLOSING trips only: the last trip of a launch and the trip a replica's episode ends on (tc_store_carried, tc_fast.h).  What
the host finds after a launch, and what the trip after a restore reloads, must be what the one-tick entry leaves: two
engines start from the same state, one is stepped with run(1) and one with run(n); the thirteen arrays of
tests/test_gpu_tick_cohorts.py, the edge penalties and the RNG words are compared at tolerance 0 after every launch (the
method and the helpers of tests/test_gpu_tick_rollout_rows.py).

The one built shape (5 taggers + 100 runners, K = 10) at E = 1, 2 and 9, with an edge penalty that is not zero (the
benchmark's is -0.0 whether an agent crossed the edge or not).  A store that is missing on a closing trip shows in the
array itself at the end of a launch, and at an episode's end in the RNG words -- no restore rewrites them, so the trip after
it reloads a stale epoch and draws other actions -- and in every array the reset table leaves out."""
import numpy as np
import pytest
import torch

from tests.test_gpu_tick_cohorts import ARRAYS, CFG, _assert_same, _state
from tests.test_gpu_tick_rollout import ROLLOUT
from tests.test_gpu_tick_rollout_rows import N, _host_write, _pair

pytestmark = pytest.mark.gpu

f32 = np.float32
EDGE = "edge_hit_reward_penalty"
BASE = dict(CFG, edge_hit_penalty=-0.25)
SIZES = [1, 2, 9]


def _full_state(w, sampler):
    from tests.hip_harness import pull

    out = _state(w, sampler)
    out[EDGE] = pull(w, EDGE)
    return out


def _run_chunks(one, multi, chunks, done=0):
    """run(1) repeated against run(chunk), compared after every launch; returns the reference's last state"""
    (w1, s1, ref, _), (wr, sr, eng, _) = one, multi
    assert eng.rollout_kernel_name == ROLLOUT and ref.rollout_kernel_name is None
    want = None
    for chunk in chunks:
        for _ in range(chunk):
            ref.run(1)
        eng.run(chunk)
        done += chunk
        got, want = _full_state(wr, sr), _full_state(w1, s1)
        assert set(ARRAYS) < set(got) and "rng_state" in got and EDGE in got
        _assert_same(got, want, f"after {done} ticks (last run({chunk}))")
    return want


def _episode_ends(chunks, episode_length, first_tick=0):
    """for every launch: the trips (0-based) on which the episode ends by time, when every replica starts at `first_tick`"""
    t, out = first_tick, []
    for chunk in chunks:
        ends = []
        for trip in range(chunk):
            t += 1
            if t == episode_length:
                ends.append(trip)
                t = 0
        out.append(ends)
    return out, t


@pytest.mark.parametrize("E", SIZES)
def test_launch_lengths(monkeypatch, E):
    """launches of 1, 2, 3 and 7 ticks in a long episode: the closing trip is the reload trip itself (the one-tick entry), the
    trip after it, or a later one; nothing but the last trip of a launch closes"""
    cfg = dict(BASE, episode_length=500, tagging_distance=0.0)
    one, multi = _pair(monkeypatch, E, cfg)
    want = _run_chunks(one, multi, (1, 2, 3, 7))
    assert (want["_timestep_"] == 13).all() and not want["_done_"].any()   # no episode ended: no restore inside a launch
    assert (want["still_in_the_game"] == 1).all() and (want["num_runners"] == 100).all()
    assert want["speed"].any() and want["acceleration"].any()


@pytest.mark.parametrize("E", SIZES)
def test_three_tick_episodes(monkeypatch, E):
    """episodes of three ticks, every replica one tick into its episode, launches of (1, 2, 3, 5, 1, 8): an episode ends by
    time on the first, on a middle and on the last trip of a launch -- on the last one both conditions hold at once"""
    chunks, T = (1, 2, 3, 5, 1, 8), 3
    ends, last = _episode_ends(chunks, T, first_tick=1)
    multi_tick = [(c, e) for c, e in zip(chunks, ends) if c >= 2]
    assert any(0 in e for _, e in multi_tick), "no episode ends on the first trip of a launch"
    assert any(c - 1 in e for c, e in multi_tick), "no episode ends on the last trip of a launch"
    assert any(any(0 < t < c - 1 for t in e) for c, e in multi_tick), "no episode ends inside a launch"
    assert any(len(e) >= 2 for _, e in multi_tick), "no launch with a restore and a later closing trip"
    one, multi = _pair(monkeypatch, E, dict(BASE, episode_length=T, tagging_distance=0.0))
    for w in (one[0], multi[0]):
        _host_write(w, "_timestep_", lambda t: t.fill(1))
    torch.cuda.synchronize()
    want = _run_chunks(one, multi, chunks)
    assert ends[-1][-1] == chunks[-1] - 1 and last == 0
    assert (want["_timestep_"] == 0).all() and (want["_done_"] == 1).all()   # the last launch ended on a restore


@pytest.mark.parametrize("E", SIZES)
def test_every_runner_tagged_inside_a_launch(monkeypatch, E):
    """tagging distance 1.0: every runner is tagged on the first tick of an episode, which ends there (`no runners left`),
    far from its 15 ticks -- on every trip of run(3) and run(2), the middle one included"""
    one, multi = _pair(monkeypatch, E, dict(BASE, episode_length=15, tagging_distance=1.0))
    (w1, s1, ref, _) = one
    ref.run(1)
    first = _full_state(w1, s1)
    multi[2].run(1)
    # the claim, on the reference: one tick, and the episode is over with the time step back at 0
    assert (first["_done_"] == 1).all() and (first["_timestep_"] == 0).all()
    assert (first["num_runners"] == 100).all() and (first["still_in_the_game"] == 1).all()   # (restored)
    want = _run_chunks(one, multi, (3, 2), done=1)
    assert (want["_done_"] == 1).all() and (want["_timestep_"] == 0).all()
    # the draws went on from episode to episode: six epochs per agent
    assert (want["rng_state"][4:] == first["rng_state"][4:] + 5).all()


@pytest.mark.parametrize("E", SIZES)
def test_reset_table_without_speed(monkeypatch, E):
    """`speed` taken out of the arrays a reset restores (the host's choice: the data manager's reset list), engines rebuilt
    on the shorter table: after an episode's end the array holds what the closing trip stored, and the next trip reloads it"""
    from warp_drive_amd import rollout

    T = 3
    one, multi = _pair(monkeypatch, E, dict(BASE, episode_length=T, tagging_distance=0.0))
    pairs = []
    for (w, sampler, old, probs), on in ((one, 0), (multi, 1)):
        dm = w.cuda_data_manager
        n_before = len(dm.reset_data_list)
        assert "speed" in dm.reset_data_list and "loc_x" in dm.reset_data_list
        dm.reset_data_list.remove("speed")
        monkeypatch.setattr(rollout, "TICK_COHORTS", 2 if on else 1)
        monkeypatch.setattr(rollout, "TICK_ROLLOUT", on)
        eng = rollout.RolloutEngine(w, sampler, probabilities=probs)
        assert len(w.env_resetter._table_names) == n_before - 1 and "speed" not in w.env_resetter._table_names
        pairs.append((w, sampler, eng, probs))
    one, multi = pairs
    start = _full_state(multi[0], multi[1])
    want = _run_chunks(one, multi, (3,))      # the episode ends on the last trip of the launch
    assert (want["_timestep_"] == 0).all() and (want["_done_"] == 1).all()
    np.testing.assert_array_equal(want["loc_x"], start["loc_x"])   # restored ...
    moving = lambda st: (st["speed"].reshape(E, N) != 0).any(axis=1).all()
    assert not start["speed"].any() and moving(want)   # ... and not: `speed` holds the closing trip's values
    want = _run_chunks(one, multi, (2, 5, 2), done=3)   # ends on the first and the fourth trip of run(5), the last of run(2)
    assert (want["_timestep_"] == 0).all() and moving(want)


@pytest.mark.parametrize("E", SIZES)
def test_host_write_between_two_launches(monkeypatch, E):
    """run(3), `loc_x` mirrored by the host in both engines, run(4): the next launch starts from what the host wrote"""
    cfg = dict(BASE, episode_length=500, tagging_distance=0.0)
    one, multi = _pair(monkeypatch, E, cfg)
    before = _run_chunks(one, multi, (3,))
    L, reach = f32(cfg["grid_length"]), 4 * cfg["max_speed"] + 1e-3
    for w in (one[0], multi[0]):
        def mirror(x):
            x[:] = L - x

        _host_write(w, "loc_x", mirror)
    torch.cuda.synchronize()
    after = _run_chunks(one, multi, (4,), done=3)
    assert (np.abs(after["loc_x"] - (L - before["loc_x"])) <= reach).all()    # four ticks away from the mirrored place ...
    assert (np.abs(after["loc_x"] - before["loc_x"]) > reach).any()           # ... which somebody could not have walked to


@pytest.mark.parametrize("E,begin,end", [(2, 1, 2), (9, 2, 7), (9, 5, 9)])
def test_replica_range_that_does_not_start_at_zero(monkeypatch, E, begin, end):
    """the multi-tick entry launched on replicas [begin, end) with three-tick episodes, five ticks (the episode ends on the
    third trip), against the one-tick entry on the same range: the closing block addresses a replica's rows off
    kEnvBegin + block, and the replicas outside the range are not touched"""
    one, multi = _pair(monkeypatch, E, dict(BASE, episode_length=3, tagging_distance=0.0))
    start = _full_state(multi[0], multi[1])
    ticks = 5
    (w1, s1, _, p1), (wr, sr, _, pr) = one, multi
    for _ in range(ticks):
        fn, args, block, grid, shared = w1.env.tick_launch(s1, p1, w1.env_resetter, env_range=(begin, end))
        assert grid[0] == end - begin
        fn(*args, block=block, grid=grid, shared=shared)
    env = wr.env
    fn, args, block, grid, shared = env.rollout_launch(sr, pr, wr.env_resetter)
    assert fn.name == ROLLOUT and grid[0] == E and len(args) == len(env._STEP_ARGS) + 8
    args = list(args)
    args[env._STEP_ARGS.index(("n_envs", "meta"))] = np.int32(end)   # kNumEnvs carries `end`, kEnvBegin `begin`
    args[len(env._STEP_ARGS)] = np.int32(begin)
    args[-1] = np.int32(ticks)
    fn(*args, block=block, grid=(end - begin, 1), shared=shared)
    got, want = _full_state(wr, sr), _full_state(w1, s1)
    _assert_same(got, want, f"after one launch of {ticks} ticks on replicas [{begin}, {end})")
    inside = np.zeros(E, dtype=bool)
    inside[begin:end] = True
    assert (want["_timestep_"][inside] == ticks % 3).all() and (want["_timestep_"][~inside] == 0).all()
    rng, rng0 = want["rng_state"][4:].reshape(E, N), start["rng_state"][4:].reshape(E, N)
    assert (rng[inside] == rng0[inside] + ticks).all() and (rng[~inside] == rng0[~inside]).all()
    for k in ("loc_x", "speed", EDGE):
        np.testing.assert_array_equal(want[k].reshape(E, -1)[~inside], start[k].reshape(E, -1)[~inside], err_msg=k)
    assert (want["loc_x"].reshape(E, -1)[inside] != start["loc_x"].reshape(E, -1)[inside]).any()
