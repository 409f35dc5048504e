"""The multi-tick TagContinuous entry stores the rows of `nearest_neighbor_ids` from the registers of the lanes that found
the ids, in front of the gather's barrier, and the row of an agent out of the game (ten times -1) only when it can have
changed: on the first tick the agent is out, on trip 0 of a launch and on the trip after a restore (tc_fast.h, "ids out").
The one-tick entry writes every row on every tick from the 16-bit copies in LDS (tc_flush_ids).  Both must leave the same
bytes: two engines start from the same state, one is stepped with run(1) and one with run(n); the thirteen arrays --
every row of `nearest_neighbor_ids` among them -- and the RNG words are compared at tolerance 0 after every chunk.

What a case claims to exercise (agents out of the game, rows with fewer than K neighbours, exact distance ties in both
wavefronts, live counts on both sides of the split search's limits) is asserted on the host from the reference's state."""
import numpy as np
import pytest
import torch

from tests.test_gpu_tick_cohorts import CFG
from tests.test_gpu_tick_rollout_rows import _host_write, _run_chunks
from tests.test_gpu_tick_rollout_straight import _compare, _engine
from tests.test_gpu_tick_rollout_tags import _pair as _pair_standing_still, _write_positions

pytestmark = pytest.mark.gpu

N, K = 105, 10
ID_SENTINEL = np.int32(-777)
f32 = np.float32


def _pull(w, name):
    return np.asarray(w.cuda_data_manager.pull_data_from_device(name))


def _scribble_ids(one, multi):
    for w in (one[0], multi[0]):
        _host_write(w, "nearest_neighbor_ids", lambda a: a.fill(ID_SENTINEL))
    torch.cuda.synchronize()


def _check_id_rows(want, E):
    """every row was written: no sentinel is left; returns the rows as [E, N, K]"""
    ids = want["nearest_neighbor_ids"].reshape(E, N, K)
    assert not (ids == ID_SENTINEL).any()
    return ids


@pytest.mark.parametrize("E", [1, 2, 9])
def test_trip_0_rewrites_every_row(monkeypatch, E):
    """`nearest_neighbor_ids` holds a sentinel before the launch, a third of the agents are out of the game and their
    observation rows are flagged as cleared already (and are zeros): the carried flag alone would skip their id rows"""
    one, multi = _engine(monkeypatch, E, False, dict(CFG, tagging_distance=0.0)), \
        _engine(monkeypatch, E, True, dict(CFG, tagging_distance=0.0))
    torch.cuda.synchronize()
    rng = np.random.default_rng(100 + E)
    types = _pull(one[0], "agent_types").reshape(-1)[:N]
    live = rng.random((E, N)) < 0.67
    live[:, types == 1] = True  # taggers never leave
    live[E - 1, 60:] = (types[60:] == 1)  # one replica with (nearly) nobody in the second wavefront
    assert (~live[:, :64]).any() and (~live[:, 64:]).any() and live[:, :64].any()
    for w in (one[0], multi[0]):
        _host_write(w, "still_in_the_game", lambda s: s.__setitem__(slice(None), live.astype(s.dtype).reshape(s.shape)))
        _host_write(w, "obs_rows_cleared", lambda c: c.__setitem__(slice(None), (~live).astype(c.dtype).reshape(c.shape)))
        _host_write(w, "observations", lambda o: o.reshape(E, N, -1).__setitem__(~live, 0))
    _scribble_ids(one, multi)
    assert (_pull(multi[0], "nearest_neighbor_ids") == ID_SENTINEL).all()
    assert (_pull(multi[0], "obs_rows_cleared").reshape(E, N)[~live] == 1).all()
    want = _run_chunks(one, multi, (2,))
    ids = _check_id_rows(want, E)
    assert np.array_equal(want["still_in_the_game"].reshape(E, N) != 0, live)  # tagging distance 0: the pattern held
    assert (ids[~live] == -1).all() and (~live).sum() > 0
    assert (ids[live][:, 0] >= 0).all()  # an agent in the game has a nearest neighbour (at least the five taggers are in)


@pytest.mark.parametrize("E", [1, 9])
def test_rows_scribbled_between_two_launches(monkeypatch, E):
    """run(3) at a tagging distance that takes most runners out on the first tick, so that their rows are skipped on the
    third; then the host overwrites the array; trip 0 of the next launch must write all of it again"""
    cfg = dict(CFG, tagging_distance=0.2)
    one, multi = _engine(monkeypatch, E, False, cfg), _engine(monkeypatch, E, True, cfg)
    want = _run_chunks(one, multi, (3,))
    out = want["still_in_the_game"].reshape(E, N) == 0
    cleared = _pull(multi[0], "obs_rows_cleared").reshape(E, N)
    n_skippable = int((out & (cleared == 1)).sum())
    print("out of the game after 3 ticks:", int(out.sum()), "of", E * N, "flagged cleared:", n_skippable)
    assert n_skippable > 0
    assert (want["nearest_neighbor_ids"].reshape(E, N, K)[out & (cleared == 1)] == -1).all()
    _scribble_ids(one, multi)
    want = _run_chunks(one, multi, (2,))
    ids = _check_id_rows(want, E)
    assert (ids[out] == -1).all()  # (whoever was out stays out: the episode has 15 ticks)


@pytest.mark.parametrize("E", [1, 2, 9])
@pytest.mark.parametrize("tagging_distance", [1.0, 0.0])
def test_run_40(monkeypatch, E, tagging_distance):
    """run(40) with 15-tick episodes.  Distance 0.0: nobody leaves, two restores inside the launch.  Distance 1.0 (the
    margin is the grid length): nearly every runner is tagged on the first tick of an episode, so a replica is out of runners
    and restarts after a tick or two -- most trips run on reloaded state, next to agents that left on the trip before.  (The
    case in which agents leave at ticks of their own is test_arena_empties_below_K_agents.)"""
    _, want = _compare(monkeypatch, E, dict(CFG, tagging_distance=tagging_distance), (40,))
    out, t = int((want["still_in_the_game"] == 0).sum()), want["_timestep_"].reshape(-1)
    print("out of the game after 40 ticks:", out, "of", E * N, "time steps:", t)
    if tagging_distance == 0.0:
        assert out == 0 and (t == 40 % 15).all()
    else:
        assert (t != 40 % 15).any()  # episodes ended early: their runners were all out of the game


def test_arena_empties_below_K_agents(monkeypatch):
    """A tagging distance of a fifth of the arena, one long episode, chunks that end at live counts of every regime: more
    than 64 agents in the game (two wavefronts of searchers; trip 0), 16 .. 64 (the split search), fewer than 16, and at most
    K (rows with -1 entries, ranked out of slot order).  The agents leave at ticks of their own."""
    E = 9
    cfg = dict(CFG, tagging_distance=0.2, episode_length=110)
    one, multi = _engine(monkeypatch, E, False, cfg), _engine(monkeypatch, E, True, cfg)
    seen, padded = [], 0
    for chunk in (1, 1, 2, 4, 8, 15, 30, 30):
        want = _run_chunks(one, multi, (chunk,))
        sig = want["still_in_the_game"].reshape(E, N) != 0
        ids = want["nearest_neighbor_ids"].reshape(E, N, K)
        seen.append(sig.sum(axis=1))
        few = sig & (sig.sum(axis=1) <= K)[:, None]
        padded += int(((ids[few] >= 0).any(axis=1) & (ids[few] < 0).any(axis=1)).sum())
    seen = np.array(seen)
    print("agents in the game after each chunk, per replica:\n", seen, "\nrows with some but fewer than K ids:", padded)
    assert ((seen >= 16) & (seen <= 64)).any() and (seen < 16).any() and (seen <= K).any()
    assert padded > 0


def test_lattice_of_exact_ties_in_both_wavefronts(monkeypatch):
    """Nobody moves (both heads put all their mass on the no-op entry, speeds start at 0) and the agents stand on a square
    lattice: every agent has 4 others at distance 1, 4 at sqrt(2), 4 at 2 lattice steps -- K = 10 cuts the third ring, the
    tie is settled by id and the entries of a row do not come out in slot order, for agents of both wavefronts"""
    E = 2
    cfg = dict(CFG, tagging_distance=0.0)
    one, multi, taggers, runners = _pair_standing_still(monkeypatch, E, cfg)
    perm = np.stack([np.random.default_rng(5 + e).permutation(N) for e in range(E)])  # ids dealt at random
    x, y = np.zeros((E, N), dtype=f32), np.zeros((E, N), dtype=f32)
    for e in range(E):
        x[e, perm[e]] = f32(2.0) + f32(1.0) * (np.arange(N) % 15).astype(f32)
        y[e, perm[e]] = f32(3.0) + f32(1.0) * (np.arange(N) // 15).astype(f32)
    _write_positions(one, multi, x, y)
    want = _run_chunks(one, multi, (3,))
    assert (want["sampled_actions"] == 0).all() and not want["speed"].any()  # nobody moved
    # the K-th and the (K + 1)-th nearest are at the same distance for agents with ids on both sides of 64
    d2 = (x[:, :, None] - x[:, None, :]) ** 2 + (y[:, :, None] - y[:, None, :]) ** 2
    d2[:, np.arange(N), np.arange(N)] = np.inf
    srt = np.sort(d2, axis=2)
    tie = srt[:, :, K - 1] == srt[:, :, K]
    assert tie[:, :64].sum() > 20 and tie[:, 64:].sum() > 10
    ids = want["nearest_neighbor_ids"].reshape(E, N, K)
    assert (ids >= 0).all()
    # ... and the rows are the reference's: ascending distance, ties by id
    order = np.lexsort((np.broadcast_to(np.arange(N), d2.shape), d2), axis=2)[:, :, :K]
    assert np.array_equal(ids, order)


def test_restore_inside_a_launch(monkeypatch):
    """three-tick episodes in chunks (1, 2, 3, 5, 1, 8): restores land inside launches and between them; at this tagging
    distance agents are out of the game when the restore comes, and the trip after it runs on reloaded state"""
    E = 9
    cfg = dict(CFG, tagging_distance=0.2, episode_length=3)
    one, multi = _engine(monkeypatch, E, False, cfg), _engine(monkeypatch, E, True, cfg)
    outs = []
    for chunk in (1, 2, 3, 5, 1, 8):
        want = _run_chunks(one, multi, (chunk,))
        outs.append(int((want["still_in_the_game"] == 0).sum()))
    print("out of the game after each chunk:", outs)
    # ticks 1, 3, 6, 11, 12, 20: a restore follows ticks 3, 6, 12; after ticks 1, 11 and 20 agents are out
    assert outs[0] > 0 and outs[3] > 0 and outs[5] > 0


def test_runners_stay_in_the_game_after_a_tag(monkeypatch):
    _, want = _compare(monkeypatch, 2, dict(CFG, tagging_distance=1.0, runner_exits_game_after_tagged=False), (6,))
    assert (want["still_in_the_game"] != 0).all() and (want["rewards"] != 0).any()
