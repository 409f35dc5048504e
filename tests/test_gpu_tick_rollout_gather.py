"""The multi-tick TagContinuous entry gathers the observation rows of its one built shape with what the shape fixes taken
out of the chunk loops (tc_rows.h: TcLeanDense / tc_gather_rows_dense_lean -- the chunk plan 19 / 19 / 15 and 19 / 19 / 14,
the own agent's live bit from the wavefront's vote, the time column from tfrac[0], per-chunk scalars advanced by
constants).  It must store the bytes the one-tick kernel stores, which keeps the generic gather: two engines start from
the same state, one is stepped with run(1) and one with run(n); the thirteen arrays and the RNG words are compared at
tolerance 0, with `observations` of both full of a sentinel before the first launch (the method of
tests/test_gpu_tick_rollout_rows.py, whose helpers are used).

`still_in_the_game` is crafted before the launch (tagging distance 0: the pattern holds) and every case asserts on the
host that the pattern it names occurs: which wavefront takes which form (sparse when live * 16 <= rows * 9: at most 29
live rows of 53 or 52), which rows of a dense chunk are out of the game, how many packed rows the sparse chunks hold.
E = 1, 2 and 9: 105 * 71 is odd, so nine consecutive replicas start at all four alignments of a row."""
import numpy as np
import pytest

from tests.test_gpu_tick_cohorts import CFG
from tests.test_gpu_tick_rollout_rows import N, SENTINEL, SPLIT, _pair, _pick, _rows, _run_chunks

pytestmark = pytest.mark.gpu

K, R_DENSE, R_SPARSE = 10, 19, 17   # neighbours per row; rows per dense / sparse chunk (tc_rows.h)
WAVES = ((0, SPLIT), (SPLIT, N))    # rows of wavefront 0 / 1


def _dense(n_live, rows):
    return n_live * 16 > rows * 9


def _forms(live):
    """[(replica, wavefront, live rows, dense?)]"""
    return [(e, w, int(live[e, lo:hi].sum()), _dense(int(live[e, lo:hi].sum()), hi - lo))
            for e in range(live.shape[0]) for w, (lo, hi) in enumerate(WAVES)]


def _chunk_edges(lo, hi):
    """first and last row of every dense chunk of a wavefront's rows [lo, hi)"""
    out = []
    for c0 in range(lo, hi, R_DENSE):
        out += [c0, min(c0 + R_DENSE, hi) - 1]
    return out


EDGES = [_chunk_edges(lo, hi) for lo, hi in WAVES]
assert EDGES == [[0, 18, 19, 37, 38, 52], [53, 71, 72, 90, 91, 104]]   # chunks of 19 / 19 / 15 and 19 / 19 / 14 rows


def _check_and_run(monkeypatch, live, ticks=2):
    E = live.shape[0]
    assert E in (1, 2, 9)
    one, multi = _pair(monkeypatch, E, dict(CFG, tagging_distance=0.0), live)
    want = _run_chunks(one, multi, (ticks,))
    # the pattern held, and the reference left no sentinel: every row was built or cleared
    assert np.array_equal((want["still_in_the_game"] & 1) != 0, live)
    assert not (want["observations"] == SENTINEL).any()
    obs = want["observations"].reshape(E, N, -1)
    assert not obs[~live].any()
    assert (obs[live][:, -1] != 0).all()   # the time column of every live row
    return want


@pytest.mark.parametrize("E", [1, 2, 9])
def test_every_agent_in_the_game(monkeypatch, E):
    """both wavefronts dense, no row out of the game: full chunks without a lane past the end but the last two of the
    third item, last chunks of 15 and 14 rows"""
    live = np.ones((E, N), dtype=bool)
    assert all(dense and n in (53, 52) for _, _, n, dense in _forms(live))
    want = _check_and_run(monkeypatch, live)
    assert (want["nearest_neighbor_ids"] >= 0).all()


def test_sparse_dense_threshold_per_wavefront(monkeypatch):
    """29 live rows of a wavefront's 53 or 52: the sparse form; 30: the dense form, one wavefront of each in a replica"""
    assert all(not _dense(29, rows) and _dense(30, rows) for rows in (SPLIT, N - SPLIT))
    per = []
    for e in range(9):
        n0, n1 = ((29, 30), (30, 29), (30, 30))[e % 3]
        per.append(_pick(10 + e, 0, SPLIT, n0) + _pick(30 + e, SPLIT, N, n1))
    live = _rows(9, *per)
    forms = _forms(live)
    assert {(n, d) for _, _, n, d in forms} == {(29, False), (30, True)}
    assert {(w, d) for _, w, _, d in forms} == {(0, False), (0, True), (1, False), (1, True)}
    _check_and_run(monkeypatch, live)


@pytest.mark.parametrize("E", [2, 9])
def test_dense_chunks_with_rows_out_of_the_game_at_their_edges(monkeypatch, E):
    """even replicas: the first and last row of every dense chunk -- and so of both wavefronts' ranges -- out of the game,
    everything else in it; odd replicas: those rows in the game and their inner neighbours out of it"""
    edge = np.zeros(N, dtype=bool)
    edge[EDGES[0] + EDGES[1]] = True
    inner = np.zeros(N, dtype=bool)
    inner[[1, 17, 20, 36, 39, 51, 54, 70, 73, 89, 92, 103]] = True
    live = np.stack([~edge if e % 2 == 0 else ~inner for e in range(E)])
    assert all(dense for _, _, _, dense in _forms(live))
    for e in range(E):
        for rows in EDGES:
            assert (live[e, rows] == (e % 2 == 1)).all()
    assert not live[0, [0, SPLIT - 1, SPLIT, N - 1]].any() and live[1, [0, SPLIT - 1, SPLIT, N - 1]].all()
    want = _check_and_run(monkeypatch, live)
    ids = want["nearest_neighbor_ids"].reshape(E, N, K)
    assert (ids[~live] == -1).all() and (ids[live] >= 0).all()


def test_dense_with_a_run_of_rows_out_of_the_game(monkeypatch):
    """a whole dense chunk out of the game (rows 19 .. 37 and 72 .. 90) in a wavefront that is still dense, at E = 1"""
    live = np.ones((1, N), dtype=bool)
    live[0, 19:38] = False
    live[0, 72:91] = False
    assert [(n, d) for _, _, n, d in _forms(live)] == [(34, True), (33, True)]
    _check_and_run(monkeypatch, live)


def test_sparse_chunks_of_17_18_and_1_rows(monkeypatch):
    """packed rows per wavefront: 17 (one full chunk), 18 (a last chunk of one row), 1; scattered and adjacent"""
    counts = [(17, 18), (18, 17), (1, 18), (18, 1), (17, 1), (1, 17), (18, 18), (17, 17), (1, 1)]
    per = []
    for e, (n0, n1) in enumerate(counts):
        if e % 2 == 0:
            per.append(_pick(50 + e, 0, SPLIT, n0) + _pick(70 + e, SPLIT, N, n1))
        else:   # adjacent rows at the end of wavefront 0's range and the start of wavefront 1's
            per.append(list(range(SPLIT - n0, SPLIT)) + list(range(SPLIT, SPLIT + n1)))
    live = _rows(9, *per)
    forms = _forms(live)
    assert all(not dense for _, _, _, dense in forms)
    assert [(forms[2 * e][2], forms[2 * e + 1][2]) for e in range(9)] == counts
    assert {n % R_SPARSE for _, _, n, _ in forms} == {0, 1} and {-(-n // R_SPARSE) for _, _, n, _ in forms} == {1, 2}
    _check_and_run(monkeypatch, live)


def test_live_rows_with_fewer_than_k_neighbours(monkeypatch):
    """6 and 10 agents in the game in a replica: 5 and 9 neighbours per live row, the other slots -1 and their values +0.0"""
    live = _rows(2, [3, 40, 52, 53, 77, 104], [0, 1, 2, 30, 52, 53, 54, 90, 103, 104])
    assert [int(r.sum()) for r in live] == [6, 10]
    want = _check_and_run(monkeypatch, live)
    ids = want["nearest_neighbor_ids"].reshape(2, N, K)
    rows = want["observations"].reshape(2, N, 7 * K + 1)
    for e, n in ((0, 5), (1, 9)):
        got = ids[e][live[e]]
        assert ((got >= 0).sum(axis=1) == n).all() and (got[:, n:] == -1).all()
        # the slots without a neighbour: every one of the seven feature groups holds +0.0 there
        feat = rows[e][live[e]][:, :7 * K].reshape(-1, 7, K)
        assert not feat[:, :, n:].any() and not np.signbit(feat[:, :, n:]).any()


def test_three_tick_episodes(monkeypatch):
    """E = 9, episodes of three ticks: every third trip restores and the next one reloads, launches of one tick among them;
    nobody is tagged, so every trip takes the dense form in both wavefronts"""
    one, multi = _pair(monkeypatch, 9, dict(CFG, episode_length=3, tagging_distance=0.0))
    want = _run_chunks(one, multi, (1, 2, 3, 5, 1, 8))
    assert not (want["observations"] == SENTINEL).any()
    assert ((want["still_in_the_game"] & 1) != 0).all()
    assert int(want["_timestep_"].max()) <= 3


def test_three_tick_episodes_with_tags(monkeypatch):
    """the same with tagging distance 1.0: replicas pass to the sparse form and restart inside the launches"""
    one, multi = _pair(monkeypatch, 9, dict(CFG, episode_length=3, tagging_distance=1.0))
    want = _run_chunks(one, multi, (1, 2, 3, 5, 1, 8))
    assert not (want["observations"] == SENTINEL).any()
