"""The multi-tick TagContinuous entry splits wavefront 1's neighbour chain over the two halves of its lanes while 65 .. 96
agents are in the game (tc_fast.h "LANE HALVES": lane l + 32 chains the candidates [h, 2 h) for the searcher of lane l,
h = 4 * ((n_live + 7) >> 3); the places n_live .. 2 h - 1 hold pad candidates; the halves swap their keys and merge).
It must store the bytes the one-tick kernel stores, which searches as before: two engines start from the same state, one
is stepped with run(1) and one with run(n); the thirteen arrays and the RNG words are compared at tolerance 0 (the method
and the helpers of tests/test_gpu_tick_rollout_rows.py).

`still_in_the_game` is crafted before the launch (tagging distance 0: the count holds).  The cases that name a searcher
also craft the positions, with skill levels 0 so that nobody moves (the speed is clipped to max_speed * skill), and every
case asserts on the host what it claims: the number of agents in the game of every replica, h, the half each crafted
candidate falls into, that a tie is a tie in float32 -- and that the row the kernels stored for the searcher is the one
the host expects from (float32 distance, id).  E = 1, 2 and 9."""
import numpy as np
import pytest

from tests.test_gpu_tick_cohorts import CFG, _assert_same, _state
from tests.test_gpu_tick_rollout_rows import N, SENTINEL, _host_write, _pair, _run_chunks

pytestmark = pytest.mark.gpu

K = 10
f32 = np.float32
STILL = dict(CFG, tagging_distance=0.0, skill_level_runner=0.0, skill_level_tagger=0.0)   # nobody is tagged, nobody moves


def half_len(n_live):
    return 4 * ((n_live + 7) >> 3)


def in_regime(n_live):
    return 64 < n_live <= 96


def pads(n_live):
    return 2 * half_len(n_live) - n_live


def _live(n_live, how, seed=0):
    """[N] bool with n_live agents in the game: the others `scattered` over the ids, or `packed` at the low ids (so that
    every packed index differs from its id by the same N - n_live)"""
    live = np.ones(N, dtype=bool)
    dead = N - n_live
    if how == "packed":
        live[:dead] = False
    else:
        live[np.random.default_rng(seed).choice(N, size=dead, replace=False)] = False
    assert int(live.sum()) == n_live
    return live


def _ids_differ_from_packed(live):
    ids = np.flatnonzero(live)
    return (ids != np.arange(len(ids))).any()


# ---------------------------------------------------------------------------------------------- the regime's edges
# both edges of the regime (64 | 65, 96 | 97), every pad count 0 .. 7, and the whole replica
N_LIVE = [64, 65, 66, 67, 68, 69, 70, 71, 72, 80, 95, 96, 97, 105]
assert {pads(n) for n in N_LIVE if in_regime(n)} == set(range(8))
assert [in_regime(n) for n in (64, 65, 96, 97)] == [False, True, True, False]
assert all(2 * half_len(n) + 8 <= ((N + 3) & ~3) + 8 for n in range(65, 97))   # pads and the last prefetch: inside xyc


@pytest.mark.parametrize("n_live", N_LIVE)
def test_agents_in_the_game(monkeypatch, n_live):
    """E = 2, moving agents, run(3): replica 0 with the agents out of the game scattered, replica 1 with them packed at the
    low ids"""
    live = np.stack([_live(n_live, "scattered", seed=n_live), _live(n_live, "packed")])
    if n_live < N:
        assert _ids_differ_from_packed(live[0]) and _ids_differ_from_packed(live[1])
    one, multi = _pair(monkeypatch, 2, dict(CFG, tagging_distance=0.0), live)
    want = _run_chunks(one, multi, (3,))
    assert np.array_equal((want["still_in_the_game"] & 1) != 0, live)
    assert (live.sum(axis=1) == n_live).all()
    ids = want["nearest_neighbor_ids"].reshape(2, N, K)
    assert (ids[live] >= 0).all() and (ids[~live] == -1).all()
    assert live[np.arange(2)[:, None, None], np.where(ids < 0, 0, ids)][live].all()   # every neighbour is in the game
    assert not (want["observations"] == SENTINEL).any()


@pytest.mark.parametrize("E", [1, 9])
def test_replicas_at_counts_of_their_own(monkeypatch, E):
    """E = 1: 80 in the game; E = 9: a count per replica on both sides of both edges, alternately scattered and packed"""
    counts = [80] if E == 1 else [65, 96, 64, 97, 73, 88, 105, 81, 66]
    live = np.stack([_live(n, "packed" if e % 2 else "scattered", seed=100 + e) for e, n in enumerate(counts)])
    one, multi = _pair(monkeypatch, E, dict(CFG, tagging_distance=0.0), live)
    want = _run_chunks(one, multi, (2, 1))
    assert [int(r.sum()) for r in (want["still_in_the_game"] & 1)] == counts
    assert {in_regime(n) for n in counts} == ({True} if E == 1 else {True, False})


# ---------------------------------------------------------------------------------------------- crafted searchers
def _dist32(x, y, s):
    """float32 distances from agent s as the kernels form them: differences, squares and their sum rounded one by one"""
    dx, dy = (x[s] - x).astype(f32), (y[s] - y).astype(f32)
    d2 = ((dx * dx).astype(f32) + (dy * dy).astype(f32)).astype(f32)
    return d2, np.sqrt(d2, dtype=f32)


def _expected_row(x, y, live, s):
    d2, d = _dist32(x, y, s)
    cand = [j for j in np.flatnonzero(live) if j != s]
    return sorted(cand, key=lambda j: (d[j], j))


def _scene(live, c_s, placed, seed, centre=(8.0, 8.0), clear=6.0):
    """positions of one replica: the searcher (packed index c_s) at `centre`, the candidates of `placed` = {packed index:
    (dx, dy)} at centre + (dx, dy), everybody else at random at least `clear` from the centre.  Returns x, y, the
    searcher's id and the placed candidates' ids."""
    ids = np.flatnonzero(live)
    rng = np.random.default_rng(seed)
    x, y = np.empty(N, dtype=f32), np.empty(N, dtype=f32)
    for j in range(N):
        while True:
            px, py = rng.uniform(0.0, 20.0, size=2)
            if np.hypot(px - centre[0], py - centre[1]) >= clear:
                break
        x[j], y[j] = px, py
    s = int(ids[c_s])
    x[s], y[s] = centre
    out = {}
    for c, (dx, dy) in placed.items():
        assert c != c_s
        j = int(ids[c])
        x[j], y[j] = f32(centre[0]) + f32(dx), f32(centre[1]) + f32(dy)
        out[c] = j
    return x, y, s, out


def _run_scenes(monkeypatch, lives, scenes, ticks=2):
    """engines at E = len(scenes) with the crafted state; returns the final arrays"""
    E = len(scenes)
    assert E in (1, 2, 9)
    live = np.stack(lives)
    one, multi = _pair(monkeypatch, E, STILL, live)
    X, Y = np.stack([sc[0] for sc in scenes]), np.stack([sc[1] for sc in scenes])
    for w in (one[0], multi[0]):
        for name, val in (("loc_x", X), ("loc_y", Y)):
            def put(a, val=val):
                assert a.shape == val.shape and a.dtype == val.dtype
                a[:] = val

            _host_write(w, name, put)
    want = _run_chunks(one, multi, (ticks,))
    # nobody moved, nobody left: the crafted scene is the scene of every tick
    assert np.array_equal(want["loc_x"], X) and np.array_equal(want["loc_y"], Y)
    assert np.array_equal((want["still_in_the_game"] & 1) != 0, live)
    rows = want["nearest_neighbor_ids"].reshape(E, N, K)
    for e, (x, y, s, _) in enumerate(scenes):
        for j in np.flatnonzero(live[e]):   # every searcher of the replica, the crafted one among them
            assert list(rows[e, j]) == _expected_row(x, y, live[e], int(j))[:K], (e, int(j))
    return want, rows


def _ring(indices, r0=0.5, dr=0.11):
    """candidates at distinct, well separated distances r0, r0 + dr, .. around the searcher, in the order given"""
    return {c: ((r0 + dr * i) * np.cos(0.7 * i), (r0 + dr * i) * np.sin(0.7 * i)) for i, c in enumerate(indices)}


@pytest.mark.parametrize("n_live,how", [(80, "scattered"), (96, "packed"), (65, "scattered")])
def test_k_nearest_in_one_half_or_split(monkeypatch, n_live, how):
    """a searcher of wavefront 1 whose ten nearest all lie in [0, h) (replica 0), all in [h, n_live) (replica 1), five and
    five (replica 2, the nearer ones alternating between the halves); the other six replicas repeat the three with the
    last searcher of the wavefront"""
    h = half_len(n_live)
    assert in_regime(n_live) and 10 <= h and h + 10 <= n_live
    lives, scenes = [], []
    for e in range(9):
        live = _live(n_live, how, seed=7 * n_live + e)
        c_s = 64 if e < 3 else n_live - 1 if e < 6 else 64 + (n_live - 64) // 2
        assert c_s >= 64   # a searcher of wavefront 1
        lower = [c for c in range(3, h, max(1, h // 12)) if c != c_s][:10]
        upper = [c for c in range(n_live - 1, h - 1, -1) if c != c_s][:10]
        mixed = [c for pair in zip(lower[:5], upper[:5]) for c in pair]
        chosen = (lower, upper, mixed)[e % 3]
        assert len(chosen) == 10
        sides = [c >= h for c in chosen]
        assert sides == ([False] * 10, [True] * 10, [False, True] * 5)[e % 3]
        x, y, s, placed = _scene(live, c_s, _ring(chosen), seed=1000 + e)
        assert _expected_row(x, y, live, s)[:K] == [placed[c] for c in chosen]
        lives.append(live)
        scenes.append((x, y, s, placed))
    _run_scenes(monkeypatch, lives, scenes)


def test_lattice_of_exact_ties_across_the_halves(monkeypatch):
    """the searcher on a lattice point, four candidates at distance 1, four at sqrt(2), four at 2, each group with members
    in both halves: inside a group the lower id goes first whichever half found it, and of the four at distance 2 -- a tie
    at the cut -- the two lower ids are taken, one from each half"""
    n_live = 80
    h = half_len(n_live)
    lives, scenes = [], []
    for e, how in enumerate(("scattered", "packed")):
        live = _live(n_live, how, seed=31)
        c_s = 70
        g1 = [h - 5, h + 7, 2, n_live - 1]          # distance 1
        g2 = [h + 1, h - 1, h + 20, 5]              # distance sqrt(2)
        g3 = [h - 2, h + 3, h + 9, h + 4]           # distance 2: h - 2 and h + 3 are taken
        assert c_s not in g1 + g2 + g3
        for g in (g1, g2, g3):
            assert any(c < h for c in g) and any(c >= h for c in g)
        off1 = [(1, 0), (-1, 0), (0, 1), (0, -1)]
        off2 = [(1, 1), (-1, 1), (1, -1), (-1, -1)]
        off3 = [(2, 0), (0, 2), (-2, 0), (0, -2)]
        placed_at = {c: o for g, offs in ((g1, off1), (g2, off2), (g3, off3)) for c, o in zip(g, offs)}
        x, y, s, placed = _scene(live, c_s, placed_at, seed=2000 + e)
        d2, d = _dist32(x, y, s)
        for g, want_d2 in ((g1, 1.0), (g2, 2.0), (g3, 4.0)):
            assert all(d2[placed[c]] == f32(want_d2) for c in g)      # exact ties in float32
        row = _expected_row(x, y, live, s)
        assert row[:4] == sorted(placed[c] for c in g1) and row[4:8] == sorted(placed[c] for c in g2)
        assert row[8:10] == [placed[h - 2], placed[h + 3]] and set(row[10:12]) == {placed[h + 9], placed[h + 4]}
        lives.append(live)
        scenes.append((x, y, s, placed))
    _run_scenes(monkeypatch, lives, scenes)


def _near_pair(delta_ulps):
    """two offsets whose squared distances from the origin are 4 and 4 + about delta_ulps ulps"""
    b = f32(np.sqrt(np.float64(delta_ulps) * np.float64(np.spacing(f32(4.0)))))
    return (2.0, 0.0), (-2.0, float(b))


@pytest.mark.parametrize("at_the_cut", [False, True], ids=["inside_the_first_k", "at_the_cut"])
def test_pair_within_two_ulps_straddling_the_halves(monkeypatch, at_the_cut):
    """two candidates whose squared distances differ by at most 2 ulps, one in each half.  Inside the first K (entries 5 and
    6) the pair is settled by its exact keys; at the cut (entries 10 and 11) the chain's one look-ahead entry cannot
    decide and the whole wavefront resolves the lane (tc_zone_resolve).  Replica 0: the lower half holds the candidate at
    squared distance 4; replica 1: the upper half does"""
    n_live = 88
    h = half_len(n_live)
    lives, scenes = [], []
    for e in range(2):
        live = _live(n_live, "scattered", seed=55 + e)
        c_s = 64 + 11
        lo_c, up_c = h - 4, h + 6
        a, b = _near_pair(2)
        near = [4, h + 2, 9, h + 11] + ([] if not at_the_cut else [13, h + 15, 17, h + 19, 21])
        far = [] if at_the_cut else [13, h + 15, 17, h + 19]
        placed_at = dict(_ring(near, r0=0.4, dr=0.15))
        placed_at.update(_ring(far, r0=2.6, dr=0.15))
        first, second = (lo_c, up_c) if e == 0 else (up_c, lo_c)
        placed_at[first], placed_at[second] = a, b
        x, y, s, placed = _scene(live, c_s, placed_at, seed=3000 + e)
        d2, d = _dist32(x, y, s)
        gap = abs(int(d2[placed[second]].view(np.int32)) - int(d2[placed[first]].view(np.int32)))
        assert d2[placed[first]] == f32(4.0) and 1 <= gap <= 2
        assert (lo_c < h) and (up_c >= h)
        row = _expected_row(x, y, live, s)
        k0 = len(near)
        assert k0 == (9 if at_the_cut else 4)
        assert set(row[k0:k0 + 2]) == {placed[first], placed[second]}   # the pair is entries k0 + 1 and k0 + 2
        assert row[:k0] == [placed[c] for c in near]
        lives.append(live)
        scenes.append((x, y, s, placed))
    _run_scenes(monkeypatch, lives, scenes)


# ---------------------------------------------------------------------------------------------- episodes
def test_three_tick_episodes_with_tags(monkeypatch):
    """E = 9, episodes of three ticks, tagging distance 1.0, launches (1, 2, 3, 5, 1, 8): restores and reloads among trips of
    the split search"""
    one, multi = _pair(monkeypatch, 9, dict(CFG, episode_length=3, tagging_distance=1.0))
    want = _run_chunks(one, multi, (1, 2, 3, 5, 1, 8))
    assert not (want["observations"] == SENTINEL).any()


@pytest.mark.parametrize("tagging_distance", [1.0, 0.15])
def test_count_falls_through_the_regime_inside_a_launch(monkeypatch, tagging_distance):
    """E = 9, one run(40) from 100 agents in the game: the count passes 96 and 65 inside the launch.  Tagging distance 1.0:
    every runner within reach is tagged on the first tick and the count jumps over the regime (100 -> 5); 0.15: the count falls
    to about 75 on the first tick and stays inside the regime for 4 to 14 ticks of every replica before it leaves it below"""
    live = np.stack([_live(100, "scattered", seed=400 + e) for e in range(9)])
    cfg = dict(CFG, episode_length=500, tagging_distance=tagging_distance)   # (no restart inside the launch)
    one, multi = _pair(monkeypatch, 9, cfg, live)
    (w1, s1, ref, _), (wr, sr, eng, _) = one, multi
    counts = [live.sum(axis=1)]
    for _ in range(40):
        ref.run(1)
        counts.append((w1.cuda_data_manager.pull_data_from_device("still_in_the_game") & 1).sum(axis=1))
    eng.run(40)
    _assert_same(_state(wr, sr), _state(w1, s1), "after run(40)")
    counts = np.stack(counts).T   # [9, 41]
    for e, col in enumerate(counts):
        print(f"tagging distance {tagging_distance}, replica {e}: agents in the game before each tick:", list(col))
    # the ticks of the launch start from these counts (the last entry is what the launch left)
    assert (counts[:, 0] == 100).all() and (counts[:, -1] < 65).all()    # every replica passes 96 and 65 inside the launch
    inside = np.array([sum(in_regime(c) for c in col[:-1]) for col in counts])
    print("ticks searched in the regime, per replica:", list(inside))
    if tagging_distance < 1.0:
        assert (inside >= 3).all()
