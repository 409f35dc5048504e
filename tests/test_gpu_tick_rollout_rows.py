"""The multi-tick TagContinuous entry flushes the rows of its sparse form from per-row descriptors (tc_rows.h, TcLeanRows:
head / tail action, alignment and byte offset of a packed row, formed once per chunk and fetched per flush round).  It
must store the bytes the one-tick kernel stores: two engines start from the same state, one is stepped with run(1) (the
one-tick entry) and one with run(n); the thirteen arrays and the RNG words are compared at tolerance 0.

`observations` of both engines is filled with a sentinel before the first launch, so a dword that the flush misses, or one
it does not own and writes, differs from the reference.  `still_in_the_game` is crafted before the launch (tagging
distance 0: the pattern holds) to put the head / tail rules, the chunk edge (17 packed rows), the wavefront split
(rows 0 .. 52 | 53 .. 104), the switch between the sparse and the dense form (at most 29 live rows of a wavefront's 53
or 52) and the 16-byte lines shared by the last row of a replica and the first row of the next under test."""
import numpy as np
import pytest
import torch

from tests.test_gpu_tick_cohorts import ARRAYS, CFG, _assert_same, _state
from tests.test_gpu_tick_rollout_straight import _engine

pytestmark = pytest.mark.gpu

N, SPLIT = 105, 53
SENTINEL = np.float32(-12345.678)


def _host_write(w, name, fn):
    from warp_drive_amd.managers import hip_driver as drv

    dm = w.cuda_data_manager
    host = np.ascontiguousarray(dm.pull_data_from_device(name))
    fn(host)
    drv.memcpy_htod(dm.device_data(name), host)


def _pair(monkeypatch, E, cfg, live=None):
    """both engines, `observations` full of the sentinel, `still_in_the_game` = live ([E, N] bool) if given"""
    one = _engine(monkeypatch, E, False, cfg)
    multi = _engine(monkeypatch, E, True, cfg)
    torch.cuda.synchronize()
    for w in (one[0], multi[0]):
        _host_write(w, "observations", lambda o: o.fill(SENTINEL))
        if live is not None:
            def craft(sig):
                assert sig.shape == live.shape
                sig[:] = live.astype(sig.dtype)

            _host_write(w, "still_in_the_game", craft)
            # the rows of the agents taken out still hold the sentinel: nothing is known to be cleared
            _host_write(w, "obs_rows_cleared", lambda c: c.fill(0))
    torch.cuda.synchronize()
    return one, multi


def _run_chunks(one, multi, chunks):
    (w1, s1, ref, _), (wr, sr, eng, _) = one, multi
    done, want = 0, None
    for chunk in chunks:
        for _ in range(chunk):
            ref.run(1)
        eng.run(chunk)
        done += chunk
        got, want = _state(wr, sr), _state(w1, s1)
        assert set(ARRAYS) < set(got) and "rng_state" in got
        _assert_same(got, want, f"after {done} ticks (last run({chunk}))")
    return want


def _rows(E, *per_replica):
    live = np.zeros((E, N), dtype=bool)
    assert len(per_replica) == E
    for e, rows in enumerate(per_replica):
        live[e, list(rows)] = True
    return live


def _pick(seed, lo, hi, n):
    """n rows of [lo, hi), a fixed choice"""
    return sorted(lo + np.random.default_rng(seed).choice(hi - lo, size=n, replace=False))


def _patterns():
    p = {}
    # every live row has dead neighbours on both sides: full lines at either end, no merge, no skip
    p["alternating"] = _rows(2, range(0, N, 2), range(1, N, 2))
    # one live row in a replica: the other wavefront has none; rows at both ends of a wavefront's rows and of a chunk
    p["one_live_row"] = _rows(9, *[[r] for r in (0, 1, 17, 52, 53, 70, 103, 104, 16)])
    # a run of live rows across the wavefront split: own dwords on both sides of rows 52 | 53
    p["run_across_the_split"] = _rows(1, range(45, 61))
    # more than 17 live rows in a wavefront, the chunk edge (packed rows 16 | 17) inside a run of adjacent rows
    p["chunk_edge_inside_a_run"] = _rows(2, list(range(0, 20)) + list(range(60, 85)),
                                         list(range(5, 29)) + list(range(53, 81)))
    # 29 live rows of a wavefront: the sparse form; 30: the dense one (29 * 16 <= 9 * 52 < 9 * 53 < 30 * 16)
    assert all(29 * 16 <= rows * 9 < 30 * 16 for rows in (SPLIT, N - SPLIT))
    p["29_and_30_live_rows"] = _rows(3, _pick(1, 0, SPLIT, 29) + _pick(2, SPLIT, N, 29),
                                     _pick(3, 0, SPLIT, 30) + _pick(4, SPLIT, N, 30),
                                     list(range(0, 29)) + list(range(N - 30, N)))
    # the line shared by row 104 of a replica and row 0 of the next: both live, both dead, one of each
    p["shared_lines_live"] = _rows(3, [0, 50, 104], [0, 104], [0, 1, 103, 104])
    p["shared_lines_dead"] = _rows(3, [1, 2, 3, 101, 102, 103], [1, 103], [1, 52, 53, 103])
    p["shared_lines_mixed"] = _rows(9, *[([0] if e & 1 else [1]) + ([104] if e & 2 else [103]) + [30 + e, 60 + e]
                                         for e in range(9)])
    return p


PATTERNS = _patterns()


@pytest.mark.parametrize("name", list(PATTERNS))
def test_crafted_live_rows(monkeypatch, name):
    """tagging distance 0, run(2): the first trip clears the rows of the agents taken out and builds the live ones, the
    second builds the live ones again with the cleared flags carried in registers"""
    live = PATTERNS[name]
    E = live.shape[0]
    assert E in (1, 2, 3, 9)
    one, multi = _pair(monkeypatch, E, dict(CFG, tagging_distance=0.0), live)
    want = _run_chunks(one, multi, (2,))
    # the pattern held, and the reference left no sentinel: every row was built or cleared
    assert np.array_equal((want["still_in_the_game"] & 1) != 0, live)
    assert not (want["observations"] == SENTINEL).any()
    obs = want["observations"].reshape(E, N, -1)
    assert not obs[~live].any()


def test_rows_die_tick_by_tick(monkeypatch):
    """E = 9, tagging distance 1.0, run(40): agents leave the game at ticks of their own, their rows are cleared once, the
    wavefronts pass from the dense to the sparse form, episodes restart inside the launch"""
    one, multi = _pair(monkeypatch, 9, dict(CFG, tagging_distance=1.0))
    want = _run_chunks(one, multi, (40,))
    assert not (want["observations"] == SENTINEL).any()


def test_restore_and_reload(monkeypatch):
    """E = 9, three-tick episodes: every third trip restores, launches of one tick among them"""
    one, multi = _pair(monkeypatch, 9, dict(CFG, episode_length=3))
    want = _run_chunks(one, multi, (1, 2, 3, 5, 1, 8))
    assert not (want["observations"] == SENTINEL).any()
