"""Host restatement of the three draws of the standalone service kernels (oracle/core_np.py): range of the uniform at
both ends, the search that finds end draws for the GPU tests, Box-Muller at the ends, the pool pick's `min` that never
binds, and the tie between the reference's binary search and the counting form at u == 1.0.  No GPU."""
import numpy as np
import pytest

from oracle import core_np as o

SEED = 7
N_ROWS, N_EPOCHS = 65536, 512


@pytest.fixture(scope="module")
def end_draws():
    """one search per session: the OU counter (word 3 = 1), words x and y, stream tag 0"""
    lo, hi = o.seed_words(SEED)
    return o.find_end_draws(lo, hi, 0, 1, N_ROWS, N_EPOCHS, words=(0, 1))


def test_seed_words_are_what_init_random_writes():
    assert o.seed_words(7) == (7, 0x5BD1E995)
    assert o.seed_words(-1) == (0x7FFFFFFF, 0x5BD1E995)
    assert o.seed_words((1 << 31) + 5) == (5, 0x5BD1E995)


def test_uniform_is_in_open_closed_unit_interval_for_every_value():
    """all 2^24 values of bits >> 8, with the 8 dropped bits all zero and all one"""
    top = np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)
    for low in (np.uint32(0), np.uint32(0xFF)):
        u = o.u01_open_closed(top | low)
        assert u.dtype == np.float32
        assert u.min() == np.float32(2.0 ** -24) and u.max() == np.float32(1.0)
        assert (u > 0).all() and (u <= 1).all()
        # exact: u * 2^24 is the integer (bits >> 8) + 1
        np.testing.assert_array_equal(u.astype(np.float64) * 2.0 ** 24, np.arange(1, (1 << 24) + 1, dtype=np.float64))
    assert o.u01_open_closed(np.uint32(0xFFFFFFFF)) == np.float32(1.0)
    assert o.u01_open_closed(np.uint32(0)) == np.float32(2.0 ** -24)


def test_search_finds_both_ends(end_draws):
    """2^25 draws hold about two of each end value; the (row, epoch) pairs below are known answers for seed words
    (7, 0x5bd1e995), tag 0, counter word 3 = 1: a change of the generator, of the counter layout or of the search
    shows here"""
    lo, hi = o.seed_words(SEED)
    assert end_draws[(0, "hi")] == [(25033, 361)]
    assert end_draws[(0, "lo")] == [(60652, 133), (63189, 165)]
    for w in (0, 1):
        for key, want in (("hi", np.float32(1.0)), ("lo", np.float32(2.0 ** -24))):
            assert len(end_draws[(w, key)]) >= 1, (w, key)
            for row, epoch in end_draws[(w, key)]:
                assert 0 <= row < N_ROWS and 0 <= epoch < N_EPOCHS
                assert o.ou_uniforms(np.uint32(row), np.uint32(epoch), lo, hi, 0)[w] == want
    # u1 == 2^-24 gives the largest normal the generator can make, u1 == 1.0 gives exactly 0
    row, epoch = end_draws[(0, "lo")][0]
    u1, u2 = o.ou_uniforms(np.uint32(row), np.uint32(epoch), lo, hi, 0)
    assert abs(o.box_muller_f64(u1, u2)) <= np.sqrt(48.0 * np.log(2.0))
    row, epoch = end_draws[(0, "hi")][0]
    assert o.box_muller_f64(*o.ou_uniforms(np.uint32(row), np.uint32(epoch), lo, hi, 0)) == 0.0


def test_vectorised_search_is_the_row_by_row_search():
    rng = np.random.RandomState(3)
    for A in (2, 3, 21, 24, 25, 65):
        p = rng.dirichlet(np.ones(A), size=600).astype(np.float32)
        p[::7, A // 2] = 0  # inner zeros, rows no longer normalised
        p[::11] = np.eye(A, dtype=np.float32)[rng.randint(0, A, size=len(p[::11]))]  # one-hot: plateaus of equal sums
        u = o.u01_open_closed(rng.randint(0, 1 << 32, size=600, dtype=np.uint64).astype(np.uint32))
        u[::5] = np.cumsum(p, axis=-1, dtype=np.float32)[::5, A // 3]  # exact ties
        u[::13] = np.float32(1.0)
        np.testing.assert_array_equal(o.sample_actions_search(p, u), o.sample_actions(p, u))


def test_draws_are_the_stated_philox_words():
    lo, hi = o.seed_words(123)
    rows = np.arange(1000, dtype=np.uint32)
    ep = (rows * np.uint32(7)) % np.uint32(13)
    tag = 0x1234567
    x0, _, _, _ = o.philox4x32_10(rows, ep, np.uint32(tag), np.uint32(0), lo, hi)
    x1, y1, _, _ = o.philox4x32_10(rows, ep, np.uint32(tag), np.uint32(1), lo, hi)
    x2, _, _, _ = o.philox4x32_10(rows, ep, np.uint32(o.POOL_STREAM_TAG), np.uint32(2), lo, hi)
    np.testing.assert_array_equal(o.categorical_uniform(rows, ep, lo, hi, tag), o.u01_open_closed(x0))
    u1, u2 = o.ou_uniforms(rows, ep, lo, hi, tag)
    np.testing.assert_array_equal(u1, o.u01_open_closed(x1))
    np.testing.assert_array_equal(u2, o.u01_open_closed(y1))
    p = o.pool_p(rows, ep, lo, hi)
    np.testing.assert_array_equal(p.astype(np.float64) * 2.0 ** 24, (x2 >> np.uint32(8)).astype(np.float64))
    assert p.min() >= 0 and p.max() < 1
    # the three streams differ, and so do two stream tags on the same rows
    assert (x0 != x1).mean() > 0.99 and (x1 != x2).mean() > 0.99
    assert (o.categorical_uniform(rows, ep, lo, hi, tag) != o.categorical_uniform(rows, ep, lo, hi, tag + 1)).mean() > 0.99


def test_box_muller_at_the_ends():
    one, tiny = np.float32(1.0), np.float32(2.0 ** -24)
    # u1 == 1.0: the normal is exactly 0 whatever u2; u1 == 2^-24: the largest magnitude, sqrt(48 ln 2) = 5.768
    assert o.box_muller_f64(one, np.float32(0.3)) == 0.0 and o.box_muller_f32(one, np.float32(0.3)) == 0.0
    big = o.box_muller_f64(tiny, one)
    assert abs(big - np.sqrt(48.0 * np.log(2.0))) < 1e-12 and 5.76 < big < 5.78
    assert abs(float(o.box_muller_f32(tiny, one)) - big) < 1e-5
    # float32 and float64 agree to float32 accuracy over random draws
    rng = np.random.RandomState(0)
    u1 = o.u01_open_closed(rng.randint(0, 1 << 32, size=100000, dtype=np.uint64).astype(np.uint32))
    u2 = o.u01_open_closed(rng.randint(0, 1 << 32, size=100000, dtype=np.uint64).astype(np.uint32))
    assert np.abs(o.box_muller_f32(u1, u2) - o.box_muller_f64(u1, u2)).max() < 1e-5


def test_ou_step_forms_agree_with_ou_step():
    rng = np.random.RandomState(1)
    s, d = rng.randn(500).astype(np.float32), rng.randn(500).astype(np.float32)
    u1 = o.u01_open_closed(rng.randint(0, 1 << 32, size=500, dtype=np.uint64).astype(np.uint32))
    u2 = o.u01_open_closed(rng.randint(0, 1 << 32, size=500, dtype=np.uint64).astype(np.uint32))
    ou32, a32 = o.ou_step_f32(s, d, u1, u2, 0.15, 0.2, 0.5)
    ou_ref, a_ref = o.ou_step(s, d, o.box_muller_f32(u1, u2), 0.15, 0.2, 0.5)
    np.testing.assert_array_equal(ou32, ou_ref)
    np.testing.assert_array_equal(a32, a_ref)
    ou64, a64 = o.ou_step_f64(s, d, u1, u2, 0.15, 0.2, 0.5)
    assert np.abs(ou64 - ou32).max() < 1e-5 and np.abs(a64 - a32).max() < 1e-5


POOL_SIZES = (1, 2, 3, 5, 8, 1000, 1 << 20, 1 << 24)


def test_pool_pick_ends_and_min_never_binds():
    """p == 0 picks row 0.  The largest p, 1 - 2^-24, picks row n_pool - 1 WITHOUT the min: in float32
    (1 - 2^-24) * n is n - n * 2^-24, which rounds to the float32 below n, never to n (asserted for every pool size up
    to 4096, the sizes the GPU tests use and the powers of two up to 2^24, where float32 still holds every row index)"""
    p_hi, p_lo = np.float32(1.0 - 2.0 ** -24), np.float32(0.0)
    assert p_hi < 1 and np.nextafter(p_hi, np.float32(2)) == 1
    for n in sorted(set(POOL_SIZES + tuple(range(1, 4097)) + tuple(1 << k for k in range(25)) + ((1 << 24) - 1,))):
        prod = p_hi * np.float32(n)
        assert prod < np.float32(n), n
        assert int(prod) == n - 1, n  # the min does not bind
        assert o.pool_pick_from_p(p_hi, n) == n - 1, n
        assert o.pool_pick_from_p(p_lo, n) == 0, n


def test_pool_pick_is_uniform_and_in_range():
    lo, hi = o.seed_words(5)
    envs = np.arange(200000, dtype=np.uint32)
    for n in (1, 2, 5, 1000):
        pick = o.pool_pick(envs, np.uint32(3), lo, hi, n)
        assert pick.min() >= 0 and pick.max() <= n - 1
        counts = np.bincount(pick, minlength=n)
        assert np.abs(counts - len(envs) / n).max() < 6 * np.sqrt(len(envs) / n) + 1


def test_reference_search_clamps_to_last_entry_at_u_one_on_a_short_row():
    """Contract at u == 1.0 on a row whose float32 sum is below 1: every prefix sum is < u, the counting form clamps to
    A - 1 even if that entry is 0 -- and the reference's binary search returns A - 1 too (asserted here on the host)."""
    for A in (2, 3, 24, 25, 65):
        row = np.zeros(A, dtype=np.float32)
        row[0] = 0.5  # sum 0.5, last entry 0
        assert o.sample_actions_counting(row[None], np.float32([1.0]))[0] == A - 1
        assert o.sample_actions(row[None], np.float32([1.0]))[0] == A - 1
        row[:] = np.float32(0.999) / A  # spread, sum below 1
        assert np.cumsum(row, dtype=np.float32)[-1] < 1
        assert o.sample_actions_counting(row[None], np.float32([1.0]))[0] == A - 1
        assert o.sample_actions(row[None], np.float32([1.0]))[0] == A - 1
        assert o.sample_actions(np.zeros((1, A), np.float32), np.float32([1.0]))[0] == A - 1  # all zeros
