"""The standalone service kernels of csrc/kernels/wd_core.hip pinned draw for draw / bitwise on the MI355X.

The generator is counter based, so the host knows every uniform before the launch (oracle/core_np.py restates the
three draws; tests/test_core_draws_host.py checks the restatement).  Every test reads the device's RNG words, computes
what the launch must return, launches, and compares EVERY row at tolerance 0 -- indices, data, and the RNG words
afterwards (rows < n_rows advanced by exactly one, every other word and the header untouched).  The only tolerance in
this file is the float32 bound of the OU step against float64 (`_ou_compare`).

  sample_actions     vs oracle.core_np.sample_actions_counting (the closed form the kernel claims to compute); the
                     tie to the reference's prefix sum + binary search is made on the host, same rows, same uniforms
                     (`_host_tie`)
  sample_ou_process  vs a float64 evaluation from the same uniforms and the pushed float32 inputs
  resets, pool reset, logger   vs oracle.core_np.reset_when_done / pool_pick / plain numpy, bitwise

`pytest -s` prints the counted tie rows per case and the OU error ratios.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import core_np as o

pytestmark = pytest.mark.gpu

F32 = np.float32
TAG = 0x1234567          # stream tag of the direct launches
SEARCH_ROWS, SEARCH_EPOCHS = 8192, 512
# seeds whose end draws (u == 1.0 and u == 2^-24) fall inside SEARCH_ROWS x SEARCH_EPOCHS, so the search stays short;
# the tests still search (from the seed words the device's header holds) and fail if an end is not found
SEED_CAT, SEED_OU, SEED_POOL = 83, 293, 38


# ----------------------------------------------------------------------------------------------------- plumbing
@functools.lru_cache(maxsize=None)
def _ctx(E, N, T=1):
    """(data manager, function manager) of one (replicas, agents) shape, shared by the tests of this module"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.managers.data_manager import HIPDataManager
    from warp_drive_amd.managers.function_manager import HIPFunctionManager

    require_gpu()
    dm = HIPDataManager(num_agents=N, episode_length=T, num_envs=E)
    fm = HIPFunctionManager(num_agents=N, num_envs=E)
    fm.load_hip_from_binary_file()
    return dm, fm


def _sampler(E, N, seed):
    from warp_drive_amd.managers.function_manager import HIPSampler

    dm, fm = _ctx(E, N)
    s = HIPSampler(fm)
    s.init_random(seed=seed)
    return dm, fm, s


def _feed(**kw):
    from warp_drive_amd.utils.data_feed import DataFeed

    f = DataFeed()
    for k, v in kw.items():
        f.add_data(name=k, data=v)
    return f


def _words(ptr, n):
    """header + n epoch words of an RNG state"""
    from warp_drive_amd.managers import hip_driver as drv

    out = np.zeros(4 + n, dtype=np.uint32)
    torch.cuda.synchronize()
    drv.synchronize()
    drv.memcpy_dtoh(out, ptr)
    drv.synchronize()
    return out


def _set_epochs(ptr, epochs):
    from warp_drive_amd.managers import hip_driver as drv

    e = np.ascontiguousarray(epochs, dtype=np.uint32)
    drv.memcpy_htod(int(ptr) + 16, e)
    drv.synchronize()


def _check_words(before, after, n_rows, advance=1, moved=None):
    """rows < n_rows (or the rows of `moved`) advanced by exactly `advance` (mod 2^32); header and every other word
    untouched"""
    np.testing.assert_array_equal(after[:4], before[:4], err_msg="RNG header")
    step = np.zeros(len(before) - 4, dtype=np.uint32)
    if moved is None:
        step[:n_rows] = advance
    else:
        step[np.asarray(moved)] = advance
    np.testing.assert_array_equal(after[4:], before[4:] + step, err_msg="RNG epoch words")  # uint32: wraps


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random_rows(rng, n, A):
    p = rng.random_sample((n, A)) ** 2
    return (p / p.sum(-1, keepdims=True)).astype(F32)


@functools.lru_cache(maxsize=None)
def _end_draws(seed_lo, seed_hi, tag, counter3, words):
    """one search per (seed words, stream) and session"""
    return o.find_end_draws(seed_lo, seed_hi, tag, counter3, SEARCH_ROWS, SEARCH_EPOCHS, words=words)


# ---------------------------------------------------------------------------------------- the tie to the reference
TIE_TOTALS = {"rows": 0, "near_below": 0, "plateau": 0}


def _host_tie(p, u, expect_near_below=None):
    """The reference's prefix sum + binary search (1e-8 early exit) against the counting form, on the host, on the rows
    and uniforms of a device case.  Three kinds of row:

      clean       no prefix sum lies within 1e-8 of u without being equal to it, and at most one equals it:
                  the two must be EQUAL.
      near        exactly one prefix sum lies within 1e-8 of u without being equal (only the crafted one-ulp rows
                  with u < 0.125 can: above that a float32 ulp exceeds 1e-8).  If it is BELOW u the search's early
                  exit returns its index, one less than the count (it counts as `< u`; in the last entry the clamp
                  makes both A - 1); if above, both agree.  Which
                  rows are near-below is fixed by the construction: `expect_near_below` (default: none) is asserted
                  as a mask, not as an upper bound.
      plateau     several prefix sums EQUAL u (a tie followed by zero entries: one-hot and trailing-zero rows at
                  u == 1.0).  The counting form returns the first of them, the entry that carries the probability;
                  the binary search's early exit returns whichever of them it probes first.  Asserted: the search
                  lands inside the plateau and the count is its first index.
    Returns the counting result (what the device must give)."""
    p = np.asarray(p, dtype=F32)
    u = np.asarray(u, dtype=F32)
    cnt, srch = o.sample_actions_counting(p, u), o.sample_actions_search(p, u)
    cum = np.cumsum(p, axis=-1, dtype=F32)
    equal = cum == u[:, None]
    near = (np.abs((cum - u[:, None]).astype(F32)) < o.K_EPS) & ~equal
    plateau = equal.sum(-1) > 1
    near_row = near.any(-1)
    near_below = (near & (cum < u[:, None])).any(-1)
    assert not (near_row & plateau).any() and (near.sum(-1) <= 1).all()
    want_mask = np.zeros(len(u), dtype=bool) if expect_near_below is None else np.asarray(expect_near_below, dtype=bool)
    np.testing.assert_array_equal(near_below, want_mask, err_msg="rows with a prefix sum within 1e-8 below u")
    rest = ~plateau
    raw = (cum < u[:, None]).sum(-1).astype(np.int32)  # the count before the clamp: a near-below entry sits at raw - 1
    np.testing.assert_array_equal(srch[rest], np.where(near_below, raw - 1, cnt)[rest],
                                  err_msg="reference search vs counting form")
    assert (np.abs(srch - cnt)[rest] <= near_below[rest]).all()  # at most one index, towards the tied entry
    rows = np.flatnonzero(plateau)
    assert (cum[rows, srch[rows]] == u[rows]).all() and (cum[rows, cnt[rows]] == u[rows]).all()
    assert (cnt[rows] <= srch[rows]).all() and ((cnt[rows] == 0) | (cum[rows, np.maximum(cnt[rows] - 1, 0)] < u[rows])).all()
    # u == 1.0 on a row whose float32 sum is below 1: every prefix sum is < u, the clamp returns A - 1 even if that entry
    # is 0, and so does the reference's search
    short = (u == F32(1.0)) & (cum[:, -1] < F32(1.0))
    assert (cnt[short] == p.shape[1] - 1).all() and (srch[short] == p.shape[1] - 1).all()
    TIE_TOTALS["rows"] += len(u)
    TIE_TOTALS["near_below"] += int(near_below.sum())
    TIE_TOTALS["plateau"] += int(plateau.sum())
    return cnt


# -------------------------------------------------------------------------------------------------- sample_actions
def _launch_cat(s, distr, out, n_rows, A, block, stride, grid, tag=TAG, argmax=0, out_stride=1, out_offset=0):
    """sample_actions launched directly: the arguments of HIPSampler.categorical_launch with a geometry of the test's
    choice, and the dynamic LDS the kernel's header comment asks for (rows x stride x 4 + 128 bytes)"""
    from warp_drive_amd.managers import hip_driver as drv

    shared = block * stride * 4 + 128
    assert stride >= A and shared <= s.MAX_DYNAMIC_LDS and distr.numel() >= n_rows * A
    assert out.numel() >= (n_rows - 1) * out_stride + out_offset + 1 and 0 <= out_offset < out_stride
    s.sample_actions(s.rng_state, distr, out, drv.DevicePtr(0), np.int32(n_rows), np.int32(A), np.int32(argmax),
                     np.int32(stride), np.int32(tag), np.int32(out_stride), np.int32(out_offset),
                     block=(block, 1, 1), grid=(grid, 1), shared=shared)


def _fits(block, stride):
    return block * stride * 4 + 128 <= 64 * 1024


def _geometries(A):
    """[(name, block, lds_stride)]: the slab path (lds_stride == A, block a multiple of 64) and the padded path (any
    other stride or block), whatever the parity of A"""
    out = [(f"slab/{b}", b, A) for b in (64, 128, 256) if _fits(b, A)]
    out += [(f"padded/{b}+2", b, A + 2) for b in (256, 64) if _fits(b, A + 2)][:1]
    out += [(f"padded/{b}", b, A) for b in (96,) if _fits(b, A)]
    out += [(f"padded/8+{d}", 8, A + d) for d in (2, 0) if _fits(8, A + d)]
    return out


A_SWEEP = (2, 3, 4, 5, 21, 23, 24, 25, 26, 63, 64, 65, 127, 128, 255, 257, 511, 512, 1023, 2043)


def _rows_per_block(A):
    """what categorical_launch chooses"""
    stride, rows = A | 1, 256
    while rows > 8 and rows * stride * 4 + 128 > 64 * 1024:
        rows //= 2
    return rows


def test_launcher_covers_every_rows_per_block():
    """the sweep reaches every block size categorical_launch can choose, and both sides of every threshold"""
    assert sorted({_rows_per_block(A) for A in A_SWEEP}) == [8, 16, 32, 64, 128, 256]
    for lo_, hi_ in ((63, 64), (127, 128), (255, 257), (511, 512), (512, 1023)):
        assert _rows_per_block(lo_) > _rows_per_block(hi_)


@pytest.mark.parametrize("E,N", [(33, 5), (7, 9), (1, 1), (300, 7), (2000, 105)])
def test_sample_actions_sweep_through_the_launcher(E, N):
    """HIPSampler.sample at every A of the sweep (2000 x 105 rows: A <= 65, two launches), three consecutive launches
    each, so epochs > 0 are used"""
    from warp_drive_amd.managers.function_manager import _stream_tag

    dm, fm, s = _sampler(E, N, seed=11)
    n = E * N
    rng = np.random.RandomState(E)
    for A in A_SWEEP:
        if n * A > (1 << 24):
            continue
        name = f"sweep_{A}"
        if not dm.is_data_on_device(name):
            dm.push_data_to_device(_feed(**{name: np.full((E, N, 1), -1, dtype=np.int32)}), torch_accessible=True)
            s.register_actions(dm, name, A)
        p = _random_rows(rng, n, A)
        dist = _cuda(p.reshape(E, N, A))
        for launch in range(2 if n > 10000 else 3):
            before = _words(s.rng_state, n)
            u = o.categorical_uniform(np.arange(n), before[4:], before[0], before[1], _stream_tag(name))
            want = _host_tie(p, u)
            dm.data_on_device_via_torch(name).fill_(-1)
            s.sample(dm, dist, name)
            got = dm.pull_data_from_device(name).reshape(-1)
            np.testing.assert_array_equal(got, want, err_msg=f"A={A} launch {launch}")
            _check_words(before, _words(s.rng_state, n), n)


@pytest.mark.parametrize("A", A_SWEEP)
def test_sample_actions_both_paths_and_grid_stride_trips(A):
    """Both kernel paths at every A, whatever the host would choose, each with a full grid and with grids of 1, 3 and 7
    blocks (>= 5 trips of the largest block: a block refills its slab, the partial last wavefront falls into a late
    trip).  Epoch words preset to arbitrary 32-bit values; the RNG state has 100 words more than the launch has rows."""
    geoms = _geometries(A)
    big = max(b for _, b, _ in geoms)
    n = 7 * big * 4 + big // 4 + 37
    dm, fm, s = _sampler(1, n + 100, seed=12)
    rng = np.random.RandomState(A)
    p = _random_rows(rng, n, A)
    dist = _cuda(p)
    epochs = rng.randint(0, 1 << 32, size=n + 100, dtype=np.uint64).astype(np.uint32)
    hdr = _words(s.rng_state, 0)
    u = o.categorical_uniform(np.arange(n), epochs[:n], hdr[0], hdr[1], TAG)
    want = _host_tie(p, u)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    for name, block, stride in geoms:
        for grid in ((n + block - 1) // block, 1, 3, 7):
            _set_epochs(s.rng_state, epochs)
            before = _words(s.rng_state, n + 100)
            out.fill_(-1)
            _launch_cat(s, dist, out, n, A, block, stride, grid)
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"A={A} {name} grid={grid}")
            _check_words(before, _words(s.rng_state, n + 100), n)


@pytest.mark.parametrize("A", (21, 24))
@pytest.mark.parametrize("H", (2, 3))
def test_sample_actions_out_stride_and_offset(A, H):
    """head k of H goes straight into column k of one [rows, H] tensor (categorical_launch's out_stride / out_offset):
    column k equals the host's, the other columns keep what they held (a sentinel until their own launch).  The heads
    draw on the same rows with different stream tags: different, individually correct draws."""
    E, N = 300, 7
    n = E * N
    dm, fm, s = _sampler(E, N, seed=13)
    rng = np.random.RandomState(A * H)
    p = _random_rows(rng, n, A)
    dist = _cuda(p)
    out = torch.full((n, H), -7, dtype=torch.int32, device="cuda")
    expect = np.full((n, H), -7, dtype=np.int32)
    _set_epochs(s.rng_state, np.full(n, 5, dtype=np.uint32))
    same_epoch = []
    for k in range(H):
        tag = np.int32(1000 + k)
        before = _words(s.rng_state, n)
        u = o.categorical_uniform(np.arange(n), before[4:], before[0], before[1], tag)
        expect[:, k] = _host_tie(p, u)
        same_epoch.append(o.sample_actions_counting(p, o.categorical_uniform(np.arange(n), 5, before[0], before[1], tag)))
        fn, args, block, grid, shared = s.categorical_launch(dist, out, n, A, False, tag, out_stride=H, out_offset=k)
        fn(*args, block=block, grid=grid, shared=shared)
        np.testing.assert_array_equal(out.cpu().numpy(), expect, err_msg=f"head {k} of {H}")
        _check_words(before, _words(s.rng_state, n), n)
    # two tags, the same rows, the same epoch: different draws
    assert (same_epoch[0] != same_epoch[1]).mean() > 0.5


# crafted rows ------------------------------------------------------------------------------------------------------
TIE_KINDS = [(pos, rel) for pos in ("first", "middle", "last") for rel in ("equal", "below", "above")]
ROW_KINDS = TIE_KINDS + ["leading zeros", "inner zeros", "trailing zeros", "one hot", "sum below 1", "sum above 1",
                         "denormals", "all zeros"]


def _crafted_rows(u, A, shift, rng):
    """float32 rows built around the uniforms the launch WILL draw: row r is of kind ROW_KINDS[(r + shift) % len].
    Returns (rows, near_below mask the construction fixes)."""
    n, K = len(u), len(ROW_KINDS)
    kind = (np.arange(n) + shift) % K
    p = _random_rows(rng, n, A)
    near_below = np.zeros(n, dtype=bool)
    third = max(1, A // 3)
    for k, what in enumerate(ROW_KINDS):
        rows = np.flatnonzero(kind == k)
        if isinstance(what, tuple):
            # prefix sum at position j exactly u / one float32 below u / one above.  u is a multiple of 2^-24; the
            # entries before j are equal multiples of 2^-23 that add up to at most u / 2, so every prefix sum up to
            # j is exact; the entries after j are 2^-6 (prefix sums far from u)
            pos, rel = what
            j = {"first": 0, "middle": A // 2, "last": A - 1}[pos]
            uu = u[rows]
            target = {"equal": uu, "below": np.nextafter(uu, F32(0)), "above": np.nextafter(uu, F32(2))}[rel]
            per = (np.floor(uu.astype(np.float64) / 2 * 2.0 ** 23) // max(j, 1)) if j else np.zeros(len(rows))
            q = np.full((len(rows), A), F32(2.0 ** -6))
            q[:, :j] = (per * 2.0 ** -23).astype(F32)[:, None]
            q[:, j] = (target.astype(np.float64) - j * per * 2.0 ** -23).astype(F32)
            p[rows] = q
            assert (np.cumsum(q, axis=-1, dtype=F32)[:, j] == target).all(), "construction: prefix sum j is not exact"
            if rel == "below":  # within 1e-8 of u only where a float32 ulp is below 1e-8
                near_below[rows] = (uu.astype(np.float64) - target.astype(np.float64)) < 1e-8
        elif what == "leading zeros":
            p[rows, :third] = 0
        elif what == "inner zeros":
            p[rows, third:max(third + 1, 2 * third)] = 0
        elif what == "trailing zeros":
            p[rows, A - third:] = 0
        elif what == "one hot":  # every position as the rows go by
            p[rows] = np.eye(A, dtype=F32)[(rows // K) % A]
        elif what == "sum below 1":
            p[rows] *= F32(0.97)
        elif what == "sum above 1":
            p[rows] *= F32(1.03)
        elif what == "denormals":
            p[rows, ::2] = F32(1e-40)
            p[rows, 0] = F32(1.4e-45)
        elif what == "all zeros":
            p[rows] = 0
    return p, near_below, kind


@pytest.mark.parametrize("A", (3, 24, 25, 65))
def test_sample_actions_crafted_rows_and_end_draws(A):
    """Rows built around the known uniform, on both kernel paths; and the end draws: the epoch words of the rows the
    search found are preset so that every launch draws u == 1.0 and u == 2^-24 there, and the kind of every row moves
    by one per launch, so the end draws fall on rows of each kind.  Contract at u == 1.0 on a row whose float32 sum is
    below 1: the clamp returns A - 1 even if that entry is 0, and the reference's search does the same (`_host_tie`)."""
    n = SEARCH_ROWS + 37
    dm, fm, s = _sampler(1, n, seed=SEED_CAT)
    hdr = _words(s.rng_state, 0)
    assert (int(hdr[0]), int(hdr[1])) == o.seed_words(SEED_CAT)
    ends = _end_draws(int(hdr[0]), int(hdr[1]), TAG, 0, (0,))
    hi, lo = ends[(0, "hi")], ends[(0, "lo")]
    assert hi and lo, "the search found no end draw: pick another seed"
    rng = np.random.RandomState(A)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    slab = [(b, A) for b in (256, 64) if _fits(b, A)][:1]
    seen = set()
    for shift in range(len(ROW_KINDS)):
        epochs = np.full(n, shift, dtype=np.uint32)
        for row, epoch in hi + lo:
            epochs[row] = epoch
        u = o.categorical_uniform(np.arange(n), epochs, hdr[0], hdr[1], TAG)
        assert all(u[r] == F32(1.0) for r, _ in hi) and all(u[r] == F32(2.0 ** -24) for r, _ in lo)
        p, near_below, kind = _crafted_rows(u, A, shift, rng)
        seen |= {(int(kind[r]), "hi") for r, _ in hi} | {(int(kind[r]), "lo") for r, _ in lo}
        want = _host_tie(p, u, near_below)
        dist = _cuda(p)
        for block, stride in slab + [(256 if _fits(256, A + 2) else 64, A + 2), (8, A)]:
            _set_epochs(s.rng_state, epochs)
            before = _words(s.rng_state, n)
            out.fill_(-1)
            _launch_cat(s, dist, out, n, A, block, stride, (n + block - 1) // block)
            got = out.cpu().numpy()
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (f"A={A} shift={shift} block={block} stride={stride}: {len(bad)} rows differ, first "
                                   f"{bad[:5]} kinds {[ROW_KINDS[kind[b]] for b in bad[:5]]} got {got[bad[:5]]} "
                                   f"want {want[bad[:5]]} u {u[bad[:5]]}")
            _check_words(before, _words(s.rng_state, n), n)
    assert seen == {(k, e) for k in range(len(ROW_KINDS)) for e in ("hi", "lo")}
    print(f"A={A}: tie rows so far {TIE_TOTALS}")


def test_sample_actions_epoch_wrap():
    """epoch words preset to 0xFFFFFFFF / 0xFFFFFFFE: the draws equal the host's with that counter, the words wrap"""
    A, n = 21, 33 * 5
    dm, fm, s = _sampler(33, 5, seed=14)
    rng = np.random.RandomState(2)
    p = _random_rows(rng, n, A)
    dist = _cuda(p)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    epochs = np.where(np.arange(n) % 2 == 0, 0xFFFFFFFF, 0xFFFFFFFE).astype(np.uint32)
    _set_epochs(s.rng_state, epochs)
    for launch in range(3):
        before = _words(s.rng_state, n)
        u = o.categorical_uniform(np.arange(n), before[4:], before[0], before[1], TAG)
        fn, args, block, grid, shared = s.categorical_launch(dist, out, n, A, False, np.int32(TAG))
        fn(*args, block=block, grid=grid, shared=shared)
        np.testing.assert_array_equal(out.cpu().numpy(), _host_tie(p, u))
        _check_words(before, _words(s.rng_state, n), n)
    after = _words(s.rng_state, n)[4:]
    np.testing.assert_array_equal(after, np.where(np.arange(n) % 2 == 0, 2, 1).astype(np.uint32))


@pytest.mark.parametrize("A", (2, 24, 25, 257))
def test_sample_actions_argmax_ties(A):
    """first maximum wins: two and many equal maxima, a maximum in the last entry, negative and all-equal rows; the RNG
    words must not move"""
    n = 7 * 64 * 2 + 37
    dm, fm, s = _sampler(1, n, seed=15)
    rng = np.random.RandomState(A)
    p = rng.standard_normal((n, A)).astype(F32)
    kind = np.arange(n) % 6
    top = p.max(-1) + F32(1.0)
    r = np.flatnonzero(kind == 0)  # two equal maxima
    p[r, rng.randint(0, A, len(r))] = top[r]
    p[r, rng.randint(0, A, len(r))] = top[r]
    r = np.flatnonzero(kind == 1)  # many equal maxima
    p[r[:, None], rng.randint(0, A, (len(r), max(2, A // 2)))] = top[r, None]
    r = np.flatnonzero(kind == 2)  # the maximum in the last entry (and a copy of it nowhere else)
    p[r, A - 1] = top[r]
    r = np.flatnonzero(kind == 3)  # all negative
    p[r] = -np.abs(p[r]) - F32(0.5)
    r = np.flatnonzero(kind == 4)  # all equal
    p[r] = p[r, :1]
    want = o.sample_actions(p, None, use_argmax=True)
    np.testing.assert_array_equal(want, p.argmax(-1))  # the oracle's strict '<' scan is numpy's first maximum
    dist = _cuda(p)
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    _set_epochs(s.rng_state, np.arange(n, dtype=np.uint32) * 3)
    before = _words(s.rng_state, n)
    launches = [s.categorical_launch(dist, out, n, A, True, np.int32(TAG))]
    launches += [(None, None, (b, 1, 1), (g, 1), None) for b, g in ((64, 3), (96, 7), (8, 5)) if _fits(b, A | 1)]
    for fn, args, block, grid, shared in launches:
        out.fill_(-1)
        if fn is None:
            _launch_cat(s, dist, out, n, A, block[0], A | 1, grid[0], argmax=1)
        else:
            fn(*args, block=block, grid=grid, shared=shared)
        np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=f"A={A} block={block} grid={grid}")
        _check_words(before, _words(s.rng_state, n), n, advance=0)


@pytest.mark.parametrize("A", (3, 21, 24))
def test_sample_actions_padding_bytes_are_dead(A):
    """for A <= 24 the kernel reads 24 entries from a row's start and masks the rest.  The same case twice, the second
    time with `distr` a view into a larger tensor whose bytes before and after it are NaN / inf / huge: identical
    indices.  (Everything stays inside the allocation.)"""
    E, N = 33, 5
    n = E * N
    dm, fm, s = _sampler(E, N, seed=16)
    rng = np.random.RandomState(A)
    p = _random_rows(rng, n, A)
    pad = 64
    junk = np.tile(np.array([np.nan, np.inf, -np.inf, 3.0e38, -3.0e38, -1.0, 1.0, 0.5], dtype=F32), pad // 8)
    big = _cuda(np.concatenate([junk, p.reshape(-1), junk]))
    view = big[pad:pad + n * A]
    assert view.data_ptr() == big.data_ptr() + 4 * pad and view.is_contiguous()
    epochs = rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    hdr = _words(s.rng_state, 0)
    want = _host_tie(p, o.categorical_uniform(np.arange(n), epochs, hdr[0], hdr[1], TAG))
    for dist in (_cuda(p), view):
        for name, block, stride in _geometries(A):
            out = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            _set_epochs(s.rng_state, epochs)
            _launch_cat(s, dist, out, n, A, block, stride, 2)
            np.testing.assert_array_equal(out.cpu().numpy(), want, err_msg=name)
    torch.testing.assert_close(big[:pad].cpu(), torch.from_numpy(junk), rtol=0, atol=0, equal_nan=True)


# ----------------------------------------------------------------------------------------------- sample_ou_process
ULP32 = 2.0 ** -24
OU_RATIOS = {}


def _ou_compare(case, got_state, got_act, state0, distr, u1, u2, damping, stddev, scale):
    """The bound (the precedent of tests/test_gpu_policy_forward_shapes.py::_within_bound): the device's largest error
    against float64 in a launch is at most 4 x the largest error of the numpy float32 evaluation of the same formula
    against float64 on the same draws, with a floor of 8 float32 ulps of the largest compared value.  The float64
    reference uses the exact 2 pi; the float32 yardstick the kernel's float32 constant and float32 product.  The worst
    err / err_f32 per case is kept for the printout."""
    s64, a64 = o.ou_step_f64(state0, distr, u1, u2, damping, stddev, scale)
    s32, a32 = o.ou_step_f32(state0, distr, u1, u2, damping, stddev, scale)
    for kind, got, w64, w32 in (("state", got_state, s64, s32), ("action", got_act, a64, a32)):
        err = float(np.abs(got.astype(np.float64) - w64).max())
        err32 = float(np.abs(w32.astype(np.float64) - w64).max())
        scl = float(np.abs(w64).max())
        ratio = err / err32 if err32 > 0 else (float("inf") if err else 0.0)
        key = (case, kind)
        OU_RATIOS[key] = max(OU_RATIOS.get(key, 0.0), ratio)
        print(f"OU {case} {kind}: err {err:.3e} err_f32 {err32:.3e} ratio {ratio:.2f} scale {scl:.3g}")
        assert err <= max(4.0 * err32, 8.0 * ULP32 * scl), (case, kind, err, err32, scl)


def _launch_ou(s, distr, actions, state, damping, stddev, scale, n, grid=None, tag=TAG):
    """sample_ou_process with the arguments of HIPSampler.ou_launch on the test's own tensors"""
    grid = max(1, min(4096, (n + 255) // 256)) if grid is None else grid
    s.sample_ou_process(s.rng_state, distr, actions, state, np.float32(damping), np.float32(stddev), np.float32(scale),
                        np.int32(n), np.int32(tag), block=(256, 1, 1), grid=(grid, 1))


OU_PARAMS = [(0.15, 0.2, 1.0), (0.0, 0.2, 0.5), (1.0, 0.2, 1.0), (0.15, 0.0, 1.0), (0.15, 0.2, 1e-8), (1.0, 0.0, 0.5)]


@pytest.mark.parametrize("E,N,grid", [(33, 5, None), (7, 9, None), (1, 1, None), (2000, 105, None), (300, 7, 2)])
def test_ou_one_step_from_known_state(E, N, grid):
    """one step at a time from a pushed state: ou_state and actions of every row against float64, RNG words as for the
    sampler.  grid = 2: a direct launch whose blocks take several grid-stride trips."""
    n = E * N
    dm, fm, s = _sampler(1, n + 100, seed=21)
    rng = np.random.RandomState(n)
    actions = torch.empty(n, dtype=torch.float32, device="cuda")
    for damping, stddev, scale in OU_PARAMS:
        state0 = (rng.standard_normal(n) * 0.4).astype(F32)
        distr = rng.uniform(-1, 1, n).astype(F32)
        state, d = _cuda(state0), _cuda(distr)
        actions.fill_(float("nan"))
        before = _words(s.rng_state, n + 100)
        u1, u2 = o.ou_uniforms(np.arange(n), before[4:4 + n], before[0], before[1], TAG)
        _launch_ou(s, d, actions, state, damping, stddev, scale, n, grid)
        _ou_compare(f"{E}x{N} d={damping} s={stddev} c={scale}", state.cpu().numpy(), actions.cpu().numpy(), state0,
                    distr, u1, u2, damping, stddev, scale)
        _check_words(before, _words(s.rng_state, n + 100), n)
        np.testing.assert_array_equal(d.cpu().numpy(), distr)


def test_ou_through_the_product_launcher():
    """HIPSampler.sample on a registered deterministic action (its `_ou_state` in the data manager)"""
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.managers.function_manager import _stream_tag

    E, N = 33, 5
    n = E * N
    dm, fm, s = _sampler(E, N, seed=22)
    name = "ou_act"
    if not dm.is_data_on_device(name):
        dm.push_data_to_device(_feed(**{name: np.zeros((E, N, 1), dtype=np.float32)}), torch_accessible=True)
        s.register_actions(dm, name, 1, is_deterministic=True)
    rng = np.random.RandomState(5)
    state0 = (rng.standard_normal(n) * 0.4).astype(F32)
    drv.memcpy_htod(dm.device_data(f"{name}_ou_state"), state0)
    drv.synchronize()
    distr = rng.uniform(-1, 1, n).astype(F32)
    for step in range(3):
        before = _words(s.rng_state, n)
        u1, u2 = o.ou_uniforms(np.arange(n), before[4:], before[0], before[1], _stream_tag(name))
        s.sample(dm, _cuda(distr.reshape(E, N, 1)), name, damping=0.15, stddev=0.2, scale=0.5)
        got_state = dm.pull_data_from_device(f"{name}_ou_state").reshape(-1)
        _ou_compare(f"sample() step {step}", got_state, dm.pull_data_from_device(name).reshape(-1), state0, distr, u1,
                    u2, 0.15, 0.2, 0.5)
        _check_words(before, _words(s.rng_state, n), n)
        state0 = got_state


@pytest.mark.parametrize("scale", (0.99e-8, 0.0))
def test_ou_pass_through_below_the_cut(scale):
    """scale < 1e-8: actions == distr bitwise, state and RNG words untouched"""
    n = 2000 * 105 + 3
    dm, fm, s = _sampler(1, n, seed=23)
    rng = np.random.RandomState(1)
    distr = rng.standard_normal(n).astype(F32)
    distr[:4] = [np.nan, np.inf, -0.0, 1e-40]
    state0 = rng.standard_normal(n).astype(F32)
    state, d = _cuda(state0), _cuda(distr)
    actions = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    _set_epochs(s.rng_state, np.arange(n, dtype=np.uint32))
    before = _words(s.rng_state, n)
    _launch_ou(s, d, actions, state, 0.15, 0.2, scale, n)
    np.testing.assert_array_equal(actions.cpu().numpy().view(np.int32), distr.view(np.int32))
    np.testing.assert_array_equal(state.cpu().numpy().view(np.int32), state0.view(np.int32))
    _check_words(before, _words(s.rng_state, n), n, advance=0)


def test_ou_end_draws():
    """rows preset (counter word 3 = 1, both words) to u1 == 2^-24 (the largest normal the generator can make, 5.77),
    u1 == 1.0 (normal exactly 0) and u2 == 1.0"""
    n = SEARCH_ROWS + 37
    dm, fm, s = _sampler(1, n, seed=SEED_OU)
    hdr = _words(s.rng_state, 0)
    assert (int(hdr[0]), int(hdr[1])) == o.seed_words(SEED_OU)
    ends = _end_draws(int(hdr[0]), int(hdr[1]), TAG, 1, (0, 1))
    assert ends[(0, "hi")] and ends[(0, "lo")] and ends[(1, "hi")], "the search found no end draw: pick another seed"
    rng = np.random.RandomState(9)
    epochs = rng.randint(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    for key in ((0, "hi"), (0, "lo"), (1, "hi"), (1, "lo")):
        for row, epoch in ends[key]:
            epochs[row] = epoch
    _set_epochs(s.rng_state, epochs)
    before = _words(s.rng_state, n)
    u1, u2 = o.ou_uniforms(np.arange(n), epochs, hdr[0], hdr[1], TAG)
    r_hi, r_lo, r_u2 = ends[(0, "hi")][0][0], ends[(0, "lo")][0][0], ends[(1, "hi")][0][0]
    assert u1[r_hi] == F32(1.0) and u1[r_lo] == F32(2.0 ** -24) and u2[r_u2] == F32(1.0)
    state0 = (rng.standard_normal(n) * 0.4).astype(F32)
    distr = rng.uniform(-1, 1, n).astype(F32)
    state, d = _cuda(state0), _cuda(distr)
    actions = torch.empty(n, dtype=torch.float32, device="cuda")
    _launch_ou(s, d, actions, state, 0.15, 0.2, 1.0, n)
    got_state, got_act = state.cpu().numpy(), actions.cpu().numpy()
    _ou_compare("end draws", got_state, got_act, state0, distr, u1, u2, 0.15, 0.2, 1.0)
    _check_words(before, _words(s.rng_state, n), n)
    # u1 == 1.0: the normal is exactly 0, the state is the damped state to the bit
    assert got_state[r_hi] == (F32(1.0) - F32(0.15)) * state0[r_hi]
    # u1 == 2^-24: |normal| = sqrt(48 ln 2) * |cos(2 pi u2)|
    normal = (np.float64(got_state[r_lo]) - np.float64(F32(1.0) - F32(0.15)) * np.float64(state0[r_lo])) / np.float64(F32(0.2))
    assert abs(normal - o.box_muller_f64(u1[r_lo], u2[r_lo])) < 1e-5 and abs(normal) <= np.sqrt(48 * np.log(2.0)) + 1e-5


def test_ou_free_running_chain():
    """200 free-running steps; each step is compared with a float64 step fed the device's own previous state, so the
    error measured is one step's"""
    n = 33 * 5
    dm, fm, s = _sampler(33, 5, seed=24)
    rng = np.random.RandomState(3)
    distr = rng.uniform(-1, 1, n).astype(F32)
    prev = np.zeros(n, dtype=F32)
    state, d = _cuda(prev), _cuda(distr)
    actions = torch.empty(n, dtype=torch.float32, device="cuda")
    hdr = _words(s.rng_state, 0)
    import contextlib
    import io

    quiet = io.StringIO()
    for step in range(200):
        u1, u2 = o.ou_uniforms(np.arange(n), step, hdr[0], hdr[1], TAG)
        _launch_ou(s, d, actions, state, 0.15, 0.2, 1.0, n)
        got = state.cpu().numpy()
        with contextlib.redirect_stdout(quiet):
            _ou_compare("chain of 200", got, actions.cpu().numpy(), prev, distr, u1, u2, 0.15, 0.2, 1.0)
        prev = got
    np.testing.assert_array_equal(_words(s.rng_state, n)[4:], np.full(n, 200, dtype=np.uint32))
    assert prev.std() > 0.2  # the chain did move: stationary std is 0.38
    print("OU chain of 200: worst err / err_f32", {k[1]: f"{v:.2f}" for k, v in OU_RATIOS.items() if k[0] == "chain of 200"})


def test_ou_ratios_report():
    """the measured worst err / err_f32 per case (runs after the OU tests; docs/rounds/r09.md keeps the values)"""
    for (case, kind), ratio in sorted(OU_RATIOS.items()):
        print(f"OU worst err / err_f32  {case:40s} {kind:6s} {ratio:.2f}")
    print("sampler tie rows:", TIE_TOTALS)


# -------------------------------------------------------------------------------------------------------- resets
RESET_ROWS = ((1,), (3,), (255,), (256,), (257,), (1050,), (4, 105, 3))  # row_elems 1 .. 1260


def _reset_table(E):
    """12 arrays: RESET_ROWS and one without a row dimension, float32 and int32 in turn, and four more of the other
    type.  Every word differs from replica to replica and from array to array, so a copy from the wrong place shows"""
    arrays = {}
    shapes = [()] + list(RESET_ROWS)
    specs = [(sh, (np.int32, np.float32)[i % 2]) for i, sh in enumerate(shapes)]
    specs += [(sh, (np.float32, np.int32)[i % 2]) for i, sh in enumerate([(), (3,), (255,), (257,)])]
    for i, (shape, dtype) in enumerate(specs):
        n = E * int(np.prod(shape, dtype=np.int64))
        bits = ((np.arange(n, dtype=np.int64) * 2654435761 + i * 40503) % (1 << 23)).astype(np.int32)
        a = bits + np.int32(1) if dtype == np.int32 else (bits | np.int32(0x3F000000)).view(F32)  # floats in [0.5, 1)
        arrays[f"r{i}_{np.dtype(dtype).name}"] = a.reshape((E,) + shape)
    return arrays


def _done_patterns(E):
    idx = np.arange(E)
    return {"none": np.zeros(E, np.int32), "all": np.ones(E, np.int32), "every third": (idx % 3 == 0).astype(np.int32),
            "only the last": (idx == E - 1).astype(np.int32), "only >= 4096": (idx >= 4096).astype(np.int32)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(got, want, msg):
    """bitwise equality of two whole arrays (the quick check first: the arrays are large)"""
    if not np.array_equal(_bits(got), _bits(want)):
        np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=msg)
        raise AssertionError(msg)


@pytest.mark.parametrize("E", (1, 2, 4095, 4096, 4097, 10000))
def test_fused_reset_table_at_scale(E):
    """HIPEnvironmentReset.reset_when_done (one fused launch over the table, grid capped at 4096 blocks) against
    oracle.core_np.reset_when_done / undo_done_flag_and_reset_timestep, every word of every array, flags and
    `_timestep_` of every replica"""
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.managers.data_manager import HIPDataManager
    from warp_drive_amd.managers.function_manager import HIPEnvironmentReset, HIPFunctionManager
    from warp_drive_amd.utils.data_feed import DataFeed

    from tests.hip_harness import require_gpu

    require_gpu()
    dm = HIPDataManager(num_agents=5, episode_length=1, num_envs=E)
    fm = HIPFunctionManager(num_agents=5, num_envs=E)
    fm.load_hip_from_binary_file()
    resetter = HIPEnvironmentReset(fm)
    ref = _reset_table(E)
    assert len(ref) >= 12
    f = DataFeed()
    for k, v in ref.items():
        f.add_data(name=k, data=v, save_copy_and_apply_at_reset=True)
    dm.push_data_to_device(f, torch_accessible=True)
    assert dm.reset_data_list == list(ref)
    rng = np.random.RandomState(E)
    # undo_done_after_reset on and off in turn over the five patterns, then force_reset with each
    cases = [(name, done, "if_done", i % 2 == 0) for i, (name, done) in enumerate(_done_patterns(E).items())]
    cases += [("every third", _done_patterns(E)["every third"], "if_done", False),
              ("none", np.zeros(E, np.int32), "force_reset", True),
              ("every third", _done_patterns(E)["every third"], "force_reset", False)]
    for name, done, mode, undo in cases:
        scr = {}
        for k, v in ref.items():  # a different scramble per case, on the device
            t = dm.data_on_device_via_torch(k)
            t.fill_(-3)
            scr[k] = np.full(v.shape, -3, dtype=v.dtype)
        steps = rng.randint(1, 100, size=E).astype(np.int32)
        dm.data_on_device_via_torch("_done_").copy_(torch.from_numpy(done))
        drv.memcpy_htod(dm.device_data("_timestep_"), steps)
        drv.synchronize()
        resetter.reset_when_done(dm, mode=mode, undo_done_after_reset=undo)
        force = mode == "force_reset"
        for k, v in ref.items():
            want = o.reset_when_done(scr[k], v, done, force_reset=force)
            _same_bits(dm.pull_data_from_device(k), want, f"{name} {mode} {k}")
        want_done, want_steps = o.undo_done_flag_and_reset_timestep(done, steps, force) if undo else (done, steps)
        np.testing.assert_array_equal(dm.pull_data_from_device("_done_"), want_done, err_msg=f"{name} {mode} undo={undo}")
        np.testing.assert_array_equal(dm.pull_data_from_device("_timestep_"), want_steps, err_msg=f"{name} {mode} undo={undo}")


@pytest.mark.parametrize("dtype", (np.float32, np.int32))
@pytest.mark.parametrize("shape", ("reference", "few blocks"))
def test_reference_signature_reset_kernels(dtype, shape):
    """reset_in_{float,int}_when_done_{2d,3d} launched directly: with the reference's launch shape
    (block = (agents, 1, 1), grid = (envs, 1)) and with a wave64-friendly shape of fewer blocks than replicas"""
    E, agents, feat = 1000, 5, 7
    dm, fm = _ctx(E, agents)
    kind = "float" if dtype == np.float32 else "int"
    block, grid = ((agents, 1, 1), (E, 1)) if shape == "reference" else ((256, 1, 1), (7, 1))
    rng = np.random.RandomState(0)
    done = (rng.random_sample(E) < 0.4).astype(np.int32)
    for dims, inner in (("2d", (agents,)), ("3d", (agents, feat))):
        fn = fm.get_function(f"reset_in_{kind}_when_done_{dims}")
        ref = (rng.randint(1, 1 << 20, size=(E,) + inner)).astype(dtype)
        data = np.full_like(ref, -3)
        for force in (0, 1):
            d, r, dn = _cuda(data), _cuda(ref), _cuda(done)
            sizes = (np.int32(agents),) if dims == "2d" else (np.int32(agents), np.int32(feat))
            fn(d, r, dn, *sizes, np.int32(force), np.int32(E), block=block, grid=grid)
            want = o.reset_when_done(data, ref, done, force_reset=bool(force))
            np.testing.assert_array_equal(_bits(d.cpu().numpy()), _bits(want), err_msg=f"{kind} {dims} force={force}")
            np.testing.assert_array_equal(r.cpu().numpy(), ref)
            np.testing.assert_array_equal(dn.cpu().numpy(), done)


def test_undo_done_flag_alone_with_a_small_grid():
    E = 10000
    dm, fm = _ctx(E, 1)
    fn = fm.get_function("undo_done_flag_and_reset_timestep")
    rng = np.random.RandomState(1)
    for force in (0, 1):
        done = (rng.random_sample(E) < 0.3).astype(np.int32)
        steps = rng.randint(1, 500, size=E).astype(np.int32)
        d, t = _cuda(done), _cuda(steps)
        fn(d, t, np.int32(force), np.int32(E), block=(256, 1, 1), grid=(3, 1))
        want_d, want_t = o.undo_done_flag_and_reset_timestep(done, steps, bool(force))
        np.testing.assert_array_equal(d.cpu().numpy(), want_d)
        np.testing.assert_array_equal(t.cpu().numpy(), want_t)


# --------------------------------------------------------------------------------------------------- pool reset
def _pool_rng(fm, E, seed):
    """an RNG state of E words as init_random makes it (what init_reset_pool does)"""
    from warp_drive_amd.managers import hip_driver as drv

    state = drv.mem_alloc(4 * (4 + E))
    fm.get_function("init_random")(state, np.int32(seed & 0x7FFFFFFF), np.int32(E), block=(256, 1, 1),
                                   grid=(max(1, min(1024, (E + 255) // 256)), 1))
    return state


POOL_CASES = [(1, 1), (2, 257), (3, 1), (5, 300), (1000, 1050), (16384, 1024)]  # (n_pool, row_elems); the last: 64 MiB


@pytest.mark.parametrize("n_pool,row", POOL_CASES)
def test_reset_from_pool_every_replica(n_pool, row):
    """reset_when_done_from_pool launched with HIPEnvironmentReset's geometry against the host pick, every replica:
    two arrays of one reset call draw the same row (advance 0, then 1: the epochs move with the second launch only), a
    mixed done pattern (replicas that are not done keep data and epoch), and the two ends of p: replicas whose epoch
    word was preset so that p is the largest value below 1 (the pick is row n_pool - 1) and p == 0 (row 0)"""
    E = 10000
    dm, fm = _ctx(E, 1)
    fn = fm.get_function("reset_when_done_from_pool")
    state = _pool_rng(fm, E, SEED_POOL)
    try:
        hdr = _words(state, 0)
        assert (int(hdr[0]), int(hdr[1])) == o.seed_words(SEED_POOL)
        ends = _end_draws(int(hdr[0]), int(hdr[1]), o.POOL_STREAM_TAG, 2, (0,))
        hi, lo = ends[(0, "hi")], ends[(0, "lo")]
        assert hi and lo, "the search found no end draw: pick another seed"
        rng = np.random.RandomState(n_pool)
        epochs = rng.randint(0, 1 << 32, size=E, dtype=np.uint64).astype(np.uint32)
        for r, e in hi + lo:
            epochs[r] = e
        done = (rng.random_sample(E) < 0.6).astype(np.int32)
        for r, _ in hi + lo:
            done[r] = 1
        block, grid = (256, 1, 1), (max(1, min(E, 4096)), 1)
        # pool words: row * row_elems + column (and its negative for the second array), built on the device
        pool_a = torch.arange(n_pool * row, dtype=torch.int32, device="cuda").reshape(n_pool, row)
        pool_b = -pool_a - 1
        for force in (0, 1):
            _set_epochs(state, epochs)
            before = _words(state, E)
            hit = np.ones(E, bool) if force else done > 0
            pick = o.pool_pick(np.arange(E), epochs, hdr[0], hdr[1], n_pool)
            p = o.pool_p(np.arange(E), epochs, hdr[0], hdr[1])
            assert all(p[r] == F32(1 - 2.0 ** -24) and pick[r] == n_pool - 1 for r, _ in hi)
            assert all(p[r] == 0 and pick[r] == 0 for r, _ in lo)
            a = torch.full((E, row), -7, dtype=torch.int32, device="cuda")
            b = torch.full((E, row), -7, dtype=torch.int32, device="cuda")
            d = _cuda(done)
            cols = np.arange(row, dtype=np.int64)[None, :]
            want_a = np.where(hit[:, None], pick[:, None] * row + cols, -7).astype(np.int32)
            fn(state, a, pool_a, d, np.int32(row), np.int32(n_pool), np.int32(force), np.int32(E), np.int32(0),
               block=block, grid=grid)
            _check_words(before, _words(state, E), E, advance=0)
            fn(state, b, pool_b, d, np.int32(row), np.int32(n_pool), np.int32(force), np.int32(E), np.int32(1),
               block=block, grid=grid)
            np.testing.assert_array_equal(a.cpu().numpy(), want_a, err_msg=f"n_pool={n_pool} force={force} first array")
            np.testing.assert_array_equal(b.cpu().numpy(), np.where(hit[:, None], -want_a - 1, -7),
                                          err_msg=f"n_pool={n_pool} force={force} second array")
            _check_words(before, _words(state, E), E, moved=np.flatnonzero(hit))
            np.testing.assert_array_equal(d.cpu().numpy(), done)
    finally:
        state.free()


def test_reset_from_pool_through_the_product():
    """HIPEnvironmentReset.reset_when_done with two pooled arrays (float and int) and one table array: the pooled arrays
    of every replica hold the row the host picks from the pool's RNG words, which advance by one for finished replicas"""
    from warp_drive_amd.managers.data_manager import HIPDataManager
    from warp_drive_amd.managers.function_manager import HIPEnvironmentReset, HIPFunctionManager
    from warp_drive_amd.utils.data_feed import DataFeed

    from tests.hip_harness import require_gpu

    require_gpu()
    E, n_pool = 4097, 5
    dm = HIPDataManager(num_agents=3, episode_length=1, num_envs=E)
    fm = HIPFunctionManager(num_agents=3, num_envs=E)
    fm.load_hip_from_binary_file()
    resetter = HIPEnvironmentReset(fm)
    rng = np.random.RandomState(4)
    pool_a = rng.standard_normal((n_pool, 3, 100)).astype(F32)
    pool_b = rng.randint(0, 1000, size=(n_pool, 3)).astype(np.int32)
    table = rng.randint(0, 1000, size=(E, 3)).astype(np.int32)
    f = DataFeed()
    f.add_data(name="a", data=np.zeros((E, 3, 100), dtype=F32))
    f.add_data(name="b", data=np.zeros((E, 3), dtype=np.int32))
    f.add_data(name="c", data=table, save_copy_and_apply_at_reset=True)
    f.add_pool_for_reset(name="a_pool", data=pool_a, reset_target="a")
    f.add_pool_for_reset(name="b_pool", data=pool_b, reset_target="b")
    dm.push_data_to_device(f, torch_accessible=True)
    resetter.init_reset_pool(dm, seed=5)
    want_a, want_b = np.zeros((E, 3, 100), F32), np.zeros((E, 3), np.int32)
    for call in range(3):
        done = (rng.random_sample(E) < 0.5).astype(np.int32)
        dm.data_on_device_via_torch("_done_").copy_(torch.from_numpy(done))
        dm.data_on_device_via_torch("c").fill_(-3)
        before = _words(resetter._pool_rng, E)
        resetter.reset_when_done(dm, mode="if_done")
        hit = done > 0
        pick = o.pool_pick(np.arange(E), before[4:], before[0], before[1], n_pool)
        want_a[hit], want_b[hit] = pool_a[pick[hit]], pool_b[pick[hit]]
        np.testing.assert_array_equal(_bits(dm.pull_data_from_device("a")), _bits(want_a), err_msg=f"call {call}")
        np.testing.assert_array_equal(dm.pull_data_from_device("b"), want_b, err_msg=f"call {call}")
        np.testing.assert_array_equal(dm.pull_data_from_device("c"), o.reset_when_done(np.full_like(table, -3), table, done))
        np.testing.assert_array_equal(dm.pull_data_from_device("_done_"), 0)
        _check_words(before, _words(resetter._pool_rng, E), E, moved=np.flatnonzero(hit))


# ------------------------------------------------------------------------------------------------------- logger
@pytest.mark.parametrize("env_id", ("first", "last"))
def test_logger_rows_longer_than_a_block(env_id):
    """HIPLogController with env_id 0 and E - 1, float and int arrays of [E, agents, feature] whose replica rows are
    longer than a block (and than the launch: 16 800 words against 64 x 256 threads), a step equal to episode_length and
    one past it (which must leave the log and the mask untouched); fetch_log against the rows the test pushed"""
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.managers.data_manager import HIPDataManager
    from warp_drive_amd.managers.function_manager import HIPFunctionManager, HIPLogController
    from warp_drive_amd.utils.data_feed import DataFeed

    from tests.hip_harness import require_gpu

    require_gpu()
    E, N, T = 4, 7, 3
    env = 0 if env_id == "first" else E - 1
    dm = HIPDataManager(num_agents=N, episode_length=T, num_envs=E)
    fm = HIPFunctionManager(num_agents=N, num_envs=E)
    fm.load_hip_from_binary_file()
    log = HIPLogController(fm)
    shapes = {"xf": ((E, N, 2400), F32), "xi": ((E, N, 60, 5), np.int32), "yf": ((E, N), F32), "yi": ((E, N, 37), np.int32)}
    rng = np.random.RandomState(env)

    def fresh():
        return {k: (rng.standard_normal(sh).astype(dt) if dt == F32 else rng.randint(-1000, 1000, size=sh).astype(dt))
                for k, (sh, dt) in shapes.items()}

    pushed = [fresh()]
    f = DataFeed()
    for k, v in pushed[0].items():
        f.add_data(name=k, data=v, log_data_across_episode=True)
    dm.push_data_to_device(f)
    log.reset_log(dm, env_id=env)
    for step in range(1, T + 1):
        pushed.append(fresh())
        for k, v in pushed[-1].items():
            drv.memcpy_htod(dm.device_data(k), v)
        drv.synchronize()
        log.update_log(dm, step=step)
    got = log.fetch_log(dm)
    np.testing.assert_array_equal(dm.pull_data_from_device("_log_mask_"), np.ones(T + 1, np.int32))
    for k in shapes:
        want = np.stack([pushed[t][k][env] for t in range(T + 1)])
        np.testing.assert_array_equal(_bits(got[f"{k}_for_log"]), _bits(want), err_msg=k)
    # a shorter fetch
    short = log.fetch_log(dm, last_step=1)
    for k in shapes:
        np.testing.assert_array_equal(_bits(short[f"{k}_for_log"]), _bits(np.stack([pushed[t][k][env] for t in (0, 1)])))
    # one step past episode_length: the kernels must write nothing
    for k, v in fresh().items():
        drv.memcpy_htod(dm.device_data(k), v)
    drv.synchronize()
    log._log_one_step(dm, T + 1, env)
    log._function_manager.get_function("update_log_mask")(dm.device_data("_log_mask_"), np.int32(T + 1),
                                                          dm.meta_info("episode_length"), block=(64, 1, 1), grid=(1, 1))
    np.testing.assert_array_equal(dm.pull_data_from_device("_log_mask_"), np.ones(T + 1, np.int32))
    for k in shapes:
        want = np.stack([pushed[t][k][env] for t in range(T + 1)])
        np.testing.assert_array_equal(_bits(dm.pull_data_from_device(f"{k}_for_log")), _bits(want), err_msg=k)
    # reset_log clears the mask and logs step 0 again
    log.reset_log(dm, env_id=env)
    np.testing.assert_array_equal(dm.pull_data_from_device("_log_mask_"), [1] + [0] * T)
