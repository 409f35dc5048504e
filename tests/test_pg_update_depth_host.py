"""Host side of tests/test_gpu_pg_update_depth.py (no GPU): the cases beside `pc.CASES` -- the matrix entry's wavefront
edges (`WAVE_CASES`), a batch with more tiles than the wrapper launches blocks (`GRID_CASES`), one block on 160 trips
(`DEPTH_CASES`) and inputs with out-of-range actions -- hold what they promise, their yardsticks agree with float64 autograd,
every planted defect still breaks the bound at 20 385 and 65 984 rows, and the wrapper picks the grids and trip counts the
GPU file relies on."""
import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests.test_pg_update_host import (RESULT_KEYS, _MUST_BREAK, _Recorder, _violations, check_float64_agreement, check_inputs,
                                       check_returns_model)
from warp_drive_amd.training import pg_update_kernels as pguk

f32, f64 = np.float32, np.float64
LARGE_CASES = pc.GRID_CASES + pc.DEPTH_CASES
NEW_CASES = pc.WAVE_CASES + LARGE_CASES
WORKLOAD_ROWS = 5_000_000          # the batch README's timing recommends the matrix entry at
DEVICE_COMPUTE_UNITS = 256         # of the MI355X


@pytest.fixture(scope="module")
def references():
    """case name -> (inputs, the float64 yardstick, float64 and float32 autograd on the CPU): computed once per case, on
    first use, never changed"""
    cache = {}

    def get(case):
        if case.name not in cache:
            inp = pc.inputs(case)
            cache[case.name] = (inp, pc.yardstick(case, inp), pc.framework(case, inp, torch.float64),
                                pc.framework(case, inp, torch.float32))
        return cache[case.name]

    return get


def _last_tile(case):
    return (case.E * case.T - 1) % pc.TILE + 1


def test_the_new_cases_are_what_they_say():
    assert len(pc.CASES) == 12 and not {c.name for c in NEW_CASES} & {c.name for c in pc.CASES}
    assert len({c.name for c in NEW_CASES}) == len(NEW_CASES) and all(c.grid is None and not c.gap for c in NEW_CASES)
    seeds = [c.seed for c in NEW_CASES]
    assert min(seeds) >= 21 and seeds[:4] == [21, 22, 23, 24] and len(set(seeds)) == len(seeds) and not set(seeds) & {c.seed for c in pc.CASES}
    # wavefront edges: 32 rows to a wavefront, four wavefronts to a tile
    assert [(c.E, c.T, c.E * c.T) for c in pc.WAVE_CASES] == [(16, 2, 32), (11, 3, 33), (32, 3, 96), (15, 15, 225)]
    assert [(pc.case_tiles(c), _last_tile(c)) for c in pc.WAVE_CASES] == [(1, 32), (1, 33), (1, 96), (2, 97)]
    assert sorted(c.H for c in pc.WAVE_CASES) == [32, 32, 64, 64] and {c.A for c in pc.WAVE_CASES} == {1, 2, 3, 8}
    shapes = {(c.H, c.O) for c in NEW_CASES}
    assert shapes == {(H, O) for H in pguk.HIDDEN for O in pguk.OBS_SIZES} and len({(c.H, c.O) for c in pc.WAVE_CASES}) == 4
    # the wrapper's grid and the workload's depth
    for cases, E, T, rows, tiles, last in ((pc.GRID_CASES, 1031, 64, 65984, 516, 64), (pc.DEPTH_CASES, 4077, 5, 20385, 160, 33)):
        assert [(c.E, c.T, c.E * c.T, pc.case_tiles(c), _last_tile(c)) for c in cases] == [(E, T, rows, tiles, last)] * 2
        assert [(c.H, c.O, c.A) for c in cases] == [(32, 4, 2), (64, 6, 3)] and {c.algo for c in cases} == {"A2C", "PPO"}
        assert all(c.done == "value 2" for c in cases)
    assert [c.algo for c in pc.GRID_CASES] == ["PPO", "A2C"]
    assert [(c.A, c.E * c.T, c.ent) for c in pc.OUT_OF_RANGE_CASES] == [(8, 325, 0.0), (2, 126, 0.1)]


@pytest.mark.parametrize("case", NEW_CASES, ids=lambda c: c.name)
def test_inputs_hold_what_the_cases_promise(case, references):
    inp, want, _, _ = references(case)
    check_inputs(case, inp, want)
    if case in LARGE_CASES:      # no row whose relu branch a float32 evaluation decides by its rounding (pc.RELU_MARGIN)
        net = {k: v.astype(f64) for k, v in pc.unflatten(inp["theta"], case.H, case.O, case.A).items()}
        _, _, (_, z1, _, z2, _) = pc.forward64(net, inp["obs"].astype(f64).reshape(-1, case.O))
        for z, zero_units in ((z1, (1, case.H - 2)), (z2, (2, case.H - 1))):
            live = np.delete(np.abs(z), zero_units, axis=1)
            assert live.min() >= pc.RELU_MARGIN, (case.name, live.min())


@pytest.mark.parametrize("case", NEW_CASES, ids=lambda c: c.name)
def test_written_out_float64_pass_agrees_with_float64_autograd(case, references):
    """within tests/test_pg_update_host.py's 1e-11, end to end and on given values"""
    check_float64_agreement(case, *references(case))


@pytest.mark.parametrize("case", NEW_CASES, ids=lambda c: c.name)
def test_returns_model_is_discounted_returns_bit_for_bit(case, references):
    """(T = 64 is the longest chain of the suite)"""
    inp, _, _, auto32 = references(case)
    check_returns_model(case, inp, auto32)


@pytest.mark.parametrize("case", NEW_CASES, ids=lambda c: c.name)
def test_the_unmutated_yardstick_passes_its_own_bound(case, references):
    _, want, _, auto32 = references(case)
    rounded = {k: np.asarray(want[k], f64).astype(f32).astype(f64) for k in RESULT_KEYS}
    assert not _violations(rounded, want, auto32, RESULT_KEYS), case.name


@pytest.mark.parametrize("case", LARGE_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("mutation", pc.MUTATIONS)
def test_a_planted_defect_breaks_the_bound(mutation, case, references):
    """on EVERY grid and depth case: 33 rows of 20 385 left out, or 64 of 65 984, do not hide under the bound"""
    assert pc.mutation_applies(case, mutation), (mutation, case.name)     # all six apply to all four
    inp, want, _, auto32 = references(case)
    broken = set(_violations(pc.yardstick(case, inp, mutate=mutation), want, auto32, RESULT_KEYS))
    assert broken >= _MUST_BREAK[mutation], (mutation, case.name, sorted(broken))


# -------------------------------------------------------------------------------------------- grids and trip counts
def _recorded_grid(case, entry, compute_units):
    """(blocks launched, rows of the wrapper's partials, tiles) of the gradient launch, through the recording manager"""
    rec = _Recorder()
    T, E, H, O, A = case.T, case.E, case.H, case.O, case.A
    k = pguk.PgUpdateKernels(rec, E, T, H, O, A, "cpu", compute_units=compute_units, gradients_entry=entry)
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)  # noqa: E731
    k.gradients(z(T, E, 1, O), z(T, E, 1, 1, dtype=torch.int32), z(k.P), case.ent, case.vf)
    (name, args, block, grid, _), = rec.launches
    assert name == pguk.gradients_entry_name(H, O, entry) and block[0] == (256 if entry == "matrix" else 128)
    assert int(args[5]) == T * E and grid[0] == k.gradients_grid == k.partials.shape[0] and k.tiles == pc.case_tiles(case)
    return grid[0], k.tiles


def _trips(tiles, grid):
    """the most trips a block makes: block b takes tiles b, b + grid, ..."""
    return -(-tiles // grid)


@pytest.mark.parametrize("entry", pguk.GRADIENTS_ENTRIES)
def test_the_wrapper_caps_the_grid_of_the_grid_cases(entry):
    """at the device's 256 compute units: 256 blocks (lanes; matrix at H = 64) or 512 (matrix at H = 32) for 516 tiles"""
    want = {("lanes", 32): 256, ("lanes", 64): 256, ("matrix", 32): 512, ("matrix", 64): 256}
    for case in pc.GRID_CASES:
        grid, tiles = _recorded_grid(case, entry, DEVICE_COMPUTE_UNITS)
        per_cu = pguk.MATRIX_BLOCKS_PER_CU[case.H] if entry == "matrix" else 1
        assert grid == want[entry, case.H] == per_cu * DEVICE_COMPUTE_UNITS < tiles == 516
        assert _trips(tiles, grid) == (2 if grid == 512 else 3) and tiles - grid in (4, 260)   # some blocks one trip more


@pytest.mark.parametrize("entry", pguk.GRADIENTS_ENTRIES)
def test_one_compute_unit_gives_the_depth_cases_the_workloads_trips(entry):
    """compute_units = 1: one block on 160 trips, or two on 80 each -- at or above the trips of 5 000 000 rows on the device"""
    workload_tiles = -(-WORKLOAD_ROWS // pc.TILE)
    assert workload_tiles == 39063
    for case in pc.DEPTH_CASES:
        grid, tiles = _recorded_grid(case, entry, 1)
        per_cu = pguk.MATRIX_BLOCKS_PER_CU[case.H] if entry == "matrix" else 1
        assert grid == per_cu == (2 if (entry, case.H) == ("matrix", 32) else 1) and tiles == 160
        trips, workload = _trips(tiles, grid), _trips(workload_tiles, per_cu * DEVICE_COMPUTE_UNITS)
        assert (trips, workload) == ((80, 77) if grid == 2 else (160, 153)) and trips >= workload
        assert tiles % grid == 0      # every block of the launch makes that many


# ---------------------------------------------------------------------------------------------- out-of-range actions
@pytest.fixture(scope="module")
def out_of_range():
    """case name -> (inputs with out-of-range actions, the same with the actions clipped, the replaced rows)"""
    out = {}
    for case in pc.OUT_OF_RANGE_CASES:
        bad = pc.out_of_range_actions(case, pc.inputs(case))
        out[case.name] = (bad, pc.clipped_actions(case, bad), pc.out_of_range_rows(case))
    return out


@pytest.mark.parametrize("case", pc.OUT_OF_RANGE_CASES, ids=lambda c: c.name)
def test_out_of_range_inputs_hold_what_they_promise(case, out_of_range):
    bad, clipped, where = out_of_range[case.name]
    inp = pc.inputs(case)
    rows, A = case.E * case.T, case.A
    taken = bad["actions"].reshape(-1)
    assert bad["actions"].dtype == np.int32 and bad["actions"].shape == inp["actions"].shape
    assert where.size == max(4, rows // 10) == np.unique(where).size and 0 <= where.min() and where.max() < rows
    assert set(taken[where].tolist()) == {-1, A, 2 ** 31 - 1, -2 ** 31}
    outside = (taken < 0) | (taken >= A)
    assert np.array_equal(np.flatnonzero(outside), where)
    assert np.array_equal(taken[~outside], inp["actions"].reshape(-1)[~outside])
    assert all(np.array_equal(pc.bits(bad[k]), pc.bits(inp[k])) for k in ("obs", "rewards", "theta")) and np.array_equal(bad["done"], inp["done"])
    assert not np.shares_memory(bad["actions"], inp["actions"])
    assert pc.out_of_range_actions(case, inp)["actions"].tobytes() == bad["actions"].tobytes()      # seeded
    c = clipped["actions"].reshape(-1)
    assert c.min() >= 0 and c.max() <= A - 1 and np.array_equal(c[~outside], taken[~outside])
    assert set(c[where].tolist()) == {0, A - 1}


@pytest.mark.parametrize("case", pc.OUT_OF_RANGE_CASES, ids=lambda c: c.name)
def test_the_yardstick_defines_an_out_of_range_row(case, out_of_range):
    """finite; the policy head's bias gradient is sum_r (adv p + ent p (logp + entropy)) / R minus the one-hot of the rows IN
    range only -- an out-of-range row contributes adv * p + the entropy term, with no -1 anywhere; sum logp * adv takes the
    clamped action.  With EVERY action out of range no one-hot is left at all."""
    bad, clipped, where = out_of_range[case.name]
    rows, A = case.E * case.T, case.A
    want = pc.yardstick(case, bad)
    assert all(np.isfinite(np.asarray(want[k])).all() for k in want)
    p, adv = want["probabilities"], want["advantages"].reshape(-1)
    lp = np.log(p)
    entropy = -(p * lp).sum(axis=1)
    per_row = adv[:, None] * p + case.ent * p * (lp + entropy[:, None])          # no one-hot
    taken = bad["actions"].reshape(-1)
    inside = np.setdiff1d(np.arange(rows), where)
    onehot = np.zeros((rows, A))
    onehot[inside, taken[inside]] = 1.0
    expected = (per_row - adv[:, None] * onehot).sum(0) / rows
    assert np.abs(want["bp"] - expected).max() <= 1e-13 * max(1.0, np.abs(expected).max())
    clamped = np.clip(taken.astype(np.int64), 0, A - 1)
    s = float(np.sum(lp[np.arange(rows), clamped] * adv))
    assert abs(want["sum logp*adv"] - s) <= 1e-12 * max(1.0, abs(s))
    # every row out of range: the bias gradient is the sum without any one-hot
    every = {k: v.copy() for k, v in bad.items()}
    every["actions"][:] = np.array([-1, A, 2 ** 31 - 1, -2 ** 31], np.int64).astype(np.int32)[np.arange(rows) % 4].reshape(every["actions"].shape)
    w = pc.yardstick(case, every)
    assert np.abs(w["bp"] - per_row.sum(0) / rows).max() <= 1e-13 * max(1.0, np.abs(per_row).sum(0).max() / rows)
    # the share of the out-of-range rows: what the clipped actions' one-hot would take away
    share = np.zeros(A)
    np.add.at(share, clamped[where], adv[where] / rows)
    w_clipped = pc.yardstick(case, clipped)
    assert np.abs((want["bp"] - w_clipped["bp"]) - share).max() <= 1e-13 * max(1.0, np.abs(share).max())
    assert np.abs(share).max() > 1e-3


@pytest.mark.parametrize("case", pc.OUT_OF_RANGE_CASES, ids=lambda c: c.name)
def test_the_framework_sees_clipped_actions_only(case, out_of_range):
    """float64 autograd on the CLIPPED actions (torch is never handed an out-of-range one) agrees with the yardstick on the
    out-of-range ones in everything that does not depend on the one-hot; the error of float32 autograd on the clipped
    actions, the err_f32 of the GPU test (`pc.float32_error_of`), leaves the rounded yardstick inside the bound; and the
    test has teeth: the yardstick of the clipped actions breaks the bound on bp (and on Wp, through the same deltas),
    which it would not with the framework's result itself as the float32 yardstick"""
    bad, clipped, _ = out_of_range[case.name]
    want, auto64, auto32 = pc.yardstick(case, bad), pc.framework(case, clipped, torch.float64), pc.framework(case, clipped, torch.float32)
    for key in ("values", "returns", "advantages", "Wv", "bv") + pc.SUM_NAMES:
        x, y = np.asarray(want[key], f64), np.asarray(auto64[key], f64)
        assert x.size == y.size and float(np.abs(x.reshape(-1) - y.reshape(-1)).max()) <= 1e-11 * max(float(np.abs(y).max()), 1.0), key
    as_clipped = pc.yardstick(case, clipped)
    yard = pc.float32_error_of(want, as_clipped, auto32, RESULT_KEYS)
    rounded = {k: np.asarray(want[k], f64).astype(f32).astype(f64) for k in RESULT_KEYS}
    assert not _violations(rounded, want, yard, RESULT_KEYS), case.name
    assert set(_violations(as_clipped, want, yard, RESULT_KEYS)) >= {"Wp", "bp"}
    assert not set(_violations(as_clipped, want, auto32, RESULT_KEYS)) & {"Wp", "bp"}
