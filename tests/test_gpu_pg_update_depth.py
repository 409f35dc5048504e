"""Both gradient entries of the A2C / PPO update ("lanes": HipPgGradients, "matrix": HipPgGradientsMx) on the device where
`pc.CASES` does not reach (cases: tests/pg_update_cases.py; host side: tests/test_pg_update_depth_host.py):

  * the matrix entry's wavefront edges (`WAVE_CASES`: a last tile of 32, 33, 96 and 97 rows), lanes as the control;
  * the grid the wrapper picks for THIS device (`GRID_CASES`: 516 tiles on 256 or 512 blocks, HipPgReduce over as many
    partials), with the values and returns launches at the same 65 984 rows;
  * the accumulation depth of the recommended workload (`DEPTH_CASES` at compute_units = 1: one block on 160 trips, or two
    on 80 each; 5 000 000 rows on 256 compute units are 153 and 77 trips);
  * out-of-range actions (-1, A, 2^31 - 1, -2^31 on a tenth of the rows): no one-hot term, logp of the clamped action.

Everything a launch is judged by is tests/test_gpu_pg_update.py's `gradients_after_reduce`: sentinel-filled outputs with
surplus rows, NaN-fenced inputs, launch counts, inputs unchanged, a second run byte-identical, and eight tensors, four
sums and the sums of squares under err <= max(4 * err_f32, 2e-6 * scale) against float64.  Per launch the worst tensor is
printed with its err, 4 * err_f32 and the 2e-6 * scale floor (pytest -s)."""
import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests.test_gpu_pg_update import DEV, fm, gradients_after_reduce, values_and_returns  # noqa: F401  (`fm` is a fixture)
from warp_drive_amd.training import pg_update_kernels as pguk

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
ENTRIES = pguk.GRADIENTS_ENTRIES


@pytest.fixture(scope="module")
def inputs():
    """case name -> its inputs, made once on first use and never changed"""
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = pc.inputs(case)
        return cache[case.name]

    return get


def _blocks_per_cu(case, entry):
    return pguk.MATRIX_BLOCKS_PER_CU[case.H] if entry == "matrix" else 1


def _margins(tag, run):
    """one line per stage: the tensor with the largest err / err_f32, and the one nearest to its bound"""
    ss_got, ss_want, ss_yard = run["ss"]
    stages = (("tensors", run["got"], run["want"], run["yard"], pc.TENSOR_NAMES),
              ("sums", run["got"], run["want"], run["yard"], pc.SUM_NAMES),
              ("sums of squares", ss_got, ss_want, ss_yard, pc.TENSOR_NAMES))
    for stage, got, want, yard, keys in stages:
        rows = []
        for key in keys:
            _, err, err_f32, scale, ratio = pc.compare(np.asarray(got[key], f64).reshape(-1), np.asarray(want[key], f64).reshape(-1),
                                                       np.asarray(yard[key], f64).reshape(-1))
            bound = max(4.0 * err_f32, 2e-6 * scale)
            rows.append((ratio, err / bound if bound else 0.0, key, err, err_f32, scale))
        fmt = lambda r: f"{r[2]} ratio {r[0]:.2f} err {r[3]:.3e} 4*err_f32 {4 * r[4]:.3e} floor {2e-6 * r[5]:.3e} err/bound {r[1]:.3f}"  # noqa: E731
        print(f"margin {tag} | {stage} | worst ratio: {fmt(max(rows))} | nearest the bound: {fmt(max(rows, key=lambda r: r[1]))}")


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", pc.WAVE_CASES, ids=lambda c: c.name)
def test_wavefront_edges(fm, inputs, case, entry):
    """a last tile that fills a wavefront of the matrix entry exactly, spills one row into the next, leaves the last
    wavefront exactly dead, or puts one row into it; one block per tile"""
    run = gradients_after_reduce(fm, case, inputs(case), entry)
    assert run["grid"] == run["k"].tiles == pc.case_tiles(case) and run["k"].gradients_entry == entry
    _margins(f"wave {entry} {case.name}", run)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", pc.GRID_CASES, ids=lambda c: c.name)
def test_the_wrappers_grid_on_this_device(fm, inputs, case, entry):
    """the kernels built with the device's own compute-unit count: the cap `blocks per compute unit * compute units` binds
    (516 tiles), so blocks make 2 or 3 trips, some one fewer, and HipPgReduce sums exactly that many partials"""
    compute_units = torch.cuda.get_device_properties(DEV).multi_processor_count
    k = pguk.PgUpdateKernels(fm, case.E, case.T, case.H, case.O, case.A, DEV, gradients_entry=entry)
    assert k.compute_units == compute_units
    assert k.gradients_grid == _blocks_per_cu(case, entry) * compute_units < k.tiles == 516
    run = gradients_after_reduce(fm, case, inputs(case), entry, compute_units=compute_units)
    assert run["k"].gradients_grid == k.gradients_grid == run["grid"] == run["partials"].shape[0]
    print(f"grid {entry} {case.name}: {run['grid']} blocks for {k.tiles} tiles, at most {-(-k.tiles // run['grid'])} trips")
    _margins(f"grid {entry} {case.name}", run)


@pytest.mark.parametrize("case", pc.GRID_CASES, ids=lambda c: c.name)
def test_values_and_returns_at_the_grid_cases(fm, inputs, case):
    """tests/test_gpu_pg_update.py::test_values_and_returns' body at 65 984 rows and T = 64: values under the bound and
    bit-identical across the three geometries, returns and advantages bit for bit"""
    inp = inputs(case)
    values_and_returns(fm, case, inp, pc.yardstick(case, inp))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", pc.DEPTH_CASES, ids=lambda c: c.name)
def test_the_workloads_accumulation_depth(fm, inputs, case, entry):
    """compute_units = 1: ONE block adds up all 160 tiles (two blocks 80 each for the matrix entry at H = 32), which is at
    or above the 153 (77) trips a block makes at 5 000 000 rows on 256 compute units.

    Measured on the MI355X (docs/rounds/r48.md): with a tile's 128 rows added one by one onto the launch's accumulator
    (20 480 serial additions) "lanes" was outside the bound on b0, b1, Wp, bp, Wv and three of the sums, err / err_f32 up
    to 99 on bp and 1097 on sum entropy; with a trip summed from +0 and added once, its worst is 26.2 on bp at 0.27 of the
    bound, as for "matrix"."""
    k = pguk.PgUpdateKernels(fm, case.E, case.T, case.H, case.O, case.A, DEV, compute_units=1, gradients_entry=entry)
    expected = 2 if (entry, case.H) == ("matrix", 32) else 1
    assert k.gradients_grid == expected == _blocks_per_cu(case, entry) and k.tiles == 160      # before anything is launched
    run = gradients_after_reduce(fm, case, inputs(case), entry, compute_units=1)
    assert run["grid"] == expected == run["partials"].shape[0]
    print(f"depth {entry} {case.name}: {run['grid']} blocks for {k.tiles} tiles, {k.tiles // run['grid']} trips each")
    _margins(f"depth {entry} {case.name}", run)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("case", pc.OUT_OF_RANGE_CASES, ids=lambda c: c.name)
def test_out_of_range_actions(fm, inputs, case, entry):
    """A tenth of the rows holds -1, A, 2^31 - 1 or -2^31 (both kernels only COMPARE with the action, never index by it).
    `want` is the yardstick on these actions.  err_f32 comes from the framework on the same inputs with the actions CLIPPED,
    against the yardstick on the clipped actions: a float32 computation of the same size and magnitude; torch never sees an
    out-of-range action.  Teeth, where the entropy coefficient is 0 (A = 8): judged against the yardstick of the CLIPPED
    actions the entry's bp breaks the bound, and is off by the out-of-range rows' share of the one-hot."""
    inp = inputs(case)
    bad = pc.out_of_range_actions(case, inp)
    run = gradients_after_reduce(fm, case, inp, entry, actions=bad["actions"])
    _margins(f"out of range {entry} {case.name}", run)
    if case.ent == 0.0:
        where, rows = pc.out_of_range_rows(case), case.E * case.T
        clipped = pc.yardstick(case, pc.clipped_actions(case, bad), values=run["values"])
        ok, err, err_f32, scale, _ = pc.compare(run["got"]["bp"], clipped["bp"], run["yard"]["bp"] - run["want"]["bp"] + clipped["bp"])
        assert not ok and err > 1e3 * max(4 * err_f32, 2e-6 * scale), (err, err_f32, scale)
        share = np.zeros(case.A)
        np.add.at(share, np.clip(bad["actions"].reshape(-1)[where].astype(np.int64), 0, case.A - 1),
                  run["want"]["advantages"].reshape(-1)[where] / rows)
        assert set(np.flatnonzero(share)) == {0, case.A - 1}
        off = np.asarray(run["got"]["bp"], f64) - clipped["bp"]
        assert np.abs(off - share).max() <= max(4 * err_f32, 2e-6 * scale) + 1e-12 < 1e-3 * np.abs(share).max(), (off, share)
