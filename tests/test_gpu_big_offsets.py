"""The update kernels and HipRolloutRecord on batch tensors past 2^30 (byte offset 2^32), 2^31 and 2^32 ELEMENTS: the sizes
of the trainer leg (one PPO iteration of 250 ticks x 2000 replicas x 100 agents is 5e7 rows), where an offset formed in
32 bits wraps INSIDE the allocation -- no fault, the rows behind the boundary computed from, or written over, rows in
front of it.  tests/big_offset_cases.py holds the scheme (zeros everywhere, seeded bands around the boundary rows, at row
0 and at the ragged end; outputs full of a sentinel), the cases and the checks; tests/test_big_offset_cases_host.py shows
on the host that those checks catch each kind of wrap on each tensor.  Here: the launches, through the `UpdateKernels`
wrappers (whose uninitialised allocations are made to come full of the sentinel) or directly where a case says so.

Nothing large reaches the host: band rows are copied, everything else is judged by chunked reductions on the device.  Every
test checks the free memory first (a skip names the GB it needs), frees its tensors and asserts the allocator gave them
back; it prints the worst err / err_f32 per result tensor, the memory it reserved and its time (pytest -s)."""
import contextlib
import gc
import time

import numpy as np
import pytest
import torch

from tests import big_offset_cases as bo
from tests import update_kernel_cases as uk

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NULL = np.uint64(0)
CHUNK = 1 << 27   # elements per reduction step: the comparisons' temporaries stay at 128 MB


@pytest.fixture(scope="module")
def fm():
    from tests.hip_harness import require_gpu
    from warp_drive_amd.managers.function_manager import HIPFunctionManager

    require_gpu()
    m = HIPFunctionManager(num_agents=1, num_envs=1)
    m.load_hip_from_binary_file()
    return m


# ====================================================================================================== device helpers
def _input(layout, data, dtype=torch.float32):
    """[R, width] zeros (a device memset) with the band rows of `data` [nb, width] copied in"""
    data = np.ascontiguousarray(data)
    t = torch.zeros((layout.R, data.shape[1]), dtype=dtype, device=DEV)
    for (a, b), k in zip(layout.bands, layout.starts):
        t[a:b].copy_(torch.from_numpy(data[k:k + b - a]))
    return t


def _fill_sentinel(t):
    t.view(torch.int32).fill_(uk.SENTINEL_BITS)
    return t


def _output(rows, width, dtype=torch.float32):
    return _fill_sentinel(torch.empty((rows, width), dtype=dtype, device=DEV))


class DeviceStore:
    """what a check of big_offset_cases.py reads results through: {name: [R, width] device tensor of 4-byte elements}"""

    def __init__(self, tensors):
        self.t = {k: v.view(torch.int32) for k, v in tensors.items()}
        self.dtype = {k: v.dtype for k, v in tensors.items()}

    def rows(self, name, r0, r1):
        return self.t[name][r0:r1].view(self.dtype[name]).cpu().numpy()

    def sentinels(self, name):
        flat, total = self.t[name].reshape(-1), torch.zeros((), dtype=torch.int64, device=DEV)
        for a in range(0, flat.numel(), CHUNK):
            total += (flat[a:a + CHUNK] == uk.SENTINEL_BITS).sum()
        return int(total)

    def mismatch_outside(self, name, bands, pattern=None):
        t = self.t[name]
        R, w = t.shape
        want = None if pattern is None else torch.from_numpy(uk.bits(np.asarray(pattern)).view(np.int32).reshape(1, w)).to(DEV)
        total, step = torch.zeros((), dtype=torch.int64, device=DEV), max(1, CHUNK // w)
        edges = [0] + [x for band in bands for x in band] + [R]
        for g0, g1 in zip(edges[0::2], edges[1::2]):
            for a in range(g0, g1, step):
                rows = t[a:min(g1, a + step)]
                total += torch.count_nonzero(rows) if want is None else (rows != want).sum()
        return int(total)


class _SentinelTorch:
    """stands in for the `torch` module inside training/update_kernels.py while a wrapper runs: what the wrapper allocates
    uninitialised comes full of the sentinel, and is kept (`made`) so that a test can read per-block partials"""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *args, **kw):
        self.made.append(_fill_sentinel(torch.empty(*args, **kw)))
        return self.made[-1]

    def empty_like(self, *args, **kw):
        self.made.append(_fill_sentinel(torch.empty_like(*args, **kw)))
        return self.made[-1]


@contextlib.contextmanager
def _sentinel_allocations():
    from warp_drive_amd.training import update_kernels as module

    shim = _SentinelTorch()
    module.torch = shim
    try:
        yield shim
    finally:
        module.torch = torch


@contextlib.contextmanager
def _counted(name):
    from warp_drive_amd.managers import hip_driver as drv

    before = drv.LAUNCH_COUNTS[name]
    yield
    assert drv.LAUNCH_COUNTS[name] == before + 1, name


def _unchanged(v, store, layout, name, data):
    """an input after the launch: its band rows as seeded, zero bits everywhere else"""
    v.exact(name + " (input)", np.concatenate([store.rows(name, a, b) for a, b in layout.bands]), data)
    v.require(store.mismatch_outside(name, layout.bands) == 0, name, "an input's zero rows changed")


def _guarded(case, body):
    """run `body` (which returns a closed Verdict: strings and floats only) if the case fits the free memory; whatever
    happens, its tensors are freed and the allocator is back where it was before the test goes on"""
    need = case.bytes() + 3 * 2 ** 30       # (+ the reductions' temporaries and the band copies)
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.0f} GB of free device memory, {free / 2 ** 30:.1f} GB free")
    assert case.bytes() < bo.CAP_BYTES
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    reserved, t0 = torch.cuda.memory_reserved(), time.perf_counter()
    report, failure = None, None
    try:
        v = body()
        report = v.report()
        v.close()
    except Exception as err:  # noqa: BLE001 -- only its text is kept: its traceback would hold the frames and their tensors
        failure = f"{type(err).__name__}: {err}"
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    peak = torch.cuda.max_memory_reserved() - reserved
    print(f"{report or case.name} | reserved {peak / 1e9:.1f} GB, {time.perf_counter() - t0:.1f} s")
    assert torch.cuda.memory_reserved() <= reserved + 2 ** 28, (torch.cuda.memory_reserved(), reserved)
    assert failure is None, failure


def _kernels(fm):
    from warp_drive_amd.training.update_kernels import UpdateKernels

    return UpdateKernels(fm)


# ================================================================================================ B. the objective
def test_policy_gradient_head_past_every_boundary(fm):
    """`UpdateKernels.policy_gradient_head` on out / grad [99 887 063, 43] (2 x 17.2 GB), heads [21, 21], entropy and value
    coefficients non-zero: the gradient of every band block against float64, every other row bit-equal to row 1's (a zero
    row's); the four sums of every band block against float64, of every other block bit-equal to a zero block's"""
    case = bo.PolicyGradientHeadCase(bo.REAL)

    def body():
        k, x, lay = _kernels(fm), case.inputs(), case.layout
        out, actions = _input(lay, x["out"]), _input(lay, x["actions"], torch.int32)
        adv, ret = _input(lay, x["adv"]).reshape(-1), _input(lay, x["ret"]).reshape(-1)
        with _sentinel_allocations() as shim, _counted("HipPolicyGradientHead"):
            grad, total = k.policy_gradient_head(out, actions, adv, ret, case.heads, uk.PG_ENT_COEFF, uk.PG_VF_COEFF)
        torch.cuda.synchronize()
        sums = next(t for t in shim.made if tuple(t.shape) == (case.blocks, 4))
        store = DeviceStore({"grad": grad, "out": out})
        v = case.check(store, sums.cpu().numpy())
        v.require(np.allclose(total.cpu().numpy(), sums.double().sum(0).cpu().numpy(), rtol=1e-12, atol=0), "the wrapper's totals")
        _unchanged(v, store, lay, "out", x["out"])
        return v

    _guarded(case, body)


# ================================================================================================ A. returns
def test_discounted_returns_past_every_boundary(fm):
    """`UpdateKernels.discounted_returns` at T = 5, E = 200 001, n = 100, W = 43, gamma = 0.99: the value column of `out`
    [5, 200 001, 100, 43] (17.2 GB) is read past 2^30, 2^31 and 2^32 at t = 1, 2 and 4; returns and advantages of the band
    chains (done flags at t = 0, mid-batch, T - 1, and of value 2) bit for bit, +0.0 everywhere else"""
    case = bo.DiscountedReturnsCase(bo.REAL)

    def body():
        k, x, lay = _kernels(fm), case.inputs(), case.layout
        shape = (case.T, case.E, case.n)
        out, rewards = _input(lay, x["out"]), _input(lay, x["rewards"])
        done = torch.from_numpy(x["done"]).to(DEV)
        with _sentinel_allocations(), _counted("HipDiscountedReturns"):
            ret, adv = k.discounted_returns(rewards.view(shape), done, out.view(shape + (case.W,)), case.gamma)
        torch.cuda.synchronize()
        store = DeviceStore({"returns": ret.view(-1, 1), "advantages": adv.view(-1, 1), "out": out})
        v = case.check(store)
        _unchanged(v, store, lay, "out", x["out"])
        return v

    _guarded(case, body)


# ================================================================================================ A. column sums
@pytest.mark.parametrize("C", (256, 64))
def test_relu_backward_column_sums_past_every_boundary(fm, C):
    """`UpdateKernels.relu_backward_colsum` on three tensors of 17.2 GB: [2^24 + 4103, 256] and, at the same byte size,
    [2^26 + 4103, 64] -- g bit for bit in the bands and +0.0 elsewhere, the column sums against float64 over the band rows"""
    case = bo.ColumnSumsCase(bo.REAL, C)

    def body():
        k, x, lay = _kernels(fm), case.inputs(), case.layout
        gx, y = _input(lay, x["gx"]), _input(lay, x["y"])
        with _sentinel_allocations(), _counted("HipReluBackwardColumnSums"):
            g, sums = k.relu_backward_colsum(gx, y)
        torch.cuda.synchronize()
        store = DeviceStore({"g": g, "gx": gx, "y": y})
        v = case.check(store, {"column sums": sums.cpu().numpy()})
        _unchanged(v, store, lay, "gx", x["gx"])
        _unchanged(v, store, lay, "y", x["y"])
        return v

    _guarded(case, body)


# ================================================================================================ B. hidden layer's input gradient
def test_linear_mask_backward_past_every_boundary(fm):
    """`UpdateKernels.linear_mask_backward` (HipLinearMaskBackwardBx3_256) on g_in, h, g_out [2^24 + 4103, 256]"""
    case = bo.MaskBackwardCase(bo.REAL)

    def body():
        k, x, lay = _kernels(fm), case.inputs(), case.layout
        g_in, h, w = _input(lay, x["g_in"]), _input(lay, x["h"]), torch.from_numpy(x["w"]).to(DEV)
        with _sentinel_allocations(), _counted(case.name):
            g_out = k.linear_mask_backward(g_in, w, h)
        torch.cuda.synchronize()
        store = DeviceStore({"g_out": g_out, "g_in": g_in, "h": h})
        v = case.check(store)
        _unchanged(v, store, lay, "g_in", x["g_in"])
        _unchanged(v, store, lay, "h", x["h"])
        return v

    _guarded(case, body)


# ================================================================================================ B. weight gradients
@pytest.mark.parametrize("ci", (256, 71))
def test_weight_grad_past_every_boundary(fm, ci):
    """`UpdateKernels.weight_grad` at R = 2^24 + 4103 (a host-side tail of 7 rows behind every boundary): ci = 256, g and x
    past all three; ci = 71 with the bias column (HipWeightGradBx3_256x96), g past all three and x [R, 71] past b30 =
    row 15 123 124 only -- b31 and b32 of x are out of reach under the 64 GB cap (x would need 3.0e7 / 6.0e7 rows, g
    then 31 / 62 GB)"""
    case = bo.WeightGradCase(bo.REAL, ci)

    def body():
        k, x, lay = _kernels(fm), case.inputs(), case.layout
        g, xs = _input(lay, x["g"]), _input(lay, x["x"])
        with _sentinel_allocations(), _counted(case.name):
            gw, gb = k.weight_grad(g, xs, with_bias=case.with_bias)
        torch.cuda.synchronize()
        results = {"weights": gw.cpu().numpy()}
        if case.with_bias:
            results["bias"] = gb.cpu().numpy()
        store = DeviceStore({"g": g, "x": xs})
        v = case.check(store, results)
        _unchanged(v, store, lay, "g", x["g"])
        _unchanged(v, store, lay, "x", x["x"])
        return v

    _guarded(case, body)


# ================================================================================================ B. output layer's backward
def test_head_backward_matrix_cores_past_every_boundary(fm):
    """`UpdateKernels.head_backward` (HipHeadBackwardBx3_W43) at R = 24 974 843: h2 / g2 [R, 256] (2 x 25.6 GB) past all
    three; g3 [R, 43] (4.3 GB) past b30 = row 24 970 740 only -- its b31 is out of reach under the cap (R = 5.0e7 makes h2
    and g2 51 GB each)"""
    case = bo.HeadBackwardCase(bo.REAL, 256)

    def body():
        k, x, lay = _kernels(fm), case.inputs(), case.layout
        g3, h2, w3 = _input(lay, x["g3"]), _input(lay, x["h2"]), torch.from_numpy(x["w3"]).to(DEV)
        with _sentinel_allocations(), _counted(case.name):
            g2, db2, dw3, db3 = k.head_backward(g3, w3, h2)
        torch.cuda.synchronize()
        store = DeviceStore({"g2": g2, "g3": g3, "h2": h2})
        v = case.check(store, {"db2": db2.cpu().numpy(), "dw3": dw3.cpu().numpy(), "db3": db3.cpu().numpy()})
        _unchanged(v, store, lay, "g3", x["g3"])
        _unchanged(v, store, lay, "h2", x["h2"])
        return v

    _guarded(case, body)


def test_head_backward_vector_units_past_every_boundary(fm):
    """HipHeadBackward_W43 launched directly at 64 threads (the wrapper routes C = 256 to the matrix-core kernel), 4096 rows
    per block, R = 67 112 967: h2 / g2 [R, 64] (2 x 17.2 GB) past all three, g3 [R, 43] (11.5 GB) past b30 and b31 -- its
    b32 is out of reach under the cap.  g2, and db2_part / dw3_part of every block that holds a band, against float64;
    the partials of every other block +0.0"""
    case = bo.HeadBackwardCase(bo.REAL, 64)

    def body():
        fm.initialize_functions(["HipHeadBackward_W43"])
        fn = fm.get_function("HipHeadBackward_W43")
        x, lay, R, grid = case.inputs(), case.layout, case.R, case.grid
        g3, h2, w3 = _input(lay, x["g3"]), _input(lay, x["h2"]), torch.from_numpy(x["w3"]).to(DEV)
        g2, db2, dw3 = _output(R, 64), _output(grid, 64), _fill_sentinel(torch.empty((grid, 43, 64), device=DEV))
        assert grid * case.rows_per_block >= R and g3.shape == (R, 43) and h2.shape == g2.shape == (R, 64)
        with _counted("HipHeadBackward_W43"):
            fn(g3, w3, h2, g2, db2, dw3, np.int64(R), np.int32(case.rows_per_block), block=(64, 1, 1), grid=(grid, 1), shared=0)
        torch.cuda.synchronize()
        store = DeviceStore({"g2": g2, "g3": g3, "h2": h2})
        v = case.check(store, {"db2_part": db2.cpu().numpy(), "dw3_part": dw3.cpu().numpy()})
        _unchanged(v, store, lay, "g3", x["g3"])
        _unchanged(v, store, lay, "h2", x["h2"])
        return v

    _guarded(case, body)


# ================================================================================================ A. HipRolloutRecord
@pytest.mark.parametrize("variant", ("a", "b"))
def test_rollout_record_past_every_boundary(fm, variant):
    """HipRolloutRecord launched directly, E = 2000, `batch_row` preset: (a) N = 100 agents of one policy, launches at t = 0
    and t - 1, t, t + 1 around t = 5368, 10737, 21474, where the reward batch [21 477, 2000, 100] (17.2 GB) passes 2^30,
    2^31, 2^32; (b) N = 1, around t = 536 870 and 1 073 741, where the done batch and the reward batch [1 073 744, 2000]
    (8.6 GB each) pass 2^30 and 2^31.  The written rows, the running sums and the counters bit for bit; every other
    row of both batches still the sentinel"""
    case = bo.RecordCase(bo.REAL, variant)

    def body():
        fm.initialize_functions(["HipRolloutRecord"])
        fn = fm.get_function("HipRolloutRecord")
        E, N = case.E, case.N
        rewards, done = case.inputs()
        slot, na, _ = case.case.slot()
        d_rewards, d_done, d_slot = (torch.from_numpy(a).to(DEV) for a in (rewards, done, slot))
        state = {k: torch.from_numpy(a).to(DEV) for k, a in case.initial_state().items()}
        batch_row = torch.zeros(E, dtype=torch.int64, device=DEV)
        reward_batch, done_batch = _output(case.R, E * N), _output(case.R, E, torch.int32)
        assert max(case.ts) < case.R and na == N
        launch = 0
        for first, launches in case.groups:
            batch_row.fill_(first)           # (the kernel advances it by one per launch)
            for j in range(launches):
                assert case.ts[launch] == first + j
                with _counted("HipRolloutRecord"):
                    fn(d_rewards[launch], d_done[launch], np.int32(N), np.int32(E), d_slot, batch_row, done_batch,
                       state["ep_count"], reward_batch, state["ep_reward_a"], state["ep_sum_a"], np.int32(N), NULL, NULL, NULL,
                       np.int32(0), block=(min(1024, (N + 63) // 64 * 64), 1, 1), grid=(E, 1), shared=4 * N)
                launch += 1
        torch.cuda.synchronize()
        v = case.check(DeviceStore({"reward_batch": reward_batch, "done_batch": done_batch}),
                       {name: t.cpu().numpy() for name, t in state.items()})
        v.require(bool((batch_row == case.ts[-1] + 1).all()), "batch_row", "not advanced by one per launch")
        return v

    _guarded(case, body)
