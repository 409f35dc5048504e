"""Every entry of the update object (wd_kernels_update.hsaco) and HipRolloutRecord, launched DIRECTLY at geometries their
wrappers cannot produce (tests/update_kernel_cases.py holds the cases, the numpy models and the reasoning behind the inputs).

`UpdateKernels` always launches 256 threads with 4096 rows per block or one slab per CU, v_col = W - 1 and fresh outputs;
`FusedRolloutTick` one shape per trainer.  Here: slabs shorter than the persistent kernels' pipelines, blocks with nothing to
do, grids with surplus blocks, tiles shorter than a staging tile, in-place outputs, other columns and block sizes, one policy /
interleaved policies / more agents than threads.

Conventions of every case:
  * an output is allocated with surplus rows (or surplus blocks of partials) filled with a sentinel NaN and the surplus is
    compared byte for byte afterwards; the rows a kernel must write start as the sentinel too, so `isfinite` shows a gap;
  * a float input a kernel may read up to its last element is a view that ENDS inside a larger allocation whose following
    floats are NaN: the kernels clamp their staged loads into the arrays, and a wrong clamp then poisons a result
    (everything stays inside allocated memory);
  * section A (fixed float32 operation order) is compared bit for bit with the numpy model; section B against float64
    with the framework's float32 operation on the same inputs as yardstick: err <= max(4 * err_f32, 2e-6 * scale) per launch
    and result tensor, per-block partials against the float64 result of that block's rows, masks exact;
  * the worst err / err_f32 of every case is printed (pytest -s)."""
import numpy as np
import pytest
import torch

from tests import update_kernel_cases as uk

pytestmark = pytest.mark.gpu
f32 = np.float32
NULL = np.uint64(0)


@pytest.fixture(scope="module")
def fm():
    from tests.hip_harness import require_gpu
    from warp_drive_amd.managers.function_manager import HIPFunctionManager

    require_gpu()
    m = HIPFunctionManager(num_agents=1, num_envs=1)
    m.load_hip_from_binary_file()
    return m


DEV = torch.device("cuda:0")


def _launcher(fm, name):
    """fn(*args, block=, grid=, shared=) that also asserts the launch was counted under `name`"""
    from warp_drive_amd.managers import hip_driver as drv

    fm.initialize_functions([name])
    fn = fm.get_function(name)

    def launch(*args, **kw):
        before = drv.LAUNCH_COUNTS[name]
        fn(*args, **kw)
        assert drv.LAUNCH_COUNTS[name] == before + 1, name

    return launch


def _fenced(a, offset=0, with_fence=False):
    """numpy float32 array -> a device view of its shape, `offset` floats into an allocation that goes on with NaN
    (with_fence: also the floats after the view)"""
    a = np.ascontiguousarray(a, f32)
    base = torch.full((offset + a.size + 72,), float("nan"), dtype=torch.float32, device=DEV)
    view = base[offset:offset + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return (view, base[offset + a.size:]) if with_fence else view


def _sentinel(rows, tail, surplus=3, dtype=torch.float32, offset=0):
    """(whole allocation, the [rows, *tail] view the kernel is given): everything holds the sentinel"""
    n = int(np.prod((rows,) + tuple(tail)))
    extra = int(np.prod((surplus,) + tuple(tail)))
    whole = torch.full((offset + n + extra,), uk.SENTINEL_BITS, dtype=torch.int32, device=DEV)
    return whole, whole[offset:offset + n].view(dtype).view((rows,) + tuple(tail))


def _untouched(whole, view, offset=0):
    """the allocation around `view` still holds the sentinel"""
    n = view.numel()
    return bool((whole[:offset] == uk.SENTINEL_BITS).all()) and bool((whole[offset + n:] == uk.SENTINEL_BITS).all())


def _same_bits(t, a):
    return np.array_equal(uk.bits(t.detach().cpu().numpy()), uk.bits(np.ascontiguousarray(a)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(name, case, results, want, yard):
    """every result tensor inside the bound; prints the worst err / err_f32 of the case"""
    ratios, failures = {}, []
    for k in want:
        got = results[k].detach().double().cpu().numpy()
        assert np.isfinite(got).all(), (name, case, k, "not finite")
        err, err_f32, scale = uk.judge(got, want[k], yard[k].detach().double().cpu().numpy())
        ratios[k] = err / err_f32 if err_f32 else (0.0 if err == 0.0 else float("inf"))
        if not uk.within_bound(err, err_f32, scale):
            failures.append((k, err, err_f32, scale))
    print(f"{name} {case}: err / err_f32 " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert not failures, (name, case, failures)


# ================================================================================================ A. HipRolloutRecord
@pytest.mark.parametrize("case", uk.RECORD_CASES, ids=lambda c: c.name)
def test_rollout_record_bit_for_bit(fm, case):
    """6 ticks, one launch per tick, into batch tensors of 9 rows starting at row 2: both reward batches, the done batch,
    both running and both episodic sums, the episode count and the row counters equal the numpy model bit for bit -- rows
    0, 1 and 8 and the three replicas past E included -- and the inputs are unchanged"""
    launch = _launcher(fm, "HipRolloutRecord")
    slot, na, nb = case.slot()
    rewards, done = case.inputs()
    want = uk.record_run_model(case)
    d_slot, d_rewards, d_done = _dev(slot), _dev(rewards), _dev(done)
    for block in case.blocks:
        state = {k: _dev(v) for k, v in case.initial_state().items()}
        b = [state["reward_batch_b"], state["ep_reward_b"], state["ep_sum_b"]] if nb else [NULL, NULL, NULL]
        for tick in range(uk.RECORD_TICKS):
            launch(d_rewards[tick], d_done[tick], np.int32(case.N), np.int32(case.E), d_slot, state["batch_row"],
                   state["done_batch"], state["ep_count"], state["reward_batch_a"], state["ep_reward_a"], state["ep_sum_a"],
                   np.int32(na), *b, np.int32(nb), block=(block, 1, 1), grid=(case.E, 1), shared=4 * case.N)
        torch.cuda.synchronize()
        for name in uk.RECORD_STATE_NAMES:
            assert _same_bits(state[name], want[name]), (case.name, block, name)
        assert _same_bits(d_rewards, rewards) and _same_bits(d_done, done) and _same_bits(d_slot, slot)


# ================================================================================================ A. HipDiscountedReturns
@pytest.mark.parametrize("case", uk.RETURNS_CASES, ids=lambda c: c.name)
def test_discounted_returns_bit_for_bit(fm, case):
    """returns and advantages equal the float32 recursion bit for bit with the value in column v_col of rows of width W, at
    64 / 128 / 256 threads, a block boundary inside a replica and surplus blocks; where v_col = W - 1 also equal to
    losses.discounted_returns on the device"""
    from warp_drive_amd.training.losses import discounted_returns

    launch = _launcher(fm, "HipDiscountedReturns")
    rewards, done, out = case.inputs()
    T, E, n = rewards.shape
    d_rewards, d_done, d_out = _fenced(rewards), _dev(done), _fenced(out)
    for gamma in uk.RETURNS_GAMMAS:
        (w_ret, ret), (w_adv, adv) = _sentinel(T, (E, n)), _sentinel(T, (E, n))
        launch(d_rewards, d_done, d_out, np.int32(case.W), np.int32(case.v_col), np.float32(gamma), np.int32(T), np.int32(E),
               np.int32(n), ret, adv, block=(case.block, 1, 1), grid=(case.grid, 1), shared=0)
        torch.cuda.synchronize()
        want_ret, want_adv = uk.returns_model(rewards, done, out, case.v_col, gamma)
        assert _same_bits(ret, want_ret) and _same_bits(adv, want_adv), (case.name, gamma)
        assert _untouched(w_ret, ret) and _untouched(w_adv, adv)
        if case.v_col == case.W - 1:
            fw = discounted_returns(d_rewards, d_done, d_out[..., -1], gamma)
            assert torch.equal(ret, fw) and torch.equal(adv, fw - d_out[..., -1])
    assert _same_bits(d_rewards, rewards) and _same_bits(d_out, out)


# ================================================================================================ A. HipReluBackwardColumnSums
@pytest.mark.parametrize("C", uk.COLSUM_WIDTHS)
def test_relu_backward_column_sums_bit_for_bit(fm, C):
    """g and the PER-BLOCK partial sums equal the numpy model (the kernel's order of float32 additions) bit for bit at five
    geometries -- one row, one row per block, ragged last blocks, blocks past R (partials exactly 0) -- and once in place
    (g == gx); the gradient under y = +0 / -0 / negative is +0.0"""
    launch = _launcher(fm, "HipReluBackwardColumnSums")
    for in_place, (R, rpb, grid) in [(False, g) for g in uk.COLSUM_GEOMETRIES] + [(True, uk.COLSUM_GEOMETRIES[3])]:
        gx, y = uk.colsum_inputs(R, C)
        want_g, want_partial = uk.colsum_model(gx, y, rpb, grid)
        (d_gx, fence), d_y = _fenced(gx, with_fence=True), _fenced(y)
        w_g, g = (None, d_gx) if in_place else _sentinel(R, (C,))
        w_p, partial = _sentinel(grid, (C,))
        launch(d_gx, d_y, g, partial, np.int64(R), np.int32(C), np.int32(rpb), block=(256, 1, 1), grid=(grid, 1), shared=0)
        torch.cuda.synchronize()
        where = (C, R, rpb, grid, in_place)
        assert _same_bits(g, want_g), where                          # (sign bits included: +0.0 wherever y <= 0)
        assert _same_bits(partial, want_partial), where
        assert _untouched(w_p, partial), where
        if in_place:
            assert bool(torch.isnan(fence).all()), where
        else:
            assert _untouched(w_g, g) and _same_bits(d_gx, gx), where
        assert _same_bits(d_y, y), where
        for b, (r0, r1) in enumerate(uk.slab_rows(R, rpb, grid)):
            if r0 == r1:
                assert bool((partial[b] == 0).all()), where


# ================================================================================================ B. output layer's backward
def _head_yardstick(g3, w3, h2, R, rpb, grid, db3_waves):
    """the framework's float32 operations on the device, per block of rows"""
    W, C = w3.shape
    g2 = torch.ops.aten.threshold_backward(g3 @ w3, h2, 0)
    res = {"g2": g2, "db2_part": torch.zeros(grid, C, device=DEV), "dw3_part": torch.zeros(grid, W, C, device=DEV)}
    if db3_waves:
        res["db3_part"] = torch.zeros(grid * 4, W, device=DEV)
    for b, (r0, r1) in enumerate(uk.slab_rows(R, rpb, grid)):
        if r0 == r1:
            continue
        res["db2_part"][b] = g2[r0:r1].sum(0)
        res["dw3_part"][b] = g3[r0:r1].t() @ h2[r0:r1]
        if db3_waves:
            local = torch.arange(r1 - r0, device=DEV)
            for wv in range(4):
                res["db3_part"][4 * b + wv] = g3[r0:r1][(local % 32) // 8 == wv].sum(0)
    return res


def _head_common_checks(where, results, wholes, h2, R, rpb, grid):
    g2 = results["g2"]
    assert bool((g2[torch.from_numpy(h2 <= 0).to(DEV)] == 0).all()), where          # the mask is exact
    for k, (whole, view) in wholes.items():
        assert _untouched(whole, view), (where, k)
    for b, (r0, r1) in enumerate(uk.slab_rows(R, rpb, grid)):
        if r0 == r1:   # a block with nothing to do leaves exact zeros
            assert all(bool((results[k][b] == 0).all()) for k in ("db2_part", "dw3_part")), where
            if "db3_part" in results:
                assert bool((results["db3_part"][4 * b:4 * b + 4] == 0).all()), where


@pytest.mark.parametrize("W,C,geometry", uk.HEAD_VECTOR_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_head_backward_vector_units_per_block(fm, W, C, geometry):
    """HipHeadBackward_W<W> at C threads: one row, tiles of 32 + 1 / 32 + 8 / 5 rows, blocks with nothing to do -- g2, and
    db2_part / dw3_part of EVERY block against float64 of that block's rows"""
    R, rpb, grid = geometry
    launch = _launcher(fm, f"HipHeadBackward_W{W}")
    g3, w3, h2 = uk.head_inputs(R, W, C)
    d_g3, d_w3, d_h2 = _fenced(g3), _fenced(w3), _fenced(h2)
    wholes = {"g2": _sentinel(R, (C,)), "db2_part": _sentinel(grid, (C,)), "dw3_part": _sentinel(grid, (W, C))}
    results = {k: v[1] for k, v in wholes.items()}
    launch(d_g3, d_w3, d_h2, results["g2"], results["db2_part"], results["dw3_part"], np.int64(R), np.int32(rpb),
           block=(C, 1, 1), grid=(grid, 1), shared=0)
    torch.cuda.synchronize()
    where = (W, C, geometry)
    _check(f"HipHeadBackward_W{W}", where, results, uk.head_reference(g3, w3, h2, rpb, grid),
           _head_yardstick(d_g3, d_w3, d_h2, R, rpb, grid, False))
    _head_common_checks(where, results, wholes, h2, R, rpb, grid)
    assert _same_bits(d_g3, g3) and _same_bits(d_h2, h2)


def _pack_w3(w3):
    """W3^T as HipHeadBackwardBx3's A operand, the layout `UpdateKernels._head_backward_bx3` spells out: register-image
    order [wave][tile][k step][term][lane = 32 kg + i][e], element = W3[k = 16 ks + 8 kg + e][unit = 64 wave + 32 tile + i],
    zero for k >= W"""
    from warp_drive_amd.training.policy_kernel import split_bf16x3

    W, C = w3.shape
    ks = (W + 15) // 16
    wt = torch.zeros((C, 16 * ks), dtype=torch.float32, device=DEV)
    wt[:, :W] = w3.t()
    return split_bf16x3(wt).reshape(3, 4, 2, 32, ks, 2, 8).permute(1, 2, 4, 0, 5, 3, 6).contiguous()


@pytest.mark.parametrize("W,geometry", uk.HEAD_BX3_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_head_backward_matrix_cores_per_block(fm, W, geometry):
    """HipHeadBackwardBx3_W<W>: slabs of 1, 2, 3 and 5 steps around its 3 stages, a last slab of one step, blocks with
    nothing to do -- g2, db2_part, dw3_part of every block and db3_part of every (block, wavefront) against float64"""
    R, rpb, grid = geometry
    launch = _launcher(fm, f"HipHeadBackwardBx3_W{W}")
    g3, w3, h2 = uk.head_inputs(R, W, 256, one_sign=True)
    d_g3, d_w3, d_h2 = _fenced(g3), _dev(w3), _fenced(h2)
    wholes = {"g2": _sentinel(R, (256,), surplus=33), "db2_part": _sentinel(grid, (256,)),
              "dw3_part": _sentinel(grid, (W, 256)), "db3_part": _sentinel(4 * grid, (W,), surplus=5)}
    results = {k: v[1] for k, v in wholes.items()}
    launch(d_g3, _pack_w3(d_w3), d_h2, results["g2"], results["db2_part"], results["dw3_part"], results["db3_part"],
           np.int64(R), np.int64(rpb), block=(256, 1, 1), grid=(grid, 1), shared=uk.head_bx3_lds_bytes(W))
    torch.cuda.synchronize()
    where = (W, geometry)
    _check(f"HipHeadBackwardBx3_W{W}", where, results, uk.head_reference(g3, w3, h2, rpb, grid, db3_waves=True),
           _head_yardstick(d_g3, d_w3, d_h2, R, rpb, grid, True))
    _head_common_checks(where, results, wholes, h2, R, rpb, grid)
    assert _same_bits(d_g3, g3) and _same_bits(d_h2, h2)


@pytest.mark.parametrize("W", uk.HEAD_WIDTHS)
def test_head_backward_matrix_cores_through_the_wrapper_with_two_blocks(fm, W):
    """`UpdateKernels._head_backward_bx3` at R = 77 with the cached block count set to 2: two slabs of one step and the
    host-side tail of 13 rows -- the four results against float64"""
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.training.update_kernels import UpdateKernels

    name, R = f"HipHeadBackwardBx3_W{W}", 77
    fm.initialize_functions([name])
    k = UpdateKernels(fm)
    k._head_backward_fns[("head_backward_bx3", W, str(DEV))] = (fm.get_function(name), 2)
    g3, w3, h2 = uk.head_inputs(R, W, 256, one_sign=True)
    d_g3, d_w3, d_h2 = _fenced(g3), _dev(w3), _fenced(h2)
    before = drv.LAUNCH_COUNTS[name]
    g2, db2, dw3, db3 = k._head_backward_bx3(d_g3, d_w3, d_h2)
    torch.cuda.synchronize()
    assert drv.LAUNCH_COUNTS[name] == before + 1
    ref = uk.head_reference(g3, w3, h2, R, 1)
    want = {"g2": ref["g2"], "db2": ref["db2_part"][0], "dw3": ref["dw3_part"][0], "db3": g3.astype(np.float64).sum(0)}
    y = _head_yardstick(d_g3, d_w3, d_h2, R, R, 1, False)
    yard = {"g2": y["g2"], "db2": y["db2_part"][0], "dw3": y["dw3_part"][0], "db3": d_g3.sum(0)}
    _check(name, ("wrapper", R, 2), {"g2": g2, "db2": db2, "dw3": dw3, "db3": db3}, want, yard)
    assert bool((g2[torch.from_numpy(h2 <= 0).to(DEV)] == 0).all())


# ================================================================================================ B. weight gradients
@pytest.mark.parametrize("ci,ones_col,geometry", uk.WEIGHT_GRAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_weight_grad_per_block(fm, ci, ones_col, geometry):
    """HipWeightGradBx3_256x{256,96}: slabs of 2, 4, 6 and 8 steps around its 4 stages, a last slab of 32 rows, blocks with
    nothing to do; narrow inputs of 1 .. 95 columns with and without the column of ones -- the [:, :ci] block and the bias
    column of EVERY block's partial against float64 of that block's rows, the padded columns exactly 0"""
    R, rpb, grid = geometry
    cip = 256 if ci == 256 else 96
    name = f"HipWeightGradBx3_256x{cip}"
    launch = _launcher(fm, name)
    G, X = uk.weight_grad_inputs(R, ci)
    d_G, d_X = _fenced(G), _fenced(X)
    whole, partial = _sentinel(grid, (256, cip), surplus=1)
    launch(d_G, d_X, partial, np.int64(R), np.int32(ci), np.int32(ones_col), np.int64(rpb), block=(256, 1, 1), grid=(grid, 1),
           shared=uk.weight_grad_lds_bytes(cip))
    torch.cuda.synchronize()
    where = (ci, ones_col, geometry)
    want = uk.weight_grad_reference(G, X, ones_col, rpb, grid)
    yard = torch.zeros(grid, 256, want.shape[2], device=DEV)
    ones = torch.ones(R, 1, device=DEV)
    for b, (r0, r1) in enumerate(uk.slab_rows(R, rpb, grid)):
        if r0 < r1:
            yard[b, :, :ci] = d_G[r0:r1].t() @ d_X[r0:r1]
            if ones_col >= 0:
                yard[b, :, ci:] = d_G[r0:r1].t() @ ones[r0:r1]
        else:
            assert bool((partial[b] == 0).all()), where
    results, wants, yards = {"weights": partial[:, :, :ci]}, {"weights": want[:, :, :ci]}, {"weights": yard[:, :, :ci]}
    if ones_col >= 0:
        results["bias"], wants["bias"], yards["bias"] = partial[:, :, ci], want[:, :, ci], yard[:, :, ci]
    _check(name, where, results, wants, yards)
    assert bool((partial[:, :, ci + (ones_col >= 0):] == 0).all()), where     # columns past ci (and past the ones)
    assert bool(torch.isfinite(partial).all()) and _untouched(whole, partial), where
    assert _same_bits(d_G, G) and _same_bits(d_X, X)


# ================================================================================================ B. hidden layer's input gradient
@pytest.mark.parametrize("C,R", uk.MASK_CASES)
def test_linear_mask_backward_ragged_rows(fm, C, R):
    """HipLinearMaskBackwardBx3_<C> on 1 .. 257 rows (fewer than a wavefront's 32, one more than a block's), at the exact grid
    and with one surplus block, at 512 threads and -- C = 128 / 256, whose weight chunks of 24 / 48 KB pieces divide over four
    wavefronts as they do over eight -- at 256; C = 64 (12 pieces) runs at 256 threads only.  g_out against float64, the mask
    exact, nothing past row R changed"""
    from warp_drive_amd.training.policy_kernel import _pack_indices_bx3, split_bf16x3

    name = f"HipLinearMaskBackwardBx3_{C}"
    launch = _launcher(fm, name)
    g, w, h = uk.mask_inputs(R, C)
    d_g, d_w, d_h = _fenced(g), _dev(w), _fenced(h)
    tn = C // 32
    rows, cols = _pack_indices_bx3(tn, tn, True)
    # A operand of G_out^T = W^T . G_in^T (UpdateKernels.linear_mask_backward): [k tile][term][out tile][k half][lane][8]
    wpk = split_bf16x3(d_w.t().contiguous())[:, torch.from_numpy(rows).to(DEV), torch.from_numpy(cols).to(DEV)].transpose(0, 1).contiguous()
    want = {"g_out": uk.mask_reference(g, w, h)}
    yard = {"g_out": torch.ops.aten.threshold_backward(d_g @ d_w, d_h, 0)}
    for block in uk.MASK_BLOCKS[C]:
        rows_per_block = 32 * (block // 64)
        exact = -(-R // rows_per_block)
        for grid in (exact, exact + 1):
            whole, g_out = _sentinel(R, (C,), surplus=2 * rows_per_block)
            launch(d_g, wpk, d_h, g_out, np.int64(R), block=(block, 1, 1), grid=(grid, 1), shared=uk.mask_lds_bytes(C))
            torch.cuda.synchronize()
            where = (C, R, block, grid)
            _check(name, where, {"g_out": g_out}, want, yard)
            assert bool((g_out[torch.from_numpy(h <= 0).to(DEV)] == 0).all()), where
            assert _untouched(whole, g_out), where
    assert _same_bits(d_g, g) and _same_bits(d_h, h)


# ================================================================================================ B. the objective
def _pg_float32(out, actions, adv, ret, heads):
    """the closed forms of `uk.pg_reference` in torch float32 on the device: the yardstick"""
    R, W = out.shape
    grad = torch.zeros_like(out)
    logp_taken, ent = torch.zeros(R, device=DEV), torch.zeros(R, device=DEV)
    start = 0
    for k, A in enumerate(heads):
        lp = torch.log_softmax(out[:, start:start + A], dim=-1)
        p = lp.exp()
        H = -(p * lp).sum(1)
        onehot = (torch.arange(A, device=DEV)[None, :] == actions[:, k:k + 1]).float()
        grad[:, start:start + A] = (adv[:, None] * (p - onehot) + uk.PG_ENT_COEFF * p * (lp + H[:, None])) / R
        logp_taken += lp.gather(1, actions[:, k:k + 1].long())[:, 0]
        ent += H
        start += A
    d = out[:, -1] - ret
    grad[:, -1] = 2.0 * uk.PG_VF_COEFF * d / R
    per_row = torch.stack([logp_taken * adv, ent, d * d, adv], dim=1)
    return grad, torch.stack([per_row[256 * b:256 * (b + 1)].sum(0) for b in range(-(-R // 256))])


@pytest.mark.parametrize("heads", uk.PG_HEADS, ids=str)
@pytest.mark.parametrize("R", uk.PG_ROWS)
def test_policy_gradient_head_per_block(fm, heads, R):
    """HipPolicyGradientHead on 1 .. 600 rows (a lone row, one short of / exactly / one over a block), logits of magnitude up to
    300, `out` / `grad` aligned to 16 bytes and at a float offset of 1 (the single-float copy path): the gradient and the four
    sums of EVERY block against the float64 closed forms"""
    launch = _launcher(fm, "HipPolicyGradientHead")
    out, actions, adv, ret = uk.pg_inputs(heads, R)
    W, blocks = out.shape[1], -(-R // 256)
    want_grad, want_sums = uk.pg_reference(out, actions, adv, ret, heads)
    d_actions, d_adv, d_ret = _dev(actions), _fenced(adv), _fenced(ret)
    a1 = heads[1] if len(heads) > 1 else 0
    for offset in (0, 1):
        d_out = _fenced(out, offset=offset)
        assert (d_out.data_ptr() % 16 == 0) == (offset == 0)
        w_grad, grad = _sentinel(R, (W,), offset=offset)
        w_sums, sums = _sentinel(blocks, (4,), surplus=2)
        launch(d_out, d_actions, d_adv, d_ret, grad, sums, np.int32(R), np.int32(heads[0]), np.int32(a1), np.float32(1.0 / R),
               np.float32(uk.PG_ENT_COEFF), np.float32(uk.PG_VF_COEFF), block=(256, 1, 1), grid=(blocks, 1), shared=4 * 256 * W)
        torch.cuda.synchronize()
        y_grad, y_sums = _pg_float32(d_out, d_actions, d_adv, d_ret, heads)
        names = ("logp_adv", "entropy", "vf", "adv")
        _check("HipPolicyGradientHead", (heads, R, offset),
               {"grad": grad, **{n: sums[:, i] for i, n in enumerate(names)}},
               {"grad": want_grad, **{n: want_sums[:, i] for i, n in enumerate(names)}},
               {"grad": y_grad, **{n: y_sums[:, i] for i, n in enumerate(names)}})
        assert _untouched(w_grad, grad, offset) and _untouched(w_sums, sums), (heads, R, offset)
        assert _same_bits(d_out, out)


# ================================================================================================ coverage
def test_every_entry_of_the_update_object_has_a_direct_launch_here():
    """the kernels the build's manifest places in the update object = the entries the tests above launch (each of which
    asserts its launch through hip_driver.LAUNCH_COUNTS)"""
    from warp_drive_amd.managers import hip_driver as drv

    launched = ({"HipDiscountedReturns", "HipReluBackwardColumnSums", "HipPolicyGradientHead"}
                | {f"HipHeadBackward_W{W}" for W, _, _ in uk.HEAD_VECTOR_CASES} | {f"HipHeadBackwardBx3_W{W}" for W, _ in uk.HEAD_BX3_CASES}
                | {f"HipWeightGradBx3_256x{256 if ci == 256 else 96}" for ci, _, _ in uk.WEIGHT_GRAD_CASES}
                | {f"HipLinearMaskBackwardBx3_{C}" for C, _ in uk.MASK_CASES})
    in_object = {k for k, v in drv.manifest().items() if v == drv.manifest()["HipDiscountedReturns"]}
    assert in_object == launched, in_object ^ launched
    assert drv.manifest()["HipRolloutRecord"] != drv.manifest()["HipDiscountedReturns"]
