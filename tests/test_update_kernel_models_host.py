"""tests/update_kernel_cases.py on the host: its numpy models against independent forms, conditions against the cases
passing vacuously, the teeth of the bf16x3 bound, and the cases' legality against the kernels' stated contracts.

The bound of the GPU file, err <= max(4 * err_f32, 2e-6 * scale), is a condition here, not a measurement: on every bf16x3
case's inputs the emulated six-partial-product arithmetic meets it and the arithmetic that drops the third bf16 term of
either operand violates it.  The float32 yardstick here is numpy's float32 matmul; the GPU file's is the framework's GEMM
on the device, so the condition is checked on the CPU only.

The last tests are the host side of the mutation check: restated defects (the wrong policy's agents summed, the value
column ignored, a slab's final step skipped, a bf16 term dropped) each change a model or break the bound on the cases'
own inputs, so a kernel with that defect cannot pass the GPU file."""
import numpy as np
import pytest
import torch

from tests import update_kernel_cases as uk

f32, f64 = np.float32, np.float64
U = 2.0 ** -24   # float32 unit roundoff


# ------------------------------------------------------------------------------------------------ helpers of the helpers
def test_seq_sum_is_the_sequential_float32_sum_from_plus_zero():
    x = (np.random.RandomState(0).standard_normal(300) * 10.0 ** np.random.RandomState(1).uniform(-3, 3, 300)).astype(f32)
    s = f32(0.0)
    for v in x:
        s = f32(s + v)
    assert uk.seq_sum_f32(x) == s and uk.seq_sum_f32(x) != f32(x.astype(f64).sum())
    assert not np.signbit(uk.seq_sum_f32(np.array([-0.0], f32)))   # 0.0f + -0.0f = +0.0f
    m = np.arange(12, dtype=f32).reshape(3, 4)
    assert np.array_equal(uk.seq_sum_f32(m, axis=0), m.sum(0)) and uk.seq_sum_f32(np.zeros((0, 4), f32), axis=0).shape == (4,)


def test_bf16_split_is_the_products_split():
    from warp_drive_amd.training.policy_kernel import split_bf16x3

    rng = np.random.RandomState(2)
    x = np.concatenate([(rng.standard_normal(5000) * 10.0 ** rng.uniform(-6, 6, 5000)).astype(f32),
                        uk.full_mantissa(rng, (500,)), np.array([0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9], f32)])
    want = split_bf16x3(torch.from_numpy(x)).float().numpy()
    got = uk.split3(x)
    for term in range(3):
        assert np.array_equal(uk.bits(got[term]), uk.bits(want[term])), term
    nz = x != 0
    assert np.abs((got[0].astype(f64) + got[1] + got[2] - x)[nz] / x[nz]).max() <= 2.0 ** -24


def test_full_mantissa_values_carry_a_large_third_term_of_one_sign():
    x = uk.full_mantissa(np.random.RandomState(3), (4000,), (-2, 0, 3))
    lo = uk.split3(x)[2]
    assert (x > 0).all() and (lo / x > 5.9e-6).all() and (lo / x < 7.7e-6).all()


# ------------------------------------------------------------------------------------------------ A. HipRolloutRecord
@pytest.mark.parametrize("case", uk.RECORD_CASES, ids=lambda c: c.name)
def test_record_model_against_the_trainers_per_op_formulas(case):
    """float64 torch, the per-op tick of Trainer (`ep_reward += r; ep_sum += ep_reward.mean(1) * finished; ep_reward *= 1 -
    finished`, index_copy_ of row t) -- the model within float32 rounding of the sums involved, batches exactly"""
    slot, na, nb = case.slot()
    rewards, done = case.inputs()
    E = case.E
    init, model = case.initial_state(), uk.record_run_model(case)
    pol = slot >> 16
    for p, (n_pol, sfx) in enumerate(((na, "a"), (nb, "b"))):
        if not n_pol:
            assert model[f"reward_batch_{sfx}"].size == 0 and np.array_equal(model[f"ep_sum_{sfx}"], init[f"ep_sum_{sfx}"])
            continue
        ids = torch.from_numpy(np.flatnonzero(pol == p))
        assert np.array_equal(slot[ids.numpy()] & 0xffff, np.arange(n_pol))   # the batch's agent order = ascending agent id
        ep_reward = torch.from_numpy(init[f"ep_reward_{sfx}"][:E].astype(f64))
        ep_sum = torch.from_numpy(init[f"ep_sum_{sfx}"][:E].astype(f64))
        batch = torch.zeros(uk.RECORD_ROWS, E, n_pol, dtype=torch.float64)
        magnitude = ep_reward.abs().mean(1)
        for tick in range(uk.RECORD_TICKS):
            r = torch.from_numpy(rewards[tick, :E].astype(f64)).index_select(1, ids)
            finished = torch.from_numpy((done[tick, :E] > 0).astype(f64))
            batch.index_copy_(0, torch.tensor([uk.RECORD_FIRST_ROW + tick]), r.unsqueeze(0))
            ep_reward += r
            ep_sum += ep_reward.mean(dim=1) * finished
            ep_reward *= (1.0 - finished)[:, None]
            magnitude += r.abs().mean(1)
        rows = slice(uk.RECORD_FIRST_ROW, uk.RECORD_FIRST_ROW + uk.RECORD_TICKS)
        assert np.array_equal(model[f"reward_batch_{sfx}"][rows].astype(f64), batch[rows].numpy())
        # a total is <= 7 float32 additions, a sum of n_pol of them n_pol more, then a division and an addition per episode
        tol = U * (n_pol + 7 + 2 * uk.RECORD_TICKS) * (magnitude.numpy() + np.abs(init[f"ep_sum_{sfx}"][:E]))
        assert (np.abs(model[f"ep_sum_{sfx}"][:E] - ep_sum.numpy()) <= tol).all()
        assert (np.abs(model[f"ep_reward_{sfx}"][:E] - ep_reward.numpy()) <= U * 8 * (magnitude.numpy()[:, None] * n_pol)).all()
    episodes = (done[:, :E] > 0).sum(0)
    assert np.array_equal(model["ep_count"][:E], init["ep_count"][:E] + episodes)
    assert np.array_equal(model["done_batch"][uk.RECORD_FIRST_ROW:uk.RECORD_FIRST_ROW + uk.RECORD_TICKS], done[:, :E])
    assert (model["batch_row"][:E] == uk.RECORD_FIRST_ROW + uk.RECORD_TICKS).all()
    # rows 0, 1 and 8 and the replicas past E are nobody's
    for name in uk.RECORD_STATE_NAMES:
        if name in ("reward_batch_a", "reward_batch_b", "done_batch"):
            for row in (0, 1, 8):
                assert np.array_equal(uk.bits(model[name][row]), uk.bits(init[name][row])), (name, row)
        else:
            assert np.array_equal(uk.bits(model[name][E:]), uk.bits(init[name][E:])), name


def test_record_cases_cannot_pass_vacuously():
    seen = set()
    for case in uk.RECORD_CASES:
        slot, na, nb = case.slot()
        assert na + nb == case.N and sorted(slot[slot < 65536]) == list(range(na)) and sorted(slot[slot >= 65536] - 65536) == list(range(nb))
        _, done = case.inputs()
        patterns = {case.pattern_of(e) for e in range(case.E)}
        seen |= patterns
        if case.E >= len(uk.DONE_PATTERNS):
            assert patterns == set(uk.DONE_PATTERNS), case.name          # every done pattern occurs
        assert ((done[:, :case.E] > 0).sum(0) >= 2).any(), case.name     # a replica finishes twice
        if case.N > 1:   # the order of the float32 additions shows in at least one sum
            a, b = uk.record_run_model(case), uk.record_run_model(case, summation="f64")
            assert any((a[k][:case.E] != b[k][:case.E]).any() for k in ("ep_sum_a", "ep_sum_b")), case.name
    assert seen == set(uk.DONE_PATTERNS)
    assert {p for p in uk.DONE_PATTERNS.values()} >= {(0,) * 6, (1,) * 6, (1, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 1)}
    assert any(2 in p for p in uk.DONE_PATTERNS.values()) and any("11" in "".join(map(str, p)) and 0 in p for p in uk.DONE_PATTERNS.values())
    by_name = {c.name: c for c in uk.RECORD_CASES}
    assert by_name["N105-interleaved-E130"].N > 64 and by_name["N1100-contiguous-E3"].N > 1024   # two trips of the agent loop
    assert (by_name["N105-interleaved-E130"].slot()[0][2::3] >= 65536).all()


# ------------------------------------------------------------------------------------------------ A. HipDiscountedReturns
@pytest.mark.parametrize("case", uk.RETURNS_CASES, ids=lambda c: c.name)
def test_returns_model_is_the_frameworks_recursion_bit_for_bit(case):
    from warp_drive_amd.training.losses import discounted_returns

    rewards, done, out = case.inputs()
    if case.T * case.E >= 12:
        assert set(np.unique(done)) == {0, 1, 2} and len(set(done[-1])) == 3
    for gamma in uk.RETURNS_GAMMAS:
        got, adv = uk.returns_model(rewards, done, out, case.v_col, gamma)
        v = torch.from_numpy(np.ascontiguousarray(out[..., case.v_col]))
        want = discounted_returns(torch.from_numpy(rewards), torch.from_numpy(done), v, gamma)
        assert np.array_equal(uk.bits(got), uk.bits(want.numpy()))
        assert np.array_equal(uk.bits(adv), uk.bits((want - v).numpy()))
        # and against float64: a float32 recursion of T steps
        want64 = discounted_returns(torch.from_numpy(rewards.astype(f64)), torch.from_numpy(done), v.double(), gamma).numpy()
        assert np.abs(got - want64).max() <= 4 * case.T * U * max(1.0, np.abs(want64).max())


def test_returns_cases_use_other_columns_blocks_and_surplus_grids():
    cols = {(c.W, c.v_col) for c in uk.RETURNS_CASES}
    assert any(v != W - 1 for W, v in cols) and any(v == 0 for _, v in cols) and any(v == W - 1 for W, v in cols)
    assert {c.block for c in uk.RETURNS_CASES} == {64, 128, 256}
    assert any(c.grid * c.block >= c.E * c.n + 2 * c.block for c in uk.RETURNS_CASES)
    assert any(c.grid == 2 and c.E * c.n == c.block + 2 for c in uk.RETURNS_CASES)
    assert all(c.block <= 256 and c.grid * c.block >= c.E * c.n and c.v_col < c.W for c in uk.RETURNS_CASES)


# ------------------------------------------------------------------------------------------------ A. HipReluBackwardColumnSums
@pytest.mark.parametrize("C", uk.COLSUM_WIDTHS)
@pytest.mark.parametrize("R,rows_per_block,grid", uk.COLSUM_GEOMETRIES)
def test_colsum_model_against_threshold_backward_and_a_float64_sum(R, rows_per_block, grid, C):
    gx, y = uk.colsum_inputs(R, C)
    assert (uk.bits(y) == 0).any() and (uk.bits(y) == 0x80000000).any()
    g, partial = uk.colsum_model(gx, y, rows_per_block, grid)
    want = torch.ops.aten.threshold_backward(torch.from_numpy(gx.astype(f64)), torch.from_numpy(y.astype(f64)), 0).numpy()
    assert np.array_equal(g.astype(f64), want) and not np.signbit(g[y <= 0]).any()
    assert C % 4 == 0 and 256 % (C // 4) == 0 and grid * rows_per_block >= R
    for b, (r0, r1) in enumerate(uk.slab_rows(R, rows_per_block, grid)):
        rows = r1 - r0
        assert (np.abs(partial[b] - want[r0:r1].sum(0)) <= U * (rows + 1) * np.abs(want[r0:r1]).sum(0)).all()
        if rows == 0:
            assert np.array_equal(uk.bits(partial[b]), np.zeros(C, np.uint32))
    if rows_per_block * C > 1024 and R >= 64:   # more than one row per thread: the order shows
        assert (partial != np.stack([g[r0:r1].astype(f64).sum(0) for r0, r1 in uk.slab_rows(R, rows_per_block, grid)]).astype(f32)).any()


# ------------------------------------------------------------------------------------------------ B. teeth of the bf16x3 bound
def _product(drop):
    return lambda a, b: uk.bf16x3_product(a, b, drop)


def _verdicts(results, want, yard, names):
    return {k: uk.within_bound(*uk.judge(results[k], want[k], yard[k])) for k in names}


@pytest.mark.parametrize("W,geometry", uk.HEAD_BX3_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_head_backward_bx3_bound_passes_six_products_and_fails_five(W, geometry):
    R, rpb, grid = geometry
    g3, w3, h2 = uk.head_inputs(R, W, 256, one_sign=True)
    assert (uk.bits(h2) == 0).any() and (uk.bits(h2) == 0x80000000).any() and (h2 >= 0).all()
    want = uk.head_reference(g3, w3, h2, rpb, grid, db3_waves=True)
    yard = uk.head_reference(g3, w3, h2, rpb, grid, dtype=f32, db3_waves=True)
    names = ("g2", "db2_part", "dw3_part")
    full = uk.head_reference(g3, w3, h2, rpb, grid, dtype=f32, product=_product(None), db3_waves=True)
    assert all(_verdicts(full, want, yard, names + ("db3_part",)).values())
    for drop in ("a", "b"):
        less = uk.head_reference(g3, w3, h2, rpb, grid, dtype=f32, product=_product(drop), db3_waves=True)
        assert not any(_verdicts(less, want, yard, names).values()), drop
    # the per-wavefront rows of db3_part add up to the block's column sums
    assert np.allclose(want["db3_part"].reshape(grid, 4, W).sum(1), np.stack([g3[a:b].astype(f64).sum(0) for a, b in uk.slab_rows(R, rpb, grid)]))


@pytest.mark.parametrize("ci,ones_col,geometry", uk.WEIGHT_GRAD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_weight_grad_bound_passes_six_products_and_fails_five(ci, ones_col, geometry):
    R, rpb, grid = geometry
    G, X = uk.weight_grad_inputs(R, ci)
    assert (G == 0).all(1).any() and not (G == 0).all(1).all()
    want = uk.weight_grad_reference(G, X, ones_col, rpb, grid)
    yard = uk.weight_grad_reference(G, X, ones_col, rpb, grid, dtype=f32)
    parts = {"weights": np.s_[:, :, :ci]}
    if ones_col >= 0:
        parts["bias"] = np.s_[:, :, ci]
    full = uk.weight_grad_reference(G, X, ones_col, rpb, grid, dtype=f32, product=_product(None))
    for sl in parts.values():
        assert uk.within_bound(*uk.judge(full[sl], want[sl], yard[sl]))
    for drop in ("a", "b"):
        less = uk.weight_grad_reference(G, X, ones_col, rpb, grid, dtype=f32, product=_product(drop))
        assert not uk.within_bound(*uk.judge(less[parts["weights"]], want[parts["weights"]], yard[parts["weights"]])), drop
    if ones_col >= 0:   # (the ones have no third term: only G's shows in the bias column)
        less = uk.weight_grad_reference(G, X, ones_col, rpb, grid, dtype=f32, product=_product("a"))
        assert not uk.within_bound(*uk.judge(less[parts["bias"]], want[parts["bias"]], yard[parts["bias"]]))


@pytest.mark.parametrize("C,R", uk.MASK_CASES)
def test_mask_backward_bound_passes_six_products_and_fails_five(C, R):
    g, w, h = uk.mask_inputs(R, C)
    want, yard = uk.mask_reference(g, w, h), uk.mask_reference(g, w, h, dtype=f32)
    assert (want[h <= 0] == 0).all() and (h <= 0).any() and (h > 0).any()
    assert uk.within_bound(*uk.judge(uk.mask_reference(g, w, h, dtype=f32, product=_product(None)), want, yard))
    for drop in ("a", "b"):
        assert not uk.within_bound(*uk.judge(uk.mask_reference(g, w, h, dtype=f32, product=_product(drop)), want, yard)), drop


# ------------------------------------------------------------------------------------------------ B. the other references
@pytest.mark.parametrize("heads", uk.PG_HEADS, ids=str)
def test_policy_gradient_reference_is_float64_autograd_of_the_objective(heads):
    """the closed forms of the kernel's comment = autograd of loss = mean(-logp(a) adv) + vf mean((v - ret)^2) - ent sum_heads
    mean(H), in float64; the per-block sums add up to the terms of that loss"""
    R = 257
    out, actions, adv, ret = uk.pg_inputs(heads, R)
    assert np.abs(out[:, :-1]).max() >= 200.0 and all((actions[:, k] < A).all() and (actions[:, k] >= 0).all() for k, A in enumerate(heads))
    grad, sums = uk.pg_reference(out, actions, adv, ret, heads)
    z = torch.from_numpy(out.astype(f64)).requires_grad_(True)
    a, rt = torch.from_numpy(adv.astype(f64)), torch.from_numpy(ret.astype(f64))
    logp, ent, start = 0.0, 0.0, 0
    for k, A in enumerate(heads):
        lp = torch.log_softmax(z[:, start:start + A], dim=-1)
        logp = logp + lp.gather(1, torch.from_numpy(actions[:, k:k + 1].astype(np.int64)))[:, 0]
        ent = ent - (lp.exp() * lp).sum(1)
        start += A
    loss = (-logp * a).mean() + uk.PG_VF_COEFF * ((z[:, -1] - rt) ** 2).mean() - uk.PG_ENT_COEFF * ent.mean()
    loss.backward()
    assert np.abs(grad - z.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(grad).max())
    total = sums.sum(0)
    assert sums.shape == (2, 4)
    want = [float(v.detach()) for v in ((logp * a).sum(), ent.sum(), ((z[:, -1] - rt) ** 2).sum(), a.sum())]
    assert np.allclose(total, want, rtol=1e-12, atol=1e-12)


def test_head_vector_reference_per_block_adds_up():
    g3, w3, h2 = uk.head_inputs(100, 6, 64)
    assert (uk.bits(h2) == 0x80000000).any()
    ref = uk.head_reference(g3, w3, h2, 40, 3)
    whole = uk.head_reference(g3, w3, h2, 4096, 1)
    assert np.allclose(ref["db2_part"].sum(0), whole["db2_part"][0]) and np.allclose(ref["dw3_part"].sum(0), whole["dw3_part"][0])
    assert np.array_equal(ref["g2"], whole["g2"]) and (ref["g2"][h2 <= 0] == 0).all()
    t = torch.ops.aten.threshold_backward(torch.from_numpy(g3.astype(f64) @ w3.astype(f64)), torch.from_numpy(h2.astype(f64)), 0)
    assert np.array_equal(ref["g2"], t.numpy())


def test_head_backward_row_index_trick_is_exact():
    """HipHeadBackward_W<W> stages g3 with r = (int)((q + 0.5f) * (1.0f / W)) for q / W: exact for every q < 32 W"""
    from warp_drive_amd.training.update_kernels import UpdateKernels

    assert tuple(UpdateKernels.HEAD_WIDTHS) == uk.HEAD_WIDTHS
    for W in UpdateKernels.HEAD_WIDTHS:
        q = np.arange(32 * W)
        r = ((q.astype(f32) + f32(0.5)) * (f32(1.0) / f32(W))).astype(f32).astype(np.int32)
        assert np.array_equal(r, q // W), W


# ------------------------------------------------------------------------------------------------ legality of the cases
class _Recorder:
    def __init__(self):
        self.calls = []

    def __call__(self, *args, **kw):
        self.calls.append((args, kw))


def _wrapper_without_a_device():
    """an UpdateKernels object whose cached entries are recorders: its wrappers then run on CPU tensors up to the launch,
    which is recorded (grid, block, LDS bytes) instead of made"""
    from warp_drive_amd.training.update_kernels import UpdateKernels

    k = object.__new__(UpdateKernels)
    k._fm, k._head_backward_fns = None, {}
    return k


def test_lds_bytes_are_the_wrappers_formulas():
    from warp_drive_amd.training.policy_kernel import _pack_indices_bx3
    from warp_drive_amd.training.update_kernels import UpdateKernels

    assert UpdateKernels.HEAD_BACKWARD_STAGES == uk.HEAD_BX3_STAGES and UpdateKernels.WEIGHT_GRAD_STAGES == uk.WEIGHT_GRAD_STAGES
    k = _wrapper_without_a_device()
    for W in uk.HEAD_WIDTHS:
        rec = k._head_backward_fns[("head_backward_bx3", W, "cpu")] = (_Recorder(), 2)
        k._head_backward_bx3(torch.zeros(64, W), torch.zeros(W, 256), torch.zeros(64, 256))
        assert rec[0].calls[0][1]["shared"] == uk.head_bx3_lds_bytes(W) <= 160 * 1024, W
    for ci, cip in ((256, 256), (71, 96)):
        rec = k._head_backward_fns[("weight_grad", cip, "cpu")] = (_Recorder(), 2)
        k.weight_grad(torch.zeros(64, 256), torch.zeros(64, ci))
        assert rec[0].calls[0][1]["shared"] == uk.weight_grad_lds_bytes(cip) <= 160 * 1024, cip
    for C in (64, 128, 256):
        rows, cols = _pack_indices_bx3(C // 32, C // 32, True)
        rec = k._head_backward_fns[("mask_backward", C, "cpu")] = (_Recorder(), torch.from_numpy(rows), torch.from_numpy(cols))
        k.linear_mask_backward(torch.zeros(40, C), torch.zeros(C, C), torch.zeros(40, C))
        kw = rec[0].calls[0][1]
        assert kw["shared"] == uk.mask_lds_bytes(C) <= 160 * 1024 and kw["block"][0] == uk.MASK_BLOCKS[C][0], C


def test_cases_are_inside_the_kernels_contracts():
    # the matrix-core kernels: R and rows_per_block multiples of 32, the grid covers R; below / at / over the pipeline depth
    for geometries, stages, step in ((uk.HEAD_BX3_GEOMETRIES, uk.HEAD_BX3_STAGES, uk.HEAD_BX3_STEP_ROWS),
                                     (uk.WEIGHT_GRAD_GEOMETRIES, uk.WEIGHT_GRAD_STAGES, uk.WEIGHT_GRAD_STEP_ROWS)):
        steps = set()
        for R, rpb, grid in geometries:
            assert R % 32 == 0 and rpb % 32 == 0 and R > 0 and grid * rpb >= R and R <= 4096
            steps |= {(b - a) // step for a, b in uk.slab_rows(R, rpb, grid)}
        assert 0 in steps and any(0 < s < stages for s in steps) and stages in steps and any(s > stages for s in steps)
    assert all(0 < ci <= 95 or ci == 256 for ci, _, _ in uk.WEIGHT_GRAD_CASES)
    assert all(ones in (-1, ci) and (ones < 96) for ci, ones, _ in uk.WEIGHT_GRAD_CASES)
    assert (95, 95) in {(ci, ones) for ci, ones, _ in uk.WEIGHT_GRAD_CASES}      # the ones in the last padded column
    # vector-unit head backward: block = C threads <= its launch bound, every (W, C) pair, tiles of 32, 32 + 8, < 32, none
    assert {(W, C) for W, C, _ in uk.HEAD_VECTOR_CASES} == {(W, C) for W in uk.HEAD_WIDTHS for C in (64, 128, 256)}
    tiles = set()
    for W, C, (R, rpb, grid) in uk.HEAD_VECTOR_CASES:
        assert C <= 256 and W <= 64 and grid * rpb >= R
        tiles |= {(b - a) % 32 for a, b in uk.slab_rows(R, rpb, grid)} | {b - a for a, b in uk.slab_rows(R, rpb, grid) if b - a < 32}
    assert {0, 1, 5, 8} <= tiles
    # column sums: C / 4 divides 256, a float4 per thread
    assert all(C % 4 == 0 and 256 % (C // 4) == 0 and 16 <= C <= 256 for C in uk.COLSUM_WIDTHS)
    assert any(grid * rpb >= R + 2 * rpb for R, rpb, grid in uk.COLSUM_GEOMETRIES)
    # mask backward: blocks at or under __launch_bounds__(512), a chunk's pieces divide over the wavefronts
    for C, blocks in uk.MASK_BLOCKS.items():
        for block in blocks:
            assert block in (256, 512) and (6 * C // 32) % (block // 64) == 0, (C, block)
    assert (6 * 64 // 32) % 8 != 0   # why C = 64 has no 512-thread case
    # objective: one or two heads, W <= 64, 64 KB of LDS at most
    assert all(1 <= len(h) <= 2 and sum(h) + 1 <= 64 for h in uk.PG_HEADS) and max(sum(h) + 1 for h in uk.PG_HEADS) == 64
    assert {r % 256 for r in uk.PG_ROWS} >= {0, 1, 255} and max(uk.PG_ROWS) <= 4096
    # record: blocks are multiples of 64 up to 1024, LDS = 4 N bytes
    assert all(b % 64 == 0 and 64 <= b <= 1024 for c in uk.RECORD_CASES for b in c.blocks)
    assert max(c.N for c in uk.RECORD_CASES) * 4 <= 64 * 1024 and max(c.N for c in uk.RECORD_CASES) < 65536


# ------------------------------------------------------------------------------------------------ host side of the mutation check
def test_summing_the_wrong_policys_agents_changes_the_record_model():
    for case in uk.RECORD_CASES:
        if case.slot()[2] == 0:
            continue
        good, bad = uk.record_run_model(case), uk.record_run_model(case, sum_policy_of=(1, 0))
        assert (good["ep_sum_a"][:case.E] != bad["ep_sum_a"][:case.E]).any() and (good["ep_sum_b"][:case.E] != bad["ep_sum_b"][:case.E]).any()


def test_ignoring_v_col_changes_the_returns_model():
    hit = 0
    for case in uk.RETURNS_CASES:
        if case.v_col == case.W - 1:
            continue
        rewards, done, out = case.inputs()
        for gamma in uk.RETURNS_GAMMAS:
            good, bad = uk.returns_model(rewards, done, out, case.v_col, gamma), uk.returns_model(rewards, done, out, case.W - 1, gamma)
            assert (good[0] != bad[0]).any() and (good[1] != bad[1]).any()
            hit += 1
    assert hit >= 4


def test_skipping_a_slabs_final_step_breaks_the_bound():
    """both persistent kernels: the last 32 (head backward) / 16 (weight gradient) rows of the last non-empty slab left out"""
    for W, (R, rpb, grid) in uk.HEAD_BX3_CASES:
        g3, w3, h2 = uk.head_inputs(R, W, 256, one_sign=True)
        want = uk.head_reference(g3, w3, h2, rpb, grid, db3_waves=True)
        yard = uk.head_reference(g3, w3, h2, rpb, grid, dtype=f32, db3_waves=True)
        cut = uk.head_reference(g3[:R - 32], w3, h2[:R - 32], rpb, grid, dtype=f32, product=_product(None), db3_waves=True)
        for k in ("db2_part", "dw3_part", "db3_part"):
            assert not uk.within_bound(*uk.judge(cut[k], want[k], yard[k])), (W, R, k)
    for ci, ones, (R, rpb, grid) in uk.WEIGHT_GRAD_CASES:
        G, X = uk.weight_grad_inputs(R, ci)
        want = uk.weight_grad_reference(G, X, ones, rpb, grid)
        yard = uk.weight_grad_reference(G, X, ones, rpb, grid, dtype=f32)
        cut = uk.weight_grad_reference(G[:R - 16], X[:R - 16], ones, rpb, grid, dtype=f32, product=_product(None))
        assert not uk.within_bound(*uk.judge(cut, want, yard)), (ci, R)
