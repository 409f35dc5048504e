"""tests/big_offset_cases.py on the host.

Layout, at the REAL boundaries (2^30, 2^31, 2^32 elements; nothing is allocated): every band straddles the boundary row it
claims, holds a whole aligned block / tile / 32-row step of its kernel on both sides, the bands of a case do not overlap,
every case stays under the memory cap, and a tensor reaches exactly the boundaries the case claims for it.

Teeth, at the boundaries scaled down to 2^10, 2^11, 2^12 elements: the same case builders and the same checks against numpy
stand-ins of the kernels whose flat offsets go through a map.  With the identity every case passes its own checks; with an
offset taken mod 2^32 ("u32"), sign-wrapped at 2^31 ("s32": zeros read, writes dropped) or a byte offset taken mod 2^32
("byte"), applied to each big tensor of the case in turn, the case FAILS its checks wherever the tensor crosses the mutated
boundary.  `NOT_CROSSED` lists the (tensor, boundary) pairs that do not, where the mutation is the identity and the case
must pass."""
import numpy as np
import pytest

from tests import big_offset_cases as bo
from tests import update_kernel_cases as uk

f32, f64 = np.float32, np.float64

# The pairs a case cannot reach under the 64 GB cap (the docstrings of the cases give the sizes): nothing else is excused.
NOT_CROSSED = {
    ("HipWeightGradBx3_256x96", "x", "b31"), ("HipWeightGradBx3_256x96", "x", "b32"),
    ("HipHeadBackwardBx3_W43", "g3", "b31"), ("HipHeadBackwardBx3_W43", "g3", "b32"),
    ("HipHeadBackward_W43 C=64", "g3", "b32"),
    ("HipRolloutRecord (b)", "reward_batch", "b32"), ("HipRolloutRecord (b)", "done_batch", "b32"),
}
SMALL_CASES = bo.all_cases(bo.SMALL)
REAL_CASES = bo.all_cases(bo.REAL)
ids = lambda c: c.name  # noqa: E731


def test_the_excused_pairs_are_the_ones_the_cases_do_not_claim_and_do_not_reach():
    for cases in (SMALL_CASES, REAL_CASES):
        assert {(c.name, t, b) for c in cases for t, b in c.not_crossed()} == NOT_CROSSED
        for c in cases:
            for t, b in c.claims:
                assert c.reach(t, b), (c.name, t, b)
            for t, b in c.not_crossed():     # (not merely unclaimed: the tensor ends in front of the boundary)
                assert not c.reach(t, b), (c.name, t, b)


def test_every_kernel_of_the_issue_has_a_case():
    assert [c.name for c in REAL_CASES] == [
        "HipPolicyGradientHead", "HipDiscountedReturns", "HipReluBackwardColumnSums C=256", "HipReluBackwardColumnSums C=64",
        "HipLinearMaskBackwardBx3_256", "HipWeightGradBx3_256x256", "HipWeightGradBx3_256x96", "HipHeadBackwardBx3_W43",
        "HipHeadBackward_W43 C=64", "HipRolloutRecord (a)", "HipRolloutRecord (b)"]


# ================================================================================================ layout, real boundaries
def test_boundary_rows_are_the_ones_worked_out_on_paper():
    by = {c.name: c for c in REAL_CASES}
    pg = by["HipPolicyGradientHead"]
    assert [pg.boundary_rows[("out", b)] for b in bo.BOUNDARIES] == [24970740, 49941480, 99882960] and pg.R < 2 ** 31
    assert pg.R % 256 and pg.R % 32
    for name in ("HipReluBackwardColumnSums C=256", "HipLinearMaskBackwardBx3_256", "HipWeightGradBx3_256x256", "HipWeightGradBx3_256x96"):
        c = by[name]
        assert c.R == 2 ** 24 + 4096 + 7 and c.R % 32 == 7
        t = "gx" if "Relu" in name else ("g_in" if "Mask" in name else "g")
        assert [c.boundary_rows[(t, b)] for b in bo.BOUNDARIES] == [4194304, 8388608, 16777216]
    assert by["HipWeightGradBx3_256x96"].boundary_rows[("x", "b30")] == 15123124
    assert by["HipReluBackwardColumnSums C=64"].bytes() - by["HipReluBackwardColumnSums C=64"].small_bytes == \
        pytest.approx(by["HipReluBackwardColumnSums C=256"].bytes(), rel=1e-3)
    assert by["HipHeadBackwardBx3_W43"].boundary_rows[("g3", "b30")] == 24970740 and by["HipHeadBackwardBx3_W43"].R % 32
    hv = by["HipHeadBackward_W43 C=64"]
    assert hv.boundary_rows[("g3", "b31")] == 49941480 and hv.boundary_rows[("h2", "b32")] == 2 ** 26 and hv.R % 32
    ret = by["HipDiscountedReturns"]
    assert ret.E * ret.n >= 20000100 and ret.R * 43 > 2 ** 32
    # the chain that meets 2^31 and the chain that meets 2^32 do so at different t; chains near the latter are past 2^31 at t = 3
    assert [ret.boundary_rows[("out", b)] // ret.S for b in bo.BOUNDARIES] == [1, 2, 4]
    a, b = by["HipRolloutRecord (a)"], by["HipRolloutRecord (b)"]
    assert [a.boundary_rows[("reward_batch", k)] for k in bo.BOUNDARIES] == [5368, 10737, 21474]
    assert [b.boundary_rows[("done_batch", k)] for k in bo.BOUNDARIES[:2]] == [536870, 1073741]


@pytest.mark.parametrize("case", REAL_CASES, ids=ids)
def test_bands_straddle_hold_a_unit_on_both_sides_and_do_not_overlap(case):
    assert case.bytes() < bo.CAP_BYTES, case.bytes()
    if isinstance(case, bo.RecordCase):
        for (t, b), r in case.boundary_rows.items():
            w = case.widths[t]
            assert r * w <= bo.REAL.e[b] < (r + 1) * w and {r - 1, r, r + 1} <= set(case.ts) and r + 1 < case.R - 1
        assert len(set(case.ts)) == len(case.ts) and 0 in case.ts
        return
    returns = isinstance(case, bo.DiscountedReturnsCase)
    raw = (case.chains if returns else case.layout).raw
    unit, period = case.unit, (case.S if returns else None)
    for (t, b), r in case.boundary_rows.items():
        w = case.widths[t]
        assert r * w <= bo.REAL.e[b] < (r + 1) * w                                   # the boundary lies in row r
        pos = r % period if returns else r
        a, z = next((a, z) for a, z, _ in raw if a <= pos < z)
        assert -(-a // unit) * unit + unit <= pos, (case.name, t, b, "no whole unit in front of the boundary row")
        assert -(-(pos + 1) // unit) * unit + unit <= z, (case.name, t, b, "no whole unit behind the boundary row")
    spans = sorted((a, z) for a, z, _ in raw)
    assert all(z0 <= a1 for (_, z0), (a1, _) in zip(spans, spans[1:])), (case.name, "bands overlap")
    assert spans[0][0] == 0 and spans[-1][1] == (case.S if returns else case.R)      # row 0 and the ragged end
    assert case.layout.nb < 40000                                                    # (a few hundred rows per band)
    if returns:   # every t of a band chain is a band of the row space, and the rows of `out` that hold the boundaries are in one
        for r in case.boundary_rows.values():
            assert any(a <= r < z for a, z in case.layout.bands)
    else:
        assert spans[-1][1] - spans[-1][0] > case.R % 32 > 0                         # a wrapper's host-side tail is seeded


def test_band_contents_all_differ():
    """no two band rows of an input are equal (the whole zero rows that masked gradients have aside), so a wrapped read
    cannot meet its own data"""
    for c in SMALL_CASES + [bo.MaskBackwardCase(bo.REAL), bo.PolicyGradientHeadCase(bo.REAL)]:
        if isinstance(c, bo.RecordCase):
            x = {"rewards": c.inputs()[0].reshape(len(c.ts), -1)}
        else:
            x = {k: v for k, v in c.inputs().items() if k in c.widths or k in ("rewards",)}
        for k, v in x.items():
            live = v[np.abs(v).reshape(v.shape[0], -1).max(1) > 0]
            assert v.shape[0] == c.layout.nb and len(live) > 0.7 * c.layout.nb and len(np.unique(live, axis=0)) == len(live), (c.name, k)


def test_layout_places_band_data_and_zeros():
    lay = bo.Layout(40, [(0, 2, "a"), (10, 13, "b"), (12, 15, "c"), (38, 45, "end")])
    assert lay.bands == [(0, 2), (10, 15), (38, 40)] and lay.nb == 9 and lay.gaps() == [(2, 10), (15, 38)]
    data = np.arange(1, 10, dtype=f32)[:, None] * np.ones((1, 3), f32)
    full = lay.host_rows(data, 0, 40)
    assert np.array_equal(np.flatnonzero(full[:, 0]), [0, 1, 10, 11, 12, 13, 14, 38, 39])
    assert np.array_equal(lay.host_rows(data, 11, 39), full[11:39]) and lay.blocks(8) == [0, 1, 4]


# ================================================================================================ the models
def test_pg_eval_is_the_closed_form_of_the_update_kernel_cases():
    heads, R = [21, 21], 600
    out, actions, adv, ret = uk.pg_inputs(heads, R)
    want_grad, want_sums = uk.pg_reference(out, actions, adv, ret, heads)
    grad, per_row = bo.pg_eval(out, actions, adv, ret, heads, 1.0 / R, f64)
    assert np.allclose(grad, want_grad, rtol=1e-13, atol=0) and np.allclose(bo.block_sums(per_row, 0, 256, f64), want_sums, rtol=1e-12)
    g32, p32 = bo.pg_eval(out, actions, adv, ret, heads, f32(1.0 / R), f32)
    assert g32.dtype == f32 and p32.dtype == f32 and 0 < np.abs(g32 - want_grad).max() < 1e-5 * np.abs(want_grad).max()


def test_mutations_are_the_identity_in_front_of_their_boundary_and_wrap_behind_it():
    o = np.array([0, 1023, 1024, 2047, 2048, 4095, 4096, 5000], np.int64)
    assert all(np.array_equal(bo.mutation(k, bo.SMALL)(o[o < bo.SMALL.e[b]])[0], o[o < bo.SMALL.e[b]]) for k, b in bo.MUTATIONS.items())
    assert list(bo.mutation("u32", bo.SMALL)(o)[0]) == [0, 1023, 1024, 2047, 2048, 4095, 0, 904]
    assert list(bo.mutation("s32", bo.SMALL)(o)[1]) == [True, True, True, True, False, False, True, True]
    assert list(bo.mutation("byte", bo.SMALL)(o)[0]) == [0, 1023, 0, 1023, 0, 1023, 0, 904]


# ================================================================================================ teeth, scaled boundaries
def _run(case, maps):
    store, results = case.standin(maps)
    return case.check(store, results)


@pytest.mark.parametrize("case", SMALL_CASES, ids=ids)
def test_correct_offsets_pass(case):
    v = _run(case, {})
    v.close()
    assert all(np.isfinite(r) for r in v.ratios.values()), v.ratios


@pytest.mark.parametrize("kind", sorted(bo.MUTATIONS))
@pytest.mark.parametrize("case", SMALL_CASES, ids=ids)
def test_a_planted_wrap_fails_the_case_wherever_the_tensor_crosses_the_boundary(case, kind):
    boundary = bo.MUTATIONS[kind]
    for tensor in case.widths:
        v = _run(case, {tensor: bo.mutation(kind, bo.SMALL)})
        if (tensor, boundary) in case.claims:
            assert v.failures, (case.name, tensor, kind, "the planted wrap went unnoticed")
            with pytest.raises(AssertionError):
                v.close()
        else:
            assert (case.name, tensor, boundary) in NOT_CROSSED
            v.close()


# ================================================================================================ the GPU file's store
@pytest.mark.parametrize("case", SMALL_CASES, ids=ids)
def test_the_device_store_counts_what_the_host_store_counts(case, monkeypatch):
    """`DeviceStore`, `_input` and `_output` of tests/test_gpu_big_offsets.py on the CPU device, in reduction steps of 97
    elements: the same sentinel and mismatch counts and the same rows as `HostStore`, on a correct and on a wrapped
    result, and the case's check reaches the same verdict through it"""
    import torch

    from tests import test_gpu_big_offsets as gpu

    monkeypatch.setattr(gpu, "DEV", torch.device("cpu"))
    monkeypatch.setattr(gpu, "CHUNK", 97)
    for maps in ({}, {list(case.widths)[-1]: bo.mutation("byte", bo.SMALL)}):
        host, results = case.standin(maps)
        dev = gpu.DeviceStore({name: torch.from_numpy(flat.a.copy()).view(-1, host.w[name]) for name, flat in host.t.items()})
        for name in host.t:
            pattern = host.rows(name, 1, 2)
            assert dev.sentinels(name) == host.sentinels(name)
            assert dev.mismatch_outside(name, case.layout.bands) == host.mismatch_outside(name, case.layout.bands)
            assert dev.mismatch_outside(name, case.layout.bands, pattern) == host.mismatch_outside(name, case.layout.bands, pattern)
            assert np.array_equal(uk.bits(dev.rows(name, 0, 3)), uk.bits(host.rows(name, 0, 3)))
        assert bool(case.check(dev, results).failures) == bool(maps)
    if not isinstance(case, bo.RecordCase):
        x = case.inputs()
        name = next(k for k in x if k in case.widths)
        assert np.array_equal(gpu._input(case.layout, x[name]).numpy(), case.layout.host_rows(x[name], 0, case.layout.R))
    assert bool((gpu._output(5, 3).view(torch.int32) == uk.SENTINEL_BITS).all()) and bool((gpu._output(5, 3, torch.int32) == uk.SENTINEL_BITS).all())
