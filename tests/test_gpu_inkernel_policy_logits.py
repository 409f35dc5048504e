"""The arithmetic of the in-kernel policy forward seen directly on the MI355X: wd_test_policy_<form>_H<32|64> of the
test-only code object (csrc/kernels/wd_test_kernels.hip) store, for 70 observation rows, the eight logits, probabilities and
running sums and the greedy action that csrc/kernels/rollout_policy.h's templates and cartpole_common.h::cp_policy_cum
produce -- rp_first_layer in its float4 form and in its float2 form at O = 2 and O = 6, rp_first_layer_strided<H, 21, 24>,
rp_policy_logits, rp_softmax_probs, rp_first_maximum -- at 1, 2, 3, 5 and 8 actions, the packed weights staged in LDS as the
units stage them.  Logits: bit for bit against the float32 restatement, for the crafted kinds and three random policies
(a mismatch is redone in exact rational arithmetic before it may be put down to the float64 emulation's double rounding);
-inf past the action count.  Probabilities and running sums: bit for bit for the crafted kinds; for random policies within
the project's bound |device - f64| <= max(4 |f32 restatement - f64|, 8 * 2^-24 * scale).  `pytest -s` prints the largest
deviations per form."""
import numpy as np
import pytest
import torch

from tests import crafted_policies as cp
from tests import inkernel_policy_logit_cases as lc

pytestmark = pytest.mark.gpu

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


class _Entry:
    def __init__(self, form, H):
        from tests.hip_harness import require_gpu
        from warp_drive_amd.managers import hip_driver as drv

        require_gpu()
        self.form, self.H, self.env = form, H, lc.FORMS[form]
        self.fn = drv.Module(drv.code_object_of(lc.kernel_name(form, H))).get_function(lc.kernel_name(form, H))
        self.obs_np = lc.rows(form)
        self.obs = torch.from_numpy(self.obs_np).cuda()
        R = lc.ROWS
        self.out = [torch.empty((R + 2, lc.MAXA), dtype=torch.float32, device="cuda") for _ in range(3)]
        self.best = torch.empty(R + 2, dtype=torch.int32, device="cuda")

    def run(self, parts, n_weights=None, n_actions=None):
        """-> (logits, probabilities, running sums [70, 8], first maximum [70]); the two rows behind the last keep their
        sentinels"""
        packed_np = cp.pack(self.env, parts)
        packed = torch.from_numpy(packed_np).cuda()
        A = parts["Wp"].shape[0] if n_actions is None else n_actions
        stride, H = cp.LAYOUT[self.env][1], self.H
        n_w = stride * H + H + H * H + H + parts["Wp"].shape[0] * H + parts["Wp"].shape[0]   # (without TagGridWorld's padding)
        n_w = n_w if n_weights is None else n_weights
        assert n_w <= len(packed_np)
        for t in self.out:
            t.fill_(-7.5)
        self.best.fill_(-77)
        blocks = -(-lc.ROWS // lc.THREADS)
        self.fn(packed, np.int32(n_w), self.obs, np.int32(lc.ROWS), np.int32(A), *self.out, self.best,
                block=(lc.THREADS, 1, 1), grid=(blocks, 1), shared=lc.lds_bytes(self.form, len(packed_np)))
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in self.out] + [self.best.cpu().numpy()]
        return got


@pytest.mark.parametrize("H", lc.WIDTHS)
@pytest.mark.parametrize("form", sorted(lc.FORMS))
def test_logits_probabilities_and_running_sums(form, H):
    entry = _Entry(form, H)
    obs, R = entry.obs_np, lc.ROWS
    worst = {"logit": 0.0, "prob": 0.0, "cum": 0.0}
    compared = redone = 0
    for A in lc.ACTIONS:
        for name, (parts, exact) in lc.policies(form, H, A).items():
            tag = f"{form} H{H} A{A} {name}"
            logits, probs, cums, best = entry.run(parts)
            for arr, sent in ((logits, -7.5), (probs, -7.5), (cums, -7.5)):
                assert (arr[R:] == sent).all(), (tag, "a row behind the last was written")
            assert (best[R:] == -77).all(), tag
            want_l, want_p, want_c, want_b = lc.restated(form, parts, obs)
            # ---- the logits, bit for bit; past A: -inf
            bad = np.argwhere(_bits(logits[:R, :A]) != _bits(want_l))
            redone += len(bad)
            for r, a in bad:   # only the float64 emulation's double rounding may differ: redo the row exactly
                exact_row = lc.exact_logits_row(parts, obs[r])
                assert _bits(logits[r, :A]).tolist() == _bits(exact_row).tolist(), (tag, int(r), int(a), logits[r, :A], want_l[r])
            assert np.isneginf(logits[:R, A:]).all() and (probs[:R, A:] == 0).all(), tag
            assert (best[:R] == want_b).all() and best[:R].min() >= 0 and best[:R].max() < A, tag
            l64, p64, c64 = lc.reference_f64(parts, obs)
            if exact:
                assert (_bits(probs[:R, :A]) == _bits(want_p)).all(), (tag, "probabilities")
                if form == "f4":
                    assert (_bits(cums[:R, :A]) == _bits(want_c)).all(), (tag, "running sums")
            else:
                ok, err, err32 = lc.within_bound(probs[:R, :A], want_p, p64)
                assert ok, (tag, "probabilities", err, err32)
                worst["prob"] = max(worst["prob"], err)
                worst["logit"] = max(worst["logit"], float(np.abs(logits[:R, :A].astype(np.float64) - l64).max()))
                if form == "f4":
                    ok, err, err32 = lc.within_bound(cums[:R, :A], want_c, c64)
                    assert ok, (tag, "running sums", err, err32)
                    worst["cum"] = max(worst["cum"], err)
            if form == "f4":   # the last running sum repeated up to the bound
                assert (_bits(cums[:R, A:]) == _bits(cums[:R, A - 1:A])).all(), tag
            else:
                assert (cums[:R] == -1.0).all(), tag
            compared += 1
    print(f"{lc.kernel_name(form, H)}: {compared} policies x {R} rows, {redone} logits redone in rational arithmetic; "
          f"random policies, largest deviation from float64: logits {worst['logit']:.3e}, probabilities {worst['prob']:.3e}"
          + (f", running sums {worst['cum']:.3e}" if form == "f4" else ""))


@pytest.mark.parametrize("H", lc.WIDTHS)
@pytest.mark.parametrize("form", sorted(lc.FORMS))
def test_non_finite_weights_and_the_guard(form, H):
    """a NaN and a +inf in W1: fmaxf(NaN, 0) is 0 on the device, which the numpy models do not restate, and the +inf goes
    through wherever its input unit is positive -- the result is printed and only the greedy action's range is asserted.
    Nine actions, no actions, or a weight count of another shape: the entry writes nothing."""
    entry = _Entry(form, H)
    R = lc.ROWS
    for A in (2, 5):
        logits, probs, cums, best = entry.run(lc.non_finite_parts(form, H, A))
        assert best[:R].min() >= 0 and best[:R].max() < A
        print(f"{lc.kernel_name(form, H)} A{A}, NaN and +inf in W1: {int(np.isfinite(logits[:R, :A]).all(axis=1).sum())} of {R} "
              f"rows with finite logits, {int(np.isnan(probs[:R, :A]).any(axis=1).sum())} with a NaN probability, greedy "
              f"actions {np.bincount(best[:R], minlength=A).tolist()}")
    parts = lc.random_parts(entry.env, H, 8, 1)
    full = sum(v.size for v in parts.values()) + (cp.LAYOUT[entry.env][1] - cp.LAYOUT[entry.env][0]) * H
    for n_weights, n_actions in ((full, 9), (full, 0), (full - 1, 8)):
        logits, probs, cums, best = entry.run(parts, n_weights=n_weights, n_actions=n_actions)
        assert (logits == -7.5).all() and (probs == -7.5).all() and (cums == -7.5).all() and (best == -77).all()
