"""Rows, policies and references for the entries that show the in-kernel policy forward directly
(csrc/kernels/wd_test_kernels.hip::wd_test_policy_<form>_H<32|64>, the test-only code object): the logits, probabilities,
greedy action and running sums of rollout_policy.h's templates, one observation row per lane.  Shared by
tests/test_gpu_inkernel_policy_logits.py and tests/test_inkernel_policy_exact_host.py.  Nothing here touches a GPU.

Forms: "f4" rp_first_layer's float4 form (I = 4; the running sums from cp_policy_cum<H>), "f2o2" / "f2o6" its float2 form at
O = 2 / 6, "s21" rp_first_layer_strided<H, 21, 24>.  The float32 restatements are the project's
(tests/custom_rollout_model.py::policy_logits, tests/classic_control_policy.py, oracle/tag_gridworld_np.py at five actions);
the float64 reference is a plain matrix product; `exact_logits_row` redoes one row in exact rational arithmetic with one
correct rounding per fused multiply-add -- the only ground on which a logit mismatch may be put down to the double
rounding of the float64 emulation."""
from fractions import Fraction

import numpy as np

from tests import crafted_policies as cp

F32 = np.float32
FORMS = {"f4": "cartpole", "f2o2": "mountain_car", "f2o6": "acrobot", "s21": "gridworld"}   # form -> layout
WIDTHS = cp.WIDTHS
ACTIONS = (1, 2, 3, 5, 8)
ROWS, THREADS, MAXA = 70, 64, 8       # one wavefront and six lanes of a second block
ULP32 = 2.0 ** -24


def kernel_name(form, H):
    return f"wd_test_policy_{form}_H{H}"


def lds_bytes(form, n_weights):
    """the packed weights rounded up to four floats + one row of `stride` floats per lane"""
    stride = cp.LAYOUT[FORMS[form]][1]
    return 4 * (((n_weights + 3) & ~3) + THREADS * stride)


def rows(form):
    """[70, I] float32: 40 signed rows, 28 non-negative rows of multiples of 1 / 10 (TagGridWorld's inputs), an all-zero row
    and a row of -0.0"""
    I = cp.LAYOUT[FORMS[form]][0]
    rng = np.random.RandomState(17 + I)
    signed = (rng.standard_normal((40, I)) * 1.5).astype(F32)
    grid = (rng.randint(0, 11, size=(28, I)) / 10).astype(F32)
    out = np.ascontiguousarray(np.concatenate([signed, grid, np.zeros((1, I), F32), np.full((1, I), -0.0, F32)]), dtype=F32)
    assert out.shape == (ROWS, I)
    return out


def random_parts(env, H, A, seed):
    """random weights at O(1) scale (as tests/custom_contract_model.py): the logits spread over a few units and every
    softmax term counts"""
    rng = np.random.RandomState(100000 * seed + 1000 * cp.LAYOUT[env][0] + 10 * H + A)
    scale = {"W0": 0.5, "b0": 0.5, "W1": 0.3, "b1": 0.5, "Wp": 0.3, "bp": 0.5}
    return {k: (rng.standard_normal(v.shape) * scale[k]).astype(F32) for k, v in cp.blank(env, H, A).items()}


def policies(form, H, A):
    """{name: (parts, exact)}; exact: every softmax term is expf(0) or 0, so the probabilities and running sums are
    compared bit for bit"""
    env = FORMS[form]
    out = {f"random{seed}": (random_parts(env, H, A, seed), False) for seed in (1, 2, 3)}
    out["uniform"] = (cp.uniform(env, H, A), True)
    for name, winners in cp.constant_kinds(env, A).items():
        if max(winners) < A:
            out[name] = (cp.constant(env, H, winners, A), True)
    if A == cp.LAYOUT[env][2]:
        for f in (("tagger", "runner") if env == "gridworld" else (env,)):
            for sign in (1, -1):
                out[f"{f}{sign:+d}"] = (cp.switched(f, env, H, sign), True)
    return out


def non_finite_parts(form, H, A):
    """a NaN and a +inf planted in W1 of a random policy"""
    parts = random_parts(FORMS[form], H, A, 1)
    parts["W1"][0, 0] = np.nan
    parts["W1"][1, 1] = np.inf
    return parts


def _flat(parts):
    """the unpadded packed layout W0 [H][I], b0, W1, b1, Wp, bp the restatements read"""
    return np.concatenate([np.asarray(parts[k], F32).reshape(-1) for k in ("W0", "b0", "W1", "b1", "Wp", "bp")])


def restated(form, parts, obs):
    """(logits [R, A], probabilities [R, A], running sums [R, A], first maximum [R]) of the project's float32 restatements
    (the pad columns of the strided form are never read: its arithmetic is the unpadded one's)"""
    from tests import classic_control_evaluate as ev
    from tests import classic_control_policy as ccp
    from tests.custom_rollout_model import policy_logits

    H, A = parts["W0"].shape[0], parts["Wp"].shape[0]
    flat = _flat(parts)
    logits = policy_logits(flat, H, obs, A)
    probs = ccp.policy_probabilities(flat, H, obs, A)
    if form == "s21" and A == 5:
        from oracle.tag_gridworld_np import policy_probabilities

        theirs = policy_probabilities(cp.pack("gridworld", parts), H, obs)
        assert theirs.tobytes() == probs.tobytes()
    return logits, probs, ccp.running_sums(probs), ev.first_maximum(probs)


def reference_f64(parts, obs):
    """(logits, probabilities, running sums) in float64 from the float32 weights and rows"""
    p = {k: np.asarray(v, np.float64) for k, v in parts.items()}
    x = np.asarray(obs, np.float64)
    h1 = np.maximum(x @ p["W0"].T + p["b0"], 0)
    h2 = np.maximum(h1 @ p["W1"].T + p["b1"], 0)
    logits = h2 @ p["Wp"].T + p["bp"]
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    probs = e / e.sum(axis=1, keepdims=True)
    return logits, probs, np.cumsum(probs, axis=1)


def within_bound(got, f32_value, f64_value):
    """the project's bound (tests/test_gpu_core_exact.py::_ou_compare): the device's largest error against float64 is at
    most 4 x the float32 restatement's, with a floor of 8 float32 ulps of the largest compared value -> (ok, err, err32)"""
    err = float(np.abs(np.asarray(got, np.float64) - f64_value).max())
    err32 = float(np.abs(np.asarray(f32_value, np.float64) - f64_value).max())
    scale = float(np.abs(f64_value).max())
    return err <= max(4.0 * err32, 8.0 * ULP32 * scale), err, err32


# ------------------------------------------------------------------------------------------- exact rational arithmetic
def round_to_float32(q):
    """the float32 nearest to the rational q (ties to even; subnormals; no overflow expected)"""
    q = Fraction(q)
    if q == 0:
        return F32(0)
    sign, a = (-1 if q < 0 else 1), abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()   # 2^(e-1) < a < 2^(e+1)
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e - 23, -149)                                        # the unit of the last place
    m = a / Fraction(2) ** e
    n, rest = divmod(m.numerator, m.denominator)
    twice = 2 * rest
    if twice > m.denominator or (twice == m.denominator and n % 2):
        n += 1
    return F32(sign * float(n) * 2.0 ** e) if e >= -126 - 23 else F32(0)


def exact_logits_row(parts, x):
    """the logits of ONE row by the parity contract with every fused multiply-add computed exactly and rounded once"""
    def layer(v, W, b, relu):
        out = []
        for i in range(W.shape[0]):
            acc = F32(b[i])
            for j in range(W.shape[1]):
                acc = round_to_float32(Fraction(float(W[i, j])) * Fraction(float(v[j])) + Fraction(float(acc)))
            out.append(max(acc, F32(0)) if relu else acc)
        return np.array(out, F32)

    h1 = layer(np.asarray(x, F32), parts["W0"], parts["b0"], True)
    h2 = layer(h1, parts["W1"], parts["b1"], True)
    return layer(h2, parts["Wp"], parts["bp"], False)
