"""tests/cartpole_divide_cases.py on the host alone: the fused multiply-add of the model against exact fractions (and NOT
the float64 detour), the window and the `fast` predicate's constants against the kernel sources, and every line of the
divisor table against the model.  No GPU; `pytest -s` prints one line per divisor."""
import os
import re

import numpy as np
import pytest

from tests import cartpole_divide_cases as cd

F32, U32 = np.float32, np.uint32


def _f(bits):
    return np.array([bits], U32).view(F32)[0]


def _bits(v):
    return int(np.asarray(v, F32).reshape(-1).view(U32)[0])


# ------------------------------------------------------------------------------------------------ the arithmetic
def test_fma_is_rounded_once_and_the_float64_detour_is_not():
    """(1 + 2^-23)(1 - 2^-23) + (2^24 + 2) = 2^24 + 3 - 2^-46: just below the midpoint of 2^24 + 2 and 2^24 + 4, so one
    rounding gives 2^24 + 2; float64 cannot hold the 2^-46 (70 bits), lands ON the midpoint and the second rounding goes
    to the even neighbour 2^24 + 4"""
    a, b, c = F32(1 + 2.0 ** -23), F32(1 - 2.0 ** -23), F32(2.0 ** 24 + 2)
    assert float(cd.fma_rational(a, b, c)) == 2.0 ** 24 + 2
    assert float(cd.fma32(a, b, c)) == 2.0 ** 24 + 2
    assert float(cd.fma_double_rounding(a, b, c)) == 2.0 ** 24 + 4
    # a subnormal result, the product half a quantum less 2^-46 of it: (2.5 - 2^-47) * 2^-149 stays 2 quanta
    a, b, c = F32((1 + 2.0 ** -23) * 2.0 ** -100), F32((1 - 2.0 ** -23) * 2.0 ** -50), F32(2.0 ** -148)
    assert _bits(cd.fma_rational(a, b, c)) == 2 and _bits(cd.fma32(a, b, c)) == 2
    h, g = F32(2.0 ** -100), F32(2.0 ** -50)   # exactly half a quantum: ties go to the even neighbour
    assert _bits(cd.fma32(h, g, c)) == 2 and _bits(cd.fma32(h, g, F32(3 * 2.0 ** -149))) == 4
    assert _bits(cd.fma32(a, g, c)) == 3       # half a quantum and 2^-24 of one: up


def test_fma_against_exact_fractions():
    """random bit patterns (all exponents: subnormal inputs and results, overflow to infinity), triples built to cancel,
    and triples at the subnormal quantum"""
    rng = np.random.RandomState(7)
    v = rng.randint(0, 2 ** 32, size=(3, 3000), dtype=np.uint64).astype(U32).view(F32)
    a, b = v[0], v[1]
    with np.errstate(all="ignore"):
        cancel = (-(a * b)).astype(F32)                      # c = -RN(a * b): the sum is the product's rounding error
    tiny_a = (rng.randint(0, 1 << 24, size=3000).astype(U32) | U32(0x0c000000)).view(F32)   # ~2^-103
    tiny_b = (rng.randint(0, 1 << 24, size=3000).astype(U32) | U32(0x2a000000)).view(F32)   # ~2^-43: products ~2^-146
    tiny_c = rng.randint(0, 1 << 12, size=3000).astype(U32).view(F32)                        # subnormal addends
    checked = subnormal = infinite = 0
    for A, B, C in ((a, b, v[2]), (a, b, cancel), (tiny_a, tiny_b, tiny_c)):
        got = cd.fma32(A, B, C)
        for i in np.flatnonzero(np.isfinite(A) & np.isfinite(B) & np.isfinite(C)):
            want = cd.fma_rational(A[i], B[i], C[i])
            assert _bits(got[i]) == _bits(want) or (got[i] == 0 and want == 0), (hex(_bits(A[i])), hex(_bits(B[i])), hex(_bits(C[i])))
            checked += 1
            subnormal += int(0 < abs(float(want)) < 2.0 ** -126)
            infinite += int(np.isinf(want))
    assert checked > 8000 and subnormal > 2000 and infinite > 100, (checked, subnormal, infinite)


def test_shortcut_model_against_exact_fractions():
    """div_invariant (vectors, fma32) == the same three lines in fractions, at every witness of the table and around it"""
    n = 0
    for d in cd.DIVISORS:
        xs = [0x3f800000, 0x3fffffff, 0x12800000, 0x6cffffff]
        if d.witness:
            xs += [d.witness[0] + k for k in range(-3, 4)]
        for xb in xs:
            for s in (0, 0x80000000):
                x = _f(xb | s)
                got = cd.div_invariant(np.array([x], F32), d.c)[0]
                with np.errstate(all="ignore"):
                    q = F32(x * (F32(1.0) / d.c))
                if not np.isfinite(q):
                    assert np.isnan(got), (d, hex(xb))      # q = inf -> r = -inf -> inf - inf
                    continue
                assert _bits(got) == _bits(cd.div_invariant_rational(x, d.c)), (d, hex(xb))
                n += 1
    assert n > 100


# ------------------------------------------------------------------------------------------------ the constants
def _source(name):
    from warp_drive_amd import build as wd_build

    return open(os.path.join(wd_build.KDIR, name)).read()


def test_window_and_predicate_constants_are_the_sources():
    """cp_div_in_window and cp_fast_masses_ok are one text each, in cartpole_common.h, with the model's constants; both
    `fast` predicates and cp_euler<true> / the test entry call them"""
    header = _source("cartpole_common.h")
    m = re.search(r"bool cp_div_in_window\(float x\) \{\s*return \(\(__float_as_uint\(x\) & 0x7fffffffu\) - (0x[0-9a-f]+)u\) < (0x[0-9a-f]+)u;", header)
    assert m and (int(m.group(1), 16), int(m.group(2), 16)) == (cd.WINDOW_FIRST, cd.WINDOW_SPAN)
    assert (cd.WINDOW_LO_EXP, cd.WINDOW_HI_EXP) == (-90, 90)
    assert len(re.findall(r"0x12800000u", header)) == 1 and header.count("cp_div_in_window(temp_num)") == 1
    m = re.search(r"bool cp_fast_masses_ok\(float masspole, float total_mass\) \{\s*return \(masspole >= 0x1\.0p(-?\d+)f\) && "
                  r"\(masspole <= 0x1\.0p(-?\d+)f\) && \(total_mass >= 0x1\.0p(-?\d+)f\) && \(total_mass <= 0x1\.0p(-?\d+)f\);", header)
    assert m, "cp_fast_masses_ok changed its form: restate cartpole_divide_cases.FAST"
    lo, hi, tlo, thi = (int(g) for g in m.groups())
    assert {"masspole": (lo, hi), "total_mass": (tlo, thi)} == cd.FAST
    for unit in ("cartpole.hip", "cartpole_pool.hip"):
        text = _source(unit)
        assert text.count("cp_fast_masses_ok(p.masspole, p.total_mass)") == 1 and "0x1.0p-60f" not in text, unit
    assert "cp_div_in_window(x)" in _source("wd_test_kernels.hip")


def test_window_layout_a_pattern_and_its_negation():
    """the device entry walks MAGNITUDE patterns and tests each with its negation: the count inside the window follows
    from the bounds (window_count) and equals the bit test's own on a sample that includes every edge"""
    assert cd.window_count(0, 1 << 31) == 2 * cd.WINDOW_SPAN == 3019898880
    assert cd.window_count(cd.WINDOW_FIRST, cd.WINDOW_SPAN) == 2 * cd.WINDOW_SPAN
    assert cd.window_count((68 + 127) << 23, 1 << 23) == 1 << 24 and cd.window_count((90 + 127) << 23, 1 << 23) == 0
    edges = [0, 1, 0x007fffff, 0x00800000, cd.WINDOW_FIRST - 1, cd.WINDOW_FIRST, cd.WINDOW_FIRST + cd.WINDOW_SPAN - 1,
             cd.WINDOW_FIRST + cd.WINDOW_SPAN, 0x7f7fffff, 0x7f800000, 0x7fc00000, 0x7fffffff]
    want = [False, False, False, False, False, True, True, False, False, False, False, False]
    for sign in (0, 0x80000000):
        assert cd.in_window(np.array(edges, U32) | U32(sign)).tolist() == want
    assert _f(cd.WINDOW_FIRST) == F32(2.0 ** -90) and _f(cd.WINDOW_FIRST + cd.WINDOW_SPAN) == F32(2.0 ** 90)
    first, n = cd.WINDOW_FIRST - 5000, cd.WINDOW_SPAN + 12345
    pats = np.arange(first, first + n, 997, dtype=np.int64).astype(U32)
    inside = int(cd.in_window(pats).sum() + cd.in_window(pats | U32(0x80000000)).sum())
    assert inside == 2 * int(((pats >= cd.WINDOW_FIRST) & (pats < cd.WINDOW_FIRST + cd.WINDOW_SPAN)).sum()) > 0
    assert cd.window_count(first, n) == 2 * cd.WINDOW_SPAN and cd.window_count(first, 5001) == 2


# ------------------------------------------------------------------------------------------------ the table
def test_the_named_divisors_are_the_ones_asked_for():
    by = cd.BY_NAME
    assert by["classic-1.1"].c == F32(1.1) and by["masspole-0.25"].c == F32(1.25)
    assert by["sqrt3*2^-60"].c == F32(F32(1.7320508) * F32(2.0 ** -60))
    assert F32(2.0 ** -39) <= by["1.75*2^-39"].c < F32(2.0 ** -38)
    assert by["1.25*2^39"].c == F32(1.25 * 2.0 ** 39) and by["1.25*2^60"].c == F32(1.25 * 2.0 ** 60)
    assert by["1.5*2^126"].c >= F32(2.0 ** 126) and 0 < float(F32(1.0) / by["1.5*2^126"].c) < 2.0 ** -126
    for d in cd.DIVISORS:   # the pole's mass is inside the guard: the mass predicate turns on the total mass alone
        assert cd.fast_predicate(d.masspole, 1.0) and cd.fast_predicate(d.masspole, d.c, cd.FAST_PARENT), d


@pytest.mark.parametrize("d", cd.DIVISORS, ids=repr)
def test_table_line_against_the_model(d):
    """proof verdict; first and last failing binade (exhaustive at both and at the binades next to them, the 257-stride
    scan of the whole window inside them); the binade count and the witness's bits"""
    assert cd.proof_passes(d.c) == d.proof
    first, last, sampled = cd.window_scan(d.c)
    lo, hi = cd.WINDOW_LO_EXP, cd.WINDOW_HI_EXP - 1
    if d.clean:
        assert (first, last, sampled) == (None, None, 0)
        assert cd.binade_mismatches(d.c, lo) == 0 and cd.binade_mismatches(d.c, hi) == 0   # the window's own edges, in full
        assert d.binade is None and d.count == 0 and d.witness is None
        print(f"{d.name}: c = {float(d.c).hex()}, proof passes, clean at stride {cd.STRIDE} and in binades {lo}, {hi} in full")
        return
    assert lo <= d.first <= first and last <= d.last <= hi and sampled > 0
    counts = {e: cd.binade_mismatches(d.c, e) for e in {d.first - 1, d.first, d.last, d.last + 1, d.binade} if lo <= e <= hi}
    assert counts[d.first] > 0 and counts[d.last] > 0 and counts.get(d.first - 1, 0) == 0 and counts.get(d.last + 1, 0) == 0
    assert counts[d.binade] == d.count and d.first <= d.binade <= d.last
    assert cd.verdict(d.c, d.binade - 1, d.binade + 2, 4099) == sum(cd.binade_mismatches(d.c, e, 4099) for e in range(d.binade - 1, d.binade + 2)) > 0
    assert cd.first_mismatch(d.c, d.binade) == d.witness
    x, got, want = (_f(b) for b in d.witness)
    with np.errstate(all="ignore"):
        assert _bits(x / d.c) == d.witness[2]
    if np.isfinite(got):
        assert _bits(cd.div_invariant_rational(x, d.c)) == d.witness[1] and abs(d.witness[1] - d.witness[2]) == 1
    else:
        assert np.isnan(got) and not np.isnan(want)
    print(f"{d.name}: c = {float(d.c).hex()}, proof passes, fails in binades {d.first} .. {d.last} (stride {cd.STRIDE} sees "
          f"{first} .. {last}, {sampled} mismatches); binade {d.binade}: {d.count}; x = {d.witness[0]:#010x}: shortcut "
          f"{d.witness[1]:#010x}, division {d.witness[2]:#010x}")


def test_fast_predicate_admits_no_failing_divisor():
    """with the shipping constants: fast => clean for every named divisor, the in-band ones stay fast, and the band's two
    edges are the last divisors admitted; with the parent's constants every failing divisor was admitted"""
    for d in cd.DIVISORS:
        assert not cd.fast_predicate(d.masspole, d.c) or d.clean, d
        assert cd.fast_predicate(d.masspole, d.c, cd.FAST_PARENT)
    for name in ("classic-1.1", "masspole-0.25", "masscart-2^20", "band-low-edge-2^-32", "band-high-edge-2^32"):
        assert cd.fast_predicate(cd.BY_NAME[name].masspole, cd.BY_NAME[name].c), name
    assert sum(not d.clean for d in cd.DIVISORS) == 5
    lo, hi = cd.BY_NAME["band-low-edge-2^-32"].c, cd.BY_NAME["band-high-edge-2^32"].c
    assert not cd.fast_predicate(1.0, np.nextafter(lo, F32(0))) and not cd.fast_predicate(1.0, np.nextafter(hi, F32(np.inf)))
    assert not cd.fast_predicate(2.0 ** -61, 1.0) and not cd.fast_predicate(2.0 ** 61, 1.0)
    # the band's reason: every quotient of a window dividend by a divisor of the band is a normal float32, with room
    t = cd.FAST["total_mass"]
    assert cd.WINDOW_LO_EXP - t[1] >= -126 + 4 and cd.WINDOW_HI_EXP - t[0] <= 127 - 4


# ------------------------------------------------------------------------------------------------ the rollouts' premise
def test_overflow_rollout_premise():
    """the overflow physics on the host: the oracle runs, its first tick records +-inf in both velocities, every force
    dividend is +-2^70 exactly (a failing binade of the table, inside the window) and the shortcut turns it into NaN -- a
    recorded word the oracle does not hold.  The in-band physics: finite, fast, clean."""
    from oracle.cartpole_np import CartPoleOracle

    d, ph = cd.BY_NAME["sqrt3*2^-60"], cd.OVERFLOW_PHYSICS
    assert ph["masspole"] >= 2.0 ** -60 and F32(ph["masspole"] + ph["masscart"]) == d.c
    force = F32(ph["force_mag"])
    assert d.first <= 70 <= d.last and bool(cd.in_window(force.view(U32))) and cd.fast_predicate(ph["masspole"], d.c, cd.FAST_PARENT)
    assert not cd.fast_predicate(ph["masspole"], d.c)
    start = np.array([0.03, -0.02, 0.04, 0.01], F32)
    orc = type("Oracle", (CartPoleOracle,), ph)(2, 23, initial_state=start)
    with np.errstate(all="ignore"):
        orc.step(np.array([0, 1]))
        pml = F32(ph["masspole"] * 0.5)
        temp_num = (np.array([-force, force], F32) + F32(F32(pml * F32(start[3] * start[3])) * np.sin(start[2]))).astype(F32)
        want = temp_num / d.c
    assert temp_num.tolist() == [-float(force), float(force)]
    got = cd.div_invariant(temp_num, d.c)
    assert np.isinf(want).all() and np.isnan(got).all()
    assert orc.state[:, 1].tolist() == [-np.inf, np.inf] and orc.state[:, 3].tolist() == [np.inf, -np.inf]
    assert np.isfinite(orc.state[:, [0, 2]]).all() and (orc.done == 0).all()
    with np.errstate(all="ignore"):
        orc.step(np.array([1, 0]))
    assert (orc.done == 1).all()                       # the cart is at +-inf: the episode ends, the replica restarts
    e = cd.BY_NAME["masscart-2^20"]
    assert cd.fast_predicate(e.masspole, e.c) and e.clean and cd.IN_BAND_PHYSICS["masscart"] == 2.0 ** 20


# ------------------------------------------------------------------------------------------------ the launch builder
@pytest.mark.parametrize("ticks", [0, -1])
def test_tick_launch_refuses_a_launch_of_no_ticks(ticks):
    """cp_tick_impl runs its last tick whatever `ticks` says: the host refuses before anything is initialised or launched"""
    import types

    from tests.test_cartpole_pool_rollout_host import _fake_env, _launch_inputs, _manifest
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    E = 300
    env = _fake_env(E, _manifest(), pool=0)
    probs, batch, _ = _launch_inputs(E, 4, 2, 0)
    sampler = types.SimpleNamespace(rng_state="rng")
    env.ticks_per_launch = ticks
    for kw in ({}, {"batch": batch}):
        with pytest.raises(UnsupportedRolloutShape, match="ticks_per_launch"):
            env.tick_launch(sampler, [probs], env.cuda_env_resetter, **kw)
    assert env.cuda_function_manager.initialized == []
    env.ticks_per_launch = 1
    fn, args, _, _, _ = env.tick_launch(sampler, [probs], env.cuda_env_resetter)
    assert fn.name == "HipClassicControlCartPoleEnvTick" and int(args[-1]) == 1
