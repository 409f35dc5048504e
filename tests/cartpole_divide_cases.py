"""A host model of Cartpole's division shortcut and the divisors it is judged at: csrc/kernels/cartpole_common.h::
cp_div_invariant (q = RN(x * y), r = fma(-c, q, x), fma(r, y, q), y = RN(1 / c)), the dividend window of cp_euler<true>
(cp_div_in_window), the `fast` predicates of cartpole.hip / cartpole_pool.hip and the two-binade proof of
HipCartPoleVerifyInvariantDivide.  Shared by tests/test_cartpole_divide_cases_host.py (the model against rational
arithmetic, the table below against the model) and tests/test_gpu_cartpole_divide.py (the device against the table and
the model).  Nothing here touches a GPU.

THE ARITHMETIC.  `fma32` is a correctly rounded float32 fused multiply-add that keeps subnormals: the product of two
float32 is exact in float64, the sum p + c is formed in float64 together with its exact error (two-sum), and the sum is
ROUNDED TO ODD in float64 before the one rounding to float32 -- a float64 that is inexact and even moves one place
towards the error, so the later rounding to nearest sees on which side of every float32 midpoint (subnormal ones
included: 53 >= 24 + 2 bits) the exact value lies.  That is not the float64 detour `float32(float64(a) * b + c)`, which
rounds twice; `fma_rational` (exact fractions, one rounding to nearest even) is the yardstick of both in the host test.
The division itself is numpy's float32 `/` (IEEE: correctly rounded, subnormals kept).

THE CONSTANTS the device code tests are data here (WINDOW, FAST): the host test reads them back out of the kernel
sources, so the cases follow the code."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

F32 = np.float32
U32 = np.uint32

# cp_div_in_window (cartpole_common.h): ((bits & 0x7fffffff) - WINDOW_FIRST) < WINDOW_SPAN, unsigned
WINDOW_FIRST, WINDOW_SPAN = 0x12800000, 0x5a000000
WINDOW_LO_EXP, WINDOW_HI_EXP = (WINDOW_FIRST >> 23) - 127, ((WINDOW_FIRST + WINDOW_SPAN) >> 23) - 127   # [2^-90, 2^90)
# the `fast` predicates (cartpole.hip::cp_tick_impl, cartpole_pool.hip::cp_pool_rollout): bounds as powers of two,
# inclusive; "total_mass": None = no bound (the parent of the round that wrote this file)
FAST = {"masspole": (-60, 60), "total_mass": (-32, 32)}
FAST_PARENT = {"masspole": (-60, 60), "total_mass": None}
PROOF_BINADES = (0, 40)   # HipCartPoleVerifyInvariantDivide: [1, 2) and [2^40, 2^41), both signs
STRIDE = 257              # the table's sample of the window: every 257th magnitude pattern


# ------------------------------------------------------------------------------------------------ exact arithmetic
def round_to_f32(v):
    """Fraction -> float32, round to nearest even, subnormals kept, overflow to infinity"""
    v = Fraction(v)
    if v == 0:
        return F32(0.0)
    sign, m = (-1 if v < 0 else 1), abs(v)
    e = m.numerator.bit_length() - m.denominator.bit_length()
    if Fraction(2) ** e > m:
        e -= 1                       # 2^e <= m < 2^(e+1)
    quantum = Fraction(2) ** (max(e, -126) - 23)
    n, rem = divmod(m / quantum, 1)
    n = int(n)
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    out = n * quantum
    if out >= Fraction(2) ** 128:
        return F32(sign * np.inf)
    return F32(sign * float(out))    # (exact: 24 bits and a float64 exponent)


def fma_rational(a, b, c):
    """RN(a * b + c) of three finite float32 by exact fractions"""
    return round_to_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fma_double_rounding(a, b, c):
    """the float64 detour the model must NOT be: rounds to float64, then to float32"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
                + np.asarray(c, F32).astype(np.float64)).astype(F32)


def fma32(a, b, c):
    """RN(a * b + c) in float32, element-wise, one rounding (see the module's docstring); infinities and NaN as IEEE"""
    with np.errstate(all="ignore"):
        a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
        p = a * b                                  # exact
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)            # exact: s + err == p + c
        bits = np.atleast_1d(s).view(np.int64).copy()
        s1, err = np.atleast_1d(s), np.atleast_1d(err)
        fix = np.isfinite(s1) & (err != 0) & ((bits & 1) == 0)
        away = (err > 0) == (s1 > 0)               # the exact value lies beyond s: one place up in magnitude
        bits = np.where(fix, np.where(away, bits + 1, bits - 1), bits)
        out = bits.view(np.float64).astype(F32)
    return out.reshape(np.shape(s))


def div_invariant(x, c, y=None):
    """cp_div_invariant(x, c, y); y defaults to RN(1 / c) as the kernels form it"""
    x, c = np.asarray(x, F32), F32(c)
    with np.errstate(all="ignore"):
        y = F32(1.0) / c if y is None else F32(y)
        q = (x * y).astype(F32)
    r = fma32(-c, q, x)
    return fma32(r, y, q)


def div_invariant_rational(x, c):
    """the same three lines on scalars with fma_rational (finite intermediate values only)"""
    x, c = F32(x), F32(c)
    y = round_to_f32(Fraction(1) / Fraction(float(c)))
    q = round_to_f32(Fraction(float(x)) * Fraction(float(y)))
    r = fma_rational(-c, q, x)
    return fma_rational(r, y, q)


def mismatches(x, c, y=None):
    """bool per dividend: the shortcut's float32 differs from numpy's x / c (NaN against NaN is equal, NaN against
    infinity is not); also returns both results.  y: another reciprocal than RN(1 / c)"""
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        want = (x / F32(c)).astype(F32)
    got = div_invariant(x, c, y)
    bad = (got.view(U32) != want.view(U32)) & ~(np.isnan(got) & np.isnan(want))
    return bad, got, want


# ------------------------------------------------------------------------------------------------ window, predicate
def in_window(bits):
    """cp_div_in_window on float32 bit patterns"""
    bits = np.asarray(bits, U32)
    return ((bits & U32(0x7fffffff)) - U32(WINDOW_FIRST)).astype(U32) < U32(WINDOW_SPAN)


def window_count(first_pattern, n_patterns):
    """how many of the magnitude patterns first .. first + n - 1 (< 2^31), each with its negation, lie in the window --
    from the window's bounds alone"""
    lo, hi = max(first_pattern, WINDOW_FIRST), min(first_pattern + n_patterns, WINDOW_FIRST + WINDOW_SPAN)
    return 2 * max(0, hi - lo)


def _inside(value, bounds):
    return bounds is None or (F32(2.0) ** F32(bounds[0]) <= F32(value) <= F32(2.0) ** F32(bounds[1]))


def fast_predicate(masspole, total_mass, consts=None):
    """the mass part of the kernels' `fast` predicate (the proof flag, the angles and the pool are the launch's)"""
    consts = FAST if consts is None else consts
    return bool(_inside(masspole, consts["masspole"]) and _inside(total_mass, consts["total_mass"]))


# ------------------------------------------------------------------------------------------------ verdicts
def _patterns(lo_exp, hi_exp, stride):
    return np.arange((lo_exp + 127) << 23, (hi_exp + 127) << 23, stride, dtype=np.int64).astype(U32)


def verdict(c, lo_exp, hi_exp, stride=1):
    """mismatches against numpy's float32 division over the dividends |x| in [2^lo_exp, 2^hi_exp), every `stride`-th
    magnitude pattern, both signs"""
    total = 0
    for e in range(lo_exp, hi_exp):
        total += int(binade_mismatches(c, e, stride))
    return total


def binade_mismatches(c, e, stride=1, y=None):
    """the same count for the one binade [2^e, 2^(e+1)) (in cache-sized pieces, on a few threads: numpy drops the lock)"""
    m = _patterns(e, e + 1, stride)
    jobs = [(piece | U32(s)).view(F32) for piece in np.array_split(m, max(1, len(m) >> 17)) for s in (0, 0x80000000)]
    count = lambda x: int(mismatches(x, c, y)[0].sum())   # noqa: E731
    if len(jobs) < 8:
        return sum(count(x) for x in jobs)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        return sum(pool.map(count, jobs))


@functools.lru_cache(maxsize=None)
def proof_passes(c):
    """what HipCartPoleVerifyInvariantDivide computes for (c, RN(1 / c)): no mismatch in the two proof binades"""
    return all(binade_mismatches(F32(c), e) == 0 for e in PROOF_BINADES)


@functools.lru_cache(maxsize=None)
def window_scan(c, stride=STRIDE):
    """(first failing binade, last failing binade, mismatches) over the window at `stride`; (None, None, 0) when clean"""
    counts = {e: binade_mismatches(F32(c), e, stride) for e in range(WINDOW_LO_EXP, WINDOW_HI_EXP)}
    bad = [e for e, n in counts.items() if n]
    return (bad[0], bad[-1], sum(counts.values())) if bad else (None, None, 0)


def first_mismatch(c, e):
    """(x bits, shortcut bits, division bits) of the first positive dividend of binade e that fails, or None"""
    m = _patterns(e, e + 1, 1)
    bad, got, want = mismatches(m.view(F32), c)
    i = np.flatnonzero(bad)
    return None if not len(i) else (int(m[i[0]]), int(got.view(U32)[i[0]]), int(want.view(U32)[i[0]]))


# ------------------------------------------------------------------------------------------------ the named divisors
class Divisor:
    """A total mass as the env forms it: float32(masspole + masscart), the sum in float64 (envs/cartpole.py).  The rest
    is the TABLE, pinned by the host test against the model: proof = the two-binade proof passes; first / last = the
    failing binades inside the window at STRIDE (None: clean); binade = one failing binade and its exhaustive mismatch
    count, both signs (what the device must count there); witness = (x, shortcut, division) bits at that binade."""

    def __init__(self, name, masspole, masscart, c_bits, proof, first=None, last=None, binade=None, count=0, witness=None):
        self.name, self.masspole, self.masscart = name, float(masspole), float(masscart)
        self.c = F32(self.masspole + self.masscart)
        assert int(self.c.view(U32)) == c_bits, (name, hex(int(self.c.view(U32))))
        self.proof, self.first, self.last, self.binade, self.count, self.witness = proof, first, last, binade, count, witness

    @property
    def clean(self):
        return self.first is None

    def physics(self, **more):
        return dict(masspole=self.masspole, masscart=self.masscart, **more)

    def __repr__(self):
        return self.name


SQRT3 = float(F32(1.7320508))

# Every divisor passes the two-binade proof; what happens inside the window differs.  OVERFLOW SIDE: q = RN(x * y) is
# infinite, r = -inf, the result inf - inf = NaN, where the division gives infinity -- or, at the edge (1.75 * 2^-39,
# x = 0x6c5fffff), the largest finite float32.  UNDERFLOW SIDE: the quotient is subnormal, q is rounded at the subnormal
# quantum, r * y is far below it and the last fused multiply-add returns q: off by one place wherever q rounded the other
# way than the exact quotient does.  `first` / `last` are EXHAUSTIVE (every dividend of the binades at and next to them);
# a sample of every 257th pattern sees 1.25 * 2^60 fail from 2^-82 on and 1.5 * 2^126 from 2^-15 on, the sparse failures
# below (2 .. 52 per binade) only a full sweep finds.
DIVISORS = [
    Divisor("classic-1.1", 0.1, 1.0, 0x3f8ccccd, proof=True),
    Divisor("masspole-0.25", 0.25, 1.0, 0x3fa00000, proof=True),
    Divisor("masscart-2^20", 0.1, 2.0 ** 20, 0x49800001, proof=True),
    Divisor("band-low-edge-2^-32", 2.0 ** -33, 2.0 ** -33, 0x2f800000, proof=True),
    Divisor("band-high-edge-2^32", 1.0, 2.0 ** 32 - 1.0, 0x4f800000, proof=True),
    Divisor("sqrt3*2^-60", 2.0 ** -60, (SQRT3 - 1.0) * 2.0 ** -60, 0x21ddb3d7, proof=True, first=68, last=89,
            binade=68, count=4495440, witness=(0x61ddb3d8, 0xffc00000, 0x7f800000)),
    Divisor("1.75*2^-39", 2.0 ** -40, 2.5 * 2.0 ** -40, 0x2c600000, proof=True, first=89, last=89,
            binade=89, count=4194306, witness=(0x6c5fffff, 0xffc00000, 0x7f7fffff)),
    Divisor("1.25*2^39", 1.0, 1.25 * 2.0 ** 39 - 1.0, 0x53200000, proof=True, first=-90, last=-90,
            binade=-90, count=838862, witness=(0x12800007, 0x000ccccd, 0x000cccce)),
    Divisor("1.25*2^60", 2.0 ** 60, 0.25 * 2.0 ** 60, 0x5da00000, proof=True, first=-89, last=-69,
            binade=-69, count=838862, witness=(0x1d000007, 0x000ccccd, 0x000cccce)),
    Divisor("1.5*2^126", 1.0, 1.5 * 2.0 ** 126, 0x7ec00000, proof=True, first=-22, last=-2,
            binade=-2, count=1398102, witness=(0x3e800001, 0x00155555, 0x00155556)),
]
BY_NAME = {d.name: d for d in DIVISORS}

# ------------------------------------------------------------------------------------------------ the rollouts
# OVERFLOW: total mass sqrt3 * 2^-60 with the smallest pole the guard admits and a force of 2^70 -- inside the window, in
# a failing binade (68 .. 89), and so large that the centrifugal term vanishes in it: every tick's force dividend is
# +-2^70 exactly, the quotient overflows, the oracle records +-inf in the two velocities and the shortcut NaN.
# IN BAND: a cart of 2^20 -- off every mass the suite ran so far, and fast ticks all the same.
OVERFLOW_PHYSICS = BY_NAME["sqrt3*2^-60"].physics(force_mag=2.0 ** 70)
IN_BAND_PHYSICS = BY_NAME["masscart-2^20"].physics()
ROLLOUT_E, ROLLOUT_TICKS, ROLLOUT_LAUNCHES = 1500, 16, 3
