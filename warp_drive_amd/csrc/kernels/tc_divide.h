// tc_divide.h -- division by a value that does not change during a launch, and the other per-launch constants of the
// multi-tick entry (tc_fast_rollout).  Part of the TagContinuous translation unit (tag_continuous.hip).
#pragma once
#include "wd_common.h"

namespace {

// x / y for a divisor y > 0 whose reciprocal r = RN(1 / y) was formed ONCE, by a true division: q0 = RN(x * r), the residual
// e = q0 * y - x (one FMA: exact while nothing underflows or overflows), q = RN(q0 - e * r).  Three instructions instead of the
// ~11 (float32) / ~17 (float64) of the correctly rounded division.  q equals RN(x / y) for most dividends but not for all of
// them, and which ones fail depends on y: HipTagContinuousVerifyInvariantDivide (tag_continuous.hip) compares this very
// function with the division for every float32 dividend, per divisor, and the multi-tick entry is offered only with that
// proof in hand (envs/tag_continuous.py::invariant_divide_ok).
// The residual is written q0 * y - x and NEGATED in the last FMA (a source modifier), not as x - q0 * y: for x = -0.0
// (`acceleration` is -0.0 whenever a negative value is multiplied by the "is moving" zero) q0 = -0, e = (-0) + (+0) = +0 and
// q = (-0) * r + (-0) = -0, as the division gives; the other way round e = +0 and q = (+0) + (-0) = +0.  For every other x
// the two forms compute the same values.
__device__ __forceinline__ float tc_div_const(float x, float y, float r) {
  const float q0 = x * r;
  const float e = __builtin_fmaf(q0, y, -x);
  return __builtin_fmaf(-e, r, q0);
}
__device__ __forceinline__ double tc_div_const(double x, double y, double r) {
  const double q0 = x * r;
  const double e = __builtin_fma(q0, y, -x);
  return __builtin_fma(-e, r, q0);
}

// The float32 dividends the form is USED for: zero, or 2^-65 <= |x| < 2^64.  Outside it fails for some divisors -- an infinite
// x gives inf - inf, a quotient that overflows likewise, and below 2^-104 the residual is subnormal and loses bits (0.7 and
// 2 pi fail there, 1.0 and 3.0 do not) -- so such a dividend (a state array somebody wrote by hand; none in a normal run)
// sends its wavefront to the true division (tc_move).  Three dividends share one test: the sum of the magnitudes is below
// 2^64 only if each is (NaN and inf fail the compare), and v_frexp_exp returns 0 for zero, so the smallest exponent says
// whether a NONZERO dividend is tiny.
__device__ __forceinline__ bool tc_div_const_in_class(float a, float b, float c) {
  const int lo = min(min(__builtin_amdgcn_frexp_expf(a), __builtin_amdgcn_frexp_expf(b)), __builtin_amdgcn_frexp_expf(c));
  const float sum = fabsf(a) + fabsf(b) + fabsf(c);
  return (sum < 0x1.0p64f) && (lo >= -64);
}

// what tc_fast_rollout's prologue forms once per launch from arguments the entry already has
struct TcLoopConsts {
  float r_sp;     // RN(1 / (max_speed + 1e-10f))
  double r_diag;  // RN(1 / (grid_length * sqrt 2)), float64
  double r_T;     // RN(1 / episode_length), float64
  float Bc;       // tags: a runner whose squared distance to every tagger is above this cannot be tagged (tc_tags.h)
};
#define WD_TC_TWO_PI 6.2831854820251465f           // float32(2 * pi)
#define WD_TC_R_TWO_PI (1.0f / WD_TC_TWO_PI)       // RN(1 / two_pi): folded by the compiler, correctly rounded
__device__ __forceinline__ float tc_sp_div(float max_speed) { return max_speed + 1.0e-10f; }
__device__ __forceinline__ double tc_diag(float grid_length) { return (double)grid_length * 1.4142135623730951; }
__device__ __forceinline__ TcLoopConsts tc_loop_consts(float max_speed, float grid_length, int T, float margin) {
  TcLoopConsts c;
  c.r_sp = 1.0f / tc_sp_div(max_speed);
  c.r_diag = 1.0 / tc_diag(grid_length);
  c.r_T = 1.0 / (double)T;
  // Bc = RN(margin^2) * (1 + 2^-20), rounded up (one ulp above the rounded product, which is at most half an ulp low).
  // RN(margin^2) >= margin^2 (1 - 2^-24), so t >= Bc means t > margin^2 (1 + 2^-21) and sqrt(t) > margin (1 + 2^-23):
  // the real root exceeds margin by more than half an ulp of margin (at most 2^-24 margin), hence sqrtf(t) >= margin
  // and `best < margin` is false.  (A subnormal square is off by at most 2^-150 absolutely: the ulp added covers it.
  // A square that is zero -- margin 0, or one so small that its square underflows -- stays 0: only t == 0, coincident
  // points, and NaN fail `t > 0`.  An infinite square gives NaN: nothing is above it, every wavefront takes the roots.)
  const float b = (margin * margin) * 0x1.00001p0f;
  c.Bc = (b > 0.0f) ? __uint_as_float(__float_as_uint(b) + 1u) : b;
  return c;
}

}  // namespace
