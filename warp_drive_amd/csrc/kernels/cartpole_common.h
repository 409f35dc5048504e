// cartpole_common.h -- what the two Cartpole code paths share: the Euler step (cp_euler), the in-kernel policy's running
// sums (cp_policy_cum, around rollout_policy.h) and the untracked stores through a scalar base.  Included by cartpole.hip
// (the main code object: Step, Tick, Rollout_H<H>, Evaluate_H<H>, the two Verify entries) and by cartpole_pool.hip
// (wd_kernels_cp_pool.hsaco: the T-tick rollout whose finished replicas restart from a reset pool).  A change here
// changes both objects: compare the main object's disassembly as profiles/r26_cartpole_asm_diff.txt did.
#pragma once
#include "wd_common.h"
#include "rollout_policy.h"

namespace {

struct CpPhysics {
  float gravity, masspole, total_mass, length, polemass_length, force_mag, tau;
  float theta_threshold_radians, x_threshold;
  float inv_total_mass;  // RN(1 / total_mass) (correctly rounded: -fhip-fp32-correctly-rounded-divide-sqrt)
};

// x / c for a divisor that is the same on every tick of every replica (the total mass): q = RN(x * y), r = x - c * q
// (exact: one FMA), RN(q + r * y), y = RN(1 / c) -- three instructions instead of the ~10 of the correctly rounded division.
// WHAT IS PROVED, per divisor: HipCartPoleVerifyInvariantDivide compares this form with `/` for the 2^24 significands of the
// binade [1, 2) (and of [2^40, 2^41)), both signs, once per total mass (no float32 divisor tried so far fails it; the
// classical guarantee has exceptions, and an exhaustive check costs one launch).  Scaling x by a power of two scales q, r
// and the result exactly AS LONG AS q AND THE QUOTIENT STAY NORMAL float32 -- then, and only then, one binade speaks for
// the others.  Where the quotient overflows the form returns NaN (q = inf, r = -inf, inf - inf) and where it is subnormal
// it is off by one place (q is rounded at the subnormal quantum and the correction vanishes below it):
// tests/cartpole_divide_cases.py lists divisors that pass the proof and fail there.
// WHERE IT IS USED: cp_euler<true>, for dividends with |x| in [2^-90, 2^90) (cp_div_in_window) and a total mass in
// [2^-32, 2^32] (cp_fast_masses_ok): the quotient's magnitude then lies in [2^-122, 2^122), q within a place of it, and the
// scaling argument holds for every such pair.
__device__ __forceinline__ float cp_div_invariant(float x, float c, float y) {
  const float q = x * y;
  const float r = __builtin_fmaf(-c, q, x);
  return __builtin_fmaf(r, y, q);
}

// the dividends cp_euler<true> hands to cp_div_invariant: |x| inside [2^-90, 2^90) by its exponent field (zero, subnormal,
// infinite, NaN: outside)
__device__ __forceinline__ bool cp_div_in_window(float x) {
  return ((__float_as_uint(x) & 0x7fffffffu) - 0x12800000u) < 0x5a000000u;
}

// the masses a launch may run cp_euler<true> with (part of the `fast` predicates of cartpole.hip and cartpole_pool.hip):
// the pole's mass keeps the second dividend, masspole * cos^2, inside the window; the total mass keeps every quotient of
// a window dividend normal (cp_div_invariant)
__device__ __forceinline__ bool cp_fast_masses_ok(float masspole, float total_mass) {
  return (masspole >= 0x1.0p-60f) && (masspole <= 0x1.0p60f) && (total_mass >= 0x1.0p-32f) && (total_mass <= 0x1.0p32f);
}

// numpy's float32 sin / cos kernel (wd_np_sincosf) for |x| <= 0.75: the quadrant is 0 -- RN(x * 2/pi + magic) - magic = 0
// exactly (|x * 2/pi| < 0.478) and the three reduction FMAs return x itself -- so the reduction and the quadrant selects drop
// out: the same two polynomials on r = x, bit for bit (checked against wd_np_sincosf for every float32 in [-0.75, 0.75] by
// tests/test_gpu_core.py).  A pole beyond 12 degrees has fallen: the angle of a replica that is still running is below 0.21.
__device__ __forceinline__ void cp_sincos_small(float x, float &sin_out, float &cos_out) {
  const float r2 = x * x;
  float c = __builtin_fmaf(0x1.98e616p-16f, r2, -0x1.6c06dcp-10f);
  c = __builtin_fmaf(c, r2, 0x1.55553cp-05f);
  c = __builtin_fmaf(c, r2, -0x1.000000p-01f);
  c = __builtin_fmaf(c, r2, 0x1.000000p+00f);
  float sn = __builtin_fmaf(0x1.7d3bbcp-19f, r2, -0x1.a06bbap-13f);
  sn = __builtin_fmaf(sn, r2, 0x1.11119ap-07f);
  sn = __builtin_fmaf(sn, r2, -0x1.555556p-03f);
  sn = __builtin_fmaf(sn, r2, 0.0f);
  sn = __builtin_fmaf(sn, x, x);
  sin_out = sn;
  cos_out = c;
}

// one Euler update, cartpole_step_numba.py:42-78 (float32 state; everything downstream of the
// Python literal 4.0/3.0 in float64, as Numba types it).
// FAST (compile time; the middle ticks of a recorded launch whose PRECONDITIONS the kernel checked once, cp_tick_impl):
// |theta| <= 0.75 on entry -> the quadrant-free sin / cos; the two float32 divisions by the total mass in three
// instructions each.  Bit-identical to the general form: the one data-dependent condition left -- a dividend outside the
// window the division shortcut is used in (the force term's dividend; the other one is the pole's mass times cos^2) --
// redoes both divisions in a cold block behind a branch that is never taken in practice (the dividends are ~10 and ~0.1).
template <bool FAST = false>
__device__ __forceinline__ bool cp_euler(float4 &s, int action, const CpPhysics &p) {
  float x = s.x, x_dot = s.y, theta = s.z, theta_dot = s.w;
  const float force = (action > 0) ? p.force_mag : -p.force_mag;  // action > 0.5
  float sintheta, costheta;
  if (FAST) cp_sincos_small(theta, sintheta, costheta);
  else wd_np_sincosf(theta, sintheta, costheta);
  const float temp_num = force + p.polemass_length * (theta_dot * theta_dot) * sintheta;
  const float frac_num = p.masspole * (costheta * costheta);
  float temp, frac;
  if (FAST) {
    temp = cp_div_invariant(temp_num, p.total_mass, p.inv_total_mass);
    frac = cp_div_invariant(frac_num, p.total_mass, p.inv_total_mass);
    // frac_num is the pole's mass (inside [2^-60, 2^60]: a precondition of the launch) times cos^2 >= 0.53: always inside
    const bool in_range = cp_div_in_window(temp_num);
    if (__builtin_expect(__ballot(!in_range) != 0ull, 0)) {
      temp = temp_num / p.total_mass;
      frac = frac_num / p.total_mass;
    }
  } else {
    temp = temp_num / p.total_mass;
    frac = frac_num / p.total_mass;
  }
  const double den = (double)p.length * (4.0 / 3.0 - (double)frac);
  const double thetaacc = (double)(p.gravity * sintheta - costheta * temp) / den;
  const double xacc = (double)temp - (double)p.polemass_length * thetaacc * (double)costheta / (double)p.total_mass;
  x = x + p.tau * x_dot;
  x_dot = (float)((double)x_dot + (double)p.tau * xacc);
  theta = theta + p.tau * theta_dot;
  theta_dot = (float)((double)theta_dot + (double)p.tau * thetaacc);
  s = make_float4(x, x_dot, theta, theta_dot);
  return x < -p.x_threshold || x > p.x_threshold || theta < -p.theta_threshold_radians ||
         theta > p.theta_threshold_radians;
}

// ---- the policy INSIDE the rollout and evaluation kernels: rollout_policy.h (the network, the parity contract and the
// packed layout, pack_rollout_policy with I = 4) behind the float4 first layer; restated on the host in
// oracle/cartpole_np.py::policy_probabilities.  cp_policy_probs: the probabilities e[a] / sum (what the greedy scan
// needs); cp_policy_cum: their running float32 sums (what the inverse-CDF sampler compares the uniform with).
constexpr int CP_MAX_REG_ACTIONS = 8;

template <int H>
__device__ __forceinline__ void cp_policy_probs(const float *w, const float4 &s, int n_actions,
                                                float (&prob)[CP_MAX_REG_ACTIONS]) {
  float h1[H], logit[CP_MAX_REG_ACTIONS];
  rp_first_layer<H>(w, w + 4 * H, s, h1);
  const float m = rp_policy_logits<H>(w + 4 * H + H, h1, n_actions, logit);
  rp_softmax_probs(logit, m, n_actions, prob);
}

// (the softmax's terms and divisions stand here next to the running sums: behind a call the rollout entries compile to
// another schedule; rollout_policy.h::rp_softmax_probs is the same statements)
template <int H>
__device__ __forceinline__ void cp_policy_cum(const float *w, const float4 &s, int n_actions,
                                              float (&cumv)[CP_MAX_REG_ACTIONS]) {
  float h1[H], logit[CP_MAX_REG_ACTIONS];
  rp_first_layer<H>(w, w + 4 * H, s, h1);
  const float m = rp_policy_logits<H>(w + 4 * H + H, h1, n_actions, logit);
  float e[CP_MAX_REG_ACTIONS], sum = 0.0f;
#pragma unroll
  for (int a = 0; a < CP_MAX_REG_ACTIONS; ++a) {
    e[a] = (a < n_actions) ? expf(logit[a] - m) : 0.0f;
    sum += e[a];
  }
  float cum = 0.0f;
#pragma unroll
  for (int a = 0; a < CP_MAX_REG_ACTIONS; ++a) {
    const float p = e[a] / sum;
    if (a < n_actions) cum = (a == 0) ? p : cum + p;
    cumv[a] = cum;
  }
}

// Fused rollout tick(s): sample the action + step + reset a finished replica, `ticks` times per launch
// with the state kept in registers (a single tick at E = 100 000 moves 6.8 MB: under 1 us of HBM time,
// so one launch per tick is launch-bound -- SURVEY 8(d) asks the ceiling run to fuse T ticks).  The
// policy's probabilities are read once per launch, so ticks > 1 is a fixed-policy rollout; every tick
// still writes its action, observation, reward, done and timestep.  `_done_` reports the last tick.
// With the four `*_batch` pointers (the trainer's [T, E, ...] batch tensors, training/data_loader.py:
// processed observations, actions, rewards, done flags) tick k of the launch writes ROW k of them --
// the observation the policy acted on, the sampled action, the reward and the done flag, exactly what
// trainer_base.py:392-426 records per tick -- so T ticks move T times the bytes (28 B per env-step,
// all coalesced: the real HBM ceiling run of configs[4]); the per-tick arrays then receive the last
// tick only.  With `policy` (packed weights of a two-hidden-layer MLP of width `hidden` = 32 or 64 and one
// head, in dynamic LDS) the rollout runs with a LIVE policy: every tick evaluates the network on the
// replica's current observation instead of reading `probs` -- a whole training batch of ticks is then
// one launch (the reference runs policy forward, sampler, step and reset as separate launches with
// three host synchronisations per tick, trainer_base.py:392-426).
// (No __restrict__ on the arrays: the reset table aliases them.)
// stores of the tick loop through a wave-uniform base (SGPR pair) + a 32-bit per-lane byte offset: the per-lane 64-bit
// address arithmetic of four record arrays per tick (a v_mad_u64 and three-instruction adds each) becomes scalar work.
// Untracked like wd_store_untracked (wd_common.h): the loop never reads these addresses back.
__device__ __forceinline__ void cp_store_s(const void *sbase, uint32_t voff, int v) {
  asm volatile("global_store_dword %0, %1, %2" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
__device__ __forceinline__ void cp_store_s(const void *sbase, uint32_t voff, float v) {
  asm volatile("global_store_dword %0, %1, %2" ::"v"(voff), "v"(v), "s"(sbase) : "memory");
}
__device__ __forceinline__ void cp_store_s(const void *sbase, uint32_t voff, float4 v) {
  typedef float v4f_ __attribute__((ext_vector_type(4)));
  const v4f_ q = {v.x, v.y, v.z, v.w};
  asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" ::"v"(voff), "v"(q), "s"(sbase) : "memory");
}

}  // namespace
