// wd_test_kernels.hip -- kernels that exist for the test suite and the measurement scripts only; their own code
// object (wd_kernels_test.hsaco), so that nothing of it ships inside the product objects.
#include "wd_common.h"
#include "cartpole_common.h"   // rollout_policy.h (the in-kernel policy forward) + Cartpole's wrappers around it

namespace {

// ------------------------------------------------------------- the in-kernel policy forward, seen directly
// tests/test_gpu_inkernel_policy_logits.py: the logits, probabilities, greedy action and (float4 form) running sums of one
// observation row per lane, through the same templates the rollout and evaluation entries call, the packed weights
// staged in dynamic LDS as the units stage them.  FORM 0: rp_first_layer's float4 form (Cartpole: I = 4), the running
// sums from cp_policy_cum<H>; 1 / 2: its float2 form at O = 2 / O = 6 (MountainCar, Acrobot); 3: rp_first_layer_strided
// <H, 21, 24> with the row read from LDS (TagGridWorld).  Eight floats per row and output; the logits past n_actions are
// -inf, the probabilities 0.  Dynamic LDS: the packed weights rounded up to four floats + blockDim.x rows of STRIDE floats.
constexpr int TP_MAXA = 8;

template <int H, int FORM>
__device__ __forceinline__ void tp_policy_impl(float *lds, const float *packed, int n_weights, const float *obs, int n_rows,
                                               int n_actions, float *logits, float *probs, float *cums, int *first_max) {
  constexpr int I = FORM == 0 ? 4 : FORM == 1 ? 2 : FORM == 2 ? 6 : 21;
  constexpr int STRIDE = FORM == 3 ? 24 : I;
  // (uniform) another action count or another buffer than this form reads: nothing is written
  if (packed == nullptr || n_actions < 1 || n_actions > TP_MAXA || n_weights != rp_policy_floats(STRIDE, H, n_actions)) return;
  for (int i = threadIdx.x; i < n_weights; i += blockDim.x) lds[i] = packed[i];
  float *x = lds + ((n_weights + 3) & ~3) + threadIdx.x * STRIDE;
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = row < n_rows;
#pragma unroll
  for (int j = 0; j < I; ++j) x[j] = live ? obs[(long)row * I + j] : 0.0f;
  __syncthreads();
  if (!live) return;
  const float *w = lds;
  float h1[H], logit[TP_MAXA], prob[TP_MAXA], cumv[TP_MAXA];
#pragma unroll
  for (int a = 0; a < TP_MAXA; ++a) cumv[a] = -1.0f;   // (no running sums in this form)
  if constexpr (FORM == 0) {
    const float4 s = make_float4(x[0], x[1], x[2], x[3]);
    rp_first_layer<H>(w, w + 4 * H, s, h1);
    cp_policy_cum<H>(w, s, n_actions, cumv);
  } else if constexpr (FORM == 3) {
    rp_first_layer_strided<H, I, STRIDE>(w, w + H * STRIDE, x, h1);
  } else {
    float o[I];
#pragma unroll
    for (int j = 0; j < I; ++j) o[j] = x[j];
    rp_first_layer<H, I>(w, w + I * H, o, h1);
  }
  const float m = rp_policy_logits<H>(w + STRIDE * H + H, h1, n_actions, logit);
  rp_softmax_probs(logit, m, n_actions, prob);
  first_max[row] = rp_first_maximum(prob, n_actions);
#pragma unroll
  for (int a = 0; a < TP_MAXA; ++a) {
    logits[(long)row * TP_MAXA + a] = logit[a];
    probs[(long)row * TP_MAXA + a] = prob[a];
    cums[(long)row * TP_MAXA + a] = cumv[a];
  }
}

}  // namespace

extern "C" {

#define WD_TEST_POLICY(NAME, HH, FORM)                                                                              \
  __global__ __launch_bounds__(64) void NAME(const float *packed, int n_weights, const float *obs, int n_rows,     \
                                             int n_actions, float *logits, float *probs, float *cums,               \
                                             int *first_max) {                                                      \
    extern __shared__ __attribute__((aligned(16))) float tp_lds[];                                                  \
    tp_policy_impl<HH, FORM>(tp_lds, packed, n_weights, obs, n_rows, n_actions, logits, probs, cums, first_max);     \
  }
WD_TEST_POLICY(wd_test_policy_f4_H32, 32, 0)
WD_TEST_POLICY(wd_test_policy_f4_H64, 64, 0)
WD_TEST_POLICY(wd_test_policy_f2o2_H32, 32, 1)
WD_TEST_POLICY(wd_test_policy_f2o2_H64, 64, 1)
WD_TEST_POLICY(wd_test_policy_f2o6_H32, 32, 2)
WD_TEST_POLICY(wd_test_policy_f2o6_H64, 64, 2)
WD_TEST_POLICY(wd_test_policy_s21_H32, 32, 3)
WD_TEST_POLICY(wd_test_policy_s21_H64, 64, 3)

// Write-bandwidth probe (scripts/write_pattern_probe.py): every block streams `floats_per_block`
// floats into its own contiguous slice of `out` (slice b starts at b * slice_stride floats), `vec`
// floats per lane per store (1 or 4).  Shows what the HBM write path gives to the rollout's access
// pattern -- thousands of blocks, each writing one replica's contiguous rows -- as opposed to a
// grid-stride fill.
__global__ void wd_write_probe(float *out, long slice_stride, int floats_per_block, int vec, float value) {
  float *dst = out + (long)blockIdx.x * slice_stride;
  if (vec == 4) {
    for (int i = 4 * threadIdx.x; i + 3 < floats_per_block; i += 4 * blockDim.x)
      *(float4 *)(dst + i) = make_float4(value, value, value, value);
  } else {
    for (int i = threadIdx.x; i < floats_per_block; i += blockDim.x) dst[i] = value;
  }
}

// ------------------------------------------------------------- Cartpole's division shortcut, counted
// tests/test_gpu_cartpole_divide.py: for every float32 magnitude pattern first_pattern .. first_pattern + n_patterns - 1
// (below 2^31) and its negation, the shipping window test (cp_div_in_window) and, inside the window, the shipping
// cp_div_invariant(x, c, y) against x / c.  out[0] += dividends inside the window, out[1] += those whose two results differ
// (NaN against NaN is equal, NaN against infinity is not).  Independent of HipCartPoleVerifyInvariantDivide: no binade is
// chosen here, the caller sweeps what it likes (the whole window is 0x5a000000 patterns).
__global__ void wd_test_cartpole_divide(float c, float y, uint32_t first_pattern, uint32_t n_patterns,
                                        unsigned long long *out) {
  unsigned long long inside = 0ull, differ = 0ull;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_patterns; i += stride) {
    const uint32_t bits = first_pattern + (uint32_t)i;
#pragma unroll
    for (int sgn = 0; sgn < 2; ++sgn) {
      const float x = __uint_as_float(bits | (sgn ? 0x80000000u : 0u));
      if (!cp_div_in_window(x)) continue;
      const float want = x / c, got = cp_div_invariant(x, c, y);
      inside += 1ull;
      if (__float_as_uint(want) != __float_as_uint(got) && !(want != want && got != got)) differ += 1ull;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    inside += __shfl_down(inside, off);
    differ += __shfl_down(differ, off);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(out, inside);
    atomicAdd(out + 1, differ);
  }
}

// ------------------------------------------------------------- math self-test hook
// Evaluates the device restatements of numpy's float32 routines so the GPU parity
// suite can compare them bit-for-bit with numpy on the host (tests/test_gpu_math.py).
__global__ void wd_test_math(const float *__restrict__ a, const float *__restrict__ b,
                             float *out_sin, float *out_cos, float *out_rem, float *out_sqrt,
                             float *out_div, int n) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float s, c;
    wd_np_sincosf(a[i], s, c);
    out_sin[i] = s;
    out_cos[i] = c;
    out_rem[i] = wd_np_remainderf(a[i], b[i]);
    out_sqrt[i] = sqrtf(a[i] * a[i] + b[i] * b[i]);
    out_div[i] = a[i] / b[i];
  }
}

}  // extern "C"
