// pg_update_matrix_common.h -- what the gradient launches on the float32 matrix cores share: pg_update_matrix.hip (the
// in-tree policies, O in {2, 4, 6} inputs) and include/wd_env_update_matrix.h (the kit for custom environments, F = 1 .. 32).
// The split both use -- a wavefront owns 32 rows, lanes l and l + 32 share row l % 32, lane half hf = l / 32 holds of
// every 32 hidden units the sixteen that its registers of a 32 x 32 accumulator hold -- is stated in pg_update_matrix.hip;
// here are the lane's unit list, the exchange between the halves and the unit-major staged arrays [unit][PGM_LD].
#pragma once
#include "pg_update_common.h"

#define PGM_LD 36                 // staged arrays are [unit][PGM_LD]: 32 rows, rows of 16-byte multiples

typedef float pgm_f16 __attribute__((ext_vector_type(16)));

// unit s of the list of lane half hf: tile s / 16, register v = s % 16 of the accumulator layout
__device__ __forceinline__ constexpr int pgm_unit(int s, int hf) {
  return 32 * (s / 16) + 8 * ((s % 16) / 4) + 4 * hf + s % 4;
}

// lower half's number + upper half's, on both halves
__device__ __forceinline__ float pgm_add_halves(float mine, int hf) {
  const float other = __shfl_xor(mine, 32);
  return (hf ? other : mine) + (hf ? mine : other);
}

template <int NU>
__device__ __forceinline__ uint32_t pgm_positive_mask(const float (&h)[NU]) {
  uint32_t m = 0;
#pragma unroll
  for (int s = 0; s < NU; ++s) m |= (h[s] > 0.0f) ? (1u << s) : 0u;
  return m;
}

// the lane's units of its row, unit-major: S[unit][row]
template <int NU>
__device__ __forceinline__ void pgm_stage(float *S, int r, int hf, const float (&h)[NU]) {
#pragma unroll
  for (int s = 0; s < NU; ++s) S[(pgm_unit(s, 0) + 4 * hf) * PGM_LD + r] = h[s];
}

// unit 32 t + m of the staged array, rows 16 hf .. 16 hf + 15
template <int TO>
__device__ __forceinline__ void pgm_unit_rows(const float *S, int m, int hf, float4 (&out)[TO][4]) {
#pragma unroll
  for (int t = 0; t < TO; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) out[t][q] = *(const float4 *)(S + (32 * t + m) * PGM_LD + 16 * hf + 4 * q);
}

// acc += sum over the sixteen rows, ascending, of a[row] * b[row]
__device__ __forceinline__ float pgm_dot16(float acc, const float4 (&a)[4], const float4 (&b)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc = fmaf(a[q].x, b[q].x, acc); acc = fmaf(a[q].y, b[q].y, acc);
    acc = fmaf(a[q].z, b[q].z, acc); acc = fmaf(a[q].w, b[q].w, acc);
  }
  return acc;
}

__device__ __forceinline__ float pgm_sum16(float acc, const float4 (&a)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) { acc += a[q].x; acc += a[q].y; acc += a[q].z; acc += a[q].w; }
  return acc;
}
