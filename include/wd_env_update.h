// wd_env_update.h -- the kit for the A2C / PPO UPDATE of a custom environment's in-kernel policy AS KERNELS: the five
// launches of csrc/kernels/pg_update.hip -- values, returns, gradients, reduce, clip + Adam + refill of the rollout's packed
// policy -- for an observation size F the author fixes at compile time (docs/custom_environments.md, "The update as
// kernels").  One macro per device source:
//
//     #include "wd_env_update.h"
//     WD_PG_UPDATE_ENTRIES(MyEnv, 5)        // F = 5 observation floats per row
//
// defines six `extern "C"` entries (the returns launch stays the package's own HipDiscountedReturns):
//
//     HipMyEnvPgValues_H32 / _H64      (obs, theta, long rows, int A, values)
//                                      values[row] = v(obs[row]); __launch_bounds__(256), one thread per row, grid-stride;
//                                      dynamic LDS: wd_pg_values_lds_floats(H, F) floats
//     HipMyEnvPgGradients_H32 / _H64   (obs, actions, adv, ret, theta, long rows, int A, inv_R, ent_coeff, vf_coeff, partials)
//                                      the block is the 128-row tile; one partial of P + 4 floats per block (the eight
//                                      gradient tensors, then the sums of logp * adv, of the entropy, of (v - ret)^2 and of
//                                      adv); dynamic LDS: wd_pg_gradients_lds_floats(H, F) floats
//     HipMyEnvPgReduce                 (partials, n_blocks, H, A, grads, sumsq, sums)     9 blocks of 1024 threads
//     HipMyEnvPgApply                  (theta, exp_avg, exp_avg_sq, grads, sumsq, packed, H, A, max_norm, step_size,
//                                      bc2_sqrt, one_minus_beta1, beta2, one_minus_beta2, eps)   one thread per parameter
//
// An entry launched with H not in {32, 64} or with A outside 1 .. 8 touches nothing.
// warp_drive_amd/training/pg_update_custom_kernels.py packs exactly these arguments;
// warp_drive_amd/utils/custom_tick.py::FusedUpdateMixin gives an env class the launches.
//
// A row is (t, replica, agent): rows = T * E * N, obs [rows][F] float32, actions [rows] int32, adv / ret / values [rows].
//
// The network FLAT, in the order of the module's parameters (training/models.py::FullyConnected; P =
// upd_pg_net_floats(H, F, A) floats): W0 [H][F], b0 [H], W1 [H][H], b1 [H], Wp [A][H], bp [A], Wv [H], bv [1].  Its first
// P - H - 1 floats are the rollout kit's packed policy (wd_env_rollout.h; pack_rollout_policy), which the Apply entry
// refills: packed[idx] = theta[idx] for idx < P - H - 1.
//
// This header is NOT self-contained: it includes the package's csrc/kernels/pg_update_common.h (the build of a custom
// environment's unit passes that directory with -I), which states the PARITY CONTRACT of the update kernels -- summation
// order, relu'(0) = 0, no float atomics, the clip and Adam expressions -- once, for the in-tree units and for this kit.
// What this file adds to it:
//   * the first layer: W0's rows sit in LDS at stride pad4(F), the pad columns zero; a row is read as whole float4s and
//     a scalar tail; exactly F fmaf per unit in index order, no arithmetic on a pad column;
//   * A at run time: eight logit slots guarded by A, the value as output 8; the objective's statements are
//     policy_mlp.hip::HipPolicyGradientHead's, the shift by the maximum first;
//   * a tile's 128 * F observation floats are loaded coalesced and written transposed into the staged [F][LD] array;
//     the forward reads the lane's own column from there.
// No inline assembly beyond the empty compiler barrier of the value loop; no atomics.
#pragma once
#include "pg_update_common.h"

#define WD_UPD_TILE 128                        // rows per tile = threads per block of a Gradients entry
#define WD_UPD_LD (WD_UPD_TILE + 4)            // staged arrays are [unit][WD_UPD_LD]
#define WD_UPD_MAX_ACTIONS 8
#define WD_UPD_OUTPUTS (WD_UPD_MAX_ACTIONS + 1)   // staged output deltas: the logits' (those below A are real), the value's
#define WD_UPD_MAX_OBS 32
#define WD_UPD_REDUCE_THREADS 1024

// the two dynamic LDS sizes, in floats (pg_update_custom_kernels.py states the same formulas)
constexpr int wd_pg_values_lds_floats(int H, int F) {
  return upd_pad4(H * upd_pad4(F) + H + H * H + H + WD_UPD_MAX_ACTIONS * H + WD_UPD_MAX_ACTIONS + H + 1);
}
constexpr int wd_pg_gradients_lds_floats(int H, int F) {
  return wd_pg_values_lds_floats(H, F) + (2 * H + F + WD_UPD_OUTPUTS + 4) * WD_UPD_LD;
}

// offsets inside the LDS copy: W0 with rows of pad4(F) floats, b0 .. bp as in the flat buffer behind it, the value head
// on a 16-byte boundary behind eight bias slots; and inside the flat buffer
template <int H, int F>
struct WdUpdNet {
  static_assert(F >= 1 && F <= WD_UPD_MAX_OBS, "the update kit takes 1 to 32 observation floats");
  static_assert(H % 4 == 0, "the rows of W1 / Wp / Wv are read as float4");
  static constexpr int S = upd_pad4(F);   // floats per row of W0 in LDS
  static constexpr int W0 = 0, B0 = H * S, W1 = B0 + H, B1 = W1 + H * H, WP = B1 + H;
  static constexpr int bp(int A) { return WP + A * H; }
  static constexpr int wv(int A) { return WP + A * H + WD_UPD_MAX_ACTIONS; }
  static constexpr int LDS = upd_pad4(WP + WD_UPD_MAX_ACTIONS * H + WD_UPD_MAX_ACTIONS + H + 1);
  static_assert(LDS == wd_pg_values_lds_floats(H, F), "the LDS copy of the network");
  static constexpr int F_B0 = H * F, F_W1 = F_B0 + H, F_B1 = F_W1 + H * H, F_WP = F_B1 + H;   // the flat buffer
};

template <int H, int F>
__device__ __forceinline__ void wd_upd_copy_net_to_lds(float *dst, const float *__restrict__ theta, int A) {
  using L = WdUpdNet<H, F>;
  for (int i = threadIdx.x; i < H * L::S; i += blockDim.x) {
    const int r = i / L::S, c = i - r * L::S;
    dst[i] = c < F ? theta[r * F + c] : 0.0f;
  }
  const int rest = H + H * H + H + A * H + A;   // b0 .. bp
  for (int i = threadIdx.x; i < rest; i += blockDim.x) dst[L::B0 + i] = theta[L::F_B0 + i];
  for (int i = threadIdx.x; i < H + 1; i += blockDim.x) dst[L::wv(A) + i] = theta[L::F_B0 + rest + i];
}

// h1 = relu(W0 x + b0), x[k] = x_column[k * x_stride]: whole float4s of a row, then its tail as scalars
template <int H, int F>
__device__ __forceinline__ void wd_upd_layer0(const float *w, const float *x_column, int x_stride, float (&h1)[H]) {
  using L = WdUpdNet<H, F>;
  constexpr int F4 = F & ~3;
  float x[F];
#pragma unroll
  for (int k = 0; k < F; ++k) x[k] = x_column[k * x_stride];
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = w[L::B0 + i];
#pragma unroll
    for (int k = 0; k < F4; k += 4) {
      const float4 wr = *(const float4 *)(w + L::W0 + i * L::S + k);
      acc = fmaf(wr.x, x[k], acc); acc = fmaf(wr.y, x[k + 1], acc);
      acc = fmaf(wr.z, x[k + 2], acc); acc = fmaf(wr.w, x[k + 3], acc);
    }
#pragma unroll
    for (int k = F4; k < F; ++k) acc = fmaf(w[L::W0 + i * L::S + k], x[k], acc);
    h1[i] = fmaxf(acc, 0.0f);
  }
}

// ------------------------------------------------------------------------------------------------------ 1. values
template <int H, int F>
__device__ __forceinline__ void wd_upd_values(const float *__restrict__ obs, const float *__restrict__ theta, long rows,
                                              int A, float *__restrict__ values) {
  using L = WdUpdNet<H, F>;
  extern __shared__ __attribute__((aligned(16))) float wd_upd_lds[];
  wd_upd_copy_net_to_lds<H, F>(wd_upd_lds, theta, A);
  __syncthreads();
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < rows; g += (long)gridDim.x * blockDim.x) {
    // (the weights are the same for every trip: without this the compiler hoists their LDS reads out of the loop and
    // spills them)
    asm volatile("" ::: "memory");
    float h1[H], h2[H];
    wd_upd_layer0<H, F>(wd_upd_lds, obs + g * F, 1, h1);
    values[g] = upd_layer1_and_value<H>(wd_upd_lds + L::W1, wd_upd_lds + L::B1, wd_upd_lds + L::wv(A), h1, h2);
  }
}

// --------------------------------------------------------------------------------------------------- 3. gradients
// What a thread owns of the gradient for the whole launch (128 threads): UpdOwn's share of dW0, db0, dW1, db1, and
//   dWp [A][H], dWv [H]: unit i = tid % H, outputs o = tid / H + KG c (c < OB; o < A: a logit, o = 8: the value)
//   dbp, dbv: output o = tid (tid < 9);  the four sums: threads 16 .. 19
template <int H>
struct WdUpdOwn : UpdOwn<H, WD_UPD_TILE> {
  static constexpr int OB = (WD_UPD_OUTPUTS + WdUpdOwn::KG - 1) / WdUpdOwn::KG;
};

template <int H, int F>
using WdUpdAcc = UpdAcc<WdUpdOwn<H>::JB, (F + WdUpdOwn<H>::KG - 1) / WdUpdOwn<H>::KG, WdUpdOwn<H>::OB>;

// dWp[o][i] += sum_r dz[o][r] * h2[i][r]; dWv[i] += sum_r dv[r] * h2[i][r]; dbp[o] += sum_r dz[o][r]; dbv += sum_r dv[r];
// the four sums += their staged per-row terms   (rows ascending; SD = [WD_UPD_OUTPUTS][LD], SS = [4][LD])
template <int H, int F>
__device__ __forceinline__ void wd_upd_acc_heads(WdUpdAcc<H, F> &g, const float *S1, const float *SD, const float *SS, int A) {
  using W = WdUpdOwn<H>;
  const int tid = threadIdx.x, i = tid % H, o0 = tid / H;
#pragma unroll
  for (int c = 0; c < W::OB; ++c) {
    const int o = o0 + W::KG * c;
    if (o < A || o == WD_UPD_MAX_ACTIONS) {
      float acc = g.wo[c];
      for (int r = 0; r < WD_UPD_TILE; r += 4) {
        const float4 h = *(const float4 *)(S1 + i * WD_UPD_LD + r), d = *(const float4 *)(SD + o * WD_UPD_LD + r);
        acc = fmaf(d.x, h.x, acc); acc = fmaf(d.y, h.y, acc); acc = fmaf(d.z, h.z, acc); acc = fmaf(d.w, h.w, acc);
      }
      g.wo[c] = acc;
    }
  }
  if (tid < A || tid == WD_UPD_MAX_ACTIONS) {
    for (int r = 0; r < WD_UPD_TILE; ++r) g.bo += SD[tid * WD_UPD_LD + r];
  }
  if (tid >= 16 && tid < 20) {
    for (int r = 0; r < WD_UPD_TILE; ++r) g.sum += SS[(tid - 16) * WD_UPD_LD + r];
  }
}

// the block's partial, in the FLAT layout (A logits): P floats, then the four sums
template <int H, int F>
__device__ __forceinline__ void wd_upd_write_partial(const WdUpdAcc<H, F> &g, float *out, int A) {
  using L = WdUpdNet<H, F>;
  using W = WdUpdOwn<H>;
  constexpr int JB = W::JB, KB = WdUpdAcc<H, F>::KB;
  const int tid = threadIdx.x, ib = tid % W::NIB, jb = tid / W::NIB;
  const int BP = L::F_WP + A * H, WV = BP + A, BV = WV + H;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < JB; ++b) out[L::F_W1 + (ib + W::NIB * a) * H + jb + W::NJB * b] = g.w1[a][b];
  const int i = tid % H, k0 = KB * (tid / H), o0 = tid / H;
#pragma unroll
  for (int c = 0; c < KB; ++c)
    if (k0 + c < F) out[i * F + k0 + c] = g.w0[c];
#pragma unroll
  for (int c = 0; c < W::OB; ++c) {
    const int o = o0 + W::KG * c;
    if (o < A) out[L::F_WP + o * H + i] = g.wo[c];
    else if (o == WD_UPD_MAX_ACTIONS) out[WV + i] = g.wo[c];
  }
  if (tid < H) {
    out[L::F_B0 + tid] = g.b0;
    out[L::F_B1 + tid] = g.b1;
  }
  if (tid < A) out[BP + tid] = g.bo;
  else if (tid == WD_UPD_MAX_ACTIONS) out[BV] = g.bo;
  if (tid >= 16 && tid < 20) out[BV + 1 + tid - 16] = g.sum;
}

// blockDim.x = WD_UPD_TILE; partials [gridDim.x][P + 4]
template <int H, int F>
__device__ __forceinline__ void wd_upd_gradients(const float *__restrict__ obs, const int *__restrict__ actions,
                                                 const float *__restrict__ adv, const float *__restrict__ ret,
                                                 const float *__restrict__ theta, long rows, int A, float inv_R,
                                                 float ent_coeff, float vf_coeff, float *__restrict__ partials) {
  using L = WdUpdNet<H, F>;
  constexpr int LD = WD_UPD_LD, TILE = WD_UPD_TILE, MAXA = WD_UPD_MAX_ACTIONS;
  static_assert(wd_pg_gradients_lds_floats(H, F) == L::LDS + (2 * H + F + WD_UPD_OUTPUTS + 4) * LD, "the LDS carve-up");
  extern __shared__ __attribute__((aligned(16))) float wd_upd_lds[];
  float *w = wd_upd_lds, *S0 = w + L::LDS, *S1 = S0 + H * LD, *S2 = S1 + H * LD, *SD = S2 + F * LD;
  float *SS = SD + WD_UPD_OUTPUTS * LD;
  wd_upd_copy_net_to_lds<H, F>(w, theta, A);
  const int tid = threadIdx.x;
  const long tiles = (rows + TILE - 1) / TILE;
  const long obs_floats = rows * F;
  WdUpdAcc<H, F> acc;
  acc.clear();
  __syncthreads();
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long g = tile * TILE + tid;
    const bool live = g < rows;
    // the tile's observation floats, contiguous in memory, transposed into S2 [F][LD] (rows beyond the batch: zeros)
    {
      const long first = tile * (TILE * F);
#pragma unroll
      for (int q = tid; q < TILE * F; q += TILE) {
        const int r = q / F, k = q - r * F;
        S2[k * LD + r] = first + q < obs_floats ? obs[first + q] : 0.0f;
      }
    }
    float a = 0.0f, rt = 0.0f;
    int taken = 0;
    if (live) {
      a = adv[g];
      rt = ret[g];
      taken = actions[g];
    }
    __syncthreads();
    uint64_t m1, m2;
    {
      float dz[MAXA], dv;
      float h1[H], h2[H];
      wd_upd_layer0<H, F>(w, S2 + tid, LD, h1);
      const float v = upd_layer1_and_value<H>(w + L::W1, w + L::B1, w + L::wv(A), h1, h2);
      m1 = upd_positive_mask<H>(h1);
      m2 = upd_positive_mask<H>(h2);
      // the logits: acc = bias, one fmaf per hidden unit in index order
      float z[MAXA], m = -__builtin_inff();
#pragma unroll
      for (int j = 0; j < MAXA; ++j) {
        z[j] = -__builtin_inff();
        if (j < A) {
          float s = w[L::bp(A) + j];
#pragma unroll
          for (int i = 0; i < H; i += 4) {
            const float4 wr = *(const float4 *)(w + L::WP + j * H + i);
            s = fmaf(wr.x, h2[i], s); s = fmaf(wr.y, h2[i + 1], s);
            s = fmaf(wr.z, h2[i + 2], s); s = fmaf(wr.w, h2[i + 3], s);
          }
          z[j] = s;
          m = fmaxf(m, s);
        }
      }
      // HipPolicyGradientHead's statements (policy_mlp.hip), one head: the shift by the maximum FIRST (they stay in each
      // unit: see pg_update.hip)
      float total = 0.0f;
#pragma unroll
      for (int j = 0; j < MAXA; ++j)
        if (j < A) total += expf(z[j] - m);
      const float lse = logf(total);
      float Hent = 0.0f;
#pragma unroll
      for (int j = 0; j < MAXA; ++j)
        if (j < A) {
          const float lp = (z[j] - m) - lse;
          Hent -= expf(lp) * lp;
        }
      const int clamped = min(max(taken, 0), A - 1);
      float logp_taken = 0.0f;
#pragma unroll
      for (int j = 0; j < MAXA; ++j)
        if (j == clamped) logp_taken = (z[j] - m) - lse;
#pragma unroll
      for (int j = 0; j < MAXA; ++j) {
        dz[j] = 0.0f;
        if (j < A && live) {
          const float lp = (z[j] - m) - lse, pj = expf(lp);
          dz[j] = (a * (pj - (j == taken ? 1.0f : 0.0f)) + ent_coeff * pj * (lp + Hent)) * inv_R;
        }
      }
      const float d = v - rt;
      dv = live ? 2.0f * vf_coeff * d * inv_R : 0.0f;
      upd_stage<H, LD>(S0, tid, h1);
      upd_stage<H, LD>(S1, tid, h2);
#pragma unroll
      for (int j = 0; j < MAXA; ++j) SD[j * LD + tid] = dz[j];
      SD[MAXA * LD + tid] = dv;
      SS[0 * LD + tid] = live ? logp_taken * a : 0.0f;
      SS[1 * LD + tid] = live ? Hent : 0.0f;
      SS[2 * LD + tid] = live ? d * d : 0.0f;
      SS[3 * LD + tid] = live ? a : 0.0f;
    }
    __syncthreads();
    wd_upd_acc_heads<H, F>(acc, S1, SD, SS, A);
    __syncthreads();
    {
      // d2[i] = relu'(h2[i]) * (sum_j dz[j] Wp[j][i] + dv Wv[i]), j ascending from +0, the value last (the deltas read
      // back from the lane's own staged column).  Four units at a time, staged as they are formed (the form of
      // pg_update_gridworld.hip -- the same sums in the same order as pg_update.hip's, which keeps all H in flight and
      // spills next to a long observation row)
      float dz[MAXA];
#pragma unroll
      for (int j = 0; j < MAXA; ++j) dz[j] = SD[j * LD + tid];
      const float dv = SD[MAXA * LD + tid];
#pragma unroll
      for (int i = 0; i < H; i += 4) {
        float d2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < MAXA; ++j) {
          if (j < A) {
            const float4 wr = *(const float4 *)(w + L::WP + j * H + i);
            d2[0] = fmaf(wr.x, dz[j], d2[0]); d2[1] = fmaf(wr.y, dz[j], d2[1]);
            d2[2] = fmaf(wr.z, dz[j], d2[2]); d2[3] = fmaf(wr.w, dz[j], d2[3]);
          }
        }
        const float4 wr = *(const float4 *)(w + L::wv(A) + i);
        d2[0] = fmaf(wr.x, dv, d2[0]); d2[1] = fmaf(wr.y, dv, d2[1]);
        d2[2] = fmaf(wr.z, dv, d2[2]); d2[3] = fmaf(wr.w, dv, d2[3]);
#pragma unroll
        for (int c = 0; c < 4; ++c) S1[(i + c) * LD + tid] = ((m2 >> (i + c)) & 1ull) ? d2[c] : 0.0f;
      }
    }
    __syncthreads();
    upd_acc_w1<H, TILE, LD>(acc, S0, S1);
    {
      float d1[H];
      upd_layer1_backward<H, LD>(w + L::W1, S1 + tid, m1, d1);
      __syncthreads();
      upd_stage<H, LD>(S1, tid, d1);
    }
    __syncthreads();
    upd_acc_w0<H, TILE, LD, F>(acc, S1, S2);
    __syncthreads();
  }
  wd_upd_write_partial<H, F>(acc, partials + (long)blockIdx.x * (upd_pg_net_floats(H, F, A) + 4), A);
}

// ------------------------------------------------------------------------------------------- 4 and 5: reduce, apply
__device__ __forceinline__ bool wd_upd_shape_ok(int H, int A) {
  return (H == 32 || H == 64) && A >= 1 && A <= WD_UPD_MAX_ACTIONS;
}

template <int F>
__device__ __forceinline__ void wd_upd_reduce(float *tree, const float *__restrict__ partials, int n_blocks, int H, int A,
                                              float *__restrict__ grads, float *__restrict__ sumsq,
                                              float *__restrict__ sums) {
  if (!wd_upd_shape_ok(H, A)) return;
  upd_pg_reduce<WD_UPD_REDUCE_THREADS>(tree, partials, n_blocks, upd_pg_net_floats(H, F, A), H, F, A, grads, sumsq, sums);
}

// one thread per parameter; `packed`: the rollout's copy of the policy (the first P - H - 1 floats) or null
template <int F>
__device__ __forceinline__ void wd_upd_apply(float *__restrict__ theta, float *__restrict__ exp_avg,
                                             float *__restrict__ exp_avg_sq, const float *__restrict__ grads,
                                             const float *__restrict__ sumsq, float *__restrict__ packed, int H, int A,
                                             float max_norm, float step_size, float bc2_sqrt, float one_minus_beta1,
                                             float beta2, float one_minus_beta2, float eps) {
  if (!wd_upd_shape_ok(H, A)) return;
  const int P = upd_pg_net_floats(H, F, A);
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P) return;
  const float p = upd_clip_adam(idx, theta, exp_avg, exp_avg_sq, grads, sumsq, 8, max_norm, step_size, bc2_sqrt,
                                one_minus_beta1, beta2, one_minus_beta2, eps);
  if (packed != nullptr && idx < P - H - 1) packed[idx] = p;
}

#define WD_PG_UPDATE_WIDTH_ENTRIES_(Name, F, HH)                                                                       \
  extern "C" __global__ void __launch_bounds__(256) Hip##Name##PgValues_H##HH(                                         \
      const float *__restrict__ obs, const float *__restrict__ theta, long rows, int A, float *__restrict__ values) {  \
    if (A < 1 || A > WD_UPD_MAX_ACTIONS) return;                                                                       \
    wd_upd_values<HH, F>(obs, theta, rows, A, values);                                                                 \
  }                                                                                                                    \
  extern "C" __global__ void __launch_bounds__(WD_UPD_TILE) Hip##Name##PgGradients_H##HH(                              \
      const float *__restrict__ obs, const int *__restrict__ actions, const float *__restrict__ adv,                   \
      const float *__restrict__ ret, const float *__restrict__ theta, long rows, int A, float inv_R, float ent_coeff,  \
      float vf_coeff, float *__restrict__ partials) {                                                                  \
    if (A < 1 || A > WD_UPD_MAX_ACTIONS) return;                                                                       \
    wd_upd_gradients<HH, F>(obs, actions, adv, ret, theta, rows, A, inv_R, ent_coeff, vf_coeff, partials);             \
  }

// the six entries of one environment: Name its prefix (Hip<Name>Pg...), F its observation floats per row
#define WD_PG_UPDATE_ENTRIES(Name, F)                                                                                  \
  WD_PG_UPDATE_WIDTH_ENTRIES_(Name, F, 32)                                                                             \
  WD_PG_UPDATE_WIDTH_ENTRIES_(Name, F, 64)                                                                             \
  extern "C" __global__ void __launch_bounds__(WD_UPD_REDUCE_THREADS) Hip##Name##PgReduce(                             \
      const float *__restrict__ partials, int n_blocks, int H, int A, float *__restrict__ grads,                       \
      float *__restrict__ sumsq, float *__restrict__ sums) {                                                           \
    __shared__ float tree[WD_UPD_REDUCE_THREADS];                                                                      \
    wd_upd_reduce<F>(tree, partials, n_blocks, H, A, grads, sumsq, sums);                                              \
  }                                                                                                                    \
  extern "C" __global__ void __launch_bounds__(256) Hip##Name##PgApply(                                                \
      float *__restrict__ theta, float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,                          \
      const float *__restrict__ grads, const float *__restrict__ sumsq, float *__restrict__ packed, int H, int A,      \
      float max_norm, float step_size, float bc2_sqrt, float one_minus_beta1, float beta2, float one_minus_beta2,      \
      float eps) {                                                                                                     \
    wd_upd_apply<F>(theta, exp_avg, exp_avg_sq, grads, sumsq, packed, H, A, max_norm, step_size, bc2_sqrt,             \
                    one_minus_beta1, beta2, one_minus_beta2, eps);                                                     \
  }
