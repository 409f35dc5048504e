// pg_update_gridworld.hip -- pg_update.hip's A2C / PPO update (training/trainer.py, `trainer.fused_update: "all"`) for the
// policies the one-launch TagGridWorld rollout evaluates itself (tag_gridworld_n5.hip: "tagger", 4 agents, and "runner",
// 1 agent): 21 observation floats, two hidden layers of H = 32 / 64 ReLU units, one head of FIVE logits and the value
// head.  Five launches per trained policy, as there:
//
//   1. HipPgGwValues_H<H>      values[row] = v(obs[row]) of the rows = T * E * n recorded rows (row = (t, replica, agent
//                              of the policy)); one thread per row, grid-stride.
//   2. HipDiscountedReturns    the existing entry of wd_kernels_update.hsaco (policy_mlp.hip) on `values`, n agents,
//                              w = 1, v_col = 0.
//   3. HipPgGwGradients_H<H>   forward, HipPolicyGradientHead's statements, backward; one partial of the eight gradient
//                              tensors and of four sums per block.
//   4. HipPgGwReduce           the partials summed in block order, the per-tensor sums of squares, the four sums.
//   5. HipPgGwApply            clip_grad_norm_, Adam, and the refill of the rollout's packed policy in
//                              pack_gridworld_policy's layout -- EVERY float of that block, pad columns and tail included.
//
// The summation order, relu'(0) = 0, "no float atomics, nothing read back" and the clip and Adam expressions are the parity
// contract pg_update_common.h states, with the pieces this unit shares with pg_update.hip and ddpg_update.hip.
//
// The network FLAT, in the order of the module's parameters (the parameters are views of it: FlatPolicy): W0 [H][21]
// (unpadded), b0 [H], W1 [H][H], b1 [H], Wp [5][H], bp [5], Wv [H], bv [1].  In LDS the rows of W0 are GW_IN_STRIDE = 24
// floats apart (tag_gridworld_n5_common.h's GW5_IN_STRIDE: every row starts on a 16-byte boundary), the three pad columns
// zero, and the value head starts on a 16-byte boundary behind eight bias slots.
//
// Forward arithmetic is gw5_policy_probs' (that header).  The probabilities are not claimed bit-identical to the rollout's.
//
// Stage 3 differs from pg_update.hip's in one thing: a tile's 128 x 21 observation floats are contiguous in memory, so the
// block loads them with coalesced loads and writes them transposed into the staged [21][LD] array FIRST, and the forward
// reads the lane's own column from there (no observation registers live across the backward pass; no 84-byte-strided
// loads).
//
// Restated in float64 in tests/pg_update_cases.py (generic in O and A) with tests/pg_update_gridworld_cases.py's inputs.
#include "pg_update_common.h"

#define GW_TILE 128                 // rows per tile = threads per block of HipPgGwGradients
#define GW_LD (GW_TILE + 4)         // staged arrays are [unit][GW_LD]
#define GW_O 21                     // observation floats of a row
#define GW_IN_STRIDE 24             // floats per row of W0 in LDS and in the packed policy
#define GW_A 5                      // actions
#define GW_OUTPUTS (GW_A + 1)       // staged output deltas: the five logits', then the value's
#define GW_BIAS_SLOTS 8

constexpr int gw_net_floats(int H) { return upd_pg_net_floats(H, GW_O, GW_A); }
// pack_gridworld_policy's block: W0 [H][24], b0, W1, b1, Wp, bp, rounded up to whole 16-byte vectors
constexpr int gw_packed_body(int H) { return H * GW_IN_STRIDE + H + H * H + H + GW_A * H + GW_A; }
constexpr int gw_packed_floats(int H) { return upd_pad4(gw_packed_body(H)); }

// offsets inside the LDS copy
template <int H>
struct GwNet {
  static_assert(H % 4 == 0, "the rows of W0 / W1 / Wp / Wv are read as float4");
  static constexpr int W0 = 0, B0 = H * GW_IN_STRIDE, W1 = B0 + H, B1 = W1 + H * H, WP = B1 + H, BP = WP + GW_A * H;
  static constexpr int WV = BP + GW_BIAS_SLOTS, BV = WV + H;
  static constexpr int LDS = upd_pad4(BV + 1);
  // the flat buffer
  static constexpr int F_B0 = H * GW_O, F_W1 = F_B0 + H, F_B1 = F_W1 + H * H, F_WP = F_B1 + H, F_BP = F_WP + GW_A * H;
  static constexpr int F_WV = F_BP + GW_A, F_BV = F_WV + H, P = F_BV + 1;
  static_assert(P == gw_net_floats(H), "the flat layout");
};

template <int H>
__device__ __forceinline__ void gw_copy_net_to_lds(float *dst, const float *__restrict__ theta) {
  using L = GwNet<H>;
  for (int i = threadIdx.x; i < H * GW_IN_STRIDE; i += blockDim.x) {
    const int r = i / GW_IN_STRIDE, c = i - r * GW_IN_STRIDE;
    dst[i] = c < GW_O ? theta[r * GW_O + c] : 0.0f;
  }
  for (int i = threadIdx.x; i < L::F_WV - L::F_B0; i += blockDim.x) dst[L::B0 + i] = theta[L::F_B0 + i];   // b0 .. bp
  for (int i = threadIdx.x; i < H + 1; i += blockDim.x) dst[L::WV + i] = theta[L::F_WV + i];
}

// h1 = relu(W0 x + b0), x[k] = x_column[k * x_stride].  (Stays here: float4 rows at stride 24 plus a tail; pg_update.hip
// reads float2 rows of O floats.)
template <int H>
__device__ __forceinline__ void gw_layer0(const float *w, const float *x_column, int x_stride, float (&h1)[H]) {
  using L = GwNet<H>;
  float x[GW_O];
#pragma unroll
  for (int k = 0; k < GW_O; ++k) x[k] = x_column[k * x_stride];
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = w[L::B0 + i];
#pragma unroll
    for (int k = 0; k < 20; k += 4) {
      const float4 wr = *(const float4 *)(w + L::W0 + i * GW_IN_STRIDE + k);
      acc = fmaf(wr.x, x[k], acc); acc = fmaf(wr.y, x[k + 1], acc);
      acc = fmaf(wr.z, x[k + 2], acc); acc = fmaf(wr.w, x[k + 3], acc);
    }
    acc = fmaf(w[L::W0 + i * GW_IN_STRIDE + 20], x[20], acc);
    h1[i] = fmaxf(acc, 0.0f);
  }
}

// ------------------------------------------------------------------------------------------------------ 1. values
// obs [rows][21]; values [rows].  Dynamic LDS: GwNet<H>::LDS floats.
template <int H>
__device__ __forceinline__ void gw_values_impl(const float *__restrict__ obs, const float *__restrict__ theta, long rows,
                                               float *__restrict__ values) {
  extern __shared__ __attribute__((aligned(16))) float gw_lds[];
  gw_copy_net_to_lds<H>(gw_lds, theta);
  __syncthreads();
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < rows; g += (long)gridDim.x * blockDim.x) {
    // (the weights are the same for every trip: without this the compiler hoists their LDS reads out of the loop and
    // spills them)
    asm volatile("" ::: "memory");
    float h1[H], h2[H];
    gw_layer0<H>(gw_lds, obs + g * GW_O, 1, h1);
    values[g] = upd_layer1_and_value<H>(gw_lds + GwNet<H>::W1, gw_lds + GwNet<H>::B1, gw_lds + GwNet<H>::WV, h1, h2);
  }
}

// --------------------------------------------------------------------------------------------------- 3. gradients
// What a thread owns of the gradient for the whole launch (128 threads): UpdOwn's share of dW0, db0, dW1, db1, and
//   dWp [5][H], dWv [H]: unit i = tid % H, outputs o = tid / H + KG c (c < OB; o < 5: a logit, o = 5: the value)
//   dbp, dbv: output o = tid (tid < 6);  the four sums: threads 16 .. 19
template <int H>
struct GwOwn : UpdOwn<H, GW_TILE> {
  static constexpr int OB = (GW_OUTPUTS + GwOwn::KG - 1) / GwOwn::KG, KB = (GW_O + GwOwn::KG - 1) / GwOwn::KG;
};

template <int H>
using GwAcc = UpdAcc<GwOwn<H>::JB, GwOwn<H>::KB, GwOwn<H>::OB>;

// dWp[o][i] += sum_r dz[o][r] * h2[i][r]; dWv[i] += sum_r dv[r] * h2[i][r]; dbp[o] += sum_r dz[o][r]; dbv += sum_r dv[r];
// the four sums += their staged per-row terms   (rows ascending; SD = [GW_OUTPUTS][GW_LD], SS = [4][GW_LD]).  (Stays here:
// six output rows, all real; pg_update.hip's are eight logit slots guarded by A, then the value's.)
template <int H>
__device__ __forceinline__ void gw_acc_heads(GwAcc<H> &g, const float *S1, const float *SD, const float *SS) {
  using W = GwOwn<H>;
  const int tid = threadIdx.x, i = tid % H, o0 = tid / H;
#pragma unroll
  for (int c = 0; c < W::OB; ++c) {
    const int o = o0 + W::KG * c;
    if (o < GW_OUTPUTS) {
      float acc = g.wo[c];
      for (int r = 0; r < GW_TILE; r += 4) {
        const float4 h = *(const float4 *)(S1 + i * GW_LD + r), d = *(const float4 *)(SD + o * GW_LD + r);
        acc = fmaf(d.x, h.x, acc); acc = fmaf(d.y, h.y, acc); acc = fmaf(d.z, h.z, acc); acc = fmaf(d.w, h.w, acc);
      }
      g.wo[c] = acc;
    }
  }
  if (tid < GW_OUTPUTS) {
    for (int r = 0; r < GW_TILE; ++r) g.bo += SD[tid * GW_LD + r];
  }
  if (tid >= 16 && tid < 20) {
    for (int r = 0; r < GW_TILE; ++r) g.sum += SS[(tid - 16) * GW_LD + r];
  }
}

// the block's partial, in the FLAT layout: P floats, then the four sums.  (Stays here for its head part.)
template <int H>
__device__ __forceinline__ void gw_write_partial(const GwAcc<H> &g, float *out) {
  using L = GwNet<H>;
  using W = GwOwn<H>;
  constexpr int JB = W::JB, KB = W::KB;
  const int tid = threadIdx.x, ib = tid % W::NIB, jb = tid / W::NIB;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < JB; ++b) out[L::F_W1 + (ib + W::NIB * a) * H + jb + W::NJB * b] = g.w1[a][b];
  const int i = tid % H, k0 = KB * (tid / H), o0 = tid / H;
#pragma unroll
  for (int c = 0; c < KB; ++c)
    if (k0 + c < GW_O) out[i * GW_O + k0 + c] = g.w0[c];
#pragma unroll
  for (int c = 0; c < W::OB; ++c) {
    const int o = o0 + W::KG * c;
    if (o < GW_A) out[L::F_WP + o * H + i] = g.wo[c];
    else if (o == GW_A) out[L::F_WV + i] = g.wo[c];
  }
  if (tid < H) {
    out[L::F_B0 + tid] = g.b0;
    out[L::F_B1 + tid] = g.b1;
  }
  if (tid < GW_A) out[L::F_BP + tid] = g.bo;
  else if (tid == GW_A) out[L::F_BV] = g.bo;
  if (tid >= 16 && tid < 20) out[L::P + tid - 16] = g.sum;
}

// obs [rows][21], actions [rows] int32, adv / ret [rows]; theta flat; partials [gridDim.x][P + 4]: the block's gradient,
// then its sums of logp * adv, of the entropy, of (v - ret)^2 and of adv.  Dynamic LDS: gw_gradients_lds_floats(H)
// floats.  blockDim.x = GW_TILE.
constexpr int gw_gradients_lds_floats(int H) {
  return upd_pad4(H * GW_IN_STRIDE + H + H * H + H + GW_A * H + GW_BIAS_SLOTS + H + 1) + 2 * H * GW_LD + GW_O * GW_LD +
         GW_OUTPUTS * GW_LD + 4 * GW_LD;
}

template <int H>
__device__ __forceinline__ void gw_gradients_impl(const float *__restrict__ obs, const int *__restrict__ actions,
                                                  const float *__restrict__ adv, const float *__restrict__ ret,
                                                  const float *__restrict__ theta, long rows, float inv_R, float ent_coeff,
                                                  float vf_coeff, float *__restrict__ partials) {
  using L = GwNet<H>;
  static_assert(gw_gradients_lds_floats(H) == L::LDS + (2 * H + GW_O + GW_OUTPUTS + 4) * GW_LD, "the LDS carve-up");
  extern __shared__ __attribute__((aligned(16))) float gw_lds[];
  float *w = gw_lds, *S0 = w + L::LDS, *S1 = S0 + H * GW_LD, *S2 = S1 + H * GW_LD, *SD = S2 + GW_O * GW_LD;
  float *SS = SD + GW_OUTPUTS * GW_LD;
  gw_copy_net_to_lds<H>(w, theta);
  const int tid = threadIdx.x;
  const long tiles = (rows + GW_TILE - 1) / GW_TILE;
  const long obs_floats = rows * GW_O;
  GwAcc<H> acc;
  acc.clear();
  __syncthreads();
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long g = tile * GW_TILE + tid;
    const bool live = g < rows;
    // the tile's observation floats, contiguous in memory, transposed into S2 [21][GW_LD] (rows beyond the batch: zeros).
    // (This unit's alone: pg_update.hip's rows of 2 .. 6 floats are loaded by their lanes.)
    {
      const long first = tile * (GW_TILE * GW_O);
      for (int q = tid; q < GW_TILE * GW_O; q += GW_TILE) {
        const int r = q / GW_O, k = q - r * GW_O;
        S2[k * GW_LD + r] = first + q < obs_floats ? obs[first + q] : 0.0f;
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
      float dz[GW_A], dv;
      float h1[H], h2[H];
      gw_layer0<H>(w, S2 + tid, GW_LD, h1);
      const float v = upd_layer1_and_value<H>(w + L::W1, w + L::B1, w + L::WV, h1, h2);
      m1 = upd_positive_mask<H>(h1);
      m2 = upd_positive_mask<H>(h2);
      // the logits: acc = bias, one fmaf per hidden unit in index order
      float z[GW_A], m = -__builtin_inff();
#pragma unroll
      for (int j = 0; j < GW_A; ++j) {
        float s = w[L::BP + j];
#pragma unroll
        for (int i = 0; i < H; i += 4) {
          const float4 wr = *(const float4 *)(w + L::WP + j * H + i);
          s = fmaf(wr.x, h2[i], s); s = fmaf(wr.y, h2[i + 1], s);
          s = fmaf(wr.z, h2[i + 2], s); s = fmaf(wr.w, h2[i + 3], s);
        }
        z[j] = s;
        m = fmaxf(m, s);
      }
      // HipPolicyGradientHead's statements (policy_mlp.hip), one head: the shift by the maximum FIRST (they stay in each
      // unit: see pg_update.hip)
      float total = 0.0f;
#pragma unroll
      for (int j = 0; j < GW_A; ++j) total += expf(z[j] - m);
      const float lse = logf(total);
      float Hent = 0.0f;
#pragma unroll
      for (int j = 0; j < GW_A; ++j) {
        const float lp = (z[j] - m) - lse;
        Hent -= expf(lp) * lp;
      }
      const int clamped = min(max(taken, 0), GW_A - 1);
      float logp_taken = 0.0f;
#pragma unroll
      for (int j = 0; j < GW_A; ++j)
        if (j == clamped) logp_taken = (z[j] - m) - lse;
#pragma unroll
      for (int j = 0; j < GW_A; ++j) {
        dz[j] = 0.0f;
        if (live) {
          const float lp = (z[j] - m) - lse, pj = expf(lp);
          dz[j] = (a * (pj - (j == taken ? 1.0f : 0.0f)) + ent_coeff * pj * (lp + Hent)) * inv_R;
        }
      }
      const float d = v - rt;
      dv = live ? 2.0f * vf_coeff * d * inv_R : 0.0f;
      upd_stage<H, GW_LD>(S0, tid, h1);
      upd_stage<H, GW_LD>(S1, tid, h2);
#pragma unroll
      for (int j = 0; j < GW_A; ++j) SD[j * GW_LD + tid] = dz[j];
      SD[GW_A * GW_LD + tid] = dv;
      SS[0 * GW_LD + tid] = live ? logp_taken * a : 0.0f;
      SS[1 * GW_LD + tid] = live ? Hent : 0.0f;
      SS[2 * GW_LD + tid] = live ? d * d : 0.0f;
      SS[3 * GW_LD + tid] = live ? a : 0.0f;
    }
    __syncthreads();
    gw_acc_heads<H>(acc, S1, SD, SS);
    __syncthreads();
    {
      // d2[i] = relu'(h2[i]) * (sum_j dz[j] Wp[j][i] + dv Wv[i]), j ascending from +0, the value last (the deltas read
      // back from the lane's own staged column).  Four units at a time, staged as they are formed: with all H sums in
      // flight at once (pg_update.hip's form) the compiler splits the weight rows into 8-byte reads at addresses of their
      // own and spills.
      float dz[GW_A];
#pragma unroll
      for (int j = 0; j < GW_A; ++j) dz[j] = SD[j * GW_LD + tid];
      const float dv = SD[GW_A * GW_LD + tid];
#pragma unroll
      for (int i = 0; i < H; i += 4) {
        float d2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int j = 0; j < GW_A; ++j) {
          const float4 wr = *(const float4 *)(w + L::WP + j * H + i);
          d2[0] = fmaf(wr.x, dz[j], d2[0]); d2[1] = fmaf(wr.y, dz[j], d2[1]);
          d2[2] = fmaf(wr.z, dz[j], d2[2]); d2[3] = fmaf(wr.w, dz[j], d2[3]);
        }
        const float4 wr = *(const float4 *)(w + L::WV + i);
        d2[0] = fmaf(wr.x, dv, d2[0]); d2[1] = fmaf(wr.y, dv, d2[1]);
        d2[2] = fmaf(wr.z, dv, d2[2]); d2[3] = fmaf(wr.w, dv, d2[3]);
#pragma unroll
        for (int c = 0; c < 4; ++c) S1[(i + c) * GW_LD + tid] = ((m2 >> (i + c)) & 1ull) ? d2[c] : 0.0f;
      }
    }
    __syncthreads();
    upd_acc_w1<H, GW_TILE, GW_LD>(acc, S0, S1);
    {
      float d1[H];
      upd_layer1_backward<H, GW_LD>(w + L::W1, S1 + tid, m1, d1);
      __syncthreads();
      upd_stage<H, GW_LD>(S1, tid, d1);
    }
    __syncthreads();
    upd_acc_w0<H, GW_TILE, GW_LD, GW_O>(acc, S1, S2);
    __syncthreads();
  }
  gw_write_partial<H>(acc, partials + (long)blockIdx.x * (L::P + 4));
}

// ------------------------------------------------------------------------------------------- 4 and 5: reduce, apply
__device__ __forceinline__ bool gw_width_ok(int H) { return H == 32 || H == 64; }

#define GW_REDUCE_THREADS 1024

extern "C" {

#define GW_ENTRIES(HH)                                                                                                 \
  __global__ void __launch_bounds__(256) HipPgGwValues_H##HH(const float *__restrict__ obs,                            \
                                                             const float *__restrict__ theta, long rows,               \
                                                             float *__restrict__ values) {                             \
    gw_values_impl<HH>(obs, theta, rows, values);                                                                      \
  }                                                                                                                    \
  __global__ void __launch_bounds__(GW_TILE) HipPgGwGradients_H##HH(                                                   \
      const float *__restrict__ obs, const int *__restrict__ actions, const float *__restrict__ adv,                   \
      const float *__restrict__ ret, const float *__restrict__ theta, long rows, float inv_R, float ent_coeff,         \
      float vf_coeff, float *__restrict__ partials) {                                                                  \
    gw_gradients_impl<HH>(obs, actions, adv, ret, theta, rows, inv_R, ent_coeff, vf_coeff, partials);                  \
  }
GW_ENTRIES(32)
GW_ENTRIES(64)

// upd_pg_reduce on grid = 9 blocks of GW_REDUCE_THREADS.  (A width other than 32 / 64: touches nothing.)
__global__ void __launch_bounds__(GW_REDUCE_THREADS) HipPgGwReduce(const float *__restrict__ partials, int n_blocks, int H,
                                                                   float *__restrict__ grads, float *__restrict__ sumsq,
                                                                   float *__restrict__ sums) {
  __shared__ float tree[GW_REDUCE_THREADS];
  if (!gw_width_ok(H)) return;
  upd_pg_reduce<GW_REDUCE_THREADS>(tree, partials, n_blocks, gw_net_floats(H), H, GW_O, GW_A, grads, sumsq, sums);
}

// One thread per float of max(P, the packed block).  theta / exp_avg / exp_avg_sq / grads: P floats.
//   clip over the eight tensor norms and Adam: upd_clip_adam
//   packed the rollout's copy of the policy in pack_gridworld_policy's layout (gw_packed_floats(H) floats) or null:
//          thread idx < P - H - 1 writes its parameter where that layout has it (W0 [r][c] at r * 24 + c, the rest 3 H
//          further on than in the flat buffer); thread idx < gw_packed_floats(H) writes +0 if float idx of the block is a
//          pad column of W0 or the tail.  Every float of the block is written by exactly one thread.  (This refill is
//          the unit's own: pg_update.hip's packed policy is a prefix of the flat buffer.)
__global__ void __launch_bounds__(256) HipPgGwApply(float *__restrict__ theta, float *__restrict__ exp_avg,
                                                    float *__restrict__ exp_avg_sq, const float *__restrict__ grads,
                                                    const float *__restrict__ sumsq, float *__restrict__ packed, int H,
                                                    float max_norm, float step_size, float bc2_sqrt, float one_minus_beta1,
                                                    float beta2, float one_minus_beta2, float eps) {
  if (!gw_width_ok(H)) return;
  const int P = gw_net_floats(H);
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (packed != nullptr && idx < gw_packed_floats(H)) {
    const bool pad = idx < H * GW_IN_STRIDE ? (idx % GW_IN_STRIDE) >= GW_O : idx >= gw_packed_body(H);
    if (pad) packed[idx] = 0.0f;
  }
  if (idx >= P) return;
  const float p = upd_clip_adam(idx, theta, exp_avg, exp_avg_sq, grads, sumsq, 8, max_norm, step_size, bc2_sqrt,
                                one_minus_beta1, beta2, one_minus_beta2, eps);
  if (packed != nullptr && idx < P - H - 1) {
    const int w0 = H * GW_O;
    packed[idx < w0 ? (idx / GW_O) * GW_IN_STRIDE + idx % GW_O : idx + H * (GW_IN_STRIDE - GW_O)] = p;
  }
}

}  // extern "C"
