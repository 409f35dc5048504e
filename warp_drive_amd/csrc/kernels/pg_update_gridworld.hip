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
// No float atomics, no cross-block communication inside a launch, nothing read back by the host.
//
// The network FLAT, in the order of the module's parameters (the parameters are views of it: FlatPolicy): W0 [H][21]
// (unpadded), b0 [H], W1 [H][H], b1 [H], Wp [5][H], bp [5], Wv [H], bv [1].  In LDS the rows of W0 are GW_IN_STRIDE = 24
// floats apart (tag_gridworld_n5_common.h's GW5_IN_STRIDE: every row starts on a 16-byte boundary), the three pad columns
// zero, and the value head starts on a 16-byte boundary behind eight bias slots.
//
// Forward arithmetic is gw5_policy_probs' (the same header): acc = bias, then one fmaf per input in index order, fmaxf(acc, 0).  relu'(0) = 0.
// The probabilities are not claimed bit-identical to the rollout's.
//
// Stage 3 keeps pg_update.hip's structure: a tile of 128 rows per 128-thread block, activations and deltas staged
// unit-major in LDS, every thread owning a fixed set of gradient entries for the whole launch (tiles ascending, rows
// ascending: one fixed summation order), one partial per block, zeros from a block without rows.  One thing differs: a
// tile's 128 x 21 observation floats are contiguous in memory, so the block loads them with coalesced loads and writes
// them transposed into the staged [21][LD] array FIRST, and the forward reads the lane's own column from there (no
// observation registers live across the backward pass; no 84-byte-strided loads).
//
// Restated in float64 in tests/pg_update_cases.py (generic in O and A) with tests/pg_update_gridworld_cases.py's inputs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GW_TILE 128                 // rows per tile = threads per block of HipPgGwGradients
#define GW_LD (GW_TILE + 4)         // staged arrays are [unit][GW_LD]
#define GW_O 21                     // observation floats of a row
#define GW_IN_STRIDE 24             // floats per row of W0 in LDS and in the packed policy
#define GW_A 5                      // actions
#define GW_OUTPUTS (GW_A + 1)       // staged output deltas: the five logits', then the value's
#define GW_BIAS_SLOTS 8

constexpr int gw_net_floats(int H) { return H * GW_O + H + H * H + H + GW_A * H + GW_A + H + 1; }
constexpr int gw_pad4(int n) { return (n + 3) & ~3; }
// pack_gridworld_policy's block: W0 [H][24], b0, W1, b1, Wp, bp, rounded up to whole 16-byte vectors
constexpr int gw_packed_body(int H) { return H * GW_IN_STRIDE + H + H * H + H + GW_A * H + GW_A; }
constexpr int gw_packed_floats(int H) { return gw_pad4(gw_packed_body(H)); }

// offsets inside the LDS copy
template <int H>
struct GwNet {
  static_assert(H % 4 == 0, "the rows of W0 / W1 / Wp / Wv are read as float4");
  static constexpr int W0 = 0, B0 = H * GW_IN_STRIDE, W1 = B0 + H, B1 = W1 + H * H, WP = B1 + H, BP = WP + GW_A * H;
  static constexpr int WV = BP + GW_BIAS_SLOTS, BV = WV + H;
  static constexpr int LDS = gw_pad4(BV + 1);
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

// h1 = relu(W0 x + b0), x[k] = x_column[k * x_stride]
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

// h2 = relu(W1 h1 + b1), returns v = Wv h2 + bv
template <int H>
__device__ __forceinline__ float gw_layer1_and_value(const float *w, const float (&h1)[H], float (&h2)[H]) {
  using L = GwNet<H>;
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = w[L::B1 + i];
#pragma unroll
    for (int j = 0; j < H; j += 4) {
      const float4 wr = *(const float4 *)(w + L::W1 + i * H + j);
      acc = fmaf(wr.x, h1[j], acc); acc = fmaf(wr.y, h1[j + 1], acc);
      acc = fmaf(wr.z, h1[j + 2], acc); acc = fmaf(wr.w, h1[j + 3], acc);
    }
    h2[i] = fmaxf(acc, 0.0f);
  }
  float v = w[L::BV];
#pragma unroll
  for (int j = 0; j < H; j += 4) {
    const float4 wr = *(const float4 *)(w + L::WV + j);
    v = fmaf(wr.x, h2[j], v); v = fmaf(wr.y, h2[j + 1], v);
    v = fmaf(wr.z, h2[j + 2], v); v = fmaf(wr.w, h2[j + 3], v);
  }
  return v;
}

template <int H>
__device__ __forceinline__ uint64_t gw_positive_mask(const float (&h)[H]) {
  uint64_t m = 0;
#pragma unroll
  for (int i = 0; i < H; ++i) m |= (h[i] > 0.0f) ? (1ull << i) : 0ull;
  return m;
}

// d1[j] = relu'(h1[j]) * sum_i W1[i][j] d2[i], i ascending from +0; d2[i] read from the lane's own staged column
template <int H>
__device__ __forceinline__ void gw_layer1_backward(const float *w, const float *d2_column, uint64_t mask1, float (&d1)[H]) {
  using L = GwNet<H>;
#pragma unroll
  for (int j = 0; j < H; ++j) d1[j] = 0.0f;
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const float d2 = d2_column[i * GW_LD];
#pragma unroll
    for (int j = 0; j < H; j += 4) {
      const float4 wr = *(const float4 *)(w + L::W1 + i * H + j);
      d1[j] = fmaf(wr.x, d2, d1[j]); d1[j + 1] = fmaf(wr.y, d2, d1[j + 1]);
      d1[j + 2] = fmaf(wr.z, d2, d1[j + 2]); d1[j + 3] = fmaf(wr.w, d2, d1[j + 3]);
    }
  }
#pragma unroll
  for (int j = 0; j < H; ++j) d1[j] = ((mask1 >> j) & 1ull) ? d1[j] : 0.0f;
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
    values[g] = gw_layer1_and_value<H>(gw_lds, h1, h2);
  }
}

// --------------------------------------------------------------------------------------------------- 3. gradients
// What a thread owns of the gradient for the whole launch (128 threads):
//   dW1 [H][H]: rows i = ib + NIB a (a < 4), columns j = jb + NJB b (b < JB), ib = tid % NIB, jb = tid / NIB
//   dW0 [H][21]: row i = tid % H, columns k = KB (tid / H) + c (c < KB, k < 21)
//   dWp [5][H], dWv [H]: unit i = tid % H, outputs o = tid / H + KG c (c < OB; o < 5: a logit, o = 5: the value)
//   db0, db1: unit i = tid (tid < H);  dbp, dbv: output o = tid (tid < 6);  the four sums: threads 16 .. 19
template <int H>
struct GwOwn {
  static constexpr int NIB = H / 4, NJB = GW_TILE / NIB, JB = H / NJB, KG = GW_TILE / H;
  static constexpr int OB = (GW_OUTPUTS + KG - 1) / KG, KB = (GW_O + KG - 1) / KG;
  static_assert(NIB * NJB == GW_TILE && NJB * JB == H && KG * H == GW_TILE, "ownership covers the matrix exactly");
};

template <int H>
struct GwAcc {
  static constexpr int JB = GwOwn<H>::JB, KB = GwOwn<H>::KB, OB = GwOwn<H>::OB;
  float w1[4][JB], w0[KB], wo[OB], b0, b1, bo, sum;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < JB; ++b) w1[a][b] = 0.0f;
#pragma unroll
    for (int c = 0; c < KB; ++c) w0[c] = 0.0f;
#pragma unroll
    for (int c = 0; c < OB; ++c) wo[c] = 0.0f;
    b0 = b1 = bo = sum = 0.0f;
  }
};

// dWp[o][i] += sum_r dz[o][r] * h2[i][r]; dWv[i] += sum_r dv[r] * h2[i][r]; dbp[o] += sum_r dz[o][r]; dbv += sum_r dv[r];
// the four sums += their staged per-row terms   (rows ascending; SD = [GW_OUTPUTS][GW_LD], SS = [4][GW_LD])
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

// dW1[i][j] += sum_r d2[i][r] * h1[j][r]; db1[i] += sum_r d2[i][r]
template <int H>
__device__ __forceinline__ void gw_acc_w1(GwAcc<H> &g, const float *S0, const float *S1) {
  using W = GwOwn<H>;
  constexpr int JB = W::JB;
  const int tid = threadIdx.x, ib = tid % W::NIB, jb = tid / W::NIB;
  for (int r = 0; r < GW_TILE; r += 4) {
    float4 d[4], h[JB];
#pragma unroll
    for (int a = 0; a < 4; ++a) d[a] = *(const float4 *)(S1 + (ib + W::NIB * a) * GW_LD + r);
#pragma unroll
    for (int b = 0; b < JB; ++b) h[b] = *(const float4 *)(S0 + (jb + W::NJB * b) * GW_LD + r);
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < JB; ++b) {
        float acc = g.w1[a][b];
        acc = fmaf(d[a].x, h[b].x, acc); acc = fmaf(d[a].y, h[b].y, acc);
        acc = fmaf(d[a].z, h[b].z, acc); acc = fmaf(d[a].w, h[b].w, acc);
        g.w1[a][b] = acc;
      }
  }
  if (tid < H) {
    for (int r = 0; r < GW_TILE; r += 4) {
      const float4 d = *(const float4 *)(S1 + tid * GW_LD + r);
      g.b1 += d.x; g.b1 += d.y; g.b1 += d.z; g.b1 += d.w;
    }
  }
}

// dW0[i][k] += sum_r d1[i][r] * x[k][r]; db0[i] += sum_r d1[i][r]   (x staged as [21][GW_LD])
template <int H>
__device__ __forceinline__ void gw_acc_w0(GwAcc<H> &g, const float *S1, const float *S2) {
  constexpr int KB = GwOwn<H>::KB;
  const int tid = threadIdx.x, i = tid % H, k0 = KB * (tid / H);
  for (int r = 0; r < GW_TILE; r += 4) {
    const float4 d = *(const float4 *)(S1 + i * GW_LD + r);
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      if (k0 + c < GW_O) {
        const float4 x = *(const float4 *)(S2 + (k0 + c) * GW_LD + r);
        float acc = g.w0[c];
        acc = fmaf(d.x, x.x, acc); acc = fmaf(d.y, x.y, acc); acc = fmaf(d.z, x.z, acc); acc = fmaf(d.w, x.w, acc);
        g.w0[c] = acc;
      }
    }
  }
  if (tid < H) {
    for (int r = 0; r < GW_TILE; r += 4) {
      const float4 d = *(const float4 *)(S1 + tid * GW_LD + r);
      g.b0 += d.x; g.b0 += d.y; g.b0 += d.z; g.b0 += d.w;
    }
  }
}

// the block's partial, in the FLAT layout: P floats, then the four sums
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

template <int H>
__device__ __forceinline__ void gw_stage(float *S, int row, const float (&h)[H]) {
#pragma unroll
  for (int i = 0; i < H; ++i) S[i * GW_LD + row] = h[i];
}

// obs [rows][21], actions [rows] int32, adv / ret [rows]; theta flat; partials [gridDim.x][P + 4]: the block's gradient,
// then its sums of logp * adv, of the entropy, of (v - ret)^2 and of adv.  Dynamic LDS: gw_gradients_lds_floats(H)
// floats.  blockDim.x = GW_TILE.
constexpr int gw_gradients_lds_floats(int H) {
  return gw_pad4(H * GW_IN_STRIDE + H + H * H + H + GW_A * H + GW_BIAS_SLOTS + H + 1) + 2 * H * GW_LD + GW_O * GW_LD +
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
    // the tile's observation floats, contiguous in memory, transposed into S2 [21][GW_LD] (rows beyond the batch: zeros)
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
      const float v = gw_layer1_and_value<H>(w, h1, h2);
      m1 = gw_positive_mask<H>(h1);
      m2 = gw_positive_mask<H>(h2);
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
      // HipPolicyGradientHead's statements (policy_mlp.hip), one head: the shift by the maximum FIRST
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
      gw_stage<H>(S0, tid, h1);
      gw_stage<H>(S1, tid, h2);
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
      // flight at once the compiler splits the weight rows into 8-byte reads at addresses of their own and spills.
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
    gw_acc_w1<H>(acc, S0, S1);
    {
      float d1[H];
      gw_layer1_backward<H>(w, S1 + tid, m1, d1);
      __syncthreads();
      gw_stage<H>(S1, tid, d1);
    }
    __syncthreads();
    gw_acc_w0<H>(acc, S1, S2);
    __syncthreads();
  }
  gw_write_partial<H>(acc, partials + (long)blockIdx.x * (L::P + 4));
}

// -------------------------------------------------------------------------------------------------- 4 and 5: layout
// the eight parameter tensors inside the flat P floats
struct GwTensor { int off, n; };

__device__ __forceinline__ GwTensor gw_tensor(int k, int H) {
  const int n[8] = {H * GW_O, H, H * H, H, GW_A * H, GW_A, H, 1};
  int off = 0;
  for (int j = 0; j < k; ++j) off += n[j];
  return {off, n[k]};
}

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

// grid = 9 blocks of GW_REDUCE_THREADS: block k < 8 sums tensor k of the n_blocks partials (rows of P + 4 floats) in
// block order into grads [P] and writes the tensor's sum of squares (per thread over its elements in ascending order,
// then a pairwise tree over the threads: a fixed order); block 8 writes sums [4] = the four sums over the blocks, in
// block order.  (A width other than 32 / 64: touches nothing.)
__global__ void __launch_bounds__(GW_REDUCE_THREADS) HipPgGwReduce(const float *__restrict__ partials, int n_blocks, int H,
                                                                   float *__restrict__ grads, float *__restrict__ sumsq,
                                                                   float *__restrict__ sums) {
  __shared__ float tree[GW_REDUCE_THREADS];
  if (!gw_width_ok(H)) return;
  const int P = gw_net_floats(H);
  const long stride = P + 4;
  const int tid = threadIdx.x;
  if (blockIdx.x >= 8) {
    if (blockIdx.x == 8 && tid < 4) {
      float s = 0.0f;
      for (int b = 0; b < n_blocks; ++b) s += partials[b * stride + P + tid];
      sums[tid] = s;
    }
    return;
  }
  const GwTensor t = gw_tensor(blockIdx.x, H);
  float sq = 0.0f;
  for (int e = tid; e < t.n; e += GW_REDUCE_THREADS) {
    float s = 0.0f;
    for (int b = 0; b < n_blocks; ++b) s += partials[b * stride + t.off + e];
    grads[t.off + e] = s;
    sq += s * s;
  }
  tree[tid] = sq;
  __syncthreads();
  for (int half = GW_REDUCE_THREADS / 2; half > 0; half >>= 1) {
    if (tid < half) tree[tid] += tree[tid + half];
    __syncthreads();
  }
  if (tid == 0) sumsq[blockIdx.x] = tree[0];
}

// One thread per float of max(P, the packed block).  theta / exp_avg / exp_avg_sq / grads: P floats.
//   clip   max_norm > 0: g *= min(1, max_norm / (norm + 1e-6)), norm = the 2-norm of the eight tensor norms
//   Adam   m = lerp(m, g, 1 - beta1); v = v beta2 + (1 - beta2) g g; denom = sqrt(v) / bc2_sqrt + eps;
//          p = p - step_size (m / denom), step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) from the host
//   packed the rollout's copy of the policy in pack_gridworld_policy's layout (gw_packed_floats(H) floats) or null:
//          thread idx < P - H - 1 writes its parameter where that layout has it (W0 [r][c] at r * 24 + c, the rest 3 H
//          further on than in the flat buffer); thread idx < gw_packed_floats(H) writes +0 if float idx of the block is a
//          pad column of W0 or the tail.  Every float of the block is written by exactly one thread.
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
  float g = grads[idx];
  if (max_norm > 0.0f) {
    float total = 0.0f;
    for (int k = 0; k < 8; ++k) {
      const float norm = sqrtf(sumsq[k]);
      total += norm * norm;
    }
    const float coef = fminf(max_norm / (sqrtf(total) + 1e-6f), 1.0f);
    g *= coef;
  }
  const float m0 = exp_avg[idx];
  const float m = fmaf(one_minus_beta1, g - m0, m0);
  const float v = fmaf(one_minus_beta2, g * g, exp_avg_sq[idx] * beta2);
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  const float p = fmaf(-step_size, m / denom, theta[idx]);
  exp_avg[idx] = m;
  exp_avg_sq[idx] = v;
  theta[idx] = p;
  if (packed != nullptr && idx < P - H - 1) {
    const int w0 = H * GW_O;
    packed[idx < w0 ? (idx / GW_O) * GW_IN_STRIDE + idx % GW_O : idx + H * (GW_IN_STRIDE - GW_O)] = p;
  }
}

}  // extern "C"
