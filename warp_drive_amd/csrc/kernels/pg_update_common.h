// pg_update_common.h -- what the update units share: pg_update.hip (Cartpole, Acrobot, MountainCar), pg_update_gridworld.hip
// (TagGridWorld's tagger and runner) and ddpg_update.hip (Pendulum, ContinuousMountainCar).  Templates on the hidden width H,
// the tile TILE (rows per tile = threads per block of a gradients entry) and the row stride LD of the arrays staged in LDS;
// nothing here reads a unit's macros.  A unit is its network layout, its first layer, its heads and its entries around this.
//
// THE PARITY CONTRACT of the update kernels, stated here once:
//   * Summation order.  Per block and per tile (grid-stride over the tiles) every lane runs the forward and backward
//     passes of its row and stages what the parameter gradients need -- activations, deltas -- in LDS, unit-major
//     ([unit][LD]: rows of 16-byte multiples, units 4 banks apart, a lane's stores conflict-free); then every thread adds
//     the tile's rows, in row order, to the FIXED set of gradient entries it owns for the whole launch (UpdOwn).  A block
//     accumulates every entry in one fixed order (tiles ascending, rows ascending) and writes its partial once; blocks
//     without rows write zeros.  The reduce launch sums the partials in block order, and a tensor's sum of squares per
//     thread over its elements in ascending order, then in a pairwise tree over the threads.
//   * relu'(0) = 0: a unit passes a delta on where its activation is > 0 (upd_positive_mask).
//   * No float atomics, no cross-block communication inside a launch, nothing read back by the host.
//   * clip_grad_norm_: max_norm > 0: g *= min(1, max_norm / (norm + 1e-6)), norm = the 2-norm of the tensors' norms.
//   * torch.optim.Adam's default expression: m = lerp(m, g, 1 - beta1); v = v beta2 + (1 - beta2) g g;
//     denom = sqrt(v) / bc2_sqrt + eps; p = p - step_size (m / denom), with step_size = lr / (1 - beta1^step) and
//     bc2_sqrt = sqrt(1 - beta2^step) from the host.
//   * Forward arithmetic: acc = bias, then one fmaf per input in index order, fmaxf(acc, 0); the weights in LDS read as
//     broadcasts, one row per lane.  The objective's statements are policy_mlp.hip::HipPolicyGradientHead's.
// Restated in float64 in tests/pg_update_cases.py and tests/ddpg_update_cases.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int upd_pad4(int n) { return (n + 3) & ~3; }

// h2 = relu(W1 h1 + b1), returns v = Wv h2 + bv; `wv` = the H floats of Wv, then bv
template <int H>
__device__ __forceinline__ float upd_layer1_and_value(const float *W1, const float *b1, const float *wv, const float (&h1)[H],
                                                      float (&h2)[H]) {
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = b1[i];
#pragma unroll
    for (int j = 0; j < H; j += 4) {
      const float4 wr = *(const float4 *)(W1 + i * H + j);
      acc = fmaf(wr.x, h1[j], acc); acc = fmaf(wr.y, h1[j + 1], acc);
      acc = fmaf(wr.z, h1[j + 2], acc); acc = fmaf(wr.w, h1[j + 3], acc);
    }
    h2[i] = fmaxf(acc, 0.0f);
  }
  float v = wv[H];
#pragma unroll
  for (int j = 0; j < H; j += 4) {
    const float4 wr = *(const float4 *)(wv + j);
    v = fmaf(wr.x, h2[j], v); v = fmaf(wr.y, h2[j + 1], v);
    v = fmaf(wr.z, h2[j + 2], v); v = fmaf(wr.w, h2[j + 3], v);
  }
  return v;
}

template <int H>
__device__ __forceinline__ uint64_t upd_positive_mask(const float (&h)[H]) {
  uint64_t m = 0;
#pragma unroll
  for (int i = 0; i < H; ++i) m |= (h[i] > 0.0f) ? (1ull << i) : 0ull;
  return m;
}

template <int H, int LD>
__device__ __forceinline__ void upd_stage(float *S, int row, const float (&h)[H]) {
#pragma unroll
  for (int i = 0; i < H; ++i) S[i * LD + row] = h[i];
}

// d1[j] = relu'(h1[j]) * sum_i W1[i][j] d2[i], i ascending from +0; d2[i] is read from the lane's own staged column
// (no second H-wide array in registers)
template <int H, int LD>
__device__ __forceinline__ void upd_layer1_backward(const float *W1, const float *d2_column, uint64_t mask1, float (&d1)[H]) {
#pragma unroll
  for (int j = 0; j < H; ++j) d1[j] = 0.0f;
#pragma unroll
  for (int i = 0; i < H; ++i) {
    const float d2 = d2_column[i * LD];
#pragma unroll
    for (int j = 0; j < H; j += 4) {
      const float4 wr = *(const float4 *)(W1 + i * H + j);
      d1[j] = fmaf(wr.x, d2, d1[j]); d1[j + 1] = fmaf(wr.y, d2, d1[j + 1]);
      d1[j + 2] = fmaf(wr.z, d2, d1[j + 2]); d1[j + 3] = fmaf(wr.w, d2, d1[j + 3]);
    }
  }
#pragma unroll
  for (int j = 0; j < H; ++j) d1[j] = ((mask1 >> j) & 1ull) ? d1[j] : 0.0f;
}

// What a thread owns of the two hidden layers' gradient for the whole launch (TILE threads):
//   dW1 [H][H]: rows i = ib + NIB a (a < 4), columns j = jb + NJB b (b < JB), ib = tid % NIB, jb = tid / NIB
//   dW0 [H][I]: row i = tid % H, columns k = KB (tid / H) + c (c < KB = ceil(I / KG), k < I)
//   db0, db1: unit i = tid (tid < H)
// (its share of the heads' gradient is the unit's own)
template <int H, int TILE>
struct UpdOwn {
  static constexpr int NIB = H / 4, NJB = TILE / NIB, JB = H / NJB, KG = TILE / H;
  static_assert(NIB * NJB == TILE && NJB * JB == H && KG * H == TILE, "ownership covers the matrix exactly");
};

// the accumulators of a network with OB_ head outputs per thread, one bias output and one of the block's sums
template <int JB_, int KB_, int OB_>
struct UpdAcc {
  static constexpr int JB = JB_, KB = KB_, OB = OB_;
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

// dW1[i][j] += sum_r d2[i][r] * h1[j][r]; db1[i] += sum_r d2[i][r]   (Acc: w1 [4][JB] and b1)
template <int H, int TILE, int LD, class Acc>
__device__ __forceinline__ void upd_acc_w1(Acc &g, const float *S0, const float *S1) {
  using W = UpdOwn<H, TILE>;
  constexpr int JB = W::JB;
  const int tid = threadIdx.x, ib = tid % W::NIB, jb = tid / W::NIB;
  for (int r = 0; r < TILE; r += 4) {
    float4 d[4], h[JB];
#pragma unroll
    for (int a = 0; a < 4; ++a) d[a] = *(const float4 *)(S1 + (ib + W::NIB * a) * LD + r);
#pragma unroll
    for (int b = 0; b < JB; ++b) h[b] = *(const float4 *)(S0 + (jb + W::NJB * b) * LD + r);
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
    for (int r = 0; r < TILE; r += 4) {
      const float4 d = *(const float4 *)(S1 + tid * LD + r);
      g.b1 += d.x; g.b1 += d.y; g.b1 += d.z; g.b1 += d.w;
    }
  }
}

// dW0[i][k] += sum_r d1[i][r] * x[k][r]; db0[i] += sum_r d1[i][r]   (x staged as [I][LD]; Acc: w0 [Acc::KB] and b0)
template <int H, int TILE, int LD, int I, class Acc>
__device__ __forceinline__ void upd_acc_w0(Acc &g, const float *S1, const float *S2) {
  constexpr int KB = Acc::KB;
  const int tid = threadIdx.x, i = tid % H, k0 = KB * (tid / H);
  for (int r = 0; r < TILE; r += 4) {
    const float4 d = *(const float4 *)(S1 + i * LD + r);
#pragma unroll
    for (int c = 0; c < KB; ++c) {
      if (k0 + c < I) {
        const float4 x = *(const float4 *)(S2 + (k0 + c) * LD + r);
        float acc = g.w0[c];
        acc = fmaf(d.x, x.x, acc); acc = fmaf(d.y, x.y, acc); acc = fmaf(d.z, x.z, acc); acc = fmaf(d.w, x.w, acc);
        g.w0[c] = acc;
      }
    }
  }
  if (tid < H) {
    for (int r = 0; r < TILE; r += 4) {
      const float4 d = *(const float4 *)(S1 + tid * LD + r);
      g.b0 += d.x; g.b0 += d.y; g.b0 += d.z; g.b0 += d.w;
    }
  }
}

// ------------------------------------------------------------------------------- the reduce and apply launches
constexpr int upd_pg_net_floats(int H, int O, int A) { return H * O + H + H * H + H + A * H + A + H + 1; }

// the eight parameter tensors of a policy inside its flat P floats: W0 [H][O], b0, W1 [H][H], b1, Wp [A][H], bp, Wv, bv
struct UpdTensor { int off, n; };

__device__ __forceinline__ UpdTensor upd_pg_tensor(int k, int H, int O, int A) {
  const int n[8] = {H * O, H, H * H, H, A * H, A, H, 1};
  int off = 0;
  for (int j = 0; j < k; ++j) off += n[j];
  return {off, n[k]};
}

// One block of a reduce entry: tensor t of the n_blocks partials (rows of `stride` floats) summed in block order into
// grads, and the tensor's sum of squares to sumsq[blockIdx.x].  `tree`: THREADS floats of LDS.
template <int THREADS>
__device__ __forceinline__ void upd_reduce_tensor(float *tree, const float *__restrict__ partials, int n_blocks, long stride,
                                                  UpdTensor t, float *__restrict__ grads, float *__restrict__ sumsq) {
  const int tid = threadIdx.x;
  float sq = 0.0f;
  for (int e = tid; e < t.n; e += THREADS) {
    float s = 0.0f;
    for (int b = 0; b < n_blocks; ++b) s += partials[b * stride + t.off + e];
    grads[t.off + e] = s;
    sq += s * s;
  }
  tree[tid] = sq;
  __syncthreads();
  for (int half = THREADS / 2; half > 0; half >>= 1) {
    if (tid < half) tree[tid] += tree[tid + half];
    __syncthreads();
  }
  if (tid == 0) sumsq[blockIdx.x] = tree[0];
}

// The body of a policy's reduce entry.  grid = 9 blocks of THREADS: block k < 8 sums tensor k of the n_blocks partials
// (rows of P + 4 floats) into grads [P] and writes the tensor's sum of squares; block 8 writes sums [4] = the four
// sums over the blocks.  `tree`: THREADS floats of LDS; P = upd_pg_net_floats(H, O, A).
template <int THREADS>
__device__ __forceinline__ void upd_pg_reduce(float *tree, const float *__restrict__ partials, int n_blocks, int P, int H,
                                              int O, int A, float *__restrict__ grads, float *__restrict__ sumsq,
                                              float *__restrict__ sums) {
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
  upd_reduce_tensor<THREADS>(tree, partials, n_blocks, stride, upd_pg_tensor(blockIdx.x, H, O, A), grads, sumsq);
}

// Parameter idx of a network of n_tensors tensors: the clip over sumsq [n_tensors], the Adam step; writes theta, exp_avg
// and exp_avg_sq and returns the new parameter (the caller refills its packed policy with it)
__device__ __forceinline__ float upd_clip_adam(int idx, float *__restrict__ theta, float *__restrict__ exp_avg,
                                               float *__restrict__ exp_avg_sq, const float *__restrict__ grads,
                                               const float *__restrict__ sumsq, int n_tensors, float max_norm,
                                               float step_size, float bc2_sqrt, float one_minus_beta1, float beta2,
                                               float one_minus_beta2, float eps) {
  float g = grads[idx];
  if (max_norm > 0.0f) {
    float total = 0.0f;
    for (int k = 0; k < n_tensors; ++k) {
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
  return p;
}
