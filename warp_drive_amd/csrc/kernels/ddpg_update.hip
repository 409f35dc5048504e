// ddpg_update.hip -- the update of TrainerDDPG (training/trainer_ddpg.py, `trainer.fused_update: true`) as FOUR launches:
//
//   1. HipDdpgTargets_H<H>_O<O>    next_value[t, e] = Q'(obs[t + 1, e], mu'(obs[t + 1, e])) for the T - 1 rows that have a
//                                  next row, with the two TARGET networks; one thread per row, grid-stride.
//   2. HipDdpgGradients_H<H>_O<O>  prologue: the n-step return of every valid row (t < V = T - n_step + 1), the expression
//                                  of training/losses.py::DDPG.n_step_returns operation for operation; then the gradient of
//                                  mse_loss(returns, Q(obs, action)) with respect to the critic and of -mean(Q(obs, mu(obs)))
//                                  with respect to the ACTOR only (the critic is differentiated with respect to its action
//                                  input alone), as one partial per block, plus the block's two loss sums.
//   3. HipDdpgReduce               the blocks' partials summed in block order into the flat gradient, the sum of squares of
//                                  every parameter tensor, and the two losses.
//   4. HipDdpgApply                clip_grad_norm_ per network, torch.optim.Adam's default expression, the soft update of
//                                  both targets, and the refill of the packed actor the rollout kernels read.
//
// The summation order, relu'(0) = 0, "no float atomics, nothing read back" and the clip and Adam expressions are the parity
// contract pg_update_common.h states, with the pieces this unit shares with pg_update.hip and pg_update_gridworld.hip.
//
// One network = two hidden layers of H ReLU units on I inputs and one linear output, all float32, FLAT in the order of
// the module's parameters: W0 [H][I], b0 [H], W1 [H][H], b1 [H], Wo [H], bo [1] (ddpg_net_floats(H, I) floats).  The actor
// has I = O (the observation), output mean = fmaf(action_scale, tanhf(z), action_bias); the critic has I = O + 1 (the
// observation, then the action).  The buffers of the launches hold the actor, then the critic: PA + PC floats.
//
// Forward arithmetic is csrc/kernels/classic_control.hip::cc_actor_mean's.  In stage 2 no H-wide array is live in registers
// across an accumulation: the deltas the next layer needs are read back from the lane's own staged column.
//
// Restated in float64 in tests/ddpg_update_cases.py.
#include "pg_update_common.h"

#define DDPG_TILE 128                 // rows per tile = threads per block of HipDdpgGradients
#define DDPG_LD (DDPG_TILE + 4)       // staged arrays are [unit][DDPG_LD]

constexpr int ddpg_net_floats(int H, int I) { return H * I + H + H * H + H + H + 1; }

template <int H, int I>
struct DdpgNet {
  static_assert(H % 4 == 0, "the rows of W1 and Wo are read as float4");
  static constexpr int W0 = 0, B0 = H * I, W1 = B0 + H, B1 = W1 + H * H, WO = B1 + H, BO = WO + H, N = BO + 1;
};

__device__ __forceinline__ void ddpg_copy_to_lds(float *dst, const float *__restrict__ src, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

// h1 = relu(W0 x + b0)
template <int H, int I>
__device__ __forceinline__ void ddpg_layer0(const float *w, const float (&x)[I], float (&h1)[H]) {
  using L = DdpgNet<H, I>;
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = w[L::B0 + i];
#pragma unroll
    for (int k = 0; k < I; ++k) acc = fmaf(w[L::W0 + i * I + k], x[k], acc);
    h1[i] = fmaxf(acc, 0.0f);
  }
}

// h2 = relu(W1 h1 + b1)
template <int H, int I>
__device__ __forceinline__ void ddpg_layer1(const float *w, const float (&h1)[H], float (&h2)[H]) {
  using L = DdpgNet<H, I>;
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
}

// Wo h2 + bo
template <int H, int I>
__device__ __forceinline__ float ddpg_head(const float *w, const float (&h2)[H]) {
  using L = DdpgNet<H, I>;
  float z = w[L::BO];
#pragma unroll
  for (int j = 0; j < H; j += 4) {
    const float4 wr = *(const float4 *)(w + L::WO + j);
    z = fmaf(wr.x, h2[j], z); z = fmaf(wr.y, h2[j + 1], z);
    z = fmaf(wr.z, h2[j + 2], z); z = fmaf(wr.w, h2[j + 3], z);
  }
  return z;
}

// d1[j] = relu'(h1[j]) * sum_i W1[i][j] d2[i], i ascending from +0.  (Not the header's: d2 is an array in registers here.)
template <int H, int I>
__device__ __forceinline__ void ddpg_layer1_backward(const float *w, const float (&d2)[H], uint64_t mask1, float (&d1)[H]) {
  using L = DdpgNet<H, I>;
#pragma unroll
  for (int j = 0; j < H; ++j) d1[j] = 0.0f;
#pragma unroll
  for (int i = 0; i < H; ++i) {
#pragma unroll
    for (int j = 0; j < H; j += 4) {
      const float4 wr = *(const float4 *)(w + L::W1 + i * H + j);
      d1[j] = fmaf(wr.x, d2[i], d1[j]); d1[j + 1] = fmaf(wr.y, d2[i], d1[j + 1]);
      d1[j + 2] = fmaf(wr.z, d2[i], d1[j + 2]); d1[j + 3] = fmaf(wr.w, d2[i], d1[j + 3]);
    }
  }
#pragma unroll
  for (int j = 0; j < H; ++j) d1[j] = ((mask1 >> j) & 1ull) ? d1[j] : 0.0f;
}

// ------------------------------------------------------------------------------------------------- 1. next values
// obs [T, E, O]; next_values [T - 1, E]; `target` = the two target networks, actor then critic.  Dynamic LDS:
// (pad4(PA) + pad4(PC)) floats.
template <int H, int O>
__device__ __forceinline__ void ddpg_targets_impl(const float *__restrict__ obs, const float *__restrict__ target, int T, int E,
                                                  float action_scale, float action_bias, float *__restrict__ next_values) {
  constexpr int I = O + 1, PA = ddpg_net_floats(H, O), PC = ddpg_net_floats(H, I);
  extern __shared__ __attribute__((aligned(16))) float ddpg_lds[];
  float *wa = ddpg_lds, *wc = ddpg_lds + upd_pad4(PA);
  ddpg_copy_to_lds(wa, target, PA);
  ddpg_copy_to_lds(wc, target + PA, PC);
  __syncthreads();
  const long rows = (long)(T - 1) * E;
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < rows; g += (long)gridDim.x * blockDim.x) {
    // (the weights are the same for every trip: without this the compiler hoists their LDS reads out of the loop and
    // spills a few thousand of them)
    asm volatile("" ::: "memory");
    float x[I];
#pragma unroll
    for (int k = 0; k < O; ++k) x[k] = obs[(g + E) * O + k];
    float h1[H], h2[H];
    {
      float xa[O];
#pragma unroll
      for (int k = 0; k < O; ++k) xa[k] = x[k];
      ddpg_layer0<H, O>(wa, xa, h1);
    }
    ddpg_layer1<H, O>(wa, h1, h2);
    x[O] = fmaf(action_scale, tanhf(ddpg_head<H, O>(wa, h2)), action_bias);
    ddpg_layer0<H, I>(wc, x, h1);
    ddpg_layer1<H, I>(wc, h1, h2);
    next_values[g] = ddpg_head<H, I>(wc, h2);
  }
}

// ---------------------------------------------------------------------------------------------------- 2. gradients
// What a thread owns of one network's gradient for the whole launch (128 threads): UpdOwn's share of dW0, db0, dW1, db1, and
//   dWo: unit i = tid (tid < H);  dbo and the loss sum: thread 0
template <int H>
using DdpgOwn = UpdOwn<H, DDPG_TILE>;

// (not UpdAcc: one head unit per thread and no sum)
template <int H, int I>
struct DdpgAcc {
  static constexpr int JB = DdpgOwn<H>::JB, KB = (I + DdpgOwn<H>::KG - 1) / DdpgOwn<H>::KG;
  float w1[4][JB], w0[KB], b0, b1, wo, bo;
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < JB; ++b) w1[a][b] = 0.0f;
#pragma unroll
    for (int c = 0; c < KB; ++c) w0[c] = 0.0f;
    b0 = b1 = wo = bo = 0.0f;
  }
};

// dWo[i] += sum_r s[r] * h2[i][r]; dbo += sum_r s[r]; loss += sum_r l[r]   (rows ascending)
template <int H, int I>
__device__ __forceinline__ void ddpg_acc_head(DdpgAcc<H, I> &g, float &loss, const float *S1, const float *s, const float *l) {
  const int tid = threadIdx.x;
  if (tid < H) {
    for (int r = 0; r < DDPG_TILE; r += 4) {
      const float4 h = *(const float4 *)(S1 + tid * DDPG_LD + r), sv = *(const float4 *)(s + r);
      g.wo = fmaf(sv.x, h.x, g.wo); g.wo = fmaf(sv.y, h.y, g.wo); g.wo = fmaf(sv.z, h.z, g.wo); g.wo = fmaf(sv.w, h.w, g.wo);
    }
  }
  if (tid == 0) {
    for (int r = 0; r < DDPG_TILE; ++r) { g.bo += s[r]; loss += l[r]; }
  }
}

template <int H, int I>
__device__ __forceinline__ void ddpg_write_partial(const DdpgAcc<H, I> &g, float *out) {
  using L = DdpgNet<H, I>;
  using W = DdpgOwn<H>;
  constexpr int JB = W::JB, KB = DdpgAcc<H, I>::KB;
  const int tid = threadIdx.x, ib = tid % W::NIB, jb = tid / W::NIB;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < JB; ++b) out[L::W1 + (ib + W::NIB * a) * H + jb + W::NJB * b] = g.w1[a][b];
  const int i = tid % H, k0 = KB * (tid / H);
#pragma unroll
  for (int c = 0; c < KB; ++c)
    if (k0 + c < I) out[L::W0 + i * I + k0 + c] = g.w0[c];
  if (tid < H) {
    out[L::B0 + tid] = g.b0;
    out[L::B1 + tid] = g.b1;
    out[L::WO + tid] = g.wo;
  }
  if (tid == 0) out[L::BO] = g.bo;
}

// obs [T, E, O], actions / rewards / next_values as [T (- 1), E] floats, done [T, E] int32; theta = actor, then critic;
// returns_out [V, E]; partials [gridDim.x][PA + PC + 2]: the block's gradient of the actor, of the critic, then its sums of
// (returns - Q)^2 and of Q(obs, mu(obs)).  Dynamic LDS: ddpg_gradients_lds_floats(H, O) floats.  blockDim.x = DDPG_TILE.
constexpr int ddpg_gradients_lds_floats(int H, int O) {
  return upd_pad4(ddpg_net_floats(H, O)) + upd_pad4(ddpg_net_floats(H, O + 1)) + 2 * H * DDPG_LD + 4 * DDPG_LD + 2 * DDPG_TILE;
}

template <int H, int O>
__device__ __forceinline__ void ddpg_gradients_impl(const float *__restrict__ obs, const float *__restrict__ actions,
                                                    const float *__restrict__ rewards, const int *__restrict__ done,
                                                    const float *__restrict__ next_values, const float *__restrict__ theta,
                                                    int T, int E, int n_step, float gamma, float action_scale,
                                                    float action_bias, float *__restrict__ returns_out,
                                                    float *__restrict__ partials) {
  constexpr int I = O + 1, PA = ddpg_net_floats(H, O), PC = ddpg_net_floats(H, I);
  using LA = DdpgNet<H, O>;
  using LC = DdpgNet<H, I>;
  extern __shared__ __attribute__((aligned(16))) float ddpg_lds[];
  float *wa = ddpg_lds, *wc = wa + upd_pad4(PA), *S0 = wc + upd_pad4(PC), *S1 = S0 + H * DDPG_LD, *S2 = S1 + H * DDPG_LD;
  float *S3 = S2 + 4 * DDPG_LD, *S4 = S3 + DDPG_TILE;
  ddpg_copy_to_lds(wa, theta, PA);
  ddpg_copy_to_lds(wc, theta + PA, PC);
  const int tid = threadIdx.x;
  const int V = T - n_step + 1;
  const long rows = (long)V * E;
  const long tiles = (rows + DDPG_TILE - 1) / DDPG_TILE;
  const float inv_rows = 1.0f / (float)rows;
  DdpgAcc<H, O> ga;
  DdpgAcc<H, I> gc;
  ga.clear();
  gc.clear();
  float sum_sq = 0.0f, sum_j = 0.0f;
  __syncthreads();
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long g = tile * DDPG_TILE + tid;
    const bool live = g < rows;
    float x[I];
#pragma unroll
    for (int k = 0; k < I; ++k) x[k] = 0.0f;
    float ret = 0.0f;
    if (live) {
#pragma unroll
      for (int k = 0; k < O; ++k) x[k] = obs[g * O + k];
      x[O] = actions[g];
      // the n-step return: losses.DDPG.n_step_returns, operation for operation (two roundings per product-sum)
      const long e = g % E, t = g / E;
      long at = (t + n_step - 1) * E + e;
      const float dl = done[at] > 0 ? 1.0f : 0.0f;
      if (t + n_step - 1 < T - 1) {
        ret = rewards[at] + ((1.0f - dl) * gamma) * next_values[at];
      } else {
        ret = dl * rewards[at] + (1.0f - dl) * next_values[(long)(T - 2) * E + e];
      }
      for (int j = 1; j < n_step; ++j) {
        at -= E;
        const float dj = done[at] > 0 ? 1.0f : 0.0f;
        ret = rewards[at] + ((1.0f - dj) * gamma) * ret;
      }
      returns_out[g] = ret;
    }

    // ======================================================================= critic loss: mse(returns, Q(obs, action))
    uint64_t m1, m2;
    float dq;
    {
      float c1[H], c2[H];
      ddpg_layer0<H, I>(wc, x, c1);
      ddpg_layer1<H, I>(wc, c1, c2);
      const float q = ddpg_head<H, I>(wc, c2);
      m1 = upd_positive_mask<H>(c1);
      m2 = upd_positive_mask<H>(c2);
      const float diff = live ? q - ret : 0.0f;
      dq = (2.0f * diff) * inv_rows;
      upd_stage<H, DDPG_LD>(S0, tid, c1);
      upd_stage<H, DDPG_LD>(S1, tid, c2);
      S3[tid] = dq;
      S4[tid] = diff * diff;
    }
    __syncthreads();
    ddpg_acc_head<H, I>(gc, sum_sq, S1, S3, S4);
    __syncthreads();
    {
      float d2[H];
#pragma unroll
      for (int i = 0; i < H; ++i) d2[i] = ((m2 >> i) & 1ull) ? dq * wc[LC::WO + i] : 0.0f;
      upd_stage<H, DDPG_LD>(S1, tid, d2);
    }
    __syncthreads();
    upd_acc_w1<H, DDPG_TILE, DDPG_LD>(gc, S0, S1);
    {
      float d2[H], d1[H];
#pragma unroll
      for (int i = 0; i < H; ++i) d2[i] = S1[i * DDPG_LD + tid];
      ddpg_layer1_backward<H, I>(wc, d2, m1, d1);
      __syncthreads();
      upd_stage<H, DDPG_LD>(S1, tid, d1);
#pragma unroll
      for (int k = 0; k < I; ++k) S2[k * DDPG_LD + tid] = x[k];
    }
    __syncthreads();
    upd_acc_w0<H, DDPG_TILE, DDPG_LD, I>(gc, S1, S2);
    __syncthreads();

    // ========================================= actor loss: -mean(Q(obs, mu(obs))), differentiated through the action only
    float dz;
    {
      float th;
      {
        float xa[O], a1[H], a2[H];
#pragma unroll
        for (int k = 0; k < O; ++k) xa[k] = x[k];
        ddpg_layer0<H, O>(wa, xa, a1);
        ddpg_layer1<H, O>(wa, a1, a2);
        th = tanhf(ddpg_head<H, O>(wa, a2));
        m1 = upd_positive_mask<H>(a1);
        m2 = upd_positive_mask<H>(a2);
        upd_stage<H, DDPG_LD>(S0, tid, a1);
        upd_stage<H, DDPG_LD>(S1, tid, a2);
      }
      x[O] = fmaf(action_scale, th, action_bias);
      float dmu = 0.0f;
      {
        float j1[H], j2[H];
        ddpg_layer0<H, I>(wc, x, j1);
        ddpg_layer1<H, I>(wc, j1, j2);
        S4[tid] = live ? ddpg_head<H, I>(wc, j2) : 0.0f;
        const uint64_t mj1 = upd_positive_mask<H>(j1), mj2 = upd_positive_mask<H>(j2);
        const float dj = live ? -inv_rows : 0.0f;
#pragma unroll
        for (int i = 0; i < H; ++i) j2[i] = ((mj2 >> i) & 1ull) ? dj * wc[LC::WO + i] : 0.0f;
        ddpg_layer1_backward<H, I>(wc, j2, mj1, j1);
#pragma unroll
        for (int j = 0; j < H; ++j) dmu = fmaf(j1[j], wc[LC::W0 + j * I + O], dmu);
      }
      dz = (dmu * action_scale) * (1.0f - th * th);
      S3[tid] = dz;
    }
    __syncthreads();
    ddpg_acc_head<H, O>(ga, sum_j, S1, S3, S4);
    __syncthreads();
    {
      float f2[H];
#pragma unroll
      for (int i = 0; i < H; ++i) f2[i] = ((m2 >> i) & 1ull) ? dz * wa[LA::WO + i] : 0.0f;
      upd_stage<H, DDPG_LD>(S1, tid, f2);
    }
    __syncthreads();
    upd_acc_w1<H, DDPG_TILE, DDPG_LD>(ga, S0, S1);
    {
      float f2[H], f1[H];
#pragma unroll
      for (int i = 0; i < H; ++i) f2[i] = S1[i * DDPG_LD + tid];
      ddpg_layer1_backward<H, O>(wa, f2, m1, f1);
      __syncthreads();
      upd_stage<H, DDPG_LD>(S1, tid, f1);
    }
    __syncthreads();
    upd_acc_w0<H, DDPG_TILE, DDPG_LD, O>(ga, S1, S2);   // (S2 still holds the tile's observations)
    __syncthreads();
  }
  float *out = partials + (long)blockIdx.x * (PA + PC + 2);
  ddpg_write_partial<H, O>(ga, out);
  ddpg_write_partial<H, I>(gc, out + PA);
  if (tid == 0) {
    out[PA + PC] = sum_sq;
    out[PA + PC + 1] = sum_j;
  }
}

// -------------------------------------------------------------------------------------------------- 3 and 4: layout
// the twelve parameter tensors of (actor, critic) inside the flat PA + PC floats
__device__ __forceinline__ UpdTensor ddpg_tensor(int k, int H, int O) {
  const int PA = ddpg_net_floats(H, O);
  const int I = k < 6 ? O : O + 1, base = k < 6 ? 0 : PA, j = k < 6 ? k : k - 6;
  const int o1 = H * I, o2 = o1 + H, o3 = o2 + H * H, o4 = o3 + H, o5 = o4 + H, o6 = o5 + 1;
  const int lo = j == 0 ? 0 : j == 1 ? o1 : j == 2 ? o2 : j == 3 ? o3 : j == 4 ? o4 : o5;
  const int hi = j == 0 ? o1 : j == 1 ? o2 : j == 2 ? o3 : j == 3 ? o4 : j == 4 ? o5 : o6;
  return {base + lo, hi - lo};
}

#define DDPG_REDUCE_THREADS 1024

extern "C" {

#define DDPG_ENTRIES(HH, OO)                                                                                           \
  __global__ void __launch_bounds__(256) HipDdpgTargets_H##HH##_O##OO(                                                 \
      const float *__restrict__ obs, const float *__restrict__ target, int T, int E, float action_scale,               \
      float action_bias, float *__restrict__ next_values) {                                                            \
    ddpg_targets_impl<HH, OO>(obs, target, T, E, action_scale, action_bias, next_values);                              \
  }                                                                                                                    \
  __global__ void __launch_bounds__(DDPG_TILE) HipDdpgGradients_H##HH##_O##OO(                                         \
      const float *__restrict__ obs, const float *__restrict__ actions, const float *__restrict__ rewards,             \
      const int *__restrict__ done, const float *__restrict__ next_values, const float *__restrict__ theta, int T,     \
      int E, int n_step, float gamma, float action_scale, float action_bias, float *__restrict__ returns_out,          \
      float *__restrict__ partials) {                                                                                  \
    ddpg_gradients_impl<HH, OO>(obs, actions, rewards, done, next_values, theta, T, E, n_step, gamma, action_scale,    \
                                action_bias, returns_out, partials);                                                   \
  }
DDPG_ENTRIES(32, 2)
DDPG_ENTRIES(32, 3)
DDPG_ENTRIES(64, 2)
DDPG_ENTRIES(64, 3)

// grid = 13 blocks of DDPG_REDUCE_THREADS: block k < 12 is upd_reduce_tensor on tensor k of the n_blocks partials (rows of
// `stride` floats) into grads [PA + PC]; block 12 writes losses = {sum of squared errors / rows, -(sum of Q) / rows}.
// (Twelve tensors of two networks and two losses divided by the rows: not the policies' reduce body.)
__global__ void __launch_bounds__(DDPG_REDUCE_THREADS) HipDdpgReduce(const float *__restrict__ partials, int n_blocks,
                                                                     int H, int O, long rows, float *__restrict__ grads,
                                                                     float *__restrict__ sumsq, float *__restrict__ losses) {
  __shared__ float tree[DDPG_REDUCE_THREADS];
  const int PT = ddpg_net_floats(H, O) + ddpg_net_floats(H, O + 1);
  const long stride = PT + 2;
  const int tid = threadIdx.x;
  if (blockIdx.x >= 12) {
    if (blockIdx.x == 12 && tid < 2) {
      float s = 0.0f;
      for (int b = 0; b < n_blocks; ++b) s += partials[b * stride + PT + tid];
      losses[tid] = tid == 0 ? s / (float)rows : -(s / (float)rows);
    }
    return;
  }
  upd_reduce_tensor<DDPG_REDUCE_THREADS>(tree, partials, n_blocks, stride, ddpg_tensor(blockIdx.x, H, O), grads, sumsq);
}

// One thread per parameter of (actor, critic).  theta / target / exp_avg / exp_avg_sq / grads: PA + PC floats.
//   clip over the network's six tensor norms and Adam: upd_clip_adam's statements with the network's step size (written
//          out here, where the soft update follows them: as a call they compile to another schedule)
//   target t = t (1 - tau) + p tau: two products, one sum
//   packed the rollout's copy of the actor (pack_rollout_actor: W0 rows padded to an even length) or null
__global__ void __launch_bounds__(256) HipDdpgApply(float *__restrict__ theta, float *__restrict__ target,
                                                    float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq,
                                                    const float *__restrict__ grads, const float *__restrict__ sumsq,
                                                    float *__restrict__ packed, int H, int O, float max_norm,
                                                    float step_size_actor, float step_size_critic, float bc2_sqrt,
                                                    float one_minus_beta1, float beta2, float one_minus_beta2, float eps,
                                                    float tau, float one_minus_tau) {
  const int PA = ddpg_net_floats(H, O), PT = PA + ddpg_net_floats(H, O + 1);
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= PT) return;
  const bool is_actor = idx < PA;
  float g = grads[idx];
  if (max_norm > 0.0f) {
    float total = 0.0f;
    for (int k = 0; k < 6; ++k) {
      const float norm = sqrtf(sumsq[(is_actor ? 0 : 6) + k]);
      total += norm * norm;
    }
    const float coef = fminf(max_norm / (sqrtf(total) + 1e-6f), 1.0f);
    g *= coef;
  }
  const float m0 = exp_avg[idx];
  const float m = fmaf(one_minus_beta1, g - m0, m0);
  const float v = fmaf(one_minus_beta2, g * g, exp_avg_sq[idx] * beta2);
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  const float p = fmaf(-(is_actor ? step_size_actor : step_size_critic), m / denom, theta[idx]);
  exp_avg[idx] = m;
  exp_avg_sq[idx] = v;
  theta[idx] = p;
  target[idx] = target[idx] * one_minus_tau + p * tau;
  if (packed != nullptr && is_actor) {
    const int OP = (O + 1) & ~1;
    const int at = idx < H * O ? (idx / O) * OP + idx % O : idx + H * (OP - O);
    packed[at] = p;
  }
}

}  // extern "C"
