// pg_update.hip -- the A2C / PPO update of Trainer (training/trainer.py, `trainer.fused_update: "all"`) for the small
// discrete policies the rollout kernels evaluate themselves (Cartpole, Acrobot, MountainCar), as FIVE launches:
//
//   1. HipPgValues_H<H>_O<O>     values[t, e] = v(obs[t, e]) of all T * E recorded rows; one thread per row, grid-stride.
//   2. HipDiscountedReturns      the existing entry of wd_kernels_update.hsaco (policy_mlp.hip), launched on `values`
//                                with w = 1, v_col = 0: returns and advantages [T, E].
//   3. HipPgGradients_H<H>_O<O>  per row the forward pass (the same function as launch 1: the same bits for v), the
//                                statements of policy_mlp.hip::HipPolicyGradientHead for log-softmax, entropy, d loss / d
//                                logits and d loss / d v, and the backward pass through the heads and the two hidden layers;
//                                one partial of the eight gradient tensors and of four sums per block.
//   4. HipPgReduce               the blocks' partials summed in block order into the flat gradient, the sum of squares of
//                                every parameter tensor, and the four sums.
//   5. HipPgApply                clip_grad_norm_ over the eight tensors, torch.optim.Adam's default expression, and the
//                                refill of the packed policy the rollout kernels read.
//
// The summation order, relu'(0) = 0, "no float atomics, nothing read back" and the clip and Adam expressions are the parity
// contract pg_update_common.h states, with the pieces this unit shares with pg_update_gridworld.hip and ddpg_update.hip.
//
// One network = two hidden layers of H ReLU units on O inputs, one head of A logits (1 <= A <= 8, a launch argument) and
// the value head, all float32, FLAT in the order of the module's parameters (training/models.py::FullyConnected):
// W0 [H][O], b0 [H], W1 [H][H], b1 [H], Wp [A][H], bp [A], Wv [H], bv [1] (upd_pg_net_floats(H, O, A) floats).  The first
// six are pack_rollout_policy's layout: the packed policy is a prefix of the flat buffer.  In LDS the value head starts
// at a fixed 16-byte aligned offset behind EIGHT bias slots (PgNet), whatever A is.
//
// Forward arithmetic is cartpole.hip::cp_policy_cum's / classic_control.hip::cc_policy_cum's.
//
// Restated in float64 in tests/pg_update_cases.py.
#include "pg_update_common.h"

#define PG_TILE 128                 // rows per tile = threads per block of HipPgGradients
#define PG_LD (PG_TILE + 4)         // staged arrays are [unit][PG_LD]
#define PG_MAX_ACTIONS 8
#define PG_OUTPUTS (PG_MAX_ACTIONS + 1)   // staged output deltas: the logits' (those below A are real), then the value's

// offsets inside the LDS copy (W0 .. bp as in the flat buffer; the value head behind eight bias slots)
template <int H, int O>
struct PgNet {
  static_assert(H % 4 == 0 && O % 2 == 0, "the rows of W1 / Wp / Wv are read as float4, those of W0 as float2");
  static constexpr int W0 = 0, B0 = H * O, W1 = B0 + H, B1 = W1 + H * H, WP = B1 + H;
  static constexpr int bp(int A) { return WP + A * H; }
  static constexpr int wv(int A) { return WP + A * H + PG_MAX_ACTIONS; }
  static constexpr int bv(int A) { return WP + A * H + PG_MAX_ACTIONS + H; }
  static constexpr int LDS = upd_pad4(WP + PG_MAX_ACTIONS * H + PG_MAX_ACTIONS + H + 1);
};

template <int H, int O>
__device__ __forceinline__ void pg_copy_net_to_lds(float *dst, const float *__restrict__ theta, int A) {
  using L = PgNet<H, O>;
  const int head = L::bp(A) + A;   // W0 .. bp: the same offsets in both
  for (int i = threadIdx.x; i < head; i += blockDim.x) dst[i] = theta[i];
  for (int i = threadIdx.x; i < H + 1; i += blockDim.x) dst[L::wv(A) + i] = theta[head + i];
}

// the forward: h1 = relu(W0 x + b0), then the header's second layer and value head.  (The first layer stays here: it reads
// float2 rows of O floats, the gridworld unit's float4 rows at stride 24 plus a tail.)
template <int H, int O>
__device__ __forceinline__ float pg_forward(const float *w, int A, const float (&x)[O], float (&h1)[H], float (&h2)[H]) {
  using L = PgNet<H, O>;
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = w[L::B0 + i];
#pragma unroll
    for (int k = 0; k < O; k += 2) {
      const float2 wr = *(const float2 *)(w + L::W0 + i * O + k);
      acc = fmaf(wr.x, x[k], acc); acc = fmaf(wr.y, x[k + 1], acc);
    }
    h1[i] = fmaxf(acc, 0.0f);
  }
  return upd_layer1_and_value<H>(w + L::W1, w + L::B1, w + L::wv(A), h1, h2);
}

// ------------------------------------------------------------------------------------------------------ 1. values
// obs [T * E][O]; values [T * E].  Dynamic LDS: PgNet<H, O>::LDS floats.
template <int H, int O>
__device__ __forceinline__ void pg_values_impl(const float *__restrict__ obs, const float *__restrict__ theta, long rows,
                                               int A, float *__restrict__ values) {
  extern __shared__ __attribute__((aligned(16))) float pg_lds[];
  pg_copy_net_to_lds<H, O>(pg_lds, theta, A);
  __syncthreads();
  for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < rows; g += (long)gridDim.x * blockDim.x) {
    // (the weights are the same for every trip: without this the compiler hoists their LDS reads out of the loop and
    // spills them)
    asm volatile("" ::: "memory");
    float x[O], h1[H], h2[H];
#pragma unroll
    for (int k = 0; k < O; ++k) x[k] = obs[g * O + k];
    values[g] = pg_forward<H, O>(pg_lds, A, x, h1, h2);
  }
}

// --------------------------------------------------------------------------------------------------- 3. gradients
// What a thread owns of the gradient for the whole launch (128 threads): UpdOwn's share of dW0, db0, dW1, db1, and
//   dWp [A][H], dWv [H]: unit i = tid % H, outputs o = tid / H + KG c (c < OB; o < A: a logit, o = 8: the value)
//   dbp, dbv: output o = tid (tid < 9);  the four sums: threads 16 .. 19
template <int H>
struct PgOwn : UpdOwn<H, PG_TILE> {
  static constexpr int OB = (PG_OUTPUTS + PgOwn::KG - 1) / PgOwn::KG;
};

template <int H, int O>
using PgAcc = UpdAcc<PgOwn<H>::JB, (O + PgOwn<H>::KG - 1) / PgOwn<H>::KG, PgOwn<H>::OB>;

// dWp[o][i] += sum_r dz[o][r] * h2[i][r]; dWv[i] += sum_r dv[r] * h2[i][r]; dbp[o] += sum_r dz[o][r]; dbv += sum_r dv[r];
// the four sums += their staged per-row terms   (rows ascending; SD = [PG_OUTPUTS][PG_LD], SS = [4][PG_LD]).  (Stays here:
// the output rows are eight logit slots of which A are real, then the value's; the gridworld unit's are all real.)
template <int H, int O>
__device__ __forceinline__ void pg_acc_heads(PgAcc<H, O> &g, const float *S1, const float *SD, const float *SS, int A) {
  using W = PgOwn<H>;
  const int tid = threadIdx.x, i = tid % H, o0 = tid / H;
#pragma unroll
  for (int c = 0; c < W::OB; ++c) {
    const int o = o0 + W::KG * c;
    if (o < A || o == PG_MAX_ACTIONS) {
      float acc = g.wo[c];
      for (int r = 0; r < PG_TILE; r += 4) {
        const float4 h = *(const float4 *)(S1 + i * PG_LD + r), d = *(const float4 *)(SD + o * PG_LD + r);
        acc = fmaf(d.x, h.x, acc); acc = fmaf(d.y, h.y, acc); acc = fmaf(d.z, h.z, acc); acc = fmaf(d.w, h.w, acc);
      }
      g.wo[c] = acc;
    }
  }
  if (tid < A || tid == PG_MAX_ACTIONS) {
    for (int r = 0; r < PG_TILE; ++r) g.bo += SD[tid * PG_LD + r];
  }
  if (tid >= 16 && tid < 20) {
    for (int r = 0; r < PG_TILE; ++r) g.sum += SS[(tid - 16) * PG_LD + r];
  }
}

// the block's partial, in the FLAT layout (A logits): P floats, then the four sums.  (Stays here for its head part.)
template <int H, int O>
__device__ __forceinline__ void pg_write_partial(const PgAcc<H, O> &g, float *out, int A) {
  using L = PgNet<H, O>;
  using W = PgOwn<H>;
  constexpr int JB = W::JB, KB = PgAcc<H, O>::KB;
  const int tid = threadIdx.x, ib = tid % W::NIB, jb = tid / W::NIB;
  const int BP = L::WP + A * H, WV = BP + A, BV = WV + H;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < JB; ++b) out[L::W1 + (ib + W::NIB * a) * H + jb + W::NJB * b] = g.w1[a][b];
  const int i = tid % H, k0 = KB * (tid / H), o0 = tid / H;
#pragma unroll
  for (int c = 0; c < KB; ++c)
    if (k0 + c < O) out[L::W0 + i * O + k0 + c] = g.w0[c];
#pragma unroll
  for (int c = 0; c < W::OB; ++c) {
    const int o = o0 + W::KG * c;
    if (o < A) out[L::WP + o * H + i] = g.wo[c];
    else if (o == PG_MAX_ACTIONS) out[WV + i] = g.wo[c];
  }
  if (tid < H) {
    out[L::B0 + tid] = g.b0;
    out[L::B1 + tid] = g.b1;
  }
  if (tid < A) out[BP + tid] = g.bo;
  else if (tid == PG_MAX_ACTIONS) out[BV] = g.bo;
  if (tid >= 16 && tid < 20) out[BV + 1 + tid - 16] = g.sum;
}

// obs [T * E][O], actions [T * E] int32, adv / ret [T * E]; theta flat; partials [gridDim.x][P + 4]: the block's gradient,
// then its sums of logp * adv, of the entropy, of (v - ret)^2 and of adv.  Dynamic LDS: pg_gradients_lds_floats(H, O)
// floats.  blockDim.x = PG_TILE.
constexpr int pg_gradients_lds_floats(int H, int O) {
  return upd_pad4(H * O + H + H * H + H + PG_MAX_ACTIONS * H + PG_MAX_ACTIONS + H + 1) + 2 * H * PG_LD + O * PG_LD +
         PG_OUTPUTS * PG_LD + 4 * PG_LD;
}

template <int H, int O>
__device__ __forceinline__ void pg_gradients_impl(const float *__restrict__ obs, const int *__restrict__ actions,
                                                  const float *__restrict__ adv, const float *__restrict__ ret,
                                                  const float *__restrict__ theta, long rows, int A, float inv_R,
                                                  float ent_coeff, float vf_coeff, float *__restrict__ partials) {
  using L = PgNet<H, O>;
  extern __shared__ __attribute__((aligned(16))) float pg_lds[];
  float *w = pg_lds, *S0 = w + L::LDS, *S1 = S0 + H * PG_LD, *S2 = S1 + H * PG_LD, *SD = S2 + O * PG_LD;
  float *SS = SD + PG_OUTPUTS * PG_LD;
  pg_copy_net_to_lds<H, O>(w, theta, A);
  const int tid = threadIdx.x;
  const long tiles = (rows + PG_TILE - 1) / PG_TILE;
  PgAcc<H, O> acc;
  acc.clear();
  __syncthreads();
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long g = tile * PG_TILE + tid;
    const bool live = g < rows;
    float x[O];
#pragma unroll
    for (int k = 0; k < O; ++k) x[k] = 0.0f;
    float a = 0.0f, rt = 0.0f;
    int taken = 0;
    if (live) {
#pragma unroll
      for (int k = 0; k < O; ++k) x[k] = obs[g * O + k];
      a = adv[g];
      rt = ret[g];
      taken = actions[g];
    }
    uint64_t m1, m2;
    {
      float dz[PG_MAX_ACTIONS], dv;
      float h1[H], h2[H];
      const float v = pg_forward<H, O>(w, A, x, h1, h2);
      m1 = upd_positive_mask<H>(h1);
      m2 = upd_positive_mask<H>(h2);
      // the logits: acc = bias, one fmaf per hidden unit in index order
      float z[PG_MAX_ACTIONS], m = -__builtin_inff();
#pragma unroll
      for (int j = 0; j < PG_MAX_ACTIONS; ++j) {
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
      // HipPolicyGradientHead's statements (policy_mlp.hip), one head: the shift by the maximum FIRST.  (Same statements,
      // same build flags -- no contraction -- but other logits and another schedule around them: the results agree with
      // that entry's under the tests' bound and are not claimed bit-identical to it.  They stay in each unit: as one
      // template over the action bound they compile to another schedule here.)
      float total = 0.0f;
#pragma unroll
      for (int j = 0; j < PG_MAX_ACTIONS; ++j)
        if (j < A) total += expf(z[j] - m);
      const float lse = logf(total);
      float Hent = 0.0f;
#pragma unroll
      for (int j = 0; j < PG_MAX_ACTIONS; ++j)
        if (j < A) {
          const float lp = (z[j] - m) - lse;
          Hent -= expf(lp) * lp;
        }
      const int clamped = min(max(taken, 0), A - 1);
      float logp_taken = 0.0f;
#pragma unroll
      for (int j = 0; j < PG_MAX_ACTIONS; ++j)
        if (j == clamped) logp_taken = (z[j] - m) - lse;
#pragma unroll
      for (int j = 0; j < PG_MAX_ACTIONS; ++j) {
        dz[j] = 0.0f;
        if (j < A && live) {
          const float lp = (z[j] - m) - lse, pj = expf(lp);
          dz[j] = (a * (pj - (j == taken ? 1.0f : 0.0f)) + ent_coeff * pj * (lp + Hent)) * inv_R;
        }
      }
      const float d = v - rt;
      dv = live ? 2.0f * vf_coeff * d * inv_R : 0.0f;
      upd_stage<H, PG_LD>(S0, tid, h1);
      upd_stage<H, PG_LD>(S1, tid, h2);
#pragma unroll
      for (int j = 0; j < PG_MAX_ACTIONS; ++j) SD[j * PG_LD + tid] = dz[j];
      SD[PG_MAX_ACTIONS * PG_LD + tid] = dv;
      SS[0 * PG_LD + tid] = live ? logp_taken * a : 0.0f;
      SS[1 * PG_LD + tid] = live ? Hent : 0.0f;
      SS[2 * PG_LD + tid] = live ? d * d : 0.0f;
      SS[3 * PG_LD + tid] = live ? a : 0.0f;
#pragma unroll
      for (int k = 0; k < O; ++k) S2[k * PG_LD + tid] = x[k];
    }
    __syncthreads();
    pg_acc_heads<H, O>(acc, S1, SD, SS, A);
    __syncthreads();
    {
      // d2[i] = relu'(h2[i]) * (sum_j dz[j] Wp[j][i] + dv Wv[i]), j ascending from +0, the value last (the deltas read
      // back from the lane's own staged column).  (Stays here: all H sums in flight; that form spills in the gridworld unit.)
      float d2[H], dz[PG_MAX_ACTIONS];
#pragma unroll
      for (int j = 0; j < PG_MAX_ACTIONS; ++j) dz[j] = SD[j * PG_LD + tid];
      const float dv = SD[PG_MAX_ACTIONS * PG_LD + tid];
#pragma unroll
      for (int i = 0; i < H; ++i) d2[i] = 0.0f;
#pragma unroll
      for (int j = 0; j < PG_MAX_ACTIONS; ++j) {
        if (j < A) {
#pragma unroll
          for (int i = 0; i < H; i += 4) {
            const float4 wr = *(const float4 *)(w + L::WP + j * H + i);
            d2[i] = fmaf(wr.x, dz[j], d2[i]); d2[i + 1] = fmaf(wr.y, dz[j], d2[i + 1]);
            d2[i + 2] = fmaf(wr.z, dz[j], d2[i + 2]); d2[i + 3] = fmaf(wr.w, dz[j], d2[i + 3]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < H; i += 4) {
        const float4 wr = *(const float4 *)(w + L::wv(A) + i);
        d2[i] = fmaf(wr.x, dv, d2[i]); d2[i + 1] = fmaf(wr.y, dv, d2[i + 1]);
        d2[i + 2] = fmaf(wr.z, dv, d2[i + 2]); d2[i + 3] = fmaf(wr.w, dv, d2[i + 3]);
      }
#pragma unroll
      for (int i = 0; i < H; ++i) d2[i] = ((m2 >> i) & 1ull) ? d2[i] : 0.0f;
      upd_stage<H, PG_LD>(S1, tid, d2);
    }
    __syncthreads();
    upd_acc_w1<H, PG_TILE, PG_LD>(acc, S0, S1);
    {
      float d1[H];
      upd_layer1_backward<H, PG_LD>(w + L::W1, S1 + tid, m1, d1);
      __syncthreads();
      upd_stage<H, PG_LD>(S1, tid, d1);
    }
    __syncthreads();
    upd_acc_w0<H, PG_TILE, PG_LD, O>(acc, S1, S2);
    __syncthreads();
  }
  pg_write_partial<H, O>(acc, partials + (long)blockIdx.x * (upd_pg_net_floats(H, O, A) + 4), A);
}

// ------------------------------------------------------------------------------------------- 4 and 5: reduce, apply
__device__ __forceinline__ bool pg_shape_ok(int H, int O, int A) {
  return (H == 32 || H == 64) && (O == 2 || O == 4 || O == 6) && A >= 1 && A <= PG_MAX_ACTIONS;
}

#define PG_REDUCE_THREADS 1024

extern "C" {

// (an entry launched with another width or observation size than its own, or with A outside 1 .. 8, touches nothing)
#define PG_ENTRIES(HH, OO)                                                                                             \
  __global__ void __launch_bounds__(256) HipPgValues_H##HH##_O##OO(                                                    \
      const float *__restrict__ obs, const float *__restrict__ theta, long rows, int H, int O, int A,                  \
      float *__restrict__ values) {                                                                                    \
    if (H != HH || O != OO || A < 1 || A > PG_MAX_ACTIONS) return;                                                     \
    pg_values_impl<HH, OO>(obs, theta, rows, A, values);                                                               \
  }                                                                                                                    \
  __global__ void __launch_bounds__(PG_TILE) HipPgGradients_H##HH##_O##OO(                                             \
      const float *__restrict__ obs, const int *__restrict__ actions, const float *__restrict__ adv,                   \
      const float *__restrict__ ret, const float *__restrict__ theta, long rows, int H, int O, int A, float inv_R,     \
      float ent_coeff, float vf_coeff, float *__restrict__ partials) {                                                 \
    if (H != HH || O != OO || A < 1 || A > PG_MAX_ACTIONS) return;                                                     \
    pg_gradients_impl<HH, OO>(obs, actions, adv, ret, theta, rows, A, inv_R, ent_coeff, vf_coeff, partials);           \
  }
PG_ENTRIES(32, 2)
PG_ENTRIES(32, 4)
PG_ENTRIES(32, 6)
PG_ENTRIES(64, 2)
PG_ENTRIES(64, 4)
PG_ENTRIES(64, 6)

// upd_pg_reduce on grid = 9 blocks of PG_REDUCE_THREADS
__global__ void __launch_bounds__(PG_REDUCE_THREADS) HipPgReduce(const float *__restrict__ partials, int n_blocks, int H,
                                                                 int O, int A, float *__restrict__ grads,
                                                                 float *__restrict__ sumsq, float *__restrict__ sums) {
  __shared__ float tree[PG_REDUCE_THREADS];
  if (!pg_shape_ok(H, O, A)) return;
  upd_pg_reduce<PG_REDUCE_THREADS>(tree, partials, n_blocks, upd_pg_net_floats(H, O, A), H, O, A, grads, sumsq, sums);
}

// One thread per parameter.  theta / exp_avg / exp_avg_sq / grads: P floats.
//   clip over the eight tensor norms and Adam: upd_clip_adam
//   packed the rollout's copy of the policy (pack_rollout_policy: W0 .. bp, the first P - H - 1 floats) or null
__global__ void __launch_bounds__(256) HipPgApply(float *__restrict__ theta, float *__restrict__ exp_avg,
                                                  float *__restrict__ exp_avg_sq, const float *__restrict__ grads,
                                                  const float *__restrict__ sumsq, float *__restrict__ packed, int H, int O,
                                                  int A, float max_norm, float step_size, float bc2_sqrt,
                                                  float one_minus_beta1, float beta2, float one_minus_beta2, float eps) {
  if (!pg_shape_ok(H, O, A)) return;
  const int P = upd_pg_net_floats(H, O, A);
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P) return;
  const float p = upd_clip_adam(idx, theta, exp_avg, exp_avg_sq, grads, sumsq, 8, max_norm, step_size, bc2_sqrt,
                                one_minus_beta1, beta2, one_minus_beta2, eps);
  if (packed != nullptr && idx < P - H - 1) packed[idx] = p;
}

}  // extern "C"
