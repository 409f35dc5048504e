// ddpg_update_matrix.hip -- launch 2 of TrainerDDPG's update (ddpg_update.hip: HipDdpgGradients_H<H>_O<O>) ON THE FLOAT32
// MATRIX CORES: HipDdpgGradientsMatrix_H<H>_O<O>, the same arguments, the same returns_out [V, E] and the same partials
// [gridDim.x][PA + PC + 2] in the flat layout (actor, critic, the block's sum of (Q - ret)^2, its sum of Q(obs, mu(obs))),
// consumed unchanged by HipDdpgReduce and HipDdpgApply.  Opt-in (`trainer.fused_update_gradients: "matrix"`,
// training/ddpg_update_kernels.py); a code object of its own.
//
// The lanes entry runs one row per lane: six dependent passes of H x H fmafs, 300 us whatever the batch.  Here a row's
// passes are split over two lanes and their H x H products go to v_mfma_f32_32x32x2_f32 (D[32][32] += A[32][2] B[2][32]; lane
// l supplies A[l % 32][l / 32] and B[l / 32][l % 32]).  pg_update_matrix.hip's split: a block is four wavefronts on a
// 128-row tile (blocks stride over the tiles), a wavefront owns 32 rows, lanes l and l + 32 share row r = l % 32, and lane
// half hf = l / 32 holds of every 32 hidden units the sixteen that its registers of a 32 x 32 accumulator hold
// (pg_update_matrix_common.h::pgm_unit).  A DDPG row is TWO networks and a chain between them; per trip of a wavefront:
//   1. the row's observation and recorded action, and its n-step return -- ddpg_update.hip's expression, operation for
//      operation; the lower lane half stores it;
//   2. critic on (obs, action): first layer (I = O + 1 <= 4 inputs) per lane on the lane's units; c2 = relu(W1c c1 + b1c)
//      on the matrix cores, the accumulator started from the bias; q per lane, ONE exchange between the halves;
//      d2 = relu'(c2) dq Woc; d1 = relu'(c1) W1c^T d2, the mirror product; dW1c += d2 c1^T contracts over the ROWS from
//      the wavefront's unit-major staged c1 and d2, 16 MFMAs per 32 x 32 tile into accumulators that live for the launch;
//   3. actor on obs: first layer per lane, second on the matrix cores with W1a, head, one exchange,
//      mu = fmaf(action_scale, tanhf(z), action_bias); a1 and a2 stay staged for step 5;
//   4. critic on (obs, mu): forward as in 2; dj2 = relu' (-1 / rows) Woc; dj1 = relu' W1c^T dj2 on the matrix cores;
//      dmu = sum_j dj1[j] W0c[j][O] per lane and one exchange.  Nothing of this pass is staged or reaches the critic's gradient;
//   5. actor backward: dz = (dmu action_scale) (1 - th th); f2; f1 = relu' W1a^T f2 on the matrix cores; dW1a += f2 a1^T.
// Eight H x H products per row tile.  All four A operands -- each network's W1 as W1[unit][32 to + r] for the mirror
// product and transposed for the forward one -- are ONE conflict-free LDS read per MFMA from copies with rows padded by 8
// (rows 4 apart, the two lane halves, are 32 banks apart); no weight lives in registers, which leaves them to the two
// networks' dW1 accumulators (2 x H / 32 x H / 32 x 16).  The small tensors (dW0, db0, db1, dWo) are vector sums over the
// staged tiles: a lane adds its sixteen rows from +0, in row order, and that sum to the launch's accumulator of unit
// 32 t + r; dbo and the two loss sums are one number per row slot and trip.
//
// A wavefront's staged arrays are its own: writer and readers are lanes of ONE wavefront, ordered by a wavefront-scope
// fence.  The trip loop has NO block barrier: the four wavefronts of a block run their chains independently.
//
// ORDER (the parity contract of pg_update_common.h).  No float atomics, nothing between blocks.  A lane accumulates tiles
// ascending; at the end a wavefront adds its upper half to its lower half, the wavefronts add into the block's partial in
// wavefront order, the per-row sums are added row slot by row slot: two launches on the same inputs give the same bytes.
// A block without rows writes zeros; rows past `rows` are never read and contribute exactly zero; relu'(0) = 0.
//
// Dynamic LDS: dgm_lds_floats(H, O) floats (training/ddpg_update_kernels.py::gradients_matrix_lds_bytes).
#include "pg_update_matrix_common.h"   // PGM_LD, pgm_f16, the lane's unit list, the staged arrays; pg_update_common.h

#define DGM_THREADS 256
#define DGM_WAVES 4
#define DGM_TILE 128                   // rows per block tile
#define DGM_ROW_SUMS 4                 // per row slot: dq (dboc), (Q - ret)^2, dz (dboa), Q(obs, mu(obs))

constexpr int ddpg_net_floats(int H, int I) { return H * I + H + H * H + H + H + 1; }

// One network.  F_*: the flat buffer, as ddpg_update.hip's DdpgNet has it (restated: that unit is not touched).  The
// rest: its small tensors in LDS -- everything but W1 -- as W0 [H][I], b0, b1, Wo, bo.
template <int H, int I>
struct DgmNet {
  static constexpr int F_W0 = 0, F_B0 = H * I, F_W1 = F_B0 + H, F_B1 = F_W1 + H * H, F_WO = F_B1 + H, F_BO = F_WO + H;
  static constexpr int N = F_BO + 1;
  static_assert(N == ddpg_net_floats(H, I), "the flat layout");
  static constexpr int W0 = 0, B0 = H * I, B1 = B0 + H, WO = B1 + H, BO = WO + H, SMALL = upd_pad4(BO + 1);
  static_assert(WO % 4 == 0, "Wo is read as float4");
};

// the dynamic LDS in floats: the two networks' small tensors, the four copies of W1 (actor, actor transposed, critic,
// critic transposed) with their rows padded by 8, per wavefront two staged arrays [H][PGM_LD], the staged inputs
// [O + 1][32] and the two deltas [2][32]
constexpr int dgm_lds_floats(int H, int O) {
  return upd_pad4(H * O + 3 * H + 1) + upd_pad4(H * (O + 1) + 3 * H + 1) + 4 * H * (H + 8) +
         DGM_WAVES * (2 * H * PGM_LD + (O + 3) * 32);
}

template <int H, int O>
struct DgmLds {
  static_assert(H == 32 || H == 64, "32-unit tiles, a 32-bit mask of the lane's units");
  using LA = DgmNet<H, O>;
  using LC = DgmNet<H, O + 1>;
  static constexpr int LDW = H + 8, SMALL_A = 0, SMALL_C = LA::SMALL, W1A = SMALL_C + LC::SMALL, W1AT = W1A + H * LDW;
  static constexpr int W1C = W1AT + H * LDW, W1CT = W1C + H * LDW, STAGE = W1CT + H * LDW, WAVE_STAGE = 2 * H * PGM_LD;
  static constexpr int MISC = STAGE + DGM_WAVES * WAVE_STAGE, WAVE_MISC = (O + 3) * 32, TOTAL = MISC + DGM_WAVES * WAVE_MISC;
  static_assert(TOTAL == dgm_lds_floats(H, O), "the LDS carve-up");
  static_assert(4 * TOTAL <= 160 * 1024, "one block per compute unit");
  static_assert(STAGE % 4 == 0 && MISC % 4 == 0 && WAVE_MISC % 4 == 0, "float4 reads");
  static constexpr int PA = LA::N, PC = LC::N, PT = PA + PC;
  // the block's partial and the per-row sums are formed in the staging area once the tiles are done
  static_assert(upd_pad4(PT + 2) + DGM_WAVES * 32 * DGM_ROW_SUMS <= DGM_WAVES * WAVE_STAGE, "the staging area holds the block's partial");
};

// what one lane of a wavefront wrote to LDS is visible to the wavefront's other lanes behind this
__device__ __forceinline__ void dgm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a trip's vector sum, opaque to the scheduler: the sums of a trip are formed one after the other, not all at once
__device__ __forceinline__ float dgm_finished(float sum) {
  asm volatile("" : "+v"(sum));
  return sum;
}

// what a lane holds of one network's gradient for the whole launch: dW1 as 32 x 32 accumulator tiles, the rest for unit
// 32 t + r from its sixteen rows of every trip
template <int H, int I>
struct DgmAcc {
  static constexpr int TO = H / 32;
  pgm_f16 w1[TO][TO];
  float b1[TO], b0[TO], w0[TO][I], wo[TO];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int ti = 0; ti < TO; ++ti) {
#pragma unroll
      for (int tj = 0; tj < TO; ++tj)
#pragma unroll
        for (int v = 0; v < 16; ++v) w1[ti][tj][v] = 0.0f;
      b1[ti] = b0[ti] = wo[ti] = 0.0f;
#pragma unroll
      for (int k = 0; k < I; ++k) w0[ti][k] = 0.0f;
    }
  }
};

// h1 = relu(W0 x + b0), the lane's units; `w`: the network's small tensors in LDS
template <int H, int I>
__device__ __forceinline__ void dgm_layer0(const float *w, int hf, const float (&x)[I], float (&h1)[H / 2]) {
  using L = DgmNet<H, I>;
#pragma unroll
  for (int s = 0; s < H / 2; ++s) {
    const int u = pgm_unit(s, 0) + 4 * hf;
    float acc = w[L::B0 + u];
#pragma unroll
    for (int k = 0; k < I; ++k) acc = fmaf(w[L::W0 + u * I + k], x[k], acc);
    h1[s] = fmaxf(acc, 0.0f);
  }
  __builtin_amdgcn_sched_barrier(0);
}

// h2 = relu(W1 h1 + b1) on the matrix cores, the accumulator started from the bias.  wt: the transposed copy at the
// lane's coordinates, W1[32 to + r][pgm_unit(s, hf)] at wt[pgm_unit(s, 0) * LDW + 32 to]; step s contracts unit
// pgm_unit(s, 0) from the lower half with unit pgm_unit(s, 1) from the upper one
template <int H>
__device__ __forceinline__ void dgm_layer1(const float *wt, const float *b1, int hf, const float (&h1)[H / 2], float (&h2)[H / 2]) {
  constexpr int TO = H / 32, NU = H / 2, LDW = H + 8;
  pgm_f16 z2[TO];
#pragma unroll
  for (int to = 0; to < TO; ++to)
#pragma unroll
    for (int v = 0; v < 16; ++v) z2[to][v] = b1[pgm_unit(16 * to + v, 0) + 4 * hf];
#pragma unroll
  for (int s = 0; s < NU; ++s)
#pragma unroll
    for (int to = 0; to < TO; ++to)
      z2[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[pgm_unit(s, 0) * LDW + 32 * to], h1[s], z2[to], 0, 0, 0);
#pragma unroll
  for (int to = 0; to < TO; ++to)
#pragma unroll
    for (int v = 0; v < 16; ++v) h2[16 * to + v] = fmaxf(z2[to][v], 0.0f);
  __builtin_amdgcn_sched_barrier(0);
}

// d1 = relu'(h1) * W1^T d2 on the matrix cores, from +0, masked by the lane's h1 > 0 bits.  wb: W1 at the lane's
// coordinates, W1[pgm_unit(s, hf)][32 to + r] at wb[pgm_unit(s, 0) * LDW + 32 to]
template <int H>
__device__ __forceinline__ void dgm_layer1_backward(const float *wb, const float (&d2)[H / 2], uint32_t m1, float (&d1)[H / 2]) {
  constexpr int TO = H / 32, NU = H / 2, LDW = H + 8;
  pgm_f16 acc[TO];
#pragma unroll
  for (int to = 0; to < TO; ++to)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[to][e] = 0.0f;
#pragma unroll
  for (int s = 0; s < NU; ++s)
#pragma unroll
    for (int to = 0; to < TO; ++to)
      acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[pgm_unit(s, 0) * LDW + 32 * to], d2[s], acc[to], 0, 0, 0);
#pragma unroll
  for (int to = 0; to < TO; ++to)
#pragma unroll
    for (int e = 0; e < 16; ++e) d1[16 * to + e] = ((m1 >> (16 * to + e)) & 1u) ? acc[to][e] : 0.0f;
  __builtin_amdgcn_sched_barrier(0);
}

// the lane's share of Wo h2 (the lower half starts from the bias), in the order of the lane's list
template <int H, int I>
__device__ __forceinline__ float dgm_head(const float *w, int hf, const float (&h2)[H / 2]) {
  using L = DgmNet<H, I>;
  float s = hf ? 0.0f : w[L::BO];
#pragma unroll
  for (int i = 0; i < H / 2; i += 4) {
    const float4 wr = *(const float4 *)(w + L::WO + pgm_unit(i, 0) + 4 * hf);
    s = fmaf(wr.x, h2[i], s); s = fmaf(wr.y, h2[i + 1], s);
    s = fmaf(wr.z, h2[i + 2], s); s = fmaf(wr.w, h2[i + 3], s);
  }
  return s;
}

// d2[i] = relu'(h2[i]) * d * Wo[i], the lane's units
template <int H, int I>
__device__ __forceinline__ void dgm_head_backward(const float *w, int hf, float d, uint32_t m2, float (&d2)[H / 2]) {
  using L = DgmNet<H, I>;
#pragma unroll
  for (int i = 0; i < H / 2; i += 4) {
    const float4 wr = *(const float4 *)(w + L::WO + pgm_unit(i, 0) + 4 * hf);
    d2[i] = ((m2 >> i) & 1u) ? d * wr.x : 0.0f;
    d2[i + 1] = ((m2 >> (i + 1)) & 1u) ? d * wr.y : 0.0f;
    d2[i + 2] = ((m2 >> (i + 2)) & 1u) ? d * wr.z : 0.0f;
    d2[i + 3] = ((m2 >> (i + 3)) & 1u) ? d * wr.w : 0.0f;
  }
}

// One network's backward from its head's delta `d` (staged in sd [32] by the caller, h1 in SA and h2 in SB, all behind
// a wave sync): dWo, then d2, d1 and the gradients of both hidden layers.  dW0 takes the first I inputs of SX [.][32].
template <int H, int I>
__device__ __forceinline__ void dgm_backward(DgmAcc<H, I> &g, const float *w, const float *wb, float *SA, float *SB,
                                             const float *SX, const float *sd, int r, int hf, float d, uint32_t m1, uint32_t m2) {
  constexpr int TO = H / 32, NU = H / 2;
  // ---- dWo[i] += sum_r d[r] h2[i][r]: unit 32 t + r, the half's sixteen rows
#pragma unroll
  for (int t = 0; t < TO; ++t) {
    float4 hu[4], dl[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      hu[q] = *(const float4 *)(SB + (32 * t + r) * PGM_LD + 16 * hf + 4 * q);
      dl[q] = *(const float4 *)(sd + 16 * hf + 4 * q);
    }
    g.wo[t] += dgm_finished(pgm_dot16(0.0f, dl, hu));
  }
  float d2[NU], d1[NU];
  dgm_head_backward<H, I>(w, hf, d, m2, d2);
  __builtin_amdgcn_sched_barrier(0);
  dgm_layer1_backward<H>(wb, d2, m1, d1);
  dgm_wave_sync();                   // (h2 has been read by every lane)
  pgm_stage<NU>(SB, r, hf, d2);
  dgm_wave_sync();
  // ---- dW1[i][j] += sum_r d2[i][r] h1[j][r] on the matrix cores, two rows per step (one from each half);
  //      db1[i] += sum_r d2[i][r] from the operand the lane holds
  {
    float sb1[TO];
#pragma unroll
    for (int t = 0; t < TO; ++t) sb1[t] = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float4 du[TO], hu[TO];
#pragma unroll
      for (int t = 0; t < TO; ++t) {
        du[t] = *(const float4 *)(SB + (32 * t + r) * PGM_LD + 16 * hf + 4 * q);
        hu[t] = *(const float4 *)(SA + (32 * t + r) * PGM_LD + 16 * hf + 4 * q);
        sb1[t] += du[t].x; sb1[t] += du[t].y; sb1[t] += du[t].z; sb1[t] += du[t].w;
      }
#pragma unroll
      for (int ti = 0; ti < TO; ++ti)
#pragma unroll
        for (int tj = 0; tj < TO; ++tj) {
          g.w1[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[ti].x, hu[tj].x, g.w1[ti][tj], 0, 0, 0);
          g.w1[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[ti].y, hu[tj].y, g.w1[ti][tj], 0, 0, 0);
          g.w1[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[ti].z, hu[tj].z, g.w1[ti][tj], 0, 0, 0);
          g.w1[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[ti].w, hu[tj].w, g.w1[ti][tj], 0, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < TO; ++t) g.b1[t] += sb1[t];
  }
  dgm_wave_sync();                   // (h1 has been read by every lane)
  pgm_stage<NU>(SA, r, hf, d1);
  dgm_wave_sync();
  // ---- dW0[i][k] += sum_r d1[i][r] x[k][r]; db0[i] += sum_r d1[i][r]
  //      (one unit and one input at a time, each sum finished before the next starts: with all TO x I in flight the entry spills)
#pragma unroll
  for (int t = 0; t < TO; ++t) {
    float4 du[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) du[q] = *(const float4 *)(SA + (32 * t + r) * PGM_LD + 16 * hf + 4 * q);
#pragma unroll
    for (int k = 0; k < I; ++k) {
      float4 xl[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) xl[q] = *(const float4 *)(SX + k * 32 + 16 * hf + 4 * q);
      g.w0[t][k] += dgm_finished(pgm_dot16(0.0f, du, xl));
    }
    g.b0[t] += dgm_finished(pgm_sum16(0.0f, du));
  }
  dgm_wave_sync();                   // (the staged tile is free)
}

// one wavefront's share of a network's gradient into the block's partial R (the network's flat floats), `first`: stored,
// else added
template <int H, int I>
__device__ __forceinline__ void dgm_add_partial(float *R, DgmAcc<H, I> &g, bool first, int r, int hf) {
  using L = DgmNet<H, I>;
  constexpr int TO = H / 32;
#pragma unroll
  for (int ti = 0; ti < TO; ++ti) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int unit = pgm_unit(16 * ti + e, 0) + 4 * hf;   // (register e of lane (r, hf): this unit, column r)
#pragma unroll
      for (int tj = 0; tj < TO; ++tj) {
        float *at = R + L::F_W1 + unit * H + 32 * tj + r;
        *at = first ? g.w1[ti][tj][e] : *at + g.w1[ti][tj][e];
      }
    }
    const float b0 = pgm_add_halves(g.b0[ti], hf), b1 = pgm_add_halves(g.b1[ti], hf), wo = pgm_add_halves(g.wo[ti], hf);
    float w0[I];
#pragma unroll
    for (int k = 0; k < I; ++k) w0[k] = pgm_add_halves(g.w0[ti][k], hf);
    if (hf == 0) {
      const int i = 32 * ti + r;
      float *at = R + L::F_B0 + i;
      *at = first ? b0 : *at + b0;
      at = R + L::F_B1 + i;
      *at = first ? b1 : *at + b1;
      at = R + L::F_WO + i;
      *at = first ? wo : *at + wo;
#pragma unroll
      for (int k = 0; k < I; ++k) {
        at = R + L::F_W0 + i * I + k;
        *at = first ? w0[k] : *at + w0[k];
      }
    }
  }
}

// blockDim.x = DGM_THREADS; the arguments of ddpg_update.hip::ddpg_gradients_impl
template <int H, int O>
__device__ __forceinline__ void dgm_gradients_impl(const float *__restrict__ obs, const float *__restrict__ actions,
                                                   const float *__restrict__ rewards, const int *__restrict__ done,
                                                   const float *__restrict__ next_values, const float *__restrict__ theta,
                                                   int T, int E, int n_step, float gamma, float action_scale,
                                                   float action_bias, float *__restrict__ returns_out,
                                                   float *__restrict__ partials) {
  using L = DgmLds<H, O>;
  using LA = DgmNet<H, O>;
  using LC = DgmNet<H, O + 1>;
  constexpr int I = O + 1, NU = H / 2, LDW = L::LDW, PA = L::PA, PT = L::PT;
  extern __shared__ __attribute__((aligned(16))) float dgm_lds[];
  float *wa = dgm_lds + L::SMALL_A, *wc = dgm_lds + L::SMALL_C;
  int tid = threadIdx.x;
  // ---- the two networks: the small tensors as they lie in the flat buffer around W1; W1 and its transpose, padded
  for (int i = tid; i < LA::F_W1; i += DGM_THREADS) wa[i] = theta[i];
  for (int i = tid; i < 2 * H + 1; i += DGM_THREADS) wa[LA::B1 + i] = theta[LA::F_B1 + i];
  for (int i = tid; i < LC::F_W1; i += DGM_THREADS) wc[i] = theta[PA + i];
  for (int i = tid; i < 2 * H + 1; i += DGM_THREADS) wc[LC::B1 + i] = theta[PA + LC::F_B1 + i];
  for (int i = tid; i < H * H; i += DGM_THREADS) {
    const float a = theta[LA::F_W1 + i], c = theta[PA + LC::F_W1 + i];
    const int at = (i / H) * LDW + i % H, att = (i % H) * LDW + i / H;
    dgm_lds[L::W1A + at] = a;
    dgm_lds[L::W1AT + att] = a;
    dgm_lds[L::W1C + at] = c;
    dgm_lds[L::W1CT + att] = c;
  }
  DgmAcc<H, O> ga;
  DgmAcc<H, I> gc;
  ga.clear();
  gc.clear();
  float grow[DGM_ROW_SUMS];
#pragma unroll
  for (int j = 0; j < DGM_ROW_SUMS; ++j) grow[j] = 0.0f;
  __syncthreads();

  const int V = T - n_step + 1;
  const long rows = (long)V * E;
  const long tiles = (rows + DGM_TILE - 1) / DGM_TILE;
  const float inv_rows = 1.0f / (float)rows;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    // (the weights and the lane's LDS addresses are the same for every trip: derived behind an empty asm, or the compiler
    // keeps a few hundred of them across the trips and spills them)
    int l = threadIdx.x;
    asm volatile("" : "+v"(l)::"memory");
    const int wave = l >> 6, r = l & 31, hf = (l >> 5) & 1;
    float *SA = dgm_lds + L::STAGE + wave * L::WAVE_STAGE, *SB = SA + H * PGM_LD;
    float *SX = dgm_lds + L::MISC + wave * L::WAVE_MISC, *SQ = SX + I * 32, *SZ = SQ + 32;
    const int lane_at = 4 * hf * LDW + r;
    const float *wba = dgm_lds + L::W1A + lane_at, *wta = dgm_lds + L::W1AT + lane_at;
    const float *wbc = dgm_lds + L::W1C + lane_at, *wtc = dgm_lds + L::W1CT + lane_at;
    const long g = tile * DGM_TILE + wave * 32 + r;
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
      if (hf == 0) returns_out[g] = ret;
    }
    if (hf == 0) {
#pragma unroll
      for (int k = 0; k < I; ++k) SX[k * 32 + r] = x[k];
    }

    // ======================================================================= critic loss: mse(returns, Q(obs, action))
    {
      float c1[NU], c2[NU];
      dgm_layer0<H, I>(wc, hf, x, c1);
      const uint32_t m1 = pgm_positive_mask<NU>(c1);
      pgm_stage<NU>(SA, r, hf, c1);
      dgm_layer1<H>(wtc, wc + LC::B1, hf, c1, c2);
      const uint32_t m2 = pgm_positive_mask<NU>(c2);
      pgm_stage<NU>(SB, r, hf, c2);
      const float q = pgm_add_halves(dgm_head<H, I>(wc, hf, c2), hf);
      const float diff = live ? q - ret : 0.0f;
      const float dq = (2.0f * diff) * inv_rows;
      grow[0] += dq;
      grow[1] += diff * diff;
      if (hf == 0) SQ[r] = dq;
      dgm_wave_sync();
      dgm_backward<H, I>(gc, wc, wbc, SA, SB, SX, SQ, r, hf, dq, m1, m2);
    }

    // ========================================= actor loss: -mean(Q(obs, mu(obs))), differentiated through the action only
    {
      uint32_t m1, m2;
      float th;
      {
        float xa[O], a1[NU], a2[NU];
#pragma unroll
        for (int k = 0; k < O; ++k) xa[k] = x[k];
        dgm_layer0<H, O>(wa, hf, xa, a1);
        m1 = pgm_positive_mask<NU>(a1);
        pgm_stage<NU>(SA, r, hf, a1);
        dgm_layer1<H>(wta, wa + LA::B1, hf, a1, a2);
        m2 = pgm_positive_mask<NU>(a2);
        pgm_stage<NU>(SB, r, hf, a2);
        th = tanhf(pgm_add_halves(dgm_head<H, O>(wa, hf, a2), hf));
      }
      x[O] = fmaf(action_scale, th, action_bias);
      float dmu;
      {
        float j1[NU], j2[NU];
        dgm_layer0<H, I>(wc, hf, x, j1);
        const uint32_t mj1 = pgm_positive_mask<NU>(j1);
        dgm_layer1<H>(wtc, wc + LC::B1, hf, j1, j2);
        const uint32_t mj2 = pgm_positive_mask<NU>(j2);
        const float qj = pgm_add_halves(dgm_head<H, I>(wc, hf, j2), hf);
        grow[3] += live ? qj : 0.0f;
        dgm_head_backward<H, I>(wc, hf, live ? -inv_rows : 0.0f, mj2, j2);
        __builtin_amdgcn_sched_barrier(0);
        dgm_layer1_backward<H>(wbc, j2, mj1, j1);
        float s = 0.0f;
#pragma unroll
        for (int i = 0; i < NU; ++i) s = fmaf(j1[i], wc[LC::W0 + (pgm_unit(i, 0) + 4 * hf) * I + O], s);
        dmu = pgm_add_halves(s, hf);
      }
      const float dz = (dmu * action_scale) * (1.0f - th * th);
      grow[2] += dz;
      if (hf == 0) SZ[r] = dz;
      dgm_wave_sync();
      dgm_backward<H, O>(ga, wa, wba, SA, SB, SX, SZ, r, hf, dz, m1, m2);   // (SX still holds the tile's observations)
    }
  }

  // ---- the block's partial: the halves of a wavefront, then the wavefronts in order, in LDS in the flat layout
  __syncthreads();                   // (every wavefront is done with its staged tile)
  tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int wave = tid >> 6, r = tid & 31, hf = (tid >> 5) & 1;
  float *R = dgm_lds + L::STAGE, *RS = R + upd_pad4(PT + 2);
  for (int w = 0; w < DGM_WAVES; ++w) {
    if (wave == w) {
      dgm_add_partial<H, O>(R, ga, w == 0, r, hf);
      dgm_add_partial<H, I>(R + PA, gc, w == 0, r, hf);
      if (hf == 0) {
#pragma unroll
        for (int j = 0; j < DGM_ROW_SUMS; ++j) RS[(w * 32 + r) * DGM_ROW_SUMS + j] = grow[j];
      }
    }
    __syncthreads();
  }
  if (tid < DGM_ROW_SUMS) {
    float s = 0.0f;
    for (int i = 0; i < DGM_WAVES * 32; ++i) s += RS[i * DGM_ROW_SUMS + tid];
    R[tid == 0 ? PA + LC::F_BO : tid == 1 ? PT : tid == 2 ? LA::F_BO : PT + 1] = s;
  }
  __syncthreads();
  float *out = partials + (long)blockIdx.x * (PT + 2);
  for (int i = tid; i < PT + 2; i += DGM_THREADS) out[i] = R[i];
}

extern "C" {

#define DGM_ENTRY(HH, OO)                                                                                              \
  __global__ void __launch_bounds__(DGM_THREADS, 1) HipDdpgGradientsMatrix_H##HH##_O##OO(                              \
      const float *__restrict__ obs, const float *__restrict__ actions, const float *__restrict__ rewards,             \
      const int *__restrict__ done, const float *__restrict__ next_values, const float *__restrict__ theta, int T,     \
      int E, int n_step, float gamma, float action_scale, float action_bias, float *__restrict__ returns_out,          \
      float *__restrict__ partials) {                                                                                  \
    dgm_gradients_impl<HH, OO>(obs, actions, rewards, done, next_values, theta, T, E, n_step, gamma, action_scale,     \
                               action_bias, returns_out, partials);                                                    \
  }
DGM_ENTRY(32, 2)
DGM_ENTRY(32, 3)
DGM_ENTRY(64, 2)
DGM_ENTRY(64, 3)

}  // extern "C"
