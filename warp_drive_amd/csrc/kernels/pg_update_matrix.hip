// pg_update_matrix.hip -- launch 3 of the A2C / PPO update of pg_update.hip (HipPgGradients_H<H>_O<O>) with its three
// H x H products per row on the float32 matrix cores: HipPgGradientsMx_H<H>_O<O>, the same arguments, the same partials
// [gridDim.x][P + 4] in the flat layout, consumed unchanged by HipPgReduce and HipPgApply.  Opt-in
// (`trainer.fused_update_gradients: "matrix"`, training/pg_update_kernels.py); a code object of its own.
//
// v_mfma_f32_32x32x2_f32: D[32][32] += A[32][2] B[2][32], products and sums in float32.  Lane l supplies A[l % 32][l / 32]
// and B[l / 32][l % 32]; register v of lane l holds D[8 (v / 4) + 4 (l / 32) + v % 4][l % 32].
//
// SPLIT.  A block is four wavefronts, a block tile 128 rows (blocks stride over the tiles), a wavefront owns 32 rows of
// it: lanes l and l + 32 share row r = l % 32 and lane half hf = l / 32 holds, of every 32 hidden units 32 t .. 32 t + 31,
// the sixteen units 32 t + 8 q + 4 hf + c (q, c < 4) -- the rows of D its registers hold.  So with "hidden unit" as M
// and "row of the batch" as N
//   second layer forward   Z^T = W1 h1^T   the contraction walks the lane's own unit list, one unit from each half per
//                          step, and Z lands on the lane that owns the row, in the lane's own units: no shuffle;
//   second layer backward  d1^T = W1^T d2^T, the mirror product;
// with the forward's arrangement of W1 in registers for the whole launch (H / 32 x H / 2 floats, gathered once from global
// memory) and the backward's read from LDS, one conflict-free read per MFMA.  The first layer (O <= 6 inputs), the heads
// (A + 1 outputs) and the objective are per-lane fmaf chains on the lane's units; the two halves of a row meet in ONE
// exchange of A + 1 partial sums and from there on compute the same bits.  The objective's statements are
// policy_mlp.hip::HipPolicyGradientHead's as pg_update.hip copies them.
//   weight gradient        dW1 += d2 h1^T contracts over the ROWS: the wavefront stages its 32 x H h1 and d2 in LDS
//                          unit-major and reads them back unit per lane (lane (m, hf): unit 32 t + m, rows 16 hf .. 16 hf +
//                          15, four float4 reads), 16 MFMAs per 32 x 32 tile of dW1 into accumulators that live for the launch.
// The small tensors are vector sums over the same staged tiles: a lane adds its sixteen rows, in row order, to the
// entries of unit 32 t + m (dWp, dWv from h2 and the staged deltas; dW0, db0 from d1 and the staged inputs; db1 from the
// d2 operand it already holds); dbp, dbv and the four sums are per-row numbers a lane adds up for its own row slot.
//
// ORDER.  No float atomics, nothing between blocks.  A lane accumulates tiles ascending; at the end a wavefront adds its
// upper half to its lower half, the wavefronts add into the block's partial in wavefront order, the per-row sums are added
// wavefront by wavefront, row slot by row slot: two launches on the same inputs give the same bytes.  A block without
// rows writes zeros; rows past `rows` are never read and contribute exactly zero; relu'(0) = 0.
//
// Dynamic LDS: PgmLds<H, O>::TOTAL floats (training/pg_update_kernels.py::gradients_matrix_lds_bytes).
#include "pg_update_matrix_common.h"   // PGM_LD, pgm_f16, the lane's unit list, the staged arrays

#define PGM_THREADS 256
#define PGM_WAVES 4
#define PGM_TILE 128              // rows per block tile
#define PGM_MAX_ACTIONS 8
#define PGM_OUTPUTS (PGM_MAX_ACTIONS + 1)   // the logits' deltas (those below A are real), then the value's
#define PGM_MAX_OBS 6
#define PGM_ROW_SUMS (PGM_OUTPUTS + 4)      // per row slot: the nine deltas (dbp, dbv), then the four sums

// LDS, in floats: the network (Wp as eight rows, so everything behind it sits at a fixed 16-byte aligned offset; W1
// last, its rows padded), then per wavefront two staged arrays [H][PGM_LD], then per wavefront the staged inputs [6][32]
// and deltas [9][32]
template <int H, int O>
struct PgmLds {
  static_assert(H % 32 == 0 && O % 2 == 0 && O <= PGM_MAX_OBS, "32-unit tiles; rows of W0 are read as float2");
  static constexpr int W0 = 0, B0 = H * O, B1 = B0 + H, WP = B1 + H, BP = WP + PGM_MAX_ACTIONS * H;
  static constexpr int WV = BP + PGM_MAX_ACTIONS, BV = WV + H;
  // W1 [H][LDW] for the backward product's operand: rows 4 apart (the two lane halves) are 32 banks apart
  static constexpr int LDW = H + 8, W1 = upd_pad4(BV + 1), NET = W1 + H * LDW;
  static constexpr int STAGE = NET, WAVE_STAGE = 2 * H * PGM_LD;
  static constexpr int MISC = STAGE + PGM_WAVES * WAVE_STAGE, WAVE_MISC = (PGM_MAX_OBS + PGM_OUTPUTS) * 32;
  static constexpr int TOTAL = MISC + PGM_WAVES * WAVE_MISC;
  // the block's partial and the per-row sums are formed in the staging area once the tiles are done
  static_assert(upd_pad4(upd_pg_net_floats(H, O, PGM_MAX_ACTIONS) + 4) + PGM_WAVES * 32 * PGM_ROW_SUMS <=
                PGM_WAVES * WAVE_STAGE, "the staging area holds the block's partial");
};

template <int H, int O>
__device__ __forceinline__ void pgm_gradients_impl(const float *__restrict__ obs, const int *__restrict__ actions,
                                                   const float *__restrict__ adv, const float *__restrict__ ret,
                                                   const float *__restrict__ theta, long rows, int A, float inv_R,
                                                   float ent_coeff, float vf_coeff, float *__restrict__ partials) {
  using L = PgmLds<H, O>;
  constexpr int TO = H / 32, NU = H / 2;
  extern __shared__ __attribute__((aligned(16))) float pgm_lds[];
  float *net = pgm_lds;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hf = lane >> 5;
  float *SA = pgm_lds + L::STAGE + wave * L::WAVE_STAGE, *SB = SA + H * PGM_LD;
  float *SX = pgm_lds + L::MISC + wave * L::WAVE_MISC, *SD = SX + PGM_MAX_OBS * 32;
  // the flat buffer's offsets (A logits)
  const int W1F = H * O + H, B1F = W1F + H * H, WPF = B1F + H, BPF = WPF + A * H, WVF = BPF + A, BVF = WVF + H;
  const int P = BVF + 1;
  for (int i = tid; i < H * O + H; i += PGM_THREADS) net[i] = theta[i];
  for (int i = tid; i < H; i += PGM_THREADS) net[L::B1 + i] = theta[B1F + i];
  for (int i = tid; i < A * H; i += PGM_THREADS) net[L::WP + i] = theta[WPF + i];
  for (int i = tid; i < A; i += PGM_THREADS) net[L::BP + i] = theta[BPF + i];
  for (int i = tid; i < H + 1; i += PGM_THREADS) net[L::WV + i] = theta[WVF + i];
  for (int i = tid; i < H * H; i += PGM_THREADS) net[L::W1 + (i / H) * L::LDW + i % H] = theta[W1F + i];
  // W1 as the A operand of both products, in the order the lane halves walk their units: step s contracts unit
  // pgm_unit(s, 0) from the lower half with unit pgm_unit(s, 1) from the upper one.  The forward's arrangement
  // (W1[32 to + r][unit]) stays in registers for the launch; the backward's (W1[unit][32 to + r]) is one conflict-free
  // LDS read per 64-cycle MFMA: both in registers spill at H = 64
  float wf[TO][NU];
#pragma unroll
  for (int to = 0; to < TO; ++to)
#pragma unroll
    for (int s = 0; s < NU; ++s) wf[to][s] = theta[W1F + (32 * to + r) * H + pgm_unit(s, 0) + 4 * hf];
  const float *wb = net + L::W1 + 4 * hf * L::LDW + r;
  pgm_f16 gw1[TO][TO];
  float gb1[TO], gb0[TO], gw0[TO][O], gwo[TO][PGM_OUTPUTS], grow[PGM_ROW_SUMS];
#pragma unroll
  for (int ti = 0; ti < TO; ++ti) {
#pragma unroll
    for (int tj = 0; tj < TO; ++tj)
#pragma unroll
      for (int v = 0; v < 16; ++v) gw1[ti][tj][v] = 0.0f;
    gb1[ti] = gb0[ti] = 0.0f;
#pragma unroll
    for (int k = 0; k < O; ++k) gw0[ti][k] = 0.0f;
#pragma unroll
    for (int o = 0; o < PGM_OUTPUTS; ++o) gwo[ti][o] = 0.0f;
  }
#pragma unroll
  for (int j = 0; j < PGM_ROW_SUMS; ++j) grow[j] = 0.0f;
  __syncthreads();

  const long tiles = (rows + PGM_TILE - 1) / PGM_TILE;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long g = tile * PGM_TILE + wave * 32 + r;
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
    // ---- first layer, the lane's units
    float h1[NU];
#pragma unroll
    for (int s = 0; s < NU; ++s) {
      const int u = pgm_unit(s, 0) + 4 * hf;
      float acc = net[L::B0 + u];
#pragma unroll
      for (int k = 0; k < O; k += 2) {
        const float2 wr = *(const float2 *)(net + L::W0 + u * O + k);
        acc = fmaf(wr.x, x[k], acc); acc = fmaf(wr.y, x[k + 1], acc);
      }
      h1[s] = fmaxf(acc, 0.0f);
    }
    const uint32_t m1 = pgm_positive_mask<NU>(h1);
    pgm_stage<NU>(SA, r, hf, h1);
    if (hf == 0) {
#pragma unroll
      for (int k = 0; k < O; ++k) SX[k * 32 + r] = x[k];
    }
    // ---- second layer forward on the matrix cores: the accumulator starts as the bias
    float h2[NU];
    {
      pgm_f16 z2[TO];
#pragma unroll
      for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int v = 0; v < 16; ++v) z2[to][v] = net[L::B1 + pgm_unit(16 * to + v, 0) + 4 * hf];
#pragma unroll
      for (int s = 0; s < NU; ++s)
#pragma unroll
        for (int to = 0; to < TO; ++to) z2[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[to][s], h1[s], z2[to], 0, 0, 0);
#pragma unroll
      for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int v = 0; v < 16; ++v) h2[16 * to + v] = fmaxf(z2[to][v], 0.0f);
    }
    const uint32_t m2 = pgm_positive_mask<NU>(h2);
    pgm_stage<NU>(SB, r, hf, h2);
    // ---- the heads: each half sums its units (the lower half starts from the bias), one exchange, the same bits after it
    float z[PGM_MAX_ACTIONS], m = -__builtin_inff();
#pragma unroll
    for (int j = 0; j < PGM_MAX_ACTIONS; ++j) {
      z[j] = -__builtin_inff();
      if (j < A) {
        float s = hf ? 0.0f : net[L::BP + j];
#pragma unroll
        for (int i = 0; i < NU; i += 4) {
          const float4 wr = *(const float4 *)(net + L::WP + j * H + pgm_unit(i, 0) + 4 * hf);
          s = fmaf(wr.x, h2[i], s); s = fmaf(wr.y, h2[i + 1], s);
          s = fmaf(wr.z, h2[i + 2], s); s = fmaf(wr.w, h2[i + 3], s);
        }
        z[j] = pgm_add_halves(s, hf);
        m = fmaxf(m, z[j]);
      }
    }
    float v;
    {
      float s = hf ? 0.0f : net[L::BV];
#pragma unroll
      for (int i = 0; i < NU; i += 4) {
        const float4 wr = *(const float4 *)(net + L::WV + pgm_unit(i, 0) + 4 * hf);
        s = fmaf(wr.x, h2[i], s); s = fmaf(wr.y, h2[i + 1], s);
        s = fmaf(wr.z, h2[i + 2], s); s = fmaf(wr.w, h2[i + 3], s);
      }
      v = pgm_add_halves(s, hf);
    }
    // HipPolicyGradientHead's statements (policy_mlp.hip), one head, as pg_update.hip has them: the shift by the maximum
    // FIRST, then expf and logf
    float total = 0.0f;
#pragma unroll
    for (int j = 0; j < PGM_MAX_ACTIONS; ++j)
      if (j < A) total += expf(z[j] - m);
    const float lse = logf(total);
    float Hent = 0.0f;
#pragma unroll
    for (int j = 0; j < PGM_MAX_ACTIONS; ++j)
      if (j < A) {
        const float lp = (z[j] - m) - lse;
        Hent -= expf(lp) * lp;
      }
    const int clamped = min(max(taken, 0), A - 1);
    float logp_taken = 0.0f;
#pragma unroll
    for (int j = 0; j < PGM_MAX_ACTIONS; ++j)
      if (j == clamped) logp_taken = (z[j] - m) - lse;
    float dz[PGM_MAX_ACTIONS];
#pragma unroll
    for (int j = 0; j < PGM_MAX_ACTIONS; ++j) {
      dz[j] = 0.0f;
      if (j < A && live) {
        const float lp = (z[j] - m) - lse, pj = expf(lp);
        dz[j] = (a * (pj - (j == taken ? 1.0f : 0.0f)) + ent_coeff * pj * (lp + Hent)) * inv_R;
      }
    }
    const float d = v - rt;
    const float dv = live ? 2.0f * vf_coeff * d * inv_R : 0.0f;
#pragma unroll
    for (int j = 0; j < PGM_MAX_ACTIONS; ++j) grow[j] += dz[j];
    grow[PGM_MAX_ACTIONS] += dv;
    grow[PGM_OUTPUTS + 0] += live ? logp_taken * a : 0.0f;
    grow[PGM_OUTPUTS + 1] += live ? Hent : 0.0f;
    grow[PGM_OUTPUTS + 2] += live ? d * d : 0.0f;
    grow[PGM_OUTPUTS + 3] += live ? a : 0.0f;
    if (hf == 0) {
#pragma unroll
      for (int j = 0; j < PGM_MAX_ACTIONS; ++j) SD[j * 32 + r] = dz[j];
      SD[PGM_MAX_ACTIONS * 32 + r] = dv;
    }
    __syncthreads();
    // ---- dWp[o][i] += sum_r dz[o][r] h2[i][r], dWv[i] += sum_r dv[r] h2[i][r]: unit 32 t + r, the half's sixteen rows
    {
      float4 hu[TO][4];
      pgm_unit_rows<TO>(SB, r, hf, hu);
#pragma unroll
      for (int o = 0; o < PGM_OUTPUTS; ++o)
        if (o < A || o == PGM_MAX_ACTIONS) {
          float4 dl[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) dl[q] = *(const float4 *)(SD + o * 32 + 16 * hf + 4 * q);
#pragma unroll
          for (int t = 0; t < TO; ++t) gwo[t][o] = pgm_dot16(gwo[t][o], dl, hu[t]);
        }
    }
    // ---- d2 = relu'(h2) * (sum_j dz[j] Wp[j] + dv Wv), j ascending from +0, the value last; the lane's units
    float d2[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) d2[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < PGM_MAX_ACTIONS; ++j)
      if (j < A) {
#pragma unroll
        for (int i = 0; i < NU; i += 4) {
          const float4 wr = *(const float4 *)(net + L::WP + j * H + pgm_unit(i, 0) + 4 * hf);
          d2[i] = fmaf(wr.x, dz[j], d2[i]); d2[i + 1] = fmaf(wr.y, dz[j], d2[i + 1]);
          d2[i + 2] = fmaf(wr.z, dz[j], d2[i + 2]); d2[i + 3] = fmaf(wr.w, dz[j], d2[i + 3]);
        }
      }
#pragma unroll
    for (int i = 0; i < NU; i += 4) {
      const float4 wr = *(const float4 *)(net + L::WV + pgm_unit(i, 0) + 4 * hf);
      d2[i] = fmaf(wr.x, dv, d2[i]); d2[i + 1] = fmaf(wr.y, dv, d2[i + 1]);
      d2[i + 2] = fmaf(wr.z, dv, d2[i + 2]); d2[i + 3] = fmaf(wr.w, dv, d2[i + 3]);
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) d2[i] = ((m2 >> i) & 1u) ? d2[i] : 0.0f;
    // ---- second layer backward on the matrix cores: d1^T = W1^T d2^T, masked by the lane's h1 > 0 bits
    float d1[NU];
    {
      pgm_f16 acc[TO];
#pragma unroll
      for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[to][e] = 0.0f;
#pragma unroll
      for (int s = 0; s < NU; ++s)
#pragma unroll
        for (int to = 0; to < TO; ++to)
          acc[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(wb[pgm_unit(s, 0) * L::LDW + 32 * to], d2[s], acc[to], 0, 0, 0);
#pragma unroll
      for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int e = 0; e < 16; ++e) d1[16 * to + e] = ((m1 >> (16 * to + e)) & 1u) ? acc[to][e] : 0.0f;
    }
    __syncthreads();                 // (h2 has been read by every lane)
    pgm_stage<NU>(SB, r, hf, d2);
    __syncthreads();
    // ---- dW1[i][j] += sum_r d2[i][r] h1[j][r] on the matrix cores, two rows per step (one from each half);
    //      db1[i] += sum_r d2[i][r] from the operand the lane holds
    {
      float4 du[TO][4], hu[TO][4];
      pgm_unit_rows<TO>(SB, r, hf, du);
      pgm_unit_rows<TO>(SA, r, hf, hu);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int ti = 0; ti < TO; ++ti)
#pragma unroll
          for (int tj = 0; tj < TO; ++tj) {
            gw1[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[ti][q].x, hu[tj][q].x, gw1[ti][tj], 0, 0, 0);
            gw1[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[ti][q].y, hu[tj][q].y, gw1[ti][tj], 0, 0, 0);
            gw1[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[ti][q].z, hu[tj][q].z, gw1[ti][tj], 0, 0, 0);
            gw1[ti][tj] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[ti][q].w, hu[tj][q].w, gw1[ti][tj], 0, 0, 0);
          }
#pragma unroll
      for (int t = 0; t < TO; ++t) gb1[t] = pgm_sum16(gb1[t], du[t]);
    }
    __syncthreads();                 // (h1 has been read by every lane)
    pgm_stage<NU>(SA, r, hf, d1);
    __syncthreads();
    // ---- dW0[i][k] += sum_r d1[i][r] x[k][r]; db0[i] += sum_r d1[i][r]
    {
      float4 du[TO][4];
      pgm_unit_rows<TO>(SA, r, hf, du);
#pragma unroll
      for (int k = 0; k < O; ++k) {
        float4 xl[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) xl[q] = *(const float4 *)(SX + k * 32 + 16 * hf + 4 * q);
#pragma unroll
        for (int t = 0; t < TO; ++t) gw0[t][k] = pgm_dot16(gw0[t][k], du[t], xl);
      }
#pragma unroll
      for (int t = 0; t < TO; ++t) gb0[t] = pgm_sum16(gb0[t], du[t]);
    }
    __syncthreads();                 // (the staged tile is free for the next trip)
  }

  // ---- the block's partial: the halves of a wavefront, then the wavefronts in order, in LDS in the flat layout
#pragma unroll
  for (int t = 0; t < TO; ++t) {
    gb1[t] = pgm_add_halves(gb1[t], hf);
    gb0[t] = pgm_add_halves(gb0[t], hf);
#pragma unroll
    for (int k = 0; k < O; ++k) gw0[t][k] = pgm_add_halves(gw0[t][k], hf);
#pragma unroll
    for (int o = 0; o < PGM_OUTPUTS; ++o) gwo[t][o] = pgm_add_halves(gwo[t][o], hf);
  }
  float *R = pgm_lds + L::STAGE, *RS = R + upd_pad4(P + 4);
  for (int w = 0; w < PGM_WAVES; ++w) {
    if (wave == w) {
      const bool first = w == 0;
#pragma unroll
      for (int ti = 0; ti < TO; ++ti) {
#pragma unroll
        for (int tj = 0; tj < TO; ++tj)
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            float *at = R + W1F + (pgm_unit(16 * ti + e, 0) + 4 * hf) * H + 32 * tj + r;
            *at = first ? gw1[ti][tj][e] : *at + gw1[ti][tj][e];
          }
        if (hf == 0) {
          const int i = 32 * ti + r;
          float *at = R + H * O + i;
          *at = first ? gb0[ti] : *at + gb0[ti];
          at = R + B1F + i;
          *at = first ? gb1[ti] : *at + gb1[ti];
#pragma unroll
          for (int k = 0; k < O; ++k) {
            at = R + i * O + k;
            *at = first ? gw0[ti][k] : *at + gw0[ti][k];
          }
#pragma unroll
          for (int o = 0; o < PGM_OUTPUTS; ++o)
            if (o < A || o == PGM_MAX_ACTIONS) {
              at = R + (o < A ? WPF + o * H : WVF) + i;
              *at = first ? gwo[ti][o] : *at + gwo[ti][o];
            }
        }
      }
      if (hf == 0) {
#pragma unroll
        for (int j = 0; j < PGM_ROW_SUMS; ++j) RS[(w * 32 + r) * PGM_ROW_SUMS + j] = grow[j];
      }
    }
    __syncthreads();
  }
  if (tid < PGM_ROW_SUMS) {
    float s = 0.0f;
    for (int i = 0; i < PGM_WAVES * 32; ++i) s += RS[i * PGM_ROW_SUMS + tid];
    if (tid < A) R[BPF + tid] = s;
    else if (tid == PGM_MAX_ACTIONS) R[BVF] = s;
    else if (tid > PGM_MAX_ACTIONS) R[P + tid - PGM_OUTPUTS] = s;
  }
  __syncthreads();
  float *out = partials + (long)blockIdx.x * (P + 4);
  for (int i = tid; i < P + 4; i += PGM_THREADS) out[i] = R[i];
}

extern "C" {

// (an entry launched with another width or observation size than its own, or with A outside 1 .. 8, touches nothing)
#define PGM_ENTRY(HH, OO)                                                                                              \
  __global__ void __launch_bounds__(PGM_THREADS, 64 / HH) HipPgGradientsMx_H##HH##_O##OO(                              \
      const float *__restrict__ obs, const int *__restrict__ actions, const float *__restrict__ adv,                   \
      const float *__restrict__ ret, const float *__restrict__ theta, long rows, int H, int O, int A, float inv_R,     \
      float ent_coeff, float vf_coeff, float *__restrict__ partials) {                                                 \
    if (H != HH || O != OO || A < 1 || A > PGM_MAX_ACTIONS) return;                                                    \
    pgm_gradients_impl<HH, OO>(obs, actions, adv, ret, theta, rows, A, inv_R, ent_coeff, vf_coeff, partials);          \
  }
PGM_ENTRY(32, 2)
PGM_ENTRY(32, 4)
PGM_ENTRY(32, 6)
PGM_ENTRY(64, 2)
PGM_ENTRY(64, 4)
PGM_ENTRY(64, 6)

}  // extern "C"
