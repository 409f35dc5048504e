// pg_update_gridworld_matrix.hip -- launch 3 of the A2C / PPO update of pg_update_gridworld.hip (HipPgGwGradients_H<H>) ON
// THE FLOAT32 MATRIX CORES: HipPgGwGradientsMatrix_H<H>, the same arguments, the same partials [gridDim.x][P + 4] in the
// flat layout (W0 [H][21] unpadded ... the four sums), consumed unchanged by HipPgGwReduce and HipPgGwApply.  Opt-in
// (`trainer.fused_update_gradients: "matrix"`, training/pg_update_gridworld_kernels.py); a code object of its own.
//
// This is pg_update_matrix.hip's split with every shape a compile-time constant: 21 inputs (22 with the pad), FIVE logits
// and the value.  A block is four wavefronts on a 128-row tile (blocks stride over the tiles), a wavefront owns 32 rows,
// lanes l and l + 32 share row r = l % 32, and lane half hf = l / 32 holds of every 32 hidden units the sixteen that its
// registers of a 32 x 32 accumulator hold (pg_update_matrix_common.h::pgm_unit).  v_mfma_f32_32x32x2_f32: lane l supplies
// A[l % 32][l / 32] and B[l / 32][l % 32].  Per trip of a wavefront:
//   * the observation tile: its 32 rows are 672 contiguous floats (a row is (t, replica, agent)), loaded coalesced -- each
//     float's index is compared with what the batch still has, nothing behind rows * 21 is read -- and written transposed
//     into the wavefront's own SX [22][PGM_LD], the pad row 21 zero for the launch.  Writer and readers are lanes of ONE
//     wavefront: a wavefront-scope fence orders them, no block barrier;
//   * first layer: Z1^T = W0 x^T, 11 MFMAs per 32 units, the accumulator started from b0; step s contracts input 2 s from
//     the lower lane half and 2 s + 1 from the upper.  The A operand is one read of W0 staged k-major [22][LDK] (the pad
//     k-row zero; LDK = 32 mod 64 floats, so the lane halves sit 32 banks apart), the B operand one read of SX[2 s + hf][r];
//   * second layer forward Z2^T = W1 h1^T and backward d1^T = W1^T d2^T (the mirror product), H / 2 MFMAs per 32 units
//     each.  Both A operands are one LDS read per MFMA: the backward's from W1 [H][H + 8], the forward's from a transposed
//     copy [H][H + 8] (in registers it spills: at width 64 as in include/wd_env_update_matrix.h, at width 32 next to the
//     dW0 tile at two blocks per compute unit);
//   * heads and objective per lane on the lane's units, five logits and the value as compile-time counts, ONE exchange of
//     six partial sums between the halves of a row; the statements are policy_mlp.hip::HipPolicyGradientHead's as
//     pg_update_gridworld.hip copies them (the shift by the maximum first, `taken` clamped for logp_taken only);
//   * dW1 += d2 h1^T: the wavefront stages h1 and d2 unit-major [unit][PGM_LD] and contracts over its 32 rows, 16 MFMAs per
//     32 x 32 tile into accumulators that live for the launch;
//   * dW0 += d1 x^T as one more MFMA tile per 32 units, units by inputs: lane r supplies SX[r][16 hf ..] for r < 21 and zero
//     for r = 21 .. 31; only the 21 real columns are stored;
//   * the vector sums (db0, db1, dWp, dWv) add the trip's sixteen rows from +0 and then that sum to the launch's
//     accumulator; dbp, dbv and the four sums are one number per row slot and trip.
//
// ORDER (the parity contract of pg_update_common.h).  No float atomics, nothing between blocks.  A lane accumulates tiles
// ascending; at the end a wavefront adds its upper half to its lower half, the wavefronts add into the block's partial in
// wavefront order, the per-row sums are added row slot by row slot: two launches on the same inputs give the same bytes.
// A block without rows writes zeros; rows past `rows` contribute exactly zero; relu'(0) = 0.
//
// Dynamic LDS: gwm_lds_floats(H) floats (training/pg_update_gridworld_kernels.py::gradients_matrix_lds_bytes).
#include "pg_update_matrix_common.h"   // PGM_LD, pgm_f16, the lane's unit list, the staged arrays; pg_update_common.h

#define GWM_THREADS 256
#define GWM_WAVES 4
#define GWM_TILE 128                   // rows per block tile
#define GWM_O 21                       // observation floats of a row
#define GWM_O2 22                      // ... with the pad input of the last MFMA step
#define GWM_A 5                        // actions
#define GWM_OUTPUTS (GWM_A + 1)        // the five logits' deltas, then the value's
#define GWM_BIAS_SLOTS 8               // bp in LDS: the value head behind it starts on a 16-byte boundary
#define GWM_ROW_SUMS (GWM_OUTPUTS + 4) // per row slot: the six deltas (dbp, dbv), then the four sums

// floats between two inputs of the k-major W0: 32 mod 64, so the two lane halves of a read are 32 banks apart
constexpr int gwm_ldk(int H) { return H % 64 == 32 ? H : H + 32; }

// the dynamic LDS in floats: the network (W0 k-major, b0, b1, Wp, eight bias slots, Wv, bv, W1 and its transpose with
// their rows padded by 8), per wavefront two staged arrays [H][PGM_LD], the observation tile [22][PGM_LD] and the
// deltas [6][32]
constexpr int gwm_lds_floats(int H) {
  return upd_pad4(GWM_O2 * gwm_ldk(H) + H + H + GWM_A * H + GWM_BIAS_SLOTS + H + 1) +
         2 * H * (H + 8) + GWM_WAVES * (2 * H * PGM_LD + GWM_O2 * PGM_LD + GWM_OUTPUTS * 32);
}

template <int H>
struct GwmLds {
  static_assert(H == 32 || H == 64, "32-unit tiles, a 32-bit mask of the lane's units");
  static constexpr int LDK = gwm_ldk(H);
  static constexpr int W0T = 0, B0 = GWM_O2 * LDK, B1 = B0 + H, WP = B1 + H, BP = WP + GWM_A * H;
  static constexpr int WV = BP + GWM_BIAS_SLOTS, BV = WV + H;
  // W1 [H][LDW] for the backward product's operand and its transpose [H][LDW] for the forward's: rows 4 apart (the two
  // lane halves) are 32 banks apart
  static constexpr int LDW = H + 8, W1 = upd_pad4(BV + 1), W1T = W1 + H * LDW, NET = W1T + H * LDW;
  static constexpr int STAGE = NET, WAVE_STAGE = 2 * H * PGM_LD;
  static constexpr int MISC = STAGE + GWM_WAVES * WAVE_STAGE, WAVE_MISC = GWM_O2 * PGM_LD + GWM_OUTPUTS * 32;
  static constexpr int TOTAL = MISC + GWM_WAVES * WAVE_MISC;
  static_assert(TOTAL == gwm_lds_floats(H), "the LDS carve-up");
  static_assert(WP % 4 == 0 && WV % 4 == 0 && STAGE % 4 == 0 && MISC % 4 == 0 && WAVE_MISC % 4 == 0, "float4 reads");
  // the flat buffer, as pg_update_gridworld.hip's GwNet has it (restated: that unit is not touched)
  static constexpr int F_B0 = H * GWM_O, F_W1 = F_B0 + H, F_B1 = F_W1 + H * H, F_WP = F_B1 + H, F_BP = F_WP + GWM_A * H;
  static constexpr int F_WV = F_BP + GWM_A, F_BV = F_WV + H, P = F_BV + 1;
  static_assert(P == upd_pg_net_floats(H, GWM_O, GWM_A), "the flat layout");
  // the block's partial and the per-row sums are formed in the staging area once the tiles are done
  static_assert(upd_pad4(P + 4) + GWM_WAVES * 32 * GWM_ROW_SUMS <= GWM_WAVES * WAVE_STAGE,
                "the staging area holds the block's partial");
};

// what one lane of a wavefront wrote to LDS is visible to the wavefront's other lanes behind this
__device__ __forceinline__ void gwm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// s += sum over the lane's units of w[unit] * h[unit], in the order of the lane's list (w: a row of H floats in LDS)
template <int NU>
__device__ __forceinline__ float gwm_head_dot(float s, const float *w, int hf, const float (&h)[NU]) {
#pragma unroll
  for (int i = 0; i < NU; i += 4) {
    const float4 wr = *(const float4 *)(w + pgm_unit(i, 0) + 4 * hf);
    s = fmaf(wr.x, h[i], s); s = fmaf(wr.y, h[i + 1], s);
    s = fmaf(wr.z, h[i + 2], s); s = fmaf(wr.w, h[i + 3], s);
  }
  return s;
}

// blockDim.x = GWM_THREADS; partials [gridDim.x][P + 4]
template <int H>
__device__ __forceinline__ void gwm_gradients_impl(const float *__restrict__ obs, const int *__restrict__ actions,
                                                   const float *__restrict__ adv, const float *__restrict__ ret,
                                                   const float *__restrict__ theta, long rows, float inv_R,
                                                   float ent_coeff, float vf_coeff, float *__restrict__ partials) {
  using L = GwmLds<H>;
  constexpr int TO = H / 32, NU = H / 2, LDK = L::LDK, WAVE_FLOATS = 32 * GWM_O;
  extern __shared__ __attribute__((aligned(16))) float gwm_lds[];
  float *net = gwm_lds;
  int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hf = lane >> 5;
  float *SA = gwm_lds + L::STAGE + wave * L::WAVE_STAGE, *SB = SA + H * PGM_LD;
  float *SX = gwm_lds + L::MISC + wave * L::WAVE_MISC, *SD = SX + GWM_O2 * PGM_LD;
  // W0 k-major, the pad k-row zero: W0T[k][unit]
  for (int i = tid; i < GWM_O2 * H; i += GWM_THREADS) {
    const int k = i / H, u = i - k * H;
    net[L::W0T + k * LDK + u] = k < GWM_O ? theta[u * GWM_O + k] : 0.0f;
  }
  for (int i = tid; i < H; i += GWM_THREADS) {
    net[L::B0 + i] = theta[L::F_B0 + i];
    net[L::B1 + i] = theta[L::F_B1 + i];
  }
  for (int i = tid; i < GWM_A * H + GWM_A; i += GWM_THREADS) net[L::WP + i] = theta[L::F_WP + i];   // Wp, then bp
  for (int i = tid; i < H + 1; i += GWM_THREADS) net[L::WV + i] = theta[L::F_WV + i];
  for (int i = tid; i < H * H; i += GWM_THREADS) {
    const float w = theta[L::F_W1 + i];
    net[L::W1 + (i / H) * L::LDW + i % H] = w;
    net[L::W1T + (i % H) * L::LDW + i / H] = w;
  }
  // the pad row of the wavefront's observation tile: zero for the launch (the loads below write rows k < 21 only)
  if (lane < 32) SX[GWM_O * PGM_LD + lane] = 0.0f;
  // W1 as the A operand of the second layer's products: step s contracts unit pgm_unit(s, 0) from the lower half with unit
  // pgm_unit(s, 1) from the upper one
  const float *wt = net + L::W1T + 4 * hf * L::LDW + r;   // W1[32 to + r][pgm_unit(s, hf)] at wt[pgm_unit(s, 0) * LDW + 32 to]
  const float *wb = net + L::W1 + 4 * hf * L::LDW + r;    // W1[pgm_unit(s, hf)][32 to + r] at wb[pgm_unit(s, 0) * LDW + 32 to]
  const float *w0 = net + L::W0T + hf * LDK + r;          // W0[32 to + r][2 s + hf] at w0[2 s * LDK + 32 to]
  const float *xb = SX + hf * PGM_LD + r;                 // x[row r][2 s + hf] at xb[2 s * PGM_LD]
  pgm_f16 gw1[TO][TO], gw0[TO];
  float gb1[TO], gb0[TO], gwo[TO][GWM_OUTPUTS], grow[GWM_ROW_SUMS];
#pragma unroll
  for (int ti = 0; ti < TO; ++ti) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
#pragma unroll
      for (int tj = 0; tj < TO; ++tj) gw1[ti][tj][v] = 0.0f;
      gw0[ti][v] = 0.0f;
    }
    gb1[ti] = gb0[ti] = 0.0f;
#pragma unroll
    for (int o = 0; o < GWM_OUTPUTS; ++o) gwo[ti][o] = 0.0f;
  }
#pragma unroll
  for (int j = 0; j < GWM_ROW_SUMS; ++j) grow[j] = 0.0f;
  __syncthreads();

  const long tiles = (rows + GWM_TILE - 1) / GWM_TILE;
  const long obs_floats = rows * GWM_O;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long g = tile * GWM_TILE + wave * 32 + r;
    const bool live = g < rows;
    // ---- the wavefront's 32 rows: 672 contiguous floats, transposed into SX [k][row]
    {
      const long first = (tile * GWM_TILE + wave * 32) * GWM_O;
      const long left = obs_floats - first;              // (<= 0: the wavefront has no rows)
      const int have = left < WAVE_FLOATS ? (left > 0 ? (int)left : 0) : WAVE_FLOATS;
      const float *from = obs + first;
      // (the eleven (k, row) pairs of a lane are the same on every trip: derived behind an empty asm, or the compiler
      // keeps them across the trips and spills them)
      int l = lane;
      asm volatile("" : "+v"(l));
#pragma unroll
      for (int q0 = 0; q0 < WAVE_FLOATS; q0 += 64) {
        const int q = q0 + l;
        if (q0 + 64 <= WAVE_FLOATS || q < WAVE_FLOATS) {
          const int row = q / GWM_O, k = q - row * GWM_O;
          SX[k * PGM_LD + row] = q < have ? from[q] : 0.0f;
        }
      }
    }
    float a = 0.0f, rt = 0.0f;
    int taken = 0;
    if (live) {
      a = adv[g];
      rt = ret[g];
      taken = actions[g];
    }
    gwm_wave_sync();
    // ---- first layer on the matrix cores: the accumulator starts as the bias; the pad step adds exact zeros
    float h1[NU];
    {
      pgm_f16 z1[TO];
#pragma unroll
      for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int v = 0; v < 16; ++v) z1[to][v] = net[L::B0 + pgm_unit(16 * to + v, 0) + 4 * hf];
#pragma unroll
      for (int s = 0; s < GWM_O2 / 2; ++s) {
        const float x = xb[2 * s * PGM_LD];
#pragma unroll
        for (int to = 0; to < TO; ++to)
          z1[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[2 * s * LDK + 32 * to], x, z1[to], 0, 0, 0);
      }
#pragma unroll
      for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int v = 0; v < 16; ++v) h1[16 * to + v] = fmaxf(z1[to][v], 0.0f);
    }
    const uint32_t m1 = pgm_positive_mask<NU>(h1);
    pgm_stage<NU>(SA, r, hf, h1);
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
        for (int to = 0; to < TO; ++to)
          z2[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(wt[pgm_unit(s, 0) * L::LDW + 32 * to], h1[s], z2[to], 0, 0, 0);
#pragma unroll
      for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int v = 0; v < 16; ++v) h2[16 * to + v] = fmaxf(z2[to][v], 0.0f);
    }
    const uint32_t m2 = pgm_positive_mask<NU>(h2);
    pgm_stage<NU>(SB, r, hf, h2);
    // ---- the heads: each half sums its units (the lower half starts from the bias), one exchange, the same bits after it
    float z[GWM_A], m = -__builtin_inff();
#pragma unroll
    for (int j = 0; j < GWM_A; ++j) {
      z[j] = pgm_add_halves(gwm_head_dot<NU>(hf ? 0.0f : net[L::BP + j], net + L::WP + j * H, hf, h2), hf);
      m = fmaxf(m, z[j]);
    }
    const float v = pgm_add_halves(gwm_head_dot<NU>(hf ? 0.0f : net[L::BV], net + L::WV, hf, h2), hf);
    // HipPolicyGradientHead's statements (policy_mlp.hip), one head, as pg_update_gridworld.hip has them: the shift by the
    // maximum FIRST, then expf and logf
    float total = 0.0f;
#pragma unroll
    for (int j = 0; j < GWM_A; ++j) total += expf(z[j] - m);
    const float lse = logf(total);
    float Hent = 0.0f;
#pragma unroll
    for (int j = 0; j < GWM_A; ++j) {
      const float lp = (z[j] - m) - lse;
      Hent -= expf(lp) * lp;
    }
    const int clamped = min(max(taken, 0), GWM_A - 1);
    float logp_taken = 0.0f;
#pragma unroll
    for (int j = 0; j < GWM_A; ++j)
      if (j == clamped) logp_taken = (z[j] - m) - lse;
    float dz[GWM_A];
#pragma unroll
    for (int j = 0; j < GWM_A; ++j) {
      dz[j] = 0.0f;
      if (live) {
        const float lp = (z[j] - m) - lse, pj = expf(lp);
        dz[j] = (a * (pj - (j == taken ? 1.0f : 0.0f)) + ent_coeff * pj * (lp + Hent)) * inv_R;
      }
    }
    const float d = v - rt;
    const float dv = live ? 2.0f * vf_coeff * d * inv_R : 0.0f;
#pragma unroll
    for (int j = 0; j < GWM_A; ++j) grow[j] += dz[j];
    grow[GWM_A] += dv;
    grow[GWM_OUTPUTS + 0] += live ? logp_taken * a : 0.0f;
    grow[GWM_OUTPUTS + 1] += live ? Hent : 0.0f;
    grow[GWM_OUTPUTS + 2] += live ? d * d : 0.0f;
    grow[GWM_OUTPUTS + 3] += live ? a : 0.0f;
    if (hf == 0) {
#pragma unroll
      for (int j = 0; j < GWM_A; ++j) SD[j * 32 + r] = dz[j];
      SD[GWM_A * 32 + r] = dv;
    }
    __syncthreads();
    // ---- dWp[o][i] += sum_r dz[o][r] h2[i][r], dWv[i] += sum_r dv[r] h2[i][r]: unit 32 t + r, the half's sixteen rows
    {
      float4 hu[TO][4];
      pgm_unit_rows<TO>(SB, r, hf, hu);
#pragma unroll
      for (int o = 0; o < GWM_OUTPUTS; ++o) {
        float4 dl[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) dl[q] = *(const float4 *)(SD + o * 32 + 16 * hf + 4 * q);
#pragma unroll
        for (int t = 0; t < TO; ++t) gwo[t][o] += pgm_dot16(0.0f, dl, hu[t]);
      }
    }
    // ---- d2 = relu'(h2) * (sum_j dz[j] Wp[j] + dv Wv), j ascending from +0, the value last; the lane's units
    //      Four units at a time, as in pg_update_gridworld.hip: with all the sums in flight at once, and every count a
    //      compile-time constant, the scheduler pulls the six weight rows' reads to the front and the entry spills
    float d2[NU];
#pragma unroll
    for (int i = 0; i < NU; i += 4) {
      float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
      for (int j = 0; j < GWM_OUTPUTS; ++j) {
        const bool logit = j < GWM_A;
        const float dj = logit ? dz[logit ? j : 0] : dv;
        const float4 wr = *(const float4 *)(net + (logit ? L::WP + j * H : L::WV) + pgm_unit(i, 0) + 4 * hf);
        acc.x = fmaf(wr.x, dj, acc.x); acc.y = fmaf(wr.y, dj, acc.y);
        acc.z = fmaf(wr.z, dj, acc.z); acc.w = fmaf(wr.w, dj, acc.w);
      }
      d2[i] = ((m2 >> i) & 1u) ? acc.x : 0.0f;
      d2[i + 1] = ((m2 >> (i + 1)) & 1u) ? acc.y : 0.0f;
      d2[i + 2] = ((m2 >> (i + 2)) & 1u) ? acc.z : 0.0f;
      d2[i + 3] = ((m2 >> (i + 3)) & 1u) ? acc.w : 0.0f;
      __builtin_amdgcn_sched_barrier(0);
    }
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
      for (int t = 0; t < TO; ++t) gb1[t] += pgm_sum16(0.0f, du[t]);
    }
    __syncthreads();                 // (h1 has been read by every lane)
    pgm_stage<NU>(SA, r, hf, d1);
    __syncthreads();
    // ---- dW0[i][k] += sum_r d1[i][r] x[k][r] as a 32 x 32 tile per 32 units: unit as M, input as N (lane r supplies
    //      input r, zero behind the 21st), two rows per step; db0[i] += sum_r d1[i][r]
    {
      float4 du[TO][4];
      pgm_unit_rows<TO>(SA, r, hf, du);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 xl = r < GWM_O ? *(const float4 *)(SX + r * PGM_LD + 16 * hf + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int t = 0; t < TO; ++t) {
          gw0[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[t][q].x, xl.x, gw0[t], 0, 0, 0);
          gw0[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[t][q].y, xl.y, gw0[t], 0, 0, 0);
          gw0[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[t][q].z, xl.z, gw0[t], 0, 0, 0);
          gw0[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[t][q].w, xl.w, gw0[t], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < TO; ++t) gb0[t] += pgm_sum16(0.0f, du[t]);
    }
    __syncthreads();                 // (the staged tile is free for the next trip)
  }

  // ---- the block's partial: the halves of a wavefront, then the wavefronts in order, in LDS in the flat layout
  // (the lane's coordinates are derived again behind an empty asm: held across the trips for this they cost spilled registers)
  tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  wave = tid >> 6, r = tid & 31, hf = (tid >> 5) & 1;
#pragma unroll
  for (int t = 0; t < TO; ++t) {
    gb1[t] = pgm_add_halves(gb1[t], hf);
    gb0[t] = pgm_add_halves(gb0[t], hf);
#pragma unroll
    for (int o = 0; o < GWM_OUTPUTS; ++o) gwo[t][o] = pgm_add_halves(gwo[t][o], hf);
  }
  float *R = gwm_lds + L::STAGE, *RS = R + upd_pad4(L::P + 4);
  for (int w = 0; w < GWM_WAVES; ++w) {
    if (wave == w) {
      const bool first = w == 0;
#pragma unroll
      for (int ti = 0; ti < TO; ++ti) {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int unit = pgm_unit(16 * ti + e, 0) + 4 * hf;   // (register e of lane (r, hf): this unit, column r)
#pragma unroll
          for (int tj = 0; tj < TO; ++tj) {
            float *at = R + L::F_W1 + unit * H + 32 * tj + r;
            *at = first ? gw1[ti][tj][e] : *at + gw1[ti][tj][e];
          }
          if (r < GWM_O) {
            float *at = R + unit * GWM_O + r;
            *at = first ? gw0[ti][e] : *at + gw0[ti][e];
          }
        }
        if (hf == 0) {
          const int i = 32 * ti + r;
          float *at = R + L::F_B0 + i;
          *at = first ? gb0[ti] : *at + gb0[ti];
          at = R + L::F_B1 + i;
          *at = first ? gb1[ti] : *at + gb1[ti];
#pragma unroll
          for (int o = 0; o < GWM_OUTPUTS; ++o) {
            at = R + (o < GWM_A ? L::F_WP + o * H : L::F_WV) + i;
            *at = first ? gwo[ti][o] : *at + gwo[ti][o];
          }
        }
      }
      if (hf == 0) {
#pragma unroll
        for (int j = 0; j < GWM_ROW_SUMS; ++j) RS[(w * 32 + r) * GWM_ROW_SUMS + j] = grow[j];
      }
    }
    __syncthreads();
  }
  if (tid < GWM_ROW_SUMS) {
    float s = 0.0f;
    for (int i = 0; i < GWM_WAVES * 32; ++i) s += RS[i * GWM_ROW_SUMS + tid];
    R[tid < GWM_A ? L::F_BP + tid : tid == GWM_A ? L::F_BV : L::P + tid - GWM_OUTPUTS] = s;
  }
  __syncthreads();
  float *out = partials + (long)blockIdx.x * (L::P + 4);
  for (int i = tid; i < L::P + 4; i += GWM_THREADS) out[i] = R[i];
}

extern "C" {

#define GWM_ENTRY(HH)                                                                                                  \
  __global__ void __launch_bounds__(GWM_THREADS, 64 / HH) HipPgGwGradientsMatrix_H##HH(                                \
      const float *__restrict__ obs, const int *__restrict__ actions, const float *__restrict__ adv,                   \
      const float *__restrict__ ret, const float *__restrict__ theta, long rows, float inv_R, float ent_coeff,         \
      float vf_coeff, float *__restrict__ partials) {                                                                  \
    gwm_gradients_impl<HH>(obs, actions, adv, ret, theta, rows, inv_R, ent_coeff, vf_coeff, partials);                 \
  }
GWM_ENTRY(32)
GWM_ENTRY(64)

}  // extern "C"
