// wd_env_update_matrix.h -- the gradient launch of the update kit (include/wd_env_update.h) ON THE FLOAT32 MATRIX CORES,
// for an observation size F = 1 .. 32 the author fixes at compile time.  One macro, next to WD_PG_UPDATE_ENTRIES:
//
//     #include "wd_env_update.h"
//     #include "wd_env_update_matrix.h"
//     WD_PG_UPDATE_ENTRIES(MyEnv, 5)
//     WD_PG_UPDATE_MX_ENTRIES(MyEnv, 5)
//
// defines HipMyEnvPgGradientsMx_H32 / _H64: the argument list of HipMyEnvPgGradients_H*, the same partials
// [gridDim.x][P + 4] in the flat layout, consumed unchanged by HipMyEnvPgReduce and HipMyEnvPgApply.  A is 1 .. 8 at run
// time; an entry launched with A outside that range touches nothing.  256 threads, __launch_bounds__(256, 64 / H); dynamic
// LDS: wd_pg_gradients_mx_lds_floats(H, F) floats (training/pg_update_custom_kernels.py::gradients_matrix_lds_bytes).
// Opt-in: `trainer.fused_update_gradients: "matrix"` (docs/custom_environments.md, "The update as kernels").
//
// The split, the second layer's two products, dW1, the heads and the order of every sum are csrc/kernels/
// pg_update_matrix.hip's, stated there: a block is four wavefronts on a 128-row tile, a wavefront owns 32 rows, lanes l and
// l + 32 share row r = l % 32 and lane half hf = l / 32 holds the sixteen units per 32 that its accumulator registers hold.
// What this header has of its own (v_mfma_f32_32x32x2_f32: lane l supplies A[l % 32][l / 32] and B[l / 32][l % 32]):
//   * the observation tile: a wavefront's 32 rows are 32 F contiguous floats, loaded coalesced (floats behind rows * F read
//     as zero and are never loaded) and written transposed into the wavefront's own SX [F2][PGM_LD], k-major, F2 = F
//     rounded up to even, the pad row zero for the whole launch.  Writer and readers are lanes of ONE wavefront: a
//     wavefront-scope fence orders them, no block barrier;
//   * the first layer on the matrix cores for every F: Z1^T = W0 x^T, hidden unit as M, batch row as N, the accumulator
//     starts as b0, step s contracts input 2 s from the lower lane half and 2 s + 1 from the upper one: F2 / 2 MFMAs per
//     32-unit tile, the B operand one read of SX[2 s + hf][r], and h1 lands on the lane that owns the row in the lane's
//     own unit list.  The A operand W0[32 to + r][2 s + hf] is read from LDS, where W0 sits k-major with a zero pad column
//     ([F2][LDK], LDK = 32 mod 64 floats: the lane halves 32 banks apart, one conflict-free read per MFMA): in registers it
//     spills next to the dW0 tile at H = 64;
//   * dW0 += d1 x^T in two forms chosen by F.  F <= 16: vector sums, the lane of unit 32 t + m adds its sixteen rows per
//     input, each float4 of SX feeding four fmaf.  F > 16: a 32 x 32 MFMA tile per 32 units, contracting over the rows (16
//     MFMAs per tile and trip): the A operand is the d1 rows the lane reads for db0 anyway, the B operand SX[m][16 hf ..] for
//     m < F and zero from the lanes with m >= F; the accumulators live for the launch.  Either form holds at most 16 H / 32
//     accumulator registers.  (16 F fmaf against 16 MFMAs; docs/rounds/r49.md: equal cost at F = 16 | 17.)
//
// The vector sums (dW0 for F <= 16, db0, db1, dWp, dWv) add a trip's sixteen rows from +0 and then that sum to the
// launch-long accumulator, so no chain of additions is longer than the trips of a block (at 160 trips a single chain
// would be 2560 long: docs/rounds/r48.md found the lanes entry's over the float32 bound at that depth).
//
// THE PARITY CONTRACT of pg_update_common.h holds: no float atomics, nothing between blocks, every sum in a fixed order
// (tiles ascending per lane; the upper half added to the lower; the wavefronts into the block's partial in wavefront
// order; the per-row sums row slot by row slot), so two launches on the same inputs give the same bytes; relu'(0) = 0; rows
// past `rows` are never read and contribute exactly zero; a block without rows writes zeros.  The objective's statements
// are policy_mlp.hip::HipPolicyGradientHead's, the shift by the maximum first.
//
// REGISTERS.  The width-32 entries sit at the 256 registers two blocks per compute unit leave a lane, the width-64 entries
// at 400 to 470 of 512.  Zero scratch and zero spilled vector registers are CHECKED at F = 1, 5, 16, 17 and 32 only
// (tests/test_custom_env_update_matrix_build.py); at another F, or with another compiler, an entry may spill -- correct, but
// slower.  An author can read it off the built object: `.private_segment_fixed_size` and `.vgpr_spill_count` of the entry in
// the notes of the code object (`llvm-readelf --notes <object>.hsaco`), or hipcc's -Rpass-analysis=kernel-resource-usage.
//
// Like wd_env_update.h this header is not self-contained: it includes the package's csrc/kernels/
// pg_update_matrix_common.h (and through it pg_update_common.h), which a custom environment's build finds with -I.
#pragma once
#include "pg_update_matrix_common.h"

#define WD_UPDM_THREADS 256
#define WD_UPDM_WAVES 4
#define WD_UPDM_TILE 128                                 // rows per block tile
#define WD_UPDM_MAX_ACTIONS 8
#define WD_UPDM_OUTPUTS (WD_UPDM_MAX_ACTIONS + 1)        // the logits' deltas (those below A are real), then the value's
#define WD_UPDM_MAX_OBS 32
#define WD_UPDM_ROW_SUMS (WD_UPDM_OUTPUTS + 4)           // per row slot: the nine deltas (dbp, dbv), then the four sums
#define WD_UPDM_VECTOR_DW0_MAX_OBS 16                    // above it dW0 is an MFMA tile

constexpr int wd_updm_even(int F) { return (F + 1) & ~1; }
// floats between two inputs of the k-major W0: = 32 mod 64, so the two lane halves of a read are 32 banks apart
constexpr int wd_updm_ldk(int H) { return H % 64 == 32 ? H : H + 32; }

// the forward operand of the second layer (W1[32 to + r][unit]) is read from LDS, not held in registers, at this width
constexpr bool wd_updm_w1t_in_lds(int H) { return H == 64; }

// the dynamic LDS in floats: the network (W0 k-major, b0, b1, eight head rows, eight bias slots, Wv, bv, W1 with its rows
// padded by 8), per wavefront two staged arrays [H][PGM_LD], the observation tile [F2][PGM_LD] and the deltas [9][32]
constexpr int wd_pg_gradients_mx_lds_floats(int H, int F) {
  return upd_pad4(wd_updm_even(F) * wd_updm_ldk(H) + H + H + WD_UPDM_MAX_ACTIONS * H + WD_UPDM_MAX_ACTIONS + H + 1) +
         (wd_updm_w1t_in_lds(H) ? 2 : 1) * H * (H + 8) +
         WD_UPDM_WAVES * (2 * H * PGM_LD + wd_updm_even(F) * PGM_LD + WD_UPDM_OUTPUTS * 32);
}

template <int H, int F>
struct WdUpdmLds {
  static_assert(H == 32 || H == 64, "32-unit tiles, a 32-bit mask of the lane's units");
  static_assert(F >= 1 && F <= WD_UPDM_MAX_OBS, "the update kit takes 1 to 32 observation floats");
  static constexpr int F2 = wd_updm_even(F), LDK = wd_updm_ldk(H);
  static constexpr int W0T = 0, B0 = F2 * LDK, B1 = B0 + H, WP = B1 + H, BP = WP + WD_UPDM_MAX_ACTIONS * H;
  static constexpr int WV = BP + WD_UPDM_MAX_ACTIONS, BV = WV + H;
  // W1 [H][LDW] for the backward product's operand: rows 4 apart (the two lane halves) are 32 banks apart
  static constexpr int LDW = H + 8, W1 = upd_pad4(BV + 1);
  // ... and W1 transposed, [H][LDW] too, for the forward product's operand where it is not in registers
  static constexpr bool W1T_IN_LDS = wd_updm_w1t_in_lds(H);
  static constexpr int W1T = W1 + H * LDW, NET = W1T + (W1T_IN_LDS ? H * LDW : 0);
  static constexpr int STAGE = NET, WAVE_STAGE = 2 * H * PGM_LD;
  static constexpr int MISC = STAGE + WD_UPDM_WAVES * WAVE_STAGE, WAVE_MISC = F2 * PGM_LD + WD_UPDM_OUTPUTS * 32;
  static constexpr int TOTAL = MISC + WD_UPDM_WAVES * WAVE_MISC;
  static_assert(TOTAL == wd_pg_gradients_mx_lds_floats(H, F), "the LDS carve-up");
  static_assert(WP % 4 == 0 && WV % 4 == 0 && STAGE % 4 == 0 && MISC % 4 == 0 && WAVE_MISC % 4 == 0, "float4 reads");
  // the block's partial and the per-row sums are formed in the staging area once the tiles are done
  static_assert(upd_pad4(upd_pg_net_floats(H, F, WD_UPDM_MAX_ACTIONS) + 4) + WD_UPDM_WAVES * 32 * WD_UPDM_ROW_SUMS <=
                WD_UPDM_WAVES * WAVE_STAGE, "the staging area holds the block's partial");
};

// what one lane of a wavefront wrote to LDS is visible to the wavefront's other lanes behind this
__device__ __forceinline__ void wd_updm_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// blockDim.x = WD_UPDM_THREADS; partials [gridDim.x][P + 4]
template <int H, int F>
__device__ __forceinline__ void wd_updm_gradients(const float *__restrict__ obs, const int *__restrict__ actions,
                                                  const float *__restrict__ adv, const float *__restrict__ ret,
                                                  const float *__restrict__ theta, long rows, int A, float inv_R,
                                                  float ent_coeff, float vf_coeff, float *__restrict__ partials) {
  using L = WdUpdmLds<H, F>;
  constexpr int TO = H / 32, NU = H / 2, F2 = L::F2, LDK = L::LDK, MAXA = WD_UPDM_MAX_ACTIONS;
  constexpr bool MFMA_DW0 = F > WD_UPDM_VECTOR_DW0_MAX_OBS;
  constexpr int KV = MFMA_DW0 ? 1 : F;      // dW0 accumulators of the vector form, per 32-unit tile
  extern __shared__ __attribute__((aligned(16))) float wd_updm_lds[];
  float *net = wd_updm_lds;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hf = lane >> 5;
  float *SA = wd_updm_lds + L::STAGE + wave * L::WAVE_STAGE, *SB = SA + H * PGM_LD;
  float *SX = wd_updm_lds + L::MISC + wave * L::WAVE_MISC, *SD = SX + F2 * PGM_LD;
  // the flat buffer's offsets (A logits)
  const int W1F = H * F + H, B1F = W1F + H * H, WPF = B1F + H, BPF = WPF + A * H, WVF = BPF + A, BVF = WVF + H;
  const int P = BVF + 1;
  // W0 k-major, the pad column zero: W0T[k][unit]
  for (int i = tid; i < F2 * H; i += WD_UPDM_THREADS) {
    const int k = i / H, u = i - k * H;
    net[L::W0T + k * LDK + u] = k < F ? theta[u * F + k] : 0.0f;
  }
  for (int i = tid; i < H; i += WD_UPDM_THREADS) {
    net[L::B0 + i] = theta[H * F + i];
    net[L::B1 + i] = theta[B1F + i];
  }
  for (int i = tid; i < A * H; i += WD_UPDM_THREADS) net[L::WP + i] = theta[WPF + i];
  for (int i = tid; i < A; i += WD_UPDM_THREADS) net[L::BP + i] = theta[BPF + i];
  for (int i = tid; i < H + 1; i += WD_UPDM_THREADS) net[L::WV + i] = theta[WVF + i];
  for (int i = tid; i < H * H; i += WD_UPDM_THREADS) {
    const float w = theta[W1F + i];
    net[L::W1 + (i / H) * L::LDW + i % H] = w;
    if constexpr (L::W1T_IN_LDS) net[L::W1T + (i % H) * L::LDW + i / H] = w;
  }
  // the pad row of the wavefront's observation tile: zero for the launch (the loads below write rows k < F only)
  if (F2 > F && lane < 32) SX[F * PGM_LD + lane] = 0.0f;
  // W1 as the A operand of the second layer's products (pg_update_matrix.hip): the forward's arrangement in registers
  // for the launch, the backward's read from LDS
  float wf[L::W1T_IN_LDS ? 1 : TO][L::W1T_IN_LDS ? 1 : NU];
  if constexpr (!L::W1T_IN_LDS) {
#pragma unroll
    for (int to = 0; to < TO; ++to)
#pragma unroll
      for (int s = 0; s < NU; ++s) wf[to][s] = theta[W1F + (32 * to + r) * H + pgm_unit(s, 0) + 4 * hf];
  }
  const float *wt = net + L::W1T + 4 * hf * L::LDW + r;   // W1[32 to + r][pgm_unit(s, hf)] at wt[pgm_unit(s, 0) * LDW + 32 to]
  const float *wb = net + L::W1 + 4 * hf * L::LDW + r;
  const float *w0 = net + L::W0T + hf * LDK + r;       // W0[32 to + r][2 s + hf] at w0[2 s * LDK + 32 to]
  const float *xb = SX + hf * PGM_LD + r;              // x[row r][2 s + hf] at xb[2 s * PGM_LD]
  pgm_f16 gw1[TO][TO], gw0m[MFMA_DW0 ? TO : 1];
  float gb1[TO], gb0[TO], gw0[TO][KV], gwo[TO][WD_UPDM_OUTPUTS], grow[WD_UPDM_ROW_SUMS];
#pragma unroll
  for (int ti = 0; ti < TO; ++ti) {
#pragma unroll
    for (int tj = 0; tj < TO; ++tj)
#pragma unroll
      for (int v = 0; v < 16; ++v) gw1[ti][tj][v] = 0.0f;
    if constexpr (MFMA_DW0) {
#pragma unroll
      for (int v = 0; v < 16; ++v) gw0m[ti][v] = 0.0f;
    }
    gb1[ti] = gb0[ti] = 0.0f;
#pragma unroll
    for (int k = 0; k < KV; ++k) gw0[ti][k] = 0.0f;
#pragma unroll
    for (int o = 0; o < WD_UPDM_OUTPUTS; ++o) gwo[ti][o] = 0.0f;
  }
#pragma unroll
  for (int j = 0; j < WD_UPDM_ROW_SUMS; ++j) grow[j] = 0.0f;
  __syncthreads();

  const long tiles = (rows + WD_UPDM_TILE - 1) / WD_UPDM_TILE;
  const long obs_floats = rows * F;
  for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long g = tile * WD_UPDM_TILE + wave * 32 + r;
    const bool live = g < rows;
    // ---- the wavefront's 32 rows: 32 F contiguous floats, transposed into SX [k][row]
    {
      const long first = (tile * WD_UPDM_TILE + wave * 32) * F;
      const long left = obs_floats - first;            // (<= 0: the wavefront has no rows)
      const int have = left < 32 * F ? (left > 0 ? (int)left : 0) : 32 * F;
      const float *from = obs + first;
#pragma unroll
      for (int q0 = 0; q0 < 32 * F; q0 += 64) {
        const int q = q0 + lane;
        if (q0 + 64 <= 32 * F || q < 32 * F) {
          const int row = q / F, k = q - row * F;
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
    wd_updm_wave_sync();
    // ---- first layer on the matrix cores: the accumulator starts as the bias; a pad step adds exact zeros
    float h1[NU];
    {
      pgm_f16 z1[TO];
#pragma unroll
      for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int v = 0; v < 16; ++v) z1[to][v] = net[L::B0 + pgm_unit(16 * to + v, 0) + 4 * hf];
#pragma unroll
      for (int s = 0; s < F2 / 2; ++s) {
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
        for (int to = 0; to < TO; ++to) {
          float w;
          if constexpr (L::W1T_IN_LDS) w = wt[pgm_unit(s, 0) * L::LDW + 32 * to];
          else w = wf[to][s];
          z2[to] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, h1[s], z2[to], 0, 0, 0);
        }
#pragma unroll
      for (int to = 0; to < TO; ++to)
#pragma unroll
        for (int v = 0; v < 16; ++v) h2[16 * to + v] = fmaxf(z2[to][v], 0.0f);
    }
    const uint32_t m2 = pgm_positive_mask<NU>(h2);
    pgm_stage<NU>(SB, r, hf, h2);
    // ---- the heads: each half sums its units (the lower half starts from the bias), one exchange, the same bits after it
    float z[MAXA], m = -__builtin_inff();
#pragma unroll
    for (int j = 0; j < MAXA; ++j) {
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
    // HipPolicyGradientHead's statements (policy_mlp.hip), one head, as wd_env_update.h has them: the shift by the
    // maximum FIRST, then expf and logf
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
    float dz[MAXA];
#pragma unroll
    for (int j = 0; j < MAXA; ++j) {
      dz[j] = 0.0f;
      if (j < A && live) {
        const float lp = (z[j] - m) - lse, pj = expf(lp);
        dz[j] = (a * (pj - (j == taken ? 1.0f : 0.0f)) + ent_coeff * pj * (lp + Hent)) * inv_R;
      }
    }
    const float d = v - rt;
    const float dv = live ? 2.0f * vf_coeff * d * inv_R : 0.0f;
#pragma unroll
    for (int j = 0; j < MAXA; ++j) grow[j] += dz[j];
    grow[MAXA] += dv;
    grow[WD_UPDM_OUTPUTS + 0] += live ? logp_taken * a : 0.0f;
    grow[WD_UPDM_OUTPUTS + 1] += live ? Hent : 0.0f;
    grow[WD_UPDM_OUTPUTS + 2] += live ? d * d : 0.0f;
    grow[WD_UPDM_OUTPUTS + 3] += live ? a : 0.0f;
    if (hf == 0) {
#pragma unroll
      for (int j = 0; j < MAXA; ++j) SD[j * 32 + r] = dz[j];
      SD[MAXA * 32 + r] = dv;
    }
    __syncthreads();
    // ---- dWp[o][i] += sum_r dz[o][r] h2[i][r], dWv[i] += sum_r dv[r] h2[i][r]: unit 32 t + r, the half's sixteen rows
    {
      float4 hu[TO][4];
      pgm_unit_rows<TO>(SB, r, hf, hu);
#pragma unroll
      for (int o = 0; o < WD_UPDM_OUTPUTS; ++o)
        if (o < A || o == MAXA) {
          float4 dl[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) dl[q] = *(const float4 *)(SD + o * 32 + 16 * hf + 4 * q);
#pragma unroll
          for (int t = 0; t < TO; ++t) gwo[t][o] += pgm_dot16(0.0f, dl, hu[t]);
        }
    }
    // ---- d2 = relu'(h2) * (sum_j dz[j] Wp[j] + dv Wv), j ascending from +0, the value last; the lane's units
    float d2[NU];
#pragma unroll
    for (int i = 0; i < NU; ++i) d2[i] = 0.0f;
#pragma unroll
    for (int j = 0; j < MAXA; ++j)
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
      for (int t = 0; t < TO; ++t) gb1[t] += pgm_sum16(0.0f, du[t]);
    }
    __syncthreads();                 // (h1 has been read by every lane)
    pgm_stage<NU>(SA, r, hf, d1);
    __syncthreads();
    // ---- dW0[i][k] += sum_r d1[i][r] x[k][r]; db0[i] += sum_r d1[i][r]
    {
      float4 du[TO][4];
      pgm_unit_rows<TO>(SA, r, hf, du);
      if constexpr (MFMA_DW0) {
        // a 32 x 32 tile per 32 units: unit as M, input as N (lane r supplies input r, zero behind F), two rows per step
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 xl = r < F ? *(const float4 *)(SX + r * PGM_LD + 16 * hf + 4 * q) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
          for (int t = 0; t < TO; ++t) {
            gw0m[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[t][q].x, xl.x, gw0m[t], 0, 0, 0);
            gw0m[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[t][q].y, xl.y, gw0m[t], 0, 0, 0);
            gw0m[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[t][q].z, xl.z, gw0m[t], 0, 0, 0);
            gw0m[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(du[t][q].w, xl.w, gw0m[t], 0, 0, 0);
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < KV; ++k) {
          float4 xl[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) xl[q] = *(const float4 *)(SX + k * PGM_LD + 16 * hf + 4 * q);
#pragma unroll
          for (int t = 0; t < TO; ++t) gw0[t][k] += pgm_dot16(0.0f, du[t], xl);
        }
      }
#pragma unroll
      for (int t = 0; t < TO; ++t) gb0[t] += pgm_sum16(0.0f, du[t]);
    }
    __syncthreads();                 // (the staged tile is free for the next trip)
  }

  const auto epilogue = [&](const int tid) {
    const int wave = tid >> 6, lane = tid & 63, r = lane & 31, hf = lane >> 5;
    (void)lane;
#pragma unroll
    for (int t = 0; t < TO; ++t) {
      gb1[t] = pgm_add_halves(gb1[t], hf);
      gb0[t] = pgm_add_halves(gb0[t], hf);
      if constexpr (!MFMA_DW0) {
#pragma unroll
        for (int k = 0; k < KV; ++k) gw0[t][k] = pgm_add_halves(gw0[t][k], hf);
      }
#pragma unroll
      for (int o = 0; o < WD_UPDM_OUTPUTS; ++o) gwo[t][o] = pgm_add_halves(gwo[t][o], hf);
    }
    float *R = wd_updm_lds + L::STAGE, *RS = R + upd_pad4(P + 4);
    for (int w = 0; w < WD_UPDM_WAVES; ++w) {
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
          if constexpr (MFMA_DW0) {     // (register e of lane (r, hf): unit pgm_unit(16 ti + e, hf), input r)
#pragma unroll
            for (int e = 0; e < 16; ++e)
              if (r < F) {
                float *at = R + (pgm_unit(16 * ti + e, 0) + 4 * hf) * F + r;
                *at = first ? gw0m[ti][e] : *at + gw0m[ti][e];
              }
          }
          if (hf == 0) {
            const int i = 32 * ti + r;
            float *at = R + H * F + i;
            *at = first ? gb0[ti] : *at + gb0[ti];
            at = R + B1F + i;
            *at = first ? gb1[ti] : *at + gb1[ti];
            if constexpr (!MFMA_DW0) {
#pragma unroll
              for (int k = 0; k < KV; ++k) {
                at = R + i * F + k;
                *at = first ? gw0[ti][k] : *at + gw0[ti][k];
              }
            }
#pragma unroll
            for (int o = 0; o < WD_UPDM_OUTPUTS; ++o)
              if (o < A || o == MAXA) {
                at = R + (o < A ? WPF + o * H : WVF) + i;
                *at = first ? gwo[ti][o] : *at + gwo[ti][o];
              }
          }
        }
        if (hf == 0) {
#pragma unroll
          for (int j = 0; j < WD_UPDM_ROW_SUMS; ++j) RS[(w * 32 + r) * WD_UPDM_ROW_SUMS + j] = grow[j];
        }
      }
      __syncthreads();
    }
    if (tid < WD_UPDM_ROW_SUMS) {
      float s = 0.0f;
      for (int i = 0; i < WD_UPDM_WAVES * 32; ++i) s += RS[i * WD_UPDM_ROW_SUMS + tid];
      if (tid < A) R[BPF + tid] = s;
      else if (tid == MAXA) R[BVF] = s;
      else if (tid > MAXA) R[P + tid - WD_UPDM_OUTPUTS] = s;
    }
    __syncthreads();
    float *out = partials + (long)blockIdx.x * (P + 4);
    for (int i = tid; i < P + 4; i += WD_UPDM_THREADS) out[i] = R[i];
  };
  // ---- the block's partial: the halves of a wavefront, then the wavefronts in order, in LDS in the flat layout
  // (at width 32 the lane's coordinates are derived again behind an empty asm: held across the trips they cost the
  // entries of F > 16 three spilled registers; at width 64 it is the other way round)
  int tid_again = threadIdx.x;
  if constexpr (H == 32) asm volatile("" : "+v"(tid_again));
  epilogue(tid_again);
}

#define WD_PG_UPDATE_MX_WIDTH_ENTRY_(Name, F, HH)                                                                      \
  extern "C" __global__ void __launch_bounds__(WD_UPDM_THREADS, 64 / HH) Hip##Name##PgGradientsMx_H##HH(               \
      const float *__restrict__ obs, const int *__restrict__ actions, const float *__restrict__ adv,                   \
      const float *__restrict__ ret, const float *__restrict__ theta, long rows, int A, float inv_R, float ent_coeff,  \
      float vf_coeff, float *__restrict__ partials) {                                                                  \
    if (A < 1 || A > WD_UPDM_MAX_ACTIONS) return;                                                                      \
    wd_updm_gradients<HH, F>(obs, actions, adv, ret, theta, rows, A, inv_R, ent_coeff, vf_coeff, partials);            \
  }

// the two matrix-core gradient entries of one environment: Name and F as given to WD_PG_UPDATE_ENTRIES
#define WD_PG_UPDATE_MX_ENTRIES(Name, F)                                                                               \
  WD_PG_UPDATE_MX_WIDTH_ENTRY_(Name, F, 32)                                                                            \
  WD_PG_UPDATE_MX_WIDTH_ENTRY_(Name, F, 64)
