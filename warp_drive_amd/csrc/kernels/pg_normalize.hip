// pg_normalize.hip -- `normalize_return` / `normalize_advantage` of the A2C / PPO update on the kernels path
// (training/pg_update_kernels.py::_PgUpdateLaunches.normalize, `trainer.fused_update_normalize`): what
// training/losses.py::_normalise computes on x [T, E, n],
//
//     (x - mean_t) / (std_t + eps),   mean_t and the UNBIASED std_t over the C = E * n columns of tick t,
//
// as two or three launches between HipDiscountedReturns and the gradient launch.  Nothing here knows a network: the
// entries see [T][C] float32 arrays, so one set serves every user of the update launches.
//
//   HipPgTickMoments          x -> partials [T][chunks][2]: (mean, M2) of every chunk of every tick
//   HipPgNormalizeReturns     returns, values, the returns' partials -> norm_returns, advantages = norm_returns - values
//                             (and, asked for, the chunk moments of those advantages, from the registers that hold them)
//   HipPgNormalizeAdvantages  advantages, their partials -> norm_advantages
//
// WORK SPLIT.  A tick's row of C floats is cut into chunks of PGN_CHUNK = 4096 columns (the last one shorter).  One block
// of 256 threads owns one (tick, chunk): blockIdx.x = tick * chunks + chunk.  It reads the chunk ONCE, by coalesced dword
// loads (lane `tid` takes columns first + 256 k + tid, k < 16: no alignment is asked of C or of the row start), and keeps
// it in registers, 16 values per lane.
//
// MOMENTS.  The means here can lie fifty standard deviations from zero and the result is divided by std + 1e-10, so no
// sum of squares of raw values is formed anywhere.  A chunk's moments are two passes over the registers:
//     mean_chunk = (sum of x) / count,   M2 = sum of (x - mean_chunk)^2.
// A block sum is: per lane its values in k order from +0; a butterfly over the wavefront's 64 lanes (xor 1, 2, 4, 8, 16,
// 32: both partners of a step form the same commutative sum, so every lane ends with the same bits); the four wavefront
// results added from +0 in wavefront order through LDS.  No float atomics; the order never depends on timing
// (pg_update_common.h's contract).
// A tick's moments are its chunks' partials merged in ascending chunk order by the pairwise update (Chan et al.):
//     delta = mean_b - mean_a;  n = n_a + n_b;  mean = mean_a + delta (n_b / n);  M2 = M2_a + M2_b + delta^2 (n_a n_b / n)
// (a chunk's count follows from C and its index).  EVERY block of a tick repeats that merge from the same partials, so
// all blocks of a tick use bit-identical mean and std: no second grid-wide stage, no cooperative launch.
// Then std = sqrt(M2 / (C - 1)) and out = (x - mean) / (std + eps), the framework's expression with its division (the
// build's correctly rounded divide and square root).  C >= 2 (the host refuses C < 2: the unbiased std is NaN there).
//
// Outputs are out of place: the raw returns and the advantages before their normalisation stay for the metrics.
#include <hip/hip_runtime.h>

#define PGN_THREADS 256
#define PGN_PER_LANE 16
#define PGN_CHUNK (PGN_THREADS * PGN_PER_LANE)

// what a block owns: tick `tick` (its row starts at float `row`), the columns first .. first + count - 1
struct PgnChunk {
  long row;
  int tick, first, count;
};

__device__ __forceinline__ PgnChunk pgn_chunk(int C, int chunks) {
  const int t = blockIdx.x / chunks, first = (blockIdx.x % chunks) * PGN_CHUNK;
  return {(long)t * (long)C, t, first, min(PGN_CHUNK, C - first)};
}

// r[k] = x[row + first + 256 k + tid], 0 past the chunk's end
__device__ __forceinline__ void pgn_load(const float *__restrict__ x, const PgnChunk &w, float (&r)[PGN_PER_LANE]) {
#pragma unroll
  for (int k = 0; k < PGN_PER_LANE; ++k) {
    const int j = k * PGN_THREADS + (int)threadIdx.x;
    r[k] = j < w.count ? x[w.row + w.first + j] : 0.0f;
  }
}

__device__ __forceinline__ void pgn_store(float *__restrict__ out, const PgnChunk &w, const float (&r)[PGN_PER_LANE]) {
#pragma unroll
  for (int k = 0; k < PGN_PER_LANE; ++k) {
    const int j = k * PGN_THREADS + (int)threadIdx.x;
    if (j < w.count) out[w.row + w.first + j] = r[k];
  }
}

// the block's sum of every lane's `lane`, the same bits in every thread; `slot`: four floats of LDS nobody else uses
__device__ __forceinline__ float pgn_block_sum(float lane, float *slot) {
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) lane += __shfl_xor(lane, step, 64);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = lane;
  __syncthreads();
  float s = 0.0f;
#pragma unroll
  for (int wave = 0; wave < PGN_THREADS / 64; ++wave) s += slot[wave];
  return s;
}

// (mean, M2) of the chunk held in r; `slots`: eight floats of LDS
__device__ __forceinline__ void pgn_chunk_moments(const float (&r)[PGN_PER_LANE], int count, float *slots, float &mean,
                                                  float &m2) {
  float s = 0.0f;
#pragma unroll
  for (int k = 0; k < PGN_PER_LANE; ++k) s += r[k];   // (a value past the chunk's end is +0)
  mean = pgn_block_sum(s, slots) / (float)count;
  float q = 0.0f;
#pragma unroll
  for (int k = 0; k < PGN_PER_LANE; ++k) {
    const float d = k * PGN_THREADS + (int)threadIdx.x < count ? r[k] - mean : 0.0f;
    q += d * d;
  }
  m2 = pgn_block_sum(q, slots + 4);
}

// the tick's (mean, std) from its chunks' partials `p` [chunks][2], merged in ascending chunk order
__device__ __forceinline__ void pgn_tick_mean_std(const float *__restrict__ p, int C, int chunks, float &mean, float &std_) {
  float m2 = p[1], n_a = (float)min(PGN_CHUNK, C);
  mean = p[0];
  for (int b = 1; b < chunks; ++b) {
    const float n_b = (float)min(PGN_CHUNK, C - b * PGN_CHUNK), n = n_a + n_b;
    const float delta = p[2 * b] - mean;
    mean = mean + delta * (n_b / n);
    m2 = m2 + p[2 * b + 1] + delta * delta * (n_a * n_b / n);
    n_a = n;
  }
  std_ = sqrtf(m2 / (float)(C - 1));
}

__device__ __forceinline__ void pgn_write_partial(float *__restrict__ partials, float mean, float m2) {
  if (threadIdx.x == 0) {
    partials[2 * (long)blockIdx.x] = mean;
    partials[2 * (long)blockIdx.x + 1] = m2;
  }
}

extern "C" {

// grid = T * chunks blocks of 256 (every entry; a launch with another geometry or C < 2 touches nothing)
__global__ void __launch_bounds__(PGN_THREADS) HipPgTickMoments(const float *__restrict__ x, int T, int C, int chunks,
                                                                float *__restrict__ partials) {
  __shared__ float slots[8];
  if (C < 2 || chunks != (C + PGN_CHUNK - 1) / PGN_CHUNK || (long)gridDim.x != (long)T * chunks) return;
  const PgnChunk w = pgn_chunk(C, chunks);
  float r[PGN_PER_LANE], mean, m2;
  pgn_load(x, w, r);
  pgn_chunk_moments(r, w.count, slots, mean, m2);
  pgn_write_partial(partials, mean, m2);
}

// partials_adv: null, or [T][chunks][2] for the chunk moments of the advantages this launch writes
__global__ void __launch_bounds__(PGN_THREADS) HipPgNormalizeReturns(
    const float *__restrict__ returns, const float *__restrict__ values, const float *__restrict__ partials, int T, int C,
    int chunks, float eps, float *__restrict__ norm_returns, float *__restrict__ advantages, float *__restrict__ partials_adv) {
  __shared__ float slots[8];
  if (C < 2 || chunks != (C + PGN_CHUNK - 1) / PGN_CHUNK || (long)gridDim.x != (long)T * chunks) return;
  const PgnChunk w = pgn_chunk(C, chunks);
  float r[PGN_PER_LANE], v[PGN_PER_LANE], mean, std_;
  pgn_load(returns, w, r);
  pgn_load(values, w, v);
  pgn_tick_mean_std(partials + 2 * (long)w.tick * chunks, C, chunks, mean, std_);
  const float denom = std_ + eps;
#pragma unroll
  for (int k = 0; k < PGN_PER_LANE; ++k) r[k] = (r[k] - mean) / denom;
  pgn_store(norm_returns, w, r);
#pragma unroll
  for (int k = 0; k < PGN_PER_LANE; ++k)   // (past the chunk's end: +0, which the moments below rely on)
    r[k] = k * PGN_THREADS + (int)threadIdx.x < w.count ? r[k] - v[k] : 0.0f;
  pgn_store(advantages, w, r);
  if (partials_adv != nullptr) {   // (the same for every thread of the launch: the barriers inside are safe)
    float mean_adv, m2_adv;
    pgn_chunk_moments(r, w.count, slots, mean_adv, m2_adv);
    pgn_write_partial(partials_adv, mean_adv, m2_adv);
  }
}

__global__ void __launch_bounds__(PGN_THREADS) HipPgNormalizeAdvantages(
    const float *__restrict__ advantages, const float *__restrict__ partials, int T, int C, int chunks, float eps,
    float *__restrict__ norm_advantages) {
  if (C < 2 || chunks != (C + PGN_CHUNK - 1) / PGN_CHUNK || (long)gridDim.x != (long)T * chunks) return;
  const PgnChunk w = pgn_chunk(C, chunks);
  float r[PGN_PER_LANE], mean, std_;
  pgn_load(advantages, w, r);
  pgn_tick_mean_std(partials + 2 * (long)w.tick * chunks, C, chunks, mean, std_);
  const float denom = std_ + eps;
#pragma unroll
  for (int k = 0; k < PGN_PER_LANE; ++k) r[k] = (r[k] - mean) / denom;
  pgn_store(norm_advantages, w, r);
}

}  // extern "C"
