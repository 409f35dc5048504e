// pg_downsample.hip -- `trainer.neg_pos_env_ratio` of the A2C / PPO update on the kernels path
// (training/pg_update_kernels.py::_PgUpdateLaunches.downsample, `trainer.fused_update_downsample`): what
// training/losses.py::_sample_positive_negative_env_ids and the fancy indexing after it do,
//
//     positives = replicas with done == 2 at any tick;  neg = int(pos * ratio);
//     pos == 0 or pos + neg >= E: every replica stays;  else: all positives and a uniform `neg` of the others,
//
// as three launches before HipPgValues.  Everything here is integer work or copies: all results are exact and every
// launch writes the same bytes.  No float atomics, no scratch.
//
//   HipPgSelectScan      done [T][E] -> positive [E], key [E], one positive count per block
//   HipPgSelectKeep      key, positive, the block counts, ratio -> keep_ids [K] ascending, counts = (K, pos, negatives kept)
//   HipPgGatherColumns   up to four arrays [T][E][w] -> [T][K][w] by keep_ids
//
// THE DRAW.  Replica e's key in update number `epoch` is word 0 of wd_philox4x32_10 with counter
// (e, epoch, stream_tag, 6) and the trainer's seed words.  Counter word 3 = 6 is this file's stream; 0 to 5 are taken
// (0 sample_actions, 1 the OU process, 2 the reset pool -- wd_core.hip; 3 the two-head tick, 4 the single-head tick --
// wd_common.h; 5 the in-kernel policies -- mlp_forward.h, classic_control.hip, the tick kit).  The kept negatives are the
// `neg` smallest (key, e) pairs among the negatives: independent uniform keys, so a uniform subset; a tie on the key goes
// to the lower replica id.
//
// SCAN.  One lane per replica column, 256 per block: the T loads of a wavefront are 64 consecutive dwords.  A block's
// positive count is four ballots' popcounts added through LDS.
//
// KEEP.  ONE block of 1024 threads.  The neg-th smallest key is found by a radix select, most significant byte first:
// four passes, each a 256-bin histogram in LDS (integer atomics) over the negatives whose higher bytes equal the prefix
// found so far, each striding over the E keys; 256 threads then locate the bin that holds the wanted rank.  That leaves
// the threshold key v and r = how many of the negatives with key == v are taken (the lowest r replica ids among them).
// The compaction walks e in chunks of 1024 in ascending order: per chunk two block scans (wavefront ballot + popcount,
// then the sixteen wavefront totals through LDS) -- the rank of a replica among the key == v negatives, then among the
// kept -- carried from chunk to chunk in registers every thread holds alike.
//
// GATHER.  blockIdx.x = tick * chunks + chunk of 256 kept columns; the chunk's keep_ids go to LDS once.  Per array the
// chunk's output is one contiguous run of count * w words, written coalesced; a row moves as 16-byte accesses when
// w % 4 == 0 and both bases are 16-byte aligned, as dwords otherwise.  All offsets are 64-bit.  An id outside 0 .. E - 1
// (never written by HipPgSelectKeep) is not followed: its row is left as it is.
#include "wd_common.h"

#define PGS_SCAN_THREADS 256
#define PGS_KEEP_THREADS 1024
#define PGS_KEEP_WAVES (PGS_KEEP_THREADS / 64)
#define PGS_GATHER_THREADS 256
#define PGS_GATHER_CHUNK 256
#define PGS_COUNTER_WORD 6u

// lanes of this wavefront below mine in which `pred` holds, and (total) in all of it
__device__ __forceinline__ int pgs_wave_rank(bool pred, int &total) {
  const unsigned long long mask = __ballot(pred);
  total = __popcll(mask);
  return __popcll(mask & ((1ull << (threadIdx.x & 63u)) - 1ull));
}

// exclusive rank of `pred` over the block's 1024 threads in thread order, `total` for the whole block; `slots`: sixteen
// ints of LDS nobody else uses until the next barrier after this call
__device__ __forceinline__ int pgs_block_rank(bool pred, int *slots, int &total) {
  int wave_total;
  int rank = pgs_wave_rank(pred, wave_total);
  if ((threadIdx.x & 63u) == 0) slots[threadIdx.x >> 6] = wave_total;
  __syncthreads();
  total = 0;
#pragma unroll
  for (int w = 0; w < PGS_KEEP_WAVES; ++w) {
    const int c = slots[w];
    if (w < (int)(threadIdx.x >> 6)) rank += c;
    total += c;
  }
  return rank;
}

template <typename V>
__device__ __forceinline__ void pgs_gather(const V *__restrict__ src, V *__restrict__ dst, int w, long t, long E, long K,
                                           long first, int count, const int *ids) {
  const long out = (t * K + first) * (long)w, in = t * E;
  for (int j = threadIdx.x; j < count * w; j += PGS_GATHER_THREADS) {
    const int col = j / w, i = j - col * w, id = ids[col];
    if (id >= 0 && (long)id < E) dst[out + j] = src[(in + id) * (long)w + i];
  }
}

__device__ __forceinline__ void pgs_gather_array(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, int w, long t,
                                                 long E, long K, long first, int count, const int *ids) {
  if (src == nullptr || dst == nullptr || w < 1) return;
  if ((w & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0)
    pgs_gather((const uint4 *)src, (uint4 *)dst, w >> 2, t, E, K, first, count, ids);
  else
    pgs_gather(src, dst, w, t, E, K, first, count, ids);
}

extern "C" {

// grid = ceil(E / 256) blocks of 256 (a launch with another geometry touches nothing)
__global__ void __launch_bounds__(PGS_SCAN_THREADS) HipPgSelectScan(
    const int *__restrict__ done, int T, int E, uint32_t epoch, uint32_t stream_tag, uint32_t seed_lo, uint32_t seed_hi,
    int *__restrict__ positive, uint32_t *__restrict__ keys, int *__restrict__ block_counts) {
  __shared__ int slots[PGS_SCAN_THREADS / 64];
  if (T < 1 || E < 1 || (long)gridDim.x != ((long)E + PGS_SCAN_THREADS - 1) / PGS_SCAN_THREADS) return;
  const long e = (long)blockIdx.x * PGS_SCAN_THREADS + threadIdx.x;
  bool pos = false;
  if (e < E) {
    for (int t = 0; t < T; ++t) pos |= done[(long)t * E + e] == 2;
    positive[e] = pos ? 1 : 0;
    keys[e] = wd_philox4x32_10(wd_u4{(uint32_t)e, epoch, stream_tag, PGS_COUNTER_WORD}, seed_lo, seed_hi).x;
  }
  int total;
  pgs_wave_rank(pos, total);
  if ((threadIdx.x & 63u) == 0) slots[threadIdx.x >> 6] = total;
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = slots[0] + slots[1] + slots[2] + slots[3];
}

// ONE block of 1024; keep_ids has room for E ids, counts for three ints
__global__ void __launch_bounds__(PGS_KEEP_THREADS) HipPgSelectKeep(
    const uint32_t *__restrict__ keys, const int *__restrict__ positive, const int *__restrict__ block_counts, int n_blocks,
    int E, double ratio, int *__restrict__ keep_ids, int *__restrict__ counts) {
  __shared__ int hist[256];
  __shared__ int slots_a[PGS_KEEP_WAVES], slots_b[PGS_KEEP_WAVES];
  __shared__ int sum, chosen_bin, chosen_rank;
  if (E < 1 || n_blocks < 1 || gridDim.x != 1 || blockDim.x != PGS_KEEP_THREADS) return;
  const int tid = threadIdx.x;
  // ---- pos: the block counts, integer adds (any order gives the same sum)
  if (tid == 0) sum = 0;
  __syncthreads();
  int mine = 0;
  for (int b = tid; b < n_blocks; b += PGS_KEEP_THREADS) mine += block_counts[b];
  if (mine) atomicAdd(&sum, mine);
  __syncthreads();
  const int pos = sum;
  // ---- Python's int(pos * ratio); pos + neg >= E  <=>  pos * ratio >= E - pos (an integer), so no overflow to fear
  const double want = (double)pos * ratio;
  const bool keep_all = pos == 0 || want >= (double)(E - pos);
  const int neg = keep_all ? E - pos : (want > 0.0 ? (int)(long long)want : 0);
  // ---- the neg-th smallest key among the negatives: threshold v, and `rank` of its run of equals still to take
  uint32_t v = 0;
  int rank = keep_all ? 0 : neg;
  if (rank > 0) {   // (the same for every thread: the barriers inside are safe)
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      if (tid == 0) chosen_bin = 0, chosen_rank = 0;
      __syncthreads();
      const uint32_t above = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
      for (int e = tid; e < E; e += PGS_KEEP_THREADS) {
        const uint32_t key = keys[e];
        if (positive[e] == 0 && (key & above) == (v & above)) atomicAdd(&hist[(key >> shift) & 255u], 1);
      }
      __syncthreads();
      if (tid < 256) {
        int before = 0;
        for (int b = 0; b < tid; ++b) before += hist[b];
        if (before < rank && rank <= before + hist[tid]) {   // exactly one bin: rank <= the count of the prefix
          chosen_bin = tid;
          chosen_rank = rank - before;
        }
      }
      __syncthreads();
      v |= (uint32_t)chosen_bin << shift;
      rank = chosen_rank;
      __syncthreads();
    }
  }
  // ---- compaction in ascending replica order
  int equals_before = 0, kept_before = 0;
  for (int first = 0; first < E; first += PGS_KEEP_THREADS) {
    const int e = first + tid;
    bool is_pos = false, is_neg = false;
    uint32_t key = 0;
    if (e < E) {
      is_pos = positive[e] != 0;
      is_neg = !is_pos;
      key = keys[e];
    }
    bool keep = e < E;
    if (!keep_all) {
      const bool equal = is_neg && neg > 0 && key == v;
      int equals_total;
      const int equal_rank = equals_before + pgs_block_rank(equal, slots_a, equals_total);
      equals_before += equals_total;
      keep = is_pos || (is_neg && neg > 0 && (key < v || (equal && equal_rank < rank)));
    }
    int kept_total;
    const int at = kept_before + pgs_block_rank(keep, slots_b, kept_total);
    if (keep && at < E) keep_ids[at] = e;
    kept_before += kept_total;
    __syncthreads();   // (the slots are rewritten by the next chunk)
  }
  if (tid == 0) {
    counts[0] = kept_before;
    counts[1] = pos;
    counts[2] = kept_before - pos;
  }
}

// grid = T * ceil(K / 256) blocks of 256; array a: src_a [T][E][w_a] -> dst_a [T][K][w_a] 32-bit words (a null one is
// skipped)
__global__ void __launch_bounds__(PGS_GATHER_THREADS) HipPgGatherColumns(
    const int *__restrict__ keep_ids, int K, int T, int E, const uint32_t *__restrict__ src0, uint32_t *__restrict__ dst0,
    int w0, const uint32_t *__restrict__ src1, uint32_t *__restrict__ dst1, int w1, const uint32_t *__restrict__ src2,
    uint32_t *__restrict__ dst2, int w2, const uint32_t *__restrict__ src3, uint32_t *__restrict__ dst3, int w3) {
  __shared__ int ids[PGS_GATHER_CHUNK];
  const int chunks = (K + PGS_GATHER_CHUNK - 1) / PGS_GATHER_CHUNK;
  if (K < 1 || K > E || T < 1 || (long)gridDim.x != (long)T * chunks) return;
  const long t = blockIdx.x / chunks, first = (long)(blockIdx.x % chunks) * PGS_GATHER_CHUNK;
  const int count = (int)min((long)PGS_GATHER_CHUNK, (long)K - first);
  if ((int)threadIdx.x < count) ids[threadIdx.x] = keep_ids[first + threadIdx.x];
  __syncthreads();
  pgs_gather_array(src0, dst0, w0, t, E, K, first, count, ids);
  pgs_gather_array(src1, dst1, w1, t, E, K, first, count, ids);
  pgs_gather_array(src2, dst2, w2, t, E, K, first, count, ids);
  pgs_gather_array(src3, dst3, w3, t, E, K, first, count, ids);
}

}  // extern "C"
