// tc_rows.h -- observation rows / neighbour-id rows: LDS staging, write-through flush, LDS carve-up of the fast path, sparse row gather.
// Part of the TagContinuous translation unit (tag_continuous.hip, which holds the design notes, the probe macros
// and the kernel entries); split by phase in round 6 with every shipped code object byte-identical before / after.
#pragma once
#include "wd_common.h"
#include "tc_move.h"

namespace {

// Stream `n` dwords from a wavefront's staging buffer to global memory as one contiguous run.
// The producer placed dword i of the run at stage[mis + i], mis = (address of dst / 4) & 3, so the
// 16-byte vectors of the run are 16-byte aligned in LDS and in memory alike; the <= 3 dwords before
// the first / after the last aligned vector go out as single dwords.
// (tc_flush_run_at: the same with `mis` given by the caller, who advances it from run to run instead of reading it off
// the address: the dense form of the multi-tick entry, tc_gather_rows_dense_lean below)
__device__ __forceinline__ void tc_flush_run_at(const float *stage, float *dst, int mis, int n, int lane) {
  const int head = min(n, (4 - mis) & 3);
  const int nvec = (n - head) >> 2;
  const int tail0 = head + 4 * nvec;
  typedef float v4f __attribute__((ext_vector_type(4)));
  const v4f *sv = (const v4f *)(stage + mis + head);
  v4f *dv = (v4f *)(dst + head);
  // write-through (sc1) 16-byte stores: the rows go to memory as they are produced instead of piling
  // up dirty in the L2 until the kernel-boundary write-back (47.0 -> 45.3 us per tick; 16-byte sc1
  // stores cost the same as plain ones, narrower ones do not).  Three vectors per lane per trip, LDS
  // reads in flight together; whole 64-lane groups are stored under wave-uniform branches, only the
  // last partial group is exec-masked.
#define WD_TC_STORE_WT(ptr, val) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(ptr), "v"(val) : "memory")
  for (int base = 0; base < nvec; base += 192) {
    const int nrem = nvec - base;  // wave-uniform
    const int q = base + lane;
    const v4f v0 = sv[min(q, nvec - 1)], v1 = sv[min(q + 64, nvec - 1)], v2 = sv[min(q + 128, nvec - 1)];
    if (nrem >= 64) WD_TC_STORE_WT(&dv[q], v0);
    else if (lane < nrem) WD_TC_STORE_WT(&dv[q], v0);
    if (nrem >= 128) WD_TC_STORE_WT(&dv[q + 64], v1);
    else if (lane + 64 < nrem) WD_TC_STORE_WT(&dv[q + 64], v1);
    if (nrem >= 192) WD_TC_STORE_WT(&dv[q + 128], v2);
    else if (lane + 128 < nrem) WD_TC_STORE_WT(&dv[q + 128], v2);
  }
#undef WD_TC_STORE_WT
  if (lane < head) dst[lane] = stage[mis + lane];
  if (lane < n - tail0) dst[tail0 + lane] = stage[mis + tail0 + lane];
}
__device__ __forceinline__ void tc_flush_run(const float *stage, float *dst, int n, int lane) {
  tc_flush_run_at(stage, dst, (int)(((size_t)dst >> 2) & 3), n, lane);
}

// nearest_neighbor_ids rows from the block-local 16-bit ids in LDS: n dwords starting at `dst`, dword i =
// id i of the run (0xffff -> -1; block-local -> replica-local when a block holds several replicas);
// aligned 16-byte write-through stores, single dwords before / after the aligned part.
__device__ __forceinline__ void tc_flush_ids(const unsigned short *src, int *dst, int n, int lane, int row0, int N,
                                             float invK, float invN, bool one_replica) {
  const int mis = (int)(((size_t)dst >> 2) & 3);
  const int head = min(n, (4 - mis) & 3);
  const int nvec = (n - head) >> 2;
  const int tail0 = head + 4 * nvec;
  // replica-local id of run element i holding block-local id v (v < 0: none)
  auto local = [&](int v, int i) -> int {
    if (one_replica) return v;
    const int row = row0 + (int)(((float)i + 0.5f) * invK);  // i / K, exact (see the gather)
    const int sub = (int)(((float)row + 0.5f) * invN) * N;
    return v - (v >= 0 ? sub : 0);
  };
  typedef int v4i __attribute__((ext_vector_type(4)));
  for (int q = lane; q < nvec; q += 64) {
    const int i = head + 4 * q;
    const int r0 = (int)(short)src[i], r1 = (int)(short)src[i + 1], r2 = (int)(short)src[i + 2],
              r3 = (int)(short)src[i + 3];
    const v4i v = {local(r0, i), local(r1, i + 1), local(r2, i + 2), local(r3, i + 3)};
    asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst + i), "v"(v) : "memory");
  }
  if (lane < head) dst[lane] = local((int)(short)src[lane], lane);
  if (lane < n - tail0) dst[tail0 + lane] = local((int)(short)src[tail0 + lane], tail0 + lane);
}

// One nearest_neighbor_ids row of K = 10 int32 from a lane's registers (the multi-tick entry: the lane that found the
// ids stores them, tc_fast.h "ids out").  The row is 8-byte aligned (rows are 40 bytes), so it is two 16-byte
// stores (global stores need dword alignment only) and an 8-byte tail.  Plain stores: written through (sc1), the form of
// tc_flush_run, these 40-byte pieces cost more than the whole tc_flush_ids they replace (measured: docs/rounds/r32.md,
// which also has five 8-byte stores, plain -- the compiler merges them into these three -- and written through).
// DWORD_TAIL: the tail as two single dwords -- the form of the rare row of an agent that has just left the game; the loop
// keeps as many single-dword store sites as the one-tick entry, whose tc_flush_ids has two.
template <bool DWORD_TAIL, int NN>
__device__ __forceinline__ void tc_store_id_row(int *replica_rows, unsigned row_bytes, const int (&v)[NN]) {
  static_assert(NN >= 10, "a row of ten ids");
  typedef int v4i __attribute__((ext_vector_type(4)));
  typedef int v2i __attribute__((ext_vector_type(2)));
  typedef v4i __attribute__((aligned(8))) v4i_a8;
  typedef v2i __attribute__((aligned(8))) v2i_a8;
  // (the replica's first row is uniform, the row's place in it a 32-bit byte offset: scalar base + vector offset)
  int *const dst = (int *)((char *)replica_rows + row_bytes);
  const v4i q0 = {v[0], v[1], v[2], v[3]}, q1 = {v[4], v[5], v[6], v[7]};
  *(v4i_a8 *)dst = q0;
  *(v4i_a8 *)(dst + 4) = q1;
  if constexpr (DWORD_TAIL) {
    // (asm: two stores, not one merged pair)
    asm volatile("global_store_dword %0, %1, off offset:32" ::"v"(dst), "v"(v[8]) : "memory");
    asm volatile("global_store_dword %0, %1, off offset:36" ::"v"(dst), "v"(v[9]) : "memory");
  } else {
    const v2i q2 = {v[8], v[9]};
    *(v2i_a8 *)(dst + 8) = q2;
  }
}

// rows of a wavefront's staging buffer: the host sizes the buffer with the same formula
// (envs/tag_continuous.py: lds_bytes_fast)
#define WD_TC_STAGE_TARGET 5400  // bytes of rows per wavefront (19 rows of 71 floats); half of it for blocks of more
                                 // than four wavefronts (replicas of more than 256 agents), whose LDS also holds
                                 // the larger replica
// sparse / dense choice of the multi-tick entry: sparse when at most this many sixteenths of a wavefront's rows are live
#ifndef WD_TC_LOOP_SPARSE_NUM
#define WD_TC_LOOP_SPARSE_NUM 9
#endif
__device__ __forceinline__ int tc_stage_rows(int row_dwords, int n_waves) {
  const int target = (n_waves > 4) ? WD_TC_STAGE_TARGET / 2 : WD_TC_STAGE_TARGET;
  return max(1, min(64, target / (4 * row_dwords)));
}

// LDS of the fast path.  The per-trip area doubles as the two probability slabs of the fused tick,
// which are dead before the move phase writes it.
struct TcFastLds {
  TcFeatArrays feat;     // [A] + [A] observation features, two 16-byte halves per agent
  float2 *xy;            // [epb][NP] positions after the move (x = +BIG for agents out of the game); NP = N rounded up
                         // to a multiple of 4, plus 8 entries of padding that the search's prefetches may read
  int *sig;              // [A] still_in_the_game before this tick's tagging
  int *tagcnt;           // [A] tags credited to a tagger this tick
  float2 *xyc;           // one replica per block: [NP] positions of the agents IN THE GAME, packed in ascending id order
                         // (the candidates and the searchers of the neighbour search); else == xy
  short *cid;            // one replica per block: [1 + N] cid[1 + c] = id of the c-th agent in the game, cid[0] = -1
  unsigned short *ids;   // [A][K] block-local neighbour indices (0xffff = none)
  float *stage;          // [n_waves][stage_dwords] wave-private staging buffers
  int stage_dwords;
  TcTables tb;
};

__device__ __forceinline__ TcFastLds tc_carve_fast(unsigned char *p0, int epb, int N, int K, int n_waves,
                                                   size_t min_area_bytes, bool compact) {
  TcFastLds l;
  const size_t A = (size_t)epb * N;
  const int F = 7 * K + 1;
  size_t off = 0;
  l.feat.a = (TcFeatA *)(p0 + off); off += sizeof(TcFeatA) * A;
  l.feat.b = (TcFeatB *)(p0 + off); off += sizeof(TcFeatB) * A;
  l.xy = (float2 *)(p0 + off); off += 8 * (size_t)epb * (((N + 3) & ~3) + 8);  // see TcFastLds::xy
  l.sig = (int *)(p0 + off); off += 4 * A;
  l.tagcnt = (int *)(p0 + off); off += 4 * A;
  l.xyc = l.xy;
  l.cid = nullptr;
  if (compact) {  // (the host adds the same bytes: envs/tag_continuous.py lds_bytes)
    off = tc_align16(off);
    l.xyc = (float2 *)(p0 + off); off += 8 * (size_t)(((N + 3) & ~3) + 8);
    l.cid = (short *)(p0 + off); off += tc_align16(2 * ((size_t)N + 1));
  }
  l.ids = (unsigned short *)(p0 + off); off = tc_align16(off + 2 * A * K);
  l.stage_dwords = (int)(tc_align16((size_t)4 * tc_stage_rows(F, n_waves) * F) / 4) + 4 + 16;  // + the list of live rows (64 bytes)
  // replicas of more than 128 agents: the buffer also holds the prefiltered search's hints (8 dwords per lane) and, after
  // them, its candidate lists (tc_knn.h WD_TC_LIST_DWORDS = 1152; the host adds the same, envs/tag_continuous.py lds_bytes)
  if (compact && N > 128) l.stage_dwords = max(l.stage_dwords, 1152);
  l.stage = (float *)(p0 + off); off += (size_t)4 * l.stage_dwords * n_waves;
  off = tc_align16(off > min_area_bytes ? off : min_area_bytes);
  l.tb = tc_carve_tables(p0 + off, epb, N);
  return l;
}

// ---- observation rows of one wavefront, SPARSE form (chosen per wavefront when at most 9/16 of its rows
// belong to agents in the game: late in an episode; the dense form -- contiguous chunks of rows, every row
// computed and written -- is cheaper per row but moves every byte): rows [wrow0, wrow0 + wrows) of the block.
// A row of an agent that is out of the game is all zeros until the episode restarts (:476-560): it is
// cleared ONCE, on the first tick the agent is out (bit 1 of l.sig / obs_rows_cleared remember it), and
// costs nothing afterwards -- under the benchmark's own policy half of the rows, on average over an
// episode.  Rows of agents IN the game are built in the wavefront's private LDS staging buffer, `rs`
// rows at a time in packed order (the wavefront's list of live rows maps the packed ordinal to the
// row): work item = (live row, neighbour slot) -> 7 values at c*K + k of the row image; then the time
// column; then every row image leaves as 16-byte write-through stores.
//   A row image starts `mis` dwords into its slot, mis = (row address / 4) & 3, so that its 16-byte
// vectors are aligned in LDS and in memory alike (rows are 4 * F bytes, F odd: the alignment changes
// from row to row); the slot's pads are zeroed.  The <= 3 dwords at either end of a row share a
// 16-byte line with the neighbouring row:
//   * neighbour out of the game: its row is (or is being) cleared, so the whole line is stored with
//     zeros in the neighbour's part;
//   * neighbour in the game and built in the same chunk (the next slot): the lower row stores the line,
//     merged (OR) with the first vector of the next slot; the upper row skips its first vector;
//   * neighbour unknown (other wavefront / other block) or in another chunk: single dwords, own part only.
// The flush below decides all of this per round and per lane; the multi-tick entry (LOOP) decides it once per row and
// flushes from descriptors (TcLeanRows, further down): same rules, same bytes, a third of the instructions.
__device__ __forceinline__ void tc_store_own_dwords(float *rowp, int F, int d0, const float (&v)[4], bool on) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (on && d0 + e >= 0 && d0 + e < F) rowp[d0 + e] = v[e];
}

// ---- the LOOP variant (the multi-tick entry, one shape: K = 10) builds and stores the same row images from the same
// two forms, but its flush works from one DESCRIPTOR word per packed row, formed once per chunk by lane j for slot j and
// fetched in the flush round by lane (fsub, fv) with one ds_bpermute_b32 -- what depends on the row alone (the row list
// read, mis, the shifts against lmask, the head / tail rules, the address) is not redone per round and per lane:
//   bits  0.. 1  action of vector 0: the row's head (head mode: skip / own dwords / full line; no head when mis = 0: full)
//   bits  2.. 3  action of vector NV - 2: the row's tail when mis = 0, else a full line
//   bits  4.. 5  action of vector NV - 1: the row's tail when mis >= 2, else nothing (it lies past the row)
//                (tail mode: merge with the next slot's first vector / own dwords / full line; no tail when mis = 1)
//   bits  6.. 7  action of every other vector: a full line
//   bits  8.. 9  mis
//   bits 10..11  zero: what the lanes beyond the round's RPR * NV read
//   bits 16..31  4 * (r * F - mis + 3): byte offset of the slot's first vector from the wavefront's first row, + 12
// actions: 0 nothing, 1 own dwords only, 2 the whole 16-byte line, 3 the whole line OR-merged with the next slot's first
// vector.  Lanes at or past the chunk's row count hold 0: nothing is stored for them.
template <int KC>
struct TcLeanRows {
  static constexpr int F = 7 * KC + 1, SL = (F + 6) & ~3, NV = SL >> 2, RPR = 64 / NV;
  // the wavefront's staging buffer (tc_carve_fast, blocks of at most four wavefronts) and the rows per chunk it gives
  static constexpr int STAGE_DWORDS = (((4 * (WD_TC_STAGE_TARGET / (4 * F)) * F) + 15) & ~15) / 4 + 4 + 16;
  static constexpr int CAP = STAGE_DWORDS - 16;
  static constexpr int RS = (CAP / SL < 192 / KC) ? (CAP / SL < 64 ? CAP / SL : 64) : (192 / KC < 64 ? 192 / KC : 64);
  static constexpr int ACT_NONE = 0, ACT_OWN = 1, ACT_FULL = 2, ACT_MERGE = 3;
  // the flush reads slots up to RS (one past the chunk: the merge operand of the last slot, never used) without clamping
  static_assert((RS + 1) * SL + 4 <= STAGE_DWORDS, "the unclamped LDS reads of the flush stay inside the staging buffer");
  static_assert(((RS - 1) / (3 * RPR)) * 3 * RPR + 3 * RPR - 1 <= RS, "highest slot a trip of three rounds reads");
  // the row's end lies in vector NV - 2 (mis = 0), nowhere short of a line end (mis = 1) or in vector NV - 1 (mis >= 2)
  static_assert(4 * (NV - 2) < F && 4 * (NV - 2) + 4 > F && 4 * (NV - 1) - 1 == F, "tail positions of the descriptor");
  static_assert(4 * (52 * F + 3) < 65536 && NV >= 4 && RPR * NV <= 64, "descriptor fields");
};

// the own-dword store sites of the LOOP flush: p = address of the vector's first dword, d0 its row-relative index
__device__ __forceinline__ void tc_store_own_dwords_at(float *p, int F, int d0, const float (&v)[4], bool on) {
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (on && d0 + e >= 0 && d0 + e < F) p[e] = v[e];
}

template <bool LOOP = false, int KC = 0>
__device__ __forceinline__ void tc_gather_rows_sparse(const TcArgs &a, const TcFastLds &l, const TcTables &tb, float *stage,
                                               int env0, int wrow0, int wrows, int lane, int K_, int N, float invK,
                                               float invN) {
  typedef float v4f __attribute__((ext_vector_type(4)));
  const int K = LOOP ? KC : K_;
  const int F = 7 * K + 1;
  const int SL = (F + 6) & ~3;       // dwords per row slot (mis + F <= SL)
  const int NV = SL >> 2;            // 16-byte vectors per slot
  const int cap = l.stage_dwords - 16;
  // rows per chunk (at most 3 items per lane); LOOP: the value the formula gives for the shape, as a constant
  int rs = min(min(64, cap / SL), 192 / K);
  if constexpr (LOOP) rs = TcLeanRows<KC>::RS;
  const int RPR = 64 / NV;           // rows per flush round (NV <= 58 for K <= 32)
  const float invNV = 1.0f / (float)NV;
  constexpr int U = 3;
  int rr[U], kk[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int t = lane + 64 * u;
    rr[u] = (int)(((float)t + 0.5f) * invK);  // t / K (exact: the quotient is >= 0.5/K away from an integer)
    kk[u] = t - rr[u] * K;
  }
  const int fsub = (int)(((float)lane + 0.5f) * invNV), fv = lane - fsub * NV;  // flush: (row of the round, vector)
  const int sgv = (lane < wrows) ? l.sig[wrow0 + lane] : 2;
  const unsigned long long lmask = __ballot((sgv & 1) != 0);  // rows to build (a wavefront gathers at most 64 rows)
  unsigned long long zmask = __ballot(sgv == 0);              // rows to clear: out of the game, not cleared yet
  unsigned char *const rowlist = (unsigned char *)(stage + cap);
  if (sgv & 1) rowlist[__popcll(lmask & ((1ull << lane) - 1ull))] = (unsigned char)lane;
  float *const obs_w = a.obs + ((long)env0 * N + wrow0) * F;
  const unsigned bdw = (unsigned)((size_t)obs_w >> 2);
  const unsigned short *const idw = l.ids + (size_t)wrow0 * K;
  const int n_rows = __popcll(lmask);
  // ---- rows of agents that left the game since the last tick: zeros, straight from registers
  while (zmask) {  // wave-uniform, rare
    const int r = __ffsll((long long)zmask) - 1;
    zmask &= zmask - 1ull;
    float *const rowp = obs_w + (long)r * F;
    const int mis = (int)((bdw + (unsigned)(r * F)) & 3u);
    const int d0 = 4 * lane - mis;
    const float z[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (lane < NV) {
      if (d0 >= 0 && d0 + 4 <= F) {
        const v4f q = {0.0f, 0.0f, 0.0f, 0.0f};
        asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(rowp + d0), "v"(q) : "memory");
      } else {
        tc_store_own_dwords(rowp, F, d0, z, true);
      }
    }
  }
  // LOOP: what depends on the lane alone (the flush's place in a round) is formed in front of the chunks
  [[maybe_unused]] int fs = 0;
  [[maybe_unused]] unsigned sh = 0u;
  if constexpr (LOOP) {
    typedef TcLeanRows<KC> D;
    const bool idle = (fsub >= D::RPR);  // the lanes past RPR * NV: they read slot 0's neighbours and a zero field
    fs = idle ? 0 : fsub;
    sh = idle ? 10u : (fv == 0) ? 0u : (fv == D::NV - 2) ? 2u : (fv == D::NV - 1) ? 4u : 6u;
  }
  // ---- rows of agents in the game
  for (int j0 = 0; j0 < n_rows; j0 += rs) {
    const int rc = min(rs, n_rows - j0);
    const int items = rc * K;
    if (lane < rc) {  // zero the pads of the slot (first vector, last two vectors)
      const v4f zero = {0.0f, 0.0f, 0.0f, 0.0f};
      v4f *const sl = (v4f *)(stage + lane * SL);
      sl[0] = zero;
      sl[NV - 2] = zero;
      sl[NV - 1] = zero;
    }
    [[maybe_unused]] unsigned desc = 0u;  // LOOP: the descriptor of slot `lane` (see TcLeanRows)
    if constexpr (LOOP) {
      typedef TcLeanRows<KC> D;
      // What depends on the row alone is formed once per chunk, by lane j for packed slot j: the row list entry, mis, the
      // time column (one replica per block: the replica of the row is 0, so tfrac[0] at a uniform address; read here, per
      // chunk -- held in a register from the top of the function it upsets the allocation of the search, which grows by
      // 80 instructions: docs/rounds/r35.md) and the descriptor.  The item lanes fetch (row | 4 * mis << 8) of their slot
      // with one ds_bpermute_b32 per item, issued with every lane active (a disabled source lane reads as 0).
      unsigned rw = 0u;
      if (lane < rc) {
        const int r = rowlist[j0 + lane];
        const int mis = (int)((bdw + (unsigned)(r * F)) & 3u);
        stage[lane * SL + mis + 7 * K] = tb.tfrac[0];  // float(t) / episode_length (agents in the game, :474,:493,:543)
        rw = (unsigned)r | ((unsigned)mis << 10);
        // the neighbouring rows: in the game?  known at all (inside this wavefront's rows)?  The packed order is the
        // row order, so a live neighbour is the previous / next slot unless the chunk ends in between.
        const bool prev_known = (r > 0), next_known = (r + 1 < wrows);
        const bool prev_live = (((lmask << 1) >> r) & 1ull) != 0ull, next_live = (((lmask >> 1) >> r) & 1ull) != 0ull;
        const unsigned head = (mis == 0)                   ? D::ACT_FULL   // no head: vector 0 is the row's own
                              : (prev_live && lane > 0)    ? D::ACT_NONE   // stored by the row below, merged
                              : (prev_live || !prev_known) ? D::ACT_OWN
                                                           : D::ACT_FULL;  // the row below is (being) cleared
        const unsigned tail = (next_live && lane + 1 < rc) ? D::ACT_MERGE
                              : (next_live || !next_known) ? D::ACT_OWN
                                                           : D::ACT_FULL;
        const unsigned a_nv2 = (mis == 0) ? tail : (unsigned)D::ACT_FULL, a_nv1 = (mis >= 2) ? tail : (unsigned)D::ACT_NONE;
        desc = head | (a_nv2 << 2) | (a_nv1 << 4) | ((unsigned)D::ACT_FULL << 6) | ((unsigned)mis << 8) |
               ((unsigned)(4 * (r * F - mis + 3)) << 16);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (64 * u < items) {  // wave-uniform
          const unsigned w = (unsigned)__builtin_amdgcn_ds_bpermute(4 * rr[u], (int)rw);
          if (lane + 64 * u < items) {
            const int r = (int)(w & 0xffu);  // row of the item inside the wavefront's rows
            const unsigned jq = idw[r * K + kk[u]];
            const TcFeat me = tc_feat_load(l.feat, wrow0 + r);
            // no neighbour in this slot: the agent's own record stands in, so every difference
            // below is +0.0 without a select
            const bool valid = (jq != 0xffffu);
            const TcFeat nb = tc_feat_load(l.feat, valid ? (int)jq : wrow0 + r);
            unsigned mv = valid ? 0xffffffffu : 0u;
            asm volatile("" : "+v"(mv));  // (opaque: keeps the AND below from being turned into selects)
            const unsigned ts = (unsigned)nb.type_sig & mv;
            float *o = (float *)((char *)(stage + rr[u] * SL + kk[u]) + (w >> 8));  // (+ mis dwords)
            o[0] = (float)(nb.nx - me.nx);   // float64 difference, narrowed (:560)
            o[K] = (float)(nb.ny - me.ny);
            o[2 * K] = nb.nsp - me.nsp;      // float32 operands: the float64 difference rounds to this
            o[3 * K] = nb.nac - me.nac;
            o[4 * K] = nb.ndir - me.ndir;
            o[5 * K] = __uint_as_float(ts & 0x3f800000u);
            o[6 * K] = __uint_as_float((0u - (ts & 1u)) & 0x3f800000u);
          }
        }
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (64 * u < items) {  // wave-uniform
          if (lane + 64 * u < items) {
            const int r = rowlist[j0 + rr[u]];  // row of the item inside the wavefront's rows
            const unsigned jq = idw[r * K + kk[u]];
            const TcFeat me = tc_feat_load(l.feat, wrow0 + r);
            // no neighbour in this slot: the agent's own record stands in, so every difference
            // below is +0.0 without a select
            const bool valid = (jq != 0xffffu);
            const TcFeat nb = tc_feat_load(l.feat, valid ? (int)jq : wrow0 + r);
            unsigned mv = valid ? 0xffffffffu : 0u;
            asm volatile("" : "+v"(mv));  // (opaque: keeps the AND below from being turned into selects)
            const unsigned ts = (unsigned)nb.type_sig & mv;
            const int mis = (int)((bdw + (unsigned)(r * F)) & 3u);
            float *o = stage + rr[u] * SL + mis + kk[u];
            o[0] = (float)(nb.nx - me.nx);   // float64 difference, narrowed (:560)
            o[K] = (float)(nb.ny - me.ny);
            o[2 * K] = nb.nsp - me.nsp;      // float32 operands: the float64 difference rounds to this
            o[3 * K] = nb.nac - me.nac;
            o[4 * K] = nb.ndir - me.ndir;
            o[5 * K] = __uint_as_float(ts & 0x3f800000u);
            o[6 * K] = __uint_as_float((0u - (ts & 1u)) & 0x3f800000u);
          }
        }
      }
      if (lane < rc) {
        // time column: float(t) / episode_length (agents in the game, :474,:493,:543)
        const int r = rowlist[j0 + lane];
        const int e_m = (int)(((float)(wrow0 + r) + 0.5f) * invN);
        const int mis = (int)((bdw + (unsigned)(r * F)) & 3u);
        stage[lane * SL + mis + 7 * K] = tb.tfrac[e_m];
      }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    if constexpr (LOOP) {
      // ---- flush from the descriptors: three rounds of RPR rows per trip, as below; per round and lane one
      // bpermute, the action and the byte offset out of the word, the two LDS vectors, the OR-merge, one store
      typedef TcLeanRows<KC> D;
      static_assert(D::RPR == 3 && D::NV == 19 && D::F == 71 && D::SL == 76 && D::RS == 17, "built for K = 10");
      constexpr int W = 3;
      for (int sb = 0; sb < rc; sb += W * D::RPR) {
        unsigned dd[W];
        v4f q[W], nx[W];
#pragma unroll
        for (int u = 0; u < W; ++u)
          dd[u] = (unsigned)__builtin_amdgcn_ds_bpermute(4 * (sb + u * D::RPR + fs), (int)desc);
#pragma unroll
        for (int u = 0; u < W; ++u) {
          q[u] = *(const v4f *)(stage + (sb + u * D::RPR + fs) * D::SL + 4 * fv);
          nx[u] = *(const v4f *)(stage + (sb + u * D::RPR + fs + 1) * D::SL);  // first vector of the next slot (merge)
        }
#pragma unroll
        for (int u = 0; u < W; ++u) {
          if (sb + u * D::RPR < rc) {  // wave-uniform
            const unsigned act = (dd[u] >> sh) & 3u;
            const unsigned voff = (dd[u] >> 16) + 16u * (unsigned)fv;  // byte offset of the vector from obs_w, + 12
            unsigned mm = (act == (unsigned)D::ACT_MERGE) ? 0xffffffffu : 0u;
            asm volatile("" : "+v"(mm));  // (AND mask, not four selects)
            v4f o = q[u];
            o.x = __uint_as_float(__float_as_uint(o.x) | (__float_as_uint(nx[u].x) & mm));
            o.y = __uint_as_float(__float_as_uint(o.y) | (__float_as_uint(nx[u].y) & mm));
            o.z = __uint_as_float(__float_as_uint(o.z) | (__float_as_uint(nx[u].z) & mm));
            o.w = __uint_as_float(__float_as_uint(o.w) | (__float_as_uint(nx[u].w) & mm));
            if (act >= (unsigned)D::ACT_FULL)
              asm volatile("global_store_dwordx4 %0, %1, %2 offset:-12 sc1" ::"v"(voff), "v"(o), "s"(obs_w) : "memory");
            if (__ballot(act == (unsigned)D::ACT_OWN) != 0ull) {  // wave-uniform: a row at the edge of the wavefront's rows or of the chunk
              const float vals[4] = {o.x, o.y, o.z, o.w};
              const int d0 = 4 * fv - (int)((dd[u] >> 8) & 3u);
              tc_store_own_dwords_at((float *)((char *)obs_w + voff) - 3, F, d0, vals, act == (unsigned)D::ACT_OWN);
            }
          }
        }
      }
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      continue;
    }
    // ---- flush: RPR rows per round, lane = (row of the round, 16-byte vector of its slot); three rounds
    // per trip so that three independent chains of LDS reads are in flight
    for (int sb = 0; sb < rc; sb += 3 * RPR) {
      constexpr int W = 3;
      int slot[W], r[W], d0[W];
      bool on[W];
#pragma unroll
      for (int u = 0; u < W; ++u) {
        slot[u] = sb + u * RPR + fsub;
        on[u] = (fsub < RPR) && (slot[u] < rc);
        slot[u] = min(slot[u], rc - 1);
        r[u] = rowlist[j0 + slot[u]];
      }
      v4f q[W], nx[W];
#pragma unroll
      for (int u = 0; u < W; ++u) {
        const int mis = (int)((bdw + (unsigned)(r[u] * F)) & 3u);
        d0[u] = 4 * fv - mis;  // row-relative index of the vector's first dword
        q[u] = *(const v4f *)(stage + slot[u] * SL + 4 * fv);
        nx[u] = *(const v4f *)(stage + min(slot[u] + 1, rc - 1) * SL);  // first vector of the next slot (merge)
      }
#pragma unroll
      for (int u = 0; u < W; ++u) {
        if (sb + u * RPR < rc) {  // wave-uniform
          float *const rowp = obs_w + (long)r[u] * F;
          const bool head_part = on[u] && (d0[u] < 0), tail_part = on[u] && (d0[u] < F) && (d0[u] + 4 > F);
          // the neighbouring rows: in the game?  known at all (inside this wavefront's rows)?
          const bool prev_known = (r[u] > 0), next_known = (r[u] + 1 < wrows);
          const bool prev_live = prev_known && ((lmask >> (r[u] - 1)) & 1ull);
          const bool next_live = next_known && ((lmask >> (r[u] + 1)) & 1ull);
          const bool merge_next = tail_part && next_live && (slot[u] + 1 < rc);
          unsigned mm = merge_next ? 0xffffffffu : 0u;
          asm volatile("" : "+v"(mm));  // (AND mask, not four selects)
          v4f o = q[u];
          o.x = __uint_as_float(__float_as_uint(o.x) | (__float_as_uint(nx[u].x) & mm));
          o.y = __uint_as_float(__float_as_uint(o.y) | (__float_as_uint(nx[u].y) & mm));
          o.z = __uint_as_float(__float_as_uint(o.z) | (__float_as_uint(nx[u].z) & mm));
          o.w = __uint_as_float(__float_as_uint(o.w) | (__float_as_uint(nx[u].w) & mm));
          const bool skip = head_part && prev_live && (slot[u] > 0);            // stored by the row below
          const bool own_only = (head_part && !skip && (prev_live || !prev_known)) ||
                                (tail_part && !merge_next && (next_live || !next_known));
          const bool full = on[u] && (d0[u] < F) && !skip && !own_only;
          if (full) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(rowp + d0[u]), "v"(o) : "memory");
          if (__ballot(own_only) != 0ull) {  // wave-uniform: a row at the edge of the wavefront's rows or of the chunk
            const float vals[4] = {o.x, o.y, o.z, o.w};
            tc_store_own_dwords(rowp, F, d0[u], vals, own_only);
          }
        }
      }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
}

// ---- observation rows of one wavefront, DENSE form, as the multi-tick entry builds them (one shape: SN agents in two
// wavefronts, one replica per block).  The same items, the same staging image and the same flush (tc_flush_run) as the
// chunk loop of tc_fast.h, which the one-tick entries keep; what the shape fixes is not worked out per chunk:
//   * the chunk plan: NCH chunks of R rows, the last one of LAST0 / LAST1 rows.  Every chunk has more than 128 items, so
//     the first two items of a lane always exist; only the third can lie past the end (lanes 62 and 63 of a full chunk,
//     more lanes of the last one).  Such a lane computes its second item twice -- the same values to the same place, as
//     the generic loop recomputes the chunk's last item -- chosen by one compare per chunk; no item index is clamped and
//     no (row, offset) split is redone.
//   * whether the row's own agent is in the game: bit r of `live`, the vote over l.sig the caller has just taken, instead
//     of bit 0 of the own record's type_sig.  Both are written from the same register on the same trip (tc_fast.h:
//     m.ft.type_sig and l.sig[li] take `sg`), so the neighbour's address no longer waits for the own record, and there is
//     no branch around the neighbour reads: a row out of the game takes the "own record stands in" select, every
//     difference is +0.0 and the type bits are masked, as before.
//   * the time column: one replica per block, so the row's replica is 0 and tfrac[0] is read once; the live test per row
//     is the same bit of `live`.
//   * dst, mis, the id row and the first record advance by constants from chunk to chunk.
template <int KC, int SN>
struct TcLeanDense {
  static constexpr int F = 7 * KC + 1;
  static constexpr int R = WD_TC_STAGE_TARGET / (4 * F);           // tc_stage_rows: blocks of at most four wavefronts
  static constexpr int ROWS0 = (SN + 1) / 2, ROWS1 = SN - ROWS0;   // the even split of tc_fast.h
  static constexpr int NCH = (ROWS0 + R - 1) / R;
  static constexpr int LAST0 = ROWS0 - (NCH - 1) * R, LAST1 = ROWS1 - (NCH - 1) * R;
  static_assert(R >= 1 && R <= 32 && R * KC <= 192 && R * KC > 128, "at most three items per lane; bit tests on 32 bits");
  static_assert((ROWS1 + R - 1) / R == NCH && LAST1 >= 1 && LAST1 <= LAST0 && LAST0 <= R, "both wavefronts: NCH chunks");
  static_assert(LAST1 * KC > 128, "the first two items of a lane exist in every chunk");
  static_assert(4 * R * F + 12 <= WD_TC_STAGE_TARGET + 16, "a chunk image at any alignment fits the staging buffer");
};

template <int KC, int SN>
__device__ __forceinline__ void tc_gather_rows_dense_lean(const TcArgs &a, const TcFastLds &l, const TcTables &tb,
                                                          float *stage, int env0, int wave, int lane,
                                                          unsigned long long live) {
  typedef TcLeanDense<KC, SN> D;
  constexpr int K = KC, F = D::F, R = D::R, U = 3;
  const int wrow0 = wave * D::ROWS0;
  const int last_rows = wave ? D::LAST1 : D::LAST0;  // wave-uniform
  int t0[U], r0[U], s0[U];  // item, its row in the chunk, offset of its first value in the chunk image
#pragma unroll
  for (int u = 0; u < U; ++u) {
    t0[u] = lane + 64 * u;
    r0[u] = (int)((unsigned)t0[u] / (unsigned)K);
    s0[u] = r0[u] * F + (t0[u] - r0[u] * K);
  }
  float *dst = a.obs + ((long)env0 * SN + wrow0) * F;
  int mis = (int)(((size_t)dst >> 2) & 3);
  const unsigned short *idp = l.ids + wrow0 * K;  // ids of item t: idp[t]
  int fp = wrow0;
  const float tfrac = tb.tfrac[0];
#pragma nounroll
  for (int c = 0; c < D::NCH; ++c) {
    const int rc = (c == D::NCH - 1) ? last_rows : R;
    // a lane whose third item lies past the end of the chunk computes its second item twice
    const bool past = lane + 128 >= rc * K;
    const int tt[U] = {t0[0], t0[1], past ? t0[1] : t0[2]}, rr[U] = {r0[0], r0[1], past ? r0[1] : r0[2]},
              so[U] = {s0[0], s0[1], past ? s0[1] : s0[2]};
    const unsigned lv = (unsigned)live;  // bit r: row r of the chunk belongs to an agent in the game
    // the three ids first; then one item after the other, its two records in flight together.  (All six records of a
    // lane in flight at once, as the source of tc_fast.h asks for, is what the compiler did NOT build there -- its
    // branch on the own record serialised them -- and costs 45 registers here: the object then needs 128 VGPRs and the
    // search, allocated around that peak, grows by 66 instructions.  Read off the object; docs/rounds/r35.md.)
    unsigned jq[U];
#pragma unroll
    for (int u = 0; u < U; ++u) jq[u] = idp[tt[u]];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int m = fp + rr[u];
      const TcFeat me = tc_feat_load(l.feat, m);
      // no neighbour (or the agent is out of the game): its own record stands in, so every
      // difference below is +0.0 without a select
      const bool valid = (((lv >> rr[u]) & 1u) != 0u) && (jq[u] != 0xffffu);
      const TcFeat nb = tc_feat_load(l.feat, valid ? (int)jq[u] : m);
      unsigned mv = valid ? 0xffffffffu : 0u;
      asm volatile("" : "+v"(mv));  // (opaque: keeps the AND below from being turned into selects)
      const unsigned ts = (unsigned)nb.type_sig & mv;
      float *o = stage + mis + so[u];
      o[0] = (float)(nb.nx - me.nx);   // float64 difference, narrowed (:560)
      o[K] = (float)(nb.ny - me.ny);
      o[2 * K] = nb.nsp - me.nsp;      // float32 operands: the float64 difference rounds to this
      o[3 * K] = nb.nac - me.nac;
      o[4 * K] = nb.ndir - me.ndir;
      o[5 * K] = __uint_as_float(ts & 0x3f800000u);
      o[6 * K] = __uint_as_float((0u - (ts & 1u)) & 0x3f800000u);
    }
    // time column: float(t) / episode_length for agents in the game, else 0 (:474,:493,:543)
    if (lane < rc) stage[mis + lane * F + 7 * K] = ((lv >> lane) & 1u) ? tfrac : 0.0f;
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    tc_flush_run_at(stage, dst, mis, rc * F, lane);
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    dst += R * F;
    mis = (mis + R * F) & 3;
    idp += R * K;
    fp += R;
    live >>= R;
  }
}

}  // namespace
