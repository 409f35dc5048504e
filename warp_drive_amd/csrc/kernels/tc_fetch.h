// tc_fetch.h -- fetch: every global load of a tick issued up front, probability slabs straight into LDS; the replica-independent tables.
// (The multi-tick entry loads its state through tc_load_state on the trips that need it only, and issues the slabs itself.)
// Part of the TagContinuous translation unit (tag_continuous.hip, which holds the design notes, the probe macros
// and the kernel entries); split by phase in round 6 with every shipped code object byte-identical before / after.
#pragma once
#include "wd_common.h"
#include "tc_types.h"

namespace {

// this wavefront's 64 rows of one head's probability tensor -> LDS (asynchronous: wd_slab_fetch)
__device__ __forceinline__ void tc_fetch_slab(float *slab, const float *probs, const TcArgs &a, int env0, int epb, int N,
                                              int n_actions, int tid) {
  const int rows_here = min(epb, a.E - env0) * N;
  const int r0 = (tid >> 6) * 64, lane = tid & 63;
  const int wrows = max(0, min(64, rows_here - r0));
  wd_slab_fetch(slab + (size_t)r0 * n_actions, probs + ((long)env0 * N + r0) * n_actions, wrows * n_actions, lane);
}

// ---- Multi-tick entry only: the slab issue as straight-line code, for a shape whose sizes are compile-time constants
// (N agents = ONE replica per block of T threads, A-way heads).  tc_fetch_slab above derives the wavefront's row count from
// `tid >> 6` in vector registers, so each slab is compiled as a divergent exec-mask loop of 17 instructions per
// global_load_lds (docs/rounds/r23.md); here the wavefront index is a scalar, the counts below are constants, and a
// wavefront's pieces of a slab are consecutive loads off ONE per-lane global address and ONE LDS base: the instruction's
// immediate offset advances both alike (1 KiB per piece).  The immediate reaches 4095, so every WD_TC_SLAB_REACH pieces take
// a new base pair.  Only the last, partial vector piece and the < 4 trailing floats are exec-masked.  The LDS image is
// wd_slab_fetch's, byte for byte.
constexpr int WD_TC_SLAB_REACH = 4;  // pieces of 64 lanes x 16 bytes that one base pair reaches: 1024 * 3 <= 4095
constexpr int tc_slab_rows(int N, int wave) { return N - 64 * wave >= 64 ? 64 : N - 64 * wave > 0 ? N - 64 * wave : 0; }
constexpr int tc_slab_vecs(int N, int A, int wave) { return tc_slab_rows(N, wave) * A / 4; }       // 16-byte vectors
constexpr int tc_slab_full(int N, int A, int wave) { return tc_slab_vecs(N, A, wave) / 64; }       // unmasked pieces
constexpr int tc_slab_last(int N, int A, int wave) { return tc_slab_vecs(N, A, wave) % 64; }       // lanes of the last piece
constexpr int tc_slab_tail(int N, int A, int wave) { return tc_slab_rows(N, wave) * A % 4; }       // trailing floats

// pieces [C, END) of a wavefront's part of one slab.  s = the part's first byte in memory, vo = 16 * lane, l = the part's
// first byte in LDS (an LDS address, a constant of the kernel)
template <int C, int END>
__device__ __forceinline__ void tc_slab_pieces(const char *s, unsigned vo, unsigned l) {
  if constexpr (C < END) {
    constexpr unsigned B = (C / WD_TC_SLAB_REACH) * WD_TC_SLAB_REACH * 1024u;  // bytes from piece 0 to this piece's base pair
    __builtin_amdgcn_global_load_lds(WD_GLOBAL_PTR(s + (vo + B)), (__attribute__((address_space(3))) void *)(l + B), 16,
                                     1024 * (C % WD_TC_SLAB_REACH), 0);
    tc_slab_pieces<C + 1, END>(s, vo, l);
  }
}

// rows [64 * WAVE, ...) of both heads: pa, pt = the replica's first row in memory; la, lt = the slabs' LDS addresses
template <int N, int A, int WAVE>
__device__ __forceinline__ void tc_fetch_slabs_wave(unsigned la, unsigned lt, const float *pa, const float *pt, int lane) {
  constexpr int NVEC = tc_slab_vecs(N, A, WAVE), FULL = tc_slab_full(N, A, WAVE), LAST = tc_slab_last(N, A, WAVE),
                TAIL = tc_slab_tail(N, A, WAVE);
  constexpr unsigned PART = 4u * 64 * WAVE * A;  // bytes of a slab in front of this wavefront's rows
  const char *const sa = (const char *)pa + PART, *const st = (const char *)pt + PART;
  const unsigned vo = 16u * (unsigned)lane;
  tc_slab_pieces<0, FULL>(sa, vo, la + PART);
  tc_slab_pieces<0, FULL>(st, vo, lt + PART);
  if constexpr (LAST != 0) {
    if (lane < LAST) {
      tc_slab_pieces<FULL, FULL + 1>(sa, vo, la + PART);
      tc_slab_pieces<FULL, FULL + 1>(st, vo, lt + PART);
    }
  }
  if constexpr (TAIL != 0) {  // (one dword per lane: an address of its own, the base pair of the piece it follows)
    constexpr unsigned B = (NVEC / (64 * WD_TC_SLAB_REACH)) * WD_TC_SLAB_REACH * 1024u;
    static_assert(16 * NVEC - B <= 4095, "the trailing floats are within reach of the last base pair");
    if (lane < TAIL) {
      const unsigned v1 = 4u * (unsigned)lane + B;
      __builtin_amdgcn_global_load_lds(WD_GLOBAL_PTR(sa + v1), (__attribute__((address_space(3))) void *)(la + PART + B), 4,
                                       16 * NVEC - B, 0);
      __builtin_amdgcn_global_load_lds(WD_GLOBAL_PTR(st + v1), (__attribute__((address_space(3))) void *)(lt + PART + B), 4,
                                       16 * NVEC - B, 0);
    }
  }
}

// both slabs of the block's replica `env`; `wave` is the wavefront's index in a scalar register (readfirstlane)
template <int N, int A, int T>
__device__ __forceinline__ void tc_fetch_slabs_straight(float *slab_acc, float *slab_turn, const float *probs_acc,
                                                        const float *probs_turn, int env, int wave, int lane) {
  static_assert(N > 64 && N <= 128 && T == 128, "one replica per block of two wavefronts, at most 128 agents");
  static_assert(tc_slab_rows(N, 0) + tc_slab_rows(N, 1) == N, "the two wavefronts' rows are the replica's");
  static_assert(64 * A % 4 == 0, "wavefront 1's rows start on a 16-byte boundary of the slab");
  const float *const pa = probs_acc + (size_t)env * (N * A), *const pt = probs_turn + (size_t)env * (N * A);
  // (an LDS pointer, not the low half of the generic one: that conversion carries a null check per use)
  unsigned la = (unsigned)(size_t)WD_LDS_PTR(slab_acc), lt = (unsigned)(size_t)WD_LDS_PTR(slab_turn);
  // (opaque per trip: the LDS base of every group of pieces, the M0 of its loads, is then an s_add_i32 off these two; seen
  // through, the bases are launch constants that the compiler holds in lanes of a vector register and reads back one by one)
  asm volatile("" : "+s"(la), "+s"(lt));
  if (wave == 0) tc_fetch_slabs_wave<N, A, 0>(la, lt, pa, pt, lane);
  else tc_fetch_slabs_wave<N, A, 1>(la, lt, pa, pt, lane);
}

// Replicas of more than 256 agents sample the two heads one after the other from ONE slab (the second head's rows
// are fetched into the same LDS after the first head was sampled: wave-private rows, no block barrier): both slabs
// of a 1005-agent replica with 21-way heads are 169 KB, and at ~510 agents half the LDS means two blocks per CU.
__device__ __forceinline__ bool tc_one_slab(int N) { return N > 256; }

// FUSED: the launch also restores finished replicas; SAMPLE: it also draws the actions (false: they are read from
// `actions`, e.g. drawn by the policy forward's epilogue -- csrc/kernels/policy_mlp.hip)
template <bool FUSED, bool SAMPLE = FUSED>
__device__ __forceinline__ void tc_issue_loads(TcIn &in, const TcArgs &a, const TcFuse &fz, int env0, int epb,
                                               int N, int n_acc, int n_turn, int tid, float *slab_acc,
                                               float *slab_turn, bool want_cleared = false) {
  const int el = tid / N, ag = tid - el * N;
  const int env = env0 + el;
  const bool active = (el < epb) && (env < a.E);
  const int gi = env * N + ag;
  in.sg = 0; in.type = 0; in.dir = in.acc = in.speed = in.x = in.y = in.skill = 0.f;
  in.sampled = make_int2(0, 0);
  in.epoch = 0u;
  in.step_reward = 0.f;
  in.tstep = in.nrun = 0;
  in.tab_acc = in.tab_turn = 0.f;
  in.cleared = 0;
  if (n_acc <= WD_TC_TAB && n_turn <= WD_TC_TAB) {  // (a block has at least 64 threads)
    if (tid < n_acc) in.tab_acc = a.acc_actions[tid];
    if (tid < n_turn) in.tab_turn = a.turn_actions[tid];
  }
  if (active) {
    in.sg = a.sig_arr[gi];
    in.dir = a.direction[gi];
    in.acc = a.acceleration[gi];
    in.speed = a.speed[gi];
    in.x = a.loc_x[gi];
    in.y = a.loc_y[gi];
    in.skill = a.skill_levels[ag];
    in.type = a.agent_types[ag];
    // (the counters return in order: a load issued after the tick's stores would wait for all of them)
    in.step_reward = a.step_rewards[ag];
    if (want_cleared) in.cleared = a.obs_rows_cleared[gi];
    if (ag == 0) {
      in.tstep = a.timestep[env];
      in.nrun = a.num_runners[env];
    }
    if (!SAMPLE) in.sampled = ((const int2 *)a.actions)[gi];
    if (SAMPLE) in.epoch = fz.rng_state[WD_RNG_HEADER + gi];
  }
  if (SAMPLE) {
    // this wavefront's rows of both probability slabs -> LDS (the second one later when they share the LDS)
    tc_fetch_slab(slab_acc, fz.probs_acc, a, env0, epb, N, n_acc, tid);
    if (!tc_one_slab(N)) tc_fetch_slab(slab_turn, fz.probs_turn, a, env0, epb, N, n_turn, tid);
  }
}

// Multi-tick entry only: the state loads of tc_issue_loads WITHOUT the slabs, for the trips that read their state from
// memory (trip 0 of a launch, the trip after a restore); every other trip carries it in registers (TcCarry).  Ends with
// the wait for all of them, taken once behind the whole block of loads (the opaque asm reads every loaded value, so
// nothing that depends on one -- the `tstep + 1` of the move -- can be pulled up between the loads) and BEFORE the caller
// issues the slabs: the counter returns in order, a state load behind the slabs would wait for them.
__device__ __forceinline__ void tc_load_state(TcIn &in, const TcArgs &a, const TcFuse &fz, int env0, int epb, int N,
                                              int n_acc, int n_turn, int tid, bool want_tables) {
  const int el = tid / N, ag = tid - el * N;
  const int env = env0 + el;
  const bool active = (el < epb) && (env < a.E);
  const int gi = env * N + ag;
  in.sg = 0; in.type = 0; in.dir = in.acc = in.speed = in.x = in.y = in.skill = 0.f;
  in.sampled = make_int2(0, 0);
  in.epoch = 0u;
  in.step_reward = 0.f;
  in.tstep = in.nrun = 0;
  in.tab_acc = in.tab_turn = 0.f;
  in.cleared = 0;
  if (want_tables && n_acc <= WD_TC_TAB && n_turn <= WD_TC_TAB) {
    if (tid < n_acc) in.tab_acc = a.acc_actions[tid];
    if (tid < n_turn) in.tab_turn = a.turn_actions[tid];
  }
  if (active) {
    in.sg = a.sig_arr[gi];
    in.dir = a.direction[gi];
    in.acc = a.acceleration[gi];
    in.speed = a.speed[gi];
    in.x = a.loc_x[gi];
    in.y = a.loc_y[gi];
    in.skill = a.skill_levels[ag];
    in.type = a.agent_types[ag];
    in.step_reward = a.step_rewards[ag];
    in.cleared = a.obs_rows_cleared[gi];
    in.epoch = fz.rng_state[WD_RNG_HEADER + gi];
    if (ag == 0) {
      in.tstep = a.timestep[env];
      in.nrun = a.num_runners[env];
    }
  }
  asm volatile("" : "+v"(in.sg), "+v"(in.dir), "+v"(in.acc), "+v"(in.speed), "+v"(in.x), "+v"(in.y), "+v"(in.skill),
                    "+v"(in.type), "+v"(in.step_reward), "+v"(in.cleared), "+v"(in.epoch), "+v"(in.tstep), "+v"(in.nrun),
                    "+v"(in.tab_acc), "+v"(in.tab_turn));
}

// ---- replica-independent tables: ascending tagger list, action tables.
// Returns the number of taggers.  Ends WITHOUT a barrier: the caller's next barrier publishes them.
__device__ __forceinline__ int tc_build_tables(const TcTables &tb, const TcArgs &a, int N, int n_acc, int n_turn,
                                               bool tab_in_lds, const TcIn &in, int tid_in = threadIdx.x) {
  // (tid_in: the multi-tick entry passes its per-trip opaque copy of the thread index, see tc_reset_finished)
  const int tid = tid_in, T_ = WD_TC_BLOCKDIM;
  const int my_type = in.type;
  if (tab_in_lds) {  // (entries loaded up front, before the probability slabs)
    if (tid < n_acc) tb.acc_tab[tid] = in.tab_acc;
    if (tid < n_turn) tb.turn_tab[tid] = in.tab_turn;
  }
  int n_taggers = 0;
  // rank of a tagger = number of taggers with a smaller id: wave ballots + per-wave counts
  const int wave = tid >> 6, lane = tid & 63, n_waves = (T_ + 63) >> 6;
  if (N <= T_) {  // usual case: one barrier
    // (thread tid < N is agent tid of the block's first replica: its type is among the loads issued up
    // front, BEFORE the probability slabs, so waiting for it does not wait for the slabs)
    const int ty = (tid < N) ? my_type : 0;
    const unsigned long long m = __ballot(ty == 1);
    if (lane == 0) tb.wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0;
    for (int w2 = 0; w2 < n_waves; ++w2) {
      const int c = tb.wave_cnt[w2];
      before += (w2 < wave) ? c : 0;
      n_taggers += c;
    }
    if (ty == 1) tb.tagger_ids[before + __popcll(m & ((1ull << lane) - 1ull))] = tid;
  } else {
    for (int base = 0; base < N; base += T_) {
      const int i = base + tid;
      const int ty = (i < N) ? a.agent_types[i] : 0;
      const unsigned long long m = __ballot(ty == 1);
      if (lane == 0) tb.wave_cnt[wave] = __popcll(m);
      __syncthreads();
      int before = n_taggers;
      for (int w2 = 0; w2 < wave; ++w2) before += tb.wave_cnt[w2];
      if (ty == 1) tb.tagger_ids[before + __popcll(m & ((1ull << lane) - 1ull))] = i;
      for (int w2 = 0; w2 < n_waves; ++w2) n_taggers += tb.wave_cnt[w2];
      __syncthreads();
    }
  }
  return n_taggers;
}

}  // namespace
