// tc_fast.h -- tc_fast_impl: one tick of whole replicas per block (N <= 1024, partial observations, K <= KMAX).
// Part of the TagContinuous translation unit (tag_continuous.hip, which holds the design notes, the probe macros
// and the kernel entries); split by phase in round 6 with every shipped code object byte-identical before / after.
#pragma once
#include "wd_common.h"
#include "tc_kernarg.h"
#include "tc_fetch.h"
#include "tc_sample.h"
#include "tc_move.h"
#include "tc_tags.h"
#include "tc_reset.h"
#include "tc_knn.h"
#include "tc_rows.h"

namespace {

// What the multi-tick entry keeps out of memory until a CLOSING trip (the last of a launch, or the one a replica's episode
// ends on): position, speed, heading, acceleration, the edge penalty, the RNG epoch word; from lane 0 the time step and the
// runner count.  `s` is the thread's carry AFTER the move (TcCarry::in), `epoch` the word the next trip starts from.
// One replica per block (`env0`, SN agents): every array is addressed off the replica's row on the scalar side, and the
// agent's place in it is ONE 32-bit byte offset shared by all seven (the form of tc_store_id_row, tc_rows.h).
template <int SN>
__device__ __forceinline__ void tc_store_carried(const TcArgs &a, const TcFuse &fz, const TcIn &s, float edge_pen,
                                                 uint32_t epoch, int env0, int ag, int nrun) {
  const long row0 = (long)env0 * SN;
  const unsigned off = 4u * (unsigned)ag;
  *(float *)((char *)(a.loc_x + row0) + off) = s.x;
  *(float *)((char *)(a.loc_y + row0) + off) = s.y;
  *(float *)((char *)(a.speed + row0) + off) = s.speed;
  *(float *)((char *)(a.direction + row0) + off) = s.dir;
  *(float *)((char *)(a.acceleration + row0) + off) = s.acc;
  *(float *)((char *)(a.edge_pen_arr + row0) + off) = edge_pen;
  *(uint32_t *)((char *)(fz.rng_state + WD_RNG_HEADER + row0) + off) = epoch;
  if (ag == 0) {
    a.timestep[env0] = s.tstep;
    a.num_runners[env0] = nrun;
  }
}

// EXACTK: K == KMAX, known at compile time (row offsets become immediates, the K-dependent selects fold away)
// LOOP: called as the body of the multi-tick entry (tc_fast_rollout below) for trip `tick` of a launch; the replica-independent tables
// are built on trip 0 and stay (`n_taggers` carries their length); the thread's own state arrives in `cy` and leaves in it
// (TcCarry: read from memory on the trips `cy->reload` names only); the probes stamp the one trip the harness chose
// SN, SA, ST (LOOP only): the shape's agents, head size and block size as constants, for the straight-line slab issue
template <int KMAX, bool FUSED, bool EXACTK, int IDB, bool SAMPLE = FUSED, bool LOOP = false, int SN = 0, int SA = 0,
          int ST = 0>
__device__ __forceinline__ int tc_fast_impl(const TcArgs &a, const TcFuse &fz, unsigned char *smem, int n_acc,
                                            int n_turn, int tick = 0, int n_taggers_in = 0, TcCarry *cy = nullptr,
                                            const TcLoopConsts *lc = nullptr) {
  WD_TC_PROBE_TICK(LOOP, tick);
  const int N = a.N, K = EXACTK ? KMAX : a.K;
  const int F = 7 * K + 1;
  int tid_ = threadIdx.x;
  // (a value the compiler cannot see through, per trip: without it every address that depends on the thread alone -- two
  // registers per array -- is computed once and held across the loop, far beyond the register budget)
  if constexpr (LOOP) asm volatile("" : "+v"(tid_));
  const int tid = tid_, T_ = WD_TC_BLOCKDIM;
  const int epb = max(1, T_ / N);
  // (readfirstlane: the wavefront index is uniform, but only the hardware knows -- without it every loop whose
  // bounds depend on it is compiled as a divergent loop)
  const int n_waves = (T_ + 63) >> 6, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const size_t slab_acc_bytes = tc_align16((size_t)4 * epb * N * n_acc);
  // One replica per block (more than 64 agents: the BASELINE shape): the neighbour search runs over
  // the agents that are still IN THE GAME only, packed in ascending id order -- as candidates (the
  // chain is as long as the live list, not N) and as searchers (searcher lane c works for the c-th
  // live agent, so a wavefront whose lanes are all >= the live count skips the search).  Under the
  // reference's own benchmark policy (uniform random actions) 54 of 105 agents are in the game on
  // average over a 500-tick episode (105 at the start, ~27 at the end).  Packing preserves the id
  // order, so ties break exactly as before; ids are translated back through `cid`.
  const bool compact = (epb == 1);
  const size_t slab_turn_bytes = tc_align16((size_t)4 * epb * N * n_turn);
  const bool one_slab = tc_one_slab(N);
  const TcFastLds l = tc_carve_fast(smem, epb, N, K, n_waves,
                                    !SAMPLE ? 0 : one_slab ? max(slab_acc_bytes, slab_turn_bytes) : slab_acc_bytes + slab_turn_bytes,
                                    compact);
  const TcTables &tb = l.tb;
  float *const slab_acc = (float *)smem, *const slab_turn = (float *)(smem + (one_slab ? 0 : slab_acc_bytes));
  float *const stage = l.stage + (size_t)wave * l.stage_dwords;
  const int el = tid / N, ag = tid - el * N;
  const float invK = 1.0f / (float)K, invN = 1.0f / (float)N;
  const int NP = ((N + 3) & ~3) + 8;  // stride of a replica's positions in LDS (16-byte aligned pairs + padding)

  // ONE trip per block (the host launches ceil(replicas / epb) blocks): every pointer argument is
  // used once and dies, which is what keeps the kernel inside 128 VGPRs / 104 SGPRs.
  // All global loads go out before anything else: the table set-up below (a dependent global load +
  // barrier) then runs in their shadow.
  // Blocks are dealt to the 8 XCDs round-robin (block b runs on XCD b % 8).  A replica's rows of the state arrays are
  // 4 * N bytes, so with replicas in blockIdx order the first and last cache line of every such row is shared with a
  // block on ANOTHER XCD, whose L2 cannot merge the two halves before they go to memory.  Replicas of <= 128 agents
  // get a contiguous range of replica groups per XCD instead (a bijection of [0, gridDim.x) for any grid size; what a
  // replica computes does not depend on its block): headline tick 25.30 -> 24.81 us, 16 000 replicas 216 -> 210 us.
  // Replicas of > 128 agents keep blockIdx order: their rows are long, and the same remap measured 2.5 % SLOWER at
  // 500 replicas of 505 / 1005 agents (profiles/r06_ab_tc_block_order.txt).
  int group = blockIdx.x;
#ifndef WD_TC_BLOCK_ORDER_PLAIN
  if constexpr (IDB == 7) {
    const int bx = blockIdx.x & 7, bq = gridDim.x >> 3, br = gridDim.x & 7;
    group = bx * bq + min(bx, br) + (int)(blockIdx.x >> 3);
  }
#endif
  const int env0 = a.env_begin + group * epb;
  // Wave priority falls with the phase (3: fetch .. tags, 2: first half of the search, 0: the rest
  // of it and everything after, with a short stretch at 1 where the ids come out of the keys): a
  // wavefront that is behind wins VALU arbitration over one that is ahead, so the wavefronts of a
  // SIMD finish together.  The default oldest-first arbitration keeps leaders ahead
  // and leaves the last wavefront of every SIMD running alone, latency-bound (measured with the
  // two-pass search: 48.6 -> 44.4 us per tick; the schedule was re-tuned for the one-pass search,
  // experiments/README.md).
  __builtin_amdgcn_s_setprio(3);
  WD_TC_PROBE_RT(16); WD_TC_PROBE(0); WD_TC_PROBE_HW(21);
  TcIn in;
  bool reloaded = false;  // LOOP: block-uniform
  if constexpr (LOOP) {
    // The steady-state trip loads nothing but the slabs: the state is what this thread computed on the trip before.  Trip 0
    // of a launch and the trip after a restore read it from memory (all of it: which arrays a restore rewrites is the
    // host's choice), and wait for it, BEFORE the slabs are issued.
    in = cy->in;
    reloaded = cy->reload != 0;
    if (reloaded) {
      const TcPhase pv(a, fz);  // (a view of its own: cold)
      tc_load_state(in, pv.a, pv.fz, env0, epb, N, n_acc, n_turn, tid, tick == 0);
      cy->in.type = in.type; cy->in.skill = in.skill; cy->in.step_reward = in.step_reward;  // (no trip writes these)
    }
  } else {
    tc_issue_loads<FUSED, SAMPLE>(in, a, fz, env0, epb, N, n_acc, n_turn, tid, slab_acc, slab_turn, true);
  }
  const bool tab_in_lds = (n_acc <= WD_TC_TAB) && (n_turn <= WD_TC_TAB);
  int n_taggers_ = n_taggers_in;
  if constexpr (LOOP) {
    if (tick == 0) n_taggers_ = tc_build_tables(tb, a, N, n_acc, n_turn, tab_in_lds, in, tid);
  } else {
    n_taggers_ = tc_build_tables(tb, a, N, n_acc, n_turn, tab_in_lds, in);
  }
  const int n_taggers = n_taggers_;
  if (env0 >= a.E) return n_taggers;  // whole block (no barrier is skipped by part of a block; the same on every trip)
  if constexpr (!LOOP) WD_TC_PROBE(1);  // (LOOP: behind the slab issue below, so that the phase holds the same work)

  const int env = env0 + el;
  const bool active = (el < epb) && (env < a.E);
  const int gi = env * N + ag;  // index into [E, N] arrays
  const int li = tid;           // index into LDS arrays (= el * N + ag)
  const int agents_here = min(epb, a.E - env0) * N;
  if constexpr (LOOP) {
    // the pointers of this phase, taken behind the trip-end barrier and BEFORE the first piece of the slabs: the wait for
    // them stands in front of the store below, not inside the slab window
    const TcPhase pv(a, fz);
    // (a store between the slab issue and the slab wait would be waited for with the slabs: this one goes first)
    if (active && ag == 0) pv.a.done[env] = 0;  // a replica that finished (and was reset) last tick
    // the slabs alias the work area: issued here, after the trip-end barrier, never earlier
    // (straight-line code: the shape is a constant of this object -- a.N == SN, n_acc == n_turn == SA, one replica per
    // block, all set by the entry -- and so is where the slabs lie)
    static_assert(!LOOP || (SN > 0 && SA > 0 && ST == WD_TC_BLOCKDIM), "the multi-tick entry is built for one shape");
    tc_fetch_slabs_straight<SN, SA, ST>(slab_acc, slab_turn, pv.fz.probs_acc, pv.fz.probs_turn, env0, wave, lane);
    WD_TC_PROBE(1);
  }
  int2 sampled = in.sampled;
  const unsigned long long live_mask = __ballot(active && in.sg != 0);
  if constexpr (!LOOP) {
    if (compact && lane == 0) tb.live_cnt[wave] = __popcll(live_mask);
  }
  if constexpr ((IDB != 7) && (KMAX <= 12)) {  // (the cell-sorted packing's counters, see below)
    if (compact && tid < 64) tb.cell_cnt[tid] = 0;
  }
  if constexpr (LOOP) {
    // (two slabs side by side, no tc_one_slab path: replicas of at most 128 agents, which is what the 7-bit ids mean)
    static_assert(!LOOP || IDB == 7, "tc_sample_heads_carried samples from two slabs: replicas of at most 128 agents");
    sampled = tc_sample_heads_carried<SA>(a, fz, in.epoch, cy->k0, cy->k1, active, gi, li, slab_acc, slab_turn, n_acc, n_turn);
    if (compact && lane == 0) tb.live_cnt[wave] = __popcll(live_mask);  // (no LDS access between slab issue and slab wait)
  } else if (FUSED) {
    if (active && ag == 0) a.done[env] = 0;  // a replica that finished (and was reset) last tick
    if (SAMPLE) sampled = tc_sample_heads(a, fz, in, active, gi, li, slab_acc, slab_turn, n_acc, n_turn, env0, epb);
  }
  WD_TC_PROBE(2);
  __syncthreads();  // tables are published; every wavefront is done with the slabs
  WD_TC_PROBE(3);
  // (LOOP: obs_rows_cleared, from a view taken behind the barrier; the state arrays are stored on a closing trip only)
  typename TcPhaseArgs<LOOP>::type pv_move = tc_phase<LOOP>(a, fz);
  // packed index of this lane's agent among the agents in the game, and their number
  int my_c = ag, n_live = N;
  if (compact) {
    int before = 0;
    n_live = 0;
    for (int w2 = 0; w2 < n_waves; ++w2) {
      const int c = tb.live_cnt[w2];
      before += (w2 < wave) ? c : 0;
      n_live += c;
    }
    my_c = before + __popcll(live_mask & ((1ull << lane) - 1ull));
  }
  // the prefiltered search (tc_pre_pass1 / tc_pre_pass2): on for big replicas while enough agents are in the game
  constexpr bool PRE = (IDB != 7) && (KMAX <= 12);
  // equal distances are settled by agent id through the packed-index -> id table wherever the candidates of a block may be
  // packed in another order than ascending id (tc_tie_order, tc_knn.h): replicas of more than 128 agents, one per block
  constexpr bool TIE_TABLE = (IDB != 7);
  bool pre_on = false;  // block-uniform
  int cells_C = 0;      // block-uniform: side of the cell grid the agents in the game are packed by (0: by id)
  float cell_len = 0.0f, cell_inv = 0.0f;
  int my_cell = 0, my_cell_slot = 0;  // this lane's agent: its cell and its arrival number in it
  uint4 hint_a = make_uint4(~0u, ~0u, ~0u, ~0u), hint_b = hint_a;
  if constexpr (PRE) {
    pre_on = compact && (a.knn_prev != nullptr) && (n_live >= WD_TC_PRE_MIN_LIVE) && (l.stage_dwords >= WD_TC_LIST_DWORDS);
    if (pre_on && active && in.sg != 0) {  // (in flight during the move)
      const uint4 *const h = (const uint4 *)(a.knn_prev + (size_t)(env * N + ag) * 8);
      hint_a = h[0];
      hint_b = h[1];
    }
    // ... and then the agents in the game are packed by grid cell, not by id (tc_knn.h "CELL-SORTED packing")
    if (pre_on) {
      cells_C = tc_cell_grid(n_live, K);
      cell_len = a.grid_length / (float)max(cells_C, 1);
      cell_inv = (float)cells_C / a.grid_length;
    }
  }

  // ------------------------------------------------------------ move
  float edge_pen = 0.0f, my_x = 0.0f, my_y = 0.0f;
  const int sg = in.sg;
  const bool is_runner = active && (in.type == 0) && (sg != 0);  // member of self.runners
  if (active) {
    const TcMoved m = tc_move<LOOP, !LOOP>(tc_phase_a(pv_move), tb, in, sampled, gi, tab_in_lds, LOOP ? cy : nullptr, LOOP ? lc : nullptr);
    edge_pen = m.edge_pen; my_x = m.x; my_y = m.y;
    if constexpr (LOOP) {  // what the next trip would read back, and what a closing trip stores
      cy->in.x = m.x; cy->in.y = m.y;
      cy->in.cleared = (sg == 0) ? 1 : 0;
    }
    // agents out of the game are pushed to +BIG for the neighbour search only; every other
    // consumer (taggers are never out of the game) reads real positions
    // (with the prefilter on: NaN -- only its bound reads the entry of an agent that is out of the game then)
    l.xy[el * NP + ag] = make_float2(sg ? m.x : (PRE && pre_on ? __builtin_nanf("") : WD_BIG), m.y);
    if (compact) {
      if (sg) {
        bool by_cell = false;
        if constexpr (PRE) {
          if (cells_C != 0) {  // its packed place is known after the barrier (counting sort)
            const int2 c = tc_cell_xy(m.x, m.y, cell_inv, cells_C);
            my_cell = tc_cell_place(c, cells_C);
            my_cell_slot = atomicAdd(&tb.cell_cnt[my_cell], 1);
            by_cell = true;
          }
        }
        if (!by_cell) {
          l.xyc[my_c] = make_float2(m.x, m.y);
          l.cid[1 + my_c] = (short)ag;
          if (PRE && pre_on) {  // the hint goes to the lane that searches for this agent: slot my_c & 63 of wavefront my_c >> 6
            uint4 *const slot = (uint4 *)(l.stage + (size_t)(my_c >> 6) * l.stage_dwords) + 2 * (my_c & 63);
            slot[0] = hint_a;
            slot[1] = hint_b;
          }
        }
      }
      if (ag == 0) {
        l.cid[0] = -1;
        if (PRE && pre_on) {
          l.xyc[n_live] = make_float2(WD_BIG, WD_BIG);         // the pad candidate of pass 2: a position at +inf
          l.xy[N] = make_float2(__builtin_nanf(""), 0.0f);     // what a remembered id of 0xffff (none) reads
        }
      }
      if constexpr (LOOP) {
        // the pad candidates of wavefront 1's two half chains (the search below, "LANE HALVES"): places n_live ..
        // 2 h - 1, at most seven, one per lane of the first eight.  2 h <= 96 and the chain's last prefetch ends at
        // 2 h + 7 <= 103: inside the NP = 116 places of xyc
        if (tc_lane_halves(compact, n_waves, n_live) && ag < 8 && n_live + ag < 2 * tc_half_len(n_live))
          l.xyc[n_live + ag] = make_float2(WD_BIG, WD_BIG);
      }
    }
    tc_feat_store(l.feat, li, m.ft);
    // bit 0: in the game before this tick's tagging; bit 1: the observation row in HBM is all zeros already
    l.sig[li] = (sg ? 1 : 0) | (in.cleared ? 2 : 0);
    // after this tick's gather (either form) the row of an agent out of the game is zeros, the row of one in it is not
    if ((in.cleared != 0) != (sg == 0)) tc_phase_a(pv_move).obs_rows_cleared[gi] = sg ? 0 : 1;
    l.tagcnt[li] = 0;
    if (ag == 0) {
      const int t = in.tstep + 1;  // :800
      if constexpr (!LOOP) tc_phase_a(pv_move).timestep[env] = t;  // (LOOP: on a closing trip, from the carry)
      tb.tstep[el] = t;
      // float(t) / episode_length, :474 (LOOP: by the reciprocal, proved for t = 1 .. T by the same verifier)
      if constexpr (LOOP) tb.tfrac[el] = (float)tc_div_const((double)t, (double)a.T, lc->r_T);
      else tb.tfrac[el] = (float)((double)t / (double)a.T);
      if constexpr (LOOP) {
        cy->in.tstep = t;
        if (reloaded) tb.nrun[el] = in.nrun;  // (otherwise the count the last trip left there: the tables survive the trip)
      } else {
        tb.nrun[el] = in.nrun;
      }
    }
  }
  WD_TC_PROBE(4);
  __syncthreads();
  WD_TC_PROBE(5);
  int cell_incl = 0;  // lane c: agents in the game in cells 0 .. c (every wavefront scans the 64 counters for itself)
  if constexpr (PRE) {
    if (cells_C != 0) {  // block-uniform
      const int cnt = tb.cell_cnt[lane];
      cell_incl = cnt;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(cell_incl, d, 64);
        cell_incl += (lane >= d) ? up : 0;
      }
      my_c = __builtin_amdgcn_ds_bpermute(my_cell << 2, cell_incl - cnt) + my_cell_slot;
      if (active && sg != 0) {
        l.xyc[my_c] = make_float2(my_x, my_y);
        l.cid[1 + my_c] = (short)ag;
        uint4 *const slot = (uint4 *)(l.stage + (size_t)(my_c >> 6) * l.stage_dwords) + 2 * (my_c & 63);
        slot[0] = hint_a;
        slot[1] = hint_b;
      }
    }
  }

  // ------------------------------------------------------------ tags (counts are read after the
  // barrier that follows the gather)
  bool tagged = false;
  if constexpr (LOOP) {
    // the roots are taken only by a wavefront with a runner near enough for them to matter; lanes that are not runners
    // take no part in that vote
    if (is_runner)
      tagged = tc_find_tag<true>(tc_phase_a(pv_move), tb, l.xy + el * NP, l.tagcnt + el * N, &tb.nrun[el], n_taggers, my_x, my_y, lc->Bc);
  } else {
    if (is_runner)
      tagged = tc_find_tag(a, tb, l.xy + el * NP, l.tagcnt + el * N, &tb.nrun[el], n_taggers, my_x, my_y);
  }
  if constexpr (PRE) {
    if (cells_C != 0) __syncthreads();  // the packed positions, ids and hints are in place
  }

  // ------------------------------------------------------------ search
  WD_TC_PROBE(6);
  int nid[KMAX + 1], rank[KMAX + 1];  // entry k is one of the K nearest iff rank[k] < K
#pragma unroll
  for (int k = 0; k <= KMAX; ++k) { nid[k] = -1; rank[k] = k; }
  // in_order: slot k of the agent's row is entry k (true as well for agents that are not searched
  // for: all their entries are "none")
  bool in_order = true;
  __builtin_amdgcn_s_setprio(2);
  // searcher lane `ag` works for the ag-th agent in the game (packed) or for its own agent
  const bool searcher = compact ? (tid < n_live) : (active && sg != 0);  // (tid == ag for these lanes)
  const float2 *const sxy = compact ? l.xyc : l.xy + el * NP;
  const int n_cand = compact ? n_live : N;
  int row_agent = ag;  // the agent whose row this lane's search fills
  // TWO WAVEFRONTS PER SEARCHER while at most 64 agents are in the game (70 % of an episode of the benchmark
  // policy): the searchers then fit the first wavefront and the second one used to wait at the barrier below for
  // the whole search -- with two of the four wavefronts of a SIMD idle the chain is bound by the issue latency of a
  // single wavefront (~10 cycles per instruction), not by the VALU.  Now lane i of BOTH wavefronts works for searcher
  // i: wavefront 0 runs the chain over the first half of the candidates, wavefront 1 over the second half; wavefront
  // 1 hands its L keys over through its staging buffer (dead until the gather) and wavefront 0 merges the two sorted
  // lists (tc_merge_sorted: the L smallest of the union are exactly what one chain over all candidates keeps).
  // self + K others + the look-ahead entries: two; ONE where K == KMAX is known and the replica has at most 128 agents (the
  // BASELINE shape's entries): one v_med3_u32 less per candidate, near-ties at the cut go to tc_zone_resolve (tc_resolve_keys)
  constexpr int L = KMAX + ((EXACTK && IDB == 7) ? 2 : 3);
  const bool split = compact && (n_waves == 2) && (n_live <= 64) && (n_live >= 16) &&
                     (l.stage_dwords >= 64 * L);                          // block-uniform
  const int j_half = split ? (((n_live + 7) >> 3) << 2) : n_cand;        // first candidate of wavefront 1's half
  const bool helper = split && (wave == 1);                               // wave-uniform
  unsigned S[L];
  bool prefiltered = false;           // wave-uniform
  unsigned extra = 0xffffffffu;       // the (L+1)-th key (prefiltered search only)
  if constexpr (PRE) {
    if (pre_on) {  // block-uniform
      unsigned Tb = 0u;
      float sx = 0.0f, sy = 0.0f;
      int2 scell = make_int2(0, 0);
      if (searcher) {
        const uint4 *const slot = (const uint4 *)stage + 2 * lane;
        const uint4 pa = slot[0], pb = slot[1];
        sx = sxy[ag].x; sy = sxy[ag].y;
        Tb = tc_knn_bound16<KMAX>(l.xy, N, sx, sy, pa, pb, K);
        if (cells_C != 0) {  // nothing outside the searcher's 3 x 3 cell block is inside the radius
          scell = tc_cell_xy(sx, sy, cell_inv, cells_C);
          Tb = min(Tb, tc_cell_cover2(sx, sy, scell, cell_len, cells_C));
        }
      }
      WD_TC_PROBE(7);
      // every searcher of the wavefront has a radius -- and there IS a searcher: a wavefront without one (tid >=
      // n_live: up to 11 of 16 at ~300 agents in the game) would run pass 1 over every candidate for nothing and
      // compete for the VALU with the searching wavefronts of its SIMD; it goes straight to the barrier instead
      if (__ballot(searcher) != 0ull && __ballot(searcher && Tb == 0x7f800000u) == 0ull) {
        // (lanes without a searcher: radius -1, nothing listed; they only take part in the wave-wide votes)
        // (candidates popped per trip: the fullest lane of a 32-candidate word holds ~2 at 1000 agents, ~4 at 500)
        const float Tf = searcher ? __uint_as_float(Tb) : -1.0f;
#pragma unroll
        for (int k = 0; k < L; ++k) S[k] = 0xffffffffu;
        // Packed by id: ONE run, every candidate.  Packed by cell: the wavefront's searchers hold consecutive packed places,
        // i.e. the cells (x_lo, y_lo) .. (x_hi, y_hi) of the serpentine sweep; per cell row r, the cells within one column of
        // any of them in the rows r - 1 .. r + 1 are one run of packed places (the hull of the columns).  Runs are taken in
        // ascending order, widened to multiples of 4 places, never overlapping (a candidate must not enter the chain
        // twice) and joined where they touch.  All of it is scalar work; pass 1 and pass 2 have ONE call site each:
        // pass 1 lists up to WD_TC_LIST_CAP words of candidates (from one run or several), pass 2 empties the lists.
        const int C = cells_C;
        int r = 0, r_end = -1, run0 = 0, run1 = n_cand, x_lo = 0, y_lo = 0, x_hi = 0, y_hi = 0;
        if (C != 0) {
          const int last = min(63, __builtin_amdgcn_readfirstlane(n_live) - 1 - 64 * wave);
          x_lo = __builtin_amdgcn_readfirstlane(scell.x); y_lo = __builtin_amdgcn_readfirstlane(scell.y);
          x_hi = __builtin_amdgcn_readlane(scell.x, last); y_hi = __builtin_amdgcn_readlane(scell.y, last);
          r = max(0, y_lo - 1);
          r_end = min(C - 1, y_hi + 1);
          run1 = 0;
        }
        const TcPreList pl = tc_pre_list(stage, lane);
        int j = 0, j_end = 0;       // the part of the current run that pass 1 has not seen
        int listed = 0, words = 0;  // per lane: words in its list; wave-uniform: words since the last round of pass 2
        int probe_trips = 0;
        bool finished = false;
        while (!finished) {
          while (words < WD_TC_LIST_CAP) {
            if (j >= j_end) {  // the next run
              bool flush = false;
              int p0 = 0, p1 = 0;
              while (!flush && r <= r_end) {
                int lo = C, hi = -1;
                for (int yy = max(y_lo, r - 1); yy <= min(y_hi, r + 1); ++yy) {
                  // the columns of cell row yy that hold searchers of this wavefront: the sweep runs left to right in even
                  // rows, right to left in odd ones; it enters the wavefront at (x_lo, y_lo) and leaves it at (x_hi, y_hi)
                  const bool fwd = (yy & 1) == 0;
                  const int from = (yy == y_lo) ? x_lo : (fwd ? 0 : C - 1), to = (yy == y_hi) ? x_hi : (fwd ? C - 1 : 0);
                  lo = min(lo, min(from, to));
                  hi = max(hi, max(from, to));
                }
                lo = max(0, lo - 1);
                hi = min(C - 1, hi + 1);
                // (an odd row's cells are packed in descending column order)
                const int first_cell = r * C + ((r & 1) ? C - 1 - hi : lo), last_cell = r * C + ((r & 1) ? C - 1 - lo : hi);
                ++r;
                if (hi < lo) continue;
                const int b = first_cell == 0 ? 0 : __builtin_amdgcn_readlane(cell_incl, max(first_cell, 1) - 1);
                const int e = __builtin_amdgcn_readlane(cell_incl, last_cell);
                const int j0 = max(run1, b & ~3), j1 = min(n_cand, (e + 3) & ~3);
                if (j1 <= j0) continue;
                if (run1 > run0 && j0 != run1) { p0 = run0; p1 = run1; flush = true; run0 = j0; run1 = j1; }
                else if (run1 > run0) run1 = j1;
                else { run0 = j0; run1 = j1; }
              }
              if (!flush) {
                if (run1 <= run0) { finished = true; break; }
                p0 = run0; p1 = run1; run0 = run1;
              }
              j = p0;
              j_end = p1;
            }
            const int j_stop = min(j_end, j + 32 * (WD_TC_LIST_CAP - words));
            tc_pre_pass1(sxy, sx, sy, j, j_stop, Tf, pl, listed);
            words += (j_stop - j + 31) >> 5;
            j = j_stop;
          }
          if (words != 0) tc_pre_pass2<L, IDB>(sxy, sx, sy, pl, listed, S, extra, probe_trips);
          listed = 0;
          words = 0;
        }
        WD_TC_PROBE_VAL(18, probe_trips);
        // the radius held the K nearest iff the K-th other agent found (entry K with the agent's own) lies at least
        // two key buckets inside it: everything that was not listed is then past the buckets tc_resolve_keys looks at
        unsigned sK = S[KMAX];
#pragma unroll
        for (int k = 1; k < KMAX; ++k) sK = (k == K) ? S[k] : sK;
        const bool held = (sK >> IDB) + 2u <= (Tb >> IDB);
        prefiltered = __ballot(searcher && !held) == 0ull;
        WD_TC_PROBE_VAL(19, prefiltered ? 1 : 2);
        if (!prefiltered) extra = 0xffffffffu;
      }
      WD_TC_PROBE(8);
    }
  }
  bool half_lane = false;  // LOOP: this lane chains half of the candidates for a searcher of wavefront 1 (LANE HALVES)
  int half_up = 0;         //       and its candidates start here
  if constexpr (LOOP) {
    // LANE HALVES (the multi-tick entry, 65 .. 96 agents in the game): wavefront 1 holds n_live - 64 <= 32 searchers, and
    // ran the chain over all n_live candidates with at most half of its lanes at work -- on a VALU that the other
    // wavefronts of its SIMD are waiting for.  Lane l + 32 now works for the searcher of lane l: the lower lanes chain
    // the candidates [0, h), the upper lanes [h, 2 h), h = tc_half_len(n_live), in ONE call of the chain -- the same
    // groups for every lane, from a per-lane base, so that the indices in the upper lanes' keys are h too low until h
    // is added to the L keys that come out (they stay ascending: all L slots hold candidates, h >= 36 > L, and an index
    // of at most 2 h - 1 <= 95 carries nothing out of the low 7 bits).  The places n_live .. 2 h - 1 hold pad candidates
    // at (BIG, BIG) (the move phase): their keys are +inf with an index, behind the key of every candidate there is --
    // the candidates are the agents IN the game, whose positions are clipped to the arena, so no two of them are
    // infinitely far apart -- and at least 65 > L keys are real: no pad is among the L smallest of the union.  The halves
    // swap their lists (v_permlane32_swap) and merge them: the L smallest of the union, which is exactly what one chain
    // over all candidates keeps (the argument of the cross-wavefront split above), ids and their tie-break order
    // included since they ride in the keys.  Wavefront 0 is as it was; the priority drops where the chain drops it.
    const bool halves = tc_lane_halves(compact, n_waves, n_live) && (wave == 1);   // wave-uniform
    const int h_len = tc_half_len(n_live);
    half_lane = halves && ((lane & 31) < n_live - 64);
    half_up = (halves && lane >= 32) ? h_len : 0;
    if (searcher || (helper && lane < n_live) || half_lane) {
      const int me = helper ? lane : halves ? 64 + (lane & 31) : ag;
      tc_chain_range<L, IDB>(sxy + half_up, sxy[me].x, sxy[me].y, helper ? j_half : 0,
                             helper ? n_cand : halves ? h_len : j_half, S);
    }
  } else if (!prefiltered && (searcher || (helper && lane < n_live))) {
    // one pass with packed keys (this wavefront's share of the candidates)
    const int me = helper ? lane : ag;
    tc_chain_range<L, IDB>(sxy, sxy[me].x, sxy[me].y, helper ? j_half : 0, helper ? n_cand : j_half, S);
  }
  WD_TC_PROBE(9);
  if constexpr (LOOP) {
    // the partner's list comes from wavefront 1 (the split over the wavefronts) or from the other half of the lanes; ONE
    // merge serves both
    unsigned P[L];
    bool merge = false;
    if (split) {  // block-uniform
      if (helper && lane < n_live) {
#pragma unroll
        for (int k = 0; k < L; ++k) ((unsigned *)stage)[64 * k + lane] = S[k];
        __builtin_amdgcn_s_setprio(0);
      }
      __syncthreads();
      if (searcher) {
        const unsigned *const theirs = (const unsigned *)(l.stage + (size_t)l.stage_dwords);  // wavefront 1's buffer
#pragma unroll
        for (int k = 0; k < L; ++k) P[k] = theirs[64 * k + lane];
        merge = true;
      }
    } else if (half_lane) {
      tc_swap_lane_halves<L>(S, P, (unsigned)half_up);
      merge = true;
    }
    if (merge) tc_merge_sorted<L>(S, P);
  } else if (split) {  // block-uniform
    if (helper && lane < n_live) {
#pragma unroll
      for (int k = 0; k < L; ++k) ((unsigned *)stage)[64 * k + lane] = S[k];
      __builtin_amdgcn_s_setprio(0);
    }
    __syncthreads();
    if (searcher) {
      const unsigned *const theirs = (const unsigned *)(l.stage + (size_t)l.stage_dwords);  // wavefront 1's buffer
      unsigned P[L];
#pragma unroll
      for (int k = 0; k < L; ++k) P[k] = theirs[64 * k + lane];
      tc_merge_sorted<L>(S, P);
    }
  }
  bool exact = true;
  unsigned zone_hi = 0u;
  if (searcher) {
    // a lane with three candidates inside 256 ulps at the cut (~1e-7 per agent) repeats the search with the
    // two-pass one (up to 128 candidates) / has the whole wavefront resolve it (more)
    unsigned o[L - 1];
    __builtin_amdgcn_s_setprio(1);
    exact = tc_resolve_keys<KMAX, IDB, L, TIE_TABLE>(sxy, ag, K, S, o, nid, rank, in_order, l.cid);
    WD_TC_PROBE(10);
    {  // the last key bucket the answer can come from: the K-th other agent's + 1
      unsigned oKth = o[KMAX - 1];
#pragma unroll
      for (int k = 0; k < KMAX - 1; ++k) oKth = (k == K - 1) ? o[k] : oKth;
      zone_hi = (oKth >> IDB) + 1u;
    }
    if constexpr (PRE) {
      if (pre_on) {  // remember the K + 3 nearest others (agent ids, 16 bits each; 0xffff = none) for the next tick's radius
        unsigned w[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          unsigned pair = 0u;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int k = 2 * q + h;
            const unsigned key = (k < L - 1) ? o[k < L - 1 ? k : 0] : (k == L - 1) ? extra : 0xffffffffu;
            const unsigned id = (key >= 0x7f800000u) ? 0xffffu : (unsigned)(unsigned short)l.cid[1 + (key & ((1u << IDB) - 1u))];
            pair |= id << (16 * h);
          }
          w[q] = pair;
        }
        uint4 *const h = (uint4 *)(a.knn_prev + (size_t)(env * N + l.cid[1 + ag]) * 8);
        h[0] = make_uint4(w[0], w[1], w[2], w[3]);
        h[1] = make_uint4(w[4], w[5], w[6], w[7]);
      }
    }
    if (!exact && !(EXACTK && IDB == 7) && (IDB == 7 || n_cand <= 128)) {
      WD_TC_PROBE_VAL(20, 1);
      int nid2[KMAX], rank2[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; ++k) { nid2[k] = -1; rank2[k] = k; }
      tc_knn_registers<KMAX>(sxy, ag, n_cand, K, nid2, rank2);
#pragma unroll
      for (int k = 0; k < KMAX; ++k) { nid[k] = nid2[k]; rank[k] = rank2[k]; }
      nid[KMAX] = -1;
      rank[KMAX] = KMAX;
      in_order = false;
      exact = true;
    }
  }
  if constexpr (IDB != 7 || EXACTK) {
    // more than 128 candidates, or the chain with ONE look-ahead entry (L above): the lanes that need the exact resolution
    // get it from the whole wavefront, one after the other (tc_zone_resolve)
    unsigned long long need = __ballot(searcher && !exact);  // wave-uniform
    if (need != 0ull) {
      WD_TC_PROBE_VAL(20, 1);
      unsigned long long unresolved = 0ull;
      const float mx = searcher ? sxy[ag].x : 0.0f, my = searcher ? sxy[ag].y : 0.0f;
      while (need != 0ull) {
        const int fl = __ffsll((long long)need) - 1;
        need &= need - 1ull;
        const float sx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mx), fl));
        const float sy = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my), fl));
        const unsigned zh = (unsigned)__builtin_amdgcn_readlane((int)zone_hi, fl);
        const int self = __builtin_amdgcn_readlane(ag, fl);
        // (several replicas per block -- small replicas, never packed: the candidates are the replica's of lane fl)
        const float2 *const zxy = compact ? sxy : l.xy + __builtin_amdgcn_readlane(el, fl) * NP;
        const int cnt = tc_zone_resolve<TIE_TABLE>(zxy, n_cand, sx, sy, self, zh, IDB, K, (unsigned char *)stage, lane, l.cid);
        if (cnt > 64) {
          unresolved |= 1ull << fl;
        } else {
          const unsigned short *const out = (const unsigned short *)((const unsigned char *)stage + 128 + 512);
#pragma unroll
          for (int k = 0; k < KMAX; ++k) {
            const int v = (k < K) ? (int)out[k] : -1;
            if (lane == fl) { nid[k] = v; rank[k] = k; }
          }
          if (lane == fl) { nid[KMAX] = -1; rank[KMAX] = KMAX; in_order = false; }
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_wave_barrier();
      }
      if ((unresolved >> lane) & 1ull) {  // more than 64 candidates inside the zone: the K-pass scan, this lane alone
        int nid2[KMAX];
#pragma unroll
        for (int k = 0; k < KMAX; ++k) nid2[k] = -1;
        tc_knn_scan<KMAX, TIE_TABLE>(sxy, ag, n_cand, K, nid2, l.cid);  // (entries in the reference's order)
#pragma unroll
        for (int k = 0; k < KMAX; ++k) { nid[k] = nid2[k]; rank[k] = k; }
        nid[KMAX] = -1;
        rank[KMAX] = KMAX;
        in_order = false;
      }
    }
  }
  if (searcher && compact) {  // packed indices -> agent ids (cid[0] = -1 stands for "none")
    row_agent = l.cid[1 + ag];
#pragma unroll
    for (int k = 0; k <= KMAX; ++k) nid[k] = l.cid[1 + nid[k]];
  }
  __builtin_amdgcn_s_setprio(0);
  WD_TC_PROBE(11);

  // ------------------------------------------------------------ ids out: block-local 16-bit neighbour
  // ids per agent row in LDS (0xffff = none), read by the gather and turned into the
  // `nearest_neighbor_ids` rows after the barrier.  Entry k goes to slot k at fixed offsets; the few
  // lanes whose entries are not in order (a near-tie, fewer than K agents in the game) then rewrite
  // their rows by rank.
  if constexpr (LOOP) {
    static_assert(!LOOP || (EXACTK && KMAX == 10 && IDB == 7), "the id rows of the multi-tick entry are built for K = 10");
    // The multi-tick entry (one replica per block: block-local ids ARE agent ids) also stores the `nearest_neighbor_ids`
    // rows here, from the registers of the lanes that found them, in front of the barrier: 40 bytes at
    // ((env0 * N + row_agent) * K) int32, 8-byte aligned.  Nothing reads the 16-bit LDS copies back for it
    // (tc_flush_ids, which the one-tick entries keep, did so for every row on every tick).
    const bool any_out_of_order = __ballot(!in_order) != 0ull;  // wave-uniform
    const TcPhase pv_ids(a, fz);  // (nearest_ids alone)
    if (searcher) {
      // the LDS row, for the gather: ten halfwords as five dwords (rows are 20 bytes apart; -1 gives 0xffff)
      unsigned *const idrow = (unsigned *)(l.ids + row_agent * KMAX);
#pragma unroll
      for (int k = 0; k < KMAX; k += 2) idrow[k >> 1] = ((unsigned)nid[k] & 0xffffu) | ((unsigned)nid[k + 1] << 16);
      if (any_out_of_order && !in_order) {
        // entries not in slot order: the row is rewritten by rank as before, then read back (sign-extending: 0xffff
        // gives -1; the reads follow the lane's own writes in LDS order and are waited for before the store), so that
        // such a lane takes the common store below
        unsigned short *const hrow = l.ids + row_agent * KMAX;
#pragma unroll
        for (int k = 0; k <= KMAX; ++k)  // (K of the KMAX + 1 entries have a rank < K)
          if (rank[k] < KMAX) hrow[rank[k]] = (unsigned short)(nid[k] < 0 ? 0xffff : nid[k]);
#pragma unroll
        for (int k = 0; k < KMAX; ++k) nid[k] = (int)((const short *)hrow)[k];
      }
      tc_store_id_row<false>(pv_ids.a.nearest_ids + (long)env0 * (SN * KMAX), __umul24((unsigned)row_agent, 4u * KMAX), nid);
    }
    // An agent out of the game has the row ten times -1, and so it had on the tick before -- unless this is the first
    // tick it is out (an agent tagged on trip t is in the game, and a searcher, on t; on t + 1 it arrives here with
    // cleared == 0 and the row is written; from t + 2 on cleared == 1 and nothing is stored), or trip 0 of a launch or
    // the trip after a restore (`reloaded`: the host may have written anything to the array, and to obs_rows_cleared).
    // Its 16-bit LDS row is not written at all: the sparse gather reads the ids of live rows only (its row list), and
    // the dense gather reads idp[] of such a row in bounds and discards the value (`valid` needs me.type_sig & 1).
    if (active && sg == 0 && (reloaded || in.cleared == 0)) {
      int none[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; ++k) none[k] = -1;
      tc_store_id_row<true>(pv_ids.a.nearest_ids + (long)env0 * (SN * KMAX), __umul24((unsigned)ag, 4u * KMAX), none);
    }
  } else {
    const int ebase = el * N;
    const bool any_out_of_order = __ballot(!in_order) != 0ull;  // wave-uniform
    if (active && sg == 0) {  // out of the game: no neighbours
      unsigned short *const own = l.ids + (size_t)li * K;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) own[k] = 0xffff;
    }
    if (searcher) {
      unsigned short *const idrow = l.ids + (size_t)(ebase + row_agent) * K;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)  // (an in-order row holds K ids)
        if (k < K) idrow[k] = (unsigned short)(ebase + nid[k]);
      if (any_out_of_order && !in_order) {
#pragma unroll
        for (int k = 0; k <= KMAX; ++k)  // (K of the KMAX + 1 entries have a rank < K)
          if (rank[k] < K) idrow[rank[k]] = (unsigned short)(nid[k] < 0 ? 0xffff : ebase + nid[k]);
      }
    }
  }
  // ------------------------------------------------------------ gather: the block's rows are split
  // evenly over its wavefronts (105 agents: 53 + 52 rows instead of 64 + 41: one chunk less on the
  // longer side), so a wavefront also gathers rows whose neighbours another wavefront found
  __syncthreads();
  typename TcPhaseArgs<LOOP>::type pv_rows = tc_phase<LOOP>(a, fz);  // (LOOP: the observation array, from a view taken behind the barrier)
  const int rpw = (agents_here + n_waves - 1) / n_waves;
  const int wrow0 = wave * rpw;
  const int wrows = max(0, min(rpw, agents_here - wrow0));
  // nearest_neighbor_ids [E, N, K]: this wavefront's rows, straight from the 16-bit LDS copies
  // (LOOP: stored in front of the barrier, from registers)
  if constexpr (!LOOP)
    tc_flush_ids(l.ids + (size_t)wrow0 * K, a.nearest_ids + ((long)env0 * N + wrow0) * K, wrows * K, lane, wrow0, N,
                 invK, invN, epb == 1);
  WD_TC_PROBE(12);
  // the sparse form pays when few rows are live (late in an episode); wave-uniform choice
  const unsigned long long live_rows = __ballot(lane < wrows && (l.sig[wrow0 + lane] & 1));
  const int n_live_rows = __popcll(live_rows);
  // (LOOP: a constant pair of its own, WD_TC_LOOP_SPARSE_NUM / 16 -- both forms are valid on any tick, the choice is cost
  // alone, and a free-running block pays for latency where the one-tick kernel pays for bytes: docs/rounds/r30.md)
  constexpr int SPARSE_NUM = LOOP ? WD_TC_LOOP_SPARSE_NUM : 9, SPARSE_DEN = 16;
  if (n_live_rows * SPARSE_DEN <= wrows * SPARSE_NUM) {
    if constexpr (LOOP) {
      static_assert(!LOOP || (EXACTK && KMAX == 10), "the descriptor flush of the multi-tick entry is built for K = 10");
      tc_gather_rows_sparse<true, KMAX>(tc_phase_a(pv_rows), l, tb, stage, env0, wrow0, wrows, lane, K, N, invK, invN);
    } else {
      tc_gather_rows_sparse(a, l, tb, stage, env0, wrow0, wrows, lane, K, N, invK, invN);
    }
  } else if constexpr (LOOP) {
    // the same chunks, items and flush as below with what the one built shape fixes taken out of the chunk loop
    // (tc_rows.h, TcLeanDense)
    static_assert(!LOOP || (EXACTK && KMAX == 10 && IDB == 7 && SN > 64 && SN <= 128), "two wavefronts, one replica per block");
    tc_gather_rows_dense_lean<KMAX, SN>(tc_phase_a(pv_rows), l, tb, stage, env0, wave, lane, live_rows);
  } else {
    // observation rows, R rows per chunk: work item = (row, neighbour slot) -> 7 values at
    // row*F + c*K + k of the chunk image; then the time column; then the chunk leaves as one run.
    // A chunk holds at most 192 items (tc_stage_rows), i.e. at most 3 per lane; their (row, slot)
    // split is the same for every chunk and is worked out once.
    int R = tc_stage_rows(F, n_waves);
    if constexpr (IDB != 7) {  // replicas of more than 128 agents: the buffer is at least the search's lists -- fill it
      R = max(R, min(min(64, (l.stage_dwords - 20) / F), 192 / K));
    }
    constexpr int U = 3;
    int rr[U], so[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = lane + 64 * u;
      rr[u] = (int)(((float)t + 0.5f) * invK);  // t / K (exact: the quotient is >= 0.5/K away from an integer)
      so[u] = rr[u] * F + (t - rr[u] * K);      // offset of the item's first value in the chunk image
    }
    float *const obs_w = a.obs + ((long)env0 * N + wrow0) * F;
    for (int r0 = 0; r0 < wrows; r0 += R) {
      const int rc = min(R, wrows - r0);
      float *const dst = obs_w + (long)r0 * F;
      const int mis = (int)(((size_t)dst >> 2) & 3);
      const int items = rc * K;
      const unsigned short *const idp = l.ids + (size_t)(wrow0 + r0) * K;  // ids of item t: idp[t]
      const int fp = wrow0 + r0;
      // ids, then feature records, all reads of a lane's items in flight together.  A lane whose item
      // index is past the end recomputes the LAST item and writes the same values to the same place:
      // straight-line code (exec-mask branches would cost more than the duplicate work)
      int tt[U];
      unsigned jq[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { tt[u] = min(lane + 64 * u, items - 1); jq[u] = idp[tt[u]]; }
      const bool clamped2 = lane + 128 >= items, clamped1 = lane + 64 >= items, clamped0 = lane >= items;
      TcFeat me[U], nb[U];
      int off[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool cl = (u == 0) ? clamped0 : (u == 1) ? clamped1 : clamped2;
        // (row, offset) of the item: precomputed for unclamped lanes, recomputed for the last item
        const int r_last = rc - 1, o_last = r_last * F + (K - 1);
        const int r = cl ? r_last : rr[u];
        off[u] = cl ? o_last : so[u];
        me[u] = tc_feat_load(l.feat, fp + r);
        // no neighbour (or the agent is out of the game): its own record stands in, so every
        // difference below is +0.0 without a select
        const bool valid = ((me[u].type_sig & 1) != 0) && (jq[u] != 0xffffu);
        nb[u] = tc_feat_load(l.feat, valid ? (int)jq[u] : fp + r);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool valid = ((me[u].type_sig & 1) != 0) && (jq[u] != 0xffffu);
        unsigned mv = valid ? 0xffffffffu : 0u;
        asm volatile("" : "+v"(mv));  // (opaque: keeps the AND below from being turned into selects)
        const unsigned ts = (unsigned)nb[u].type_sig & mv;
        float *o = stage + mis + off[u];
        o[0] = (float)(nb[u].nx - me[u].nx);   // float64 difference, narrowed (:560)
        o[K] = (float)(nb[u].ny - me[u].ny);
        o[2 * K] = nb[u].nsp - me[u].nsp;      // float32 operands: the float64 difference rounds to this
        o[3 * K] = nb[u].nac - me[u].nac;
        o[4 * K] = nb[u].ndir - me[u].ndir;
        o[5 * K] = __uint_as_float(ts & 0x3f800000u);
        o[6 * K] = __uint_as_float((0u - (ts & 1u)) & 0x3f800000u);
      }
      if (lane < rc) {
        // time column: float(t) / episode_length for agents in the game, else 0 (:474,:493,:543)
        const int m = wrow0 + r0 + lane;
        const int e_m = (int)(((float)m + 0.5f) * invN);
        stage[mis + lane * F + 7 * K] = (l.sig[m] & 1) ? tb.tfrac[e_m] : 0.0f;
      }
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();
      tc_flush_run(stage, dst, rc * F, lane);
      asm volatile("" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
  }
  WD_TC_PROBE(13);
  __syncthreads();  // every runner's tag is counted
  WD_TC_PROBE(14);

  // ------------------------------------------------------------ rewards / done
  typename TcPhaseArgs<LOOP>::type pv_fin = tc_phase<LOOP>(a, fz);  // (LOOP: rewards, still_in_the_game, num_runners, done, behind the barrier)
  if (active) tc_finish_agent(tc_phase_a(pv_fin), tb, el, ag, gi, env, sg, is_runner, tagged, l.tagcnt[li], edge_pen, in.step_reward, FUSED, !LOOP);
  if constexpr (LOOP) {
    // CLOSING TRIP: the last trip of the launch, or the trip the replica's episode ends on (the predicate of
    // tc_finish_agent; tb.tstep and tb.nrun are final behind the barrier above, so it is block-uniform).  Nothing can read
    // the carried state from memory before one -- the next trip overwrites it, the host cannot look inside a launch -- so
    // only here does it go to memory: what the one-tick kernel stores on this trip.  In front of the `doneflag` barrier: the
    // restore's drain and barrier separate these stores from tc_reset_finished, which may rewrite the same rows, and the
    // trip after a restore (or the next launch) reloads every one of them.
    // (both words read, no short circuit: one wait for the pair; their index is a zero the compiler cannot see through --
    // a constant LDS address would be formed in front of the loop and parked in a lane; the launch's length comes from the
    // phase's view, so that nothing of it stays in a register across the trip either)
    int first = 0;
    asm volatile("" : "+v"(first));
    const int ended = ((tb.tstep[first] >= tc_phase_a(pv_fin).T) | (tb.nrun[first] == 0)) ? 1 : 0;
    if ((tick + 1 == pv_fin.n_ticks) | (__builtin_amdgcn_readfirstlane(ended) != 0)) {
      static_assert(!LOOP || SN > 0, "one replica of SN agents per block");
      const TcPhase pv_close(a, fz);  // (a view of its own: cold)
      if (active) tc_store_carried<SN>(pv_close.a, pv_close.fz, cy->in, edge_pen, in.epoch + 1u, env0, ag, tb.nrun[0]);
    }
  }
  if (FUSED) {
    __syncthreads();  // doneflag
    bool any = false;
    for (int e = 0; e < min(epb, a.E - env0); ++e) any = any || (tb.doneflag[e] != 0);
    if constexpr (LOOP) {
      if (active) {
        cy->in.sg = (tagged && tc_phase_a(pv_fin).runner_exits) ? 0 : sg;
        cy->in.epoch = in.epoch + 1u;
      }
      cy->reload = __builtin_amdgcn_readfirstlane(any ? 1 : 0);  // the next trip reads the restored rows from memory
    }
    if (any) {  // block-uniform, rare (once per episode)
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wavefront's stores are complete ...
      __syncthreads();                                  // ... before any wavefront rewrites the rows
      if constexpr (LOOP) {  // (the reset table and the time steps: a view of its own, behind the guard)
        const TcPhase pv_rst(a, fz);
        tc_reset_finished(pv_rst.a, pv_rst.fz, tb, env0, epb, tid);
      } else {
        tc_reset_finished(a, fz, tb, env0, epb);
      }
      if constexpr (LOOP) {
        // (Redundant TODAY: tc_fast_rollout's trip-end drain and barrier follow at once.  The pair is here so that the
        // restore is safe by itself -- the reload does not depend on the trip-end drain, which the steady-state trip no
        // longer needs and a later change may drop.  One barrier per episode.)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the rows this wavefront restored are complete ...
        __syncthreads();                                  // ... before any thread of the block reads its state again
      }
    }
  }
  WD_TC_PROBE(15); WD_TC_PROBE_RT(17);
  return n_taggers;
}

// `ticks` ticks of the block's replicas in ONE launch (one replica per block; the fused, sampling tick).  The replicas of a
// launch are independent, so nothing but the kernel boundary made replica r's tick t + 1 wait for replica s's tick t: here
// every block runs on at its own pace and the blocks of a CU drift out of phase (one block's fetch and row flush under
// another's search).  Every trip computes the whole tick, fetches both slabs again (the probabilities change every tick) and
// STORES what a caller of a tick reads: observations, neighbour ids, sampled actions, rewards, done flags, and the
// change-only still_in_the_game and obs_rows_cleared words.  What a trip does not do is read back the state its own threads
// computed on the trip before: sg, heading, acceleration, speed, position, RNG epoch, the cleared flag and the time step
// travel in registers (TcCarry; the runner count stays in tb.nrun), the Philox key is read once per launch.  Nor does it
// store that state where nobody can read it: the five state arrays, the edge penalty, epoch + 1, the time step and the
// runner count go to memory on CLOSING trips only -- the last trip of the launch and the trip the replica's episode ends on
// (tc_store_carried, in the rewards phase), with the values the one-tick kernel stores on that trip.  Any other trip's
// values would be overwritten by the next trip before the launch ends, and the host cannot look inside a launch; the trip
// after a restore reloads all of it, arrays the reset table leaves out included.  A steady-state trip is: done = 0,
// slab issue, Philox in the shadow of the fetch, slab wait, both inverse-CDF scans, move ... -- no other load, and no
// store, LDS access or second vmcnt wait between the slab issue and the slab wait.  The state is read from memory on trip 0
// of a launch (the host may have written anything in between) and on the trip after a restore (tc_reset_finished,
// block-uniform, once per episode: everything is reloaded, the reset table is the host's choice of arrays), in both cases
// with its wait BEFORE the slabs are issued.  Between two trips each wavefront waits for its own stores
// (s_waitcnt vmcnt(0)) and the block meets at a barrier:
//   * the trip after a restore reads what this one stored and the rows OTHER threads of the block restored; the restore
//     is followed by a drain and a barrier of its own.  All wavefronts of a block share their CU's vector L1, which
//     the stores write through, and every such read is a vector load issued after the barrier: it cannot return a line
//     older than the stores (the reset table, read with scalar loads, is never written);
//   * the probability slabs alias the work area: the next trip's global_load_lds may only go out once every wavefront
//     is done with this trip's staging buffers and tables.
// (Replacing the trip-end vmcnt(0) by the lgkmcnt(0) the LDS reuse needs was measured in round 21: correct -- every address
// is stored by the same wavefront on every trip it is stored on, same-wavefront stores to one address complete in program
// order, the restore keeps its drains -- but no faster, docs/rounds/r21.md; the drain stays.)
// No barrier across blocks, no communication between them.
template <int KMAX, bool EXACTK, int IDB, int SN, int SA, int ST>
__device__ __forceinline__ void tc_fast_rollout(const TcArgs &a, const TcFuse &fz, unsigned char *smem, int n_acc,
                                                int n_turn, int ticks) {
  int n_taggers = 0;
  TcCarry cy;
  cy.in = TcIn{};
  cy.reload = 1;
  // the Philox key never changes: read once per launch, kept in scalar registers
  cy.k0 = __builtin_amdgcn_readfirstlane(fz.rng_state[0]);
  cy.k1 = __builtin_amdgcn_readfirstlane(fz.rng_state[1]);
  // the reciprocals of the launch's divisors and the tag filter's bound: the only true divisions of the launch
  const TcLoopConsts lc = tc_loop_consts(a.max_speed, a.grid_length, a.T, a.margin);
  for (int tick = 0; tick < ticks; ++tick) {
    n_taggers = tc_fast_impl<KMAX, true, EXACTK, IDB, true, true, SN, SA, ST>(a, fz, smem, n_acc, n_turn, tick, n_taggers, &cy,
                                                                              &lc);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }
}

}  // namespace
