// tag_continuous.hip -- TagContinuous step / fused rollout tick for gfx950.
//
// Semantics: the reference CPU step, example_envs/tag_continuous/tag_continuous.py
//   update_state :339-401, compute_distance :403-420, k_nearest_neighbors :422-444,
//   generate_observation :446-610, compute_reward :612-678, done :880-883.
// Where the reference's own CUDA kernel (tag_continuous_step_pycuda.cu:351-520)
// disagrees with its CPU step the CPU wins: stable (distance, id) neighbour order,
// tag counts accumulated without races, no end-of-game bonus for a runner tagged out
// on the last tick.  Argument order is the reference kernel's (:351-385) plus trailing
// n_envs, the two action-table lengths and the first replica of the launch; the two O(N^2)
// global scratch arrays it sorts in HBM (neighbor_distances,
// neighbor_ids_sorted_by_distance; :167-199) are accepted and never touched.
//
// Two implementations share the move / reward code:
//
//   tc_fast_impl<KMAX>   N <= 1024 agents per replica, K <= KMAX <= 32 observed neighbours (K <= 16 beyond 512 agents)
//     (the BASELINE shape: N = 105, K = 10; entry points Hip...Step_K<k> / Tick_K<k> up to 128 agents, ..._K<k>_N512 up to
//     512, ..._K<k>_N1024 beyond).
//     block = `epb` whole replicas (105 agents -> 1 replica on 128 threads), thread = agent.
//       fetch    every global LOAD of the tick is issued first (state, step rewards, time step, action
//                tables; the memory counters return in order, so a load issued later would wait for all
//                stores issued before it); fused tick: each wavefront's rows of the two probability
//                tensors go straight into LDS (global_load_lds_dwordx4, 1 KiB per instruction);
//       sample   (fused tick) Philox4x32-10 + inverse CDF on a running float32 sum, both heads;
//       move     float32 kinematics exactly as numpy evaluates them (numpy-exact cos/sin);
//                post-move state staged in LDS (positions; 32-byte feature records);
//       tags     every runner finds its nearest tagger; tag counts through LDS atomics (their
//                block barrier is the one after the gather);
//       search   over the agents still IN THE GAME only (one replica per block: they are packed in
//                ascending id order -- as candidates, so the chain is as long as the live list, and as
//                searchers, so a wavefront without a live searcher skips the search; 54 of 105 agents
//                are in the game on average over an episode of the benchmark policy).  Per searcher,
//                in registers, ONE pass over the candidates: the candidate's packed index rides in
//                the low 7 bits of the squared distance through a v_med3_u32 chain that keeps the
//                K+3 smallest keys (K+2 -- ONE look-ahead entry -- where K == KMAX is known and the replica
//                has at most 128 agents: the BASELINE shape's entries; a near-tie at the cut, ~5e-4 per agent,
//                then goes to tc_zone_resolve); where the first K+1 keys are far enough apart the chain order
//                is the reference's order and the ids are read off the keys, otherwise the exact
//                (sqrt(d^2), id) keys of the first K(+1) entries are ranked by pairwise
//                compare-and-count -- an ISOLATED close pair by one exact compare of the two (round 4);
//                ~1e-7 of the agents repeat the search with the two-pass one (tc_knn_registers: exact K-th
//                distance, compare-mask pass, id-ordered peeling) or, beyond 128 candidates, have the whole
//                wavefront resolve the zone around the cut (tc_zone_resolve).  While at most 64 agents are in
//                the game both wavefronts of a block chain half of the candidates each (tc_merge_sorted).  Replicas
//                of more than 128 agents search inside a radius derived from the previous tick's neighbours while at
//                least 200 agents are in the game (tc_pre_pass1 / tc_pre_pass2, cell-sorted since round 6: one subtraction per candidate of the cell rows around a wavefront, the chain over
//                the candidates inside the radius only, the radius checked afterwards);
//       ids out  packed indices -> agent ids through an LDS table; 16-bit block-local ids per agent
//                row in LDS (entry k -> slot k; out-of-order lanes rewrite their rows by rank); one
//                block barrier; nearest_neighbor_ids rows are converted from them and stored;
//       gather   the block's rows are split evenly over its wavefronts; each WAVEFRONT turns its rows
//                into observation rows inside a private LDS staging buffer, a chunk of rows at a
//                time, and streams every chunk out as one contiguous run of write-through 16-byte
//                stores (the [E, N, F] layout makes a replica's rows contiguous); a wavefront with at most
//                9/16 of its rows live builds and stores the live rows only (tc_gather_rows_sparse);
//       rewards  tag counts -> rewards in the CPU's add order, done flags;
//       reset    (fused tick) finished replicas are restored in place from the registered
//                `*_at_reset` copies.
//     Wave priority falls with the phase (s_setprio 3, 2, 0), so the wavefronts of a SIMD finish together.
//
//   tc_generic_impl      full observations, or K beyond the specialisations (any N <= 1024; entry points
//     HipTagContinuousStep / HipTagContinuousTick): K-pass selection per agent, observation
//     rows written from a block-strided (row, slot) loop (16-byte stores in the
//     full-observation mode).
#include "wd_common.h"

// phases (each header: its own anonymous-namespace block; order = dependency order)
#include "tc_types.h"
#include "tc_kernarg.h"
#include "tc_fetch.h"
#include "tc_sample.h"
#include "tc_move.h"
#include "tc_tags.h"
#include "tc_reset.h"
#include "tc_knn.h"
#include "tc_rows.h"
#include "tc_fast.h"
#include "tc_generic.h"

// The arguments of the entries are listed ONCE, in tc_kernarg.h: WD_TC_PARAMS (a Step entry's), WD_TC_FUSE_PARAMS (what a
// Tick entry takes behind them: the reference needs 2 sampler launches, the step, and 13 reset launches per tick,
// trainer_base.py:392-426; the fused tick samples both action heads, steps and restores finished replicas in ONE launch)
// and WD_TC_ROLLOUT_PARAMS (the number of ticks of the multi-tick entry), with WD_TC_PACK / WD_TC_FUSE_PACK, which put
// them into TcArgs / TcFuse.

// ---- entries.  This file is compiled into SEVERAL code objects (warp_drive_amd/build.py UNITS; a build of all of them
// runs in parallel, and tuning one specialisation rebuilds one small object):
//   (no WD_TC_KM)                      the generic entries HipTagContinuousStep / Tick: any N <= 1024, any K, full
//                                      observations                                        -> wd_kernels_tc.hsaco
//   -DWD_TC_KM=<k> -DWD_TC_WAVES=<w>   the fast entries for K <= k: `_K<k>` up to 128 agents (7 id bits in the search
//        [-DWD_TC_BIG]                 keys), `_K<k>_N512` for 129 .. 512 (blocks of up to eight wavefronts, 9 id
//                                      bits) and, with WD_TC_BIG, `_K<k>_N1024` beyond      -> wd_kernels_tc_k<k>.hsaco
//   -DWD_TC_KM=<k> -DWD_TC_SHAPE_N=<n> -DWD_TC_SHAPE_A=<a> -DWD_TC_SHAPE_THREADS=<t>
//                                      `_K<k>_N<n>A<a>`: ONE shape (n agents, exactly k observed, a-way action heads,
//                                      blocks of t threads: the launch MUST use them, the host asserts it)
//                                      with its sizes as compile-time constants -- what the reference gets for EVERY
//                                      run by templating wkNumberAgents into the source it hands to nvcc
//                                      (template_env_config.h:19-21); built ahead of time for the BASELINE shape
//                                      (105 agents, K = 10, 21-way heads, 128 threads: -3.8 % per tick for the sizes, -3.3 % more for
//                                      the block size, experiments/README.md)
//                                                                                           -> wd_kernels_tc_k10_n105a21.hsaco
//   ... -DWD_TC_ROLLOUT=1              the same shape's multi-tick entry `HipTagContinuousRollout_K<k>_N<n>A<a>` alone
//                                                                                           -> wd_kernels_tc_k10_n105a21_rollout.hsaco
// Separate objects, so that work on the big-replica search never moves the registers or the code layout of the
// headline kernel.  Every fast size class has three entries: Step (actions given), Tick (sample both heads + step +
// restore finished replicas) and TickA (actions given -- drawn by the policy forward's epilogue, policy_mlp.hip --
// + step + restore; same arguments as Tick, the sampler's are ignored).
extern "C" {

#define WD_TC_CAT_(a, b) a##b
#define WD_TC_CAT(a, b) WD_TC_CAT_(a, b)
#define WD_TC_SMEM() extern __shared__ __attribute__((aligned(16))) unsigned char tc_smem[]

#if !defined(WD_TC_KM)

__global__ void HipTagContinuousStep(WD_TC_PARAMS) {
  WD_TC_SMEM();
  WD_TC_PACK();
  tc_generic_impl<false>(a, TcFuse{}, tc_smem, kNumAccelerationActions, kNumTurnActions);
}

__global__ void HipTagContinuousTick(WD_TC_PARAMS WD_TC_FUSE_PARAMS) {
  WD_TC_SMEM();
  WD_TC_PACK();
  WD_TC_FUSE_PACK();
  tc_generic_impl<true>(a, fz, tc_smem, kNumAccelerationActions, kNumTurnActions);
}

// Exhaustive proof, for the divisors of ONE env configuration, that the multi-tick entry's division by launch constants
// (tc_div_const behind tc_div_const_in_class, tc_divide.h -- the same functions, the same reciprocals from tc_loop_consts)
// returns the bits of the true division:
//   res[1], res[2]  every float32 bit pattern x (2^32 of them; a NaN quotient matches any NaN) against x / sp_div and
//                   x / two_pi, where x is in the class the form is used for; outside it tc_move divides, so there is nothing
//                   to compare (res[6] counts the patterns inside the class);
//   res[3]          every float32 pattern widened to float64 against x / diag, EXCEPT +-inf (res[5] counts the excluded
//                   patterns: 2), for which the form gives inf - inf: the dividends are positions clamped to [0, L];
//   res[4]          t / T for t = 1 .. T, narrowed to float32 as the time column is.
// -0.0 is NOT excluded: the form returns -0.0 for it (tc_divide.h).  res[1 .. 4] count mismatches; res[0], preset to 1 by
// the host, is cleared on any mismatch or when a divisor is not a positive finite number.  Run once per distinct
// (max_speed, grid_length, episode_length) by envs/tag_continuous.py::invariant_divide_ok; the env offers the multi-tick
// entry only when res[0] stays 1.
__global__ void HipTagContinuousVerifyInvariantDivide(float kMaxSpeed, float kGridLength, int kEpisodeLength, int *res) {
  const TcLoopConsts lc = tc_loop_consts(kMaxSpeed, kGridLength, kEpisodeLength, 0.0f);
  const float sp_div = tc_sp_div(kMaxSpeed);
  const double diag = tc_diag(kGridLength), Td = (double)kEpisodeLength;
  const uint32_t gtid = blockIdx.x * blockDim.x + threadIdx.x, gsize = gridDim.x * blockDim.x;
  if (gtid == 0) {
    const bool sane = sp_div > 0.0f && sp_div < __builtin_inff() && diag > 0.0 && diag < (double)__builtin_inff() &&
                      kEpisodeLength > 0;
    if (!sane) res[0] = 0;
    res[5] = 2;
  }
  int bad_sp = 0, bad_pi = 0, bad_diag = 0, bad_T = 0, in_class = 0;
  for (uint64_t i = gtid; i < (1ull << 32); i += gsize) {
    const float x = __uint_as_float((uint32_t)i);
    if (tc_div_const_in_class(x, 0.0f, 0.0f)) {
      ++in_class;
      const float w0 = x / sp_div, g0 = tc_div_const(x, sp_div, lc.r_sp);
      const float w1 = x / WD_TC_TWO_PI, g1 = tc_div_const(x, WD_TC_TWO_PI, WD_TC_R_TWO_PI);
      bad_sp += (__float_as_uint(w0) != __float_as_uint(g0)) && !(w0 != w0 && g0 != g0);
      bad_pi += (__float_as_uint(w1) != __float_as_uint(g1)) && !(w1 != w1 && g1 != g1);
    }
    if ((__float_as_uint(x) & 0x7fffffffu) != 0x7f800000u) {
      const double xd = (double)x, w = xd / diag, g = tc_div_const(xd, diag, lc.r_diag);
      bad_diag += (__double_as_longlong(w) != __double_as_longlong(g)) && !(w != w && g != g);
    }
  }
  for (int t = 1 + (int)gtid; t <= kEpisodeLength && t > 0; t += (int)min(gsize, 0x40000000u)) {
    const float w = (float)((double)t / Td), g = (float)tc_div_const((double)t, Td, lc.r_T);
    bad_T += __float_as_uint(w) != __float_as_uint(g);
  }
  if (bad_sp) atomicAdd(&res[1], bad_sp);
  if (bad_pi) atomicAdd(&res[2], bad_pi);
  if (bad_diag) atomicAdd(&res[3], bad_diag);
  if (bad_T) atomicAdd(&res[4], bad_T);
  if (bad_sp | bad_pi | bad_diag | bad_T) res[0] = 0;
  // (res[6 .. 7] are one 64-bit count: 2^32 does not fit an int)
  if (in_class) atomicAdd((unsigned long long *)(res + 6), (unsigned long long)in_class);
}

#elif defined(WD_TC_SHAPE_N)

// one shape, sizes folded: N, K (exactly KM) and the two head sizes are constants from here on
#define WD_TC_SHAPE_NAME(stem) WD_TC_CAT(WD_TC_CAT(WD_TC_CAT(WD_TC_CAT(WD_TC_CAT(stem, WD_TC_KM), _N), WD_TC_SHAPE_N), A), WD_TC_SHAPE_A)
static_assert(WD_TC_SHAPE_N <= 128, "the shape-specialised entries use the 7-bit-id search of replicas up to 128 agents");
#if defined(WD_TC_ROLLOUT)
// -DWD_TC_ROLLOUT: a unit of its own with ONE entry, `HipTagContinuousRollout_K<k>_N<n>A<a>`: the Tick entry's arguments
// plus the number of ticks; every block takes its replica through that many ticks (tc_fast_rollout, tc_fast.h).  After the
// launch memory holds what that many launches of the Tick entry leave; inside it a trip stores every output of its tick, but
// the state its threads carry in registers only on the last trip and on the trip an episode ends on.  A separate
// object, so that the one-tick entries below (and the records keyed to their object) never move with it.
static_assert(WD_TC_SHAPE_N > 64 && WD_TC_SHAPE_THREADS == 128, "one replica per 128-thread block");
__global__ void __launch_bounds__(512, 4) WD_TC_SHAPE_NAME(HipTagContinuousRollout_K)(WD_TC_PARAMS WD_TC_FUSE_PARAMS
                                                                                          WD_TC_ROLLOUT_PARAMS) {
  WD_TC_SMEM();
  WD_TC_PACK();
  WD_TC_FUSE_PACK();
  a.N = WD_TC_SHAPE_N; a.K = WD_TC_KM;
  // (the shape once more as template arguments: the loop's slab issue is written for constants, tc_fetch_slabs_straight)
  tc_fast_rollout<WD_TC_KM, true, 7, WD_TC_SHAPE_N, WD_TC_SHAPE_A, WD_TC_SHAPE_THREADS>(a, fz, tc_smem, WD_TC_SHAPE_A,
                                                                                        WD_TC_SHAPE_A, kNumTicks);
}
#else
__global__ void __launch_bounds__(512, 4) WD_TC_SHAPE_NAME(HipTagContinuousStep_K)(WD_TC_PARAMS) {
  WD_TC_SMEM();
  WD_TC_PACK();
  a.N = WD_TC_SHAPE_N; a.K = WD_TC_KM;
  tc_fast_impl<WD_TC_KM, false, true, 7>(a, TcFuse{}, tc_smem, WD_TC_SHAPE_A, WD_TC_SHAPE_A);
}
__global__ void __launch_bounds__(512, 4) WD_TC_SHAPE_NAME(HipTagContinuousTick_K)(WD_TC_PARAMS WD_TC_FUSE_PARAMS) {
  WD_TC_SMEM();
  WD_TC_PACK();
  WD_TC_FUSE_PACK();
  a.N = WD_TC_SHAPE_N; a.K = WD_TC_KM;
  tc_fast_impl<WD_TC_KM, true, true, 7>(a, fz, tc_smem, WD_TC_SHAPE_A, WD_TC_SHAPE_A);
}
__global__ void __launch_bounds__(512, 4) WD_TC_SHAPE_NAME(HipTagContinuousTickA_K)(WD_TC_PARAMS WD_TC_FUSE_PARAMS) {
  WD_TC_SMEM();
  WD_TC_PACK();
  WD_TC_FUSE_PACK();
  a.N = WD_TC_SHAPE_N; a.K = WD_TC_KM;
  tc_fast_impl<WD_TC_KM, true, true, 7, false>(a, fz, tc_smem, WD_TC_SHAPE_A, WD_TC_SHAPE_A);
}
#endif  // WD_TC_ROLLOUT

#else

#define WD_TC_NAME(stem, suffix) WD_TC_CAT(WD_TC_CAT(stem, WD_TC_KM), suffix)
#define WD_TC_FAST_ENTRIES(suffix, THREADS, WAVES, IDB, SPLIT_EXACT)                                            \
  __global__ void __launch_bounds__(THREADS, WAVES) WD_TC_NAME(HipTagContinuousStep_K, suffix)(WD_TC_PARAMS) {   \
    WD_TC_SMEM();                                                                                                \
    WD_TC_PACK();                                                                                                \
    if (SPLIT_EXACT && a.K == WD_TC_KM)                                                                          \
      tc_fast_impl<WD_TC_KM, false, SPLIT_EXACT, IDB>(a, TcFuse{}, tc_smem, kNumAccelerationActions, kNumTurnActions); \
    else                                                                                                         \
      tc_fast_impl<WD_TC_KM, false, false, IDB>(a, TcFuse{}, tc_smem, kNumAccelerationActions, kNumTurnActions); \
  }                                                                                                              \
  __global__ void __launch_bounds__(THREADS, WAVES) WD_TC_NAME(HipTagContinuousTick_K, suffix)(WD_TC_PARAMS WD_TC_FUSE_PARAMS) { \
    WD_TC_SMEM();                                                                                                \
    WD_TC_PACK();                                                                                                \
    WD_TC_FUSE_PACK();                                                                                           \
    if (SPLIT_EXACT && a.K == WD_TC_KM)                                                                          \
      tc_fast_impl<WD_TC_KM, true, SPLIT_EXACT, IDB>(a, fz, tc_smem, kNumAccelerationActions, kNumTurnActions);  \
    else                                                                                                         \
      tc_fast_impl<WD_TC_KM, true, false, IDB>(a, fz, tc_smem, kNumAccelerationActions, kNumTurnActions);        \
  }                                                                                                              \
  __global__ void __launch_bounds__(THREADS, WAVES) WD_TC_NAME(HipTagContinuousTickA_K, suffix)(WD_TC_PARAMS WD_TC_FUSE_PARAMS) { \
    WD_TC_SMEM();                                                                                                \
    WD_TC_PACK();                                                                                                \
    WD_TC_FUSE_PACK();                                                                                           \
    tc_fast_impl<WD_TC_KM, true, false, IDB, false>(a, fz, tc_smem, kNumAccelerationActions, kNumTurnActions);   \
  }
// up to 128 agents: the entry branches once on "exactly KM observed" (the unrolled row layout of the usual case)
WD_TC_FAST_ENTRIES(, 512, WD_TC_WAVES, 7, true)
WD_TC_FAST_ENTRIES(_N512, 512, WD_TC_WAVES, 9, false)
#if defined(WD_TC_BIG)
// replicas of 513 .. 1024 agents: blocks of up to sixteen wavefronts (1024 threads: the reference's default geometry
// serves up to 1024 agents per block, managers/function_manager.py:64-67), 10 id bits in the search keys (buckets of
// 1024 ulps of d2: the exactness argument of tc_resolve_keys holds for any bucket width)
WD_TC_FAST_ENTRIES(_N1024, 1024, 4, 10, false)
#endif

#endif

}  // extern "C"
