// tag_gridworld_n5_common.h -- the 5-agent TagGridWorld rollout and evaluation, written ONCE for the two code objects
// that hold them: tag_gridworld_n5.hip (wd_kernels_gw5.hsaco, finished replicas restart from their start state) and
// tag_gridworld_n5_pool.hip (wd_kernels_gw5_pool.hsaco, they restart from a random row of a reset pool).  A unit
// defines a VARIANT, a small trait struct
//     struct V { static constexpr bool POOL;           // restart from the reset pool (below: "pooled", else "plain")
//                static constexpr int MAX_COORD;       // cells per axis - 1 the quotient table holds: 63 or 255
//                static constexpr bool XCD_CONTIGUOUS; // replica groups dealt to the XCDs in contiguous ranges
//     };
// and its `extern "C"` entries around gw5_rollout<H, V> / gw5_evaluate<H, V::MAX_COORD>.  Where the two families differ
// the difference is BEHAVIOUR and stands under `if constexpr` with a one-line comment; the list is in the pool unit's
// header.
//
// The rollout is the TagGridWorld T-tick rollout (HipTagGridWorldRollout in tag_gridworld.hip) specialised for the shape
// every BASELINE config uses: N = 5 agents (4 taggers + the runner), full observations (F = 21), blocks of ONE
// wavefront = 12 replicas.  The host picks it when the shape matches (envs/tag_gridworld.py::tick_launch), the general
// kernel serves everything else.
//
// Why: at BASELINE configs[1] (1000 replicas) the rollout is 84 single-wavefront blocks, one per CU -- a tick is one
// wavefront's dependent chain (~530 instructions at ~5 cycles each, two block barriers, ~20 dependent LDS round
// trips: 2.14 us per tick).  What a block of one wavefront does not need:
//   * barriers and LDS vote flags: LDS operations of ONE wavefront execute in issue order, so a lane's read sees any
//     earlier write of another lane; "did any replica finish" is a ballot.  (The wavefront-scope fence at the top
//     of the tick loop is the language-level statement of the same thing; it compiles to nothing here -- the
//     instruction stream is identical with and without it, checked by diffing the assembly -- because every access
//     goes through the same image pointer and already may alias the others);
//   * positions in LDS for the tag check: the runner's cell reaches the replica's five lanes through one
//     ds_bpermute, "some tagger stands on it" is a ballot + a shift;
//   * the per-replica time step in LDS: every lane keeps its replica's in a register;
//   * float divisions per tick (x / L, y / L, t / episode_length: ~15 instructions each, correctly rounded): all
//     quotients that can occur are tabulated in LDS once per launch WITH THE SAME DIVISION, so the values are the
//     reference's bit for bit (tag_gridworld.py:208-214, :273);
//   * index arithmetic with runtime N, F, epb;
//   * the mid-launch write of restored rows to the global arrays: the kernel writes the state after the last tick to
//     every array it restores (positions, observations, time step), so only its LDS / register copies are restored
//     inside the loop.  The host checks the registered reset arrays (plain: exactly those three; pooled: the
//     observations, the positions come from the pool).
// Semantics, recording and random draws are those of HipTagGridWorldRollout (same arguments + the action table's
// device address, which lives in the main code object); parity: tests/test_gpu_gridworld.py, same test, same oracle.
//
// LIVE POLICY (the `_H32` / `_H64` rollout entries, the TagGridWorld counterpart of
// HipClassicControlCartPoleEnvRollout_H32 / _H64 in cartpole.hip): every tick evaluates a small network on the agent's
// current observation row instead of reading fixed probabilities -- policy forward, sampling, step, restart and
// recording of a whole training batch in ONE launch (the reference runs a framework forward + sampler + step + reset
// launches + three synchronisations per tick, trainer_base.py:383-428).  Two policies, as in the reference's
// TagGridWorld training config (run_configs/tag_gridworld.yaml: "tagger" for agents 0 - 3, "runner" for agent 4): two
// hidden layers of H = 32 or 64 ReLU units + one softmax head of 5 actions each.  Packed weights per policy
// (training/policy_kernel.py::pack_gridworld_policy): W0 [H][24] (rows of the 21 inputs, padded to 24 floats so that
// every row starts on a 16-byte boundary; the padding is never read), b0 [H], W1 [H][H], b1 [H], Wp [5][H], bp [5],
// float32, the block padded to a multiple of four floats.  Both sets live in LDS for the whole launch; a lane reads
// its own policy's.  The network and its parity contract: rollout_policy.h; restated on the host in
// oracle/tag_gridworld_np.py::policy_probabilities.
// Measured (profiles/r05_prepared_items_first_call.txt, 1000 replicas, 20 ticks per launch): 10.9 us per tick at
// H = 32, 30.1 at H = 64 -- the trainer's per-tick path costs 390 - 490 us per tick of the same replicas.
//
// EVALUATION (the `HipTagGridWorldEvaluate_*` entries, Trainer.evaluate_episodes; the TagGridWorld counterpart of
// HipClassicControlCartPoleEnvEvaluate_H32 / _H64): ONE episode of every replica in one launch with the same two
// networks, greedy or sampled -- the rollout's geometry, tables and tick, without recording, restart and final state
// (gw5_evaluate below).
//
// Dynamic LDS of the rollout, in this order, dwords (host: envs/tag_gridworld.py::gw5_lds_bytes, the same arithmetic):
//     observation image 12 * 105 | restore cache 12 * CD | coordinate quotients MAX_COORD + 1 | time table
//     roundup4(episode_length + 1) | pooled only: the two pools, 2 * roundup4(5 * n_pool) | the two packed policies
//     2 * gw5_policy_floats(H)
// Every part is a whole number of 16-byte vectors, so the policies start aligned.  The evaluation has neither cache
// nor pools.  (The fixed-probability plain entry reads nothing behind its time table; the host does not round that
// table up for it.)
#pragma once
#include "wd_common.h"
#include "rollout_policy.h"
#include "tag_gridworld_rewards.h"

namespace {

constexpr int GW5_N = 5, GW5_F = 21, GW5_EPB = 12;
constexpr int GW5_ROW = GW5_N * GW5_F;        // 105 floats: one replica's observation rows
constexpr int GW5_IMG = GW5_EPB * GW5_ROW;    // 1260 floats: the block's observation image
constexpr int GW5_IN_STRIDE = 24;             // floats per row of W0 (21 inputs + padding)
constexpr int GW5_ACTIONS = 5;

// floats of one policy's packed weights, rounded up to whole 16-byte vectors (the second policy starts aligned)
__host__ __device__ constexpr int gw5_policy_floats(int H) {
  return rp_pad4(rp_policy_floats(GW5_IN_STRIDE, H, GW5_ACTIONS));
}

__device__ __forceinline__ int gw5_roundup4(int n) { return (n + 3) & ~3; }

// the action probabilities of one agent (the evaluation entries: the greedy action is their first maximum): w = its
// policy's packed weights (LDS), x = its observation row (LDS, 21 floats).  rollout_policy.h behind the first layer at
// stride 24 plus a tail column; the action count is a constant, so the head's guards fold away
template <int H>
__device__ __forceinline__ void gw5_policy_probs(const float *w, const float *x, float (&prob)[GW5_ACTIONS]) {
  float h1[H], logit[GW5_ACTIONS];
  rp_first_layer_strided<H, GW5_F, GW5_IN_STRIDE>(w, w + H * GW5_IN_STRIDE, x, h1);
  const float m = rp_policy_logits<H>(w + H * GW5_IN_STRIDE + H, h1, GW5_ACTIONS, logit);
  rp_softmax_probs(logit, m, GW5_ACTIONS, prob);
}

// their running float32 sums (the rollout's counting draw), the last repeated up to eight entries
template <int H>
__device__ __forceinline__ void gw5_policy_cum(const float *w, const float *x, float (&cumv)[8]) {
  float prob[GW5_ACTIONS];
  gw5_policy_probs<H>(w, x, prob);
  float cum = 0.0f;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    if (a < GW5_ACTIONS) cum = (a == 0) ? prob[0] : cum + prob[a];
    cumv[a] = cum;
  }
}

// every coordinate quotient a tick can need, computed with the division the reference's expression compiles to
template <int MAX_COORD>
__device__ __forceinline__ void gw5_fill_coord_table(float *s_div, int lane, int world_boundary) {
  const float L = (float)world_boundary;
  if constexpr (MAX_COORD < 64) {  // the 64-entry table: one predicated statement
    if (lane <= world_boundary) s_div[lane] = (float)lane / L;
  } else {                         // the 256-entry table: a strided loop
    for (int q = lane; q <= world_boundary; q += 64) s_div[q] = (float)q / L;
  }
}

// H = 0: fixed probabilities (`probs`); H = 32 / 64: the live policies.  The four pool arguments are read by the
// pooled variant only (the plain entries pass null pointers and 0)
template <int H, class V>
__device__ __forceinline__ void gw5_rollout(
    int *states_x_arr, int *states_y_arr, int *actions_arr, int *done_arr, float *rewards_arr, float *obs_arr,
    double wall_hit_penalty, double tag_reward_for_tagger, double tag_penalty_for_runner, double step_cost_for_tagger,
    int use_full_observation, int world_boundary, int *env_timestep_arr, int episode_length, int n_agents, int n_envs,
    uint32_t *rng_state, const float *probs, int n_actions, const void *reset_table, int n_reset_arrays,
    int stream_tag, int ticks, float *obs_batch, int *action_batch, float *reward_batch, int *done_batch,
    int reset_cache_dwords, const int *action_table, const float *policy_tagger, const float *policy_runner,
    uint32_t *pool_rng, const int *pool_x, const int *pool_y, int n_pool, float *gw5_smem) {
  if constexpr (V::POOL) {  // pooled only: (uniform) shapes the tables below are not sized for; the host admits none
    if (n_agents != GW5_N || use_full_observation == 0 || world_boundary < 0 || world_boundary > V::MAX_COORD ||
        episode_length < 1 || n_pool < 1 || reset_cache_dwords < GW5_ROW || pool_rng == nullptr)
      return;
  }
  const int CD = reset_cache_dwords;                        // dwords per replica in the restore cache
  float *const s_obs = gw5_smem;                            // [12][5][21] the block's observation image (16-byte aligned)
  uint32_t *const s_cache = (uint32_t *)(s_obs + GW5_IMG);  // [12][CD] the rows finished replicas are restored from
  float *const s_div = (float *)(s_cache + GW5_EPB * CD);   // [MAX_COORD + 1] c / L
  float *const s_tn = s_div + V::MAX_COORD + 1;             // [episode_length + 1] t / episode_length
  // pooled only: the two pools between the time table and the policies, [n_pool][5] each
  const int pool_dwords = V::POOL ? gw5_roundup4(GW5_N * n_pool) : 0;
  int *const s_pool_x = (int *)(s_tn + gw5_roundup4(episode_length + 1));
  int *const s_pool_y = s_pool_x + pool_dwords;
  // the two policies' packed weights behind the tables, on a 16-byte boundary (host: the same arithmetic)
  float *const s_pol = (float *)(s_pool_y + pool_dwords);   // [2][gw5_policy_floats(H)]: tagger, runner
  GW_REWARD_TABLE(wall_hit_penalty, tag_reward_for_tagger, tag_penalty_for_runner, step_cost_for_tagger);
  const int lane = threadIdx.x;                             // (blocks are one wavefront)
  const int el = lane / GW5_N, ag = lane - el * GW5_N;      // local replica (12 = none), agent
  const wd_reset_entry *const table = (const wd_reset_entry *)reset_table;
  const uint32_t k0 = rng_state[0], k1 = rng_state[1];
  uint32_t pk0 = 0u, pk1 = 0u;  // pooled only: the keys of the resetter's pool generator
  if constexpr (V::POOL) { pk0 = pool_rng[0]; pk1 = pool_rng[1]; }
  int act_dx[5], act_dy[5];  // the action table, once per launch (scalar registers)
#pragma unroll
  for (int i = 0; i < 5; ++i) { act_dx[i] = action_table[2 * i]; act_dy[i] = action_table[2 * i + 1]; }
  {
    gw5_fill_coord_table<V::MAX_COORD>(s_div, lane, world_boundary);
    for (int q = lane; q <= episode_length; q += 64) s_tn[q] = (float)q / (float)episode_length;
    if constexpr (V::POOL) {  // pooled only: both pools to LDS, so that the tick loop has no plain global load
      for (int q = lane; q < GW5_N * n_pool; q += 64) {
        s_pool_x[q] = pool_x[q];
        s_pool_y[q] = pool_y[q];
      }
    }
    if constexpr (H > 0) {
      for (int q = lane; q < gw5_policy_floats(H); q += 64) {
        s_pol[q] = policy_tagger[q];
        s_pol[gw5_policy_floats(H) + q] = policy_runner[q];
      }
    }
  }

  // Blocks are dealt to the 8 XCDs round-robin (block b runs on XCD b % 8), and a block's action / reward / done rows
  // are 240 / 240 / 48 bytes: with replicas in blockIdx order every such row shares its first and last cache line with
  // a block on ANOTHER XCD, whose L2 cannot merge the two halves.  Give each XCD a contiguous range of replica groups
  // instead (a bijection of [0, gridDim.x) for any grid size); what a replica computes does not depend on its block.
  // Measured (profiles/r06_ab_gridworld_block_order.txt): 20 000 replicas x 50 ticks 145.0 -> 127.8 us, 100 000 x 50
  // 728 -> 688 us, 1 000 x 100 (84 blocks) equal within the run-to-run spread.
  int group0 = blockIdx.x;
  if constexpr (V::XCD_CONTIGUOUS) {
    const int xcd = blockIdx.x & 7, nq = gridDim.x >> 3, nr = gridDim.x & 7;
    group0 = xcd * nq + min(xcd, nr) + (blockIdx.x >> 3);
  }
  for (int env0 = group0 * GW5_EPB; env0 < n_envs; env0 += gridDim.x * GW5_EPB) {
    const int env = env0 + el;
    const bool active = (el < GW5_EPB) && (env < n_envs);
    const int idx = env * GW5_N + ag;
    const int envs_here = min(GW5_EPB, n_envs - env0);
    const int n_out = envs_here * GW5_ROW;
    float *const obs_blk = obs_arr + (long)env0 * GW5_ROW;
    int x = 0, y = 0, t = 0;
    uint32_t epoch0 = 0u, pool_epoch = 0u;
    wd_u4 blk = wd_u4{0u, 0u, 0u, 0u};  // the Philox block of four consecutive ticks (wd_tick_draw)
    uint32_t blk_quad = 0xffffffffu;
    float cumv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) cumv[i] = 0.0f;
    if (active) {
      x = states_x_arr[idx];
      y = states_y_arr[idx];
      t = env_timestep_arr[env];
      epoch0 = rng_state[WD_RNG_HEADER + idx];
      if constexpr (V::POOL) pool_epoch = pool_rng[WD_RNG_HEADER + env];  // pooled only: the replica's pool epoch word
      if constexpr (H == 0) {
        const float *row = probs + (long)idx * n_actions;
        float cum = 0.0f;  // the running float32 sums of the (fixed) probabilities, once per launch
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          if (i < n_actions) cum = (i == 0) ? row[0] : cum + row[i];
          cumv[i] = cum;
        }
      }
    }
    for (int q = lane; q < n_out; q += 64) s_obs[q] = obs_blk[q];  // the observation the first action is sampled on
    // the rows finished replicas are restored from: per registered array one flat, coalesced copy of the block's rows.
    // Plain: positions and observations are found in it.  Pooled: the observations alone (the rows of the START
    // positions, the reference's placeholder); another array only takes its room, the copy is clamped to the block's
    // replicas and stops at a replica's share (never: CD is the sum of the rows)
    int off_x = 0, off_y = 0, off_obs = 0;
    {
      int off = 0;
      for (int r = 0; r < n_reset_arrays; ++r) {
        const wd_reset_entry ent = table[r];
        const int re = ent.row_elems;
        if constexpr (V::POOL) {
          if (off + re > CD) break;
        } else {
          if ((size_t)ent.data == (size_t)states_x_arr) off_x = off;
          if ((size_t)ent.data == (size_t)states_y_arr) off_y = off;
        }
        if ((size_t)ent.data == (size_t)obs_arr) off_obs = off;
        const wd_global_u32 *const src = ent.ref + (long)env0 * re;
        const float inv_re = 1.0f / (float)re;
        for (int q = lane; q < envs_here * re; q += 64) {
          int e = (int)(((float)q + 0.5f) * inv_re);  // q / re (exact for these sizes)
          if constexpr (V::POOL) e = min(e, envs_here - 1);
          s_cache[e * CD + off + (q - e * re)] = src[q];
        }
        off += re;
      }
    }
    __syncthreads();
    // every value loaded above is consumed HERE: the wait for a load whose first use is inside the tick loop is placed
    // inside the loop and -- the memory counter returns in order -- waits for the previous tick's stores on every trip
    if constexpr (V::POOL)  // pooled only: the pool epoch word is one of them
      asm volatile("" : "+v"(x), "+v"(y), "+v"(t), "+v"(epoch0), "+v"(pool_epoch));
    else
      asm volatile("" : "+v"(x), "+v"(y), "+v"(t), "+v"(epoch0));
    if constexpr (H == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(cumv[i]));
    }
    const float *const my_policy = s_pol + ((ag == GW5_N - 1) ? gw5_policy_floats(H) : 0);  // runner : tagger
    float last_reward = 0.0f;
    int last_action = 0, last_done = 0;
    float *const rep = s_obs + min(el, GW5_EPB - 1) * GW5_ROW;  // this lane's replica's five rows
    const uint32_t *const my_cache = s_cache + min(el, GW5_EPB - 1) * CD;
    const int runner_lane = min(el * GW5_N + GW5_N - 1, 63);

    for (int k = 0; k < ticks; ++k) {
      // the previous tick's image writes / restores, before this tick's record reads (the fixed-policy entry's statement of
      // what holds anyway -- LDS operations of one wavefront execute in issue order; it compiles to nothing there)
      if constexpr (H == 0) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      // ---- record the observation of this tick (flat, coalesced; none of the record stores is tracked).  The usual
      // case -- the block's slice of the row is a whole number of 16-byte vectors on a 16-byte boundary -- reads its
      // (up to) five vectors per lane with all LDS reads in flight, then stores them; a loop of read / wait / store
      // is five LDS round trips one after the other
      float *const brow = obs_batch + ((long)k * n_envs + env0) * GW5_ROW;
      if ((((size_t)brow & 15) | (size_t)(n_out & 3)) == 0) {  // block-uniform
        const int nvec = n_out >> 2;  // 315 for a full block
        const float4 *const img4 = (const float4 *)s_obs;
        float4 v[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) v[i] = img4[min(lane + 64 * i, GW5_IMG / 4 - 1)];  // (clamped into the image)
#pragma unroll
        for (int i = 0; i < 5; ++i)
          if (lane + 64 * i < nvec) wd_store_untracked((float4 *)brow + lane + 64 * i, v[i]);
      } else {
        for (int q = lane; q < n_out; q += 64) wd_store_untracked(brow + q, s_obs[q]);
      }
      bool hit = false;
      int a = 0;
      if (active) {
        const int n_act = (H > 0) ? GW5_ACTIONS : n_actions;
        // ---- sample (random.cu:51-85), the draw of tick k of T single-tick launches
        const float u = wd_u01_open_closed(wd_tick_draw((uint32_t)idx, epoch0 + (uint32_t)k, (uint32_t)stream_tag, k0, k1,
                                                        blk, blk_quad));
        // the LIVE policy on this tick's observation row (the image still holds what was recorded above).  AFTER the
        // draw: placed in front of it (the Philox refill is a branch) the scheduler hoists the network's ~1 500 LDS
        // operand reads over the whole block and the allocator spills 5 483 registers at H = 64 (13 x the tick time)
        if constexpr (H > 0) gw5_policy_cum<H>(my_policy, rep + ag * GW5_F, cumv);
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) cnt += (i < n_act && cumv[i] < u) ? 1 : 0;
        a = min(cnt, n_act - 1);
        wd_store_untracked(action_batch + ((long)k * n_envs * GW5_N + idx), a);
        // ---- movement :152-173
        int ddx = act_dx[0], ddy = act_dy[0];
#pragma unroll
        for (int i = 1; i < 5; ++i) { ddx = (a == i) ? act_dx[i] : ddx; ddy = (a == i) ? act_dy[i] : ddy; }
        const int ux = x + ddx, uy = y + ddy;
        const int cx = min(max(ux, 0), world_boundary), cy = min(max(uy, 0), world_boundary);
        hit = (ux != cx) || (uy != cy);  // :163-170
        x = cx;
        y = cy;
        t += 1;  // :295
      }
      // ---- tag check :175-178: does a tagger stand on the runner's cell?  (all 64 lanes take part in the exchange)
      const int cell = x | (y << 8);
      const int runner_cell = __shfl(cell, runner_lane);
      const unsigned long long on_runner = __ballot(active && (ag < GW5_N - 1) && (cell == runner_cell));
      const bool tag = ((unsigned)(on_runner >> (min(el, GW5_EPB - 1) * GW5_N)) & 0xfu) != 0u;
      const bool fin = active && ((t >= episode_length) || tag);  // :314
      if (active) {
        if (ag == 0) wd_store_untracked(done_batch + ((long)k * n_envs + env), fin ? 1 : 0);
        last_done = fin ? 1 : 0;
        last_reward = GW_REWARD(ag < GW5_N - 1, tag, hit);
        wd_store_untracked(reward_batch + ((long)k * n_envs * GW5_N + idx), last_reward);
        last_action = a;
        // ---- the image: only the positions and the time change from tick to tick (the type and "is me" columns are
        // constants that arrived with the image and return with a restore); this lane's agent is column ag (x) and
        // 5 + ag (y) of its replica's five rows, the time is column 20 of its own row.  x, y were clipped to 0 ..
        // world_boundary <= MAX_COORD just above.  Pooled only: the time-table read is clamped -- a time step past the
        // table (a start state that was already timed out) finishes the replica on this tick, and its rows are restored
        // below before anyone reads them
        const float fx = s_div[x], fy = s_div[y];
        float tnorm;
        if constexpr (V::POOL) tnorm = s_tn[min(max(t, 0), episode_length)];
        else tnorm = s_tn[t];
#pragma unroll
        for (int i = 0; i < GW5_N; ++i) {
          rep[i * GW5_F + ag] = fx;
          rep[i * GW5_F + GW5_N + ag] = fy;
        }
        rep[ag * GW5_F + 4 * GW5_N] = tnorm;
      }
      // ---- restart finished replicas: register and LDS copies only (see the header)
      unsigned long long fm = __ballot(fin);  // wave-uniform
      if (fm == 0ull) continue;
      if (fin) {
        if constexpr (V::POOL) {
          // pooled: the row reset_when_done_from_pool (wd_core.hip) draws for this replica at this epoch (its five
          // lanes compute the same one); inside the `fm != 0` branch, so a tick without a finished replica runs none of it
          const wd_u4 rnd = wd_philox4x32_10(wd_u4{(uint32_t)env, pool_epoch, 0x706f6f6cu, 2u}, pk0, pk1);
          const float p = (float)(rnd.x >> 8) * 0x1.0p-24f;
          const int ref_id = min((int)(p * (float)n_pool), n_pool - 1);
          x = s_pool_x[ref_id * GW5_N + ag];
          y = s_pool_y[ref_id * GW5_N + ag];
          t = 0;
          pool_epoch += 1u;
        } else {  // plain: the start positions, from the restore cache
          x = (int)my_cache[off_x + ag];
          y = (int)my_cache[off_y + ag];
          t = 0;
        }
      }
      while (fm != 0ull) {
        const int e = ((__ffsll((long long)fm) - 1) * 13) >> 6;  // lane / 5 for lanes < 64
        fm &= ~(0x1full << (e * GW5_N));
        for (int q = lane; q < GW5_ROW; q += 64) s_obs[e * GW5_ROW + q] = __uint_as_float(s_cache[e * CD + off_obs + q]);
      }
    }
    // ---- what the launch leaves in the per-tick arrays: the state after its last tick
    if (active) {
      states_x_arr[idx] = x;
      states_y_arr[idx] = y;
      rewards_arr[idx] = last_reward;
      actions_arr[idx] = last_action;
      rng_state[WD_RNG_HEADER + idx] = epoch0 + (uint32_t)ticks;
      if (ag == 0) {
        done_arr[env] = last_done;
        env_timestep_arr[env] = t;
        if constexpr (V::POOL) pool_rng[WD_RNG_HEADER + env] = pool_epoch;  // pooled only: one restart = one epoch
      }
    }
    for (int q = lane; q < n_out; q += 64) obs_blk[q] = s_obs[q];
    __syncthreads();  // (the next trip overwrites the image and the cache)
  }
}

// One episode of every replica with the two policies inside the kernel: the rollout's geometry (a wavefront = 12
// replicas, lane = (local replica, agent)), its quotient tables and packed policies in LDS, its tick -- draw, network,
// move, tag check by shuffle + ballot, image update -- but NO restart (no reset table, no restore cache, no pool), no
// recording and no final state: positions, time step, epoch word and observation rows are loaded once, a replica runs
// from them up to its first finished tick (or `ticks`) and stops; its lanes then only take part in the wavefront
// exchanges, and the group's loop ends when a ballot finds no live replica.  use_argmax: the action is the first maximum
// of the probabilities (the standalone sampler's strict-'<' scan); otherwise the rollout's counting draw on their running
// sums.  The two families differ in the quotient table alone (MAX_COORD = 63 or 255).
// WRITES eval_reward_sum [n_envs, 5] (float32, sum += reward in tick order, the terminal tick included), eval_steps /
// eval_done [n_envs] (done: 1, or 0 when `ticks` ran out first), action_trace [ticks, n_envs, 5] (optional) for the ticks
// a replica ran and, in sampled mode only, every agent's epoch word += its replica's steps -- nothing else.  Replica
// groups in blockIdx order (a block writes 300 bytes per launch: the rollout's XCD-contiguous order has nothing to merge).
template <int H, int MAX_COORD>
__device__ __forceinline__ void gw5_evaluate(
    const int *states_x_arr, const int *states_y_arr, const float *obs_arr, double wall_hit_penalty,
    double tag_reward_for_tagger, double tag_penalty_for_runner, double step_cost_for_tagger, int use_full_observation,
    int world_boundary, const int *env_timestep_arr, int episode_length, int n_agents, int n_envs, uint32_t *rng_state,
    int stream_tag, int ticks, const int *action_table, const float *policy_tagger, const float *policy_runner,
    int use_argmax, float *eval_reward_sum, int *eval_steps, int *eval_done, int *action_trace, float *gw5_smem) {
  if (policy_tagger == nullptr || policy_runner == nullptr || n_agents != GW5_N || use_full_observation == 0 ||
      world_boundary < 0 || world_boundary > MAX_COORD || episode_length < 1)
    return;  // (uniform)
  float *const s_obs = gw5_smem;                                // [12][5][21] the block's observation image
  float *const s_div = s_obs + GW5_IMG;                         // [MAX_COORD + 1] c / L
  float *const s_tn = s_div + MAX_COORD + 1;                    // [episode_length + 1] t / episode_length
  float *const s_pol = s_tn + gw5_roundup4(episode_length + 1);  // [2][gw5_policy_floats(H)]: tagger, runner
  GW_REWARD_TABLE(wall_hit_penalty, tag_reward_for_tagger, tag_penalty_for_runner, step_cost_for_tagger);
  const int lane = threadIdx.x;                                 // (blocks are one wavefront)
  const int el = lane / GW5_N, ag = lane - el * GW5_N;          // local replica (12 = none), agent
  const uint32_t k0 = rng_state[0], k1 = rng_state[1];
  const bool greedy = use_argmax > 0;  // (uniform)
  int act_dx[5], act_dy[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) { act_dx[i] = action_table[2 * i]; act_dy[i] = action_table[2 * i + 1]; }
  {
    gw5_fill_coord_table<MAX_COORD>(s_div, lane, world_boundary);
    for (int q = lane; q <= episode_length; q += 64) s_tn[q] = (float)q / (float)episode_length;
    for (int q = lane; q < gw5_policy_floats(H); q += 64) {
      s_pol[q] = policy_tagger[q];
      s_pol[gw5_policy_floats(H) + q] = policy_runner[q];
    }
  }
  const float *const my_policy = s_pol + ((ag == GW5_N - 1) ? gw5_policy_floats(H) : 0);  // runner : tagger
  float *const rep = s_obs + min(el, GW5_EPB - 1) * GW5_ROW;  // this lane's replica's five rows
  const int runner_lane = min(el * GW5_N + GW5_N - 1, 63);

  for (int env0 = blockIdx.x * GW5_EPB; env0 < n_envs; env0 += gridDim.x * GW5_EPB) {
    const int env = env0 + el;
    const bool active = (el < GW5_EPB) && (env < n_envs);
    const int idx = env * GW5_N + ag;
    const int n_in = min(GW5_EPB, n_envs - env0) * GW5_ROW;
    const float *const obs_blk = obs_arr + (long)env0 * GW5_ROW;
    int x = 0, y = 0, t = 0;
    uint32_t epoch0 = 0u;
    if (active) {
      x = states_x_arr[idx];
      y = states_y_arr[idx];
      t = env_timestep_arr[env];
      epoch0 = rng_state[WD_RNG_HEADER + idx];
    }
    for (int q = lane; q < n_in; q += 64) s_obs[q] = obs_blk[q];  // the observation the first action is chosen on
    __syncthreads();
    // consumed HERE, before the tick loop (as in gw5_rollout: no wait for a load inside the loop)
    asm volatile("" : "+v"(x), "+v"(y), "+v"(t), "+v"(epoch0));
    wd_u4 blk = wd_u4{0u, 0u, 0u, 0u};  // the Philox block of four consecutive ticks (wd_tick_draw)
    uint32_t blk_quad = 0xffffffffu;
    bool live = active;
    float sum = 0.0f;
    int steps = 0;
    int *trace = action_trace ? action_trace + idx : nullptr;

    for (int k = 0; k < ticks; ++k) {
      if (__ballot(live) == 0ull) break;  // wave-uniform: every replica of the group has finished
      // the other lanes' image writes of the previous tick, before this tick's row reads: the language-level statement
      // of what holds anyway (LDS operations of one wavefront execute in issue order); as in gw5_rollout it compiles
      // to nothing -- the instruction stream is identical with and without it
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      bool hit = false;
      if (live) {
        float u = 0.0f;
        if (!greedy)  // the draw of tick k of T single-tick launches, as the rollout -- and, as there, BEFORE the network
          u = wd_u01_open_closed(wd_tick_draw((uint32_t)idx, epoch0 + (uint32_t)k, (uint32_t)stream_tag, k0, k1, blk,
                                              blk_quad));
        float prob[GW5_ACTIONS];
        gw5_policy_probs<H>(my_policy, rep + ag * GW5_F, prob);
        int a = 0;
        if (greedy) {
          a = rp_first_maximum(prob, GW5_ACTIONS);
        } else {
          float cum = 0.0f;
          int cnt = 0;
#pragma unroll
          for (int i = 0; i < GW5_ACTIONS; ++i) {
            cum = (i == 0) ? prob[0] : cum + prob[i];
            cnt += (cum < u) ? 1 : 0;
          }
          a = min(cnt, GW5_ACTIONS - 1);
        }
        if (trace) wd_store_untracked(trace + (long)k * n_envs * GW5_N, a);  // (untracked: the loop never reads it back)
        // ---- movement :152-173
        int ddx = act_dx[0], ddy = act_dy[0];
#pragma unroll
        for (int i = 1; i < 5; ++i) { ddx = (a == i) ? act_dx[i] : ddx; ddy = (a == i) ? act_dy[i] : ddy; }
        const int ux = x + ddx, uy = y + ddy;
        const int cx = min(max(ux, 0), world_boundary), cy = min(max(uy, 0), world_boundary);
        hit = (ux != cx) || (uy != cy);  // :163-170
        x = cx;
        y = cy;
        t += 1;  // :295
      }
      // ---- tag check :175-178 (all 64 lanes take part in the exchange; finished replicas are masked out of the result)
      const int cell = x | (y << 8);
      const int runner_cell = __shfl(cell, runner_lane);
      const unsigned long long on_runner = __ballot(live && (ag < GW5_N - 1) && (cell == runner_cell));
      const bool tag = ((unsigned)(on_runner >> (min(el, GW5_EPB - 1) * GW5_N)) & 0xfu) != 0u;
      if (live) {
        sum += GW_REWARD(ag < GW5_N - 1, tag, hit);
        steps += 1;
        // ---- the image: positions and time columns only (see gw5_rollout); a time step past the table (a start state
        // that was already timed out) finishes the replica on this tick and its image is not read again
        const float fx = s_div[x], fy = s_div[y];  // (clipped to 0 .. world_boundary <= MAX_COORD just above)
        const float tnorm = s_tn[min(max(t, 0), episode_length)];
#pragma unroll
        for (int i = 0; i < GW5_N; ++i) {
          rep[i * GW5_F + ag] = fx;
          rep[i * GW5_F + GW5_N + ag] = fy;
        }
        rep[ag * GW5_F + 4 * GW5_N] = tnorm;
        live = !((t >= episode_length) || tag);  // :314
      }
    }
    if (active) {
      eval_reward_sum[idx] = sum;
      if (!greedy) rng_state[WD_RNG_HEADER + idx] = epoch0 + (uint32_t)steps;
      if (ag == 0) {
        eval_steps[env] = steps;
        eval_done[env] = live ? 0 : 1;
      }
    }
    __syncthreads();  // (the next trip overwrites the image)
  }
}

}  // namespace

// the rollout entries' arguments: those of HipTagGridWorldRollout (tag_gridworld.hip) + the action table's address
#define GW5_PARAMS                                                                                                    \
  int *states_x_arr, int *states_y_arr, int *actions_arr, int *done_arr, float *rewards_arr, float *obs_arr,          \
      double wall_hit_penalty, double tag_reward_for_tagger, double tag_penalty_for_runner,                           \
      double step_cost_for_tagger, int use_full_observation, int world_boundary, int *env_timestep_arr,               \
      int episode_length, int n_agents, int n_envs, uint32_t *rng_state, const float *probs, int n_actions,           \
      const void *reset_table, int n_reset_arrays, int stream_tag, int ticks, float *obs_batch, int *action_batch,    \
      float *reward_batch, int *done_batch, int reset_cache_dwords, const int *action_table
#define GW5_ARGS                                                                                                      \
  states_x_arr, states_y_arr, actions_arr, done_arr, rewards_arr, obs_arr, wall_hit_penalty, tag_reward_for_tagger,   \
      tag_penalty_for_runner, step_cost_for_tagger, use_full_observation, world_boundary, env_timestep_arr,           \
      episode_length, n_agents, n_envs, rng_state, probs, n_actions, reset_table, n_reset_arrays, stream_tag, ticks,  \
      obs_batch, action_batch, reward_batch, done_batch, reset_cache_dwords, action_table

// the evaluation entries' arguments: the step's (read only; the kernel has no use for the action, done and reward
// arrays), then the generator state, the stream tag, the tick budget, the action table, the two packed policies, the
// mode, the three outputs and the optional action trace
#define GW5_EVALUATE_PARAMS                                                                                           \
  const int *states_x_arr, const int *states_y_arr, const int *actions_arr, const int *done_arr,                      \
      const float *rewards_arr, const float *obs_arr, double wall_hit_penalty, double tag_reward_for_tagger,          \
      double tag_penalty_for_runner, double step_cost_for_tagger, int use_full_observation, int world_boundary,       \
      const int *env_timestep_arr, int episode_length, int n_agents, int n_envs, uint32_t *rng_state, int stream_tag, \
      int ticks, const int *action_table, const float *policy_tagger, const float *policy_runner, int use_argmax,     \
      float *eval_reward_sum, int *eval_steps, int *eval_done, int *action_trace
#define GW5_EVALUATE_ARGS                                                                                             \
  states_x_arr, states_y_arr, obs_arr, wall_hit_penalty, tag_reward_for_tagger, tag_penalty_for_runner,               \
      step_cost_for_tagger, use_full_observation, world_boundary, env_timestep_arr, episode_length, n_agents, n_envs, \
      rng_state, stream_tag, ticks, action_table, policy_tagger, policy_runner, use_argmax, eval_reward_sum,          \
      eval_steps, eval_done, action_trace
