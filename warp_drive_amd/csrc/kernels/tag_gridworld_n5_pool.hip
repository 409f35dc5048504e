// tag_gridworld_n5_pool.hip -- the 5-agent TagGridWorld rollout of tag_gridworld_n5.hip for the env whose finished
// replicas restart from a random row of a RESET POOL (envs/tag_gridworld.py::CUDATagGridWorldWithResetPool, the
// reference's `tag_gridworld_with_reset_pool` config: one shared [32, 32] policy, grid_length 100).  Its own code
// object (csrc/wd_kernels_gw5_pool.hsaco): wd_kernels_gw5.hsaco stays the file it was, entry for entry and byte for
// byte, so the device functions both need are RESTATED here (as pg_update_gridworld.hip restates pg_update.hip's).
//
// Geometry, tick and recording are gw5_rollout's statement for statement -- blocks of ONE wavefront = 12 replicas, lane
// = (local replica, agent), replica groups dealt to the XCDs in contiguous ranges, the draw `wd_tick_draw(idx, epoch0 +
// k, stream_tag, ...)`, the network AFTER the draw, the counting draw, the move, the tag check by shuffle + ballot,
// GW_REWARD, untracked record stores, the image update.  Read the comments there; what DIFFERS:
//   * coordinates up to 255: the quotient table has 256 entries (GW5P_MAX_COORD), filled by a loop with the same float32
//     division `(float)c / (float)L`; the packed cell `x | y << 8` of the tag check already holds 255;
//   * a finished replica restarts from the pool row reset_when_done_from_pool (wd_core.hip) would draw: counter {env,
//     pool_epoch, 0x706f6f6c, 2} under the keys pool_rng[0], pool_rng[1], p = (rnd.x >> 8) * 2^-24, row = min((int)(p *
//     n_pool), n_pool - 1); x and y come from the SAME row of the two pools, t = 0.  `pool_epoch` is a per-lane register,
//     loaded once per replica group from pool_rng[WD_RNG_HEADER + env], incremented on a restart only, written back by
//     lane ag == 0 after the last tick.  The Philox call sits inside the wave-uniform `fm != 0` branch: a tick without a
//     finished replica executes none of it;
//   * both pools ([n_pool][5] int32 each) are copied to LDS once per launch, so the tick loop has no plain global load
//     (gw5_rollout's comment on the in-order memory counter: a wait for such a load would wait for the previous tick's
//     stores on every trip);
//   * the registered reset arrays of this env are exactly {observations}: the restore cache holds CD = 105 dwords per
//     replica, the observation rows of the START positions -- NOT of the pool row.  That is the reference's behaviour (its
//     placeholder is built once, at the first reset) and what oracle/tag_gridworld_np.py::reset_done_envs(x=, y=) models;
//   * after the last tick the launch writes positions, observations, time step, `_done_`, last rewards / actions, the
//     sampler's epoch words (+= ticks) and the pool epoch words.
//
// Dynamic LDS, in this order (host: envs/tag_gridworld.py::pool_rollout_lds_bytes, the same arithmetic), dwords:
//     observation image 12 * 105 | restore cache 12 * CD | coordinate quotients 256 | time table roundup4(episode_length
//     + 1) | the two pools 2 * roundup4(5 * n_pool) | the two packed policies 2 * gw5p_policy_floats(H)
// times 4 bytes, rounded up to 16.  Every part is a whole number of 16-byte vectors, so the policies start aligned.
//
// Entries: HipTagGridWorldRollout_N5P (fixed probabilities), _N5P_H32 / _N5P_H64 (live policies: pack_gridworld_policy's
// layout, two pointers -- a shared policy is passed twice), HipTagGridWorldEvaluate_N5P_H32 / _H64 (gw5_evaluate with
// only the wider table: evaluation has no restart, so it neither reads nor writes the pool; it takes the four pool
// arguments so that the two families are called alike).
#include "wd_common.h"
#include "tag_gridworld_rewards.h"

namespace {

struct Gw5pResetEntry {  // same layout as wd_reset_entry in wd_core.hip
  wd_global_u32 *data;
  const wd_global_u32 *ref;
  int row_elems;
  int pad_;
};

constexpr int GW5P_N = 5, GW5P_F = 21, GW5P_EPB = 12;
constexpr int GW5P_ROW = GW5P_N * GW5P_F;       // 105 floats: one replica's observation rows
constexpr int GW5P_IMG = GW5P_EPB * GW5P_ROW;   // 1260 floats: the block's observation image
constexpr int GW5P_MAX_COORD = 255;             // cells per axis - 1 the quotient table (and the packed cell) holds
constexpr int GW5P_IN_STRIDE = 24;              // floats per row of W0 (21 inputs + padding)
constexpr int GW5P_ACTIONS = 5;

// floats of one policy's packed weights, rounded up to whole 16-byte vectors (the second policy starts aligned)
__host__ __device__ constexpr int gw5p_policy_floats(int H) {
  return (H * GW5P_IN_STRIDE + H + H * H + H + GW5P_ACTIONS * H + GW5P_ACTIONS + 3) & ~3;
}

// the action probabilities of one agent: w = its policy's packed weights (LDS), x = its observation row (LDS, 21
// floats).  gw5_policy_probs of tag_gridworld_n5.hip restated: acc = bias, one fmaf per input in index order, ReLU,
// softmax with the maximum subtracted, expf, one division per action (oracle/tag_gridworld_np.py::policy_probabilities)
template <int H>
__device__ __forceinline__ void gw5p_policy_probs(const float *w, const float *x, float (&prob)[GW5P_ACTIONS]) {
  const float *W0 = w, *b0 = W0 + H * GW5P_IN_STRIDE, *W1 = b0 + H, *b1 = W1 + H * H, *Wp = b1 + H,
              *bp = Wp + GW5P_ACTIONS * H;
  float in[GW5P_F];
#pragma unroll
  for (int j = 0; j < GW5P_F; ++j) in[j] = x[j];
  float h1[H], h2[H];
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = b0[i];
#pragma unroll
    for (int j = 0; j < 20; j += 4) {
      const float4 wr = *(const float4 *)(W0 + i * GW5P_IN_STRIDE + j);
      acc = fmaf(wr.x, in[j], acc); acc = fmaf(wr.y, in[j + 1], acc);
      acc = fmaf(wr.z, in[j + 2], acc); acc = fmaf(wr.w, in[j + 3], acc);
    }
    acc = fmaf(W0[i * GW5P_IN_STRIDE + 20], in[20], acc);
    h1[i] = fmaxf(acc, 0.0f);
  }
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = b1[i];
#pragma unroll
    for (int j = 0; j < H; j += 4) {
      const float4 wr = *(const float4 *)(W1 + i * H + j);
      acc = fmaf(wr.x, h1[j], acc); acc = fmaf(wr.y, h1[j + 1], acc);
      acc = fmaf(wr.z, h1[j + 2], acc); acc = fmaf(wr.w, h1[j + 3], acc);
    }
    h2[i] = fmaxf(acc, 0.0f);
  }
  float logit[GW5P_ACTIONS], m = -__builtin_inff();
#pragma unroll
  for (int a = 0; a < GW5P_ACTIONS; ++a) {
    float acc = bp[a];
#pragma unroll
    for (int j = 0; j < H; j += 4) {
      const float4 wr = *(const float4 *)(Wp + a * H + j);
      acc = fmaf(wr.x, h2[j], acc); acc = fmaf(wr.y, h2[j + 1], acc);
      acc = fmaf(wr.z, h2[j + 2], acc); acc = fmaf(wr.w, h2[j + 3], acc);
    }
    logit[a] = acc;
    m = fmaxf(m, acc);
  }
  float e[GW5P_ACTIONS], sum = 0.0f;
#pragma unroll
  for (int a = 0; a < GW5P_ACTIONS; ++a) {
    e[a] = expf(logit[a] - m);
    sum += e[a];
  }
#pragma unroll
  for (int a = 0; a < GW5P_ACTIONS; ++a) prob[a] = e[a] / sum;
}

// their running float32 sums (gw5_policy_cum: the last sum repeated up to eight entries)
template <int H>
__device__ __forceinline__ void gw5p_policy_cum(const float *w, const float *x, float (&cumv)[8]) {
  float prob[GW5P_ACTIONS];
  gw5p_policy_probs<H>(w, x, prob);
  float cum = 0.0f;
#pragma unroll
  for (int a = 0; a < 8; ++a) {
    if (a < GW5P_ACTIONS) cum = (a == 0) ? prob[0] : cum + prob[a];
    cumv[a] = cum;
  }
}

__device__ __forceinline__ int gw5p_roundup4(int n) { return (n + 3) & ~3; }

// H = 0: fixed probabilities (`probs`); H = 32 / 64: the live policies
template <int H>
__device__ __forceinline__ void gw5p_rollout(
    int *states_x_arr, int *states_y_arr, int *actions_arr, int *done_arr, float *rewards_arr, float *obs_arr,
    double wall_hit_penalty, double tag_reward_for_tagger, double tag_penalty_for_runner, double step_cost_for_tagger,
    int use_full_observation, int world_boundary, int *env_timestep_arr, int episode_length, int n_agents, int n_envs,
    uint32_t *rng_state, const float *probs, int n_actions, const void *reset_table, int n_reset_arrays,
    int stream_tag, int ticks, float *obs_batch, int *action_batch, float *reward_batch, int *done_batch,
    int reset_cache_dwords, const int *action_table, const float *policy_tagger, const float *policy_runner,
    uint32_t *pool_rng, const int *pool_x, const int *pool_y, int n_pool, float *gw5_smem) {
  // (uniform) shapes the tables below are not sized for: the host admits none of them
  if (n_agents != GW5P_N || use_full_observation == 0 || world_boundary < 0 || world_boundary > GW5P_MAX_COORD ||
      episode_length < 1 || n_pool < 1 || reset_cache_dwords < GW5P_ROW || pool_rng == nullptr)
    return;
  const int CD = reset_cache_dwords;                        // dwords per replica in the restore cache
  float *const s_obs = gw5_smem;                            // [12][5][21] the block's observation image (16-byte aligned)
  uint32_t *const s_cache = (uint32_t *)(s_obs + GW5P_IMG); // [12][CD] the rows finished replicas are restored from
  float *const s_div = (float *)(s_cache + GW5P_EPB * CD);  // [256] c / L
  float *const s_tn = s_div + GW5P_MAX_COORD + 1;           // [episode_length + 1] t / episode_length
  const int pool_dwords = gw5p_roundup4(GW5P_N * n_pool);
  int *const s_pool_x = (int *)(s_tn + gw5p_roundup4(episode_length + 1));  // [n_pool][5]
  int *const s_pool_y = s_pool_x + pool_dwords;                            // [n_pool][5]
  // the two policies' packed weights behind the tables, on a 16-byte boundary (host: the same arithmetic)
  float *const s_pol = (float *)(s_pool_y + pool_dwords);   // [2][gw5p_policy_floats(H)]: tagger, runner
  GW_REWARD_TABLE(wall_hit_penalty, tag_reward_for_tagger, tag_penalty_for_runner, step_cost_for_tagger);
  const int lane = threadIdx.x;                             // (blocks are one wavefront)
  const int el = lane / GW5P_N, ag = lane - el * GW5P_N;    // local replica (12 = none), agent
  const Gw5pResetEntry *const table = (const Gw5pResetEntry *)reset_table;
  const uint32_t k0 = rng_state[0], k1 = rng_state[1];
  const uint32_t pk0 = pool_rng[0], pk1 = pool_rng[1];
  int act_dx[5], act_dy[5];  // the action table, once per launch (scalar registers)
#pragma unroll
  for (int i = 0; i < 5; ++i) { act_dx[i] = action_table[2 * i]; act_dy[i] = action_table[2 * i + 1]; }
  {  // every quotient a tick can need, computed with the division the reference's expression compiles to
    const float L = (float)world_boundary;
    for (int q = lane; q <= world_boundary; q += 64) s_div[q] = (float)q / L;
    for (int q = lane; q <= episode_length; q += 64) s_tn[q] = (float)q / (float)episode_length;
    for (int q = lane; q < GW5P_N * n_pool; q += 64) {
      s_pool_x[q] = pool_x[q];
      s_pool_y[q] = pool_y[q];
    }
    if constexpr (H > 0) {
      for (int q = lane; q < gw5p_policy_floats(H); q += 64) {
        s_pol[q] = policy_tagger[q];
        s_pol[gw5p_policy_floats(H) + q] = policy_runner[q];
      }
    }
  }

  // each XCD gets a contiguous range of replica groups (gw5_rollout: the record rows of neighbouring groups share
  // cache lines, which only one XCD's L2 can merge); a bijection of [0, gridDim.x) for any grid size
  const int xcd = blockIdx.x & 7, nq = gridDim.x >> 3, nr = gridDim.x & 7;
  const int group0 = xcd * nq + min(xcd, nr) + (blockIdx.x >> 3);
  for (int env0 = group0 * GW5P_EPB; env0 < n_envs; env0 += gridDim.x * GW5P_EPB) {
    const int env = env0 + el;
    const bool active = (el < GW5P_EPB) && (env < n_envs);
    const int idx = env * GW5P_N + ag;
    const int envs_here = min(GW5P_EPB, n_envs - env0);
    const int n_out = envs_here * GW5P_ROW;
    float *const obs_blk = obs_arr + (long)env0 * GW5P_ROW;
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
      pool_epoch = pool_rng[WD_RNG_HEADER + env];
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
    // the rows finished replicas are restored from: per registered array one flat, coalesced copy of the block's rows
    // (this env registers the observations alone; an array that is not the observations only takes its room)
    int off_obs = 0;
    {
      int off = 0;
      for (int r = 0; r < n_reset_arrays; ++r) {
        const Gw5pResetEntry ent = table[r];
        const int re = ent.row_elems;
        if (off + re > CD) break;  // (never: CD is the sum of the rows; the cache is not written past a replica's share)
        if ((size_t)ent.data == (size_t)obs_arr) off_obs = off;
        const wd_global_u32 *const src = ent.ref + (long)env0 * re;
        const float inv_re = 1.0f / (float)re;
        for (int q = lane; q < envs_here * re; q += 64) {
          const int e = min((int)(((float)q + 0.5f) * inv_re), envs_here - 1);  // q / re (exact for these sizes)
          s_cache[e * CD + off + (q - e * re)] = src[q];
        }
        off += re;
      }
    }
    __syncthreads();
    // every value loaded above is consumed HERE, not inside the tick loop (gw5_rollout: the memory counter returns in order)
    asm volatile("" : "+v"(x), "+v"(y), "+v"(t), "+v"(epoch0), "+v"(pool_epoch));
    if constexpr (H == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(cumv[i]));
    }
    const float *const my_policy = s_pol + ((ag == GW5P_N - 1) ? gw5p_policy_floats(H) : 0);  // runner : tagger
    float last_reward = 0.0f;
    int last_action = 0, last_done = 0;
    float *const rep = s_obs + min(el, GW5P_EPB - 1) * GW5P_ROW;  // this lane's replica's five rows
    const int runner_lane = min(el * GW5P_N + GW5P_N - 1, 63);

    for (int k = 0; k < ticks; ++k) {
      if constexpr (H == 0) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      // ---- record the observation of this tick (flat, coalesced; none of the record stores is tracked)
      float *const brow = obs_batch + ((long)k * n_envs + env0) * GW5P_ROW;
      if ((((size_t)brow & 15) | (size_t)(n_out & 3)) == 0) {  // block-uniform
        const int nvec = n_out >> 2;  // 315 for a full block
        const float4 *const img4 = (const float4 *)s_obs;
        float4 v[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) v[i] = img4[min(lane + 64 * i, GW5P_IMG / 4 - 1)];  // (clamped into the image)
#pragma unroll
        for (int i = 0; i < 5; ++i)
          if (lane + 64 * i < nvec) wd_store_untracked((float4 *)brow + lane + 64 * i, v[i]);
      } else {
        for (int q = lane; q < n_out; q += 64) wd_store_untracked(brow + q, s_obs[q]);
      }
      bool hit = false;
      int a = 0;
      if (active) {
        const int n_act = (H > 0) ? GW5P_ACTIONS : n_actions;
        // ---- sample (random.cu:51-85), the draw of tick k of T single-tick launches
        const float u = wd_u01_open_closed(wd_tick_draw((uint32_t)idx, epoch0 + (uint32_t)k, (uint32_t)stream_tag, k0, k1,
                                                        blk, blk_quad));
        // the LIVE policy on this tick's observation row, AFTER the draw (gw5_rollout: in front of it the scheduler
        // hoists the network's LDS operand reads over the whole block and the allocator spills)
        if constexpr (H > 0) gw5p_policy_cum<H>(my_policy, rep + ag * GW5P_F, cumv);
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) cnt += (i < n_act && cumv[i] < u) ? 1 : 0;
        a = min(cnt, n_act - 1);
        wd_store_untracked(action_batch + ((long)k * n_envs * GW5P_N + idx), a);
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
      const unsigned long long on_runner = __ballot(active && (ag < GW5P_N - 1) && (cell == runner_cell));
      const bool tag = ((unsigned)(on_runner >> (min(el, GW5P_EPB - 1) * GW5P_N)) & 0xfu) != 0u;
      const bool fin = active && ((t >= episode_length) || tag);  // :314
      if (active) {
        if (ag == 0) wd_store_untracked(done_batch + ((long)k * n_envs + env), fin ? 1 : 0);
        last_done = fin ? 1 : 0;
        last_reward = GW_REWARD(ag < GW5P_N - 1, tag, hit);
        wd_store_untracked(reward_batch + ((long)k * n_envs * GW5P_N + idx), last_reward);
        last_action = a;
        // ---- the image: positions and time columns only.  x, y were clipped to 0 .. world_boundary <= 255 just
        // above; a time step past the table (a start state that was already timed out) finishes the replica on this
        // tick, and its rows are restored below before anyone reads them
        const float fx = s_div[x], fy = s_div[y], tnorm = s_tn[min(max(t, 0), episode_length)];
#pragma unroll
        for (int i = 0; i < GW5P_N; ++i) {
          rep[i * GW5P_F + ag] = fx;
          rep[i * GW5P_F + GW5P_N + ag] = fy;
        }
        rep[ag * GW5P_F + 4 * GW5P_N] = tnorm;
      }
      // ---- restart finished replicas: register and LDS copies only
      unsigned long long fm = __ballot(fin);  // wave-uniform
      if (fm == 0ull) continue;
      if (fin) {
        // the row reset_when_done_from_pool draws for this replica at this epoch (its five lanes compute the same one)
        const wd_u4 rnd = wd_philox4x32_10(wd_u4{(uint32_t)env, pool_epoch, 0x706f6f6cu, 2u}, pk0, pk1);
        const float p = (float)(rnd.x >> 8) * 0x1.0p-24f;
        const int ref_id = min((int)(p * (float)n_pool), n_pool - 1);
        x = s_pool_x[ref_id * GW5P_N + ag];
        y = s_pool_y[ref_id * GW5P_N + ag];
        t = 0;
        pool_epoch += 1u;
      }
      while (fm != 0ull) {
        const int e = ((__ffsll((long long)fm) - 1) * 13) >> 6;  // lane / 5 for lanes < 64
        fm &= ~(0x1full << (e * GW5P_N));
        for (int q = lane; q < GW5P_ROW; q += 64) s_obs[e * GW5P_ROW + q] = __uint_as_float(s_cache[e * CD + off_obs + q]);
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
        pool_rng[WD_RNG_HEADER + env] = pool_epoch;
      }
    }
    for (int q = lane; q < n_out; q += 64) obs_blk[q] = s_obs[q];
    __syncthreads();  // (the next trip overwrites the image and the cache)
  }
}

// One episode of every replica with the two policies inside the kernel: gw5_evaluate of tag_gridworld_n5.hip with the
// 256-entry quotient table (read its comment for what is written and what is not).  No restart, so no pool.
template <int H>
__device__ __forceinline__ void gw5p_evaluate(
    const int *states_x_arr, const int *states_y_arr, const float *obs_arr, double wall_hit_penalty,
    double tag_reward_for_tagger, double tag_penalty_for_runner, double step_cost_for_tagger, int use_full_observation,
    int world_boundary, const int *env_timestep_arr, int episode_length, int n_agents, int n_envs, uint32_t *rng_state,
    int stream_tag, int ticks, const int *action_table, const float *policy_tagger, const float *policy_runner,
    int use_argmax, float *eval_reward_sum, int *eval_steps, int *eval_done, int *action_trace, float *gw5_smem) {
  if (policy_tagger == nullptr || policy_runner == nullptr || n_agents != GW5P_N || use_full_observation == 0 ||
      world_boundary < 0 || world_boundary > GW5P_MAX_COORD || episode_length < 1)
    return;  // (uniform)
  float *const s_obs = gw5_smem;                                // [12][5][21] the block's observation image
  float *const s_div = s_obs + GW5P_IMG;                        // [256] c / L
  float *const s_tn = s_div + GW5P_MAX_COORD + 1;               // [episode_length + 1] t / episode_length
  float *const s_pol = s_tn + gw5p_roundup4(episode_length + 1);  // [2][gw5p_policy_floats(H)]: tagger, runner
  GW_REWARD_TABLE(wall_hit_penalty, tag_reward_for_tagger, tag_penalty_for_runner, step_cost_for_tagger);
  const int lane = threadIdx.x;                                 // (blocks are one wavefront)
  const int el = lane / GW5P_N, ag = lane - el * GW5P_N;        // local replica (12 = none), agent
  const uint32_t k0 = rng_state[0], k1 = rng_state[1];
  const bool greedy = use_argmax > 0;  // (uniform)
  int act_dx[5], act_dy[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) { act_dx[i] = action_table[2 * i]; act_dy[i] = action_table[2 * i + 1]; }
  {
    const float L = (float)world_boundary;
    for (int q = lane; q <= world_boundary; q += 64) s_div[q] = (float)q / L;
    for (int q = lane; q <= episode_length; q += 64) s_tn[q] = (float)q / (float)episode_length;
    for (int q = lane; q < gw5p_policy_floats(H); q += 64) {
      s_pol[q] = policy_tagger[q];
      s_pol[gw5p_policy_floats(H) + q] = policy_runner[q];
    }
  }
  const float *const my_policy = s_pol + ((ag == GW5P_N - 1) ? gw5p_policy_floats(H) : 0);  // runner : tagger
  float *const rep = s_obs + min(el, GW5P_EPB - 1) * GW5P_ROW;  // this lane's replica's five rows
  const int runner_lane = min(el * GW5P_N + GW5P_N - 1, 63);

  for (int env0 = blockIdx.x * GW5P_EPB; env0 < n_envs; env0 += gridDim.x * GW5P_EPB) {
    const int env = env0 + el;
    const bool active = (el < GW5P_EPB) && (env < n_envs);
    const int idx = env * GW5P_N + ag;
    const int n_in = min(GW5P_EPB, n_envs - env0) * GW5P_ROW;
    const float *const obs_blk = obs_arr + (long)env0 * GW5P_ROW;
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
    // consumed HERE, before the tick loop (as in the rollout: no wait for a load inside the loop)
    asm volatile("" : "+v"(x), "+v"(y), "+v"(t), "+v"(epoch0));
    wd_u4 blk = wd_u4{0u, 0u, 0u, 0u};  // the Philox block of four consecutive ticks (wd_tick_draw)
    uint32_t blk_quad = 0xffffffffu;
    bool live = active;
    float sum = 0.0f;
    int steps = 0;
    int *trace = action_trace ? action_trace + idx : nullptr;

    for (int k = 0; k < ticks; ++k) {
      if (__ballot(live) == 0ull) break;  // wave-uniform: every replica of the group has finished
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      bool hit = false;
      if (live) {
        float u = 0.0f;
        if (!greedy)  // the draw of tick k of T single-tick launches, as the rollout -- and, as there, BEFORE the network
          u = wd_u01_open_closed(wd_tick_draw((uint32_t)idx, epoch0 + (uint32_t)k, (uint32_t)stream_tag, k0, k1, blk,
                                              blk_quad));
        float prob[GW5P_ACTIONS];
        gw5p_policy_probs<H>(my_policy, rep + ag * GW5P_F, prob);
        int a = 0;
        if (greedy) {
          float best = prob[0];
#pragma unroll
          for (int i = 1; i < GW5P_ACTIONS; ++i) {
            const bool better = best < prob[i];
            best = better ? prob[i] : best;
            a = better ? i : a;
          }
        } else {
          float cum = 0.0f;
          int cnt = 0;
#pragma unroll
          for (int i = 0; i < GW5P_ACTIONS; ++i) {
            cum = (i == 0) ? prob[0] : cum + prob[i];
            cnt += (cum < u) ? 1 : 0;
          }
          a = min(cnt, GW5P_ACTIONS - 1);
        }
        if (trace) wd_store_untracked(trace + (long)k * n_envs * GW5P_N, a);  // (untracked: the loop never reads it back)
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
      const unsigned long long on_runner = __ballot(live && (ag < GW5P_N - 1) && (cell == runner_cell));
      const bool tag = ((unsigned)(on_runner >> (min(el, GW5P_EPB - 1) * GW5P_N)) & 0xfu) != 0u;
      if (live) {
        sum += GW_REWARD(ag < GW5P_N - 1, tag, hit);
        steps += 1;
        const float fx = s_div[x], fy = s_div[y];  // (clipped to 0 .. world_boundary <= 255 just above)
        const float tnorm = s_tn[min(max(t, 0), episode_length)];
#pragma unroll
        for (int i = 0; i < GW5P_N; ++i) {
          rep[i * GW5P_F + ag] = fx;
          rep[i * GW5P_F + GW5P_N + ag] = fy;
        }
        rep[ag * GW5P_F + 4 * GW5P_N] = tnorm;
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

// the arguments of HipTagGridWorldRollout_N5 (tag_gridworld_n5.hip)
#define GW5P_PARAMS                                                                                                   \
  int *states_x_arr, int *states_y_arr, int *actions_arr, int *done_arr, float *rewards_arr, float *obs_arr,          \
      double wall_hit_penalty, double tag_reward_for_tagger, double tag_penalty_for_runner,                           \
      double step_cost_for_tagger, int use_full_observation, int world_boundary, int *env_timestep_arr,               \
      int episode_length, int n_agents, int n_envs, uint32_t *rng_state, const float *probs, int n_actions,           \
      const void *reset_table, int n_reset_arrays, int stream_tag, int ticks, float *obs_batch, int *action_batch,    \
      float *reward_batch, int *done_batch, int reset_cache_dwords, const int *action_table
#define GW5P_ARGS                                                                                                     \
  states_x_arr, states_y_arr, actions_arr, done_arr, rewards_arr, obs_arr, wall_hit_penalty, tag_reward_for_tagger,   \
      tag_penalty_for_runner, step_cost_for_tagger, use_full_observation, world_boundary, env_timestep_arr,           \
      episode_length, n_agents, n_envs, rng_state, probs, n_actions, reset_table, n_reset_arrays, stream_tag, ticks,  \
      obs_batch, action_batch, reward_batch, done_batch, reset_cache_dwords, action_table
// ... then the pool: the resetter's generator words, the two pools [n_pool][5], their row count
#define GW5P_POOL_PARAMS uint32_t *pool_rng, const int *pool_x, const int *pool_y, int n_pool

extern "C" __global__ void __launch_bounds__(64) HipTagGridWorldRollout_N5P(GW5P_PARAMS, GW5P_POOL_PARAMS) {
  extern __shared__ __attribute__((aligned(16))) float gw5_smem[];
  gw5p_rollout<0>(GW5P_ARGS, nullptr, nullptr, pool_rng, pool_x, pool_y, n_pool, gw5_smem);
}
#define GW5P_POLICY_ENTRY(HH)                                                                                         \
  extern "C" __global__ void __launch_bounds__(64) HipTagGridWorldRollout_N5P_H##HH(                                  \
      GW5P_PARAMS, const float *policy_tagger, const float *policy_runner, GW5P_POOL_PARAMS) {                        \
    extern __shared__ __attribute__((aligned(16))) float gw5_smem[];                                                  \
    if (policy_tagger == nullptr || policy_runner == nullptr) return;                                                 \
    gw5p_rollout<HH>(GW5P_ARGS, policy_tagger, policy_runner, pool_rng, pool_x, pool_y, n_pool, gw5_smem);            \
  }
GW5P_POLICY_ENTRY(32)
GW5P_POLICY_ENTRY(64)

// the arguments of HipTagGridWorldEvaluate_N5_H<width>, then the pool's four (unused: an evaluation never restarts).
// Dynamic LDS: the image, 256 coordinate quotients, the time table rounded up to 16 bytes, 2 * gw5p_policy_floats(H)
// floats (envs/tag_gridworld.py::pool_rollout_lds_bytes with no cache and no pool)
#define GW5P_EVALUATE_ENTRY(HH)                                                                                       \
  extern "C" __global__ void __launch_bounds__(64) HipTagGridWorldEvaluate_N5P_H##HH(                                 \
      const int *states_x_arr, const int *states_y_arr, const int *actions_arr, const int *done_arr,                  \
      const float *rewards_arr, const float *obs_arr, double wall_hit_penalty, double tag_reward_for_tagger,          \
      double tag_penalty_for_runner, double step_cost_for_tagger, int use_full_observation, int world_boundary,       \
      const int *env_timestep_arr, int episode_length, int n_agents, int n_envs, uint32_t *rng_state, int stream_tag, \
      int ticks, const int *action_table, const float *policy_tagger, const float *policy_runner, int use_argmax,     \
      float *eval_reward_sum, int *eval_steps, int *eval_done, int *action_trace, const uint32_t *pool_rng,           \
      const int *pool_x, const int *pool_y, int n_pool) {                                                             \
    extern __shared__ __attribute__((aligned(16))) float gw5_smem[];                                                  \
    gw5p_evaluate<HH>(states_x_arr, states_y_arr, obs_arr, wall_hit_penalty, tag_reward_for_tagger,                   \
                      tag_penalty_for_runner, step_cost_for_tagger, use_full_observation, world_boundary,             \
                      env_timestep_arr, episode_length, n_agents, n_envs, rng_state, stream_tag, ticks, action_table, \
                      policy_tagger, policy_runner, use_argmax, eval_reward_sum, eval_steps, eval_done, action_trace, \
                      gw5_smem);                                                                                      \
  }
GW5P_EVALUATE_ENTRY(32)
GW5P_EVALUATE_ENTRY(64)
