// wd_env_rollout.h -- the kit for a ONE-LAUNCH ROLLOUT of a custom environment with the POLICY INSIDE THE KERNEL: for
// `ticks` ticks in a row every agent's thread evaluates the small policy network on its own observation row, draws its
// action, the author's step runs, the tick's batch rows are recorded and finished replicas restart -- a whole training
// batch in ONE launch (docs/custom_environments.md, "A policy inside the kernel").
//
// Self-contained like wd_env_tick.h, which it includes: <hip/hip_runtime.h>, <stdint.h>, <math.h>, nothing of the
// package's own kernel sources.  The network, the running sums and the pick form a section that a plain host compiler
// builds as well (no HIP header is read when __HIPCC__ is not defined): a host program can print what a kernel will
// compute (tests/c/rollout_policy_check.cpp).
//
// How an author uses it.  The step is the `__device__ __forceinline__` function of the fused tick (wd_env_tick.h).  The
// hidden width H and the observation size F are compile-time; one template serves the two entries
// `Hip<Name>Rollout_H32` and `Hip<Name>Rollout_H64`, whose parameters are the step's own followed by WD_ROLLOUT_PARAMS:
//
//     WD_ROLLOUT_KIT(kit);                                  // the trailing parameters as one struct
//     WD_ROLLOUT_WEIGHTS(wd_rollout_w);                     // extern __shared__ float wd_rollout_w[], 16-byte aligned
//     wd_rollout_stage<H, F>(kit, wd_rollout_w);            // packed policy -> LDS, once per launch, one barrier
//     for (int k = 0; k < ticks; ++k) {
//       wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
//       const int a = wd_rollout_act<H, F>(kit, wd_rollout_w, obs_arr, env, agent, n_agents, k, actions_arr);
//       my_step(..., a, ...);
//       wd_rollout_end(kit, k, done_arr, env_timestep_arr, rewards_arr, env, agent, n_agents);
//     }
//
// Geometry: the kit's.  One block per replica, one thread per agent, ceil(N / 64) * 64 threads; EVERY thread of the block
// calls every kit function, in uniform control flow.  E, the number of replicas, is gridDim.x.
//
// Trailing parameters (WD_ROLLOUT_PARAMS), in this order -- warp_drive_amd/utils/custom_tick.py::custom_rollout_launch
// packs exactly these; pointers and 32-bit scalars only:
//     uint32_t *rng_state      the sampler's state, as in wd_env_tick.h
//     const float *policy      the packed weights (below)
//     int n_actions            A, 1 .. WD_ROLLOUT_MAX_ACTIONS (8)
//     const void *reset_table  wd_tick_reset_entry[reset_entries]
//     int reset_entries
//     int stream_tag           counter word 2 of the draw
//     float *obs_batch         [T, E, N, F]   row k: the observation tick k's action was drawn on
//     int *action_batch        [T, E, N, 1]   row k: tick k's actions
//     float *reward_batch      [T, E, N]      row k: the rewards tick k's step stored
//     int *done_batch          [T, E]         row k: the done flag behind tick k's step
//     int ticks                LAST, as in WD_TICK_PARAMS; ticks <= T
// All batch indexing is 64-bit.
//
// PACKED WEIGHTS (training/policy_kernel.py::pack_rollout_policy), float32, unpadded, in this order:
//     W0 [H][F], b0 [H], W1 [H][H], b1 [H], Wp [A][H], bp [A]                    wd_rollout_policy_floats(F, H, A)
// The launch asks for 4 bytes of dynamic LDS per float, rounded up to 16.
//
// PARITY CONTRACT (what a host restatement reproduces; tests/custom_rollout_model.py is one):
//   * every unit: acc = bias, then ONE fmaf per input in index order (float32); ReLU as fmaxf(acc, 0) -- C's fmaxf, which
//     returns the other operand for a NaN: a NaN activation (non-finite weights) becomes 0, on the device and in a host
//     build alike, where numpy's maximum hands the NaN on; the contract is stated for finite weights, and whatever the
//     sums are, the pick stays in [0, A);
//   * softmax: the logits as above, their maximum subtracted, expf, the sum of the terms in action order starting from
//     0, ONE division e[a] / sum per action;
//   * running sums: cum = p[0], then cum + p[a] in action order;
//   * the draw is wd_env_tick.h's, unchanged: row = env * N + agent reads its epoch e = rng_state[4 + row], stores e + 1,
//     makes ONE Philox4x32-10 call with counter (row, e, stream_tag, 5), takes word x through wd_tick_uniform; the action
//     is the number of running sums < u, clamped to A - 1.
// The weights are read from LDS, every lane the same address (a broadcast); the activations are registers; every loop
// is fully unrolled, so nothing is indexed at run time (no scratch memory).  No inline assembly, no atomics, no
// cross-thread float reductions.
//
// REGISTERS.  A block of 1024 threads leaves 128 VGPRs per lane.  H = 32 fits; H = 64 holds two arrays of 64 activations
// next to the observation and does not.  Every entry therefore carries __launch_bounds__ (1024 for _H32, 512 for _H64
// in the worked example), and the host never launches a block over an entry's bound (FusedRolloutMixin.ROLLOUT_MAX_THREADS).
//
// WHAT ORDERS THE OBSERVATION READS BETWEEN TICKS.  wd_rollout_act reads the row of `obs_arr` the PREVIOUS tick's step (or
// restart) stored.  A row is read back by the same block that wrote it, behind the two barriers of wd_rollout_end (each
// also a memory fence over the block): what the step stored is visible to the restart, what the restart stored -- by
// whichever thread -- is visible to the next tick's read.  wd_rollout_end records `rewards_arr[row]` BEFORE the restart
// restores anything, as an author may have registered `rewards` for reset (create_and_push_data_placeholders and Trainer
// register it WITHOUT a reset copy; an author who pushes the placeholders by hand may give it one): the restart copies
// element i of a row with thread i, so the thread that restores an agent's reward is the thread that has just recorded
// it.  The notes of
// wd_env_tick.h on `__restrict__` and on hand-overs through global memory within a tick hold here as well.
#ifndef WD_ENV_ROLLOUT_H_
#define WD_ENV_ROLLOUT_H_

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#include "wd_env_tick.h"

#define WD_ROLLOUT_MAX_ACTIONS 8

// every loop over units, inputs and actions is fully unrolled on the device (a host compiler is left to itself)
#ifdef __HIPCC__
#define WD_ROLLOUT_UNROLL _Pragma("unroll")
#else
#define WD_ROLLOUT_UNROLL
#endif

// =============================================================================== host and device
constexpr int wd_rollout_policy_floats(int F, int H, int A) { return F * H + H + H * H + H + A * H + A; }

struct wd_rollout_f4 {
  float x, y, z, w;
};

// four consecutive weights; `p` is 16-byte aligned (W1, Wp and every row of them are, for H a multiple of 4, when the
// staged array is)
WD_TICK_HD wd_rollout_f4 wd_rollout_load4(const float *p) {
#ifdef __HIPCC__
  const float4 v = *(const float4 *)p;
  const wd_rollout_f4 r = {v.x, v.y, v.z, v.w};
#else
  const wd_rollout_f4 r = {p[0], p[1], p[2], p[3]};
#endif
  return r;
}

// one layer of H units over H inputs, rows of H floats: acc = bias, one fmaf per input in index order
template <int H>
WD_TICK_HD float wd_rollout_unit(const float *row, float bias, const float (&in)[H]) {
  float acc = bias;
WD_ROLLOUT_UNROLL
  for (int j = 0; j < H; j += 4) {
    const wd_rollout_f4 wr = wd_rollout_load4(row + j);
    acc = fmaf(wr.x, in[j], acc);
    acc = fmaf(wr.y, in[j + 1], acc);
    acc = fmaf(wr.z, in[j + 2], acc);
    acc = fmaf(wr.w, in[j + 3], acc);
  }
  return acc;
}

// the logits of observation `obs` under the packed weights `w` (-inf at and past n_actions); returns their maximum
template <int H, int F>
WD_TICK_HD float wd_rollout_logits(const float *w, const float (&obs)[F], int n_actions,
                                   float (&logit)[WD_ROLLOUT_MAX_ACTIONS]) {
  static_assert(H % 4 == 0 && H >= 4 && F >= 1, "the rows of W1 and of the head are read four floats at a time");
  const float *W0 = w, *b0 = W0 + F * H, *W1 = b0 + H, *b1 = W1 + H * H, *Wp = b1 + H, *bp = Wp + n_actions * H;
  float h1[H], h2[H];
WD_ROLLOUT_UNROLL
  for (int i = 0; i < H; ++i) {
    float acc = b0[i];
WD_ROLLOUT_UNROLL
    for (int j = 0; j < F; ++j) acc = fmaf(W0[i * F + j], obs[j], acc);
    h1[i] = fmaxf(acc, 0.0f);
  }
WD_ROLLOUT_UNROLL
  for (int i = 0; i < H; ++i) h2[i] = fmaxf(wd_rollout_unit<H>(W1 + i * H, b1[i], h1), 0.0f);
  float m = -INFINITY;
WD_ROLLOUT_UNROLL
  for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) {
    logit[a] = -INFINITY;
    if (a < n_actions) {
      logit[a] = wd_rollout_unit<H>(Wp + a * H, bp[a], h2);
      m = fmaxf(m, logit[a]);
    }
  }
  return m;
}

// the running sums of the softmax of the logits: cum[a] for a < n_actions, the last value repeated behind them
WD_TICK_HD void wd_rollout_running_sums(const float (&logit)[WD_ROLLOUT_MAX_ACTIONS], float m, int n_actions,
                                        float (&cum)[WD_ROLLOUT_MAX_ACTIONS]) {
  float e[WD_ROLLOUT_MAX_ACTIONS], sum = 0.0f;
WD_ROLLOUT_UNROLL
  for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) {
    e[a] = (a < n_actions) ? expf(logit[a] - m) : 0.0f;
    sum += e[a];
  }
  float run = 0.0f;
WD_ROLLOUT_UNROLL
  for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) {
    const float p = e[a] / sum;
    if (a < n_actions) run = (a == 0) ? p : run + p;
    cum[a] = run;
  }
}

// the action: how many of the first n_actions running sums are < u, clamped to n_actions - 1
WD_TICK_HD int wd_rollout_pick(const float (&cum)[WD_ROLLOUT_MAX_ACTIONS], int n_actions, float u) {
  int cnt = 0;
WD_ROLLOUT_UNROLL
  for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) cnt += (a < n_actions && cum[a] < u) ? 1 : 0;
  return cnt < n_actions - 1 ? cnt : n_actions - 1;
}

// =============================================================================== device only
#ifdef __HIPCC__

// the trailing parameters of a Rollout entry, after the step's own (the order is the contract: see the top of the file)
#define WD_ROLLOUT_PARAMS                                                                                          \
  uint32_t *wd_rollout_rng_state_, const float *wd_rollout_policy_, int wd_rollout_n_actions_,                    \
      const void *wd_rollout_reset_table_, int wd_rollout_reset_entries_, int wd_rollout_stream_tag_,             \
      float *wd_rollout_obs_batch_, int *wd_rollout_action_batch_, float *wd_rollout_reward_batch_,               \
      int *wd_rollout_done_batch_, int ticks

struct wd_rollout_kit {
  uint32_t *rng_state;
  const float *policy;
  int n_actions;
  const wd_tick_reset_entry *reset_table;
  int reset_entries;
  uint32_t stream_tag;
  float *obs_batch;
  int *action_batch;
  float *reward_batch;
  int *done_batch;
};

// gathers the trailing parameters into `const wd_rollout_kit name`
#define WD_ROLLOUT_KIT(name)                                                                                       \
  const wd_rollout_kit name = {wd_rollout_rng_state_, wd_rollout_policy_, wd_rollout_n_actions_,                  \
                               (const wd_tick_reset_entry *)wd_rollout_reset_table_, wd_rollout_reset_entries_,   \
                               (uint32_t)wd_rollout_stream_tag_, wd_rollout_obs_batch_, wd_rollout_action_batch_, \
                               wd_rollout_reward_batch_, wd_rollout_done_batch_}

// the dynamic LDS the packed policy is staged into: 16-byte aligned, whatever static LDS the entry declares
#define WD_ROLLOUT_WEIGHTS(name) extern __shared__ __attribute__((aligned(16))) float name[]

// ---- stage: the packed policy from global memory into LDS, block-strided; one barrier.  Once per launch.
template <int H, int F>
__device__ __forceinline__ void wd_rollout_stage(const wd_rollout_kit &kit, float *weights) {
  const int n = wd_rollout_policy_floats(F, H, kit.n_actions);
  for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) weights[i] = kit.policy[i];
  __syncthreads();
}

// ---- act: tick k's action of this thread's agent.  Records the observation row it is drawn on and the action; stores
// the action to actions_arr[row] as well and returns it (0, and nothing stored or drawn, behind the last agent).
template <int H, int F>
__device__ __forceinline__ int wd_rollout_act(const wd_rollout_kit &kit, const float *weights, const float *obs_arr,
                                              int env, int agent, int n_agents, int k, int *actions_arr) {
  if (agent >= n_agents) return 0;
  const int64_t row = (int64_t)env * n_agents + agent;
  const int64_t at = (int64_t)k * gridDim.x * n_agents + row;  // row of tick k in a [T, E, N, ...] batch tensor
  float obs[F];
WD_ROLLOUT_UNROLL
  for (int j = 0; j < F; ++j) obs[j] = obs_arr[row * F + j];
WD_ROLLOUT_UNROLL
  for (int j = 0; j < F; ++j) kit.obs_batch[at * F + j] = obs[j];
  float logit[WD_ROLLOUT_MAX_ACTIONS], cum[WD_ROLLOUT_MAX_ACTIONS];
  const float m = wd_rollout_logits<H, F>(weights, obs, kit.n_actions, logit);
  wd_rollout_running_sums(logit, m, kit.n_actions, cum);
  const uint32_t epoch = kit.rng_state[WD_TICK_RNG_HEADER + row];
  kit.rng_state[WD_TICK_RNG_HEADER + row] = epoch + 1u;
  const wd_tick_u4 blk = wd_tick_block((uint32_t)row, epoch, kit.stream_tag, kit.rng_state[0], kit.rng_state[1]);
  const int a = wd_rollout_pick(cum, kit.n_actions, wd_tick_uniform(blk.x));
  actions_arr[row] = a;
  kit.action_batch[at] = a;
  return a;
}

// ---- end: record tick k's rewards and done flag, then restart the replica if the step finished it.  Returns whether
// it did (the same value in every thread).
__device__ __forceinline__ bool wd_rollout_end(const wd_rollout_kit &kit, int k, int *done_arr, int *env_timestep_arr,
                                               const float *rewards_arr, int env, int agent, int n_agents) {
  __syncthreads();  // everything the step stored, the flag included, is visible to the block from here on
  const int flag = __builtin_amdgcn_readfirstlane(done_arr[env]);  // one address, one writer: the first lane's copy
  const bool finished = flag != 0;
  // the record comes BEFORE the restart: `rewards` may be one of the arrays it restores
  if (agent < n_agents) {
    const int64_t row = (int64_t)env * n_agents + agent;
    kit.reward_batch[(int64_t)k * gridDim.x * n_agents + row] = rewards_arr[row];
  }
  if (agent == 0) kit.done_batch[(int64_t)k * gridDim.x + env] = flag;
  if (finished) {
    for (int r = 0; r < kit.reset_entries; ++r) {
      const wd_tick_reset_entry ent = kit.reset_table[r];
      const int64_t base = (int64_t)env * ent.row_elems;
      for (int i = (int)threadIdx.x; i < ent.row_elems; i += (int)blockDim.x) ent.data[base + i] = ent.ref[base + i];
    }
    if (agent == 0) env_timestep_arr[env] = 0;  // `_done_[env]` stays 1: the next tick's begin clears it
  }
  __syncthreads();  // the restored rows are visible to the next tick; its begin may overwrite the flag
  return finished;
}

#endif  // __HIPCC__
#endif  // WD_ENV_ROLLOUT_H_
