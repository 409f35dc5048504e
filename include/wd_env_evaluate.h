// wd_env_evaluate.h -- the kit for a ONE-LAUNCH EVALUATION of a custom environment with the POLICY INSIDE THE KERNEL: every
// replica runs ONE episode -- policy network on the agent's observation row, the action (greedy or sampled), the author's
// step -- up to its first done or `ticks` ticks, and the launch leaves a reward sum per agent and a step count per replica
// (docs/custom_environments.md, "Evaluation in one launch"; Trainer.evaluate_episodes).
//
// Self-contained like wd_env_rollout.h, which it includes: <hip/hip_runtime.h>, <stdint.h>, <math.h>, nothing of the
// package's own kernel sources.  The network is wd_env_rollout.h's (wd_rollout_logits, the softmax terms of
// wd_rollout_running_sums): the parity contract is stated THERE and not restated here.  The probabilities and the greedy
// scan form a section that a plain host compiler builds as well: a host program can print what a kernel will pick
// (tests/c/evaluate_pick_check.cpp).
//
// How an author uses it.  The step is the `__device__ __forceinline__` function of the fused tick (wd_env_tick.h); one
// template serves the two entries `Hip<Name>Evaluate_H32` and `Hip<Name>Evaluate_H64`, whose parameters are the step's
// own followed by WD_EVALUATE_PARAMS:
//
//     WD_EVALUATE_KIT(kit);                                  // the trailing parameters as one struct
//     WD_ROLLOUT_WEIGHTS(wd_rollout_w);                      // extern __shared__ float wd_rollout_w[], 16-byte aligned
//     wd_evaluate_stage<H, F>(kit, wd_rollout_w);            // packed policy -> LDS, once per launch, one barrier
//     float reward_sum = 0.0f;
//     int k = 0;
//     bool finished = false;
//     for (; k < ticks && !finished; ++k) {
//       wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
//       const int a = wd_evaluate_act<H, F>(kit, wd_rollout_w, obs_arr, env, agent, n_agents, k, actions_arr);
//       my_step(..., a, ...);
//       finished = wd_evaluate_end(kit, done_arr, rewards_arr, env, agent, n_agents, reward_sum);
//     }
//     wd_evaluate_finish(kit, k, finished, done_arr, env_timestep_arr, env, agent, n_agents, reward_sum);
//
// Geometry: the kit's.  One block per replica, one thread per agent, ceil(N / 64) * 64 threads; EVERY thread of the block
// calls every kit function, in uniform control flow.  The loop's exit is block-uniform: `finished` is the flag read behind
// a block barrier through the first lane's copy, as wd_rollout_end reads it.  E, the number of replicas, is gridDim.x.
//
// Trailing parameters (WD_EVALUATE_PARAMS), in this order -- warp_drive_amd/utils/custom_tick.py::custom_evaluate_launch
// packs exactly these; pointers and 32-bit scalars only:
//     uint32_t *rng_state      the sampler's state, as in wd_env_tick.h
//     const float *policy      the packed weights of wd_env_rollout.h
//     int n_actions            A, 1 .. WD_ROLLOUT_MAX_ACTIONS (8)
//     const void *reset_table  wd_tick_reset_entry[reset_entries]
//     int reset_entries
//     int stream_tag           counter word 2 of the draw
//     int use_argmax           0: sampled, else greedy
//     float *reward_sum        [E, N]
//     int *steps               [E]
//     int *done                [E]
//     int *action_trace        [T, E, N], T >= ticks, or null
//     int ticks                LAST, as in WD_TICK_PARAMS and WD_ROLLOUT_PARAMS
// All indexing into [T, E, N] is 64-bit.
//
// THE ACTION.  Both modes share ONE softmax: the probabilities p[a] = e[a] / sum, with e[a] and sum the expressions of
// wd_rollout_running_sums (wd_evaluate_probabilities).
//   * sampled (use_argmax == 0): exactly wd_rollout_act's draw -- the running sums cum = p[0], then cum + p[a] in action
//     order (wd_evaluate_running_sums: the same float32 operations in the same order as wd_rollout_running_sums, so the same
//     bits; tests/c/evaluate_pick_check.cpp prints both); row = env * N + agent reads its epoch e = rng_state[4 + row],
//     stores e + 1, makes ONE Philox4x32-10 call with counter (row, e, stream_tag, 5), takes word x through
//     wd_tick_uniform; the action is the number of running sums < u, clamped to A - 1 (wd_rollout_pick);
//   * greedy: the in-tree rule (csrc/kernels/rollout_policy.h, rp_first_maximum) -- the FIRST maximum of the float32
//     probabilities under a strict `<` scan; the scan is over the probabilities, not the logits (two logits that differ
//     may round to one probability).  No RNG word is read or written.
// (One softmax for both modes is also what keeps the entries within the scalar registers: two copies of it behind the
// mode's branch parked seven scalar values in lanes of a vector register.)
//
// WHAT A LAUNCH DOES PER REPLICA.  It starts from the state, observation, `_timestep_` and `_done_` the arrays hold and
// runs ticks up to the first done, at most `ticks`.  Every tick each agent's rewards_arr[row] is added into ONE float32
// register of its thread, in tick order; the terminal tick counts.  Tick k's action is stored to actions_arr[row], and to
// action_trace[k, env, agent] when the trace is given; trace rows behind a replica's last tick are not written.  At the
// end reward_sum[env, agent] holds the sum, steps[env] the ticks run, done[env] 1 if the replica finished and 0 if `ticks`
// ran out first, and the replica is restored UNCONDITIONALLY from the reset table with `_timestep_[env] = 0` and
// `_done_[env] = 0`: what reset_when_done(mode="force_reset") leaves.  Arrays without a reset copy (`rewards`, the action
// array) keep the last tick's values.  Threads behind the last agent store nothing.
//
// TWO DIFFERENCES FROM THE IN-TREE EVALUATE ENTRIES.  Those keep a replica's state in registers and leave the env's arrays
// read-only; a custom step writes global memory, so this kit RESTORES the arrays instead.  And the reward is read back
// from rewards_arr behind the end-of-tick barrier, BEFORE anything is restored: the ordering wd_rollout_end documents
// (`rewards` may have a reset copy; the thread that restores an agent's reward is the thread that has just added it).
//
// No inline assembly, no atomics, no cross-thread float reductions; every loop over units, inputs and actions is fully
// unrolled, so nothing is indexed at run time (no scratch memory).  The notes of wd_env_tick.h on `__restrict__` and on
// hand-overs through global memory within a tick hold here as well.
#ifndef WD_ENV_EVALUATE_H_
#define WD_ENV_EVALUATE_H_

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#include "wd_env_rollout.h"

// =============================================================================== host and device
// the probabilities of the softmax of the logits: e[a] / sum for a < n_actions (the terms, the sum and the division of
// wd_rollout_running_sums), 0 at and past n_actions
WD_TICK_HD void wd_evaluate_probabilities(const float (&logit)[WD_ROLLOUT_MAX_ACTIONS], float m, int n_actions,
                                          float (&prob)[WD_ROLLOUT_MAX_ACTIONS]) {
  float e[WD_ROLLOUT_MAX_ACTIONS], sum = 0.0f;
WD_ROLLOUT_UNROLL
  for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) {
    e[a] = (a < n_actions) ? expf(logit[a] - m) : 0.0f;
    sum += e[a];
  }
WD_ROLLOUT_UNROLL
  for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) prob[a] = e[a] / sum;
}

// the running sums of the probabilities, as wd_rollout_running_sums builds them: cum = p[0], then cum + p[a] in action order,
// the last value repeated behind n_actions
WD_TICK_HD void wd_evaluate_running_sums(const float (&prob)[WD_ROLLOUT_MAX_ACTIONS], int n_actions,
                                         float (&cum)[WD_ROLLOUT_MAX_ACTIONS]) {
  float run = 0.0f;
WD_ROLLOUT_UNROLL
  for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) {
    if (a < n_actions) run = (a == 0) ? prob[a] : run + prob[a];
    cum[a] = run;
  }
}

// the greedy action: the FIRST maximum of prob[0 .. n_actions) under a strict `<` scan (a tie goes to the lower index; a
// slot at or past n_actions is never picked)
WD_TICK_HD int wd_evaluate_first_maximum(const float (&prob)[WD_ROLLOUT_MAX_ACTIONS], int n_actions) {
  int a = 0;
  float best = prob[0];
WD_ROLLOUT_UNROLL
  for (int i = 1; i < WD_ROLLOUT_MAX_ACTIONS; ++i) {
    const bool better = i < n_actions && best < prob[i];
    best = better ? prob[i] : best;
    a = better ? i : a;
  }
  return a;
}

// =============================================================================== device only
#ifdef __HIPCC__

// the trailing parameters of an Evaluate entry, after the step's own (the order is the contract: see the top of the file)
#define WD_EVALUATE_PARAMS                                                                                         \
  uint32_t *wd_evaluate_rng_state_, const float *wd_evaluate_policy_, int wd_evaluate_n_actions_,                 \
      const void *wd_evaluate_reset_table_, int wd_evaluate_reset_entries_, int wd_evaluate_stream_tag_,          \
      int wd_evaluate_use_argmax_, float *wd_evaluate_reward_sum_, int *wd_evaluate_steps_, int *wd_evaluate_done_, \
      int *wd_evaluate_action_trace_, int ticks

struct wd_evaluate_kit {
  uint32_t *rng_state;
  const float *policy;
  int n_actions;
  const wd_tick_reset_entry *reset_table;
  int reset_entries;
  uint32_t stream_tag;
  int use_argmax;
  float *reward_sum;
  int *steps;
  int *done;
  int *action_trace;
};

// gathers the trailing parameters into `const wd_evaluate_kit name`
#define WD_EVALUATE_KIT(name)                                                                                      \
  const wd_evaluate_kit name = {wd_evaluate_rng_state_, wd_evaluate_policy_, wd_evaluate_n_actions_,              \
                                (const wd_tick_reset_entry *)wd_evaluate_reset_table_, wd_evaluate_reset_entries_, \
                                (uint32_t)wd_evaluate_stream_tag_, wd_evaluate_use_argmax_,                       \
                                wd_evaluate_reward_sum_, wd_evaluate_steps_, wd_evaluate_done_,                   \
                                wd_evaluate_action_trace_}

// ---- stage: the packed policy from global memory into LDS, block-strided; one barrier.  Once per launch.
template <int H, int F>
__device__ __forceinline__ void wd_evaluate_stage(const wd_evaluate_kit &kit, float *weights) {
  const int n = wd_rollout_policy_floats(F, H, kit.n_actions);
  for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) weights[i] = kit.policy[i];
  __syncthreads();
}

// ---- act: tick k's action of this thread's agent, greedy or sampled.  Stores it to actions_arr[row] and, when the trace
// is given, to action_trace[k, env, agent]; returns it (0, and nothing stored or drawn, behind the last agent).
template <int H, int F>
__device__ __forceinline__ int wd_evaluate_act(const wd_evaluate_kit &kit, const float *weights, const float *obs_arr,
                                               int env, int agent, int n_agents, int k, int *actions_arr) {
  if (agent >= n_agents) return 0;
  const int64_t row = (int64_t)env * n_agents + agent;
  float obs[F];
WD_ROLLOUT_UNROLL
  for (int j = 0; j < F; ++j) obs[j] = obs_arr[row * F + j];
  float logit[WD_ROLLOUT_MAX_ACTIONS], prob[WD_ROLLOUT_MAX_ACTIONS];
  const float m = wd_rollout_logits<H, F>(weights, obs, kit.n_actions, logit);
  wd_evaluate_probabilities(logit, m, kit.n_actions, prob);
  int a;
  if (kit.use_argmax != 0) {  // (a kernel argument: the same branch in every thread of the launch)
    a = wd_evaluate_first_maximum(prob, kit.n_actions);
  } else {
    float cum[WD_ROLLOUT_MAX_ACTIONS];
    wd_evaluate_running_sums(prob, kit.n_actions, cum);
    const uint32_t epoch = kit.rng_state[WD_TICK_RNG_HEADER + row];
    kit.rng_state[WD_TICK_RNG_HEADER + row] = epoch + 1u;
    const wd_tick_u4 blk = wd_tick_block((uint32_t)row, epoch, kit.stream_tag, kit.rng_state[0], kit.rng_state[1]);
    a = wd_rollout_pick(cum, kit.n_actions, wd_tick_uniform(blk.x));
  }
  actions_arr[row] = a;
  if (kit.action_trace != nullptr) kit.action_trace[(int64_t)k * gridDim.x * n_agents + row] = a;
  return a;
}

// ---- end: add the tick's reward of this thread's agent into `reward_sum` (a register) and say whether the step finished
// the replica (the same value in every thread).  Nothing is restored here: wd_evaluate_finish does it, once.
__device__ __forceinline__ bool wd_evaluate_end(const wd_evaluate_kit &kit, const int *done_arr, const float *rewards_arr,
                                                int env, int agent, int n_agents, float &reward_sum) {
  (void)kit;
  __syncthreads();  // everything the step stored, the flag included, is visible to the block from here on
  const bool finished = __builtin_amdgcn_readfirstlane(done_arr[env]) != 0;  // one address, one writer: the first lane's
  if (agent < n_agents) reward_sum += rewards_arr[(int64_t)env * n_agents + agent];
  __syncthreads();  // every thread has read the flag: the next tick's begin may clear it
  return finished;
}

// ---- finish: the outputs of this replica -- `k` ticks were run, `finished` is the last wd_evaluate_end's answer -- and
// the UNCONDITIONAL restore from the reset table, `_timestep_[env] = 0`, `_done_[env] = 0`.  Behind the last tick's closing
// barrier: everything the step stored has been read, the reward included.
__device__ __forceinline__ void wd_evaluate_finish(const wd_evaluate_kit &kit, int k, bool finished, int *done_arr,
                                                   int *env_timestep_arr, int env, int agent, int n_agents,
                                                   float reward_sum) {
  if (agent < n_agents) kit.reward_sum[(int64_t)env * n_agents + agent] = reward_sum;
  if (agent == 0) {
    kit.steps[env] = k;
    kit.done[env] = finished ? 1 : 0;
  }
  for (int r = 0; r < kit.reset_entries; ++r) {
    const wd_tick_reset_entry ent = kit.reset_table[r];
    const int64_t base = (int64_t)env * ent.row_elems;
    for (int i = (int)threadIdx.x; i < ent.row_elems; i += (int)blockDim.x) ent.data[base + i] = ent.ref[base + i];
  }
  if (agent == 0) {
    env_timestep_arr[env] = 0;
    done_arr[env] = 0;
  }
}

#endif  // __HIPCC__
#endif  // WD_ENV_EVALUATE_H_
