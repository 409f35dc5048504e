// ContractProbe: a test-only custom environment that reaches the clauses of the three kits (include/wd_env.h,
// wd_env_tick.h, wd_env_rollout.h) no worked example reaches.  Its step READS `_done_[env]` in every thread (so the Tick
// and Rollout entries call wd_tick_begin(..., /*step_reads_done=*/true)), writes SIGNED observations of magnitude up to 8
// with exact 0.0 and -0.0 among them, and mutates four arrays a restart restores: a per-replica scalar (row_elems 1), a
// row that is not agent-shaped, a row longer than the block, and the rewards array itself.  Integer state (the floats
// are small integers, halves and quarters), done at the time limit only.  One block per replica, one thread per agent,
// the block rounded up to whole wavefronts.
#include "wd_env_rollout.h"

#define CONTRACT_PROBE_WIDE 7  // wide[env, agent, 0 .. 7)
#define CONTRACT_PROBE_ODD 3   // odd[env, 0 .. 3)

// observation (t, agent, j): ((t * (agent + 1) + 3 * j) % 17 - 8), negated for an odd agent, halved where j % 3 == 2
__device__ __forceinline__ float contract_probe_obs(int t, int agent, int j) {
  const int v = (t * (agent + 1) + 3 * j) % 17 - 8;
  float x = (float)v * ((agent & 1) ? -1.0f : 1.0f);  // 0 * -1 is -0.0
  if (j % 3 == 2) x = x * 0.5f;
  return x;
}

// `action`: this thread's agent's (unused behind the last agent); `n_features`: a constant in the Rollout entries
__device__ __forceinline__ void contract_probe_step(float *obs_arr, int action, float *rewards_arr, int *done_arr,
                                                    int *env_timestep_arr, int *seen_done_arr, int *per_env_arr,
                                                    float *odd_arr, int *wide_arr, int episode_length, int n_agents,
                                                    int n_features) {
  const int seen = done_arr[wd_env_id()];  // FIRST: the flag as this thread finds it when the step begins
  const int env = wd_env_id(), agent = wd_agent_id();
  const int t = env_timestep_arr[env] + 1;
  wd_sync_env_threads();  // every thread has read the flag and the counter before agent 0 writes them
  if (agent < n_agents) {
    seen_done_arr[wd_index(env, agent, 0, n_agents, 1)] += seen;
    float *row = obs_arr + wd_index(env, agent, 0, n_agents, n_features);
    for (int j = 0; j < n_features; ++j) row[j] = contract_probe_obs(t, agent, j);
    rewards_arr[wd_index(env, agent, 0, n_agents, 1)] = (float)(action + 1);
    int *wide = wide_arr + wd_index(env, agent, 0, n_agents, CONTRACT_PROBE_WIDE);
    for (int c = 0; c < CONTRACT_PROBE_WIDE; ++c) wide[c] += agent * CONTRACT_PROBE_WIDE + c + t;
  }
  if (agent == 0) {
    per_env_arr[env] += 3 * t + 1;
    for (int c = 0; c < CONTRACT_PROBE_ODD; ++c)
      odd_arr[env * CONTRACT_PROBE_ODD + c] = odd_arr[env * CONTRACT_PROBE_ODD + c] + (float)(t + c) * 0.25f;
    env_timestep_arr[env] = t;
    if (t == episode_length) done_arr[env] = 1;
  }
}

WD_ENV_KERNEL void __launch_bounds__(1024)
HipContractProbeStep(float *obs_arr, const int *actions_arr, float *rewards_arr, int *done_arr, int *env_timestep_arr,
                     int *seen_done_arr, int *per_env_arr, float *odd_arr, int *wide_arr, int episode_length,
                     int n_agents, int n_features) {
  const int agent = wd_agent_id();
  const int action = agent < n_agents ? actions_arr[wd_index(wd_env_id(), agent, 0, n_agents, 1)] : 0;
  contract_probe_step(obs_arr, action, rewards_arr, done_arr, env_timestep_arr, seen_done_arr, per_env_arr, odd_arr,
                      wide_arr, episode_length, n_agents, n_features);
}

WD_ENV_KERNEL void __launch_bounds__(1024)
HipContractProbeTick(float *obs_arr, int *actions_arr, float *rewards_arr, int *done_arr, int *env_timestep_arr,
                     int *seen_done_arr, int *per_env_arr, float *odd_arr, int *wide_arr, int episode_length,
                     int n_agents, int n_features, WD_TICK_PARAMS) {
  const int env = wd_env_id(), agent = wd_agent_id();
  WD_TICK_KIT(kit);
  for (int k = 0; k < ticks; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/true);
    int act[WD_TICK_MAX_HEADS];
    wd_tick_sample(kit, env, agent, n_agents, actions_arr, act);
    contract_probe_step(obs_arr, act[0], rewards_arr, done_arr, env_timestep_arr, seen_done_arr, per_env_arr, odd_arr,
                        wide_arr, episode_length, n_agents, n_features);
    wd_tick_end(kit, done_arr, env_timestep_arr, env, agent);
  }
}

// static LDS whose size is no multiple of 16 bytes, next to the dynamic LDS of the staged policy: filled by three
// threads before the barrier of wd_rollout_stage, read back by every thread behind it (the result is 0 when intact)
#define CONTRACT_PROBE_PAD(pad, salt)                                  \
  __shared__ int pad[3];                                               \
  if (threadIdx.x < 3) pad[threadIdx.x] = (salt) + (int)threadIdx.x
#define CONTRACT_PROBE_PAD_ERROR(pad, salt) (pad[threadIdx.x % 3] - (salt) - (int)(threadIdx.x % 3))

template <int H, int F>
__device__ __forceinline__ void contract_probe_rollout(float *obs_arr, int *actions_arr, float *rewards_arr,
                                                       int *done_arr, int *env_timestep_arr, int *seen_done_arr,
                                                       int *per_env_arr, float *odd_arr, int *wide_arr,
                                                       int episode_length, int n_agents, const wd_rollout_kit &kit,
                                                       int ticks, float *weights) {
  const int env = wd_env_id(), agent = wd_agent_id();
  CONTRACT_PROBE_PAD(pad, ticks);
  wd_rollout_stage<H, F>(kit, weights);
  for (int k = 0; k < ticks; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/true);
    const int a = wd_rollout_act<H, F>(kit, weights, obs_arr, env, agent, n_agents, k, actions_arr);
    contract_probe_step(obs_arr, a, rewards_arr, done_arr, env_timestep_arr, seen_done_arr, per_env_arr, odd_arr,
                        wide_arr, episode_length, n_agents, F);
    wd_rollout_end(kit, k, done_arr, env_timestep_arr, rewards_arr, env, agent, n_agents);
  }
  if (agent < n_agents) seen_done_arr[wd_index(env, agent, 0, n_agents, 1)] += CONTRACT_PROBE_PAD_ERROR(pad, ticks);
}

// one thread per observation row, grid-stride: the 8 logits and the 8 running sums the public functions of the header
// compute on the device, from the policy staged the way a Rollout entry stages it
template <int H, int F>
__device__ __forceinline__ void contract_probe_logits(const float *policy, int n_actions, const float *obs_arr,
                                                      int n_rows, float *logits_out, float *cum_out, float *weights) {
  const wd_rollout_kit kit = {nullptr, policy, n_actions, nullptr, 0, 0u, nullptr, nullptr, nullptr, nullptr};
  CONTRACT_PROBE_PAD(pad, n_rows);
  wd_rollout_stage<H, F>(kit, weights);
  const float pad_error = (float)CONTRACT_PROBE_PAD_ERROR(pad, n_rows);  // 0
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
    // a compiler-only fence: the staged weights are read inside every trip, as a Rollout entry reads them inside every
    // tick, not hoisted out of the loop into (far too many) registers
    __atomic_signal_fence(__ATOMIC_SEQ_CST);
    float obs[F], logit[WD_ROLLOUT_MAX_ACTIONS], cum[WD_ROLLOUT_MAX_ACTIONS];
WD_ROLLOUT_UNROLL
    for (int j = 0; j < F; ++j) obs[j] = obs_arr[r * F + j];
    const float m = wd_rollout_logits<H, F>(weights, obs, n_actions, logit);
    wd_rollout_running_sums(logit, m, n_actions, cum);
WD_ROLLOUT_UNROLL
    for (int a = 0; a < WD_ROLLOUT_MAX_ACTIONS; ++a) {
      logits_out[r * WD_ROLLOUT_MAX_ACTIONS + a] = logit[a];
      cum_out[r * WD_ROLLOUT_MAX_ACTIONS + a] = cum[a] + pad_error;
    }
  }
}

#define CONTRACT_PROBE_ENTRIES(F, H, BOUND)                                                                           \
  WD_ENV_KERNEL void __launch_bounds__(BOUND) HipContractProbeRollout_F##F##_H##H(                                    \
      float *obs_arr, int *actions_arr, float *rewards_arr, int *done_arr, int *env_timestep_arr, int *seen_done_arr, \
      int *per_env_arr, float *odd_arr, int *wide_arr, int episode_length, int n_agents, int n_features,             \
      WD_ROLLOUT_PARAMS) {                                                                                            \
    WD_ROLLOUT_KIT(kit);                                                                                              \
    WD_ROLLOUT_WEIGHTS(wd_rollout_w);                                                                                 \
    contract_probe_rollout<H, F>(obs_arr, actions_arr, rewards_arr, done_arr, env_timestep_arr, seen_done_arr,       \
                                 per_env_arr, odd_arr, wide_arr, episode_length, n_agents, kit, ticks, wd_rollout_w); \
  }                                                                                                                   \
  WD_ENV_KERNEL void __launch_bounds__(64) HipContractProbeLogits_F##F##_H##H(                                        \
      const float *policy, int n_actions, const float *obs_arr, int n_rows, float *logits_out, float *cum_out) {     \
    WD_ROLLOUT_WEIGHTS(wd_rollout_w);                                                                                 \
    contract_probe_logits<H, F>(policy, n_actions, obs_arr, n_rows, logits_out, cum_out, wd_rollout_w);              \
  }

CONTRACT_PROBE_ENTRIES(1, 4, 1024)
CONTRACT_PROBE_ENTRIES(1, 32, 1024)
CONTRACT_PROBE_ENTRIES(4, 32, 1024)
CONTRACT_PROBE_ENTRIES(7, 32, 1024)
CONTRACT_PROBE_ENTRIES(7, 64, 512)
