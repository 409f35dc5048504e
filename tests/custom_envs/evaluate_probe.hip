// EvaluateProbe: a test-only custom environment for the one-launch evaluation of include/wd_env_evaluate.h with an EVEN
// observation size (F = 2) and a RUN-TIME action count: observation (counter / L, agent parity), reward = action + 1,
// done at the time limit only.  One block per replica, one thread per agent, the block rounded up to whole wavefronts.
#include "wd_env_evaluate.h"

#define EVALUATE_PROBE_FEATURES 2

// `action`: this thread's agent's (unused behind the last agent)
__device__ __forceinline__ void evaluate_probe_step(float *obs_arr, int action, float *rewards_arr, int *done_arr,
                                                  int *env_timestep_arr, int episode_length, int n_agents) {
  const int env = wd_env_id(), agent = wd_agent_id();
  const int t = env_timestep_arr[env] + 1;
  wd_sync_env_threads();  // every thread has read the counter before agent 0 writes it back
  if (agent < n_agents) {
    float *row = obs_arr + wd_index(env, agent, 0, n_agents, EVALUATE_PROBE_FEATURES);
    row[0] = (float)t / (float)episode_length;
    row[1] = (float)(agent & 1);
    rewards_arr[wd_index(env, agent, 0, n_agents, 1)] = (float)(action + 1);
  }
  if (agent == 0) {
    env_timestep_arr[env] = t;
    if (t == episode_length) done_arr[env] = 1;
  }
}

WD_ENV_KERNEL void __launch_bounds__(1024)
HipEvaluateProbeStep(float *obs_arr, const int *actions_arr, float *rewards_arr, int *done_arr, int *env_timestep_arr,
                   int episode_length, int n_agents) {
  const int agent = wd_agent_id();
  const int action = agent < n_agents ? actions_arr[wd_index(wd_env_id(), agent, 0, n_agents, 1)] : 0;
  evaluate_probe_step(obs_arr, action, rewards_arr, done_arr, env_timestep_arr, episode_length, n_agents);
}

WD_ENV_KERNEL void __launch_bounds__(1024)
HipEvaluateProbeTick(float *obs_arr, int *actions_arr, float *rewards_arr, int *done_arr, int *env_timestep_arr,
                   int episode_length, int n_agents, WD_TICK_PARAMS) {
  const int env = wd_env_id(), agent = wd_agent_id();
  WD_TICK_KIT(kit);
  for (int k = 0; k < ticks; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
    int act[WD_TICK_MAX_HEADS];
    wd_tick_sample(kit, env, agent, n_agents, actions_arr, act);
    evaluate_probe_step(obs_arr, act[0], rewards_arr, done_arr, env_timestep_arr, episode_length, n_agents);
    wd_tick_end(kit, done_arr, env_timestep_arr, env, agent);
  }
}

template <int H>
__device__ __forceinline__ void evaluate_probe_rollout(float *obs_arr, int *actions_arr, float *rewards_arr, int *done_arr,
                                                     int *env_timestep_arr, int episode_length, int n_agents,
                                                     const wd_rollout_kit &kit, int ticks, float *weights) {
  const int env = wd_env_id(), agent = wd_agent_id();
  wd_rollout_stage<H, EVALUATE_PROBE_FEATURES>(kit, weights);
  for (int k = 0; k < ticks; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
    const int a = wd_rollout_act<H, EVALUATE_PROBE_FEATURES>(kit, weights, obs_arr, env, agent, n_agents, k, actions_arr);
    evaluate_probe_step(obs_arr, a, rewards_arr, done_arr, env_timestep_arr, episode_length, n_agents);
    wd_rollout_end(kit, k, done_arr, env_timestep_arr, rewards_arr, env, agent, n_agents);
  }
}

WD_ENV_KERNEL void __launch_bounds__(1024)
HipEvaluateProbeRollout_H32(float *obs_arr, int *actions_arr, float *rewards_arr, int *done_arr, int *env_timestep_arr,
                          int episode_length, int n_agents, WD_ROLLOUT_PARAMS) {
  WD_ROLLOUT_KIT(kit);
  WD_ROLLOUT_WEIGHTS(wd_rollout_w);
  evaluate_probe_rollout<32>(obs_arr, actions_arr, rewards_arr, done_arr, env_timestep_arr, episode_length, n_agents, kit,
                           ticks, wd_rollout_w);
}

WD_ENV_KERNEL void __launch_bounds__(512)
HipEvaluateProbeRollout_H64(float *obs_arr, int *actions_arr, float *rewards_arr, int *done_arr, int *env_timestep_arr,
                          int episode_length, int n_agents, WD_ROLLOUT_PARAMS) {
  WD_ROLLOUT_KIT(kit);
  WD_ROLLOUT_WEIGHTS(wd_rollout_w);
  evaluate_probe_rollout<64>(obs_arr, actions_arr, rewards_arr, done_arr, env_timestep_arr, episode_length, n_agents, kit,
                           ticks, wd_rollout_w);
}

template <int H>
__device__ __forceinline__ void evaluate_probe_evaluate(float *obs_arr, int *actions_arr, float *rewards_arr,
                                                        int *done_arr, int *env_timestep_arr, int episode_length,
                                                        int n_agents, const wd_evaluate_kit &kit, int ticks,
                                                        float *weights) {
  const int env = wd_env_id(), agent = wd_agent_id();
  wd_evaluate_stage<H, EVALUATE_PROBE_FEATURES>(kit, weights);
  float reward_sum = 0.0f;
  int k = 0;
  bool finished = false;
  for (; k < ticks && !finished; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
    const int a = wd_evaluate_act<H, EVALUATE_PROBE_FEATURES>(kit, weights, obs_arr, env, agent, n_agents, k, actions_arr);
    evaluate_probe_step(obs_arr, a, rewards_arr, done_arr, env_timestep_arr, episode_length, n_agents);
    finished = wd_evaluate_end(kit, done_arr, rewards_arr, env, agent, n_agents, reward_sum);
  }
  wd_evaluate_finish(kit, k, finished, done_arr, env_timestep_arr, env, agent, n_agents, reward_sum);
}

WD_ENV_KERNEL void __launch_bounds__(1024)
HipEvaluateProbeEvaluate_H32(float *obs_arr, int *actions_arr, float *rewards_arr, int *done_arr, int *env_timestep_arr,
                             int episode_length, int n_agents, WD_EVALUATE_PARAMS) {
  WD_EVALUATE_KIT(kit);
  WD_ROLLOUT_WEIGHTS(wd_rollout_w);
  evaluate_probe_evaluate<32>(obs_arr, actions_arr, rewards_arr, done_arr, env_timestep_arr, episode_length, n_agents,
                              kit, ticks, wd_rollout_w);
}

WD_ENV_KERNEL void __launch_bounds__(512)
HipEvaluateProbeEvaluate_H64(float *obs_arr, int *actions_arr, float *rewards_arr, int *done_arr, int *env_timestep_arr,
                             int episode_length, int n_agents, WD_EVALUATE_PARAMS) {
  WD_EVALUATE_KIT(kit);
  WD_ROLLOUT_WEIGHTS(wd_rollout_w);
  evaluate_probe_evaluate<64>(obs_arr, actions_arr, rewards_arr, done_arr, env_timestep_arr, episode_length, n_agents,
                              kit, ticks, wd_rollout_w);
}
