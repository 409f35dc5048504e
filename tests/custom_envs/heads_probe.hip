// HeadsProbe: a test-only custom environment that shows WHICH ACTION every head of the fused tick's draw
// (include/wd_env_tick.h) handed to the step: counts[env, agent, h] += action_h + 1.  Integer state, done at the time
// limit only.  One block per replica, one thread per agent, the block rounded up to whole wavefronts.
#include "wd_env_tick.h"

// `act`: the actions of this thread's agent (unused behind the last agent)
__device__ __forceinline__ void heads_probe_step(int *counts_arr, const int (&act)[WD_TICK_MAX_HEADS], int *done_arr,
                                                 int *env_timestep_arr, int episode_length, int n_agents, int n_heads) {
  const int env = wd_env_id(), agent = wd_agent_id();
  if (agent < n_agents) {
    int *row = counts_arr + wd_index(env, agent, 0, n_agents, n_heads);
    row[0] += act[0] + 1;
    if (n_heads > 1) row[1] += act[1] + 1;
    if (n_heads > 2) row[2] += act[2] + 1;
    if (n_heads > 3) row[3] += act[3] + 1;
  }
  if (agent == 0) {
    const int t = env_timestep_arr[env] + 1;
    env_timestep_arr[env] = t;
    if (t == episode_length) done_arr[env] = 1;
  }
}

WD_ENV_KERNEL void __launch_bounds__(1024)
HipHeadsProbeStep(int *counts_arr, const int *actions_arr, int *done_arr, int *env_timestep_arr, int episode_length,
                  int n_agents, int n_heads) {
  const int env = wd_env_id(), agent = wd_agent_id();
  int act[WD_TICK_MAX_HEADS] = {0, 0, 0, 0};
  if (agent < n_agents) {
    const int *row = actions_arr + wd_index(env, agent, 0, n_agents, n_heads);
    act[0] = row[0];
    if (n_heads > 1) act[1] = row[1];
    if (n_heads > 2) act[2] = row[2];
    if (n_heads > 3) act[3] = row[3];
  }
  heads_probe_step(counts_arr, act, done_arr, env_timestep_arr, episode_length, n_agents, n_heads);
}

WD_ENV_KERNEL void __launch_bounds__(1024)
HipHeadsProbeTick(int *counts_arr, int *actions_arr, int *done_arr, int *env_timestep_arr, int episode_length,
                  int n_agents, int n_heads, WD_TICK_PARAMS) {
  const int env = wd_env_id(), agent = wd_agent_id();
  WD_TICK_KIT(kit);
  for (int k = 0; k < ticks; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
    int act[WD_TICK_MAX_HEADS];
    wd_tick_sample(kit, env, agent, n_agents, actions_arr, act);
    heads_probe_step(counts_arr, act, done_arr, env_timestep_arr, episode_length, n_agents, n_heads);
    wd_tick_end(kit, done_arr, env_timestep_arr, env, agent);
  }
}
