// RendezvousUpdate: the Rendezvous example (examples/rendezvous/) whose WHOLE TRAINING ITERATION runs as kernels: the
// one-launch rollout with the policy inside it (include/wd_env_rollout.h, as examples/rendezvous_policy/) and the A2C /
// PPO update as five launches (include/wd_env_update.h; docs/custom_environments.md, "The update as kernels").  A custom
// environment: this file is registered with the env class and compiled on first use; it is not part of the package's
// build.
//
// The step is written ONCE, as rdvu_step(): HipRendezvousUpdateStep hands it the action it reads from the action array,
// HipRendezvousUpdateTick (wd_env_tick.h) the action it has just drawn from given probabilities, and
// HipRendezvousUpdateRollout_H32 / _H64 the action the in-kernel policy of that hidden width has just drawn on the
// agent's observation row.  Its body is the body of HipRendezvousStep (the host step of examples/rendezvous/rendezvous.py,
// line by line): integers on the state path, every float32 result ONE division of integer-valued floats (and one
// subtraction for the wall penalty), so the host's numpy float32 gives the same bits.
//
// The update's six entries -- HipRendezvousUpdatePgValues_H32 / _H64, ...PgGradients_H32 / _H64, ...PgReduce, ...PgApply
// -- are the last line of this file: the kit's macro, with the five observation floats of a row.
//
// Launch of the step, tick and rollout entries: one block per replica, one thread per agent, the block rounded up to
// whole wavefronts; threads behind the last agent carry the identity into the reductions and store nothing.  The _H64
// rollout entry is bound to 512 threads: two arrays of 64 activations do not fit the 128 registers a lane of a
// 1024-thread block has.
#include "wd_env_rollout.h"
#include "wd_env_update.h"

// (dx, dy) of action a at [2 a], [2 a + 1]; the host uploads it (initialize_shared_constants)
__constant__ int kRendezvousMoves[10];

#define RENDEZVOUS_ACTIONS 5
#define RENDEZVOUS_FEATURES 5

__device__ __forceinline__ int rdvu_abs(int v) { return v < 0 ? -v : v; }

// one tick of the replica of this block; `action`: this thread's agent's (ignored behind the last agent).  Every thread
// of the block calls it.  Nothing is handed between threads through global memory: the sums go through `scratch`.
__device__ __forceinline__ void rdvu_step(int *loc_x_arr, int *loc_y_arr, int action, int *done_arr, float *rewards_arr,
                                          float *obs_arr, float wall_penalty, int spread_limit, int grid_length,
                                          int *env_timestep_arr, int episode_length, int n_agents, int *scratch) {
  const int env = wd_env_id(), agent = wd_agent_id();
  const bool live = agent < n_agents;
  const int t = env_timestep_arr[env] + 1;  // (written back by thread 0 behind the barriers of the reductions)

  int x = 0, y = 0;
  bool hit = false;
  const int64_t at = wd_index(env, live ? agent : 0, 0, n_agents, 1);
  if (live) {
    const int a = (action < 0 || action >= RENDEZVOUS_ACTIONS) ? 0 : action;  // never index the table out of bounds
    const int mx = loc_x_arr[at] + kRendezvousMoves[2 * a], my = loc_y_arr[at] + kRendezvousMoves[2 * a + 1];
    x = mx < 0 ? 0 : (mx > grid_length ? grid_length : mx);
    y = my < 0 ? 0 : (my > grid_length ? grid_length : my);
    hit = x != mx || y != my;
  }
  const int sum_x = wd_env_sum_int(x, scratch);
  const int sum_y = wd_env_sum_int(y, scratch);
  // spread: N times the L1 distance to the centroid, an integer (0 is the identity of its maximum)
  const int spread = live ? rdvu_abs(n_agents * x - sum_x) + rdvu_abs(n_agents * y - sum_y) : 0;
  const int max_spread = wd_env_max_int(spread, scratch);

  if (live) {
    loc_x_arr[at] = x;
    loc_y_arr[at] = y;
    const float span = (float)(n_agents * grid_length), length = (float)grid_length;
    float reward = -(float)spread / span;
    if (hit) reward = reward - wall_penalty;
    rewards_arr[at] = reward;
    float *row = obs_arr + wd_index(env, agent, 0, n_agents, RENDEZVOUS_FEATURES);
    row[0] = (float)x / length;
    row[1] = (float)y / length;
    row[2] = (float)sum_x / span;
    row[3] = (float)sum_y / span;
    row[4] = (float)t / (float)episode_length;
  }
  if (agent == 0) {
    env_timestep_arr[env] = t;
    if (t == episode_length || (spread_limit >= 0 && max_spread <= spread_limit)) done_arr[env] = 1;
  }
}

WD_ENV_KERNEL void __launch_bounds__(1024)
HipRendezvousUpdateStep(int *loc_x_arr, int *loc_y_arr, const int *actions_arr, int *done_arr, float *rewards_arr,
                        float *obs_arr, float wall_penalty, int spread_limit, int grid_length, int *env_timestep_arr,
                        int episode_length, int n_agents) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  const int agent = wd_agent_id();
  const int action = agent < n_agents ? actions_arr[wd_index(wd_env_id(), agent, 0, n_agents, 1)] : 0;
  rdvu_step(loc_x_arr, loc_y_arr, action, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit, grid_length,
            env_timestep_arr, episode_length, n_agents, scratch);
}

// the fused tick (actions drawn from given probabilities): the step's parameters, then wd_env_tick.h's
WD_ENV_KERNEL void __launch_bounds__(1024)
HipRendezvousUpdateTick(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr, float *rewards_arr,
                        float *obs_arr, float wall_penalty, int spread_limit, int grid_length, int *env_timestep_arr,
                        int episode_length, int n_agents, WD_TICK_PARAMS) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  const int env = wd_env_id(), agent = wd_agent_id();
  WD_TICK_KIT(kit);
  for (int k = 0; k < ticks; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
    int act[WD_TICK_MAX_HEADS];
    wd_tick_sample(kit, env, agent, n_agents, actions_arr, act);
    rdvu_step(loc_x_arr, loc_y_arr, act[0], done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit, grid_length,
              env_timestep_arr, episode_length, n_agents, scratch);
    wd_tick_end(kit, done_arr, env_timestep_arr, env, agent);
  }
}

// the one-launch rollout, written once for both hidden widths: the policy is evaluated on the observation row the
// previous tick (or the restart) left, the batch rows of every tick are recorded
template <int H>
__device__ __forceinline__ void rdvu_rollout(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr,
                                             float *rewards_arr, float *obs_arr, float wall_penalty, int spread_limit,
                                             int grid_length, int *env_timestep_arr, int episode_length, int n_agents,
                                             const wd_rollout_kit &kit, int ticks, int *scratch, float *weights) {
  const int env = wd_env_id(), agent = wd_agent_id();
  wd_rollout_stage<H, RENDEZVOUS_FEATURES>(kit, weights);
  for (int k = 0; k < ticks; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
    const int a = wd_rollout_act<H, RENDEZVOUS_FEATURES>(kit, weights, obs_arr, env, agent, n_agents, k, actions_arr);
    rdvu_step(loc_x_arr, loc_y_arr, a, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit, grid_length,
              env_timestep_arr, episode_length, n_agents, scratch);
    wd_rollout_end(kit, k, done_arr, env_timestep_arr, rewards_arr, env, agent, n_agents);
  }
}

// the step's parameters (the action array is written here), then the kit's
WD_ENV_KERNEL void __launch_bounds__(1024)
HipRendezvousUpdateRollout_H32(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr, float *rewards_arr,
                               float *obs_arr, float wall_penalty, int spread_limit, int grid_length,
                               int *env_timestep_arr, int episode_length, int n_agents, WD_ROLLOUT_PARAMS) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  WD_ROLLOUT_KIT(kit);
  WD_ROLLOUT_WEIGHTS(wd_rollout_w);
  rdvu_rollout<32>(loc_x_arr, loc_y_arr, actions_arr, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit,
                   grid_length, env_timestep_arr, episode_length, n_agents, kit, ticks, scratch, wd_rollout_w);
}

WD_ENV_KERNEL void __launch_bounds__(512)
HipRendezvousUpdateRollout_H64(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr, float *rewards_arr,
                               float *obs_arr, float wall_penalty, int spread_limit, int grid_length,
                               int *env_timestep_arr, int episode_length, int n_agents, WD_ROLLOUT_PARAMS) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  WD_ROLLOUT_KIT(kit);
  WD_ROLLOUT_WEIGHTS(wd_rollout_w);
  rdvu_rollout<64>(loc_x_arr, loc_y_arr, actions_arr, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit,
                   grid_length, env_timestep_arr, episode_length, n_agents, kit, ticks, scratch, wd_rollout_w);
}

// the update: values, gradients (both widths), reduce, apply on rows of RENDEZVOUS_FEATURES = 5 observation floats
WD_PG_UPDATE_ENTRIES(RendezvousUpdate, 5)
