// RendezvousEvaluate: the Rendezvous example (examples/rendezvous/) whose WHOLE TRAINING AND EVALUATION CYCLE runs as
// kernels: the one-launch rollout with the policy inside it (include/wd_env_rollout.h, as examples/rendezvous_policy/), the
// A2C / PPO update as five launches (include/wd_env_update.h, as examples/rendezvous_update/) and ONE EPISODE OF EVERY
// REPLICA IN ONE LAUNCH, greedy or sampled (include/wd_env_evaluate.h; docs/custom_environments.md, "Evaluation in one
// launch").  A custom environment: this file is registered with the env class and compiled on first use; it is not part of
// the package's build.
//
// The step is written ONCE, as rdve_step(): HipRendezvousEvaluateStep hands it the action it reads from the action array,
// HipRendezvousEvaluateTick (wd_env_tick.h) the action it has just drawn from given probabilities,
// HipRendezvousEvaluateRollout_H32 / _H64 the action the in-kernel policy of that hidden width has just drawn on the
// agent's observation row, and HipRendezvousEvaluateEvaluate_H32 / _H64 that policy's greedy or sampled action.  Its body is
// the body of HipRendezvousStep (the host step of examples/rendezvous/rendezvous.py, line by line): integers on the state
// path, every float32 result ONE division of integer-valued floats (and one subtraction for the wall penalty), so the
// host's numpy float32 gives the same bits.
//
// The update's six entries -- HipRendezvousEvaluatePgValues_H32 / _H64, ...PgGradients_H32 / _H64, ...PgReduce, ...PgApply
// -- are the last line of this file: the kit's macro, with the five observation floats of a row.
//
// Launch of the step, tick, rollout and evaluate entries: one block per replica, one thread per agent, the block rounded
// up to whole wavefronts; threads behind the last agent carry the identity into the reductions and store nothing.  The
// _H64 rollout and evaluate entries are bound to 512 threads: two arrays of 64 activations do not fit the 128 registers a
// lane of a 1024-thread block has.
#include "wd_env_evaluate.h"
#include "wd_env_update.h"

// (dx, dy) of action a at [2 a], [2 a + 1]; the host uploads it (initialize_shared_constants)
__constant__ int kRendezvousMoves[10];

#define RENDEZVOUS_ACTIONS 5
#define RENDEZVOUS_FEATURES 5

__device__ __forceinline__ int rdve_abs(int v) { return v < 0 ? -v : v; }

// one tick of the replica of this block; `action`: this thread's agent's (ignored behind the last agent).  Every thread
// of the block calls it.  Nothing is handed between threads through global memory: the sums go through `scratch`.
__device__ __forceinline__ void rdve_step(int *loc_x_arr, int *loc_y_arr, int action, int *done_arr, float *rewards_arr,
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
  const int spread = live ? rdve_abs(n_agents * x - sum_x) + rdve_abs(n_agents * y - sum_y) : 0;
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
HipRendezvousEvaluateStep(int *loc_x_arr, int *loc_y_arr, const int *actions_arr, int *done_arr, float *rewards_arr,
                        float *obs_arr, float wall_penalty, int spread_limit, int grid_length, int *env_timestep_arr,
                        int episode_length, int n_agents) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  const int agent = wd_agent_id();
  const int action = agent < n_agents ? actions_arr[wd_index(wd_env_id(), agent, 0, n_agents, 1)] : 0;
  rdve_step(loc_x_arr, loc_y_arr, action, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit, grid_length,
            env_timestep_arr, episode_length, n_agents, scratch);
}

// the fused tick (actions drawn from given probabilities): the step's parameters, then wd_env_tick.h's
WD_ENV_KERNEL void __launch_bounds__(1024)
HipRendezvousEvaluateTick(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr, float *rewards_arr,
                        float *obs_arr, float wall_penalty, int spread_limit, int grid_length, int *env_timestep_arr,
                        int episode_length, int n_agents, WD_TICK_PARAMS) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  const int env = wd_env_id(), agent = wd_agent_id();
  WD_TICK_KIT(kit);
  for (int k = 0; k < ticks; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
    int act[WD_TICK_MAX_HEADS];
    wd_tick_sample(kit, env, agent, n_agents, actions_arr, act);
    rdve_step(loc_x_arr, loc_y_arr, act[0], done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit, grid_length,
              env_timestep_arr, episode_length, n_agents, scratch);
    wd_tick_end(kit, done_arr, env_timestep_arr, env, agent);
  }
}

// the one-launch rollout, written once for both hidden widths: the policy is evaluated on the observation row the
// previous tick (or the restart) left, the batch rows of every tick are recorded
template <int H>
__device__ __forceinline__ void rdve_rollout(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr,
                                             float *rewards_arr, float *obs_arr, float wall_penalty, int spread_limit,
                                             int grid_length, int *env_timestep_arr, int episode_length, int n_agents,
                                             const wd_rollout_kit &kit, int ticks, int *scratch, float *weights) {
  const int env = wd_env_id(), agent = wd_agent_id();
  wd_rollout_stage<H, RENDEZVOUS_FEATURES>(kit, weights);
  for (int k = 0; k < ticks; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
    const int a = wd_rollout_act<H, RENDEZVOUS_FEATURES>(kit, weights, obs_arr, env, agent, n_agents, k, actions_arr);
    rdve_step(loc_x_arr, loc_y_arr, a, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit, grid_length,
              env_timestep_arr, episode_length, n_agents, scratch);
    wd_rollout_end(kit, k, done_arr, env_timestep_arr, rewards_arr, env, agent, n_agents);
  }
}

// the step's parameters (the action array is written here), then the kit's
WD_ENV_KERNEL void __launch_bounds__(1024)
HipRendezvousEvaluateRollout_H32(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr, float *rewards_arr,
                               float *obs_arr, float wall_penalty, int spread_limit, int grid_length,
                               int *env_timestep_arr, int episode_length, int n_agents, WD_ROLLOUT_PARAMS) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  WD_ROLLOUT_KIT(kit);
  WD_ROLLOUT_WEIGHTS(wd_rollout_w);
  rdve_rollout<32>(loc_x_arr, loc_y_arr, actions_arr, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit,
                   grid_length, env_timestep_arr, episode_length, n_agents, kit, ticks, scratch, wd_rollout_w);
}

WD_ENV_KERNEL void __launch_bounds__(512)
HipRendezvousEvaluateRollout_H64(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr, float *rewards_arr,
                               float *obs_arr, float wall_penalty, int spread_limit, int grid_length,
                               int *env_timestep_arr, int episode_length, int n_agents, WD_ROLLOUT_PARAMS) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  WD_ROLLOUT_KIT(kit);
  WD_ROLLOUT_WEIGHTS(wd_rollout_w);
  rdve_rollout<64>(loc_x_arr, loc_y_arr, actions_arr, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit,
                   grid_length, env_timestep_arr, episode_length, n_agents, kit, ticks, scratch, wd_rollout_w);
}

// one episode of every replica in one launch, written once for both hidden widths: the policy's greedy or sampled action
// on the observation row the previous tick left, the rewards summed in a register, up to the first done or `ticks` ticks;
// the replica is restored at the end
template <int H>
__device__ __forceinline__ void rdve_evaluate(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr,
                                              float *rewards_arr, float *obs_arr, float wall_penalty, int spread_limit,
                                              int grid_length, int *env_timestep_arr, int episode_length, int n_agents,
                                              const wd_evaluate_kit &kit, int ticks, int *scratch, float *weights) {
  const int env = wd_env_id(), agent = wd_agent_id();
  wd_evaluate_stage<H, RENDEZVOUS_FEATURES>(kit, weights);
  float reward_sum = 0.0f;
  int k = 0;
  bool finished = false;
  for (; k < ticks && !finished; ++k) {
    wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
    const int a = wd_evaluate_act<H, RENDEZVOUS_FEATURES>(kit, weights, obs_arr, env, agent, n_agents, k, actions_arr);
    rdve_step(loc_x_arr, loc_y_arr, a, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit, grid_length,
              env_timestep_arr, episode_length, n_agents, scratch);
    finished = wd_evaluate_end(kit, done_arr, rewards_arr, env, agent, n_agents, reward_sum);
  }
  wd_evaluate_finish(kit, k, finished, done_arr, env_timestep_arr, env, agent, n_agents, reward_sum);
}

WD_ENV_KERNEL void __launch_bounds__(1024)
HipRendezvousEvaluateEvaluate_H32(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr, float *rewards_arr,
                                  float *obs_arr, float wall_penalty, int spread_limit, int grid_length,
                                  int *env_timestep_arr, int episode_length, int n_agents, WD_EVALUATE_PARAMS) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  WD_EVALUATE_KIT(kit);
  WD_ROLLOUT_WEIGHTS(wd_rollout_w);
  rdve_evaluate<32>(loc_x_arr, loc_y_arr, actions_arr, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit,
                    grid_length, env_timestep_arr, episode_length, n_agents, kit, ticks, scratch, wd_rollout_w);
}

WD_ENV_KERNEL void __launch_bounds__(512)
HipRendezvousEvaluateEvaluate_H64(int *loc_x_arr, int *loc_y_arr, int *actions_arr, int *done_arr, float *rewards_arr,
                                  float *obs_arr, float wall_penalty, int spread_limit, int grid_length,
                                  int *env_timestep_arr, int episode_length, int n_agents, WD_EVALUATE_PARAMS) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  WD_EVALUATE_KIT(kit);
  WD_ROLLOUT_WEIGHTS(wd_rollout_w);
  rdve_evaluate<64>(loc_x_arr, loc_y_arr, actions_arr, done_arr, rewards_arr, obs_arr, wall_penalty, spread_limit,
                    grid_length, env_timestep_arr, episode_length, n_agents, kit, ticks, scratch, wd_rollout_w);
}

// the update: values, gradients (both widths), reduce, apply on rows of RENDEZVOUS_FEATURES = 5 observation floats
WD_PG_UPDATE_ENTRIES(RendezvousEvaluate, 5)
