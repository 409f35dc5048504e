// Rendezvous: N agents on the integer grid [0, L]^2 try to meet (examples/rendezvous/rendezvous.py holds the host
// step this mirrors line by line).  A custom environment: this file is registered with the env class and compiled on
// first use; it is not part of the package's build.
//
// Launch: one block per replica, one thread per agent, the block rounded up to whole wavefronts (the reductions of
// wd_env.h need that); threads behind the last agent carry the identity into the reductions and store nothing.
// Everything on the state path is an integer; every float32 result is ONE division of integer-valued floats (and one
// subtraction for the wall penalty), so the host's numpy float32 gives the same bits.
#include "wd_env.h"

// (dx, dy) of action a at [2 a], [2 a + 1]; the host uploads it (initialize_shared_constants)
__constant__ int kRendezvousMoves[10];

#define RENDEZVOUS_ACTIONS 5
#define RENDEZVOUS_FEATURES 5

__device__ __forceinline__ int rdv_abs(int v) { return v < 0 ? -v : v; }

WD_ENV_KERNEL void __launch_bounds__(1024)
HipRendezvousStep(int *loc_x_arr, int *loc_y_arr, const int *actions_arr, int *done_arr, float *rewards_arr,
                  float *obs_arr, float wall_penalty, int spread_limit, int grid_length, int *env_timestep_arr,
                  int episode_length, int n_agents) {
  __shared__ int scratch[WD_ENV_SCRATCH_INTS];
  const int env = wd_env_id(), agent = wd_agent_id();
  const bool live = agent < n_agents;
  const int t = env_timestep_arr[env] + 1;  // (written back by thread 0 behind the barriers of the reductions)

  int x = 0, y = 0;
  bool hit = false;
  const int64_t at = wd_index(env, live ? agent : 0, 0, n_agents, 1);
  if (live) {
    int a = actions_arr[at];
    a = (a < 0 || a >= RENDEZVOUS_ACTIONS) ? 0 : a;  // never index the table out of bounds
    const int mx = loc_x_arr[at] + kRendezvousMoves[2 * a], my = loc_y_arr[at] + kRendezvousMoves[2 * a + 1];
    x = mx < 0 ? 0 : (mx > grid_length ? grid_length : mx);
    y = my < 0 ? 0 : (my > grid_length ? grid_length : my);
    hit = x != mx || y != my;
  }
  const int sum_x = wd_env_sum_int(x, scratch);
  const int sum_y = wd_env_sum_int(y, scratch);
  // spread: N times the L1 distance to the centroid, an integer (0 is the identity of its maximum)
  const int spread = live ? rdv_abs(n_agents * x - sum_x) + rdv_abs(n_agents * y - sum_y) : 0;
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

// custom reset: every agent of every replica onto the cell (cell_x, cell_y); launched with one thread per agent and
// one block per replica (the resetter's default geometry)
WD_ENV_KERNEL void HipRendezvousReset(int *loc_x_arr, int *loc_y_arr, int cell_x, int cell_y) {
  const int64_t at = wd_index(wd_env_id(), wd_agent_id(), 0, (int)blockDim.x, 1);
  loc_x_arr[at] = cell_x;
  loc_y_arr[at] = cell_y;
}
