// classic_control.hip -- ClassicControl Acrobot, MountainCar, ContinuousMountainCar and Pendulum: the device step of each
// (one thread per replica, grid-stride, as HipClassicControlCartPoleEnvStep) and one fused tick template, cc_tick_impl,
// that samples the action, steps and restarts a finished replica `ticks` times per launch with the state in registers.
// Acrobot and MountainCar also have cc_evaluate_impl (the ...EnvEvaluate_H<H> entries): one episode of every replica in one
// launch with the policy network inside the kernel, greedy or sampled, writing a reward sum and a step count per replica.
// ContinuousMountainCar and Pendulum have cc_evaluate_actor_impl (the ...EnvEvaluate_A<H> entries): the same with the
// deterministic actor of DDPG inside the kernel, noise-free or under the tick's OU draw.
//
// Follows the reference's device kernels, example_envs/single_agent/classic_control/{acrobot,mountain_car,
// continuous_mountain_car,pendulum}/*_step_numba.py.  Numba's type inference is restated expression by expression
// (the numpy restatements in envs/classic_control.py follow the same flow; tests/golden/cc_*_traj.npz pin both):
//   * a float32 op stays float32 (state, scalar arguments, the action of the continuous envs);
//   * an op with a Python float or int literal, or a module-level Python constant, widens to float64;
//   * float32 ** int literal stays float32 (Numba's power typing: RN32(x * x)); float64 ** 2 is x * x in float64;
//   * math.sin / math.cos of a float32 are the float32 functions (wd_np_sincosf: numpy's float32 kernel, bit for
//     bit), of a float64 the float64 ones (device cos / sin: within a float64 ulp of the host's libm);
//   * a variable assigned a float64 inside a loop or through a branch (wrap(), _clip() with float64 bounds) is float64
//     throughout: Numba unifies the two types.
// Per env:
//   Acrobot    RK4, dt = 0.2.  _dsdt: cos(theta2) / sin(theta2) float32; cos(theta1 + theta2 - pi/2) and cos(theta1 - pi/2)
//              float64 (the float32 sum, then the float64 subtraction); d1, d2, phi1, phi2, ddtheta float64; the derivative
//              and k-update arrays are float32 locals (each element rounded).  wrap() / bound() in float64, stored as float32.
//              _terminal and the observation: float32 cos / sin of the float32 state.
//   MountainCar  velocity and position float64 from the first `+=` on ((action - 1) is int64, `3 * position` float64);
//              the goal test on the float64 values; reward -1; done = 1 on time-out, else 2 on reaching the goal.
//   ContinuousMountainCar  force = clip(action) float32, force * power float32, the rest as MountainCar; reward
//              (100 on the goal) - pow(action, 2) * 0.1 with pow(float32, 2) = RN32(a * a) (the float32 overloads of
//              math.pow), the difference float64.
//   Pendulum   u = clip(action, +-2.0) float64; angle_normalize float64 (Python's % = fmod + sign fix, numpy's remainder);
//              thdot ** 2 float32; sin(th) float32; newthdot / newth float64; observation cos / sin of the float64 angle.
//
// Algorithmic bytes per unfused step (state read + write, action, observation, reward, done, timestep read + write):
// Acrobot 76, MountainCar 44, ContinuousMountainCar 44, Pendulum 48.
#include <type_traits>

#include "wd_common.h"
#include "rollout_policy.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ Acrobot
constexpr double AC_PI = 3.1415926535897932384626433;
constexpr double AC_MAX_VEL_1 = 12.566370614359172;  // 4 pi
constexpr double AC_MAX_VEL_2 = 28.274333882308138;  // 9 pi

__device__ __forceinline__ void ac_dsdt(const float (&st)[4], double a, float (&d)[4]) {
  constexpr double m1 = 1.0, m2 = 1.0, l1 = 1.0, lc1 = 0.5, lc2 = 0.5, I1 = 1.0, I2 = 1.0, g = 9.8;
  const float theta1 = st[0], theta2 = st[1], dtheta1 = st[2], dtheta2 = st[3];
  float s2f, c2f;
  wd_np_sincosf(theta2, s2f, c2f);
  const double s2 = (double)s2f, c2 = (double)c2f;
  const double d1 = m1 * (lc1 * lc1) + m2 * ((l1 * l1) + (lc2 * lc2) + 2.0 * l1 * lc2 * c2) + I1 + I2;
  const double d2 = m2 * ((lc2 * lc2) + l1 * lc2 * c2) + I2;
  const double phi2 = m2 * lc2 * g * cos((double)(theta1 + theta2) - AC_PI / 2.0);
  const double phi1 = -m2 * l1 * lc2 * (double)(dtheta2 * dtheta2) * s2 -
                      2.0 * m2 * l1 * lc2 * (double)dtheta2 * (double)dtheta1 * s2 +
                      (m1 * lc1 + m2 * l1) * g * cos((double)theta1 - AC_PI / 2.0) + phi2;
  const double ddtheta2 = (a + d2 / d1 * phi1 - m2 * l1 * lc2 * (double)(dtheta1 * dtheta1) * s2 - phi2) /
                          (m2 * (lc2 * lc2) + I2 - d2 * d2 / d1);
  const double ddtheta1 = -(d2 * ddtheta2 + phi1) / d1;
  d[0] = dtheta1;
  d[1] = dtheta2;
  d[2] = (float)ddtheta1;
  d[3] = (float)ddtheta2;
}

__device__ __forceinline__ float ac_wrap(float xf) {
  constexpr double m = -AC_PI, M = AC_PI, diff = M - m;
  double x = (double)xf;
  while (x > M) x = x - diff;
  while (x < m) x = x + diff;
  return (float)x;
}

__device__ __forceinline__ float ac_bound(float xf, double M) {
  double x = (double)xf;
  x = (x < -M) ? -M : x;
  x = (x > M) ? M : x;
  return (float)x;
}

struct CcAcrobot {
  static constexpr int S = 4, O = 6;
  static constexpr bool CONT = false;
  // returns the done code of a terminal state (1) or 0
  __device__ __forceinline__ int step(float (&s)[4], int action, float (&o)[6], float &rew) const {
    const double torque = (action == 0) ? -1.0 : (action == 1 ? 0.0 : 1.0);  // AVAIL_TORQUE[action]
    constexpr double dt = 0.2, dt2 = 0.1;
    float k1[4], k2[4], k3[4], k4[4], u[4];
    ac_dsdt(s, torque, k1);
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = (float)((double)s[i] + (double)k1[i] * dt2);
    ac_dsdt(u, torque, k2);
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = (float)((double)s[i] + (double)k2[i] * dt2);
    ac_dsdt(u, torque, k3);
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = (float)((double)s[i] + (double)k3[i] * dt);
    ac_dsdt(u, torque, k4);
    float ns[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      ns[i] = (float)((double)s[i] +
                      dt / 6.0 * ((double)k1[i] + 2.0 * (double)k2[i] + 2.0 * (double)k3[i] + (double)k4[i]));
    s[0] = ac_wrap(ns[0]);
    s[1] = ac_wrap(ns[1]);
    s[2] = ac_bound(ns[2], AC_MAX_VEL_1);
    s[3] = ac_bound(ns[3], AC_MAX_VEL_2);
    float s0, c0, s1, c1, s01, c01;
    wd_np_sincosf(s[0], s0, c0);
    wd_np_sincosf(s[1], s1, c1);
    wd_np_sincosf(s[1] + s[0], s01, c01);
    const bool terminated = (-c0 - c01) > 1.0f;
    rew = terminated ? 0.0f : -1.0f;
    o[0] = c0; o[1] = s0; o[2] = c1; o[3] = s1; o[4] = s[2]; o[5] = s[3];
    return terminated ? 1 : 0;
  }
};

// -------------------------------------------------------------------------------------------- MountainCar (discrete)
__device__ __forceinline__ double cc_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct CcMountainCar {
  static constexpr int S = 2, O = 2;
  static constexpr bool CONT = false;
  float min_position, max_position, max_speed, goal_position, goal_velocity, force, gravity;
  __device__ __forceinline__ int step(float (&s)[2], int action, float (&o)[2], float &rew) const {
    double position = (double)s[0], velocity = (double)s[1];
    velocity += (double)(action - 1) * (double)force + cos(3.0 * position) * (double)(-gravity);
    velocity = cc_clip(velocity, (double)(-max_speed), (double)max_speed);
    position += velocity;
    position = cc_clip(position, (double)min_position, (double)max_position);
    if (position == (double)min_position && velocity < 0.0) velocity = 0.0;
    s[0] = (float)position;
    s[1] = (float)velocity;
    o[0] = s[0];
    o[1] = s[1];
    rew = -1.0f;
    return (position >= (double)goal_position && velocity >= (double)goal_velocity) ? 2 : 0;
  }
};

// --------------------------------------------------------------------------------------------- ContinuousMountainCar
struct CcContinuousMountainCar {
  static constexpr int S = 2, O = 2;
  static constexpr bool CONT = true;
  float min_action, max_action, min_position, max_position, max_speed, goal_position, goal_velocity, power;
  __device__ __forceinline__ int step(float (&s)[2], float action, float (&o)[2], float &rew) const {
    const float f = action < min_action ? min_action : (action > max_action ? max_action : action);
    double position = (double)s[0], velocity = (double)s[1];
    velocity += (double)(f * power) - 0.0025 * cos(3.0 * position);
    velocity = cc_clip(velocity, (double)(-max_speed), (double)max_speed);
    position += velocity;
    position = cc_clip(position, (double)min_position, (double)max_position);
    if (position == (double)min_position && velocity < 0.0) velocity = 0.0;
    s[0] = (float)position;
    s[1] = (float)velocity;
    o[0] = s[0];
    o[1] = s[1];
    const bool terminated = position >= (double)goal_position && velocity >= (double)goal_velocity;
    rew = (float)((terminated ? 100.0 : 0.0) - (double)(action * action) * 0.1);
    return terminated ? 1 : 0;
  }
};

// ---------------------------------------------------------------------------------------------------------- Pendulum
struct CcPendulum {
  static constexpr int S = 2, O = 3;
  static constexpr bool CONT = true;
  __device__ __forceinline__ int step(float (&s)[2], float action, float (&o)[3], float &rew) const {
    constexpr double max_speed = 8.0, max_torque = 2.0, dt = 0.05, g = 9.81, m = 1.0, l = 1.0;
    constexpr double PI = 3.141592653589793, TWO_PI = 2.0 * 3.141592653589793;
    const double u = cc_clip((double)action, -max_torque, max_torque);
    const float th = s[0], thdot = s[1];
    // ((th + pi) % (2 pi)) - pi with Python's (and numpy's) remainder
    double an = fmod((double)th + PI, TWO_PI);
    if (an != 0.0) {
      if (an < 0.0) an += TWO_PI;
    } else {
      an = 0.0;
    }
    an = an - PI;
    const double costs = an * an + 0.1 * (double)(thdot * thdot) + 0.001 * (u * u);
    float sin_th, cos_th;
    wd_np_sincosf(th, sin_th, cos_th);
    double newthdot = (double)thdot + (3.0 * g / (2.0 * l) * (double)sin_th + 3.0 / (m * (l * l)) * u) * dt;
    newthdot = cc_clip(newthdot, -max_speed, max_speed);
    const double newth = (double)th + newthdot * dt;
    s[0] = (float)newth;
    s[1] = (float)newthdot;
    o[0] = (float)cos(newth);
    o[1] = (float)sin(newth);
    o[2] = (float)newthdot;
    rew = (float)(-costs);
    return 0;
  }
};

// ---------------------------------------------------------------------------------------------------- shared pieces
template <int N>
__device__ __forceinline__ void cc_load_row(const float *p, int env, float (&v)[N]) {
  if constexpr (N == 4) {
    const float4 q = ((const float4 *)p)[env];
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else if constexpr (N == 2) {
    const float2 q = ((const float2 *)p)[env];
    v[0] = q.x; v[1] = q.y;
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = p[(long)env * N + i];
  }
}

template <int N>
__device__ __forceinline__ void cc_store_row(float *p, int env, const float (&v)[N]) {
  if constexpr (N == 4) {
    ((float4 *)p)[env] = make_float4(v[0], v[1], v[2], v[3]);
  } else if constexpr (N == 2) {
    ((float2 *)p)[env] = make_float2(v[0], v[1]);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) p[(long)env * N + i] = v[i];
  }
}

// the per-tick record stores of the fused tick: untracked (wd_common.h), the launch never reads these addresses back
template <int N>
__device__ __forceinline__ void cc_store_row_untracked(float *p, long row, const float (&v)[N]) {
  if constexpr (N == 4) {
    wd_store_untracked((float4 *)p + row, make_float4(v[0], v[1], v[2], v[3]));
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) wd_store_untracked(p + row * N + i, v[i]);
  }
}

template <class Env, class A>
__device__ __forceinline__ void cc_step_impl(const Env &e, float *state_arr, const A *action_arr, int *done_arr,
                                             float *reward_arr, float *observation_arr, int *env_timestep_arr,
                                             int episode_length, int n_envs) {
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < n_envs; env += gridDim.x * blockDim.x) {
    const int t = env_timestep_arr[env] + 1;
    env_timestep_arr[env] = t;
    float s[Env::S], o[Env::O], rew;
    cc_load_row<Env::S>(state_arr, env, s);
    const int term = e.step(s, action_arr[env], o, rew);
    cc_store_row<Env::S>(state_arr, env, s);
    cc_store_row<Env::O>(observation_arr, env, o);
    reward_arr[env] = rew;
    const int done = (t == episode_length) ? 1 : term;
    if (done) done_arr[env] = done;
  }
}

// the arguments every fused tick takes after its env's step arguments
struct CcTickArgs {
  float *state_arr;
  void *action_arr;
  int *done_arr;
  float *reward_arr;
  float *observation_arr;
  int *env_timestep_arr;
  int episode_length, n_envs;
  uint32_t *rng_state;
  const float *probs;
  int n_actions;
  const void *reset_table;
  int n_reset_arrays, stream_tag, ticks;
  float *obs_batch;
  void *action_batch;
  float *reward_batch;
  int *done_batch;
  uint32_t *pool_rng;
  const float *pool;
  int n_pool;
  float *ou_state;
  float damping, stddev, scale;
};

constexpr int CC_MAX_ACTIONS = 8;

// ---- the policy INSIDE the tick and the evaluation: rollout_policy.h (the network, the parity contract and the packed
// layout, pack_rollout_policy with I = O) behind the float2-row first layer; restated on the host in
// tests/classic_control_policy.py::policy_probabilities.  cc_policy_probs: the probabilities e[a] / sum (what the greedy
// scan needs); cc_policy_cum: their running float32 sums.  The activations (2 H registers) and the float64 temporaries
// of the env's step are live in different phases of a tick.
// (the float2-row first layer stands in both functions: as a function of its own, here or in rollout_policy.h, the
// rollout and evaluation entries' registers are numbered otherwise)
template <int H, int O>
__device__ __forceinline__ void cc_policy_probs(const float *w, const float (&o)[O], int n_actions,
                                                float (&prob)[CC_MAX_ACTIONS]) {
  static_assert(O % 2 == 0, "the rows of W0 are read as float2");
  const float *W0 = w, *b0 = W0 + O * H, *W1 = b0 + H, *b1 = W1 + H * H, *Wp = b1 + H, *bp = Wp + n_actions * H;
  float h1[H], h2[H], logit[CC_MAX_ACTIONS];
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = b0[i];
#pragma unroll
    for (int j = 0; j < O; j += 2) {
      const float2 wr = *(const float2 *)(W0 + O * i + j);
      acc = fmaf(wr.x, o[j], acc); acc = fmaf(wr.y, o[j + 1], acc);
    }
    h1[i] = fmaxf(acc, 0.0f);
  }
  rp_second_layer<H>(W1, b1, h1, h2);
  const float m = rp_logits<H>(Wp, bp, h2, n_actions, logit);
  rp_softmax_probs(logit, m, n_actions, prob);
}

// (the softmax's terms and divisions stand here next to the running sums: behind a call the rollout entries compile to
// another schedule; rollout_policy.h::rp_softmax_probs is the same statements)
template <int H, int O>
__device__ __forceinline__ void cc_policy_cum(const float *w, const float (&o)[O], int n_actions,
                                              float (&cumv)[CC_MAX_ACTIONS]) {
  static_assert(O % 2 == 0, "the rows of W0 are read as float2");
  const float *W0 = w, *b0 = W0 + O * H, *W1 = b0 + H, *b1 = W1 + H * H, *Wp = b1 + H, *bp = Wp + n_actions * H;
  float h1[H], h2[H], logit[CC_MAX_ACTIONS];
#pragma unroll
  for (int i = 0; i < H; ++i) {
    float acc = b0[i];
#pragma unroll
    for (int j = 0; j < O; j += 2) {
      const float2 wr = *(const float2 *)(W0 + O * i + j);
      acc = fmaf(wr.x, o[j], acc); acc = fmaf(wr.y, o[j + 1], acc);
    }
    h1[i] = fmaxf(acc, 0.0f);
  }
  rp_second_layer<H>(W1, b1, h1, h2);
  const float m = rp_logits<H>(Wp, bp, h2, n_actions, logit);
  float e[CC_MAX_ACTIONS], sum = 0.0f;
#pragma unroll
  for (int a = 0; a < CC_MAX_ACTIONS; ++a) {
    e[a] = (a < n_actions) ? expf(logit[a] - m) : 0.0f;
    sum += e[a];
  }
  float cum = 0.0f;
#pragma unroll
  for (int a = 0; a < CC_MAX_ACTIONS; ++a) {
    const float p = e[a] / sum;
    if (a < n_actions) cum = (a == 0) ? p : cum + p;
    cumv[a] = cum;
  }
}

// ---- the deterministic actor INSIDE the tick and the evaluation of the Box envs (DDPG): rollout_policy.h behind the
// padded first layer (pack_rollout_actor: rows of OP = O rounded up to even floats, the pad column zero), mean =
// fmaf(action_scale, tanhf(z), action_bias); restated on the host in tests/classic_control_actor.py::actor_mean_f32.
template <int H, int O>
__device__ __forceinline__ float cc_actor_mean(const float *w, const float (&o)[O], float action_scale,
                                               float action_bias) {
  constexpr int OP = rp_actor_op(O);
  float h1[H];
  rp_first_layer_padded<H, O>(w, w + OP * H, o, h1);
  return rp_actor_mean<H>(w + OP * H + H, h1, action_scale, action_bias);
}

struct CcActorArgs {
  float action_scale, action_bias;
  float *mean_batch;  // [T, E] or null: row k = the means of tick k
};

// Fused rollout tick(s) (the conventions of HipClassicControlCartPoleEnvTick): per tick, draw the action, step, and
// restart a finished replica; the state, the observation and the timestep stay in registers.  Discrete envs draw
// the categorical action from `probs` [E, n_actions] with wd_tick_draw(row, epoch0 + k, stream_tag); continuous envs
// draw sample_ou_process's OU / Gaussian action (counter {row, epoch, stream_tag, 1}, the same Box-Muller expression,
// `ou_state` updated, the epoch advanced only when scale >= 1e-8) on the means `probs` [E].  A finished replica
// restores every array of the reset table (the observation row, and the state when it has a saved copy) and, with a
// pool (`pool` [n_pool, S], `pool_rng` = the resetter's RNG words), restarts from the pool row that
// reset_when_done_from_pool would draw: counter {env, epoch, 0x706f6f6c, 2}, epoch advanced on a hit only.
// `_done_` reports the last tick; timestep is cleared.  With the four `*_batch` pointers tick k writes row k.
// H > 0 (discrete envs, the ...EnvRollout_H<H> entries): a LIVE policy.  `weights` = dynamic LDS of n_w = O H + H + H H + H
// + A H + A floats; the block copies the packed network `policy` into it once per launch, and every tick evaluates it
// on the observation the lane holds (the one row k of `obs_batch` records) instead of reading `probs`.  The draw keeps
// the fixed-probability tick's Philox counters.
// H > 0 (Box envs, the ...EnvRollout_A<H> entries): a LIVE deterministic actor.  `weights` = dynamic LDS of
// rp_actor_floats(H, O) floats, copied from the packed network `policy` once per launch; every tick sets `mean` to
// cc_actor_mean of the observation the lane holds instead of keeping the launch's one `probs[env]` (`probs` is not read),
// and with `actor.mean_batch` records it in row k.  The OU draw, the step and the restart are the code below, unchanged.
template <class Env, bool BATCH, int H = 0>
__device__ __forceinline__ void cc_tick_impl(const Env &e, const CcTickArgs &a, float *weights = nullptr,
                                             const float *policy = nullptr,
                                             const CcActorArgs &actor = CcActorArgs{1.0f, 0.0f, nullptr}) {
  constexpr bool ACTOR = H > 0 && Env::CONT;
  if constexpr (H > 0) {
    const int n_w = ACTOR ? rp_actor_floats(H, Env::O) : rp_policy_floats(Env::O, H, a.n_actions);
    for (int i = threadIdx.x; i < n_w; i += blockDim.x) weights[i] = policy[i];
    __syncthreads();
  }
  using Act = typename std::conditional<Env::CONT, float, int>::type;
  constexpr int S = Env::S, O = Env::O;
  const wd_reset_entry *table = (const wd_reset_entry *)a.reset_table;
  const uint32_t k0 = a.rng_state[0], k1 = a.rng_state[1];
  const uint32_t pk0 = a.pool ? a.pool_rng[0] : 0u, pk1 = a.pool ? a.pool_rng[1] : 0u;
  Act *action_arr = (Act *)a.action_arr;
  const size_t E = (size_t)a.n_envs;
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < a.n_envs; env += gridDim.x * blockDim.x) {
    int t = a.env_timestep_arr[env];
    float s[S], o[O];
    cc_load_row<S>(a.state_arr, env, s);
    if (BATCH || H > 0) cc_load_row<O>(a.observation_arr, env, o);
    const uint32_t epoch0 = a.rng_state[WD_RNG_HEADER + env];
    uint32_t pool_epoch = a.pool ? a.pool_rng[WD_RNG_HEADER + env] : 0u;
    float cumv[CC_MAX_ACTIONS], mean = 0.0f, ou = 0.0f;
    if (Env::CONT) {
      if constexpr (!ACTOR) mean = a.probs[env];
      ou = a.ou_state[env];
    } else if (H == 0) {
      const float *row = a.probs + (long)env * a.n_actions;
      float cum = 0.0f;
#pragma unroll
      for (int i = 0; i < CC_MAX_ACTIONS; ++i) {
        if (i < a.n_actions) cum = (i == 0) ? row[0] : cum + row[i];
        cumv[i] = cum;
      }
    }
    wd_u4 blk = wd_u4{0u, 0u, 0u, 0u};
    uint32_t blk_quad = 0xffffffffu;
    const bool draw_ou = a.scale >= 1.0e-8f;
    int done = 0;
    for (int k = 0; k < a.ticks; ++k) {
      // ---- sample
      Act act;
      if constexpr (Env::CONT) {
        if constexpr (ACTOR) {  // live actor: THIS tick's observation
          mean = cc_actor_mean<H, O>(weights, o, actor.action_scale, actor.action_bias);
          if (actor.mean_batch) wd_store_untracked(actor.mean_batch + ((long)k * (long)E + env), mean);
        }
        if (draw_ou) {
          const wd_u4 rnd = wd_philox4x32_10(wd_u4{(uint32_t)env, epoch0 + (uint32_t)k, (uint32_t)a.stream_tag, 1u}, k0, k1);
          const float u1 = wd_u01_open_closed(rnd.x), u2 = wd_u01_open_closed(rnd.y);
          const float normal = sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
          ou = (1.0f - a.damping) * ou + a.stddev * normal;
          act = mean + a.scale * ou;
        } else {
          act = mean;
        }
      } else {
        const float u = wd_u01_open_closed(wd_tick_draw((uint32_t)env, epoch0 + (uint32_t)k, (uint32_t)a.stream_tag,
                                                        k0, k1, blk, blk_quad));
        if constexpr (H > 0) cc_policy_cum<H, O>(weights, o, a.n_actions, cumv);  // live policy: THIS tick's observation
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < CC_MAX_ACTIONS; ++i) cnt += (i < a.n_actions && cumv[i] < u) ? 1 : 0;
        act = min(cnt, a.n_actions - 1);
      }
      // ---- step
      const long rk = (long)k * (long)E + env;  // row k of the batch tensors
      if (BATCH) cc_store_row_untracked<O>(a.obs_batch, rk, o);  // the observation this action was drawn on
      t += 1;
      float rew;
      const int term = e.step(s, act, o, rew);
      done = (t == a.episode_length) ? 1 : term;
      if (BATCH) {
        wd_store_untracked((Act *)a.action_batch + rk, act);
        wd_store_untracked(a.reward_batch + rk, rew);
        wd_store_untracked(a.done_batch + rk, done);
      }
      wd_store_untracked(action_arr + env, act);
      wd_store_untracked(a.reward_arr + env, rew);
      wd_store_untracked(a.done_arr + env, done);
      cc_store_row_untracked<O>(a.observation_arr, env, o);
      // ---- restart a finished replica (reset_when_done_fused + reset_when_done_from_pool + undo)
      if (done) {
        t = 0;
        for (int r = 0; r < a.n_reset_arrays; ++r) {
          const wd_reset_entry ent = table[r];
          const long base = (long)env * ent.row_elems;
          for (int i = 0; i < ent.row_elems; ++i) ent.data[base + i] = ent.ref[base + i];
          if ((size_t)ent.data == (size_t)a.state_arr && ent.row_elems == S) {
#pragma unroll
            for (int i = 0; i < S; ++i) s[i] = __uint_as_float(ent.ref[base + i]);
          }
          if ((size_t)ent.data == (size_t)a.observation_arr && ent.row_elems == O) {
#pragma unroll
            for (int i = 0; i < O; ++i) o[i] = __uint_as_float(ent.ref[base + i]);
          }
        }
        if (a.pool) {
          const wd_u4 rnd = wd_philox4x32_10(wd_u4{(uint32_t)env, pool_epoch, 0x706f6f6cu, 2u}, pk0, pk1);
          const float p = (float)(rnd.x >> 8) * 0x1.0p-24f;
          const int ref_id = min((int)(p * (float)a.n_pool), a.n_pool - 1);
          cc_load_row<S>(a.pool, ref_id, s);
          pool_epoch += 1u;
        }
      }
    }
    cc_store_row<S>(a.state_arr, env, s);
    a.env_timestep_arr[env] = t;
    if (Env::CONT) {
      if (draw_ou) {
        a.ou_state[env] = ou;
        a.rng_state[WD_RNG_HEADER + env] = epoch0 + (uint32_t)a.ticks;
      }
    } else {
      a.rng_state[WD_RNG_HEADER + env] = epoch0 + (uint32_t)a.ticks;
    }
    if (a.pool) a.pool_rng[WD_RNG_HEADER + env] = pool_epoch;
  }
}

template <class Env>
__device__ __forceinline__ void cc_tick(const Env &e, const CcTickArgs &a) {
  if (a.obs_batch) cc_tick_impl<Env, true>(e, a);
  else cc_tick_impl<Env, false>(e, a);
}

// the rollout with a live policy; `hidden` must be the entry's width and n_actions fit the registers (else: no tick)
template <int H, class Env>
__device__ __forceinline__ void cc_rollout(const Env &e, const CcTickArgs &a, float *weights, const float *policy,
                                           int hidden) {
  if (hidden != H || a.n_actions < 1 || a.n_actions > CC_MAX_ACTIONS || policy == nullptr) return;  // (uniform)
  if (a.obs_batch) cc_tick_impl<Env, true, H>(e, a, weights, policy);
  else cc_tick_impl<Env, false, H>(e, a, weights, policy);
}

// the rollout of a Box env with a live actor; `hidden` must be the entry's width (else: no tick)
template <int H, class Env>
__device__ __forceinline__ void cc_rollout_actor(const Env &e, const CcTickArgs &a, float *weights, const float *actor,
                                                 int hidden, const CcActorArgs &aa) {
  static_assert(Env::CONT, "the actor's output is a Box action");
  if (hidden != H || actor == nullptr) return;  // (uniform)
  if (a.obs_batch) cc_tick_impl<Env, true, H>(e, a, weights, actor, aa);
  else cc_tick_impl<Env, false, H>(e, a, weights, actor, aa);
}

// ---- evaluation: ONE episode of every replica in one launch (the ...EnvEvaluate_H<H> entries), greedy or sampled.
// One lane per replica: load the state, the observation and the timestep once, then at most `ticks` ticks of
// (network on the observation in registers -> action -> Env::step), stopping at the first non-zero done; the terminal
// tick counts (sum += reward, steps += 1 before the test).  use_argmax: the first maximum of the probabilities (the
// standalone sampler's strict-'<' scan); otherwise the counting draw on the running sums with the Philox counters of the
// fixed-probability tick, wd_tick_draw(env, epoch0 + k, stream_tag).  WRITES: eval_reward_sum / eval_steps / eval_done
// [n_envs] (eval_done = the done value that ended the episode, 0 when `ticks` ran out first), row k of `action_trace`
// [ticks, n_envs] (optional) while the replica runs, and -- sampled mode only -- the replica's epoch word += steps.
// Nothing else: the env's arrays are read only, there is no restart, hence no reset table and no pool.  The guard is
// cc_rollout's.  The loads are consumed before the tick loop and the trace store is untracked (wd_common.h), as in
// cc_tick_impl: no wait inside the loop.
template <int H, class Env>
__device__ __forceinline__ void cc_evaluate_impl(const Env &e, const float *state_arr, const float *observation_arr,
                                                 const int *env_timestep_arr, int episode_length, int n_envs,
                                                 uint32_t *rng_state, int n_actions, int stream_tag,
                                                 int ticks, float *weights, const float *policy,
                                                 int hidden, int use_argmax, float *eval_reward_sum, int *eval_steps,
                                                 int *eval_done, int *action_trace) {
  static_assert(!Env::CONT, "the in-kernel policy has a softmax head");
  if (hidden != H || n_actions < 1 || n_actions > CC_MAX_ACTIONS || policy == nullptr) return;  // (uniform)
  constexpr int S = Env::S, O = Env::O;
  const int n_w = rp_policy_floats(O, H, n_actions);
  for (int i = threadIdx.x; i < n_w; i += blockDim.x) weights[i] = policy[i];
  __syncthreads();
  const uint32_t k0 = rng_state[0], k1 = rng_state[1];
  const bool greedy = use_argmax > 0;  // (uniform)
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < n_envs; env += gridDim.x * blockDim.x) {
    int t = env_timestep_arr[env];
    float s[S], o[O];
    cc_load_row<S>(state_arr, env, s);
    cc_load_row<O>(observation_arr, env, o);
    uint32_t epoch0 = rng_state[WD_RNG_HEADER + env];
    asm volatile("" : "+v"(t), "+v"(epoch0));
#pragma unroll
    for (int i = 0; i < S; ++i) asm volatile("" : "+v"(s[i]));
#pragma unroll
    for (int i = 0; i < O; ++i) asm volatile("" : "+v"(o[i]));
    wd_u4 blk = wd_u4{0u, 0u, 0u, 0u};
    uint32_t blk_quad = 0xffffffffu;
    float sum = 0.0f;
    int steps = 0, done = 0;
    int *trace = action_trace ? action_trace + env : nullptr;
    for (int k = 0; k < ticks; ++k) {
      float prob[CC_MAX_ACTIONS];
      cc_policy_probs<H, O>(weights, o, n_actions, prob);
      int act = 0;
      if (greedy) {
        act = rp_first_maximum(prob, n_actions);
      } else {
        const float u = wd_u01_open_closed(wd_tick_draw((uint32_t)env, epoch0 + (uint32_t)k, (uint32_t)stream_tag,
                                                        k0, k1, blk, blk_quad));
        float cum = 0.0f;
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < CC_MAX_ACTIONS; ++i) {
          if (i < n_actions) cum = (i == 0) ? prob[0] : cum + prob[i];
          cnt += (i < n_actions && cum < u) ? 1 : 0;
        }
        act = min(cnt, n_actions - 1);
      }
      if (trace) {
        wd_store_untracked(trace, act);
        trace += n_envs;
      }
      t += 1;
      float rew;
      const int term = e.step(s, act, o, rew);
      sum += rew;
      steps += 1;
      done = (t == episode_length) ? 1 : term;
      if (done) break;
    }
    eval_reward_sum[env] = sum;
    eval_steps[env] = steps;
    eval_done[env] = done;
    if (!greedy) rng_state[WD_RNG_HEADER + env] = epoch0 + (uint32_t)steps;
  }
}

// ---- evaluation of the Box envs (the ...EnvEvaluate_A<H> entries, DDPG): cc_evaluate_impl with cc_actor_mean in place
// of the softmax policy.  Per tick: mean = cc_actor_mean of the observation in registers; the action is the fused
// tick's own draw around it when scale >= 1e-8 (Philox counter {env, epoch0 + k, stream_tag, 1}, the same Box-Muller
// expression, ou = (1 - damping) ou + stddev normal, act = mean + scale ou), else the mean itself (greedy = scale 0, as
// the tick means it: there is no use_argmax); t += 1, Env::step, sum += reward, steps += 1, done = time-out ? 1 :
// terminal code, stop at the first done (the terminal tick counts).  WRITES: eval_reward_sum / eval_steps / eval_done
// [n_envs] (eval_done = 0 when `ticks` ran out first), row k of `mean_trace` and of `action_trace` (float [ticks, n_envs],
// each optional) while the replica runs, and -- only when it drew -- ou_state[env] and the replica's epoch word +=
// steps.  Nothing else: the env's arrays are read only, there is no restart.  The guard is cc_rollout_actor's.  The
// loads are consumed before the tick loop and the trace stores are untracked: no wait inside the loop.
template <int H, class Env>
__device__ __forceinline__ void cc_evaluate_actor_impl(const Env &e, const float *state_arr,
                                                       const float *observation_arr, const int *env_timestep_arr,
                                                       int episode_length, int n_envs, uint32_t *rng_state,
                                                       int stream_tag, int ticks, float *weights, const float *actor,
                                                       int hidden, float action_scale, float action_bias,
                                                       float *ou_state, float damping, float stddev, float scale,
                                                       float *eval_reward_sum, int *eval_steps, int *eval_done,
                                                       float *mean_trace, float *action_trace) {
  static_assert(Env::CONT, "the actor's output is a Box action");
  if (hidden != H || actor == nullptr) return;  // (uniform)
  constexpr int S = Env::S, O = Env::O;
  constexpr int n_w = rp_actor_floats(H, O);
  for (int i = threadIdx.x; i < n_w; i += blockDim.x) weights[i] = actor[i];
  __syncthreads();
  const uint32_t k0 = rng_state[0], k1 = rng_state[1];
  const bool draw_ou = scale >= 1.0e-8f;  // (uniform)
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < n_envs; env += gridDim.x * blockDim.x) {
    int t = env_timestep_arr[env];
    float s[S], o[O];
    cc_load_row<S>(state_arr, env, s);
    cc_load_row<O>(observation_arr, env, o);
    uint32_t epoch0 = rng_state[WD_RNG_HEADER + env];
    float ou = draw_ou ? ou_state[env] : 0.0f;
    asm volatile("" : "+v"(t), "+v"(epoch0), "+v"(ou));
#pragma unroll
    for (int i = 0; i < S; ++i) asm volatile("" : "+v"(s[i]));
#pragma unroll
    for (int i = 0; i < O; ++i) asm volatile("" : "+v"(o[i]));
    float sum = 0.0f;
    int steps = 0, done = 0;
    float *mtrace = mean_trace ? mean_trace + env : nullptr;
    float *atrace = action_trace ? action_trace + env : nullptr;
    for (int k = 0; k < ticks; ++k) {
      const float mean = cc_actor_mean<H, O>(weights, o, action_scale, action_bias);
      if (mtrace) {
        wd_store_untracked(mtrace, mean);
        mtrace += n_envs;
      }
      float act = mean;
      if (draw_ou) {
        const wd_u4 rnd = wd_philox4x32_10(wd_u4{(uint32_t)env, epoch0 + (uint32_t)k, (uint32_t)stream_tag, 1u}, k0, k1);
        const float u1 = wd_u01_open_closed(rnd.x), u2 = wd_u01_open_closed(rnd.y);
        const float normal = sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
        ou = (1.0f - damping) * ou + stddev * normal;
        act = mean + scale * ou;
      }
      if (atrace) {
        wd_store_untracked(atrace, act);
        atrace += n_envs;
      }
      t += 1;
      float rew;
      const int term = e.step(s, act, o, rew);
      sum += rew;
      steps += 1;
      done = (t == episode_length) ? 1 : term;
      if (done) break;
    }
    eval_reward_sum[env] = sum;
    eval_steps[env] = steps;
    eval_done[env] = done;
    if (draw_ou) {
      ou_state[env] = ou;
      rng_state[WD_RNG_HEADER + env] = epoch0 + (uint32_t)steps;
    }
  }
}

}  // namespace

// the arguments of every tick kernel after the env's step arguments
#define CC_TICK_PARAMS                                                                                                 \
  uint32_t *rng_state, const float *probs, int n_actions, const void *reset_table, int n_reset_arrays, int stream_tag, \
      int ticks, float *obs_batch, void *action_batch, float *reward_batch, int *done_batch, uint32_t *pool_rng,       \
      const float *pool, int n_pool, float *ou_state, float damping, float stddev, float scale
#define CC_TICK_ARGS(STATE, ACTION, DONE, REWARD, OBS, TIMESTEP)                                                      \
  CcTickArgs{STATE, ACTION, DONE, REWARD, OBS, TIMESTEP, episode_length, n_envs, rng_state, probs, n_actions,          \
             reset_table, n_reset_arrays, stream_tag, ticks, obs_batch, action_batch, reward_batch, done_batch,        \
             pool_rng, pool, n_pool, ou_state, damping, stddev, scale}

extern "C" {

__global__ void __launch_bounds__(256) HipClassicControlAcrobotEnvStep(float *__restrict__ state_arr, const int *__restrict__ action_arr,
                                                int *__restrict__ done_arr, float *__restrict__ reward_arr,
                                                float *__restrict__ observation_arr, int *__restrict__ env_timestep_arr,
                                                int episode_length, int n_envs) {
  cc_step_impl(CcAcrobot{}, state_arr, action_arr, done_arr, reward_arr, observation_arr, env_timestep_arr,
               episode_length, n_envs);
}

__global__ void __launch_bounds__(256) HipClassicControlMountainCarEnvStep(float *__restrict__ state_arr, const int *__restrict__ action_arr,
                                                    int *__restrict__ done_arr, float *__restrict__ reward_arr,
                                                    float *__restrict__ observation_arr, float min_position,
                                                    float max_position, float max_speed, float goal_position,
                                                    float goal_velocity, float force, float gravity,
                                                    int *__restrict__ env_timestep_arr, int episode_length, int n_envs) {
  const CcMountainCar e{min_position, max_position, max_speed, goal_position, goal_velocity, force, gravity};
  cc_step_impl(e, state_arr, action_arr, done_arr, reward_arr, observation_arr, env_timestep_arr, episode_length, n_envs);
}

__global__ void __launch_bounds__(256) HipClassicControlContinuousMountainCarEnvStep(
    float *__restrict__ state_arr, const float *__restrict__ action_arr, int *__restrict__ done_arr,
    float *__restrict__ reward_arr, float *__restrict__ observation_arr, float min_action, float max_action,
    float min_position, float max_position, float max_speed, float goal_position, float goal_velocity, float power,
    int *__restrict__ env_timestep_arr, int episode_length, int n_envs) {
  const CcContinuousMountainCar e{min_action, max_action, min_position, max_position,
                                  max_speed, goal_position, goal_velocity, power};
  cc_step_impl(e, state_arr, action_arr, done_arr, reward_arr, observation_arr, env_timestep_arr, episode_length, n_envs);
}

__global__ void __launch_bounds__(256) HipClassicControlPendulumEnvStep(float *__restrict__ state_arr, const float *__restrict__ action_arr,
                                                 int *__restrict__ done_arr, float *__restrict__ reward_arr,
                                                 float *__restrict__ observation_arr, int *__restrict__ env_timestep_arr,
                                                 int episode_length, int n_envs) {
  cc_step_impl(CcPendulum{}, state_arr, action_arr, done_arr, reward_arr, observation_arr, env_timestep_arr,
               episode_length, n_envs);
}

// (no __restrict__ on the tick kernels' arrays: the reset table aliases them)
__global__ void __launch_bounds__(256) HipClassicControlAcrobotEnvTick(float *state_arr, int *action_arr, int *done_arr, float *reward_arr,
                                                float *observation_arr, int *env_timestep_arr, int episode_length,
                                                int n_envs, CC_TICK_PARAMS) {
  cc_tick(CcAcrobot{}, CC_TICK_ARGS(state_arr, action_arr, done_arr, reward_arr, observation_arr, env_timestep_arr));
}

__global__ void __launch_bounds__(256) HipClassicControlMountainCarEnvTick(float *state_arr, int *action_arr, int *done_arr, float *reward_arr,
                                                    float *observation_arr, float min_position, float max_position,
                                                    float max_speed, float goal_position, float goal_velocity,
                                                    float force, float gravity, int *env_timestep_arr,
                                                    int episode_length, int n_envs, CC_TICK_PARAMS) {
  const CcMountainCar e{min_position, max_position, max_speed, goal_position, goal_velocity, force, gravity};
  cc_tick(e, CC_TICK_ARGS(state_arr, action_arr, done_arr, reward_arr, observation_arr, env_timestep_arr));
}

__global__ void __launch_bounds__(256) HipClassicControlContinuousMountainCarEnvTick(
    float *state_arr, float *action_arr, int *done_arr, float *reward_arr, float *observation_arr, float min_action,
    float max_action, float min_position, float max_position, float max_speed, float goal_position,
    float goal_velocity, float power, int *env_timestep_arr, int episode_length, int n_envs, CC_TICK_PARAMS) {
  const CcContinuousMountainCar e{min_action, max_action, min_position, max_position,
                                  max_speed, goal_position, goal_velocity, power};
  cc_tick(e, CC_TICK_ARGS(state_arr, action_arr, done_arr, reward_arr, observation_arr, env_timestep_arr));
}

__global__ void __launch_bounds__(256) HipClassicControlPendulumEnvTick(float *state_arr, float *action_arr, int *done_arr, float *reward_arr,
                                                 float *observation_arr, int *env_timestep_arr, int episode_length,
                                                 int n_envs, CC_TICK_PARAMS) {
  cc_tick(CcPendulum{}, CC_TICK_ARGS(state_arr, action_arr, done_arr, reward_arr, observation_arr, env_timestep_arr));
}

// the rollout with a live policy (two hidden layers of HH units + one softmax head, packed weights in dynamic LDS): the
// arguments of the env's tick, then the packed network and its width
#define CC_ROLLOUT_ENTRIES(HH)                                                                                         \
  __global__ void __launch_bounds__(256, 2) HipClassicControlAcrobotEnvRollout_H##HH(                                  \
      float *state_arr, int *action_arr, int *done_arr, float *reward_arr, float *observation_arr,                     \
      int *env_timestep_arr, int episode_length, int n_envs, CC_TICK_PARAMS, const float *policy, int hidden) {        \
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];                                                     \
    cc_rollout<HH>(CcAcrobot{},                                                                                        \
                   CC_TICK_ARGS(state_arr, action_arr, done_arr, reward_arr, observation_arr, env_timestep_arr),      \
                   cc_lds, policy, hidden);                                                                            \
  }                                                                                                                    \
  __global__ void __launch_bounds__(256, 2) HipClassicControlMountainCarEnvRollout_H##HH(                              \
      float *state_arr, int *action_arr, int *done_arr, float *reward_arr, float *observation_arr,                     \
      float min_position, float max_position, float max_speed, float goal_position, float goal_velocity, float force,  \
      float gravity, int *env_timestep_arr, int episode_length, int n_envs, CC_TICK_PARAMS, const float *policy,       \
      int hidden) {                                                                                                    \
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];                                                     \
    const CcMountainCar e{min_position, max_position, max_speed, goal_position, goal_velocity, force, gravity};        \
    cc_rollout<HH>(e, CC_TICK_ARGS(state_arr, action_arr, done_arr, reward_arr, observation_arr, env_timestep_arr),   \
                   cc_lds, policy, hidden);                                                                            \
  }
CC_ROLLOUT_ENTRIES(32)
CC_ROLLOUT_ENTRIES(64)

// the rollout of the Box envs with a live deterministic actor (two hidden layers of HH units + one tanh output, packed
// weights in dynamic LDS): the arguments of the env's tick, then the packed actor, its width, the output's scale and
// bias, and the [T, E] record of the means (or null)
#define CC_ACTOR_ENTRIES(HH)                                                                                           \
  __global__ void __launch_bounds__(256, 2) HipClassicControlContinuousMountainCarEnvRollout_A##HH(                    \
      float *state_arr, float *action_arr, int *done_arr, float *reward_arr, float *observation_arr, float min_action, \
      float max_action, float min_position, float max_position, float max_speed, float goal_position,                  \
      float goal_velocity, float power, int *env_timestep_arr, int episode_length, int n_envs, CC_TICK_PARAMS,         \
      const float *actor, int hidden, float action_scale, float action_bias, float *mean_batch) {                      \
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];                                                     \
    const CcContinuousMountainCar e{min_action, max_action, min_position, max_position,                                \
                                    max_speed, goal_position, goal_velocity, power};                                   \
    cc_rollout_actor<HH>(e, CC_TICK_ARGS(state_arr, action_arr, done_arr, reward_arr, observation_arr,                 \
                                         env_timestep_arr),                                                            \
                         cc_lds, actor, hidden, CcActorArgs{action_scale, action_bias, mean_batch});                   \
  }                                                                                                                    \
  __global__ void __launch_bounds__(256, 2) HipClassicControlPendulumEnvRollout_A##HH(                                 \
      float *state_arr, float *action_arr, int *done_arr, float *reward_arr, float *observation_arr,                   \
      int *env_timestep_arr, int episode_length, int n_envs, CC_TICK_PARAMS, const float *actor, int hidden,           \
      float action_scale, float action_bias, float *mean_batch) {                                                      \
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];                                                     \
    cc_rollout_actor<HH>(CcPendulum{}, CC_TICK_ARGS(state_arr, action_arr, done_arr, reward_arr, observation_arr,      \
                                                    env_timestep_arr),                                                 \
                         cc_lds, actor, hidden, CcActorArgs{action_scale, action_bias, mean_batch});                   \
  }
CC_ACTOR_ENTRIES(32)
CC_ACTOR_ENTRIES(64)

// one episode of every replica with the policy inside the kernel (cc_evaluate_impl): the env's step arguments (read
// only), then what the evaluation takes
#define CC_EVALUATE_PARAMS                                                                                             \
  uint32_t *rng_state, int n_actions, int stream_tag, int ticks, const float *policy, int hidden, int use_argmax,      \
      float *eval_reward_sum, int *eval_steps, int *eval_done, int *action_trace
#define CC_EVALUATE_CALL(HH, ENV)                                                                                      \
  cc_evaluate_impl<HH>(ENV, state_arr, observation_arr, env_timestep_arr, episode_length, n_envs, rng_state,           \
                       n_actions, stream_tag, ticks, cc_lds, policy, hidden, use_argmax,    \
                       eval_reward_sum, eval_steps, eval_done, action_trace)
#define CC_EVALUATE_ENTRIES(HH)                                                                                        \
  __global__ void __launch_bounds__(256, 2) HipClassicControlAcrobotEnvEvaluate_H##HH(                                 \
      const float *state_arr, const int *action_arr, const int *done_arr, const float *reward_arr,                     \
      const float *observation_arr, const int *env_timestep_arr, int episode_length, int n_envs,                       \
      CC_EVALUATE_PARAMS) {                                                                                            \
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];                                                     \
    const CcAcrobot e{};                                                                                               \
    CC_EVALUATE_CALL(HH, e);                                                                                           \
  }                                                                                                                    \
  __global__ void __launch_bounds__(256, 2) HipClassicControlMountainCarEnvEvaluate_H##HH(                             \
      const float *state_arr, const int *action_arr, const int *done_arr, const float *reward_arr,                     \
      const float *observation_arr, float min_position, float max_position, float max_speed, float goal_position,      \
      float goal_velocity, float force, float gravity, const int *env_timestep_arr, int episode_length, int n_envs,    \
      CC_EVALUATE_PARAMS) {                                                                                            \
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];                                                     \
    const CcMountainCar e{min_position, max_position, max_speed, goal_position, goal_velocity, force, gravity};        \
    CC_EVALUATE_CALL(HH, e);                                                                                           \
  }
CC_EVALUATE_ENTRIES(32)
CC_EVALUATE_ENTRIES(64)

// one episode of every replica of a Box env with the deterministic actor inside the kernel (cc_evaluate_actor_impl): the
// env's step arguments (read only), then what the evaluation takes
#define CC_EVALUATE_ACTOR_PARAMS                                                                                       \
  uint32_t *rng_state, int stream_tag, int ticks, const float *actor, int hidden, float action_scale,                  \
      float action_bias, float *ou_state, float damping, float stddev, float scale, float *eval_reward_sum,            \
      int *eval_steps, int *eval_done, float *mean_trace, float *action_trace
#define CC_EVALUATE_ACTOR_CALL(HH, ENV)                                                                                \
  cc_evaluate_actor_impl<HH>(ENV, state_arr, observation_arr, env_timestep_arr, episode_length, n_envs, rng_state,     \
                             stream_tag, ticks, cc_lds, actor, hidden, action_scale, action_bias, ou_state, damping,   \
                             stddev, scale, eval_reward_sum, eval_steps, eval_done, mean_trace, action_trace)
#define CC_EVALUATE_ACTOR_ENTRIES(HH)                                                                                  \
  __global__ void __launch_bounds__(256, 2) HipClassicControlContinuousMountainCarEnvEvaluate_A##HH(                   \
      const float *state_arr, const float *action_arr, const int *done_arr, const float *reward_arr,                   \
      const float *observation_arr, float min_action, float max_action, float min_position, float max_position,        \
      float max_speed, float goal_position, float goal_velocity, float power, const int *env_timestep_arr,             \
      int episode_length, int n_envs, CC_EVALUATE_ACTOR_PARAMS) {                                                      \
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];                                                     \
    const CcContinuousMountainCar e{min_action, max_action, min_position, max_position,                                \
                                    max_speed, goal_position, goal_velocity, power};                                   \
    CC_EVALUATE_ACTOR_CALL(HH, e);                                                                                     \
  }                                                                                                                    \
  __global__ void __launch_bounds__(256, 2) HipClassicControlPendulumEnvEvaluate_A##HH(                                \
      const float *state_arr, const float *action_arr, const int *done_arr, const float *reward_arr,                   \
      const float *observation_arr, const int *env_timestep_arr, int episode_length, int n_envs,                       \
      CC_EVALUATE_ACTOR_PARAMS) {                                                                                      \
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];                                                     \
    const CcPendulum e{};                                                                                              \
    CC_EVALUATE_ACTOR_CALL(HH, e);                                                                                     \
  }
CC_EVALUATE_ACTOR_ENTRIES(32)
CC_EVALUATE_ACTOR_ENTRIES(64)

}  // extern "C"
