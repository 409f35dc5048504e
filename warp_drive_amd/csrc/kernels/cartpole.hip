// cartpole.hip -- ClassicControl CartPole Euler step (BASELINE config 5: the
// HBM-roofline ceiling microbenchmark, 68 algorithmic bytes per env-step).
//
// Follows the reference's only device implementation,
// example_envs/single_agent/classic_control/cartpole/cartpole_step_numba.py:5-83
// (its CPU step is third-party gym.CartPoleEnv, absent here).  Numba's type
// inference is restated literally: float32 state and scalars, but the Python
// literal 4.0/3.0 makes the pole-acceleration denominator -- and everything
// downstream of thetaacc -- float64 (:56-60, :63-66).
//
// MI355X mapping: one THREAD per replica (the reference uses one 1-thread block per
// replica, cartpole.py:139-141), 16-byte state/obs accesses, grid-stride, and an
// optional `ticks` loop so many ticks fuse into one launch (a single tick at
// E = 100 000 moves 6.8 MB -- under 1 us of HBM time, i.e. launch-bound).
#include "wd_common.h"
#include "cartpole_common.h"

namespace {

// BATCH: the four `*_batch` pointers are given (every tick recorded) -- a compile-time copy of the loop for each case, so
// that the tick carries no "is there a batch" branches
struct CpTrue { static constexpr bool value = true, fast = false; };
struct CpFalse { static constexpr bool value = false, fast = false; };
struct CpTrueFast { static constexpr bool value = true, fast = true; };  // a middle tick with cp_euler<true>

// A2: exactly two actions (Cartpole's own action space), known at compile time
template <int H, bool BATCH, bool A2 = false>
__device__ __forceinline__ void cp_tick_impl(float *cp_weights,
    float4 *state_arr, int *action_arr, int *done_arr,
    float *reward_arr, float4 *observation_arr, float gravity,
    float masspole, float total_mass, float length, float polemass_length, float force_mag,
    float tau, float theta_threshold_radians, float x_threshold,
    int *env_timestep_arr, int episode_length, int n_envs, uint32_t *rng_state,
    const float *__restrict__ probs, int n_actions, const void *reset_table, int n_reset_arrays,
    int stream_tag, int ticks, float4 *obs_batch, int *action_batch, float *reward_batch, int *done_batch,
    const float *policy, int hidden, int invariant_divide_ok) {
  const CpPhysics p{gravity, masspole, total_mass, length, polemass_length, force_mag, tau,
                    theta_threshold_radians, x_threshold, 1.0f / total_mass};
  const wd_reset_entry *table = (const wd_reset_entry *)reset_table;
  const uint32_t k0 = rng_state[0], k1 = rng_state[1];
  if (H > 0) {
    const int n_w = rp_policy_floats(4, H, n_actions);
    for (int i = threadIdx.x; i < n_w; i += blockDim.x) cp_weights[i] = policy[i];
    __syncthreads();
  }
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < n_envs; env += gridDim.x * blockDim.x) {
    int t = env_timestep_arr[env];
    float4 s = state_arr[env];
    const uint32_t epoch0 = rng_state[WD_RNG_HEADER + env];
    wd_u4 blk = wd_u4{0u, 0u, 0u, 0u};   // the Philox block of four consecutive ticks (wd_tick_draw)
    uint32_t blk_quad = 0xffffffffu;
    const float *row = probs + (long)env * n_actions;
    // The running float32 sums of the (fixed) probabilities, once per launch and in registers: a load
    // inside the tick loop would wait for every store issued before it (the memory counters return in
    // order) -- 2.9 us per tick at 100 000 replicas instead of 0.5.
    // The rows a finished replica is restored from, preloaded ONCE (the usual registration: `state` and the
    // observation, four floats each).  A random policy ends a Cartpole episode every ~20 ticks, so some lane of a
    // wavefront finishes on nearly every tick; the restore used to LOAD the registered rows inside the tick loop
    // (and reload the state): 12 loads per tick and wavefront, each waiting for every store issued before it (the
    // memory counters return in order) -- 70 % of the wavefronts' cycles were waits (profiles/r04_pmc_mix_cartpole_T50.txt).
    wd_reset_entry ent0 = wd_reset_entry{nullptr, nullptr, 0, 0}, ent1 = ent0;
    uint4 row0 = make_uint4(0u, 0u, 0u, 0u), row1 = row0;
    bool cached = (n_reset_arrays >= 1) && (n_reset_arrays <= 2);
    if (cached) {
      ent0 = table[0];
      ent1 = (n_reset_arrays == 2) ? table[1] : table[0];
      cached = (ent0.row_elems == 4) && (ent1.row_elems == 4) &&
               ((size_t)ent0.data == (size_t)state_arr || (size_t)ent1.data == (size_t)state_arr);
      if (cached) {
        row0 = ((const uint4 __attribute__((address_space(1))) *)ent0.ref)[env];
        row1 = ((const uint4 __attribute__((address_space(1))) *)ent1.ref)[env];
      }
    }
    float cumv[CP_MAX_REG_ACTIONS];
    if (H == 0) {
      float cum = 0.0f;
#pragma unroll
      for (int i = 0; i < CP_MAX_REG_ACTIONS; ++i) {
        if (i < n_actions) cum = (i == 0) ? row[0] : cum + row[i];
        cumv[i] = cum;
      }
    }
    // Every value loaded above is consumed HERE, before the tick loop: the wait for a load whose first use is inside
    // the loop is placed inside the loop, executed on every tick, and also waits for every store of the previous tick.
    asm volatile("" : "+v"(t), "+v"(s.x), "+v"(s.y), "+v"(s.z), "+v"(s.w));
    asm volatile("" : "+v"(row0.x), "+v"(row0.y), "+v"(row0.z), "+v"(row0.w), "+v"(row1.x), "+v"(row1.y), "+v"(row1.z), "+v"(row1.w));
#pragma unroll
    for (int i = 0; i < CP_MAX_REG_ACTIONS; ++i) asm volatile("" : "+v"(cumv[i]));
    // per-lane byte offsets of this replica's row in the 16-byte and the 4-byte arrays (constant over the ticks); the
    // record arrays' row k starts n_envs elements further on every tick: a scalar pointer
    const uint32_t off16 = 16u * (uint32_t)env, off4 = 4u * (uint32_t)env;
    const unsigned char *ob_k = (const unsigned char *)obs_batch, *ab_k = (const unsigned char *)action_batch,
                        *rb_k = (const unsigned char *)reward_batch, *db_k = (const unsigned char *)done_batch;
    // a batch launch whose restore rows sit in registers keeps the per-tick arrays, the state and the restored rows in
    // registers until the LAST tick: every one of those addresses is written again then (the per-tick arrays and the
    // state on the last tick of every replica, the registered rows = state + observation), so what memory holds after
    // the launch is the same, and a replica that finishes mid-launch costs two register moves instead of seven stores
    // (`cached` is the same in every lane -- the table is one per launch -- but it was computed from vector loads: say so,
    // or the two loops below become divergent control flow and the record pointers vector registers)
    const bool lazy = BATCH && (__builtin_amdgcn_readfirstlane(cached ? 1 : 0) != 0);
    // the state a finished replica restarts from (the preloaded row registered for `state`)
    const uint4 sr0 = ((size_t)ent0.data == (size_t)state_arr) ? row0 : row1;
    const float4 s_restart = make_float4(__uint_as_float(sr0.x), __uint_as_float(sr0.y), __uint_as_float(sr0.z), __uint_as_float(sr0.w));

    // ---- one tick.  MID (compile time): a tick of a `lazy` launch that is not its last -- four record stores, the Euler
    // step, and a finished replica restarts by five selects: no per-tick-array stores, no branch on "finished", no
    // divergent code at all.  Otherwise the general tick (`last` = the launch's last tick).
    auto tick = [&](int k, auto mid_tag, bool last) __attribute__((always_inline)) {
      constexpr bool MID = decltype(mid_tag)::value;
      // ---- sample (random.cu:51-85): inverse CDF on a running float32 sum
      const float u = wd_u01_open_closed(wd_tick_draw((uint32_t)env, epoch0 + (uint32_t)k, (uint32_t)stream_tag, k0, k1,
                                                      blk, blk_quad));
      if (H > 0) cp_policy_cum<(H > 0 ? H : 4)>(cp_weights, s, n_actions, cumv);  // live policy: THIS tick's observation
      int cnt = 0;
      if (A2 || n_actions == 2) {  // (uniform) two compares instead of eight masked ones
        cnt = ((cumv[0] < u) ? 1 : 0) + ((cumv[1] < u) ? 1 : 0);
      } else if (n_actions <= CP_MAX_REG_ACTIONS) {
#pragma unroll
        for (int i = 0; i < CP_MAX_REG_ACTIONS; ++i) cnt += (i < n_actions && cumv[i] < u) ? 1 : 0;
      } else {
        float cum = 0.0f;
        for (int i = 0; i < n_actions; ++i) {
          cum = (i == 0) ? row[0] : cum + row[i];
          cnt += (cum < u) ? 1 : 0;
        }
      }
      const int a = min(cnt, (A2 ? 2 : n_actions) - 1);
      // ---- step
      if (BATCH) cp_store_s(ob_k, off16, s);  // the observation this action was sampled on
      t += 1;
      const bool terminated = cp_euler<decltype(mid_tag)::fast>(s, a, p);
      const bool fin = (t == episode_length) || terminated;
      if (BATCH) {
        cp_store_s(ab_k, off4, a);
        cp_store_s(rb_k, off4, 1.0f);
        cp_store_s(db_k, off4, fin ? 1 : 0);
        ob_k += 16 * (size_t)n_envs; ab_k += 4 * (size_t)n_envs; rb_k += 4 * (size_t)n_envs; db_k += 4 * (size_t)n_envs;
      }
      if (MID) {
        t = fin ? 0 : t;
        s.x = fin ? s_restart.x : s.x; s.y = fin ? s_restart.y : s.y;
        s.z = fin ? s_restart.z : s.z; s.w = fin ? s_restart.w : s.w;
        return;
      }
      // (untracked stores, wd_common.h: a store the compiler tracks inside the loop costs a wait for ALL stores on
      // every trip, executed or not.  The one place that reads such an address back -- the restore of a replica whose
      // reset rows were not preloaded -- drains the counter itself first.)
      if (!BATCH || last || (fin && !lazy)) {
        cp_store_s(action_arr, off4, a);
        cp_store_s(observation_arr, off16, s);
        cp_store_s(reward_arr, off4, 1.0f);
        cp_store_s(done_arr, off4, fin ? 1 : 0);
      }
      if (last || (fin && !lazy)) cp_store_s(state_arr, off16, s);  // otherwise the state stays in registers
      // ---- reset in place (reset.cu:9-75 for every registered array); `_done_` stays set
      if (fin) {
        t = 0;
        if (cached) {  // stores only
          if (last || !lazy) {
            // (after the untracked stores above to the same rows: stores of one wavefront to one address stay in order)
            wd_store_untracked((float4 *)ent0.data + env, make_float4(__uint_as_float(row0.x), __uint_as_float(row0.y), __uint_as_float(row0.z), __uint_as_float(row0.w)));
            if (n_reset_arrays == 2)
              wd_store_untracked((float4 *)ent1.data + env, make_float4(__uint_as_float(row1.x), __uint_as_float(row1.y), __uint_as_float(row1.z), __uint_as_float(row1.w)));
          }
          s = s_restart;
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the untracked stores above have left
          for (int r = 0; r < n_reset_arrays; ++r) {
            const wd_reset_entry ent = table[r];
            const long base = (long)env * ent.row_elems;
            for (int i = 0; i < ent.row_elems; ++i) ent.data[base + i] = ent.ref[base + i];
          }
          s = state_arr[env];
          // the reload is consumed HERE, inside the rare branch: otherwise the wait for it lands at the top
          // of the tick loop, where it also waits for every store of the previous tick
          asm volatile("" : "+v"(s.x), "+v"(s.y), "+v"(s.z), "+v"(s.w));
        }
      }
    };
    if (lazy) {  // (uniform) every tick but the last: the branch-free body
      // cp_euler<true>'s preconditions, checked ONCE per launch and wavefront: the division shortcut is proved for this total
      // mass in one binade (host flag) and the masses carry that proof over the whole dividend window (cp_fast_masses_ok), a
      // running replica's angle stays inside 0.75 (threshold), and so do the angles the wavefront starts from and
      // restarts from.  A middle tick then only ever sees the restart state or a state that did not terminate.
      const bool small = (p.theta_threshold_radians <= 0.75f) && (fabsf(s.z) <= 0.75f) && (fabsf(s_restart.z) <= 0.75f);
      const bool mass_ok = cp_fast_masses_ok(p.masspole, p.total_mass);
      const bool fast = (invariant_divide_ok != 0) && mass_ok && (__ballot(!small) == 0ull);  // (wave-uniform)
      if (fast) for (int k = 0; k < ticks - 1; ++k) tick(k, CpTrueFast{}, false);
      else for (int k = 0; k < ticks - 1; ++k) tick(k, CpTrue{}, false);
      tick(ticks - 1, CpFalse{}, true);
    } else {
      for (int k = 0; k < ticks; ++k) tick(k, CpFalse{}, k == ticks - 1);
    }
    env_timestep_arr[env] = t;
    rng_state[WD_RNG_HEADER + env] = epoch0 + (uint32_t)ticks;
  }
}

// ---- evaluation: ONE episode of every replica in one launch (the ...EnvEvaluate_H<H> entries), greedy or sampled; the
// Cartpole counterpart of classic_control.hip::cc_evaluate_impl.  The greedy scan reads cp_policy_probs, the sampled
// draw counts on the running sums formed from the same probabilities (cartpole_common.h, rollout_policy.h).
// One lane per replica: the state (= the observation the network reads, as in cp_tick_impl) and the timestep are loaded
// once, then at most `ticks` ticks of (network -> action -> cp_euler<false>), stopping at the first finished tick; the
// terminal tick counts (sum += 1, steps += 1 before the test).  use_argmax: the first maximum of the probabilities
// (the standalone sampler's strict-'<' scan); otherwise the counting draw with the Philox counters of the
// fixed-probability tick.  WRITES eval_reward_sum / eval_steps / eval_done [n_envs] (eval_done: 1, or 0 when `ticks` ran
// out first), row k of `action_trace` [ticks, n_envs] (optional) while the replica runs and, in sampled mode only, the
// replica's epoch word += steps -- nothing else.  No restart: no reset table.  The guard is the rollout entries'.
template <int H>
__device__ __forceinline__ void cp_evaluate_impl(float *cp_weights, const float4 *state_arr, const CpPhysics &p,
                                                 const int *env_timestep_arr, int episode_length, int n_envs,
                                                 uint32_t *rng_state, int n_actions, int stream_tag, int ticks,
                                                 const float *policy, int hidden, int use_argmax,
                                                 float *eval_reward_sum, int *eval_steps, int *eval_done,
                                                 int *action_trace) {
  if (hidden != H || n_actions < 1 || n_actions > CP_MAX_REG_ACTIONS || policy == nullptr) return;  // (uniform)
  const int n_w = rp_policy_floats(4, H, n_actions);
  for (int i = threadIdx.x; i < n_w; i += blockDim.x) cp_weights[i] = policy[i];
  __syncthreads();
  const uint32_t k0 = rng_state[0], k1 = rng_state[1];
  const bool greedy = use_argmax > 0;  // (uniform)
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < n_envs; env += gridDim.x * blockDim.x) {
    int t = env_timestep_arr[env];
    float4 s = state_arr[env];
    uint32_t epoch0 = rng_state[WD_RNG_HEADER + env];
    // consumed HERE, before the tick loop (as in cp_tick_impl: no wait for a load inside the loop)
    asm volatile("" : "+v"(t), "+v"(epoch0), "+v"(s.x), "+v"(s.y), "+v"(s.z), "+v"(s.w));
    wd_u4 blk = wd_u4{0u, 0u, 0u, 0u};
    uint32_t blk_quad = 0xffffffffu;
    float sum = 0.0f;
    int steps = 0, done = 0;
    int *trace = action_trace ? action_trace + env : nullptr;
    for (int k = 0; k < ticks; ++k) {
      float prob[CP_MAX_REG_ACTIONS];
      cp_policy_probs<H>(cp_weights, s, n_actions, prob);
      int a = 0;
      if (greedy) {
        a = rp_first_maximum(prob, n_actions);
      } else {
        const float u = wd_u01_open_closed(wd_tick_draw((uint32_t)env, epoch0 + (uint32_t)k, (uint32_t)stream_tag, k0, k1,
                                                        blk, blk_quad));
        float cum = 0.0f;
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < CP_MAX_REG_ACTIONS; ++i) {
          if (i < n_actions) cum = (i == 0) ? prob[0] : cum + prob[i];
          cnt += (i < n_actions && cum < u) ? 1 : 0;
        }
        a = min(cnt, n_actions - 1);
      }
      if (trace) {
        wd_store_untracked(trace, a);  // (untracked: the loop never reads it back)
        trace += n_envs;
      }
      t += 1;
      const bool terminated = cp_euler<false>(s, a, p);
      sum += 1.0f;
      steps += 1;
      done = ((t == episode_length) || terminated) ? 1 : 0;
      if (done) break;
    }
    eval_reward_sum[env] = sum;
    eval_steps[env] = steps;
    eval_done[env] = done;
    if (!greedy) rng_state[WD_RNG_HEADER + env] = epoch0 + (uint32_t)steps;
  }
}

}  // namespace

extern "C" {

// Exhaustive proof for ONE divisor c (the env's total mass) that cp_div_invariant(x, c, RN(1 / c)) == x / c for every
// float32 x of one binade, both signs (2^24 values).  Every other x follows by scaling ONLY while x / c stays a normal
// float32: the proof says nothing about a quotient that overflows or is subnormal, so the tick kernels use the form only
// with this proof AND masses that keep the quotients of their dividend window normal (cartpole_common.h::
// cp_fast_masses_ok).  `ok` (preset to 1 by the host) is cleared on the first mismatch (a test hands it a reciprocal that
// is one ulp off: it must notice).  Run once per total mass (envs/cartpole.py::invariant_divide_ok).
__global__ void HipCartPoleVerifyInvariantDivide(float c, float y, int *ok) {  // y: RN(1 / c), formed by the host
  if (y != 1.0f / c && threadIdx.x == 0 && blockIdx.x == 0) *ok = 0;  // (not what the tick kernels use: 1.0f / total_mass)
  // bits 0 .. 22: the significand; bit 23: a second binade (x 2^40: the scaling argument, spot-checked); bit 24: the sign
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < (1u << 25); i += gridDim.x * blockDim.x) {
    const float m = __uint_as_float(0x3f800000u | (i & 0x7fffffu) | ((i >> 24) << 31));
    const float x = ((i >> 23) & 1u) ? m * 0x1.0p40f : m;
    const float want = x / c, got = cp_div_invariant(x, c, y);
    if (__float_as_uint(want) != __float_as_uint(got)) *ok = 0;
  }
}

// cp_sincos_small against wd_np_sincosf for every float32 of [-0.75, 0.75] (the test of the claim in its comment)
__global__ void HipCartPoleVerifySmallAngle(int *ok) {
  const uint32_t top = __float_as_uint(0.75f);
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= top; i += gridDim.x * blockDim.x) {
    const float xs[2] = {__uint_as_float(i), __uint_as_float(i | 0x80000000u)};
    for (int k = 0; k < 2; ++k) {
      float s0, c0, s1, c1;
      wd_np_sincosf(xs[k], s0, c0);
      cp_sincos_small(xs[k], s1, c1);
      if (__float_as_uint(s0) != __float_as_uint(s1) || __float_as_uint(c0) != __float_as_uint(c1)) *ok = 0;
    }
  }
}

__global__ void HipClassicControlCartPoleEnvStep(
    float4 *__restrict__ state_arr, const int *__restrict__ action_arr, int *__restrict__ done_arr,
    float *__restrict__ reward_arr, float4 *__restrict__ observation_arr, float gravity,
    float masspole, float total_mass, float length, float polemass_length, float force_mag,
    float tau, float theta_threshold_radians, float x_threshold,
    int *__restrict__ env_timestep_arr, int episode_length, int n_envs) {
  const CpPhysics p{gravity, masspole, total_mass, length, polemass_length, force_mag, tau,
                    theta_threshold_radians, x_threshold, 1.0f / total_mass};
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < n_envs; env += gridDim.x * blockDim.x) {
    const int t = env_timestep_arr[env] + 1;
    env_timestep_arr[env] = t;
    float4 s = state_arr[env];
    const bool terminated = cp_euler(s, action_arr[env], p);
    state_arr[env] = s;
    observation_arr[env] = s;
    reward_arr[env] = 1.0f;
    if (t == episode_length || terminated) done_arr[env] = 1;
  }
}

__global__ void HipClassicControlCartPoleEnvTick(
    float4 *state_arr, int *action_arr, int *done_arr,
    float *reward_arr, float4 *observation_arr, float gravity,
    float masspole, float total_mass, float length, float polemass_length, float force_mag,
    float tau, float theta_threshold_radians, float x_threshold,
    int *env_timestep_arr, int episode_length, int n_envs, uint32_t *rng_state,
    const float *__restrict__ probs, int n_actions, const void *reset_table, int n_reset_arrays,
    int stream_tag, int ticks, float4 *obs_batch, int *action_batch, float *reward_batch, int *done_batch,
    const float *policy, int hidden, int invariant_divide_ok) {
  if (obs_batch && n_actions == 2)  // the recorded two-action rollout (configs[4]): sizes folded
    cp_tick_impl<0, true, true>(nullptr, state_arr, action_arr, done_arr, reward_arr, observation_arr, gravity, masspole, total_mass, length, polemass_length, force_mag, tau, theta_threshold_radians, x_threshold, env_timestep_arr, episode_length, n_envs, rng_state, probs, n_actions, reset_table, n_reset_arrays, stream_tag, ticks, obs_batch, action_batch, reward_batch, done_batch, policy, hidden, invariant_divide_ok);
  else if (obs_batch)
    cp_tick_impl<0, true>(nullptr, state_arr, action_arr, done_arr, reward_arr, observation_arr, gravity, masspole, total_mass, length, polemass_length, force_mag, tau, theta_threshold_radians, x_threshold, env_timestep_arr, episode_length, n_envs, rng_state, probs, n_actions, reset_table, n_reset_arrays, stream_tag, ticks, obs_batch, action_batch, reward_batch, done_batch, policy, hidden, invariant_divide_ok);
  else
    cp_tick_impl<0, false>(nullptr, state_arr, action_arr, done_arr, reward_arr, observation_arr, gravity, masspole, total_mass, length, polemass_length, force_mag, tau, theta_threshold_radians, x_threshold, env_timestep_arr, episode_length, n_envs, rng_state, probs, n_actions, reset_table, n_reset_arrays, stream_tag, ticks, obs_batch, action_batch, reward_batch, done_batch, policy, hidden, invariant_divide_ok);
}

// the rollout with a live policy (weights in dynamic LDS); `hidden` must equal the entry's width and n_actions fit the
// registers, as classic_control.hip::cc_rollout: otherwise the launch does nothing
#define WD_CP_ROLLOUT(HH)                                                                          \
  __global__ void __launch_bounds__(256, 2) HipClassicControlCartPoleEnvRollout_H##HH(             \
    float4 *state_arr, int *action_arr, int *done_arr, \
    float *reward_arr, float4 *observation_arr, float gravity, \
    float masspole, float total_mass, float length, float polemass_length, float force_mag, \
    float tau, float theta_threshold_radians, float x_threshold, \
    int *env_timestep_arr, int episode_length, int n_envs, uint32_t *rng_state, \
    const float *__restrict__ probs, int n_actions, const void *reset_table, int n_reset_arrays, \
    int stream_tag, int ticks, float4 *obs_batch, int *action_batch, float *reward_batch, int *done_batch, \
    const float *policy, int hidden, int invariant_divide_ok) {           \
    extern __shared__ __attribute__((aligned(16))) float cp_lds[];                                 \
    /* (uniform) another width or more actions than cp_policy_cum keeps in registers: no tick */   \
    if (hidden != HH || n_actions < 1 || n_actions > CP_MAX_REG_ACTIONS || policy == nullptr) return; \
    if (obs_batch)                                                                                 \
      cp_tick_impl<HH, true>(cp_lds, state_arr, action_arr, done_arr, reward_arr, observation_arr, gravity, masspole, total_mass, length, polemass_length, force_mag, tau, theta_threshold_radians, x_threshold, env_timestep_arr, episode_length, n_envs, rng_state, probs, n_actions, reset_table, n_reset_arrays, stream_tag, ticks, obs_batch, action_batch, reward_batch, done_batch, policy, hidden, invariant_divide_ok); \
    else                                                                                           \
      cp_tick_impl<HH, false>(cp_lds, state_arr, action_arr, done_arr, reward_arr, observation_arr, gravity, masspole, total_mass, length, polemass_length, force_mag, tau, theta_threshold_radians, x_threshold, env_timestep_arr, episode_length, n_envs, rng_state, probs, n_actions, reset_table, n_reset_arrays, stream_tag, ticks, obs_batch, action_batch, reward_batch, done_batch, policy, hidden, invariant_divide_ok); \
  }
WD_CP_ROLLOUT(32)
WD_CP_ROLLOUT(64)

// one episode of every replica with the policy inside the kernel (cp_evaluate_impl): the step's arguments (read only),
// then what the evaluation takes
#define WD_CP_EVALUATE(HH)                                                                         \
  __global__ void __launch_bounds__(256, 2) HipClassicControlCartPoleEnvEvaluate_H##HH(            \
    const float4 *state_arr, const int *action_arr, const int *done_arr, const float *reward_arr,  \
    const float4 *observation_arr, float gravity, float masspole, float total_mass, float length,  \
    float polemass_length, float force_mag, float tau, float theta_threshold_radians,              \
    float x_threshold, const int *env_timestep_arr, int episode_length, int n_envs,                \
    uint32_t *rng_state, int n_actions, int stream_tag, int ticks, const float *policy,            \
    int hidden, int use_argmax, float *eval_reward_sum, int *eval_steps, int *eval_done,           \
    int *action_trace) {                                                                           \
    extern __shared__ __attribute__((aligned(16))) float cp_lds[];                                 \
    const CpPhysics p{gravity, masspole, total_mass, length, polemass_length, force_mag, tau,      \
                      theta_threshold_radians, x_threshold, 1.0f / total_mass};                    \
    cp_evaluate_impl<HH>(cp_lds, state_arr, p, env_timestep_arr, episode_length, n_envs,           \
                         rng_state, n_actions, stream_tag, ticks, policy, hidden, use_argmax,      \
                         eval_reward_sum, eval_steps, eval_done, action_trace);                    \
  }
WD_CP_EVALUATE(32)
WD_CP_EVALUATE(64)

}  // extern "C"
