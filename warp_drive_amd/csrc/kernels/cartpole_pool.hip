// cartpole_pool.hip -- the T-tick Cartpole rollout for an env with a RESET POOL (wd_kernels_cp_pool.hsaco):
// HipClassicControlCartPoleEnvRollout_P (fixed probabilities) and ..._P_H32 / _P_H64 (the policy network inside the
// kernel).  They are cartpole.hip's T-tick rollout (same step cp_euler, same network cp_policy_cum, same Philox counters
// of the action draw: cartpole_common.h) with the restart of a finished replica taken from the pool inside the kernel --
// what reset_when_done_fused + reset_when_done_from_pool + undo do in three launches per tick, restated from
// classic_control.hip::cc_tick_impl:
//   * every array of the reset table is restored: for a pooled Cartpole that is `observations` alone (`state` has no
//     saved copy: envs/cartpole.py registers it with save_copy_and_apply_at_reset = False), and the entries serve
//     exactly that table -- one array, the observation rows, four floats each; anything else: no tick (the guard);
//   * `state` becomes pool row min((int)(p * n_pool), n_pool - 1), p = (float)(rnd.x >> 8) * 2^-24,
//     rnd = Philox({env, pool_epoch, 0x706f6f6c, 2}, the pool generator's key words);
//   * pool_epoch advances on a restart only and is written back once per launch;
//   * the time step is cleared; `_done_` reports the launch's last tick.
// STATE AND OBSERVATION ARE TWO THINGS HERE.  cartpole.hip keeps one float4 (a Cartpole observation is its state).  After
// a pooled restart the observation -- what the network reads and what row k of `obs_batch` records -- is the SAVED COPY
// of the observation row, while the state is the pool row (the per-tick plan feeds the framework forward exactly that);
// the lane carries both, and they coincide again after the next step.  For the same reason the launch starts from the
// observation rows memory holds, not from the state.
// Nothing but the batch rows is written inside the tick loop: every other address (state, observations, sampled_actions,
// rewards, _done_, _timestep_, both generators' epoch words) is written once, after the last tick, with what the
// per-tick plan would have left there.
// WHERE THE POOL IS (pool_in_lds, uniform per launch, the host's choice: envs/cartpole.py::pool_rollout_lds_bytes):
//   1: the block copies all n_pool rows (16 bytes each) into dynamic LDS behind the weights; a restart is one
//      ds_read_b128, which does not wait for the record stores;
//   0: the rows stay in global memory (a 10 000-row pool is 160 KB); the load sits inside the wave-level "did any
//      lane finish" branch and is consumed there, so only a wavefront that restarts waits for its stores.
// FAST TICKS.  cp_euler<true> needs |theta| <= 0.75 for every state a tick can see: with a pool that includes EVERY POOL
// ROW, whatever wrote them.  The staging loop looks at every row's angle and the block agrees on the answer
// (__syncthreads_or), so `fast` is decided once per launch and uniformly; a launch whose pool stays in global memory
// runs the general tick (scanning 160 KB per block costs more than the shortcut saves).
#include "wd_common.h"
#include "cartpole_common.h"

namespace {

struct CpPoolArgs {
  uint32_t *pool_rng;   // the resetter's generator: 4 header words (the key in the first two), then one epoch per replica
  const float *pool;    // [n_pool, 4] float32
  int n_pool;
  int pool_in_lds;
};

// which cp_euler a launch's ticks run (a compile-time copy of the tick loop each)
struct CpPoolFast { static constexpr bool fast = true; };
struct CpPoolGeneral { static constexpr bool fast = false; };

template <int H>
__device__ __forceinline__ void cp_pool_rollout(float *lds,
    float4 *state_arr, int *action_arr, int *done_arr, float *reward_arr, float4 *observation_arr, const CpPhysics &p,
    int *env_timestep_arr, int episode_length, int n_envs, uint32_t *rng_state, const float *__restrict__ probs,
    int n_actions, const void *reset_table, int n_reset_arrays, int stream_tag, int ticks, float4 *obs_batch,
    int *action_batch, float *reward_batch, int *done_batch, const float *policy, int hidden, int invariant_divide_ok,
    const CpPoolArgs &pa) {
  // ---- the guard (uniform: kernel arguments and one table entry every lane reads from the same address)
  if (hidden != H || n_actions < 1 || n_actions > CP_MAX_REG_ACTIONS || (H > 0 && policy == nullptr) || ticks < 1 ||
      pa.n_pool < 1 || pa.pool == nullptr || pa.pool_rng == nullptr || n_reset_arrays != 1 || reset_table == nullptr)
    return;
  const wd_reset_entry ent = *(const wd_reset_entry *)reset_table;
  if ((size_t)ent.data != (size_t)observation_arr || ent.row_elems != 4) return;
  const int n_pool = pa.n_pool;
  const bool staged = pa.pool_in_lds != 0;
  const int n_w = (H > 0) ? rp_policy_floats(4, H, n_actions) : 0;
  float *cp_weights = lds;
  float4 *pool_lds = (float4 *)(lds + ((n_w + 3) & ~3));
  const float4 *pool4 = (const float4 *)pa.pool;
  if (H > 0)
    for (int i = threadIdx.x; i < n_w; i += blockDim.x) cp_weights[i] = policy[i];
  bool pool_small = false;
  if (staged) {
    int wide = 0;
    for (int i = threadIdx.x; i < n_pool; i += blockDim.x) {
      const float4 r = pool4[i];
      pool_lds[i] = r;
      wide |= (fabsf(r.z) <= 0.75f) ? 0 : 1;   // (a NaN angle counts as wide)
    }
    pool_small = __syncthreads_or(wide) == 0;
  } else if (H > 0) {
    __syncthreads();
  }
  const uint32_t k0 = rng_state[0], k1 = rng_state[1];
  const uint32_t pk0 = pa.pool_rng[0], pk1 = pa.pool_rng[1];
  const bool batch = obs_batch != nullptr;
  const bool mass_ok = cp_fast_masses_ok(p.masspole, p.total_mass);
  const bool launch_fast = (invariant_divide_ok != 0) && mass_ok && (p.theta_threshold_radians <= 0.75f) && pool_small;
  for (int env = blockIdx.x * blockDim.x + threadIdx.x; env < n_envs; env += gridDim.x * blockDim.x) {
    int t = env_timestep_arr[env];
    float4 s = state_arr[env];
    float4 o = observation_arr[env];
    const uint32_t epoch0 = rng_state[WD_RNG_HEADER + env];
    uint32_t pool_epoch = pa.pool_rng[WD_RNG_HEADER + env];
    uint4 orow = ((const uint4 __attribute__((address_space(1))) *)ent.ref)[env];   // the saved observation row
    wd_u4 blk = wd_u4{0u, 0u, 0u, 0u};   // the Philox block of four consecutive ticks (wd_tick_draw)
    uint32_t blk_quad = 0xffffffffu;
    float cumv[CP_MAX_REG_ACTIONS];
    if (H == 0) {
      const float *row = probs + (long)env * n_actions;
      float cum = 0.0f;
#pragma unroll
      for (int i = 0; i < CP_MAX_REG_ACTIONS; ++i) {
        if (i < n_actions) cum = (i == 0) ? row[0] : cum + row[i];
        cumv[i] = cum;
      }
    }
    // every value loaded above is consumed HERE: a wait placed inside the tick loop would run on every tick and also
    // wait for every record store of the tick before (cartpole.hip::cp_tick_impl)
    asm volatile("" : "+v"(t), "+v"(s.x), "+v"(s.y), "+v"(s.z), "+v"(s.w), "+v"(o.x), "+v"(o.y), "+v"(o.z), "+v"(o.w));
    asm volatile("" : "+v"(orow.x), "+v"(orow.y), "+v"(orow.z), "+v"(orow.w), "+v"(pool_epoch));
    if (H == 0) {
#pragma unroll
      for (int i = 0; i < CP_MAX_REG_ACTIONS; ++i) asm volatile("" : "+v"(cumv[i]));
    }
    const float4 o_restart = make_float4(__uint_as_float(orow.x), __uint_as_float(orow.y), __uint_as_float(orow.z),
                                         __uint_as_float(orow.w));
    const uint32_t off16 = 16u * (uint32_t)env, off4 = 4u * (uint32_t)env;
    const unsigned char *ob_k = (const unsigned char *)obs_batch, *ab_k = (const unsigned char *)action_batch,
                        *rb_k = (const unsigned char *)reward_batch, *db_k = (const unsigned char *)done_batch;
    int a = 0;
    bool fin = false;
    auto tick = [&](int k, auto fast_tag) __attribute__((always_inline)) {
      // ---- sample: the unpooled entries' draw, the live policy on the OBSERVATION the lane holds
      const float u = wd_u01_open_closed(wd_tick_draw((uint32_t)env, epoch0 + (uint32_t)k, (uint32_t)stream_tag, k0, k1,
                                                      blk, blk_quad));
      if (H > 0) cp_policy_cum<(H > 0 ? H : 4)>(cp_weights, o, n_actions, cumv);
      int cnt = 0;
      if (n_actions == 2) {  // (uniform)
        cnt = ((cumv[0] < u) ? 1 : 0) + ((cumv[1] < u) ? 1 : 0);
      } else {
#pragma unroll
        for (int i = 0; i < CP_MAX_REG_ACTIONS; ++i) cnt += (i < n_actions && cumv[i] < u) ? 1 : 0;
      }
      a = min(cnt, n_actions - 1);
      // ---- step
      if (batch) cp_store_s(ob_k, off16, o);  // the observation this action was sampled on
      t += 1;
      const bool terminated = cp_euler<decltype(fast_tag)::fast>(s, a, p);
      fin = (t == episode_length) || terminated;
      if (batch) {  // (uniform)
        cp_store_s(ab_k, off4, a);
        cp_store_s(rb_k, off4, 1.0f);
        cp_store_s(db_k, off4, fin ? 1 : 0);
        ob_k += 16 * (size_t)n_envs; ab_k += 4 * (size_t)n_envs; rb_k += 4 * (size_t)n_envs; db_k += 4 * (size_t)n_envs;
      }
      o = s;
      // ---- restart: skipped by the whole wavefront when no lane finished
      if (__ballot(fin) != 0ull) {
        const wd_u4 rnd = wd_philox4x32_10(wd_u4{(uint32_t)env, pool_epoch, 0x706f6f6cu, 2u}, pk0, pk1);
        const float pf = (float)(rnd.x >> 8) * 0x1.0p-24f;
        const int ref_id = min((int)(pf * (float)n_pool), n_pool - 1);   // 0 <= ref_id < n_pool in every lane
        float4 r = s;
        if (staged) {  // (uniform)
          r = pool_lds[ref_id];
        } else if (fin) {
          r = pool4[ref_id];
          // the row is consumed HERE, inside the rare branch (the wait also covers every record store before it)
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
        }
        s.x = fin ? r.x : s.x; s.y = fin ? r.y : s.y; s.z = fin ? r.z : s.z; s.w = fin ? r.w : s.w;
        o.x = fin ? o_restart.x : o.x; o.y = fin ? o_restart.y : o.y;
        o.z = fin ? o_restart.z : o.z; o.w = fin ? o_restart.w : o.w;
        t = fin ? 0 : t;
        pool_epoch += fin ? 1u : 0u;
      }
    };
    // cp_euler<true>'s preconditions: the launch's (division proof, both masses, threshold, every pool row) and the angles
    // this wavefront starts from; a tick then only ever sees a pool row or a state that did not terminate
    const bool fast = launch_fast && (__ballot(!(fabsf(s.z) <= 0.75f)) == 0ull);  // (wave-uniform)
    if (fast) for (int k = 0; k < ticks; ++k) tick(k, CpPoolFast{});
    else for (int k = 0; k < ticks; ++k) tick(k, CpPoolGeneral{});
    // ---- what the last tick leaves in memory
    action_arr[env] = a;
    reward_arr[env] = 1.0f;
    done_arr[env] = fin ? 1 : 0;
    observation_arr[env] = o;   // (a replica that finished on the last tick: its restored row)
    state_arr[env] = s;         // (... and its pool row)
    env_timestep_arr[env] = t;
    rng_state[WD_RNG_HEADER + env] = epoch0 + (uint32_t)ticks;
    pa.pool_rng[WD_RNG_HEADER + env] = pool_epoch;
  }
}

}  // namespace

extern "C" {

// the unpooled entry's arguments (HipClassicControlCartPoleEnvTick / ...Rollout_H<H>), then the pool generator's words,
// the pool, its row count and where the kernel keeps it
#define WD_CP_POOL_PARAMS                                                                                   \
    float4 *state_arr, int *action_arr, int *done_arr, float *reward_arr, float4 *observation_arr,         \
    float gravity, float masspole, float total_mass, float length, float polemass_length, float force_mag, \
    float tau, float theta_threshold_radians, float x_threshold, int *env_timestep_arr,                    \
    int episode_length, int n_envs, uint32_t *rng_state, const float *__restrict__ probs, int n_actions,   \
    const void *reset_table, int n_reset_arrays, int stream_tag, int ticks, float4 *obs_batch,             \
    int *action_batch, float *reward_batch, int *done_batch, const float *policy, int hidden,              \
    int invariant_divide_ok, uint32_t *pool_rng, const float *pool, int n_pool, int pool_in_lds

#define WD_CP_POOL_BODY(HH)                                                                                 \
    extern __shared__ __attribute__((aligned(16))) float cp_pool_lds[];                                    \
    const CpPhysics p{gravity, masspole, total_mass, length, polemass_length, force_mag, tau,              \
                      theta_threshold_radians, x_threshold, 1.0f / total_mass};                            \
    cp_pool_rollout<HH>(cp_pool_lds, state_arr, action_arr, done_arr, reward_arr, observation_arr, p,      \
                        env_timestep_arr, episode_length, n_envs, rng_state, probs, n_actions, reset_table, \
                        n_reset_arrays, stream_tag, ticks, obs_batch, action_batch, reward_batch,          \
                        done_batch, policy, hidden, invariant_divide_ok,                                   \
                        CpPoolArgs{pool_rng, pool, n_pool, pool_in_lds});

// fixed probabilities (`hidden` must be 0; `policy` is not read)
__global__ void HipClassicControlCartPoleEnvRollout_P(WD_CP_POOL_PARAMS) { WD_CP_POOL_BODY(0) }

__global__ void __launch_bounds__(256, 2) HipClassicControlCartPoleEnvRollout_P_H32(WD_CP_POOL_PARAMS) {
  WD_CP_POOL_BODY(32)
}

__global__ void __launch_bounds__(256, 2) HipClassicControlCartPoleEnvRollout_P_H64(WD_CP_POOL_PARAMS) {
  WD_CP_POOL_BODY(64)
}

}  // extern "C"
