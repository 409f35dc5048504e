// tag_gridworld_n5_pool.hip -- the entries of the 5-agent TagGridWorld rollout and evaluation
// (tag_gridworld_n5_common.h) for the env whose finished replicas restart from a random row of a RESET POOL
// (envs/tag_gridworld.py::CUDATagGridWorldWithResetPool, the reference's `tag_gridworld_with_reset_pool` config: one
// shared [32, 32] policy, grid_length 100).  Its own code object (csrc/wd_kernels_gw5_pool.hsaco), beside
// tag_gridworld_n5.hip's.
//
// Geometry, tick and recording are one source with the plain variant's.  What DIFFERS (each under `if constexpr
// (V::POOL)` or on V::MAX_COORD in the header):
//   * coordinates up to 255: the quotient table has 256 entries, filled by a loop with the same float32 division
//     `(float)c / (float)L`; the packed cell `x | y << 8` of the tag check already holds 255;
//   * a uniform early return for shapes the tables are not sized for (the host admits none of them), and for a null
//     policy in the live-policy entries below;
//   * a finished replica restarts from the pool row reset_when_done_from_pool (wd_core.hip) would draw: counter {env,
//     pool_epoch, 0x706f6f6c, 2} under the keys pool_rng[0], pool_rng[1], p = (rnd.x >> 8) * 2^-24, row = min((int)(p *
//     n_pool), n_pool - 1); x and y come from the SAME row of the two pools, t = 0.  `pool_epoch` is a per-lane register,
//     loaded once per replica group from pool_rng[WD_RNG_HEADER + env], consumed before the tick loop with the other
//     loaded values, incremented on a restart only, written back by lane ag == 0 after the last tick.  The Philox call
//     sits inside the wave-uniform `fm != 0` branch: a tick without a finished replica executes none of it;
//   * both pools ([n_pool][5] int32 each) are copied to LDS once per launch, between the time table and the policies,
//     so the tick loop has no plain global load (the header's comment on the in-order memory counter: a wait for such a
//     load would wait for the previous tick's stores on every trip);
//   * the registered reset arrays of this env are exactly {observations}: the restore cache holds CD = 105 dwords per
//     replica, the observation rows of the START positions -- NOT of the pool row.  That is the reference's behaviour (its
//     placeholder is built once, at the first reset) and what oracle/tag_gridworld_np.py::reset_done_envs(x=, y=) models.
//     The cache copy tracks the observations' offset alone, clamps its replica index to the block's replicas and stops
//     at a replica's share;
//   * the time-table read of the rollout is clamped to the table (both evaluations clamp);
//   * after the last tick the launch writes positions, observations, time step, `_done_`, last rewards / actions, the
//     sampler's epoch words (+= ticks) and the pool epoch words.
//
// Entries: HipTagGridWorldRollout_N5P (fixed probabilities), _N5P_H32 / _N5P_H64 (live policies: pack_gridworld_policy's
// layout, two pointers -- a shared policy is passed twice), HipTagGridWorldEvaluate_N5P_H32 / _H64 (gw5_evaluate with
// only the wider table: evaluation has no restart, so it neither reads nor writes the pool; it takes the four pool
// arguments so that the two families are called alike).  Dynamic LDS: envs/tag_gridworld.py::pool_rollout_lds_bytes.
#include "tag_gridworld_n5_common.h"

namespace {

// the pooled variant: positions from the reset pool, a 256-entry quotient table
struct Gw5Pooled {
  static constexpr bool POOL = true;
  static constexpr int MAX_COORD = 255;
  static constexpr bool XCD_CONTIGUOUS = true;
};

}  // namespace

// the pool, behind the plain entries' arguments: the resetter's generator words, the two pools [n_pool][5], their
// row count
#define GW5P_POOL_PARAMS uint32_t *pool_rng, const int *pool_x, const int *pool_y, int n_pool

extern "C" __global__ void __launch_bounds__(64) HipTagGridWorldRollout_N5P(GW5_PARAMS, GW5P_POOL_PARAMS) {
  extern __shared__ __attribute__((aligned(16))) float gw5_smem[];
  gw5_rollout<0, Gw5Pooled>(GW5_ARGS, nullptr, nullptr, pool_rng, pool_x, pool_y, n_pool, gw5_smem);
}
#define GW5P_POLICY_ENTRY(HH)                                                                                         \
  extern "C" __global__ void __launch_bounds__(64) HipTagGridWorldRollout_N5P_H##HH(                                  \
      GW5_PARAMS, const float *policy_tagger, const float *policy_runner, GW5P_POOL_PARAMS) {                         \
    extern __shared__ __attribute__((aligned(16))) float gw5_smem[];                                                  \
    if (policy_tagger == nullptr || policy_runner == nullptr) return;                                                 \
    gw5_rollout<HH, Gw5Pooled>(GW5_ARGS, policy_tagger, policy_runner, pool_rng, pool_x, pool_y, n_pool, gw5_smem);   \
  }
GW5P_POLICY_ENTRY(32)
GW5P_POLICY_ENTRY(64)

// the arguments of HipTagGridWorldEvaluate_N5_H<width>, then the pool's four (unused: an evaluation never restarts).
// Dynamic LDS: the image, 256 coordinate quotients, the time table rounded up to 16 bytes, 2 * gw5_policy_floats(H)
// floats (envs/tag_gridworld.py::live_policy_evaluate_lds_bytes)
#define GW5P_EVALUATE_ENTRY(HH)                                                                                       \
  extern "C" __global__ void __launch_bounds__(64) HipTagGridWorldEvaluate_N5P_H##HH(                                 \
      GW5_EVALUATE_PARAMS, const uint32_t *pool_rng, const int *pool_x, const int *pool_y, int n_pool) {              \
    extern __shared__ __attribute__((aligned(16))) float gw5_smem[];                                                  \
    gw5_evaluate<HH, Gw5Pooled::MAX_COORD>(GW5_EVALUATE_ARGS, gw5_smem);                                              \
  }
GW5P_EVALUATE_ENTRY(32)
GW5P_EVALUATE_ENTRY(64)
