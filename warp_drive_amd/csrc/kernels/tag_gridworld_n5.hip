// tag_gridworld_n5.hip -- the entries of the 5-agent TagGridWorld rollout and evaluation (tag_gridworld_n5_common.h:
// the design, the tick and the LDS layout are explained there) for the env whose finished replicas restart from their
// START state.  Its own code object (csrc/wd_kernels_gw5.hsaco): the host picks it when the shape matches
// (envs/tag_gridworld.py::tick_launch), the general kernel of tag_gridworld.hip serves everything else.
//
// Entries: HipTagGridWorldRollout_N5 (fixed probabilities), _N5_H32 / _N5_H64 (live policies),
// HipTagGridWorldEvaluate_N5_H32 / _H64 (one episode of every replica).
#include "tag_gridworld_n5_common.h"

namespace {

// the plain variant: positions and observations restored from the restore cache, a 64-entry quotient table
struct Gw5Plain {
  static constexpr bool POOL = false;
  static constexpr int MAX_COORD = 63;
#ifndef WD_GW5_BLOCK_ORDER_PLAIN
  static constexpr bool XCD_CONTIGUOUS = true;
#else
  static constexpr bool XCD_CONTIGUOUS = false;  // replica groups in blockIdx order (experiments/README.md)
#endif
};

}  // namespace

extern "C" __global__ void __launch_bounds__(64) HipTagGridWorldRollout_N5(GW5_PARAMS) {
  extern __shared__ __attribute__((aligned(16))) float gw5_smem[];
  gw5_rollout<0, Gw5Plain>(GW5_ARGS, nullptr, nullptr, nullptr, nullptr, nullptr, 0, gw5_smem);
}
// the same arguments + the packed weights of the two policies; dynamic LDS = the fixed-policy kernel's, its time
// table rounded up to 16 bytes, + 2 * gw5_policy_floats(H) floats (envs/tag_gridworld.py::live_policy_lds_bytes)
#define GW5_POLICY_ENTRY(HH)                                                                                          \
  extern "C" __global__ void __launch_bounds__(64) HipTagGridWorldRollout_N5_H##HH(                                   \
      GW5_PARAMS, const float *policy_tagger, const float *policy_runner) {                                           \
    extern __shared__ __attribute__((aligned(16))) float gw5_smem[];                                                  \
    gw5_rollout<HH, Gw5Plain>(GW5_ARGS, policy_tagger, policy_runner, nullptr, nullptr, nullptr, 0, gw5_smem);        \
  }
GW5_POLICY_ENTRY(32)
GW5_POLICY_ENTRY(64)

// one episode of every replica with the policies inside the kernel (gw5_evaluate).  Dynamic LDS: the image, 64
// coordinate quotients, the time table rounded up to 16 bytes, 2 * gw5_policy_floats(H) floats
// (envs/tag_gridworld.py::live_policy_evaluate_lds_bytes)
#define GW5_EVALUATE_ENTRY(HH)                                                                                        \
  extern "C" __global__ void __launch_bounds__(64) HipTagGridWorldEvaluate_N5_H##HH(GW5_EVALUATE_PARAMS) {            \
    extern __shared__ __attribute__((aligned(16))) float gw5_smem[];                                                  \
    gw5_evaluate<HH, Gw5Plain::MAX_COORD>(GW5_EVALUATE_ARGS, gw5_smem);                                               \
  }
GW5_EVALUATE_ENTRY(32)
GW5_EVALUATE_ENTRY(64)
