// wd_env.h -- what the device source of a custom environment includes (docs/custom_environments.md).
//
// Self-contained: <hip/hip_runtime.h> and <stdint.h> only, nothing of the package's own kernel sources (those stay
// free to change).  A custom unit is compiled with the package's kernel flags: no floating-point contraction,
// correctly rounded divide and sqrt -- a float32 expression written the way the host step writes it gives the host's
// bits.
//
// Geometry.  One block per replica (blocks_per_env is 1), one thread per agent: the launch of
// `function_manager.block` / `.grid`, or -- needed by the reductions below -- the same block rounded up to whole
// wavefronts of 64 lanes, where the threads behind the last agent do nothing but take part in barriers and
// reductions (with the operation's identity as their value).
//
// Reductions over the agents of a replica (wd_env_sum_int, wd_env_max_int):
//   * every thread of the block calls them, in uniform control flow, with blockDim.x a multiple of 64, 64 .. 1024
//     (1 to 16 wavefronts);
//   * `scratch`: WD_ENV_SCRATCH_INTS ints of LDS (__shared__) the caller owns; the same array may be handed to one
//     call after another;
//   * every thread receives the result;
//   * cost: six cross-lane exchanges inside the wavefront, one LDS write per wavefront, TWO block barriers (one
//     before the slots are read, one after, so that the next call may overwrite them), and one broadcast LDS read
//     per wavefront of the block, combined in wavefront order 0, 1, 2, ...
// Float sums are deliberately not offered: a tree sum adds in another order than a host loop over the agents and
// does not match it bit for bit.  Sum integers (scale fixed-point values if need be) and convert once.
#ifndef WD_ENV_H_
#define WD_ENV_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define WD_ENV_KERNEL extern "C" __global__

#define WD_ENV_WAVE 64
#define WD_ENV_MAX_WAVES 16
#define WD_ENV_SCRATCH_INTS WD_ENV_MAX_WAVES

// replica of this block, agent of this thread (may be >= n_agents in a block rounded up to whole wavefronts)
__device__ __forceinline__ int wd_env_id() { return (int)blockIdx.x; }
__device__ __forceinline__ int wd_agent_id() { return (int)threadIdx.x; }

// element (env, agent, feature) of a [n_envs, n_agents, n_features] array; 64-bit, so that 2000 replicas of 1000
// agents with 1100 features do not wrap
__device__ __forceinline__ int64_t wd_index(int env, int agent, int feature, int n_agents, int n_features) {
  return ((int64_t)env * n_agents + agent) * n_features + feature;
}

// all threads of the replica: a replica is one block here, so this is the block barrier
__device__ __forceinline__ void wd_sync_env_threads() { __syncthreads(); }

// ---- inside one wavefront: butterfly over the 64 lanes, every lane ends with the result
__device__ __forceinline__ int wd_wave_sum_int(int v) {
#pragma unroll
  for (int off = WD_ENV_WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WD_ENV_WAVE);
  return v;
}
__device__ __forceinline__ int wd_wave_max_int(int v) {
#pragma unroll
  for (int off = WD_ENV_WAVE / 2; off > 0; off >>= 1) {
    const int other = __shfl_xor(v, off, WD_ENV_WAVE);
    v = other > v ? other : v;
  }
  return v;
}

// ---- over the block: one LDS slot per wavefront, combined in wavefront order
__device__ __forceinline__ int wd_env_sum_int(int v, int *scratch) {
  v = wd_wave_sum_int(v);
  const int waves = (int)(blockDim.x + WD_ENV_WAVE - 1) / WD_ENV_WAVE;
  if ((threadIdx.x & (WD_ENV_WAVE - 1)) == 0) scratch[threadIdx.x / WD_ENV_WAVE] = v;
  __syncthreads();
  int total = scratch[0];
  for (int w = 1; w < waves; ++w) total += scratch[w];
  __syncthreads();
  return total;
}
__device__ __forceinline__ int wd_env_max_int(int v, int *scratch) {
  v = wd_wave_max_int(v);
  const int waves = (int)(blockDim.x + WD_ENV_WAVE - 1) / WD_ENV_WAVE;
  if ((threadIdx.x & (WD_ENV_WAVE - 1)) == 0) scratch[threadIdx.x / WD_ENV_WAVE] = v;
  __syncthreads();
  int best = scratch[0];
  for (int w = 1; w < waves; ++w) best = scratch[w] > best ? scratch[w] : best;
  __syncthreads();
  return best;
}

#endif  // WD_ENV_H_
