// wd_env_tick.h -- the kit for a FUSED TICK of a custom environment: the actions of every head are drawn, the author's
// step runs and finished replicas restart, in ONE launch, for `ticks` ticks in a row (docs/custom_environments.md,
// "A fused tick").
//
// Self-contained like wd_env.h: "wd_env.h", <hip/hip_runtime.h> and <stdint.h>, nothing of the package's own kernel
// sources.  The generator, the bits-to-uniform conversion, the categorical pick and the layout of a reset-table
// entry form a section that a plain host compiler builds as well (no HIP header is read when __HIPCC__ is not
// defined): a host program can print what a kernel will draw.
//
// How an author uses it.  The step is written ONCE as a `__device__ __forceinline__` function that takes the action
// of its thread as a value; `Hip<Name>Step` calls it with the action it reads from the action array, and
// `Hip<Name>Tick` -- whose parameters are the step's own followed by WD_TICK_PARAMS -- calls it inside the loop
//
//     WD_TICK_KIT(kit);                                            // the trailing parameters as one struct
//     for (int k = 0; k < ticks; ++k) {
//       wd_tick_begin(done_arr, env, agent, /*step_reads_done=*/false);
//       int act[WD_TICK_MAX_HEADS];
//       wd_tick_sample(kit, env, agent, n_agents, actions_arr, act);
//       my_step(..., act[0], ...);
//       wd_tick_end(kit, done_arr, env_timestep_arr, env, agent);
//     }
//
// Geometry: wd_env.h's.  One block per replica (blocks_per_env is 1), one thread per agent, the block rounded up to
// whole wavefronts (ceil(N / 64) * 64 threads).  Threads behind the last agent draw nothing and store nothing; they
// take part in every barrier, so begin, sample, step and end are called by EVERY thread of the block, in uniform
// control flow.
//
// Trailing parameters (WD_TICK_PARAMS), in this order -- warp_drive_amd/utils/custom_tick.py packs exactly these:
//     uint32_t *rng_state            the sampler's state: [0], [1] key words, [4 + row] the epoch of agent row `row`
//     int n_heads                    H, 1 .. WD_TICK_MAX_HEADS (4)
//     const float *probs0 .. probs3  head h: [n_envs, n_agents, size_h] float32; unused heads: null
//     int size0 .. size3             actions of head h; unused heads: 0
//     const void *reset_table        wd_tick_reset_entry[reset_entries]: the arrays a restart restores
//     int reset_entries
//     int stream_tag                 counter word 2 of the draw
//     int ticks                      LAST: a launch plan's multi-tick form rewrites the last four bytes per run
// Pointers and 32-bit scalars only.
//
// The draw.  Agent row `row = env * n_agents + agent` reads its epoch e = rng_state[4 + row], stores e + 1 and makes
// ONE Philox4x32-10 call with counter (row, e, stream_tag, 5) and key (rng_state[0], rng_state[1]).  Head h takes word
// h of the block: u = ((bits >> 8) + 1) * 2^-24, in (0, 1].  Its action is the number of float32 running prefix sums of
// its probability row (summed in index order) that are < u, clamped to size_h - 1; it is stored to
// actions[row * H + h].  One rule for every H.  Counter word 3 = 5 belongs to this kit (0: sample_actions, 1: the OU
// draw, 2: the pool pick, 3 and 4: the in-tree fused ticks), so no other draw of the package collides with it.
//
// The done flag.  wd_tick_begin: the agent-0 thread clears `_done_[env]`, which the previous tick left set for a
// replica that finished (and was restarted).  The step sets it (agent 0, as in a plain step kernel).  wd_tick_end: a
// block barrier; every thread reads the flag behind it; if it is set, row `env` of every table entry is restored from
// its reference copy with block-strided 4-byte copies and `_timestep_[env]` becomes 0 -- `_done_[env]` STAYS 1 for
// whoever reads it after the launch, the next tick clears it; a final barrier.
//
// Visibility inside the loop.  Between the ticks of one launch a replica's arrays are read back by the SAME BLOCK that
// wrote them, often by another thread of it (the restart copies rows with a block stride).  What orders these accesses
// is the block barriers of begin and end (each also a memory fence over the block): everything the step stored is
// visible to the restart, everything the restart stored is visible to the next trip.  A step that hands data from one
// thread to another THROUGH GLOBAL MEMORY within one tick needs its own wd_sync_env_threads() between the store and the
// load, exactly as it does in a plain step kernel.  Do not mark an array of the reset table, `_done_` or `_timestep_`
// `__restrict__` in the step function: the restart writes them through other pointers.
#ifndef WD_ENV_TICK_H_
#define WD_ENV_TICK_H_

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "wd_env.h"
#define WD_TICK_HD __host__ __device__ __forceinline__
// a pointer READ FROM A TABLE in memory is a generic pointer to the compiler, and every access through it a flat
// instruction (whose completion both memory counters count); the table holds device-memory addresses only: say so
#define WD_TICK_GLOBAL __attribute__((address_space(1)))
#else
#define WD_TICK_HD static inline
#define WD_TICK_GLOBAL
#endif

#define WD_TICK_MAX_HEADS 4
#define WD_TICK_COUNTER_WORD3 5u
#define WD_TICK_RNG_HEADER 4  // rng_state: [0] key word 0, [1] key word 1, [2] rows, [3] reserved, [4 + row] epochs

// =============================================================================== host and device
struct wd_tick_u4 {
  uint32_t x, y, z, w;
};

// Philox4x32-10 (Salmon et al., SC'11): the generator of every draw of the package
WD_TICK_HD wd_tick_u4 wd_tick_philox4x32_10(wd_tick_u4 ctr, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)M0 * ctr.x, p1 = (uint64_t)M1 * ctr.z;
    wd_tick_u4 n;
    n.x = (uint32_t)(p1 >> 32) ^ ctr.y ^ k0;
    n.y = (uint32_t)p1;
    n.z = (uint32_t)(p0 >> 32) ^ ctr.w ^ k1;
    n.w = (uint32_t)p0;
    ctr = n;
    k0 += W0;
    k1 += W1;
  }
  return ctr;
}

// the block of agent row `row` at epoch `epoch`: one call serves every head of the row
WD_TICK_HD wd_tick_u4 wd_tick_block(uint32_t row, uint32_t epoch, uint32_t stream_tag, uint32_t k0, uint32_t k1) {
  const wd_tick_u4 ctr = {row, epoch, stream_tag, WD_TICK_COUNTER_WORD3};
  return wd_tick_philox4x32_10(ctr, k0, k1);
}

// word `head` (0 .. 3) of a block
WD_TICK_HD uint32_t wd_tick_word(wd_tick_u4 blk, int head) {
  return head == 0 ? blk.x : (head == 1 ? blk.y : (head == 2 ? blk.z : blk.w));
}

// uniform in (0, 1] from the upper 24 bits
WD_TICK_HD float wd_tick_uniform(uint32_t bits) {
  return (float)((bits >> 8) + 1u) * 5.9604644775390625e-08f;  // 2^-24, exact
}

// categorical pick: how many float32 running prefix sums of row[0 .. n) are < u, clamped to n - 1
WD_TICK_HD int wd_tick_pick(const float *row, int n, float u) {
  float cum = 0.0f;
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    cum = (i == 0) ? row[0] : cum + row[i];
    cnt += (cum < u) ? 1 : 0;
  }
  return cnt < n - 1 ? cnt : n - 1;
}

// One entry of the reset table (HIPEnvironmentReset._build_table writes it; wd_common.h's wd_reset_entry restated):
// row `env` of `data` is restored from row `env` of `ref`, row_elems 32-bit words each.
struct wd_tick_reset_entry {
  WD_TICK_GLOBAL uint32_t *data;
  const WD_TICK_GLOBAL uint32_t *ref;
  int row_elems;
  int pad_;
};
static_assert(sizeof(wd_tick_reset_entry) == 24, "the host writes 24-byte entries: u8 data, u8 ref, i4 row, i4 pad");
static_assert(__builtin_offsetof(wd_tick_reset_entry, data) == 0 && __builtin_offsetof(wd_tick_reset_entry, ref) == 8 &&
                  __builtin_offsetof(wd_tick_reset_entry, row_elems) == 16,
              "fields at 0 / 8 / 16");

// =============================================================================== device only
#ifdef __HIPCC__

// the trailing parameters of a Tick entry, after the step's own (the order is the contract: see the top of the file)
#define WD_TICK_PARAMS                                                                                               \
  uint32_t *wd_tick_rng_state_, int wd_tick_n_heads_, const float *wd_tick_probs0_, const float *wd_tick_probs1_,  \
      const float *wd_tick_probs2_, const float *wd_tick_probs3_, int wd_tick_size0_, int wd_tick_size1_,           \
      int wd_tick_size2_, int wd_tick_size3_, const void *wd_tick_reset_table_, int wd_tick_reset_entries_,         \
      int wd_tick_stream_tag_, int ticks

struct wd_tick_kit {
  uint32_t *rng_state;
  int n_heads;
  const float *probs0, *probs1, *probs2, *probs3;  // (named fields, not an array: an array indexed by a head number
  int size0, size1, size2, size3;                  //  that the compiler does not know would live in scratch memory)
  const wd_tick_reset_entry *reset_table;
  int reset_entries;
  uint32_t stream_tag;
};

// gathers the trailing parameters into `const wd_tick_kit name`
#define WD_TICK_KIT(name)                                                                                          \
  const wd_tick_kit name = {wd_tick_rng_state_, wd_tick_n_heads_, wd_tick_probs0_, wd_tick_probs1_,               \
                            wd_tick_probs2_, wd_tick_probs3_, wd_tick_size0_, wd_tick_size1_, wd_tick_size2_,     \
                            wd_tick_size3_, (const wd_tick_reset_entry *)wd_tick_reset_table_,                    \
                            wd_tick_reset_entries_, (uint32_t)wd_tick_stream_tag_}

// ---- begin: clear the flag the previous tick left set.  `step_reads_done`: the step READS `_done_[env]` (most steps
// only set it), so every thread has to see the cleared flag: one more block barrier.
__device__ __forceinline__ void wd_tick_begin(int *done_arr, int env, int agent, bool step_reads_done) {
  if (agent == 0) done_arr[env] = 0;
  if (step_reads_done) __syncthreads();
}

__device__ __forceinline__ int wd_tick_sample_head_(const float *probs, int size, int64_t row, uint32_t bits, int *out) {
  const int a = wd_tick_pick(probs + row * size, size, wd_tick_uniform(bits));
  *out = a;
  return a;
}

// ---- sample: the actions of this thread's agent, every head; stored to actions_arr[row * H + h] and returned in
// act[h] (act[h] = 0 for h >= H and for a thread behind the last agent, which draws and stores nothing)
__device__ __forceinline__ void wd_tick_sample(const wd_tick_kit &kit, int env, int agent, int n_agents, int *actions_arr,
                                               int (&act)[WD_TICK_MAX_HEADS]) {
  act[0] = act[1] = act[2] = act[3] = 0;
  if (agent >= n_agents) return;
  const int64_t row = (int64_t)env * n_agents + agent;
  const uint32_t epoch = kit.rng_state[WD_TICK_RNG_HEADER + row];
  kit.rng_state[WD_TICK_RNG_HEADER + row] = epoch + 1u;
  const wd_tick_u4 blk = wd_tick_block((uint32_t)row, epoch, kit.stream_tag, kit.rng_state[0], kit.rng_state[1]);
  const int H = kit.n_heads;
  int *out = actions_arr + row * H;
  act[0] = wd_tick_sample_head_(kit.probs0, kit.size0, row, blk.x, out);
  if (H > 1) act[1] = wd_tick_sample_head_(kit.probs1, kit.size1, row, blk.y, out + 1);
  if (H > 2) act[2] = wd_tick_sample_head_(kit.probs2, kit.size2, row, blk.z, out + 2);
  if (H > 3) act[3] = wd_tick_sample_head_(kit.probs3, kit.size3, row, blk.w, out + 3);
}

// ---- end: restart the replica if the step finished it.  Returns whether it did (the same value in every thread).
__device__ __forceinline__ bool wd_tick_end(const wd_tick_kit &kit, int *done_arr, int *env_timestep_arr, int env,
                                            int agent) {
  __syncthreads();  // everything the step stored, the flag included, is visible to the block from here on
  // read behind the barrier by every thread: one address, one writer (agent 0, before the barrier), so one value; the
  // first lane's copy makes that plain to the compiler (a scalar branch, a loop without lane masks)
  const bool finished = __builtin_amdgcn_readfirstlane(done_arr[env]) != 0;
  if (finished) {
    for (int r = 0; r < kit.reset_entries; ++r) {
      const wd_tick_reset_entry ent = kit.reset_table[r];
      const int64_t base = (int64_t)env * ent.row_elems;
      for (int i = (int)threadIdx.x; i < ent.row_elems; i += (int)blockDim.x) ent.data[base + i] = ent.ref[base + i];
    }
    if (agent == 0) env_timestep_arr[env] = 0;  // `_done_[env]` stays 1: the next tick's begin clears it
  }
  __syncthreads();  // the restored rows are visible to the next trip; its begin may overwrite the flag
  return finished;
}

#endif  // __HIPCC__
#endif  // WD_ENV_TICK_H_
