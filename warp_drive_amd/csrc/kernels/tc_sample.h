// tc_sample.h -- sample: both action heads of an agent from the LDS slabs (fused tick).
// Part of the TagContinuous translation unit (tag_continuous.hip, which holds the design notes, the probe macros
// and the kernel entries); split by phase in round 6 with every shipped code object byte-identical before / after.
#pragma once
#include "wd_common.h"
#include "tc_kernarg.h"
#include "tc_fetch.h"

namespace {

// ---- fused tick: sample both action heads for this thread's agent (replaces two sample_actions
// launches, random.cu:51-85): inverse CDF on a running float32 sum, one Philox call for both heads.
__device__ __forceinline__ int2 tc_sample_heads(const TcArgs &a, const TcFuse &fz, const TcIn &in, bool active, int gi,
                                                int li, const float *slab_acc, float *slab_turn, int n_acc,
                                                int n_turn, int env0, int epb) {
  int2 sampled = make_int2(0, 0);
  wd_u4 rnd = wd_u4{0u, 0u, 0u, 0u};
  if (active) {
    fz.rng_state[WD_RNG_HEADER + gi] = in.epoch + 1u;
    rnd = wd_philox4x32_10(wd_u4{(uint32_t)gi, in.epoch, (uint32_t)fz.stream_tag, 3u}, fz.rng_state[0],
                           fz.rng_state[1]);
  }
  // every global_load_lds of this wavefront has landed once its vmcnt drains; the rows a lane
  // reads were all fetched by its own wavefront
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  if (active) sampled.x = wd_slab_sample(slab_acc + (size_t)li * n_acc, n_acc, wd_u01_open_closed(rnd.x));
  if (tc_one_slab(a.N)) {  // block-uniform: the second head's rows replace the first head's (slab_turn == slab_acc)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wavefront's reads of its rows are complete
    __builtin_amdgcn_wave_barrier();
    // Wavefront w's rows start at float 64 * w * n_actions: with heads of EQUAL size the two heads' rows of a
    // wavefront coincide and are wave-private.  With unequal sizes w's turn rows overlap the acceleration rows of
    // its neighbours: every wavefront must have sampled its first head (which also means every acceleration fetch
    // has landed) before anybody fetches the second.  Block-uniform condition.
    if (n_acc != n_turn) __syncthreads();
    tc_fetch_slab(slab_turn, fz.probs_turn, a, env0, epb, a.N, n_turn, threadIdx.x);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
  }
  if (active) {
    sampled.y = wd_slab_sample(slab_turn + (size_t)li * n_turn, n_turn, wd_u01_open_closed(rnd.y));
    ((int2 *)fz.actions_out)[gi] = sampled;
  }
  return sampled;
}

// s_waitcnt immediate of gfx9 (vmcnt [3:0] and [15:14], expcnt [6:4], lgkmcnt [11:8]; a field of all ones does not wait).
// Through the BUILTIN, not inline asm: the compiler's own counter bookkeeping sees it, so it does not put a second
// vmcnt(0) -- which would also wait for every store issued since -- in front of the next LDS access for the sake of a
// global_load_lds it believes to be in flight.
#define WD_WAIT_VMCNT0 0x0F70

// Multi-tick entry only (two slabs side by side, no tc_one_slab path: replicas of at most 128 agents, asserted at the
// call site).  The caller has issued both slabs and NOTHING else since; between that and the wait there is only register work: the ten Philox rounds, on the epoch the thread carries
// and the key the launch read once, run in the shadow of the fetch.  No load, no store (its acknowledgement would be
// waited for in order with the slabs' data) and no LDS access lies in between.  The actions go out behind the wait.
// SA: the size of both heads as a constant (n_acc == n_turn == SA, set by the entry): SA entries read and scanned per
// head, not WD_SLAB_CH of which the last are masked off.
template <int SA>
__device__ __forceinline__ int2 tc_sample_heads_carried(const TcArgs &a, const TcFuse &fz_, uint32_t epoch, uint32_t k0, uint32_t k1,
                                                        bool active, int gi, int li, const float *slab_acc,
                                                        const float *slab_turn, int n_acc, int n_turn) {
  uint32_t e = epoch;
  asm volatile("" : "+v"(e));  // (opaque, ordered after the slab issue: the rounds are not hoisted in front of it ...)
  // (the key too, per trip: seen through, its ten round keys -- and the first round's products, which depend on nothing
  // else -- are worked out once per launch, 17 values that only fit lanes of a vector register and come back by
  // v_readlane_b32 on every trip; from an opaque key they are ten pairs of s_add_i32 on the scalar unit)
  uint32_t tag = (uint32_t)fz_.stream_tag;  // (and the stream tag: its first-round product is such a value too)
  asm volatile("" : "+s"(k0), "+s"(k1), "+s"(tag));
  wd_u4 rnd = wd_philox4x32_10(wd_u4{(uint32_t)gi, e, tag, 3u}, k0, k1);  // (every lane: no branch)
  asm volatile("" : "+v"(rnd.x), "+v"(rnd.y));  // (... and not sunk behind the wait)
  // every global_load_lds of this wavefront has landed once its vmcnt drains; the rows a lane reads were all fetched by
  // its own wavefront
  __builtin_amdgcn_s_waitcnt(WD_WAIT_VMCNT0);
  __builtin_amdgcn_wave_barrier();
  // where the actions go: a view of the kernel arguments taken behind the wait (tc_kernarg.h); its
  // scalar loads return under the two scans
  const TcFuse fz = TcPhase(a, fz_).fz;
  int2 sampled = make_int2(0, 0);
  if (active) {
    sampled.x = wd_slab_sample<SA>(slab_acc + (size_t)li * SA, wd_u01_open_closed(rnd.x));
    // (the second slab's row through a byte offset the compiler cannot see through: one address register and immediate
    // offsets, as for the first -- folded into the offsets, the slab's distance is beyond what a two-dword read encodes)
    unsigned turn_row = (unsigned)((const char *)slab_turn - (const char *)slab_acc) + 4u * SA * (unsigned)li;
    asm volatile("" : "+v"(turn_row));
    sampled.y = wd_slab_sample<SA>((const float *)((const char *)slab_acc + turn_row), wd_u01_open_closed(rnd.y));
    ((int2 *)fz.actions_out)[gi] = sampled;
    // (the epoch word is NOT stored here: the thread carries it, and memory gets epoch + 1 on a closing trip,
    // tc_store_carried in tc_fast.h)
  }
  return sampled;
}

}  // namespace
