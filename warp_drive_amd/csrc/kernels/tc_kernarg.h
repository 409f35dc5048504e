// tc_kernarg.h -- the kernel-argument segment of the TagContinuous entries, described once, and the phase-scoped views
// of it that the multi-tick entry (tc_fast_rollout, tc_fast.h) reads its pointers through.
// Part of the TagContinuous translation unit (tag_continuous.hip holds the design notes and the kernel entries).
//
// The lists below are the ONE place where the arguments are named: the parameter lists of every entry (WD_TC_PARAMS,
// WD_TC_FUSE_PARAMS) and the mirror struct of the multi-tick entry's segment (TcRolloutKernarg) are generated from them,
// so order and types cannot drift apart.  The first part of this file (down to the device section) is plain C++: a host
// build of it prints offsetof / sizeof of every field (tests/test_tick_rollout_kernarg_build.py compares them with the
// `.args` record of the compiled entry).
//
// Why views.  The loop of the multi-tick entry uses about 45 pointer arguments, each in one or two phases of a trip.  Taken
// by value they are all live from trip to trip, 90 scalar registers that the scalar file does not have: the compiler parked
// them in lanes of a vector register and fetched each back with a v_readlane_b32 -- an instruction of the VALU, the unit
// this kernel saturates -- in front of every use (97 parked values, 174 lane reads in the loop body).  The segment itself
// sits in the scalar cache for the whole launch.  So every phase of a trip that needs pointers reads THEM -- and nothing
// else -- from the segment with scalar loads (s_load_dwordx2 / x4, the scalar unit, which has headroom), through a view:
// the segment's address passed through an opaque asm, so that the compiler can neither hoist a view's loads above the
// place it was taken at nor merge them with another view's.  The launch constants the arithmetic needs on every trip stay
// in registers.
#pragma once
#include <stdint.h>

// X(type, name): the arguments of a Step entry, in order ...
#define WD_TC_PARAM_LIST(X, SEP)                                                                            \
  X(float *, loc_x_arr) SEP X(float *, loc_y_arr) SEP X(float *, speed_arr) SEP X(float *, direction_arr) SEP \
  X(float *, acceleration_arr) SEP X(const int *, agent_types_arr) SEP X(float *, edge_hit_reward_penalty) SEP \
  X(float, kEdgeHitPenalty) SEP X(float, kGridLength) SEP X(const float *, acceleration_actions_arr) SEP     \
  X(const float *, turn_actions_arr) SEP X(float, kMaxSpeed) SEP X(int, kNumOtherAgentsObserved) SEP         \
  X(const float *, skill_levels_arr) SEP X(int, kRunnerExitsGameAfterTagged) SEP X(int *, still_in_the_game_arr) SEP \
  X(int, kUseFullObservation) SEP X(float *, obs_arr) SEP X(const int *, action_indices_arr) SEP             \
  X(float *, neighbor_distances_arr) SEP X(int *, neighbor_ids_sorted_by_distance_arr) SEP                   \
  X(int *, nearest_neighbor_ids) SEP X(float *, rewards_arr) SEP X(const float *, step_rewards_arr) SEP      \
  X(int *, num_runners_arr) SEP X(float, kDistanceMarginForReward) SEP X(float, kTagRewardForTagger) SEP     \
  X(float, kTagPenaltyForRunner) SEP X(float, kEndOfGameRewardForRunner) SEP X(int *, done_arr) SEP          \
  X(int *, env_timestep_arr) SEP X(int, kNumAgents) SEP X(int, kEpisodeLength) SEP X(int, kNumEnvs) SEP      \
  X(int, kNumAccelerationActions) SEP X(int, kNumTurnActions) SEP X(int *, obs_rows_cleared_arr) SEP         \
  X(unsigned *, knn_prev_arr) SEP X(int, kEnvBegin)
// ... what a Tick entry takes behind them ...
#define WD_TC_FUSE_PARAM_LIST(X, SEP)                                                                       \
  X(uint32_t *, rng_state) SEP X(const float *, probs_acc) SEP X(const float *, probs_turn) SEP             \
  X(const void *, reset_table) SEP X(int, n_reset_arrays) SEP X(int, stream_tag)
// ... and what the multi-tick entry takes behind those
#define WD_TC_ROLLOUT_PARAM_LIST(X, SEP) X(int, kNumTicks)

#define WD_TC_AS_PARAM(type, name) type name
#define WD_TC_AS_FIELD(type, name) type name;
#define WD_TC_COMMA ,
#define WD_TC_NOTHING

#define WD_TC_PARAMS WD_TC_PARAM_LIST(WD_TC_AS_PARAM, WD_TC_COMMA)
#define WD_TC_FUSE_PARAMS , WD_TC_FUSE_PARAM_LIST(WD_TC_AS_PARAM, WD_TC_COMMA)
#define WD_TC_ROLLOUT_PARAMS , WD_TC_ROLLOUT_PARAM_LIST(WD_TC_AS_PARAM, WD_TC_COMMA)

// the kernel-argument segment of HipTagContinuousRollout_K<k>_N<n>A<a>, field for field (the hidden arguments the
// compiler appends lie behind the last one)
struct TcRolloutKernarg {
  WD_TC_PARAM_LIST(WD_TC_AS_FIELD, WD_TC_NOTHING)
  WD_TC_FUSE_PARAM_LIST(WD_TC_AS_FIELD, WD_TC_NOTHING)
  WD_TC_ROLLOUT_PARAM_LIST(WD_TC_AS_FIELD, WD_TC_NOTHING)
};

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------ device section
#include "tc_types.h"

// arguments (by those names, in scope) -> TcArgs / TcFuse
#define WD_TC_PACK()                                                                              \
  TcArgs a;                                                                                       \
  a.loc_x = loc_x_arr; a.loc_y = loc_y_arr; a.speed = speed_arr; a.direction = direction_arr;     \
  a.acceleration = acceleration_arr; a.agent_types = agent_types_arr;                             \
  a.edge_pen_arr = edge_hit_reward_penalty; a.edge_hit_penalty = kEdgeHitPenalty;                 \
  a.grid_length = kGridLength; a.acc_actions = acceleration_actions_arr;                          \
  a.turn_actions = turn_actions_arr; a.max_speed = kMaxSpeed; a.K = kNumOtherAgentsObserved;      \
  a.skill_levels = skill_levels_arr; a.runner_exits = kRunnerExitsGameAfterTagged;                \
  a.sig_arr = still_in_the_game_arr; a.use_full_obs = kUseFullObservation; a.obs = obs_arr;       \
  a.actions = action_indices_arr; a.nearest_ids = nearest_neighbor_ids; a.rewards = rewards_arr;  \
  a.step_rewards = step_rewards_arr; a.num_runners = num_runners_arr;                             \
  a.margin = kDistanceMarginForReward; a.tag_reward = kTagRewardForTagger;                        \
  a.tag_penalty = kTagPenaltyForRunner; a.end_reward = kEndOfGameRewardForRunner;                 \
  a.done = done_arr; a.timestep = env_timestep_arr; a.N = kNumAgents; a.T = kEpisodeLength;       \
  a.E = kNumEnvs; a.env_begin = kEnvBegin; a.obs_rows_cleared = obs_rows_cleared_arr;              \
  a.knn_prev = knn_prev_arr;                                                                      \
  (void)neighbor_distances_arr; (void)neighbor_ids_sorted_by_distance_arr;
#define WD_TC_FUSE_PACK()                                                                      \
  TcFuse fz;                                                                                   \
  fz.rng_state = rng_state; fz.probs_acc = probs_acc; fz.probs_turn = probs_turn;              \
  fz.actions_out = const_cast<int *>(action_indices_arr);                                      \
  fz.reset_table = (const wd_reset_entry *)reset_table; fz.n_reset_arrays = n_reset_arrays;      \
  fz.stream_tag = stream_tag;

namespace {

typedef const __attribute__((address_space(4))) TcRolloutKernarg *TcKernargView;

// A view of the segment: the same address every time, but a value the compiler cannot see through, defined HERE.  A read
// through it is a scalar load that stays behind this call and is not shared with the reads of any other view.
// ONLY inside HipTagContinuousRollout_K<k>_N<n>A<a>: any other kernel's segment is laid out differently.
__device__ __forceinline__ TcKernargView tc_kernarg_view() {
  TcKernargView p = (TcKernargView)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// The arguments of one phase of a trip of the multi-tick entry's loop: every POINTER comes from a fresh view, taken where
// this object is constructed (the compiler drops the loads of the fields the phase does not use); the launch constants are
// copied from the prologue's structures, which therefore keep no pointer alive across a trip.
struct TcPhase {
  TcArgs a;
  TcFuse fz;
  int n_ticks;  // the trips of this launch (read by the rewards phase alone: the last one is a closing trip, tc_fast.h)
  __device__ __forceinline__ TcPhase(const TcArgs &base, const TcFuse &fbase) {
    const TcKernargView k = tc_kernarg_view();
    {
#define WD_TC_FROM_VIEW(type, name) type name = k->name;
      WD_TC_PARAM_LIST(WD_TC_FROM_VIEW, WD_TC_NOTHING)
      WD_TC_FUSE_PARAM_LIST(WD_TC_FROM_VIEW, WD_TC_NOTHING)
#undef WD_TC_FROM_VIEW
      WD_TC_PACK();
      WD_TC_FUSE_PACK();
      this->a = a;
      this->fz = fz;
      (void)kNumAccelerationActions; (void)kNumTurnActions;
      this->n_ticks = k->kNumTicks;
    }
    // what is cheap to keep in registers: the launch constants the arithmetic uses (and the sizes the entry folded to
    // constants).  `runner_exits` is NOT among them: kept, it lives as two 64-bit masks that do not fit either.
    a.edge_hit_penalty = base.edge_hit_penalty; a.grid_length = base.grid_length; a.max_speed = base.max_speed;
    a.K = base.K; a.use_full_obs = base.use_full_obs; a.margin = base.margin;
    a.tag_reward = base.tag_reward; a.tag_penalty = base.tag_penalty; a.end_reward = base.end_reward;
    a.N = base.N; a.T = base.T; a.E = base.E; a.env_begin = base.env_begin;
    fz.stream_tag = fbase.stream_tag;
  }
};

// What a phase of tc_fast_impl reads its arguments through.  VIEW == false (every one-tick entry): the entry's own by-value
// structure, by reference -- the code is what it was.  VIEW == true (the multi-tick entry's loop): a TcPhase taken HERE.
template <bool VIEW> struct TcPhaseArgs { typedef const TcArgs &type; };
template <> struct TcPhaseArgs<true> { typedef const TcPhase type; };
template <bool VIEW>
__device__ __forceinline__ typename TcPhaseArgs<VIEW>::type tc_phase(const TcArgs &a, const TcFuse &fz) {
  if constexpr (VIEW) return TcPhase(a, fz);
  else return a;
}
__device__ __forceinline__ const TcArgs &tc_phase_a(const TcArgs &a) { return a; }
__device__ __forceinline__ const TcArgs &tc_phase_a(const TcPhase &p) { return p.a; }

}  // namespace
#endif  // __HIPCC__
