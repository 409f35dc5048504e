"""Device-resident rollout tick: sample every action head -> env step -> reset finished
replicas, with no host round trip between the launches.

The reference drives the same sequence from Python with one driver call per kernel, a
device->host sync on the done flags and three synchronisations per tick
(warp_drive/training/trainers/trainer_base.py:392-426; per reset it issues one launch
per registered array, pycuda_function_manager.py:686-753).  Here the whole tick is a
fixed LaunchPlan replayed from C (or captured once into a hipGraph):

    sample_actions(head 0) ... sample_actions(head H-1)   writes [E, n, H] actions directly
    Hip<Env>Step                                          obs / rewards / done in place
    reset_when_done_fused                                 every array + done/timestep, 1 launch

The probability tensors the sampler reads are whatever the policy wrote last (torch
tensors aliased in place); for kernel-only throughput they are constant uniform tensors.
"""
import os

import numpy as np
import torch

from warp_drive_amd.managers import hip_driver as drv
from warp_drive_amd.managers.function_manager import HIPSampler, _stream_tag
from warp_drive_amd.utils.constants import Constants
from warp_drive_amd.utils.launch_checks import UnsupportedRolloutShape  # noqa: F401  (its home; re-exported from here)
from warp_drive_amd.utils.spaces import Box, Discrete, MultiDiscrete

_ACTIONS = Constants.ACTIONS


# Replica cohorts of the fused tick (TagContinuous): a multi-tick run() splits the replicas into C ranges, each
# replayed on its own stream (LaunchPlan.add_cohort, wd_runtime.cpp), so one cohort's fetch, row flush, drain and
# kernel boundary run under the other cohort's work.  Measured at 2000 replicas (interleaved A/B medians): C = 1 24.4 us
# per tick, C = 2 21.9, C = 3 22.6 (docs/rounds/r07.md).  1 = one whole-range launch per tick.
TICK_COHORTS = int(os.environ.get("WD_TICK_COHORTS", "2"))
# Multi-tick form of the fused tick (TagContinuous, the shape-specialised entry): a run(n >= 2) is ONE launch whose
# blocks loop over the n ticks of their replica, so no replica waits at a kernel boundary for the slowest one
# (LaunchPlan.set_multi_tick; docs/rounds/r08.md).  0 = the cohort path exactly as before.  A custom env's tick written
# with include/wd_env_tick.h has the same form (its last argument is the tick count): env.rollout_launch().
TICK_ROLLOUT = int(os.environ.get("WD_TICK_ROLLOUT", "1"))
ROLLOUT_MAX_TICKS = 2048  # ticks per launch: ~45 ms at the BASELINE shape; longer runs are split
COHORT_ALIGN = 32  # cohort boundaries at multiples of 32 replicas: 32 rows of 4 * N bytes are N whole 128-byte lines


def cohort_bounds(n_envs, cohorts):
    """replica ranges [(begin, end), ...] of `cohorts` near-equal cohorts whose inner boundaries are multiples of
    COHORT_ALIGN replicas (never beyond n_envs: with few replicas the last cohorts are empty)"""
    last = n_envs // COHORT_ALIGN * COHORT_ALIGN
    cuts = [0] + [min(int(round(n_envs * c / cohorts / COHORT_ALIGN)) * COHORT_ALIGN, last)
                  for c in range(1, cohorts)] + [n_envs]
    return list(zip(cuts[:-1], cuts[1:]))


class RolloutEngine:
    def __init__(self, env_wrapper, sampler: HIPSampler, probabilities=None, reset_done=True, fused=True,
                 rollout_batch=None, rollout_policy=None, ticks_per_launch=None, presampled_actions=False,
                 damping=0.15, stddev=0.2, scale=1.0, rollout_actor=None, rollout_means=None):
        """probabilities: list (one per action head) of contiguous float32 CUDA tensors
        [n_envs, n_agents, n_actions_of_head]; None = uniform.  rollout_batch: the trainer's [T, E, ...] batch
        tensors for envs whose tick kernel fuses T ticks per launch and records every tick itself
        (CUDAClassicControlCartPoleEnv.tick_launch); rollout_policy: (packed weights, hidden width) of a small policy
        that such a kernel evaluates itself on every tick.  ticks_per_launch: env ticks per launch of THIS engine
        (None = the env object's own `ticks_per_launch` attribute); the env object is left as it was, so another
        engine on the same wrapper is not affected.  presampled_actions: the tick does NOT draw the actions -- whoever
        runs before it (the policy forward's epilogue, training/policy_kernel.py) has written `sampled_actions` -- and
        is the env's step + reset entry (`env.has_presampled_tick()`).  rollout_actor: (packed weights, hidden width,
        action_scale, action_bias) of a deterministic actor that a Box env's kernel evaluates itself on every tick
        (`env.has_live_actor_rollout(width)`), rollout_means: the [T, E] float32 record of its means.
        A one-dimensional `Box` action space: the
        one probability tensor [n_envs, n_agents, 1] holds the means of the actions, and the draw is
        sample_ou_process's OU / Gaussian one with `damping`, `stddev`, `scale` (HIPSampler.sample's defaults).
        With a reset pool the reset entry restarts finished replicas from it (HIPEnvironmentReset.reset_when_done:
        init_reset_pool() first); the fused tick does so itself for envs that say TICK_POOL_RESET."""
        self.ou_params = (float(damping), float(stddev), float(scale))
        env = env_wrapper.env
        self.presampled = bool(presampled_actions)
        saved = getattr(env, "ticks_per_launch", 1)
        if ticks_per_launch is not None:
            env.ticks_per_launch = int(ticks_per_launch)
        try:
            self._build(env_wrapper, sampler, probabilities, reset_done, fused, rollout_batch, rollout_policy,
                        rollout_actor, rollout_means)
        finally:
            if ticks_per_launch is not None:
                env.ticks_per_launch = saved

    def _build(self, env_wrapper, sampler, probabilities, reset_done, fused, rollout_batch, rollout_policy,
               rollout_actor=None, rollout_means=None):
        assert env_wrapper.env_backend == "hip"
        self.w = env_wrapper
        self.sampler = sampler
        dm = env_wrapper.cuda_data_manager
        E, N = env_wrapper.n_envs, env_wrapper.n_agents
        space = env_wrapper.env.action_space[0]
        self.continuous = isinstance(space, Box)
        if isinstance(space, MultiDiscrete):
            head_sizes = [int(v) for v in space.nvec]
        elif isinstance(space, Discrete):
            head_sizes = [int(space.n)]
        elif self.continuous and len(space.shape) == 1 and int(space.shape[0]) == 1:
            head_sizes = [1]  # one float action: the mean per replica and agent
        else:
            raise NotImplementedError("RolloutEngine drives discrete action spaces and one-dimensional Box ones")
        pools = len(dm.reset_target_to_pool) > 0
        dev = dm.data_on_device_via_torch(_ACTIONS).device
        if probabilities is None and self.continuous:
            probabilities = [torch.zeros((E, N, 1), dtype=torch.float32, device=dev)]
        elif probabilities is None:
            probabilities = [torch.full((E, N, a), 1.0 / a, dtype=torch.float32, device=dev) for a in head_sizes]
        assert len(probabilities) == len(head_sizes)
        for p, a in zip(probabilities, head_sizes):
            assert p.is_contiguous() and p.dtype == torch.float32 and tuple(p.shape) == (E, N, a)
        self.probabilities = probabilities
        self.head_sizes = head_sizes
        self.plan = drv.LaunchPlan()
        actions = dm.device_data(_ACTIONS)  # [E, N, H] int32 (H = 1 for Discrete)
        H = len(head_sizes)
        self.entry_names = []
        self.cohorts = 1  # replica cohorts a multi-tick run() replays in parallel (one kernel per cohort and tick)
        self._graph_ticks = 0
        self.rollout_kernel_name = None  # the multi-tick entry a run(n >= 2) launches (None: one launch per tick)
        # an env class that offers tick_launch() fuses sampling, step and reset in its own kernel
        # (restarts from a reset pool draw random members: that stays with the pool reset kernel, unless the env's tick
        # kernel draws them itself -- TICK_POOL_RESET)
        # ... or its T-tick rollout entries do while its single tick does not (ROLLOUT_POOL_RESET: TagGridWorld with a
        # reset pool) and this engine is such a rollout: the batch tensors and more than one tick per launch
        pool_rollout = bool(getattr(env_wrapper.env, "ROLLOUT_POOL_RESET", False) and rollout_batch is not None
                            and int(getattr(env_wrapper.env, "ticks_per_launch", 1)) > 1)
        self.fused = bool(fused and reset_done and hasattr(env_wrapper.env, "tick_launch")
                          and H == getattr(env_wrapper.env, "TICK_HEADS", 2)
                          and (not pools or getattr(env_wrapper.env, "TICK_POOL_RESET", False) or pool_rollout)
                          and getattr(env_wrapper.env, "can_fuse_tick", lambda: True)())
        # env ticks per launch (> 1 only for envs whose fused kernel loops over ticks, fixed policy)
        self.ticks_per_launch = int(getattr(env_wrapper.env, "ticks_per_launch", 1)) if self.fused else 1
        if self.fused:
            # whole tick = ONE launch: sampling, step and reset fused in the env's tick kernel
            extra = {"batch": rollout_batch} if rollout_batch is not None else {}
            if rollout_policy is not None:
                extra["policy"] = rollout_policy
            if self.continuous:
                extra["ou_params"] = self.ou_params
            if rollout_actor is not None:
                has = getattr(env_wrapper.env, "has_live_actor_rollout", None)
                if has is None or len(rollout_actor) != 4 or not has(int(rollout_actor[1])):
                    raise UnsupportedRolloutShape(
                        f"{type(env_wrapper.env).__name__} has no rollout kernel that evaluates an actor of hidden width "
                        f"{rollout_actor[1] if len(rollout_actor) > 1 else None}")
                extra["actor"] = rollout_actor
                if rollout_means is not None:
                    extra["mean_batch"] = rollout_means
            if self.presampled and not env_wrapper.env.has_presampled_tick():
                raise UnsupportedRolloutShape("this env / shape has no step + reset entry for given actions")
            if rollout_policy is not None:
                has = getattr(env_wrapper.env, "has_live_policy_rollout", None)
                if has is None or not has(int(rollout_policy[1]), int(head_sizes[0])):
                    raise UnsupportedRolloutShape(
                        f"{type(env_wrapper.env).__name__} has no rollout kernel that evaluates a policy of hidden width "
                        f"{rollout_policy[1]} for this shape")
            fn, args, block, grid, shared = env_wrapper.env.tick_launch(sampler, None if self.presampled else probabilities,
                                                                        env_wrapper.env_resetter, **extra)
            self.plan.add(fn, args, block, grid, shared)
            self.step_entry = 0
            self.step_kernel_name = fn.name
            self.entry_names.append(fn.name)
            # replica cohorts: envs whose tick takes a replica range (TagContinuous); the multi-tick form: any fused env
            # that offers rollout_launch(), with or without ranges (a custom env's tick of include/wd_env_tick.h)
            ranges = bool(getattr(env_wrapper.env, "TICK_ENV_RANGES", False))
            if (not self.presampled and rollout_policy is None and rollout_batch is None and self.ticks_per_launch == 1
                    and (ranges or hasattr(env_wrapper.env, "rollout_launch"))):
                if ranges:
                    self._add_cohorts(env_wrapper, sampler, probabilities, E, grid[0], dev)
                if TICK_ROLLOUT and hasattr(env_wrapper.env, "rollout_launch"):
                    multi = env_wrapper.env.rollout_launch(sampler, probabilities, env_wrapper.env_resetter)
                    if multi is not None:
                        self.plan.set_multi_tick(*multi, max_ticks=ROLLOUT_MAX_TICKS)
                        self.rollout_kernel_name = multi[0].name
            return
        assert not self.presampled, "presampled_actions needs the env's fused tick entry"
        if rollout_actor is not None:
            raise UnsupportedRolloutShape("an in-kernel actor needs the env's fused tick entry")
        if self.continuous:  # OU / Gaussian around the means, HIPSampler.sample's launch
            fn, args, block, grid, shared = sampler.ou_launch(dm, probabilities[0], _ACTIONS, E * N, *self.ou_params,
                                                              _stream_tag(_ACTIONS))
            self.plan.add(fn, args, block, grid, shared)
            self.entry_names.append("sample_ou_process")
        for k, (p, a) in enumerate(zip([] if self.continuous else probabilities, head_sizes)):
            fn, args, block, grid, shared = sampler.categorical_launch(
                p, actions, E * N, a, False, _stream_tag(f"{_ACTIONS}_{k}"), out_stride=H, out_offset=k)
            self.plan.add(fn, args, block, grid, shared)
            self.entry_names.append(f"sample_actions[{k}]")
        fn, args, block, grid, shared = env_wrapper.env.step_launch()
        self.plan.add(fn, args, block, grid, shared)
        self.step_entry = len(self.entry_names)
        self.step_kernel_name = fn.name
        self.entry_names.append(fn.name)
        if reset_done and not pools:
            fn, args, block, grid = env_wrapper.env_resetter.fused_launch(dm, np.int32(0), 1)
            self.plan.add(fn, args, block, grid, 0)
            self.entry_names.append(fn.name)
        elif reset_done:  # HIPEnvironmentReset.reset_when_done(mode="if_done"): table, pools, then done / timestep
            resetter = env_wrapper.env_resetter
            if not resetter._random_initialized:
                raise RuntimeError("the env has a reset pool: call init_reset_pool() before building the rollout")
            fn, args, block, grid = resetter.fused_launch(dm, np.int32(0), 0)
            launches = [(fn, args, block, grid)] + resetter.pool_launches(dm, np.int32(0)) + \
                [resetter.undo_launch(dm, np.int32(0))]
            for fn, args, block, grid in launches:
                self.plan.add(fn, args, block, grid, 0)
                self.entry_names.append(fn.name)

    def _add_cohorts(self, env_wrapper, sampler, probabilities, E, blocks, dev):
        """split the fused tick into replica cohorts when every cohort still covers at least half of the CUs"""
        C = min(4, TICK_COHORTS)  # caller's stream + side streams within the default 4 hardware queues
        if C < 2:
            return
        half_cus = torch.cuda.get_device_properties(dev).multi_processor_count // 2
        bounds = cohort_bounds(E, C)
        epb = max(1, -(-E // blocks))  # replicas per block
        if any(-(-(e - b) // epb) < half_cus for b, e in bounds):
            return
        env = env_wrapper.env
        for c, rng in enumerate(bounds):
            fn, args, block, grid, shared = env.tick_launch(sampler, probabilities, env_wrapper.env_resetter, env_range=rng)
            self.plan.add_cohort(0, c, fn, args, block, grid, shared)
        self.cohorts = self.plan.cohorts

    def run(self, ticks, stream=None):
        """Enqueue `ticks` rollout ticks (asynchronous).  With a multi-tick entry (`rollout_kernel_name`), ticks >= 2 are
        launches of it on `stream`; else, with cohorts, ticks >= 2 fork the cohorts onto their own streams and join
        them back into `stream` before returning."""
        self.plan.run(ticks, stream)

    def run_graph(self, ticks, ticks_per_graph=10, stream=None):
        """Same, replaying a hipGraph that holds `ticks_per_graph` ticks."""
        assert ticks % ticks_per_graph == 0
        if self._graph_ticks != ticks_per_graph:
            self.plan.instantiate_graph(ticks_per_graph, stream)
            self._graph_ticks = ticks_per_graph
        self.plan.run_graph(ticks // ticks_per_graph, stream)
