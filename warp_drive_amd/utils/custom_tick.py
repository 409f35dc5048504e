"""The host side of a custom environment's FUSED TICK (docs/custom_environments.md, "A fused tick"): the launch of a
`Hip<Name>Tick` entry written with include/wd_env_tick.h -- the step's own arguments followed by the kit's trailing
parameters, in the header's order -- as the (function, arguments, block, grid, dynamic LDS bytes) tuple `RolloutEngine`
asks an env's `tick_launch()` for, and a mixin that gives an env class `tick_launch()` / `rollout_launch()` from the
entry's name and the step's argument names.

What the kit does not do is refused with `UnsupportedRolloutShape`, never silently dropped: replica ranges, a batch
recorded inside the kernel, a policy or an actor evaluated inside the kernel, presampled actions, Box action spaces,
more than four heads.  An env with a reset pool needs nothing from here: `RolloutEngine` keeps the per-tick plan for it
(the mixin does not set TICK_POOL_RESET).
"""
import numpy as np

from warp_drive_amd.rollout import UnsupportedRolloutShape
from warp_drive_amd.utils.spaces import Box, Discrete, MultiDiscrete

MAX_HEADS = 4  # WD_TICK_MAX_HEADS of include/wd_env_tick.h


def tick_block(num_agents):
    """one thread per agent, rounded up to whole wavefronts"""
    return ((int(num_agents) + 63) // 64 * 64, 1, 1)


def tick_head_sizes(env):
    """actions per head of the env's (Discrete or MultiDiscrete) action space, one entry per head"""
    space = env.action_space[0]
    if isinstance(space, Box):
        raise UnsupportedRolloutShape(f"{type(env).__name__}: a Box action space was asked of the fused tick of "
                                      "wd_env_tick.h, which draws categorical actions only")
    if isinstance(space, MultiDiscrete):
        sizes = [int(v) for v in space.nvec]
    elif isinstance(space, Discrete):
        sizes = [int(space.n)]
    else:
        raise UnsupportedRolloutShape(f"{type(env).__name__}: an action space of type {type(space).__name__} was asked "
                                      "of the fused tick of wd_env_tick.h (Discrete and MultiDiscrete only)")
    if len(sizes) > MAX_HEADS:
        raise UnsupportedRolloutShape(f"{type(env).__name__}: {len(sizes)} action heads were asked of the fused tick of "
                                      f"wd_env_tick.h; more than {MAX_HEADS} heads are not supported")
    return sizes


def custom_tick_launch(env, tick_kernel_name, step_args, sampler, probabilities, resetter, ticks=1):
    """(function, arguments, block, grid, dynamic LDS bytes) of `tick_kernel_name`, an entry whose parameters are the
    step's own -- `step_args`, the names `env.cuda_step_function_feed` resolves -- followed by WD_TICK_PARAMS:
    RNG state, number of heads, four probability pointers and four head sizes (unused ones null / 0), reset table and
    its entry count, stream tag, and the tick count LAST (np.int32: a launch plan's multi-tick form rewrites it).
    probabilities: one contiguous float32 tensor [n_envs, n_agents, actions of the head] per head."""
    from warp_drive_amd.managers.function_manager import _stream_tag

    if probabilities is None:
        raise UnsupportedRolloutShape(f"{type(env).__name__}: presampled actions were asked of {tick_kernel_name}, "
                                      "which draws its actions itself")
    sizes = tick_head_sizes(env)
    if len(probabilities) != len(sizes):
        raise ValueError(f"{tick_kernel_name}: {len(probabilities)} probability tensors for {len(sizes)} action heads")
    fm, dm = env.cuda_function_manager, env.cuda_data_manager
    fm.initialize_functions([tick_kernel_name])
    fn = fm.get_function(tick_kernel_name)
    _, reset_args, _, _ = resetter.fused_launch(dm, 0, 0)  # builds / refreshes the descriptor table
    table, n_arrays = reset_args[0], reset_args[1]
    null = np.uint64(0)
    pad = MAX_HEADS - len(sizes)
    args = list(env.cuda_step_function_feed(step_args))
    args += [sampler.rng_state, np.int32(len(sizes))]
    args += list(probabilities) + [null] * pad
    args += [np.int32(a) for a in sizes] + [np.int32(0)] * pad
    args += [table, np.int32(n_arrays), _stream_tag("tick"), np.int32(ticks)]
    return fn, args, tick_block(env.num_agents), fm.grid, 0


class FusedTickMixin:
    """`tick_launch()` and `rollout_launch()` for an env class whose device source has a fused tick entry.  The class says
    TICK_KERNEL (the entry's name) and TICK_STEP_ARGS (the step's argument names, as `cuda_step_function_feed` takes
    them); the entry's parameters are those followed by WD_TICK_PARAMS."""

    TICK_KERNEL = None
    TICK_STEP_ARGS = None

    @property
    def TICK_HEADS(self):
        """action heads of the env: what RolloutEngine compares with the heads it samples"""
        space = self.action_space[0]
        if isinstance(space, MultiDiscrete):
            return len(space.nvec)
        if isinstance(space, Box):
            return int(space.shape[0]) if len(space.shape) == 1 else 0
        return 1

    def has_presampled_tick(self):
        """the kit has no step + reset entry for actions somebody else drew"""
        return False

    def tick_launch(self, sampler, probabilities, resetter, env_range=None, **extra):
        """one tick in one launch: the draw of every head, the step, the restart of finished replicas"""
        who = f"{type(self).__name__} ({self.TICK_KERNEL})"
        if env_range is not None:
            raise UnsupportedRolloutShape(f"{who}: a replica range {tuple(env_range)} was asked; the fused tick of "
                                          "wd_env_tick.h runs all replicas")
        asked = {"batch": "a batch recorded inside the kernel", "policy": "an in-kernel policy",
                 "actor": "an in-kernel actor", "mean_batch": "an in-kernel actor's record of means",
                 "ou_params": "a Box action space (the OU draw)"}
        for key in extra:
            raise UnsupportedRolloutShape(f"{who}: {asked.get(key, repr(key))} was asked; the fused tick of "
                                          "wd_env_tick.h has no such variant")
        return custom_tick_launch(self, self.TICK_KERNEL, self.TICK_STEP_ARGS, sampler, probabilities, resetter, ticks=1)

    def rollout_launch(self, sampler, probabilities, resetter):
        """the same launch as the multi-tick form of a launch plan: its last argument, the tick count, is rewritten per
        run (LaunchPlan.set_multi_tick)"""
        return self.tick_launch(sampler, probabilities, resetter)
