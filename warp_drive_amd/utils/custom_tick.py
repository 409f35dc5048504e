"""The host side of a custom environment's FUSED TICK (docs/custom_environments.md, "A fused tick"): the launch of a
`Hip<Name>Tick` entry written with include/wd_env_tick.h -- the step's own arguments followed by the kit's trailing
parameters, in the header's order -- as the (function, arguments, block, grid, dynamic LDS bytes) tuple `RolloutEngine`
asks an env's `tick_launch()` for, and a mixin that gives an env class `tick_launch()` / `rollout_launch()` from the
entry's name and the step's argument names.

What the kit does not do is refused with `UnsupportedRolloutShape`, never silently dropped: replica ranges, a batch
recorded inside the kernel, a policy or an actor evaluated inside the kernel, presampled actions, Box action spaces,
more than four heads.  An env with a reset pool needs nothing from here: `RolloutEngine` keeps the per-tick plan for it
(the mixin does not set TICK_POOL_RESET).

Further down: `FusedRolloutMixin` (the one-launch rollout with the policy inside the kernel, include/wd_env_rollout.h),
`FusedUpdateMixin` (the A2C / PPO update as five launches, include/wd_env_update.h) and `FusedEvaluateMixin` (one episode of
every replica in one launch, greedy or sampled, include/wd_env_evaluate.h).
"""
import numpy as np

from warp_drive_amd.utils.constants import Constants
from warp_drive_amd.utils.launch_checks import (NULL, UnsupportedRolloutShape, batch_arguments, check_packed, check_record,
                                                evaluation_outputs, rp_policy_floats, tick_tag, unpack_policy)
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
    pad = MAX_HEADS - len(sizes)
    args = list(env.cuda_step_function_feed(step_args))
    args += [sampler.rng_state, np.int32(len(sizes))]
    args += list(probabilities) + [NULL] * pad
    args += [np.int32(a) for a in sizes] + [np.int32(0)] * pad
    args += [table, np.int32(n_arrays), tick_tag(), np.int32(ticks)]
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


# ------------------------------------------------------------------------------------------------------------------
# The ONE-LAUNCH ROLLOUT with the policy inside the kernel (docs/custom_environments.md, "A policy inside the kernel"):
# the launch of a `Hip<Name>Rollout_H<width>` entry written with include/wd_env_rollout.h.
MAX_ACTIONS = 8  # WD_ROLLOUT_MAX_ACTIONS of include/wd_env_rollout.h


def rollout_policy_floats(obs_size, width, n_actions):
    """elements of the packed policy (training.policy_kernel.pack_rollout_policy; wd_rollout_policy_floats of the header)"""
    return rp_policy_floats(obs_size, width, n_actions)


def custom_rollout_launch(env, kernel_name, step_args, sampler, n_actions, packed, width, resetter, batch, ticks):
    """(function, arguments, block, grid, dynamic LDS bytes) of `kernel_name`, an entry whose parameters are the step's
    own -- `step_args` -- followed by WD_ROLLOUT_PARAMS: RNG state, packed policy, action count, reset table and its entry
    count, stream tag, the four batch tensors (observations [T, E, N, F] float32, actions [T, E, N, 1] int32, rewards
    [T, E, N] float32, done [T, E] int32, T >= ticks), and the tick count LAST (np.int32).  packed: the contiguous float32
    CUDA tensor of pack_rollout_policy for hidden width `width`.  Dynamic LDS: 4 bytes per packed float, rounded up
    to 16."""
    who = f"{type(env).__name__} ({kernel_name})"
    width, n_actions, ticks = int(width), int(n_actions), int(ticks)
    if not 1 <= n_actions <= MAX_ACTIONS:
        raise UnsupportedRolloutShape(f"{who}: {n_actions} actions were asked of the in-kernel policy of "
                                      f"wd_env_rollout.h (1 to {MAX_ACTIONS})")
    if ticks < 1:
        raise UnsupportedRolloutShape(f"{who}: a launch of {ticks} ticks was asked")
    fm, dm = env.cuda_function_manager, env.cuda_data_manager
    E, N = int(dm.meta_info("n_envs")), int(env.num_agents)
    F = int(dm.get_shape(Constants.OBSERVATIONS)[-1])
    n_w = rollout_policy_floats(F, width, n_actions)
    check_packed(packed, n_w, UnsupportedRolloutShape, f"{who}: the packed policy",
                 f"observation {F}, width {width}, {n_actions} actions")
    if batch is None:
        raise UnsupportedRolloutShape(f"{who}: the batch tensors are missing; the rollout records every tick")
    batch_args = batch_arguments(batch, ticks, E, N, F, error=UnsupportedRolloutShape, who=f"{who}: ")
    fm.initialize_functions([kernel_name])
    fn = fm.get_function(kernel_name)
    _, reset_args, _, _ = resetter.fused_launch(dm, 0, 0)  # builds / refreshes the descriptor table
    table, n_arrays = reset_args[0], reset_args[1]
    args = list(env.cuda_step_function_feed(step_args))
    args += [sampler.rng_state, packed, np.int32(n_actions), table, np.int32(n_arrays), tick_tag()] + batch_args + \
        [np.int32(ticks)]
    return fn, args, tick_block(N), fm.grid, (4 * n_w + 15) // 16 * 16


class FusedRolloutMixin(FusedTickMixin):
    """`has_live_policy_rollout()` and the `tick_launch(batch=..., policy=...)` form for an env class whose device source
    has, next to its fused tick entry, the entries `Hip<Name>Rollout_H<width>` written with include/wd_env_rollout.h.
    The class says ROLLOUT_KERNEL, a pattern with `{width}`; the entries' parameters are TICK_STEP_ARGS followed by
    WD_ROLLOUT_PARAMS.  `Trainer` takes the one launch under `trainer.fused_rollout_policy: "all"` only."""

    ROLLOUT_KERNEL = None
    ROLLOUT_POLICY_WIDTHS = (32, 64)
    ROLLOUT_MAX_THREADS = {32: 1024, 64: 512}  # the entries' __launch_bounds__: override to match the source
    ROLLOUT_POLICY_OPT_IN = True
    ticks_per_launch = 1

    def _policy_entry_refusal(self, pattern, widths, bounds, width, n_actions):
        """why this env / shape has no entry `pattern` (with `{width}`) that evaluates a policy of hidden width `width`
        with `n_actions` actions inside the kernel -- `widths`: the widths the entries exist for, `bounds`: their
        `__launch_bounds__` by width; None: it has"""
        space = self.action_space[0]
        if not isinstance(space, Discrete):
            return f"an action space of type {type(space).__name__} (one Discrete head only)"
        if not 1 <= int(n_actions) <= MAX_ACTIONS:
            return f"{int(n_actions)} actions (1 to {MAX_ACTIONS})"
        if int(width) not in tuple(widths) or int(width) not in bounds:
            return f"a hidden width of {int(width)} (entries: {sorted(widths)})"
        threads = tick_block(self.num_agents)[0]
        if threads > int(bounds[int(width)]):
            return (f"a block of {threads} threads ({self.num_agents} agents) over the launch bound "
                    f"{bounds[int(width)]} of the width-{int(width)} entry")
        if len(self.cuda_data_manager.reset_target_to_pool) > 0:
            return "a reset pool"
        name = pattern.format(width=int(width))
        if not self.cuda_function_manager.has_function(name):
            return f"the entry {name}, which the env's code object does not have"
        return None

    def _rollout_refusal(self, width, n_actions):
        """why this env / shape has no in-kernel policy of hidden width `width` with `n_actions` actions; None: it has"""
        return self._policy_entry_refusal(self.ROLLOUT_KERNEL, self.ROLLOUT_POLICY_WIDTHS, self.ROLLOUT_MAX_THREADS, width,
                                          n_actions)

    def has_live_policy_rollout(self, width, n_actions):
        """does an entry exist that evaluates a policy of hidden width `width` with `n_actions` actions for this env's
        shape?  (RolloutEngine and Trainer ask before they call `tick_launch(policy=...)`)"""
        return self._rollout_refusal(width, n_actions) is None

    def tick_launch(self, sampler, probabilities, resetter, env_range=None, batch=None, policy=None, **extra):
        """with `batch` and `policy` = (packed weights, hidden width): `ticks_per_launch` ticks in ONE launch of the
        Rollout entry of that width; with neither: the parent's fused tick"""
        if batch is None and policy is None:
            return super().tick_launch(sampler, probabilities, resetter, env_range=env_range, **extra)
        who = f"{type(self).__name__} ({self.ROLLOUT_KERNEL})"
        if env_range is not None:
            raise UnsupportedRolloutShape(f"{who}: a replica range {tuple(env_range)} was asked; the rollout of "
                                          "wd_env_rollout.h runs all replicas")
        asked = {"actor": "an in-kernel actor", "mean_batch": "an in-kernel actor's record of means",
                 "ou_params": "a Box action space (the OU draw)"}
        for key in extra:
            raise UnsupportedRolloutShape(f"{who}: {asked.get(key, repr(key))} was asked; the rollout of "
                                          "wd_env_rollout.h has no such variant")
        if batch is None:
            raise UnsupportedRolloutShape(f"{who}: an in-kernel policy without the batch tensors was asked; the rollout "
                                          "records every tick")
        if policy is None:
            raise UnsupportedRolloutShape(f"{who}: a batch recorded inside the kernel without an in-kernel policy was "
                                          "asked; the fused tick of wd_env_tick.h records nothing")
        packed, width = unpack_policy(policy, who=f"{who}: ")
        space = self.action_space[0]
        n_actions = int(space.n) if isinstance(space, Discrete) else 0
        why = self._rollout_refusal(width, n_actions)
        if why is not None:
            raise UnsupportedRolloutShape(f"{who}: {why} was asked of the in-kernel policy of wd_env_rollout.h")
        return custom_rollout_launch(self, self.ROLLOUT_KERNEL.format(width=width), self.TICK_STEP_ARGS, sampler,
                                     n_actions, packed, width, resetter, batch, int(self.ticks_per_launch))


# ------------------------------------------------------------------------------------------------------------------
# The UPDATE AS KERNELS (docs/custom_environments.md, "The update as kernels"): the six entries the macro
# WD_PG_UPDATE_ENTRIES(Name, F) of include/wd_env_update.h defines in the env's own code object.
class FusedUpdateMixin(FusedRolloutMixin):
    """`update_kernels_refusal()` and `update_kernels()` for an env class whose device source has, next to its Rollout
    entries, the update entries of include/wd_env_update.h.  The class says UPDATE_KERNEL_PREFIX -- "Hip<Name>Pg", the
    macro's first argument between "Hip" and "Pg" -- and UPDATE_OBS_SIZE, the macro's second argument: the observation
    floats of a row the entries were COMPILED for.  `Trainer` takes the five launches under
    `trainer.fused_update: "all"` only, on top of the one-launch rollout."""

    UPDATE_KERNEL_PREFIX = None
    UPDATE_OBS_SIZE = None

    def update_kernels_refusal(self, width, obs_size, n_actions):
        """(True, "") when this env's code object has update entries for a policy of hidden width `width` on `obs_size`
        observation floats with `n_actions` actions, else (False, why)"""
        from warp_drive_amd.training import pg_update_custom_kernels as pgck

        who = type(self).__name__
        if not self.UPDATE_KERNEL_PREFIX or self.UPDATE_OBS_SIZE is None:
            return False, f"{who} names no update entries (UPDATE_KERNEL_PREFIX, UPDATE_OBS_SIZE)"
        if int(width) not in pgck.HIDDEN:
            return False, f"hidden width {int(width)}: the update entries of wd_env_update.h exist for {list(pgck.HIDDEN)}"
        if not 1 <= int(n_actions) <= pgck.MAX_ACTIONS:
            return False, f"{int(n_actions)} actions: the update entries take 1 to {pgck.MAX_ACTIONS}"
        if not 1 <= int(self.UPDATE_OBS_SIZE) <= pgck.MAX_OBS:
            return False, f"{who}.UPDATE_OBS_SIZE = {self.UPDATE_OBS_SIZE}: the update entries take 1 to {pgck.MAX_OBS}"
        if int(obs_size) != int(self.UPDATE_OBS_SIZE):
            return False, (f"observation size {int(obs_size)}: the update entries of {who} were compiled for "
                           f"{int(self.UPDATE_OBS_SIZE)}")
        for name in pgck.all_kernel_names(self.UPDATE_KERNEL_PREFIX):
            if not self.cuda_function_manager.has_function(name):
                return False, f"the entry {name}, which the env's code object does not have"
        return True, ""

    def update_kernels(self, num_envs, batch_len, n_agents, width, obs_size, n_actions, device, **options):
        """the five launches (training/pg_update_custom_kernels.py::PgCustomUpdateKernels) on this env's entries"""
        from warp_drive_amd.training import pg_update_custom_kernels as pgck

        ok, why = self.update_kernels_refusal(width, obs_size, n_actions)
        if not ok:
            raise UnsupportedRolloutShape(f"{type(self).__name__}: {why}")
        return pgck.PgCustomUpdateKernels(self.cuda_function_manager, self.UPDATE_KERNEL_PREFIX, num_envs, batch_len,
                                          n_agents, width, obs_size, n_actions, device, **options)


# ------------------------------------------------------------------------------------------------------------------
# EVALUATION IN ONE LAUNCH (docs/custom_environments.md, "Evaluation in one launch"): the launch of a
# `Hip<Name>Evaluate_H<width>` entry written with include/wd_env_evaluate.h.
def custom_evaluate_launch(env, kernel_name, step_args, sampler, n_actions, packed, width, resetter, use_argmax, outputs,
                           action_trace, ticks):
    """(function, arguments, block, grid, dynamic LDS bytes) of `kernel_name`, an entry whose parameters are the step's
    own -- `step_args` -- followed by WD_EVALUATE_PARAMS: RNG state, packed policy, action count, reset table and its entry
    count, stream tag, use_argmax, reward_sum (float32, at least E * N elements), steps and done (int32, at least E), the
    action trace (int32 [>= ticks, E, N], or null), and the tick count LAST (np.int32).  Dynamic LDS: 4 bytes per packed
    float, rounded up to 16.  Whatever is not served is an `UnsupportedRolloutShape` that names the request."""
    who = f"{type(env).__name__} ({kernel_name})"
    width, n_actions, ticks = int(width), int(n_actions), int(ticks)
    if not 1 <= n_actions <= MAX_ACTIONS:
        raise UnsupportedRolloutShape(f"{who}: {n_actions} actions were asked of the in-kernel policy of "
                                      f"wd_env_evaluate.h (1 to {MAX_ACTIONS})")
    if ticks < 1:
        raise UnsupportedRolloutShape(f"{who}: an evaluation of {ticks} ticks was asked")
    fm, dm = env.cuda_function_manager, env.cuda_data_manager
    E, N = int(dm.meta_info("n_envs")), int(env.num_agents)
    F = int(dm.get_shape(Constants.OBSERVATIONS)[-1])
    n_w = rollout_policy_floats(F, width, n_actions)
    check_packed(packed, n_w, UnsupportedRolloutShape, f"{who}: the packed policy",
                 f"observation {F}, width {width}, {n_actions} actions")
    if not hasattr(outputs, "__getitem__") or any(key not in outputs for key in ("reward_sum", "steps", "done")):
        raise UnsupportedRolloutShape(f"{who}: outputs = {{'reward_sum': ..., 'steps': ..., 'done': ...}}, not {outputs!r}")
    out_args = evaluation_outputs(outputs, E, UnsupportedRolloutShape, reward_elements=E * N)
    if action_trace is not None:
        got = (tuple(getattr(action_trace, "shape", ())), getattr(action_trace, "dtype", None))
        check_record(action_trace, "action_trace", "int32", ticks, (E, N), UnsupportedRolloutShape,
                     f"{who}: action_trace must be a contiguous torch.int32 CUDA tensor [>= {ticks}, {E}, {N}], not {got}")
    if resetter is None:
        raise UnsupportedRolloutShape(f"{who}: the env has no resetter (EnvWrapper sets `cuda_env_resetter`); the "
                                      "evaluation restores every replica from the reset table")
    fm.initialize_functions([kernel_name])
    fn = fm.get_function(kernel_name)
    _, reset_args, _, _ = resetter.fused_launch(dm, 0, 0)  # builds / refreshes the descriptor table
    table, n_arrays = reset_args[0], reset_args[1]
    args = list(env.cuda_step_function_feed(step_args))
    args += [sampler.rng_state, packed, np.int32(n_actions), table, np.int32(n_arrays), tick_tag(),
             np.int32(1 if use_argmax else 0)] + out_args + [NULL if action_trace is None else action_trace, np.int32(ticks)]
    return fn, args, tick_block(N), fm.grid, (4 * n_w + 15) // 16 * 16


class FusedEvaluateMixin(FusedRolloutMixin):
    """`has_live_policy_evaluate()` and `evaluate_launch()` for an env class whose device source has, next to its Rollout
    entries, the entries `Hip<Name>Evaluate_H<width>` written with include/wd_env_evaluate.h.  The class says
    EVALUATE_KERNEL, a pattern with `{width}`; the entries' parameters are TICK_STEP_ARGS followed by WD_EVALUATE_PARAMS.
    Combines with `FusedUpdateMixin` in one class.  `Trainer.evaluate_episodes` takes the one launch under
    `trainer.fused_rollout_policy: "all"` only (EVALUATE_POLICY_OPT_IN)."""

    EVALUATE_KERNEL = None
    EVALUATE_MAX_THREADS = None  # the entries' __launch_bounds__ by width; None: the class's ROLLOUT_MAX_THREADS
    EVALUATE_POLICY_OPT_IN = True

    def _evaluate_refusal(self, width, n_actions):
        """why this env / shape has no one-launch evaluation of hidden width `width` with `n_actions` actions; None: it
        has"""
        if not self.EVALUATE_KERNEL:
            return f"an Evaluate entry, which {type(self).__name__} does not name (EVALUATE_KERNEL)"
        bounds = self.ROLLOUT_MAX_THREADS if self.EVALUATE_MAX_THREADS is None else self.EVALUATE_MAX_THREADS
        return self._policy_entry_refusal(self.EVALUATE_KERNEL, self.ROLLOUT_POLICY_WIDTHS, bounds, width, n_actions)

    def has_live_policy_evaluate(self, width, n_actions):
        """does an entry exist that runs one episode of every replica with a policy of hidden width `width` and
        `n_actions` actions inside it, for this env's shape?  (Trainer.evaluate_episodes asks before `evaluate_launch`)"""
        return self._evaluate_refusal(width, n_actions) is None

    def evaluate_launch(self, sampler, policy, use_argmax, outputs, action_trace=None, ticks=None):
        """One episode of every replica in ONE launch of the Evaluate entry of the policy's width: from the state,
        observation, `_timestep_` and `_done_` the arrays hold, at most `ticks` (default: episode_length) ticks of policy
        network -> action (use_argmax: the first maximum of the probabilities; else the rollout's counting draw) -> step,
        up to the replica's first done.  policy = (packed float32 CUDA tensor, hidden width) as in `tick_launch`.
        outputs = {"reward_sum": float32 [E, N], "steps": int32 [E], "done": int32 [E]}, CUDA tensors (at least that many
        elements); `action_trace` (optional) int32 [>= ticks, E, N]: row k = tick k's actions of the replicas still
        running.  The launch writes those, in sampled mode the sampler's epoch words, and the env's arrays: every replica
        is left as `reset_when_done(mode="force_reset")` leaves it (the table of `self.cuda_env_resetter`).
        Returns (function, arguments, block, grid, shared bytes)."""
        who = f"{type(self).__name__} ({self.EVALUATE_KERNEL})"
        packed, width = unpack_policy(policy, who=f"{who}: ")
        space = self.action_space[0]
        n_actions = int(space.n) if isinstance(space, Discrete) else 0
        why = self._evaluate_refusal(width, n_actions)
        if why is not None:
            raise UnsupportedRolloutShape(f"{who}: {why} was asked of the one-launch evaluation of wd_env_evaluate.h")
        T = int(self.episode_length if ticks is None else ticks)
        return custom_evaluate_launch(self, self.EVALUATE_KERNEL.format(width=width), self.TICK_STEP_ARGS, sampler,
                                      n_actions, packed, width, getattr(self, "cuda_env_resetter", None), use_argmax,
                                      outputs, action_trace, T)
