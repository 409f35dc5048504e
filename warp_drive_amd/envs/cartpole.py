"""ClassicControl CartPole, single agent per replica (BASELINE config 5).

Host-side mirror of reference example_envs/single_agent/classic_control/cartpole/
cartpole.py:19-141 and single_agent/base.py.  The reference's CPU step delegates to
third-party `gym.envs.classic_control.CartPoleEnv` (absent here); this class carries the
classic constants itself and its CPU step is the same Euler update the reference's device
kernel implements (cartpole_step_numba.py:29-83).  Parity is pinned by a trajectory recorded from
that kernel source run under a numba.cuda stand-in (tests/golden/cp_traj.npz).
The device step launches `HipClassicControlCartPoleEnvStep`.
"""
import math

import numpy as np

from warp_drive_amd.utils import spaces
from warp_drive_amd.utils.constants import Constants
from warp_drive_amd.utils.data_feed import DataFeed
from warp_drive_amd.utils.gpu_environment_context import CUDAEnvironmentContext
from warp_drive_amd.utils.launch_checks import (NULL, SingleAgentDeviceEnv, UnsupportedRolloutShape, batch_arguments,
                                                rp_pad4, rp_policy_floats, tick_tag, unpack_policy)

_OBSERVATIONS = Constants.OBSERVATIONS
_ACTIONS = Constants.ACTIONS
_REWARDS = Constants.REWARDS


class CartPolePhysics:
    """The constants of gym's CartPoleEnv (classic_control/cartpole.py in gym >= 0.26)."""
    gravity = 9.8
    masscart = 1.0
    masspole = 0.1
    length = 0.5  # half the pole's length
    force_mag = 10.0
    tau = 0.02
    theta_threshold_radians = 12 * 2 * math.pi / 360
    x_threshold = 2.4


def euler_step(state, action, p=CartPolePhysics):
    """One Euler tick with the dtype flow of the reference's Numba kernel
    (float32 state/scalars; the 4.0/3.0 literal widens thetaacc/xacc to float64)."""
    f32 = np.float32
    x, x_dot, theta, theta_dot = (f32(v) for v in state)
    force = f32(p.force_mag) if action > 0.5 else f32(-p.force_mag)
    costheta, sintheta = np.cos(theta), np.sin(theta)  # numpy float32 kernels
    total_mass = f32(p.masspole + p.masscart)
    polemass_length = f32(p.masspole * p.length)
    temp = f32(f32(force + f32(f32(polemass_length * f32(theta_dot * theta_dot)) * sintheta)) / total_mass)
    den = np.float64(f32(p.length)) * (4.0 / 3.0 - np.float64(f32(f32(f32(p.masspole) * f32(costheta * costheta)) / total_mass)))
    thetaacc = np.float64(f32(f32(f32(p.gravity) * sintheta) - f32(costheta * temp))) / den
    xacc = np.float64(temp) - np.float64(polemass_length) * thetaacc * np.float64(costheta) / np.float64(total_mass)
    tau = f32(p.tau)
    nx = f32(x + f32(tau * x_dot))
    nx_dot = f32(np.float64(x_dot) + np.float64(tau) * xacc)
    ntheta = f32(theta + f32(tau * theta_dot))
    ntheta_dot = f32(np.float64(theta_dot) + np.float64(tau) * thetaacc)
    return np.array([nx, nx_dot, ntheta, ntheta_dot], dtype=f32)


class ClassicControlCartPoleEnv:
    name = "ClassicControlCartPoleEnv"

    def __init__(self, episode_length=500, env_backend="cpu", reset_pool_size=0, seed=None, initial_state=None):
        """`initial_state` (optional, beyond the reference's signature): a fixed start state instead of
        the seeded draw -- the golden-trajectory tests start from the fixture's."""
        self.initial_state = None if initial_state is None else np.asarray(initial_state, dtype=np.float32)
        self.num_agents = 1
        self.agents = {0: True}
        assert episode_length > 0
        self.episode_length = episode_length
        self.env_backend = env_backend
        self.reset_pool_size = reset_pool_size
        self.seed = seed
        self.timestep = None
        self.physics = CartPolePhysics
        self._rng = np.random.default_rng(seed)
        high = np.array([self.physics.x_threshold * 2, np.finfo(np.float32).max,
                         self.physics.theta_threshold_radians * 2, np.finfo(np.float32).max], dtype=np.float32)
        self.action_space = {0: spaces.Discrete(2)}
        self.observation_space = {0: spaces.Box(-high, high, dtype=np.float32)}
        self.state = None

    def _draw_initial_state(self, fixed):
        if fixed and self.initial_state is not None:
            return np.asarray(self.initial_state, dtype=np.float32).copy()
        rng = np.random.default_rng(self.seed) if fixed else self._rng
        return rng.uniform(low=-0.05, high=0.05, size=(4,)).astype(np.float32)

    def reset(self):
        self.timestep = 0
        self.state = self._draw_initial_state(fixed=self.reset_pool_size < 2)
        return {0: self.state.copy()}

    def step(self, action=None):
        self.timestep += 1
        assert isinstance(action, dict) and len(action) == 1
        self.state = euler_step(self.state, action[0], self.physics)
        x, theta = self.state[0], self.state[2]
        p = self.physics
        terminated = bool(x < -p.x_threshold or x > p.x_threshold or theta < -p.theta_threshold_radians
                          or theta > p.theta_threshold_radians)
        done = {"__all__": self.timestep >= self.episode_length or terminated}
        return {0: self.state.copy()}, {0: 1.0}, done, {}


class CUDAClassicControlCartPoleEnv(SingleAgentDeviceEnv, CUDAEnvironmentContext, ClassicControlCartPoleEnv):
    """The device side.  Step, reset pool, `has_live_policy_evaluate` and `evaluate_launch`
    (HipClassicControlCartPoleEnvEvaluate_H<width>: the network runs on the state, which is Cartpole's observation) are
    utils/launch_checks.py::SingleAgentDeviceEnv's."""
    STATE_DIM = 4
    _PACKED_DETAIL = "width {width}, {n_act} actions"

    def __init__(self, *args, **kwargs):
        ClassicControlCartPoleEnv.__init__(self, *args, **kwargs)
        CUDAEnvironmentContext.__init__(self)

    def get_data_dictionary(self):
        p = self.physics
        feed = DataFeed()
        initial_state = self._draw_initial_state(fixed=True)
        feed.add_data(name="state", data=np.atleast_2d(initial_state),
                      save_copy_and_apply_at_reset=self.reset_pool_size < 2)
        feed.add_data_list([
            ("gravity", p.gravity), ("masspole", p.masspole), ("total_mass", p.masspole + p.masscart),
            ("length", p.length), ("polemass_length", p.masspole * p.length), ("force_mag", p.force_mag),
            ("tau", p.tau), ("theta_threshold_radians", p.theta_threshold_radians),
            ("x_threshold", p.x_threshold),
        ])
        return feed

    _STEP_ARGS = ["state", _ACTIONS, "_done_", _REWARDS, _OBSERVATIONS, "gravity", "masspole", "total_mass",
                  "length", "polemass_length", "force_mag", "tau", "theta_threshold_radians", "x_threshold",
                  "_timestep_", ("episode_length", "meta"), ("n_envs", "meta")]

    def _step_args(self):
        return self._STEP_ARGS

    def _obs_size(self):
        return 4   # the state is the observation: no data-manager query

    ROLLOUT_POLICY_WIDTHS = (32, 64)   # HipClassicControlCartPoleEnvRollout_H<width>

    # ------------------------------------------------------------------ with a reset pool (csrc/kernels/cartpole_pool.hip)
    # HipClassicControlCartPoleEnvRollout_P / _P_H<width> run T ticks per launch and draw the pool row of a finished
    # replica inside the kernel.  There is no fused SINGLE tick for the pooled env: without the batch tensors
    # RolloutEngine builds sample, step, table reset, pool launch, undo.
    @property
    def ROLLOUT_POOL_RESET(self):
        """RolloutEngine: the T-tick entries restart from the pool inside the kernel (True with a pool; without one the
        question does not arise and every answer stays as it was)"""
        return self._has_pool()

    POOL_ROLLOUT_MAX_LDS = 64 * 1024   # LDS a plain launch may ask for, static + dynamic (two such blocks fit a CU's 160 KB)
    POOL_ROLLOUT_STATIC_LDS = 256      # the entries' own static LDS (the block's vote on the pool rows' angles)
    # "auto" stages the pool in LDS when that fits the limit (1000 rows with a [64, 64] policy: 35 KB) and else reads it
    # from global memory (10 000 rows are 160 KB); "lds" / "global" force one (a forced "lds" beyond the limit is refused)
    pool_placement = "auto"

    @property
    def ROLLOUT_POLICY_OPT_IN(self):
        """Trainer: with a reset pool the one launch only under `trainer.fused_rollout_policy: "all"` (a pooled Cartpole
        trained today keeps today's per-tick path and its draws); without a pool it is the default, as before"""
        return self._has_pool()

    def _has_pool(self):
        dm = getattr(self, "cuda_data_manager", None)
        if dm is not None and getattr(dm, "reset_target_to_pool", None) is not None:
            return len(dm.reset_target_to_pool) > 0
        return self.reset_pool_size >= 2

    @staticmethod
    def pool_rollout_lds_bytes(width, n_actions, n_pool, staged):
        """dynamic LDS of the ..._P entries: the packed policy (width 0, the fixed-probability entry: none) rounded up
        to whole float4, then -- staged -- the pool's rows of 16 bytes"""
        n_w = rp_policy_floats(4, width, n_actions) if int(width) else 0
        return 4 * rp_pad4(n_w) + (16 * int(n_pool) if staged else 0)

    def _pool_rollout(self, width, n_actions):
        """(pool array's name, rows, staged) when the pooled rollout of this width (0: fixed probabilities) serves the env as
        it stands, else the reason it does not (a str)"""
        dm = self.cuda_data_manager
        pools = dict(dm.reset_target_to_pool)
        if sorted(pools) != ["state"]:
            return f"the pooled rollout restarts `state` from its pool and nothing else, not {sorted(pools)}"
        shape = tuple(dm.get_shape(pools["state"]))
        if len(shape) != 3 or shape[0] < 1 or shape[1:] != (1, 4):
            return f"the pool of `state` must be [n, 1, 4], not {shape}"
        dtype = getattr(dm, "get_dtype", lambda name: "float32")(pools["state"])
        if "float32" not in str(dtype):
            return f"the pool of `state` must be float32, not {dtype}"
        if sorted(dm.reset_data_list) != [_OBSERVATIONS]:
            return f"the pooled rollout restores the observations and nothing else, not {sorted(dm.reset_data_list)}"
        if getattr(getattr(self, "cuda_env_resetter", None), "_pool_rng", None) is None:
            return "the pool generator is not initialised: call init_reset_pool() before building the rollout"
        if int(width) not in (0,) + tuple(self.ROLLOUT_POLICY_WIDTHS):
            return f"no in-kernel policy of width {width}"
        if not 1 <= int(n_actions) <= 8:
            return f"the pooled rollout draws 1 .. 8 actions, not {n_actions}"
        name = self.cuda_step.name.replace("Step", f"Rollout_P_H{int(width)}" if int(width) else "Rollout_P")
        if not self.cuda_function_manager.has_function(name):
            return f"{name} is not in the kernel manifest"
        n_pool = int(shape[0])
        placement = self.pool_placement
        if placement not in ("auto", "lds", "global"):
            return f"pool_placement: \"auto\", \"lds\" or \"global\", not {placement!r}"
        staged_bytes = self.pool_rollout_lds_bytes(width, n_actions, n_pool, True) + self.POOL_ROLLOUT_STATIC_LDS
        staged = placement == "lds" or (placement == "auto" and staged_bytes <= self.POOL_ROLLOUT_MAX_LDS)
        need = self.pool_rollout_lds_bytes(width, n_actions, n_pool, staged) + self.POOL_ROLLOUT_STATIC_LDS
        if need > self.POOL_ROLLOUT_MAX_LDS:
            return f"{need} bytes of LDS for a pool of {n_pool} rows exceed the workgroup's {self.POOL_ROLLOUT_MAX_LDS}"
        return pools["state"], n_pool, staged

    def has_pool_rollout(self, n_actions=2):
        """with a reset pool: does HipClassicControlCartPoleEnvRollout_P (fixed probabilities) serve this env?"""
        return bool(self._has_pool() and not isinstance(self._pool_rollout(0, n_actions), str))

    def has_live_policy_rollout(self, width, n_actions):
        """does a rollout kernel exist that evaluates the policy network itself (…Rollout_H<width>; with a reset pool
        …Rollout_P_H<width>, which serves pools == {state: [n, 1, 4] float32}, reset arrays == {observations}, an
        initialised pool generator, and a staging whose LDS fits)?  (RolloutEngine asks before it calls
        `tick_launch(policy=...)`)"""
        if self._has_pool():
            return bool(int(width) in self.ROLLOUT_POLICY_WIDTHS and not isinstance(self._pool_rollout(width, n_actions), str))
        return int(width) in self.ROLLOUT_POLICY_WIDTHS and int(n_actions) <= 8 and \
            self.cuda_function_manager.has_function(self._entry(f"Rollout_H{int(width)}"))

    def tick_launch(self, sampler, probabilities, resetter, env_range=None, batch=None, policy=None):
        """Fused rollout tick(s): sample + step + reset of a finished replica, `ticks_per_launch`
        times in ONE launch (HipClassicControlCartPoleEnvTick).  probabilities = [float32 CUDA tensor
        [E, 1, n_actions]]; `_done_` reports the last tick of the launch.  `batch` (optional) = the
        trainer's batch tensors {"obs": [T, E, 1, 4] float32, "actions": [T, E, 1, 1] int32, "rewards":
        [T, E, 1] float32, "done": [T, E] int32} with T >= ticks_per_launch: tick k of the launch writes
        their row k (what trainer_base.py:392-426 records per tick).  `policy` (optional) = (packed float32
        CUDA tensor from training.policy_kernel.pack_rollout_policy, hidden width): the launch evaluates the
        policy network on every tick's observation itself (HipClassicControlCartPoleEnvRollout_H<width>)
        instead of reading `probabilities`.  An env with a reset pool: `_pool_tick_launch` (the ..._P entries)."""
        assert env_range is None and len(probabilities) == 1
        fm, dm = self.cuda_function_manager, self.cuda_data_manager
        if int(self.ticks_per_launch) < 1:   # (cp_tick_impl's last tick runs whatever `ticks` says: tick -1 of a launch of none)
            raise UnsupportedRolloutShape(f"ticks_per_launch must be at least 1, not {self.ticks_per_launch}")
        if self._has_pool():
            return self._pool_tick_launch(sampler, probabilities, resetter, batch, policy)
        name = self._entry("Tick")
        shared, pol_args = 0, [NULL, np.int32(0)]
        if policy is not None:
            packed, width = policy   # (as given: a malformed `policy` is the caller's bug here, not a refusal)
            n_act = int(probabilities[0].shape[-1])
            if not self.has_live_policy_rollout(width, n_act):
                raise UnsupportedRolloutShape(f"no in-kernel policy of width {width} with {n_act} actions")
            n_w = self._checked_policy(packed, width, n_act, AssertionError)
            name = self._entry(f"Rollout_H{width}")
            shared, pol_args = 4 * n_w, [packed, np.int32(width)]
        fm.initialize_functions([name])
        _, reset_args, _, _ = resetter.fused_launch(dm, 0, 0)  # builds / refreshes the descriptor table
        _, args, block, grid, _ = self.step_launch()
        args = list(args) + [sampler.rng_state, probabilities[0], np.int32(probabilities[0].shape[-1]), reset_args[0],
                             reset_args[1], tick_tag(), np.int32(self.ticks_per_launch)] + \
            self._batch_arguments(batch) + pol_args + [np.int32(self.invariant_divide_ok())]
        return fm.get_function(name), args, block, grid, shared

    def _batch_arguments(self, batch):
        """the four `*_batch` arguments of a tick / rollout entry (nulls without batch tensors), their shapes checked"""
        return batch_arguments(batch, int(self.ticks_per_launch), self._n_envs(), 1, 4)

    def _pool_tick_launch(self, sampler, probabilities, resetter, batch, policy):
        """`tick_launch` for the env with a reset pool: HipClassicControlCartPoleEnvRollout_P (fixed probabilities) or
        ..._P_H<width> (`policy`), T = ticks_per_launch > 1 ticks with the batch tensors.  Arguments: the unpooled
        entry's, then the pool generator's words, the pool, its row count and 1 / 0 = the kernel stages the pool in LDS /
        reads it from global memory (`pool_placement`).  Whatever the entries do not serve raises
        UnsupportedRolloutShape with the reason."""
        fm, dm = self.cuda_function_manager, self.cuda_data_manager
        if batch is None or int(self.ticks_per_launch) < 2:
            raise UnsupportedRolloutShape("Cartpole with a reset pool has no fused single tick: its one-launch rollout "
                                          "needs the batch tensors and ticks_per_launch > 1")
        n_act = int(probabilities[0].shape[-1])
        width, packed = 0, None
        if policy is not None:
            packed, width = unpack_policy(policy)
            if width not in self.ROLLOUT_POLICY_WIDTHS:
                raise UnsupportedRolloutShape(f"no in-kernel policy of width {width} with {n_act} actions")
        shape = self._pool_rollout(width, n_act)
        if isinstance(shape, str):
            raise UnsupportedRolloutShape(shape)
        pool_name, n_pool, staged = shape
        if getattr(resetter, "_pool_rng", None) is None:
            raise UnsupportedRolloutShape("the pool generator is not initialised: call init_reset_pool() before "
                                          "building the rollout")
        pol_args = [NULL, np.int32(0)]
        if policy is not None:
            self._checked_policy(packed, width, n_act, UnsupportedRolloutShape)
            pol_args = [packed, np.int32(width)]
        name = self._entry(f"Rollout_P_H{width}" if width else "Rollout_P")
        fm.initialize_functions([name])
        _, reset_args, _, _ = resetter.fused_launch(dm, 0, 0)  # builds / refreshes the descriptor table
        _, args, block, grid, _ = self.step_launch()
        args = list(args) + [sampler.rng_state, probabilities[0], np.int32(n_act), reset_args[0], reset_args[1],
                             tick_tag(), np.int32(self.ticks_per_launch)] + self._batch_arguments(batch) + \
            pol_args + [np.int32(self.invariant_divide_ok()), resetter._pool_rng, dm.device_data(pool_name),
                        np.int32(n_pool), np.int32(1 if staged else 0)]
        return fm.get_function(name), args, block, grid, self.pool_rollout_lds_bytes(width, n_act, n_pool, staged)

    def invariant_divide_ok(self):
        """1 when the device found the tick kernels' three-instruction division by this env's total mass
        (csrc/kernels/cartpole_common.h::cp_div_invariant) equal to the correctly rounded division for every float32
        dividend of two binades, [1, 2) and [2^40, 2^41), both signs -- one launch of HipCartPoleVerifyInvariantDivide per
        total mass (the verdicts are kept by the mass's float32 bits: `physics` may be replaced); 0: the kernels divide.
        That is a proof for the other binades only where the quotient stays a normal float32, which the flag does not
        say: the kernels take the fast ticks with this flag AND masses that keep it so for every dividend they hand to
        the shortcut (cp_fast_masses_ok).  (1 for the classic 1.1 and for every other mass tried so far.)"""
        if getattr(self, "_inv_div_ok", None) is not None:   # a verdict set from outside: no launch, whatever the mass
            return self._inv_div_ok
        total_mass = np.float32(self.physics.masspole + self.physics.masscart)
        verdicts = self.__dict__.setdefault("_inv_div_verdicts", {})
        key = total_mass.tobytes()
        if key not in verdicts:
            import torch

            fm = self.cuda_function_manager
            fm.initialize_functions(["HipCartPoleVerifyInvariantDivide"])
            ok = torch.ones(1, dtype=torch.int32, device=torch.device("cuda", int(fm._device_id)))
            with np.errstate(all="ignore"):   # (a reciprocal may be subnormal or overflow: the kernel is told what the host formed)
                recip = np.float32(1.0) / total_mass
            fm.get_function("HipCartPoleVerifyInvariantDivide")(total_mass, recip, ok,
                                                                block=(256, 1, 1), grid=(4096, 1), shared=0)
            verdicts[key] = int(ok.item())
        return verdicts[key]
