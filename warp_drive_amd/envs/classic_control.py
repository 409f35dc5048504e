"""ClassicControl Acrobot, MountainCar, ContinuousMountainCar and Pendulum, single agent per replica.

Host-side mirror of reference example_envs/single_agent/classic_control/{acrobot,mountain_car,continuous_mountain_car,
pendulum}/*.py.  The reference's CPU steps delegate to third-party gym (absent here): the constants, spaces and reset
distributions of gym's classic-control envs are stated below as this repository's own configuration, and the CPU step of
each env is a vectorised numpy restatement of the reference's device kernel (*_step_numba.py) with the same dtype flow
as csrc/kernels/classic_control.hip (its header lists every float32 / float64 decision).  The numpy steps are also the
test oracle: tests/golden/cc_<env>_traj.npz pin them to the reference's kernel sources (scripts/
gen_classic_control_golden.py).

The device classes launch `HipClassicControl<X>EnvStep` and the fused tick `HipClassicControl<X>EnvTick` (sampling +
step + restart of a finished replica, from the reset table or from a reset pool, `ticks_per_launch` ticks per launch).
The two discrete envs also have `HipClassicControl<X>EnvRollout_H32 / _H64`: the same tick with a small policy network
evaluated by the kernel on every tick's observation (`tick_launch(policy=...)`), and
`HipClassicControl<X>EnvEvaluate_H32 / _H64`: one episode of every replica in one launch, greedy or sampled
(`evaluate_launch`).  The two Box envs have `HipClassicControl<X>EnvRollout_A32 / _A64`: the tick with a deterministic
actor network evaluated by the kernel on every tick's observation (`tick_launch(actor=...)`, DDPG), and
`HipClassicControl<X>EnvEvaluate_A32 / _A64`: one episode of every replica in one launch with that actor, noise-free or
under the tick's exploration draw (`evaluate_actor_launch`).
"""
import math

import numpy as np

from warp_drive_amd.utils import spaces
from warp_drive_amd.utils.constants import Constants
from warp_drive_amd.utils.data_feed import DataFeed
from warp_drive_amd.utils.gpu_environment_context import CUDAEnvironmentContext
from warp_drive_amd.utils.launch_checks import (NULL, SingleAgentDeviceEnv, UnsupportedRolloutShape, batch_arguments,
                                                check_packed, check_record, evaluation_outputs, on_device, rp_actor_floats,
                                                tick_tag, unpack_actor, unpack_ou, unpack_policy)

_OBSERVATIONS = Constants.OBSERVATIONS
_ACTIONS = Constants.ACTIONS
_REWARDS = Constants.REWARDS

f32, f64 = np.float32, np.float64


# ----------------------------------------------------------------------------------------------------- configuration
class AcrobotPhysics:
    """gym's AcrobotEnv (classic_control/acrobot.py, gym >= 0.26); the kernel's link constants are its own
    (acrobot_step_numba.py:7-19)."""
    max_vel_1 = 4 * math.pi
    max_vel_2 = 9 * math.pi
    reset_low, reset_high = -0.1, 0.1  # every state component ~ U(low, high)


class MountainCarPhysics:
    """gym's MountainCarEnv"""
    min_position = -1.2
    max_position = 0.6
    max_speed = 0.07
    goal_position = 0.5
    goal_velocity = 0.0
    force = 0.001
    gravity = 0.0025
    reset_low, reset_high = -0.6, -0.4  # position ~ U(low, high), velocity 0


class ContinuousMountainCarPhysics:
    """gym's Continuous_MountainCarEnv"""
    min_action = -1.0
    max_action = 1.0
    min_position = -1.2
    max_position = 0.6
    max_speed = 0.07
    goal_position = 0.45
    goal_velocity = 0.0
    power = 0.0015
    reset_low, reset_high = -0.6, -0.4


class PendulumPhysics:
    """gym's PendulumEnv; the kernel's own constants (pendulum_step_numba.py:6-14: g = 9.81)"""
    max_speed = 8.0
    max_torque = 2.0
    reset_high = (math.pi, 1.0)  # (theta, theta_dot) ~ U(-high, high)


# ------------------------------------------------------------------------------------------------- numpy steps
# Each takes float32 state [E, S] and actions [E] and returns (state [E, S] float32, obs [E, O] float32,
# reward [E] float32, terminal code [E] int32: 0, or the done value a terminal state sets).

def _clip(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def _cos32(x):  # numpy's float32 kernels (contiguous input: a strided one may take another loop)
    return np.cos(np.ascontiguousarray(x, dtype=f32))


def _sin32(x):
    return np.sin(np.ascontiguousarray(x, dtype=f32))


def _acrobot_dsdt(st, a):
    m1 = m2 = l1 = 1.0
    lc1 = lc2 = 0.5
    I1 = I2 = 1.0
    g = 9.8
    theta1, theta2, dtheta1, dtheta2 = (st[:, i] for i in range(4))
    c2, s2 = _cos32(theta2).astype(f64), _sin32(theta2).astype(f64)  # float32 kernels, widened
    d1 = m1 * (lc1 * lc1) + m2 * ((l1 * l1) + (lc2 * lc2) + 2.0 * l1 * lc2 * c2) + I1 + I2
    d2 = m2 * ((lc2 * lc2) + l1 * lc2 * c2) + I2
    phi2 = m2 * lc2 * g * np.cos((theta1 + theta2).astype(f64) - math.pi / 2.0)
    phi1 = (-m2 * l1 * lc2 * (dtheta2 * dtheta2).astype(f64) * s2
            - 2.0 * m2 * l1 * lc2 * dtheta2.astype(f64) * dtheta1.astype(f64) * s2
            + (m1 * lc1 + m2 * l1) * g * np.cos(theta1.astype(f64) - math.pi / 2.0) + phi2)
    ddtheta2 = ((a + d2 / d1 * phi1 - m2 * l1 * lc2 * (dtheta1 * dtheta1).astype(f64) * s2 - phi2)
                / (m2 * (lc2 * lc2) + I2 - d2 * d2 / d1))
    ddtheta1 = -(d2 * ddtheta2 + phi1) / d1
    return np.stack([dtheta1, dtheta2, ddtheta1.astype(f32), ddtheta2.astype(f32)], axis=1)


def _wrap(x, m, M):
    x = x.astype(f64)
    diff = M - m
    while (x > M).any():
        x = np.where(x > M, x - diff, x)
    while (x < m).any():
        x = np.where(x < m, x + diff, x)
    return x.astype(f32)


def acrobot_step(state, action, p=AcrobotPhysics):
    s = np.asarray(state, f32)
    a = np.array([-1.0, 0.0, 1.0], dtype=f64)[np.asarray(action, np.int64).reshape(-1)]
    dt, dt2 = 0.2, 0.1
    k1 = _acrobot_dsdt(s, a)
    k2 = _acrobot_dsdt((s.astype(f64) + k1.astype(f64) * dt2).astype(f32), a)
    k3 = _acrobot_dsdt((s.astype(f64) + k2.astype(f64) * dt2).astype(f32), a)
    k4 = _acrobot_dsdt((s.astype(f64) + k3.astype(f64) * dt).astype(f32), a)
    ns = (s.astype(f64) + dt / 6.0 * (k1.astype(f64) + 2.0 * k2.astype(f64) + 2.0 * k3.astype(f64)
                                      + k4.astype(f64))).astype(f32)
    out = np.empty_like(s)
    out[:, 0] = _wrap(ns[:, 0], -math.pi, math.pi)
    out[:, 1] = _wrap(ns[:, 1], -math.pi, math.pi)
    out[:, 2] = _clip(ns[:, 2].astype(f64), -p.max_vel_1, p.max_vel_1).astype(f32)
    out[:, 3] = _clip(ns[:, 3].astype(f64), -p.max_vel_2, p.max_vel_2).astype(f32)
    terminated = (-_cos32(out[:, 0]) - _cos32(out[:, 1] + out[:, 0])) > f32(1.0)
    obs = acrobot_obs(out)
    reward = np.where(terminated, f32(0.0), f32(-1.0)).astype(f32)
    return out, obs, reward, terminated.astype(np.int32)


def acrobot_obs(state):
    s = np.asarray(state, f32).reshape(-1, 4)
    return np.stack([_cos32(s[:, 0]), _sin32(s[:, 0]), _cos32(s[:, 1]), _sin32(s[:, 1]), s[:, 2], s[:, 3]],
                    axis=1).astype(f32)


def _car_tail(position, velocity, p):
    """clip, move, the left wall, the goal test (float64 throughout)"""
    velocity = _clip(velocity, f64(f32(-p.max_speed)), f64(f32(p.max_speed)))
    position = _clip(position + velocity, f64(f32(p.min_position)), f64(f32(p.max_position)))
    velocity = np.where((position == f64(f32(p.min_position))) & (velocity < 0.0), 0.0, velocity)
    terminated = (position >= f64(f32(p.goal_position))) & (velocity >= f64(f32(p.goal_velocity)))
    out = np.stack([position, velocity], axis=1).astype(f32)
    return out, terminated


def mountain_car_step(state, action, p=MountainCarPhysics):
    s = np.asarray(state, f32)
    a = np.asarray(action, np.int64).reshape(-1)
    position, velocity = s[:, 0].astype(f64), s[:, 1].astype(f64)
    velocity = velocity + ((a - 1).astype(f64) * f64(f32(p.force)) + np.cos(3.0 * position) * f64(-f32(p.gravity)))
    out, terminated = _car_tail(position, velocity, p)
    reward = np.full(len(s), -1.0, dtype=f32)
    return out, out.copy(), reward, np.where(terminated, 2, 0).astype(np.int32)


def continuous_mountain_car_step(state, action, p=ContinuousMountainCarPhysics):
    s = np.asarray(state, f32)
    a = np.asarray(action, f32).reshape(-1)
    force = _clip(a, f32(p.min_action), f32(p.max_action)).astype(f32)
    position, velocity = s[:, 0].astype(f64), s[:, 1].astype(f64)
    velocity = velocity + ((force * f32(p.power)).astype(f64) - 0.0025 * np.cos(3.0 * position))
    out, terminated = _car_tail(position, velocity, p)
    reward = (np.where(terminated, 100.0, 0.0) - (a * a).astype(f64) * 0.1).astype(f32)
    return out, out.copy(), reward, terminated.astype(np.int32)


def pendulum_step(state, action, p=PendulumPhysics):
    s = np.asarray(state, f32)
    u = _clip(np.asarray(action, f32).reshape(-1).astype(f64), -p.max_torque, p.max_torque)
    th, thdot = s[:, 0], s[:, 1]
    dt, g, m, l = 0.05, 9.81, 1.0, 1.0
    an = np.remainder(th.astype(f64) + math.pi, 2.0 * math.pi) - math.pi
    costs = an * an + 0.1 * (thdot * thdot).astype(f64) + 0.001 * (u * u)
    newthdot = thdot.astype(f64) + (3.0 * g / (2.0 * l) * _sin32(th).astype(f64) + 3.0 / (m * (l * l)) * u) * dt
    newthdot = _clip(newthdot, -p.max_speed, p.max_speed)
    newth = th.astype(f64) + newthdot * dt
    out = np.stack([newth, newthdot], axis=1).astype(f32)
    obs = np.stack([np.cos(newth), np.sin(newth), newthdot], axis=1).astype(f32)
    return out, obs, (-costs).astype(f32), np.zeros(len(s), np.int32)


def pendulum_obs(state):
    s = np.asarray(state, f32).reshape(-1, 2)
    th = s[:, 0].astype(f64)
    return np.stack([np.cos(th), np.sin(th), s[:, 1].astype(f64)], axis=1).astype(f32)


def apply_done(done_code, timestep, episode_length):
    """the done flag the step kernels set: 1 on time-out, else the terminal code (MountainCar: 2 on the goal)"""
    return np.where(np.asarray(timestep) == episode_length, 1, done_code).astype(np.int32)


# ------------------------------------------------------------------------------------------------------- CPU envs
class _ClassicControlEnv:
    """the reference's SingleAgentEnv contract: constructor (episode_length, env_backend, reset_pool_size, seed), reset()
    -> {0: obs}, step({0: action}) -> ({0: obs}, {0: reward}, {"__all__": done}, {})"""
    physics = None
    STATE_DIM = 2

    def __init__(self, episode_length=500, env_backend="cpu", reset_pool_size=0, seed=None):
        self.num_agents = 1
        self.agents = {0: True}
        assert episode_length > 0
        self.episode_length = episode_length
        self.env_backend = env_backend
        self.reset_pool_size = reset_pool_size
        self.seed = seed
        self.timestep = None
        self._rng = np.random.default_rng(seed)
        self.state = None
        # a reset without a pool restarts from the seeded fixed start: it draws nothing
        self.RESET_IS_DETERMINISTIC = reset_pool_size < 2

    # hooks of each env
    def _sample_state(self, rng):
        raise NotImplementedError

    def _obs(self, state):
        return np.asarray(state, f32).copy()

    def _step_state(self, state, action):
        raise NotImplementedError

    def _draw_initial_state(self, fixed):
        rng = np.random.default_rng(self.seed) if fixed else self._rng
        return np.asarray(self._sample_state(rng), dtype=f32)

    def reset(self):
        self.timestep = 0
        self.state = self._draw_initial_state(fixed=self.reset_pool_size < 2)
        return {0: self._obs(self.state).reshape(-1)}

    def step(self, action=None):
        self.timestep += 1
        assert isinstance(action, dict) and len(action) == 1
        a = np.asarray(action[0]).reshape(1)
        state, obs, reward, term = self._step_state(self.state[None], a)
        self.state = state[0]
        done = {"__all__": self.timestep >= self.episode_length or bool(term[0])}
        return {0: obs[0]}, {0: float(reward[0])}, done, {}


class ClassicControlAcrobotEnv(_ClassicControlEnv):
    name = "ClassicControlAcrobotEnv"
    physics = AcrobotPhysics
    STATE_DIM = 4

    def __init__(self, episode_length=500, env_backend="cpu", reset_pool_size=0, seed=None):
        super().__init__(episode_length, env_backend, reset_pool_size, seed)
        high = np.array([1.0, 1.0, 1.0, 1.0, self.physics.max_vel_1, self.physics.max_vel_2], dtype=f32)
        self.action_space = {0: spaces.Discrete(3)}
        self.observation_space = {0: spaces.Box(-high, high, dtype=f32)}

    def _sample_state(self, rng):
        return rng.uniform(low=self.physics.reset_low, high=self.physics.reset_high, size=(4,))

    def _obs(self, state):
        return acrobot_obs(state)[0]

    def _step_state(self, state, action):
        return acrobot_step(state, action, self.physics)


class ClassicControlMountainCarEnv(_ClassicControlEnv):
    name = "ClassicControlMountainCarEnv"
    physics = MountainCarPhysics

    def __init__(self, episode_length=500, env_backend="cpu", reset_pool_size=0, seed=None):
        super().__init__(episode_length, env_backend, reset_pool_size, seed)
        p = self.physics
        self.action_space = {0: spaces.Discrete(3)}
        self.observation_space = {0: spaces.Box(np.array([p.min_position, -p.max_speed], dtype=f32),
                                                np.array([p.max_position, p.max_speed], dtype=f32), dtype=f32)}

    def _sample_state(self, rng):
        return np.array([rng.uniform(low=self.physics.reset_low, high=self.physics.reset_high), 0.0])

    def _step_state(self, state, action):
        return mountain_car_step(state, action, self.physics)


class ClassicControlContinuousMountainCarEnv(_ClassicControlEnv):
    name = "ClassicControlContinuousMountainCarEnv"
    physics = ContinuousMountainCarPhysics

    def __init__(self, episode_length=500, env_backend="cpu", reset_pool_size=0, seed=None):
        super().__init__(episode_length, env_backend, reset_pool_size, seed)
        p = self.physics
        self.action_space = {0: spaces.Box(p.min_action, p.max_action, shape=(1,), dtype=f32)}
        self.observation_space = {0: spaces.Box(np.array([p.min_position, -p.max_speed], dtype=f32),
                                                np.array([p.max_position, p.max_speed], dtype=f32), dtype=f32)}

    def _sample_state(self, rng):
        return np.array([rng.uniform(low=self.physics.reset_low, high=self.physics.reset_high), 0.0])

    def _step_state(self, state, action):
        return continuous_mountain_car_step(state, action, self.physics)


class ClassicControlPendulumEnv(_ClassicControlEnv):
    name = "ClassicControlPendulumEnv"
    physics = PendulumPhysics

    def __init__(self, episode_length=200, env_backend="cpu", reset_pool_size=0, seed=None):
        super().__init__(episode_length, env_backend, reset_pool_size, seed)
        p = self.physics
        high = np.array([1.0, 1.0, p.max_speed], dtype=f32)
        self.action_space = {0: spaces.Box(-p.max_torque, p.max_torque, shape=(1,), dtype=f32)}
        self.observation_space = {0: spaces.Box(-high, high, dtype=f32)}

    def _sample_state(self, rng):
        high = np.array(self.physics.reset_high)
        return rng.uniform(low=-high, high=high)

    def _obs(self, state):
        return pendulum_obs(state)[0]

    def _step_state(self, state, action):
        return pendulum_step(state, action, self.physics)


# ---------------------------------------------------------------------------------------------------- device envs
def rollout_actor_floats(obs_size, width):
    """floats of the packed actor the ...Rollout_A<width> entries read: rp_actor_floats(width, obs_size)"""
    return rp_actor_floats(width, obs_size)


class _CUDAClassicControlEnv(SingleAgentDeviceEnv, CUDAEnvironmentContext):
    """shared device side: data and the fused tick launch; step, reset pool, `has_live_policy_evaluate` and
    `evaluate_launch` (HipClassicControl<X>EnvEvaluate_H<width>) are utils/launch_checks.py::SingleAgentDeviceEnv's"""
    TICK_POOL_RESET = True  # the tick kernel restarts a finished replica from the reset pool itself
    CONSTANTS = ()          # names of the physics constants the kernels take, in argument order
    # the trainer runs a whole batch in one launch on these envs only when asked to
    # (`trainer.fused_rollout_policy: "all"`); the discrete subclasses list the widths (ROLLOUT_POLICY_WIDTHS)
    ROLLOUT_POLICY_OPT_IN = True

    def __init__(self, *args, **kwargs):
        CUDAEnvironmentContext.__init__(self)

    def _has_entry(self, suffix, width, box):
        """is `width` among the widths the class lists for its (Box: actor, else: policy) entries, and the entry
        ...<suffix><width> in the manifest?"""
        widths = getattr(self, "ROLLOUT_ACTOR_WIDTHS" if box else "ROLLOUT_POLICY_WIDTHS", ())
        if isinstance(self.action_space[0], spaces.Box) != box or int(width) not in widths:
            return False
        return bool(self.cuda_function_manager.has_function(self._entry(f"{suffix}{int(width)}")))

    def has_live_policy_rollout(self, width, n_actions):
        """does a rollout kernel exist that evaluates the policy network itself (...Rollout_H<width>)?  (RolloutEngine asks
        before it calls `tick_launch(policy=...)`)  The Box envs have none."""
        return 1 <= int(n_actions) <= 8 and self._has_entry("Rollout_H", width, box=False)

    def has_live_actor_rollout(self, width):
        """does a rollout kernel exist that evaluates a deterministic actor itself (...Rollout_A<width>)?  (RolloutEngine
        asks before it calls `tick_launch(actor=...)`)  Only the Box envs have one."""
        return self._has_entry("Rollout_A", width, box=True)

    def has_live_actor_evaluate(self, width):
        """does an evaluation kernel exist that runs one episode of every replica with the deterministic actor inside it
        (...Evaluate_A<width>, TrainerDDPG.evaluate_episodes)?  The widths of the Rollout_A entries; only the Box envs
        have one."""
        return self._has_entry("Evaluate_A", width, box=True)

    def _checked_actor(self, packed, width):
        """floats of the packed actor of this env, `packed` checked against them"""
        O = self._obs_size()
        n_w = rp_actor_floats(width, O)
        check_packed(packed, n_w, UnsupportedRolloutShape, "the packed actor", f"observation {O}, width {width}")
        return n_w

    def evaluate_actor_launch(self, sampler, actor, ou, outputs, mean_trace=None, action_trace=None, ticks=None):
        """One episode of every replica of a Box env in ONE launch (HipClassicControl<X>EnvEvaluate_A<width>): from the
        state, observation and timestep the arrays hold, at most `ticks` (default: episode_length) ticks of actor ->
        mean -> action -> step, up to the first done.  actor = (packed float32 CUDA tensor, hidden width, action_scale,
        action_bias) as in `tick_launch(actor=...)`; ou = (damping, stddev, scale): with scale >= 1e-8 the action is the
        fused tick's OU / Gaussian draw around the mean, else the mean itself (greedy).  outputs = {"reward_sum":
        float32, "steps": int32, "done": int32}, CUDA tensors of at least n_envs elements; `mean_trace` / `action_trace`
        (optional) float32 [>= ticks, n_envs]: row k = tick k's means / actions.  The launch writes those, and when it
        draws the OU state and the sampler's epoch words; the env's arrays are read only.
        Returns (function, arguments, block, grid, shared bytes)."""
        fm, dm = self.cuda_function_manager, self.cuda_data_manager
        packed, width, action_scale, action_bias = unpack_actor(actor)
        if not self.has_live_actor_evaluate(width):
            raise UnsupportedRolloutShape(f"{type(self).__name__} has no in-kernel evaluation of an actor of width {width}")
        damping, stddev, scale = unpack_ou(ou)
        E = self._n_envs()
        n_w = self._checked_actor(packed, width)
        T = int(self.episode_length if ticks is None else ticks)
        out_args = evaluation_outputs(outputs, E, UnsupportedRolloutShape)
        for key, t in (("mean_trace", mean_trace), ("action_trace", action_trace)):
            if t is not None:
                check_record(t, key, "float32", T, E, UnsupportedRolloutShape, min_dims=2)
        name = self._entry(f"Evaluate_A{width}")
        fm.initialize_functions([name])
        _, args, block, grid, _ = self.step_launch()
        args = list(args) + [sampler.rng_state, tick_tag(), np.int32(T), packed, np.int32(width),
                             np.float32(action_scale), np.float32(action_bias), dm.device_data(f"{_ACTIONS}_ou_state"),
                             np.float32(damping), np.float32(stddev), np.float32(scale)] + out_args + \
            [NULL if mean_trace is None else mean_trace, NULL if action_trace is None else action_trace]
        return fm.get_function(name), args, block, grid, 4 * n_w

    def get_data_dictionary(self):
        feed = DataFeed()
        feed.add_data(name="state", data=np.atleast_2d(self._draw_initial_state(fixed=True)),
                      save_copy_and_apply_at_reset=self.reset_pool_size < 2)
        if self.CONSTANTS:
            feed.add_data_list([(name, float(getattr(self.physics, name))) for name in self.CONSTANTS])
        return feed

    def _step_args(self):
        return (["state", _ACTIONS, "_done_", _REWARDS, _OBSERVATIONS] + list(self.CONSTANTS)
                + ["_timestep_", ("episode_length", "meta"), ("n_envs", "meta")])

    def tick_launch(self, sampler, probabilities, resetter, env_range=None, batch=None, policy=None,
                    ou_params=(0.15, 0.2, 1.0), actor=None, mean_batch=None):
        """Fused rollout tick(s): sample + step + restart of a finished replica, `ticks_per_launch` times in ONE launch
        (HipClassicControl<X>EnvTick).  probabilities = [float32 CUDA tensor [E, 1, n_actions]] (discrete) or [the
        means, [E, 1, 1]] (Box: OU / Gaussian exploration with ou_params = (damping, stddev, scale), the draws of
        sample_ou_process).  With a reset pool the kernel draws the restart row itself (the resetter's pool RNG:
        init_reset_pool() first).  `batch` (optional) = {"obs": [T, E, 1, O] float32, "actions": [T, E, 1, 1],
        "rewards": [T, E, 1] float32, "done": [T, E] int32} with T >= ticks_per_launch: tick k writes row k.
        `policy` (optional, Acrobot and MountainCar) = (packed float32 CUDA tensor from
        training.policy_kernel.pack_rollout_policy, hidden width): the launch evaluates the policy network on every
        tick's observation itself (HipClassicControl<X>EnvRollout_H<width>, the packed weights in dynamic LDS) instead of
        reading `probabilities`, which then only says how many actions there are.
        `actor` (optional, ContinuousMountainCar and Pendulum) = (packed float32 CUDA tensor from
        training.policy_kernel.pack_rollout_actor, hidden width, action_scale, action_bias): the launch evaluates the
        deterministic actor on every tick's observation itself (HipClassicControl<X>EnvRollout_A<width>), mean =
        action_scale * tanh(z) + action_bias, instead of reading the means; `mean_batch` (optional, float32 [T, E]): tick
        k writes its means to row k."""
        assert env_range is None and len(probabilities) == 1
        fm, dm = self.cuda_function_manager, self.cuda_data_manager
        who = type(self).__name__
        name = self._entry("Tick")
        shared, pol_args = 0, []
        if policy is not None:
            packed, width, n_act = unpack_policy(policy, lambda: probabilities[0].shape[-1])
            if not self.has_live_policy_rollout(width, n_act):
                raise UnsupportedRolloutShape(f"{who} has no in-kernel policy of width {width} with {n_act} actions")
            shared = 4 * self._checked_policy(packed, width, n_act, UnsupportedRolloutShape)
            name, pol_args = self._entry(f"Rollout_H{width}"), [packed, np.int32(width)]
        if actor is not None:
            if policy is not None:
                raise UnsupportedRolloutShape("a launch evaluates a policy or an actor, not both")
            packed, width, action_scale, action_bias = unpack_actor(actor)
            if not self.has_live_actor_rollout(width):
                raise UnsupportedRolloutShape(f"{who} has no in-kernel actor of width {width}")
            shared = 4 * self._checked_actor(packed, width)
            if mean_batch is not None:
                check_record(mean_batch, "mean_batch", "float32", int(self.ticks_per_launch), self._n_envs(),
                             UnsupportedRolloutShape)
            name = self._entry(f"Rollout_A{width}")
            pol_args = [packed, np.int32(width), np.float32(action_scale), np.float32(action_bias),
                        NULL if mean_batch is None else mean_batch]
        elif mean_batch is not None:
            raise UnsupportedRolloutShape("mean_batch is what the in-kernel actor records: it needs `actor`")
        fm.initialize_functions([name])
        _, reset_args, _, _ = resetter.fused_launch(dm, 0, 0)  # builds / refreshes the descriptor table
        _, args, block, grid, _ = self.step_launch()
        probs = probabilities[0]
        continuous = isinstance(self.action_space[0], spaces.Box)
        E, T = self._n_envs(), int(self.ticks_per_launch)
        assert on_device(probs) and probs.shape[0] == E
        if continuous:
            assert tuple(probs.shape) == (E, 1, 1)
        else:
            assert 1 <= int(probs.shape[-1]) <= 8
        batch_args = batch_arguments(batch, T, E, 1, self._obs_size(), actions="float32" if continuous else "int32")
        pools = dict(dm.reset_target_to_pool)
        if pools:
            assert set(pools) == {"state"}, f"the tick kernel restarts `state` from a pool, not {sorted(pools)}"
            if getattr(resetter, "_pool_rng", None) is None:
                raise RuntimeError("the env has a reset pool: call init_reset_pool() before building the rollout")
            pool_args = [resetter._pool_rng, dm.device_data(pools["state"]),
                         np.int32(dm.get_shape(pools["state"])[0])]
        else:
            pool_args = [NULL, NULL, np.int32(0)]
        if continuous:
            damping, stddev, scale = ou_params
            ou_args = [dm.device_data(f"{_ACTIONS}_ou_state"), np.float32(damping), np.float32(stddev),
                       np.float32(scale)]
        else:
            ou_args = [NULL, np.float32(0), np.float32(0), np.float32(0)]
        args = list(args) + [sampler.rng_state, probs, np.int32(probs.shape[-1]), reset_args[0], reset_args[1],
                             tick_tag(), np.int32(T)] + batch_args + pool_args + ou_args + pol_args
        return fm.get_function(name), args, block, grid, shared


class CUDAClassicControlAcrobotEnv(_CUDAClassicControlEnv, ClassicControlAcrobotEnv):
    ROLLOUT_POLICY_WIDTHS = (32, 64)   # HipClassicControlAcrobotEnvRollout_H<width>

    def __init__(self, *args, **kwargs):
        ClassicControlAcrobotEnv.__init__(self, *args, **kwargs)
        _CUDAClassicControlEnv.__init__(self)


class CUDAClassicControlMountainCarEnv(_CUDAClassicControlEnv, ClassicControlMountainCarEnv):
    ROLLOUT_POLICY_WIDTHS = (32, 64)   # HipClassicControlMountainCarEnvRollout_H<width>

    CONSTANTS = ("min_position", "max_position", "max_speed", "goal_position", "goal_velocity", "force", "gravity")

    def __init__(self, *args, **kwargs):
        ClassicControlMountainCarEnv.__init__(self, *args, **kwargs)
        _CUDAClassicControlEnv.__init__(self)


class CUDAClassicControlContinuousMountainCarEnv(_CUDAClassicControlEnv, ClassicControlContinuousMountainCarEnv):
    ROLLOUT_ACTOR_WIDTHS = (32, 64)    # HipClassicControlContinuousMountainCarEnvRollout_A<width>

    CONSTANTS = ("min_action", "max_action", "min_position", "max_position", "max_speed", "goal_position",
                 "goal_velocity", "power")

    def __init__(self, *args, **kwargs):
        ClassicControlContinuousMountainCarEnv.__init__(self, *args, **kwargs)
        _CUDAClassicControlEnv.__init__(self)


class CUDAClassicControlPendulumEnv(_CUDAClassicControlEnv, ClassicControlPendulumEnv):
    ROLLOUT_ACTOR_WIDTHS = (32, 64)    # HipClassicControlPendulumEnvRollout_A<width>

    def __init__(self, *args, **kwargs):
        ClassicControlPendulumEnv.__init__(self, *args, **kwargs)
        _CUDAClassicControlEnv.__init__(self)
