"""PolicyProbe: a test-only custom environment for the one-launch rollout of include/wd_env_rollout.h with an EVEN
observation size (F = 2) and an action count chosen at run time.  Observation: (counter / L, agent parity); reward:
action + 1, so the recorded rewards show which action the in-kernel policy handed to the step; the replica is done at
the time limit only and a restart puts the observation back to (0, parity)."""
import os

import numpy as np

from warp_drive_amd.utils import spaces
from warp_drive_amd.utils.constants import Constants
from warp_drive_amd.utils.custom_tick import FusedRolloutMixin, tick_block
from warp_drive_amd.utils.gpu_environment_context import CUDAEnvironmentContext

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "policy_probe.hip")

_STEP_ARGS = [Constants.OBSERVATIONS, Constants.ACTIONS, Constants.REWARDS, "_done_", "_timestep_",
              ("episode_length", "meta"), ("n_agents", "meta")]


def probe_observation(timestep, episode_length, num_agents):
    """[N, 2] float32: one float32 division, the agent's parity"""
    t = np.float32(timestep) / np.float32(episode_length)
    return np.stack([np.full(num_agents, t, dtype=np.float32), (np.arange(num_agents) & 1).astype(np.float32)], axis=1)


class PolicyProbe(FusedRolloutMixin, CUDAEnvironmentContext):
    name = "PolicyProbe"
    RESET_IS_DETERMINISTIC = True
    TICK_KERNEL = "HipPolicyProbeTick"
    TICK_STEP_ARGS = _STEP_ARGS
    ROLLOUT_KERNEL = "HipPolicyProbeRollout_H{width}"
    ROLLOUT_MAX_THREADS = {32: 1024, 64: 512}  # the entries' __launch_bounds__ in policy_probe.hip

    def __init__(self, num_agents=5, episode_length=4, n_actions=2, env_backend="cpu"):
        super().__init__()
        self.num_agents, self.episode_length, self.n_actions = int(num_agents), int(episode_length), int(n_actions)
        self.action_space = {a: spaces.Discrete(self.n_actions) for a in range(self.num_agents)}
        self.observation_space = None  # filled in by EnvWrapper
        self.env_backend = env_backend
        self.timestep = None

    def _observation(self):
        obs = probe_observation(self.timestep, self.episode_length, self.num_agents)
        return {a: obs[a] for a in range(self.num_agents)}

    def reset(self):
        self.timestep = 0
        return self._observation()

    def step(self, actions=None):
        if self.env_backend != "cpu":
            self.cuda_step(*self.cuda_step_function_feed(_STEP_ARGS), block=tick_block(self.num_agents),
                           grid=self.cuda_function_manager.grid)
            return None
        self.timestep += 1
        rewards = {a: np.float32(int(np.asarray(actions[a]).reshape(-1)[0]) + 1) for a in range(self.num_agents)}
        return self._observation(), rewards, {"__all__": self.timestep == self.episode_length}, {}

    def get_data_dictionary(self):
        from warp_drive_amd.utils.data_feed import DataFeed

        return DataFeed()

    def step_launch(self):
        return (self.cuda_step, list(self.cuda_step_function_feed(_STEP_ARGS)), tick_block(self.num_agents),
                self.cuda_function_manager.grid, 0)
