"""ContractProbe: a test-only custom environment for the contract clauses of include/wd_env.h, wd_env_tick.h and
wd_env_rollout.h that no worked example reaches (tests/test_gpu_custom_env_contract.py).  The step reads `_done_` in
every thread and adds it into `seen_done`; observations are signed, up to 8 in magnitude, with exact 0.0 and -0.0;
reward = action + 1; done at the time limit only; `per_env` (one word per replica), `odd` (three floats per replica) and
`wide` (seven words per agent) change on every tick and are restored by a restart.  The host step is plain numpy and
exact: every float is a small integer, a half or a quarter."""
import os

import numpy as np

from warp_drive_amd.utils import spaces
from warp_drive_amd.utils.constants import Constants
from warp_drive_amd.utils.custom_tick import FusedRolloutMixin, tick_block
from warp_drive_amd.utils.data_feed import DataFeed
from warp_drive_amd.utils.gpu_environment_context import CUDAEnvironmentContext

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "contract_probe.hip")

f32 = np.float32
SHAPES = ((1, 4), (1, 32), (4, 32), (7, 32), (7, 64))   # (F, H) of the Rollout and Logits entries in contract_probe.hip
WIDE, ODD = 7, 3
PER_ENV_AT_RESET = 1000
ODD_AT_RESET = np.array([-0.0, 2.5, -7.0], dtype=f32)
REWARD_AT_RESET = f32(-3.5)   # no step stores it: a reward is action + 1

_STEP_ARGS = [Constants.OBSERVATIONS, Constants.ACTIONS, Constants.REWARDS, "_done_", "_timestep_", "seen_done", "per_env",
              "odd", "wide", ("episode_length", "meta"), ("n_agents", "meta"), "n_features"]


def wide_at_reset(num_agents):
    return (100000 + np.arange(num_agents * WIDE, dtype=np.int32)).reshape(num_agents, WIDE)


def probe_observation(timestep, num_agents, features):
    """[N, F] float32: ((t * (agent + 1) + 3 * j) % 17 - 8), negated for an odd agent (so a 0 becomes -0.0), halved where
    j % 3 == 2"""
    agent, j = np.arange(num_agents)[:, None], np.arange(features)[None, :]
    v = (int(timestep) * (agent + 1) + 3 * j) % 17 - 8
    x = v.astype(f32) * np.where(agent & 1, f32(-1), f32(1)).astype(f32)
    return np.where(j % 3 == 2, x * f32(0.5), x).astype(f32)


class ContractProbe(FusedRolloutMixin, CUDAEnvironmentContext):
    name = "ContractProbe"
    RESET_IS_DETERMINISTIC = True
    TICK_KERNEL = "HipContractProbeTick"
    TICK_STEP_ARGS = _STEP_ARGS
    ROLLOUT_POLICY_WIDTHS = (4, 32, 64)
    ROLLOUT_MAX_THREADS = {4: 1024, 32: 1024, 64: 512}  # the entries' __launch_bounds__ in contract_probe.hip

    def __init__(self, num_agents=5, episode_length=4, n_actions=2, features=7, num_envs=1, env_backend="cpu"):
        super().__init__()
        self.num_agents, self.episode_length, self.n_actions = int(num_agents), int(episode_length), int(n_actions)
        self.features, self.num_envs = int(features), int(num_envs)
        assert self.features in {F for F, _ in SHAPES}
        self.ROLLOUT_KERNEL = f"HipContractProbeRollout_F{self.features}_H{{width}}"
        self.action_space = {a: spaces.Discrete(self.n_actions) for a in range(self.num_agents)}
        self.observation_space = None  # filled in by EnvWrapper
        self.env_backend = env_backend
        self.timestep = None
        self.per_env = self.odd = self.wide = None

    def logits_kernel(self, width):
        return f"HipContractProbeLogits_F{self.features}_H{int(width)}"

    def _observation(self):
        obs = probe_observation(self.timestep, self.num_agents, self.features)
        return {a: obs[a] for a in range(self.num_agents)}

    def reset(self):
        self.timestep = 0
        self.per_env = np.array([PER_ENV_AT_RESET], dtype=np.int32)
        self.odd = ODD_AT_RESET.copy()
        self.wide = wide_at_reset(self.num_agents)
        return self._observation()

    def step(self, actions=None):
        if self.env_backend != "cpu":
            self.cuda_step(*self.cuda_step_function_feed(_STEP_ARGS), block=tick_block(self.num_agents),
                           grid=self.cuda_function_manager.grid)
            return None
        self.timestep += 1
        t = self.timestep
        self.per_env = self.per_env + np.int32(3 * t + 1)
        self.odd = (self.odd + (np.arange(ODD) + t).astype(f32) * f32(0.25)).astype(f32)
        self.wide = self.wide + (np.arange(self.num_agents * WIDE, dtype=np.int32).reshape(self.num_agents, WIDE) + np.int32(t))
        rewards = {a: f32(int(np.asarray(actions[a]).reshape(-1)[0]) + 1) for a in range(self.num_agents)}
        return self._observation(), rewards, {"__all__": self.timestep == self.episode_length}, {}

    def get_data_dictionary(self):
        feed = DataFeed()
        feed.add_data(name="seen_done", data=np.zeros((self.num_envs, self.num_agents), dtype=np.int32))
        feed.add_data(name="per_env", data=np.array([PER_ENV_AT_RESET], dtype=np.int32), save_copy_and_apply_at_reset=True)
        feed.add_data(name="odd", data=ODD_AT_RESET.copy(), save_copy_and_apply_at_reset=True)
        feed.add_data(name="wide", data=wide_at_reset(self.num_agents), save_copy_and_apply_at_reset=True)
        feed.add_data_list([("n_features", self.features)])
        return feed

    def step_launch(self):
        return (self.cuda_step, list(self.cuda_step_function_feed(_STEP_ARGS)), tick_block(self.num_agents),
                self.cuda_function_manager.grid, 0)
