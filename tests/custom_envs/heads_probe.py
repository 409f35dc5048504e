"""HeadsProbe: a test-only custom environment for the fused tick of include/wd_env_tick.h with SEVERAL action heads.
`counts[env, agent, h] += action_h + 1` on every tick, so the counts show which action each head's draw handed to the
step; the replica is done at the time limit only, and a restart puts the counts back to zero.  One head is a
`Discrete` space, several a `MultiDiscrete` one."""
import os

import numpy as np

from warp_drive_amd.utils import spaces
from warp_drive_amd.utils.constants import Constants
from warp_drive_amd.utils.custom_tick import FusedTickMixin, tick_block
from warp_drive_amd.utils.data_feed import DataFeed
from warp_drive_amd.utils.gpu_environment_context import CUDAEnvironmentContext

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "heads_probe.hip")

_STEP_ARGS = ["counts", Constants.ACTIONS, "_done_", "_timestep_", ("episode_length", "meta"), ("n_agents", "meta"),
              "n_heads"]


class HeadsProbe(FusedTickMixin, CUDAEnvironmentContext):
    name = "HeadsProbe"
    RESET_IS_DETERMINISTIC = True
    TICK_KERNEL = "HipHeadsProbeTick"
    TICK_STEP_ARGS = _STEP_ARGS

    def __init__(self, num_agents=5, episode_length=4, head_sizes=(3,), env_backend="cpu"):
        super().__init__()
        self.num_agents, self.episode_length = int(num_agents), int(episode_length)
        self.head_sizes = tuple(int(v) for v in head_sizes)
        space = spaces.Discrete(self.head_sizes[0]) if len(self.head_sizes) == 1 else spaces.MultiDiscrete(self.head_sizes)
        self.action_space = {a: space for a in range(self.num_agents)}
        self.observation_space = None  # filled in by EnvWrapper
        self.env_backend = env_backend
        self.timestep = None
        self.counts = None

    def reset(self):
        self.timestep = 0
        self.counts = np.zeros((self.num_agents, len(self.head_sizes)), dtype=np.int32)
        return {a: np.zeros(1, dtype=np.float32) for a in range(self.num_agents)}

    def step(self, actions=None):
        if self.env_backend != "cpu":
            self.cuda_step(*self.cuda_step_function_feed(_STEP_ARGS), block=tick_block(self.num_agents),
                           grid=self.cuda_function_manager.grid)
            return None
        self.timestep += 1
        self.counts += np.asarray(actions, dtype=np.int32).reshape(self.counts.shape) + 1
        return self.timestep == self.episode_length

    def get_data_dictionary(self):
        feed = DataFeed()
        feed.add_data(name="counts", data=np.zeros((self.num_agents, len(self.head_sizes)), dtype=np.int32),
                      save_copy_and_apply_at_reset=True)
        feed.add_data_list([("n_heads", len(self.head_sizes))])
        return feed

    def step_launch(self):
        return (self.cuda_step, list(self.cuda_step_function_feed(_STEP_ARGS)), tick_block(self.num_agents),
                self.cuda_function_manager.grid, 0)
