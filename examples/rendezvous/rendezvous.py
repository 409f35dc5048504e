"""Rendezvous: a worked CUSTOM environment (docs/custom_environments.md).

N agents on the integer grid [0, L]^2 are rewarded for standing close to their common centroid; the episode ends at the
time limit or as soon as the largest spread falls to `spread_limit`.  The class is dual-mode: `env_backend="cpu"` steps
one replica in numpy, `env_backend="hip"` launches `HipRendezvousStep` of rendezvous_step.hip over all replicas.  That
source is NOT part of the package's build: it is registered with the class,

    registrar = EnvironmentRegistrar()
    registrar.add(env_backend=["cpu", "hip"], cuda_env_src_path=SOURCE)(Rendezvous)
    wrapper = EnvWrapper(env_name="Rendezvous", env_config={...}, num_envs=E, env_backend="hip", env_registrar=registrar)

and compiled by the function manager on first use.  State and spread are integers, and every float32 the step produces
is one division of integer-valued floats (one more subtraction for the wall penalty), so host and device agree bit for
bit.
"""
import os

import numpy as np

from warp_drive_amd.utils import spaces
from warp_drive_amd.utils.constants import Constants
from warp_drive_amd.utils.data_feed import DataFeed
from warp_drive_amd.utils.gpu_environment_context import CUDAEnvironmentContext

SOURCE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rendezvous_step.hip")

_OBSERVATIONS, _ACTIONS, _REWARDS = Constants.OBSERVATIONS, Constants.ACTIONS, Constants.REWARDS
_LOC_X, _LOC_Y = "loc_x", "loc_y"
_MOVES = "kRendezvousMoves"  # the __constant__ table of rendezvous_step.hip
# stay, +x, -x, +y, -y
DEFAULT_MOVES = ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1))
_F32 = np.float32

_STEP_ARGS = [_LOC_X, _LOC_Y, _ACTIONS, "_done_", _REWARDS, _OBSERVATIONS, "wall_penalty", "spread_limit", "grid_length",
              "_timestep_", ("episode_length", "meta"), ("n_agents", "meta")]


class Rendezvous(CUDAEnvironmentContext):
    name = "Rendezvous"
    RESET_IS_DETERMINISTIC = True  # reset() restarts from the cells drawn in the constructor

    def __init__(self, num_agents=5, grid_length=10, episode_length=20, seed=0, wall_penalty=0.1, spread_limit=-1,
                 moves=None, reset_cell=(0, 0), env_backend="cpu"):
        super().__init__()
        assert 1 <= int(num_agents) <= 1024 and int(grid_length) >= 1 and int(episode_length) >= 1
        assert int(num_agents) * int(grid_length) < 2 ** 24, "N * L must be exact in float32"
        self.num_agents = int(num_agents)
        self.grid_length = int(grid_length)
        self.episode_length = int(episode_length)
        self.wall_penalty = float(wall_penalty)
        self.spread_limit = int(spread_limit)  # done when the largest spread is <= this; -1: never
        self.reset_cell = (int(reset_cell[0]), int(reset_cell[1]))  # where HipRendezvousReset puts everybody
        self.moves = np.array(DEFAULT_MOVES if moves is None else moves, dtype=np.int32)
        assert self.moves.shape == (5, 2)
        rng = np.random.RandomState(seed)
        self.starting_x = rng.randint(0, self.grid_length + 1, self.num_agents).astype(np.int32)
        self.starting_y = rng.randint(0, self.grid_length + 1, self.num_agents).astype(np.int32)
        self.action_space = {a: spaces.Discrete(len(self.moves)) for a in range(self.num_agents)}
        self.observation_space = None  # filled in by EnvWrapper
        self.env_backend = env_backend
        self.timestep = None
        self.loc_x = self.loc_y = None
        self.last_max_spread = None  # largest spread of the last host step (tests choose `spread_limit` from it)

    # ------------------------------------------------------------------ host
    def reset(self):
        self.timestep = 0
        self.loc_x, self.loc_y = self.starting_x.copy(), self.starting_y.copy()
        return self._observation()

    def set_cells(self, x, y):
        """put the agents of the host replica on the given cells (what the device's custom reset does)"""
        self.loc_x = np.broadcast_to(np.int32(x), (self.num_agents,)).astype(np.int32)
        self.loc_y = np.broadcast_to(np.int32(y), (self.num_agents,)).astype(np.int32)

    def _observation(self):
        N, L = self.num_agents, self.grid_length
        span, length = _F32(N * L), _F32(L)
        sx, sy = np.int32(self.loc_x.sum(dtype=np.int32)), np.int32(self.loc_y.sum(dtype=np.int32))
        shared = [_F32(sx) / span, _F32(sy) / span, _F32(self.timestep) / _F32(self.episode_length)]
        return {a: np.array([_F32(self.loc_x[a]) / length, _F32(self.loc_y[a]) / length, *shared], dtype=np.float32)
                for a in range(N)}

    def step(self, actions=None):
        if self.env_backend != "cpu":
            return self._device_step()
        assert isinstance(actions, dict) and len(actions) == self.num_agents
        self.timestep += 1
        N, L = self.num_agents, self.grid_length
        move = self.moves[[int(np.asarray(actions[a]).reshape(-1)[0]) for a in range(N)]]
        mx, my = self.loc_x + move[:, 0], self.loc_y + move[:, 1]
        self.loc_x, self.loc_y = np.clip(mx, 0, L).astype(np.int32), np.clip(my, 0, L).astype(np.int32)
        hit = (self.loc_x != mx) | (self.loc_y != my)
        sx, sy = self.loc_x.sum(dtype=np.int32), self.loc_y.sum(dtype=np.int32)
        spread = (np.abs(N * self.loc_x - sx) + np.abs(N * self.loc_y - sy)).astype(np.int32)
        reward = -spread.astype(np.float32) / _F32(N * L)
        reward = np.where(hit, reward - _F32(self.wall_penalty), reward).astype(np.float32)
        self.last_max_spread = int(spread.max())
        done = self.timestep == self.episode_length or (self.spread_limit >= 0 and self.last_max_spread <= self.spread_limit)
        return self._observation(), {a: reward[a] for a in range(N)}, {"__all__": bool(done)}, {}

    # ---------------------------------------------------------------- device
    def get_data_dictionary(self):
        feed = DataFeed()
        feed.add_data(name=_LOC_X, data=self.starting_x.copy(), save_copy_and_apply_at_reset=True)
        feed.add_data(name=_LOC_Y, data=self.starting_y.copy(), save_copy_and_apply_at_reset=True)
        feed.add_data_list([("wall_penalty", self.wall_penalty), ("spread_limit", self.spread_limit),
                            ("grid_length", self.grid_length), ("reset_cell_x", self.reset_cell[0]),
                            ("reset_cell_y", self.reset_cell[1])])
        return feed

    def initialize_step_function_context(self, cuda_data_manager, cuda_function_manager, cuda_step_function_feed,
                                         step_function_name):
        ready = super().initialize_step_function_context(cuda_data_manager, cuda_function_manager,
                                                         cuda_step_function_feed, step_function_name)
        if ready:  # the move table goes into the __constant__ symbol of this env's own code object
            cuda_data_manager.add_shared_constants({_MOVES: self.moves.reshape(-1)})
            cuda_function_manager.initialize_shared_constants(cuda_data_manager, [_MOVES])
        return ready

    def _block(self):
        """one thread per agent, rounded up to whole wavefronts (the reductions of wd_env.h need whole wavefronts)"""
        return ((self.num_agents + 63) // 64 * 64, 1, 1)

    def step_launch(self):
        """(function, arguments, block, grid, dynamic LDS bytes) of one device step: RolloutEngine's per-tick plan"""
        return (self.cuda_step, list(self.cuda_step_function_feed(_STEP_ARGS)), self._block(),
                self.cuda_function_manager.grid, 0)

    def _device_step(self):
        self.timestep += 1
        self.cuda_step(*self.cuda_step_function_feed(_STEP_ARGS), block=self._block(),
                       grid=self.cuda_function_manager.grid)
