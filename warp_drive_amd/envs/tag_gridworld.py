"""TagGridWorld: N taggers chase one runner on an integer grid.

Host-side mirror of reference example_envs/tag_gridworld/tag_gridworld.py
(`TagGridWorld` :22-317, `CUDATagGridWorld` :320-380,
`CUDATagGridWorldWithResetPool` :383-475): same constructor, same reset()/step()
contract, same DataFeed registration; the device step launches the gfx950 kernel
`HipTagGridWorldStep` (csrc/kernels/tag_gridworld.hip) instead of the CUDA/Numba ones.
"""
import os

import numpy as np

from warp_drive_amd.utils import spaces
from warp_drive_amd.utils.constants import Constants
from warp_drive_amd.utils.data_feed import DataFeed
from warp_drive_amd.utils.gpu_environment_context import CUDAEnvironmentContext
from warp_drive_amd.utils.launch_checks import (NULL, UnsupportedRolloutShape, batch_arguments, check_packed, check_record,
                                                evaluation_outputs, rp_pad4, rp_policy_floats, tick_tag, unpack_policy_pair)

_OBSERVATIONS = Constants.OBSERVATIONS
_ACTIONS = Constants.ACTIONS
_REWARDS = Constants.REWARDS
_LOC_X = "loc_x"
_LOC_Y = "loc_y"


class TagGridWorld:
    """CPU environment (one replica)."""

    name = "TagGridWorld"
    RESET_IS_DETERMINISTIC = True  # reset() restarts from the constructor's starting locations: no random draw

    def __init__(self, num_taggers=10, grid_length=10, episode_length=100, starting_location_x=None,
                 starting_location_y=None, seed=None, wall_hit_penalty=0.1, tag_reward_for_tagger=10.0,
                 tag_penalty_for_runner=2.0, step_cost_for_tagger=0.01, use_full_observation=True,
                 env_backend="cpu"):
        assert num_taggers > 0 and episode_length > 0
        self.num_taggers = num_taggers
        self.num_agents = num_taggers + 1  # the last agent is the only runner (:65-66)
        self.episode_length = episode_length
        self.grid_length = grid_length
        self.np_random = np.random
        if seed is not None:
            self.seed(seed)
        # type 0 = tagger, 1 = runner (:81-87)
        self.agent_type = {a: int(a >= num_taggers) for a in range(self.num_agents)}
        self.taggers = {a: True for a in range(num_taggers)}
        self.runners = {self.num_agents - 1: True}
        if starting_location_x is None:
            assert starting_location_y is None
            centre = int(0.5 * grid_length)  # taggers start in the centre, the runner at (0, 0)
            starting_location_x = centre * np.ones(self.num_agents)
            starting_location_y = centre * np.ones(self.num_agents)
            starting_location_x[-1] = 0
            starting_location_y[-1] = 0
        else:
            assert len(starting_location_x) == self.num_agents
            assert len(starting_location_y) == self.num_agents
        self.starting_location_x = starting_location_x
        self.starting_location_y = starting_location_y
        # no-op, right, left, up, down
        self.step_actions = np.array([[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]])
        self.observation_space = None  # filled in by EnvWrapper
        self.action_space = {a: spaces.Discrete(len(self.step_actions)) for a in range(self.num_agents)}
        self.timestep = None
        self.global_state = None
        self.wall_hit_penalty = wall_hit_penalty
        self.tag_reward_for_tagger = tag_reward_for_tagger
        self.tag_penalty_for_runner = tag_penalty_for_runner
        self.step_cost_for_tagger = step_cost_for_tagger
        self.use_full_observation = use_full_observation
        self.env_backend = env_backend

    def seed(self, seed=None):
        self.np_random.seed(seed)
        return [seed]

    # ---------------------------------------------------------------- host reset / step
    def reset(self):
        self.timestep = 0
        T1 = self.episode_length + 1
        self.global_state = {
            _LOC_X: np.zeros((T1, self.num_agents), dtype=np.int32),
            _LOC_Y: np.zeros((T1, self.num_agents), dtype=np.int32),
        }
        self.global_state[_LOC_X][0] = self.starting_location_x
        self.global_state[_LOC_Y][0] = self.starting_location_y
        return self.generate_observation()

    def generate_observation(self):
        n, L, t = self.num_agents, self.grid_length, self.timestep
        x = self.global_state[_LOC_X][t]
        y = self.global_state[_LOC_Y][t]
        time = float(t) / self.episode_length
        types = np.array([self.agent_type[a] for a in range(n)])
        obs = {}
        if self.use_full_observation:
            shared = np.concatenate([x / L, y / L, types])
            for a in range(n):
                me = np.zeros(n)
                me[a] = 1
                obs[a] = np.concatenate([shared, me, [time]])
            return obs
        # partial: own cell, the other side's cell (runner for taggers, closest tagger for the runner)
        d2 = np.square(x[:-1] - x[-1]) + np.square(y[:-1] - y[-1])
        closest = int(np.argmin(d2))
        for a in range(n):
            o = n - 1 if a < n - 1 else closest
            obs[a] = np.array([x[a] / L, y[a] / L, x[o] / L, y[o] / L, self.agent_type[a], time])
        return obs

    def step(self, actions=None):
        self.timestep += 1
        assert isinstance(actions, dict) and len(actions) == self.num_agents
        n, L, t = self.num_agents, self.grid_length, self.timestep
        moves = self.step_actions[[actions[a] for a in range(n)]]
        x = self.global_state[_LOC_X][t - 1] + moves[:, 0]
        y = self.global_state[_LOC_Y][t - 1] + moves[:, 1]
        cx, cy = np.clip(x, 0, L), np.clip(y, 0, L)
        hit_wall = (x != cx) | (y != cy)
        self.global_state[_LOC_X][t] = cx
        self.global_state[_LOC_Y][t] = cy
        tag = bool(((cx[:-1] == cx[-1]) & (cy[:-1] == cy[-1])).any())
        reward = np.empty(n)
        reward[:-1] = self.tag_reward_for_tagger if tag else -1.0 * self.step_cost_for_tagger
        reward[-1] = -1.0 * self.tag_penalty_for_runner if tag else 1.0 * self.step_cost_for_tagger
        reward = reward + (-1.0 * self.wall_hit_penalty * hit_wall)
        rew = {a: reward[a] for a in range(n)}
        obs = self.generate_observation()
        done = {"__all__": t >= self.episode_length or tag}
        return obs, rew, done, {}


def gridworld_policy_floats(hidden):
    """floats of one packed policy of the live-policy rollout kernel (gw5_policy_floats in tag_gridworld_n5_common.h):
    W0 [H][24], b0 [H], W1 [H][H], b1 [H], Wp [5][H], bp [5], rounded up to whole 16-byte vectors"""
    return rp_pad4(rp_policy_floats(24, hidden, 5))


def _check_packed_policies(tensors, width, error):
    """every packed policy is a contiguous float32 CUDA tensor of gridworld_policy_floats(width) elements, else `error`"""
    for t in tensors:
        check_packed(t, gridworld_policy_floats(width), error, "a packed policy", f"width {width}")


_STEP_ARGS = [
    _LOC_X, _LOC_Y, _ACTIONS, "_done_", _REWARDS, _OBSERVATIONS, "wall_hit_penalty",
    "tag_reward_for_tagger", "tag_penalty_for_runner", "step_cost_for_tagger", "use_full_observation",
    "world_boundary", "_timestep_", ("episode_length", "meta"), ("n_agents", "meta"), ("n_envs", "meta"),
]


class _DeviceStepMixin(CUDAEnvironmentContext):
    """Device step: one launch of HipTagGridWorldStep over all replicas."""

    TICK_HEADS = 1  # action heads the fused tick kernel samples (RolloutEngine)

    def _scalar_feed(self):
        return [
            ("wall_hit_penalty", self.wall_hit_penalty),
            ("tag_reward_for_tagger", self.tag_reward_for_tagger),
            ("tag_penalty_for_runner", self.tag_penalty_for_runner),
            ("step_cost_for_tagger", self.step_cost_for_tagger),
            ("use_full_observation", self.use_full_observation),
            ("world_boundary", self.grid_length),
        ]

    def _geometry(self):
        """Blocks pack whole replicas (the kernels derive replicas-per-block from blockDim).  Small
        batches get small blocks so that the launch still spreads over the chip (1000 replicas of 5
        agents: 84 single-wavefront blocks instead of 20 blocks of 256 threads)."""
        fm = self.cuda_function_manager
        choice = None
        for max_threads in (256, 128, 64):
            choice = fm.packed_geometry(self.num_agents, max_threads=max(max_threads, self.num_agents))
            if choice[2][0] >= 512:
                break
        return choice

    def lds_bytes(self, epb):
        """dynamic LDS of HipTagGridWorldStep / Tick: positions (int + normalised float), per-replica
        timestep / done, and the [epb * N, F] observation image"""
        A = epb * self.num_agents
        F = 4 * self.num_agents + 1 if self.use_full_observation else 6
        tables = (4 * (4 * A + 2 * epb + 2) + 15) // 16 * 16   # positions, time steps, done + 2 vote flags; the image starts 16-byte aligned (read as float4)
        with_image = tables + 4 * A * F
        return with_image if with_image <= 60000 else tables  # WD_GW_IMAGE_MAX_BYTES

    def _step_args(self):
        """the step kernel's positional arguments.  The four reward scalars go in as FLOAT64 -- the env's own Python
        floats, not the float32 copies the data manager holds -- so that the kernel can form `reward_tag +
        reward_penalty` the way the CPU step does (float64, narrowed once: csrc/kernels/tag_gridworld_rewards.h)."""
        args = list(self.cuda_step_function_feed(_STEP_ARGS))
        first = _STEP_ARGS.index("wall_hit_penalty")
        args[first:first + 4] = [np.float64(self.wall_hit_penalty), np.float64(self.tag_reward_for_tagger),
                                 np.float64(self.tag_penalty_for_runner), np.float64(self.step_cost_for_tagger)]
        return args

    def step_launch(self):
        """(function, args, block, grid, shared_bytes) of one device step."""
        epb, block, grid = self._geometry()
        return self.cuda_step, self._step_args(), block, grid, self.lds_bytes(epb)

    ticks_per_launch = 1    # > 1 (with batch tensors): fixed-policy rollout, T ticks fused per launch

    ROLLOUT_POLICY_WIDTHS = (32, 64)   # HipTagGridWorldRollout_N5_H<width>
    ROLLOUT_POLICY_PACKING = "gridworld"   # training.policy_kernel.pack_gridworld_policy

    def rollout_policy_groups(self):
        """agents the live-policy rollout kernel evaluates ONE network for, in its argument order: the taggers, the
        runner (run_configs/tag_gridworld.yaml maps them to the "tagger" / "runner" policies)"""
        return [list(range(self.num_agents - 1)), [self.num_agents - 1]]

    ROLLOUT_POLICY_MAX_LDS = 160 * 1024   # dynamic LDS the live-policy rollout may ask for: a gfx950 workgroup's

    def n5_lds_bytes(self, table_entries, cache_dwords, pool_rows, width, round_time_table=True):
        """dynamic LDS of a 5-agent entry, the layout of tag_gridworld_n5_common.h in dwords: the image and the restore
        cache of 12 replicas, `table_entries` coordinate quotients (64, with a reset pool 256), the time table, the two
        pools of `pool_rows` rows, the two packed policies (width None: an entry without policies); times 4 bytes,
        rounded up to 16.  Every part is a whole number of 16-byte vectors -- but for the time table of the plain
        fixed-probability entry, which has nothing behind it (round_time_table=False)."""
        N, F = self.num_agents, 4 * self.num_agents + 1
        up4 = lambda n: (int(n) + 3) // 4 * 4   # noqa: E731
        time_table = int(self.episode_length) + 1
        dwords = (12 * N * F + 12 * int(cache_dwords) + int(table_entries)
                  + (up4(time_table) if round_time_table else time_table) + 2 * up4(N * int(pool_rows))
                  + (0 if width is None else 2 * gridworld_policy_floats(width)))
        return (4 * dwords + 15) // 16 * 16

    def live_policy_lds_bytes(self, width, cache_dwords=None):
        """dynamic LDS of HipTagGridWorldRollout_N5_H<width>: the restore cache, 64 coordinate quotients, no pools"""
        N, F = self.num_agents, 4 * self.num_agents + 1
        if cache_dwords is None:   # the reset arrays of the shape the kernel is admitted for: positions + observations
            cache_dwords = 2 * N + N * F
        return self.n5_lds_bytes(64, cache_dwords, 0, width)

    def has_live_policy_rollout(self, width, n_actions):
        """does a rollout kernel exist that evaluates the two policy networks itself (HipTagGridWorldRollout_N5_H<width>)
        for this env shape?  5 agents, full observations, 5 actions, hidden width 32 / 64, and its tables (the time
        table grows with the episode length) within ROLLOUT_POLICY_MAX_LDS (RolloutEngine asks before it calls
        `tick_launch(policy=...)`)"""
        return (int(width) in self.ROLLOUT_POLICY_WIDTHS and int(n_actions) == 5 and len(self.step_actions) == 5
                and self._specialised_rollout_shape()
                and self.live_policy_lds_bytes(width) <= self.ROLLOUT_POLICY_MAX_LDS
                and self.cuda_function_manager.has_function(f"HipTagGridWorldRollout_N5_H{int(width)}"))

    # Trainer.evaluate_episodes takes the one-launch evaluation of this env only under
    # `trainer.fused_rollout_policy: "all"`: the shipped configs keep the per-tick path they evaluate on
    EVALUATE_POLICY_OPT_IN = True
    _EVALUATE_SHAPES = ("the in-kernel evaluation exists for 5 agents with full observations, 5 actions and hidden "
                        "widths 32 / 64 only")

    def _evaluate_entry(self, width):
        return f"HipTagGridWorldEvaluate_N5_H{int(width)}"

    def _extra_launch_args(self):
        """what the 5-agent entries of this env take behind the common arguments"""
        return []

    def live_policy_evaluate_lds_bytes(self, width):
        """dynamic LDS of HipTagGridWorldEvaluate_N5_H<width>: the rollout's without the restore cache"""
        return self.n5_lds_bytes(64, 0, 0, width)

    def has_live_policy_evaluate(self, width, n_actions):
        """does an evaluation kernel exist that runs one episode of every replica with the two policy networks inside
        it (`_evaluate_entry(width)`, Trainer.evaluate_episodes)?  The shapes of the live-policy rollout, with the
        evaluation's own (smaller) tables within ROLLOUT_POLICY_MAX_LDS and its entry in the manifest."""
        return bool(self.has_live_policy_rollout(width, n_actions)
                    and self.live_policy_evaluate_lds_bytes(width) <= self.ROLLOUT_POLICY_MAX_LDS
                    and self.cuda_function_manager.has_function(self._evaluate_entry(width)))

    def evaluate_launch(self, sampler, policy, use_argmax, outputs, action_trace=None, ticks=None):
        """One episode of every replica in ONE launch (HipTagGridWorldEvaluate_N5_H<width>; with a reset pool _N5P_H<width>,
        which takes the pool's four arguments last and leaves the pool alone: an evaluation never restarts): from the
        positions, observation rows and time step the arrays hold, at most `ticks` (default: episode_length) ticks of policy
        networks -> action (use_argmax: the first maximum of the probabilities; else the counting draw of the rollout)
        -> step, up to the replica's first done.  policy = ((packed tagger policy, packed runner policy), hidden width)
        as in `tick_launch`.  outputs = {"reward_sum": float32 [E * 5] or [E, 5], "steps": int32 [E], "done": int32
        [E]}, CUDA tensors (at least that many elements); `action_trace` (optional) int32 [>= ticks, E, 5]: row k = tick
        k's actions of the replicas still running.  The launch writes those and, in sampled mode, the sampler's epoch
        words; the env's arrays are read only.  Returns (function, arguments, block, grid, shared bytes)."""
        fm, dm = self.cuda_function_manager, self.cuda_data_manager
        tagger, runner, width = unpack_policy_pair(policy)
        if not self.has_live_policy_evaluate(width, len(self.step_actions)):
            raise UnsupportedRolloutShape(self._EVALUATE_SHAPES)
        _check_packed_policies((tagger, runner), width, UnsupportedRolloutShape)
        E, N = int(dm.meta_info("n_envs")), self.num_agents
        T = int(self.episode_length if ticks is None else ticks)
        out_args = evaluation_outputs(outputs, E, AssertionError, reward_elements=E * N)
        if action_trace is not None:
            check_record(action_trace, "action_trace", "int32", T, E * N, AssertionError)
        name = self._evaluate_entry(width)
        fm.initialize_functions([name])
        args = self._step_args() + [
            sampler.rng_state, tick_tag(), np.int32(T), fm.global_address("kIndexToActionArr"), tagger, runner,
            np.int32(1 if use_argmax else 0)] + out_args + \
            [NULL if action_trace is None else action_trace] + self._extra_launch_args()
        return fm.get_function(name), args, (64, 1, 1), ((E + 11) // 12, 1), self.live_policy_evaluate_lds_bytes(width)

    def image_fits(self, epb):
        """does a block of `epb` replicas keep its observation rows in LDS (lds_bytes: the image is part of the sum)?"""
        F = 4 * self.num_agents + 1 if self.use_full_observation else 6
        return self.lds_bytes(epb) > 4 * epb * self.num_agents * F

    def _rollout_geometry(self, cache_dwords):
        """geometry of the T-tick rollout, which needs the LDS observation image: `_geometry()` where its blocks have
        one; else (wide rows: 15 agents with full observations have an image at 4 replicas per block and none at 17)
        the largest block size that has one, preferring a size that also holds the restore cache.  No size has one:
        UnsupportedRolloutShape -- the caller keeps its one-launch-per-tick path."""
        choice = self._geometry()
        if self.image_fits(choice[0]):
            return choice
        fm = self.cuda_function_manager
        fits = [g for g in (fm.packed_geometry(self.num_agents, max_threads=max(m, self.num_agents))
                            for m in (256, 128, 64)) if self.image_fits(g[0])]
        if not fits:
            raise UnsupportedRolloutShape(f"{self.num_agents} agents: the observation rows of one replica do not fit "
                                          "the LDS image the rollout kernel needs")
        with_cache = [g for g in fits if self.lds_bytes(g[0]) + 4 * g[0] * cache_dwords <= 60000]
        return (with_cache or fits)[0]

    def tick_launch(self, sampler, probabilities, resetter, env_range=None, batch=None, policy=None):
        """Fused rollout tick: sample the action + step + reset finished replicas in ONE launch
        (HipTagGridWorldTick).  probabilities = [float32 CUDA tensor [E, N, n_actions]].  `_done_`
        stays set for replicas that finished on the tick (already reset); the next tick clears it.
        With `ticks_per_launch` > 1 and `batch` = {"obs": [T, E, N, F] float32, "actions": [T, E, N, 1] int32,
        "rewards": [T, E, N] float32, "done": [T, E] int32} (env-level batch tensors, T >= ticks_per_launch) the
        launch is HipTagGridWorldRollout: T ticks of a fixed-policy rollout, tick k recorded in row k.
        `policy` (optional, 5 agents / full observations only) = ((packed tagger policy, packed runner policy), hidden
        width) -- float32 CUDA tensors from training.policy_kernel.pack_gridworld_policy: the launch evaluates the two
        policy networks itself on every tick's observation rows (HipTagGridWorldRollout_N5_H<width>) instead of reading
        `probabilities`."""
        assert env_range is None, "replica ranges are a TagContinuous experiment"
        assert len(probabilities) == 1
        fm, dm = self.cuda_function_manager, self.cuda_data_manager
        rollout = batch is not None and int(self.ticks_per_launch) > 1
        assert rollout or int(self.ticks_per_launch) == 1, "ticks_per_launch > 1 needs the batch tensors"
        name = self.cuda_step.name.replace("Step", "Rollout" if rollout else "Tick")
        fm.initialize_functions([name])
        _, reset_args, _, _ = resetter.fused_launch(dm, 0, 0)  # builds / refreshes the descriptor table
        cache_dwords = sum(int(np.prod(dm.get_shape(k)[1:])) for k in dm.reset_data_list) if rollout else 0
        epb, block, grid = self._rollout_geometry(cache_dwords) if rollout else self._geometry()
        if rollout and self._specialised_rollout_shape():
            # the specialised rollout kernel runs blocks of ONE wavefront (12 replicas) at every batch size
            epb, block, grid = 12, (64, 1, 1), ((int(dm.meta_info("n_envs")) + 11) // 12, 1)
        args = self._step_args() + [
            sampler.rng_state, probabilities[0], np.int32(probabilities[0].shape[-1]), reset_args[0], reset_args[1],
            tick_tag()]
        if rollout:
            E, N, T = int(dm.meta_info("n_envs")), self.num_agents, int(self.ticks_per_launch)
            F = 4 * N + 1 if self.use_full_observation else 6
            assert int(probabilities[0].shape[-1]) <= 8 and self.image_fits(epb) and len(self.step_actions) == 5, \
                "the rollout kernel needs the LDS observation image and at most 8 actions"
            batch_args = batch_arguments(batch, T, E, N, F)
            # the rows finished replicas are restored from are kept in LDS for the whole launch (no loads inside the
            # tick loop): the sum of the registered arrays' row lengths per replica, 0 = no room
            lds = self.lds_bytes(epb)
            if lds + 4 * epb * cache_dwords <= 60000:
                lds += 4 * epb * cache_dwords
            else:
                cache_dwords = 0
            args += [np.int32(T)] + batch_args + [np.int32(cache_dwords)]
            special = self._specialised_rollout(name, block, cache_dwords)
            if policy is not None:
                (tagger, runner), width = policy   # (as given: a malformed `policy` is the caller's bug here)
                if special is None or not self.has_live_policy_rollout(width, int(probabilities[0].shape[-1])):
                    raise UnsupportedRolloutShape("the live-policy rollout exists for 5 agents with full observations, "
                                                  "5 actions and hidden widths 32 / 64 only")
                _check_packed_policies((tagger, runner), width, AssertionError)
                special = f"{special}_H{width}"
                fm.initialize_functions([special])
                # the fixed-policy kernel's LDS with the time table rounded up to 16 bytes, then the two policies
                lds5 = self.live_policy_lds_bytes(width, cache_dwords)
                assert lds5 <= self.ROLLOUT_POLICY_MAX_LDS, (lds5, self.ROLLOUT_POLICY_MAX_LDS)
                return (fm.get_function(special), args + [fm.global_address("kIndexToActionArr"), tagger, runner], block,
                        grid, lds5)
            if special is not None:
                # the kernel specialised for this shape (csrc/kernels/tag_gridworld_n5.hip, its own code object):
                # same arguments + the device address of the action table the host uploads into the main code object
                fm.initialize_functions([special])
                return (fm.get_function(special), args + [fm.global_address("kIndexToActionArr")], block, grid,
                        self.n5_lds_bytes(64, cache_dwords, 0, None, round_time_table=False))
            return fm.get_function(name), args, block, grid, lds
        if policy is not None:
            raise UnsupportedRolloutShape("the live-policy rollout needs ticks_per_launch > 1 and the batch tensors")
        return fm.get_function(name), args, block, grid, self.lds_bytes(epb)

    SPECIALISED_ROLLOUT = os.environ.get("WD_GW_ROLLOUT_N5", "1") != "0"  # False: always the general rollout kernel

    def _specialised_rollout_shape(self):
        """the shape `HipTagGridWorldRollout_N5` is written for: 5 agents, full observations, and the registered reset
        arrays exactly the positions and the observations (the kernel restores those, and only those, in registers /
        LDS and writes them out after the last tick)"""
        dm, fm = self.cuda_data_manager, self.cuda_function_manager
        return (self.SPECIALISED_ROLLOUT and self.num_agents == 5 and bool(self.use_full_observation)
                and int(self.grid_length) <= 63 and int(self.episode_length) <= 4095
                and sorted(dm.reset_data_list) == sorted([_LOC_X, _LOC_Y, _OBSERVATIONS])
                and fm.has_function("HipTagGridWorldRollout_N5"))

    def _specialised_rollout(self, name, block, cache_dwords):
        """`HipTagGridWorldRollout_N5` when the launch has its shape, blocks of one wavefront and the restore rows
        cached in LDS, else None: the general kernel."""
        ok = (name == "HipTagGridWorldRollout" and int(block[0]) == 64 and cache_dwords > 0
              and self._specialised_rollout_shape())
        return name + "_N5" if ok else None

    def step(self, actions=None):
        self.timestep += 1
        if self.env_backend != "hip":
            raise Exception(f"{type(self).__name__} expects env_backend = 'hip'")
        fn, args, block, grid, shared = self.step_launch()
        fn(*args, block=block, grid=grid, shared=shared)


class CUDATagGridWorld(_DeviceStepMixin, TagGridWorld):
    """Device version (reference :320-380); the class name is kept for drop-in use."""

    def __init__(self, *args, **kwargs):
        TagGridWorld.__init__(self, *args, **kwargs)
        CUDAEnvironmentContext.__init__(self)

    def get_data_dictionary(self):
        feed = DataFeed()
        for key in (_LOC_X, _LOC_Y):
            feed.add_data(name=key, data=self.global_state[key][0], save_copy_and_apply_at_reset=True,
                          log_data_across_episode=True)
        feed.add_data_list(self._scalar_feed())
        return feed


class CUDATagGridWorldWithResetPool(_DeviceStepMixin, TagGridWorld):
    """Device version whose replicas restart from a random member of a pool (reference :383-475)."""

    POOL_SIZE = 5  # hard-coded in the reference too (:429)
    RESET_IS_DETERMINISTIC = False  # (kept per-replica: the observation placeholders are built the reference's way)

    def __init__(self, *args, **kwargs):
        TagGridWorld.__init__(self, *args, **kwargs)
        CUDAEnvironmentContext.__init__(self)

    def get_data_dictionary(self):
        feed = DataFeed()
        for key in (_LOC_X, _LOC_Y):
            feed.add_data(name=key, data=self.global_state[key][0], save_copy_and_apply_at_reset=False,
                          log_data_across_episode=False)
        feed.add_data_list(self._scalar_feed())
        return feed

    def get_reset_pool_dictionary(self):
        L = int(self.grid_length)
        cells = np.linspace(1, L - 1, L - 1)

        def draw():
            v = self.np_random.choice(cells, self.num_agents).astype(np.int32)
            v[-1] = 0  # the runner always restarts in the corner
            return v

        xs, ys = [], []
        for _ in range(self.POOL_SIZE):
            xs.append(draw())
            ys.append(draw())
        pool = DataFeed()
        pool.add_pool_for_reset(name=f"{_LOC_X}_reset_pool", data=np.stack(xs), reset_target=_LOC_X)
        pool.add_pool_for_reset(name=f"{_LOC_Y}_reset_pool", data=np.stack(ys), reset_target=_LOC_Y)
        return pool

    # ------------------------------------------------------------------ the one-launch rollout (tag_gridworld_n5_pool.hip)
    # HipTagGridWorldRollout_N5P / _N5P_H<width> run T ticks per launch and draw the pool row of a finished replica
    # themselves, HipTagGridWorldEvaluate_N5P_H<width> runs one episode per replica.  There is no fused SINGLE tick for this
    # env: without the batch tensors RolloutEngine builds sample, step, table reset, two pool launches, undo.
    ROLLOUT_POOL_RESET = True      # RolloutEngine: the T-tick entries restart from the pool inside the kernel
    ROLLOUT_POLICY_OPT_IN = True   # Trainer: the one launch only under `trainer.fused_rollout_policy: "all"`
    POOL_MAX_COORD = 255           # Gw5Pooled::MAX_COORD: the quotient table has 256 entries

    def _pools(self):
        """(name of the x pool, name of the y pool, rows) when the pools are exactly loc_x's and loc_y's, [rows, 5] each
        with the same number of rows; else None"""
        dm = self.cuda_data_manager
        pools = dict(dm.reset_target_to_pool)
        if sorted(pools) != sorted([_LOC_X, _LOC_Y]):
            return None
        sx, sy = tuple(dm.get_shape(pools[_LOC_X])), tuple(dm.get_shape(pools[_LOC_Y]))
        if sx != sy or len(sx) != 2 or sx[1] != self.num_agents or sx[0] < 1:
            return None
        return pools[_LOC_X], pools[_LOC_Y], int(sx[0])

    def _pool_generator(self):
        """the resetter's pool generator words (HIPEnvironmentReset.init_reset_pool), None before that call"""
        return getattr(getattr(self, "cuda_env_resetter", None), "_pool_rng", None)

    def pool_rollout_lds_bytes(self, width=0, cache_dwords=None, n_pool=None):
        """dynamic LDS of the N5P entries: `n5_lds_bytes` with 256 coordinate quotients, the two pools and the two packed
        policies (width 0, the fixed-probability entry: none).  The evaluation entries have neither cache nor pools
        (cache_dwords = 0, n_pool = 0)."""
        if cache_dwords is None:   # the reset arrays of the shape the kernel is admitted for: the observations
            cache_dwords = self.num_agents * (4 * self.num_agents + 1)
        if n_pool is None:
            pools = self._pools()
            n_pool = pools[2] if pools else 0
        return self.n5_lds_bytes(256, cache_dwords, n_pool, int(width) or None)

    def _pool_rollout_shape(self):
        """the shape the N5P entries are written for: 5 agents, full observations, coordinates within the 256-entry
        table, the registered reset arrays exactly the observations (the kernel restores those rows from LDS and the
        positions from the pools), the pools exactly loc_x / loc_y with equal row counts"""
        dm = self.cuda_data_manager
        return (self.num_agents == 5 and bool(self.use_full_observation) and len(self.step_actions) == 5
                and 1 <= int(self.grid_length) <= self.POOL_MAX_COORD and 1 <= int(self.episode_length) <= 4095
                and sorted(dm.reset_data_list) == [_OBSERVATIONS] and self._pools() is not None)

    def has_pool_rollout(self, n_actions=5):
        """HipTagGridWorldRollout_N5P (fixed probabilities) for this shape?"""
        return bool(1 <= int(n_actions) <= 8 and self._pool_rollout_shape() and self._pool_generator() is not None
                    and self.pool_rollout_lds_bytes(0) <= self.ROLLOUT_POLICY_MAX_LDS
                    and self.cuda_function_manager.has_function("HipTagGridWorldRollout_N5P"))

    def has_live_policy_rollout(self, width, n_actions):
        """HipTagGridWorldRollout_N5P_H<width> for this shape?  5 agents, full observations, 5 actions, width 32 / 64,
        grid_length <= 255, episode_length <= 4095, reset arrays = {observations}, pools = loc_x / loc_y with equal row
        counts, the pool generator initialised, the LDS within ROLLOUT_POLICY_MAX_LDS, the entry in the manifest"""
        return bool(int(width) in self.ROLLOUT_POLICY_WIDTHS and int(n_actions) == 5 and self._pool_rollout_shape()
                    and self._pool_generator() is not None
                    and self.pool_rollout_lds_bytes(width) <= self.ROLLOUT_POLICY_MAX_LDS
                    and self.cuda_function_manager.has_function(f"HipTagGridWorldRollout_N5P_H{int(width)}"))

    def live_policy_evaluate_lds_bytes(self, width):
        return self.pool_rollout_lds_bytes(width, cache_dwords=0, n_pool=0)

    _EVALUATE_SHAPES = ("the in-kernel evaluation with a reset pool exists for 5 agents with full observations, 5 actions, "
                        "grid_length <= 255 and hidden widths 32 / 64 only")

    def _evaluate_entry(self, width):
        return f"HipTagGridWorldEvaluate_N5P_H{int(width)}"

    def _extra_launch_args(self):
        """the pool generator's words, the two pools and their row count: the last four arguments of every N5P entry"""
        dm = self.cuda_data_manager
        x_pool, y_pool, n_pool = self._pools()
        return [self._pool_generator(), dm.device_data(x_pool), dm.device_data(y_pool), np.int32(n_pool)]

    def tick_launch(self, sampler, probabilities, resetter, env_range=None, batch=None, policy=None):
        """The T-tick rollout in ONE launch (`ticks_per_launch` > 1 and `batch`, as `CUDATagGridWorld.tick_launch`):
        HipTagGridWorldRollout_N5P on `probabilities`, or, with `policy` = ((packed tagger policy, packed runner policy),
        hidden width) -- a shared policy is the same tensor twice -- HipTagGridWorldRollout_N5P_H<width>.  Arguments: the
        N5 entry's, then the pool generator's words, the two pools and their row count."""
        assert env_range is None, "replica ranges are a TagContinuous experiment"
        assert len(probabilities) == 1
        fm, dm = self.cuda_function_manager, self.cuda_data_manager
        if batch is None or int(self.ticks_per_launch) <= 1:
            raise UnsupportedRolloutShape("the env with a reset pool has no fused single tick: its one-launch rollout needs "
                                          "ticks_per_launch > 1 and the batch tensors")
        if getattr(resetter, "_pool_rng", None) is None or self._pool_generator() is None:
            raise RuntimeError("the env has a reset pool: call init_reset_pool() before building the rollout")
        n_actions = int(probabilities[0].shape[-1])
        if policy is None:
            width, name = 0, "HipTagGridWorldRollout_N5P"
            if not self.has_pool_rollout(n_actions):
                raise UnsupportedRolloutShape("the one-launch rollout with a reset pool exists for 5 agents with full "
                                              "observations, grid_length <= 255 and the loc_x / loc_y pools only")
            pol_args = []
        else:
            tagger, runner, width = unpack_policy_pair(policy)
            if not self.has_live_policy_rollout(width, n_actions):
                raise UnsupportedRolloutShape("the live-policy rollout with a reset pool exists for 5 agents with full "
                                              "observations, 5 actions, grid_length <= 255 and hidden widths 32 / 64 only")
            _check_packed_policies((tagger, runner), width, UnsupportedRolloutShape)
            name, pol_args = f"HipTagGridWorldRollout_N5P_H{width}", [tagger, runner]
        fm.initialize_functions([name])
        _, reset_args, _, _ = resetter.fused_launch(dm, 0, 0)  # builds / refreshes the descriptor table
        E, N, T = int(dm.meta_info("n_envs")), self.num_agents, int(self.ticks_per_launch)
        F = 4 * N + 1
        batch_args = batch_arguments(batch, T, E, N, F)
        cache_dwords = N * F   # the registered reset arrays are exactly the observations (_pool_rollout_shape)
        args = self._step_args() + [
            sampler.rng_state, probabilities[0], np.int32(n_actions), reset_args[0], reset_args[1], tick_tag(),
            np.int32(T)] + batch_args + [np.int32(cache_dwords), fm.global_address("kIndexToActionArr")] + pol_args + \
            self._extra_launch_args()
        return fm.get_function(name), args, (64, 1, 1), ((E + 11) // 12, 1), self.pool_rollout_lds_bytes(width)
