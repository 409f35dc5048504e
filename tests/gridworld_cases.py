"""TagGridWorld cases shared by tests/test_gridworld_shapes_logic.py (host: every case is simulated with the oracle
alone and must reach the coverage it is meant to have) and tests/test_gpu_gridworld_shapes.py (device: the same
trajectories, bit for bit, under several launch geometries).  Nothing here touches a GPU.

A case's whole expected trajectory is a pure function of the case: the draws of the fused tick / rollout kernels are
`single_head_tick_uniform(row, epoch, seed words, "tick")`; the device tests write `Case.start_epochs()` into the epoch
words before the first tick, so tick k of a run uses epoch `start + k` (and they assert the device's own words say so
after every launch)."""
import zlib

import numpy as np

from oracle.core_np import sample_actions_counting, seed_words, single_head_tick_uniform
from oracle.tag_gridworld_np import STEP_ACTIONS, TagGridWorldOracle

F32 = np.float32
TICK_TAG = np.int32(zlib.crc32(b"tick") & 0x7FFFFFFF)   # function_manager._stream_tag("tick")
SAMPLER_SEED = 5

# (wall_hit_penalty, tag_reward_for_tagger, tag_penalty_for_runner, step_cost_for_tagger).  The first is the shipped
# set; for every other one the host test asserts that the float32-add form of at least one of the eight sums differs
# from float32 of the float64 sum (what the kernels must produce).
REWARD_SETS = {
    "shipped": (0.1, 10.0, 2.0, 0.01),
    "thirds": (1.0 / 3.0, 10.1, 2.7, 0.07),
    "small_cost": (0.3, 7.3, 1.9, 1e-3),
    "negative": (-0.7, -3.1, -0.41, 0.011),
    "big": (1234.567, 98765.4321, 0.1, 3.3e-5),
}


def reward_table(scalars):
    """float32 of the oracle's float64 `reward_tag + penalty`, [kind (0 tagger, 1 runner)][tagged][wall]"""
    wall, tag_t, tag_r, cost = (float(v) for v in scalars)
    out = np.empty((2, 2, 2), F32)
    for kind in (0, 1):
        for tg in (0, 1):
            base = (tag_t if tg else -1.0 * cost) if kind == 0 else (-1.0 * tag_r if tg else 1.0 * cost)
            for wl in (0, 1):
                out[kind, tg, wl] = F32(np.float64(base) + np.float64(-1.0 * wall * wl))
    return out


def reward_table_float32_add(scalars):
    """the same eight sums the way the reference's CUDA kernel forms them: float32 scalars, float32 add"""
    wall, tag_t, tag_r, cost = (F32(v) for v in scalars)
    out = np.empty((2, 2, 2), F32)
    for kind in (0, 1):
        for tg in (0, 1):
            base = (tag_t if tg else F32(-1.0) * cost) if kind == 0 else (F32(-1.0) * tag_r if tg else cost)
            for wl in (0, 1):
                out[kind, tg, wl] = F32(base + (F32(-1.0) * wall if wl else F32(0.0)))
    return out


class Case:
    def __init__(self, name, N, L, T, full, E, ticks, reward="thirds", starts="random", push_t=None, onehot=0.25,
                 seed=0):
        self.name, self.N, self.L, self.T, self.full, self.E, self.ticks = name, N, L, T, bool(full), E, ticks
        self.reward, self.starts, self.push_t, self.onehot, self.seed = reward, starts, push_t, onehot, seed
        self.F = 4 * N + 1 if full else 6

    def __repr__(self):
        return self.name

    def config(self):
        wall, tag_t, tag_r, cost = REWARD_SETS[self.reward]
        cfg = dict(num_taggers=self.N - 1, grid_length=self.L, episode_length=self.T, wall_hit_penalty=wall,
                   tag_reward_for_tagger=tag_t, tag_penalty_for_runner=tag_r, step_cost_for_tagger=cost,
                   use_full_observation=self.full)
        x, y = self.start_cells()
        if x is not None:
            cfg["starting_location_x"], cfg["starting_location_y"] = x, y
        return cfg

    def start_cells(self):
        N, L = self.N, self.L
        rng = np.random.RandomState(1000 + self.seed)
        if self.starts == "default":
            return None, None
        if self.starts == "random":
            return rng.randint(0, L + 1, size=N).astype(np.int32), rng.randint(0, L + 1, size=N).astype(np.int32)
        if self.starts == "stacked":
            # every tagger on ONE cell two steps off the runner's diagonal: after a tick, taggers that moved right and
            # taggers that moved up stand on different cells at the same distance -- the first argmin decides by index
            c = min(2, L)
            x, y = np.full(N, c, np.int32), np.full(N, c, np.int32)
            x[-1] = y[-1] = 0
            return x, y
        assert self.starts == "corners"
        # tagger 0 in the far corner (walks into the wall), tagger 1 next to the runner (steps onto it), the others
        # on the far wall, the runner in the near corner
        x, y = np.full(N, L, np.int32), np.full(N, L, np.int32)
        if N > 2:
            x[1], y[1] = min(1, L), 0
            x[2:N - 1] = max(L - 1, 0)
        else:
            x[0], y[0] = min(1, L), 0
        x[-1] = y[-1] = 0
        return x, y

    def start_timesteps(self):
        """`_timestep_` pushed before the first tick (None: 0 everywhere): every replica of classes 2 and 3 (see
        probabilities) starts `push_t` ticks into its episode, so that a long episode times out inside the run"""
        if self.push_t is None:
            return None
        t = np.zeros(self.E, np.int32)
        t[np.arange(self.E) % 4 >= 2] = self.push_t
        return t

    def start_epochs(self):
        """epoch word of every agent row before the first tick: different from row to row (after `init_random` they are
        all 0, and every fused launch advances all of them alike -- a kernel that used another row's word would go
        unnoticed)"""
        rows = np.arange(self.E * self.N, dtype=np.uint64)
        return (((rows * np.uint64(2654435761)) >> np.uint64(9)) & np.uint64(0xFFF)).astype(np.uint32)

    def probabilities(self):
        """float32 [E, N, 5]: Dirichlet rows, a share of one-hot rows (agents that keep walking into a wall or onto the
        runner), and for the crafted starts four replica classes by e % 4 with fixed one-hot rows:
        0: tagger 0 right (wall), tagger 1 left (onto the runner), runner left (wall): tagged, taggers and runner at a wall
        1: tagger 1 left, runner stays: tagged, runner not at a wall
        2: everyone stays, tagger 0 right: nobody tagged, tagger at a wall -- runs into the time-out
        3: runner down (wall), the others stay: nobody tagged, runner at a wall -- runs into the time-out"""
        E, N = self.E, self.N
        rng = np.random.RandomState(2000 + self.seed)
        p = rng.dirichlet(np.ones(5), size=(E, N)).astype(F32)
        hot = rng.random_sample((E, N)) < self.onehot
        p[hot] = np.eye(5, dtype=F32)[rng.randint(0, 5, size=int(hot.sum()))]
        if self.starts == "corners":
            stay, right, left, down = 0, 1, 2, 4
            near = 1 if N > 2 else 0   # the tagger next to the runner
            cls = np.arange(E) % 4
            rows = np.full((E, N), stay)
            if N > 2:
                rows[:, 0] = right
            rows[cls <= 1, near] = left
            rows[cls == 0, N - 1] = left
            rows[cls == 3, N - 1] = down
            fixed = np.arange(E) % 8 < 4 if self.push_t is None else np.ones(E, bool)   # (half stay random otherwise)
            p[fixed] = np.eye(5, dtype=F32)[rows[fixed]]
        return p


class Coverage:
    """what a simulated run exercised, counted from the oracle alone"""

    def __init__(self):
        self.tags = self.timeouts = self.restarts = self.ticks = 0
        self.seen = np.zeros((2, 2, 2), bool)   # [kind][tagged][wall]
        self.consecutive = 0                    # replicas that finished on two consecutive ticks
        self._last_done = None

    def add(self, orc, px, py, a):
        wall = ((px + STEP_ACTIONS[a, 0]) != orc.loc_x) | ((py + STEP_ACTIONS[a, 1]) != orc.loc_y)
        tagged = ((orc.loc_x[:, :-1] == orc.loc_x[:, -1:]) & (orc.loc_y[:, :-1] == orc.loc_y[:, -1:])).any(axis=1)
        self.tags += int(tagged.sum())
        self.timeouts += int(((orc.timestep >= orc.T) & ~tagged).sum())
        self.restarts += int((orc.done > 0).sum())
        self.ticks += 1
        for tg in (0, 1):
            m = tagged == bool(tg)
            for wl in (0, 1):
                self.seen[0, tg, wl] |= bool((wall[m, :-1] == bool(wl)).any())
                self.seen[1, tg, wl] |= bool((wall[m, -1] == bool(wl)).any())
        if self._last_done is not None:
            self.consecutive += int(((orc.done > 0) & self._last_done).sum())
        self._last_done = orc.done > 0

    def line(self):
        return (f"{self.ticks} ticks, {self.tags} tags, {self.timeouts} time-outs, {self.restarts} restarts, "
                f"{int(self.seen.sum())}/8 reward cases, {self.consecutive} back-to-back finishes")

    def check(self, E):
        """the conditions every Tick / Rollout case of the shape and geometry matrix must meet"""
        assert self.tags >= 1 and self.timeouts >= 1 and 2 * self.restarts >= E and self.seen.all(), self.line()


def make_oracle(case):
    orc = TagGridWorldOracle(num_envs=case.E, **case.config())
    t0 = case.start_timesteps()
    if t0 is not None:
        orc.timestep = t0.copy()   # (the observations keep the time of the reset: the device array is pushed the same way)
    return orc


def simulate(case, sampled=True, keep_obs_step=False, restart_rows=None):
    """expected trajectory of `case.ticks` ticks: a list of per-tick records and the Coverage.  sampled: the actions
    are the fused kernels' draws (epoch k on tick k) on case.probabilities(); else uniform random actions (Step)."""
    E, N = case.E, case.N
    orc = make_oracle(case)
    lo, hi = seed_words(SAMPLER_SEED)
    probs = case.probabilities() if sampled else None
    rng = np.random.RandomState(3000 + case.seed)
    cov, ticks = Coverage(), []
    epoch0 = case.start_epochs()
    obs0 = orc.obs.astype(F32)
    for k in range(case.ticks):
        if sampled:
            u = single_head_tick_uniform(E * N, epoch0 + np.uint32(k), lo, hi, TICK_TAG)
            a = sample_actions_counting(probs, u.reshape(E, N))
        else:
            a = rng.randint(0, 5, size=(E, N)).astype(np.int32)
        px, py = orc.loc_x.copy(), orc.loc_y.copy()
        orc.step(a)
        cov.add(orc, px, py, a)
        rec = dict(actions=a, rewards=orc.rewards.astype(F32), done=orc.done.copy(), step_x=orc.loc_x.copy(),
                   step_y=orc.loc_y.copy(), step_t=orc.timestep.copy())
        if keep_obs_step:
            rec["obs_step"] = orc.obs.astype(F32)
        orc.reset_done_envs()
        rec.update(loc_x=orc.loc_x.copy(), loc_y=orc.loc_y.copy(), timestep=orc.timestep.copy(), obs=orc.obs.astype(F32))
        ticks.append(rec)
    return obs0, ticks, cov


# ---------------------------------------------------------------------------------------------- the case matrix
# (N, L, T) with uniform actions and random starts reach all eight reward cases within 21 .. 60 ticks for the small
# grids; grids of 63 / 64 / 200 do not -- those use the crafted corner starts and a pushed timestep.
STEP_CASES = [
    Case("step_N2_L1_full", 2, 1, 5, True, 1777, 24, reward="thirds", seed=1),
    Case("step_N3_L2_partial_stacked", 3, 2, 7, False, 1201, 24, reward="negative", starts="stacked", seed=2),
    Case("step_N7_L7_partial", 7, 7, 11, False, 515, 30, reward="small_cost", seed=3),
    Case("step_N13_L10_full", 13, 10, 23, True, 333, 40, reward="big", seed=4),
    Case("step_N16_L200_partial_corners", 16, 200, 12, False, 260, 24, reward="thirds", starts="corners", seed=5),
    Case("step_N33_L10_full", 33, 10, 12, True, 150, 24, reward="negative", seed=6),
    Case("step_N64_L64_full_noimage", 64, 64, 9, True, 50, 20, reward="small_cost", starts="corners", seed=7),
    Case("step_N65_L4_partial", 65, 4, 3, False, 70, 16, reward="big", starts="default", seed=8),
    Case("step_N105_L3_full_noimage", 105, 3, 3, True, 23, 16, reward="thirds", starts="default", seed=9),
    Case("step_N257_L3_full_noimage", 257, 3, 2, True, 7, 14, reward="negative", starts="default", seed=10),
]
TICK_CASES = [
    Case("tick_N2_L1_full", 2, 1, 5, True, 1700, 30, reward="thirds", seed=11),
    Case("tick_N6_L7_partial_stacked", 6, 7, 11, False, 700, 60, reward="negative", starts="stacked", seed=12),
    Case("tick_N8_L10_full", 8, 10, 23, True, 500, 60, reward="small_cost", seed=13),
    Case("tick_N14_L63_partial_corners", 14, 63, 40, False, 300, 30, reward="big", starts="corners", push_t=30, seed=14),
    Case("tick_N64_L3_full_noimage", 64, 3, 3, True, 50, 40, reward="thirds", starts="default", seed=15),
    Case("tick_N105_L4_partial", 105, 4, 3, False, 30, 40, reward="negative", starts="default", seed=16),
]
ROLLOUT_CASES = [   # ticks = ticks per launch x launches (the device test splits them)
    Case("rollout_N2_L1_full", 2, 1, 5, True, 1800, 32, reward="thirds", seed=21),
    Case("rollout_N3_L2_partial_stacked", 3, 2, 7, False, 1300, 36, reward="negative", starts="stacked", seed=22),
    Case("rollout_N6_L7_full", 6, 7, 11, True, 640, 60, reward="small_cost", seed=23),
    Case("rollout_N8_L64_partial_corners", 8, 64, 50, False, 400, 30, reward="big", starts="corners", push_t=40, seed=24),
    Case("rollout_N13_L10_full_nocache", 13, 10, 23, True, 310, 60, reward="thirds", seed=25),
    Case("rollout_N16_L6_partial", 16, 6, 12, False, 260, 48, reward="negative", seed=26),
    Case("rollout_N33_L10_full", 33, 10, 12, True, 100, 48, reward="small_cost", seed=27),
]
ROLLOUT_TICKS_PER_LAUNCH = {"rollout_N2_L1_full": 8, "rollout_N3_L2_partial_stacked": 9, "rollout_N6_L7_full": 15,
                            "rollout_N8_L64_partial_corners": 10, "rollout_N13_L10_full_nocache": 12,
                            "rollout_N16_L6_partial": 12, "rollout_N33_L10_full": 8}
