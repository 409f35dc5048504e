"""Cases, launch geometries and a host replay for the five single-agent envs off their one tested shape: Cartpole
(csrc/kernels/cartpole.hip) and Acrobot, MountainCar, ContinuousMountainCar, Pendulum (csrc/kernels/classic_control.hip).
Shared by tests/test_classic_control_shapes_logic.py (host: every case is replayed with the numpy steps and the host's
Philox replay alone and must reach the coverage it is meant to have) and tests/test_gpu_classic_control_shapes.py (device:
the same cases under several blocks and grids).  Nothing here touches a GPU.

The host replay sizes the cases; it is not the device tests' yardstick (a float64 cos may differ from the device's in
its last bit): those compare with the Step kernel + reset_when_done, and Cartpole with oracle/cartpole_np.py.  What IS
shared bit for bit is every draw: the discrete actions are a pure function of (seed words, row, epoch, probabilities)
and so is every pool pick."""
import math
import zlib

import numpy as np

from oracle.core_np import (ou_step_f32, ou_uniforms, pool_pick, sample_actions_counting, seed_words,
                            single_head_tick_uniform)

F32 = np.float32
TICK_TAG = np.int32(zlib.crc32(b"tick") & 0x7FFFFFFF)   # function_manager._stream_tag("tick")
SAMPLER_SEED, POOL_SEED, ENV_SEED = 5, 23, 5
# the one (row, epoch) among rows 0 .. 62 x epochs 0 .. 16643 (2^20 candidates) whose uniform is exactly 1.0 under
# SAMPLER_SEED (found with the host replay; test_classic_control_shapes_logic.py asserts it)
ONE_DRAW = (61, 3719)
WRAP_EPOCH = 0xFFFFFFFD            # a launch of >= 3 ticks that starts here crosses the 2^32 wrap
WRAP_ROWS = slice(8, 24)           # the rows that start there (cases with "residue" epochs and E >= 63)
LAUNCH_BOUND = 256                 # __launch_bounds__ of every classic_control.hip entry; no block may exceed it
OU_PARAMS = (0.15, 0.2, 1.0)       # damping, stddev, scale: tick_launch's defaults

ENVS = ("cartpole", "acrobot", "mountain_car", "continuous_mountain_car", "pendulum")
DISCRETE = ("cartpole", "acrobot", "mountain_car")
STATE_DIM = {"cartpole": 4, "acrobot": 4, "mountain_car": 2, "continuous_mountain_car": 2, "pendulum": 2}
OBS_DIM = {"cartpole": 4, "acrobot": 6, "mountain_car": 2, "continuous_mountain_car": 2, "pendulum": 3}
ENTRY = {"cartpole": "HipClassicControlCartPoleEnv", "acrobot": "HipClassicControlAcrobotEnv",
         "mountain_car": "HipClassicControlMountainCarEnv",
         "continuous_mountain_car": "HipClassicControlContinuousMountainCarEnv",
         "pendulum": "HipClassicControlPendulumEnv"}

# physics other than gym's defaults, passed through the env's `physics` class (and the same class to the numpy step)
OTHER_PHYSICS = {
    "mountain_car": dict(goal_velocity=0.05, max_speed=0.05, min_position=-0.9, force=0.002),
    "continuous_mountain_car": dict(min_action=-0.5, max_action=2.0, power=0.003, goal_position=0.3),
}


# ------------------------------------------------------------------------------------------------------ geometries
# "product": the host's own; (threads, None): one trip, ceil(E / threads) blocks; (threads, blocks): a fixed grid, which
# must take >= 3 trips of the grid-stride loop; (threads, "idle"): one trip and two further blocks without a replica.
GEOMETRIES = ("product", (64, None), (128, 3), (192, 1), (256, 3), (64, "idle"))


def geometry(E, geom, product=None):
    """(threads, blocks, trips) of `geom` at E replicas; None when a fixed grid would take fewer than three trips (the
    case is too small for it: it is skipped there, and the host test asserts every fixed grid runs somewhere).  A block
    above the entries' launch bound is refused here and never launched."""
    if geom == "product":
        threads, blocks = product if product is not None else (256, max(1, min(4096, -(-E // 256))))
    else:
        threads, blocks = geom
        if threads > LAUNCH_BOUND:
            raise ValueError(f"a block of {threads} threads exceeds the entries' launch bound of {LAUNCH_BOUND}")
        if blocks is None:
            blocks = -(-E // threads)
        elif blocks == "idle":
            blocks = -(-E // threads) + 2
        else:
            if -(-E // (threads * blocks)) < 3:
                return None
    return int(threads), int(blocks), -(-E // (threads * blocks))


def geometries(E):
    return [g for g in GEOMETRIES if geometry(E, g) is not None]


# ------------------------------------------------------------------------------------------------------------ envs
def device_class(env):
    from warp_drive_amd.envs import cartpole as cp
    from warp_drive_amd.envs import classic_control as cc

    return {"cartpole": cp.CUDAClassicControlCartPoleEnv, "acrobot": cc.CUDAClassicControlAcrobotEnv,
            "mountain_car": cc.CUDAClassicControlMountainCarEnv,
            "continuous_mountain_car": cc.CUDAClassicControlContinuousMountainCarEnv,
            "pendulum": cc.CUDAClassicControlPendulumEnv}[env]


def make_env(env, episode_length, pool=0, physics=None):
    """the device env object of a case (no GPU is touched until a wrapper is built around it)"""
    e = device_class(env)(episode_length=episode_length, seed=ENV_SEED, reset_pool_size=pool)
    if physics:
        e.physics = type("Physics", (e.physics,), dict(physics))
    return e


def _cartpole_step(state, action):
    from oracle.cartpole_np import CartPoleOracle

    orc = CartPoleOracle(len(state), 1 << 30)
    orc.state = np.asarray(state, F32).copy()
    obs, rew, done = orc.step(action)
    return orc.state, obs, rew, done.astype(np.int32)


def numpy_step(env, physics=None):
    """f(state [E, S] float32, action [E]) -> (state, obs, reward, terminal code)"""
    from warp_drive_amd.envs import classic_control as cc

    if env == "cartpole":
        return _cartpole_step
    fn = {"acrobot": cc.acrobot_step, "mountain_car": cc.mountain_car_step,
          "continuous_mountain_car": cc.continuous_mountain_car_step, "pendulum": cc.pendulum_step}[env]
    base = {"acrobot": cc.AcrobotPhysics, "mountain_car": cc.MountainCarPhysics,
            "continuous_mountain_car": cc.ContinuousMountainCarPhysics, "pendulum": cc.PendulumPhysics}[env]
    p = type("Physics", (base,), dict(physics)) if physics else base
    return lambda s, a: fn(s, a, p)


def spread_states(env, rng, E):
    """first episodes from all over the state space (terminal states and the walls included)"""
    lo, hi = {"cartpole": ([-2.3, -1.0, -0.2, -1.0], [2.3, 1.0, 0.2, 1.0]),
              "acrobot": ([-3.1, -3.1, -12.0, -28.0], [3.1, 3.1, 12.0, 28.0]),
              "mountain_car": ([-1.2, -0.07], [0.58, 0.07]), "continuous_mountain_car": ([-1.2, -0.07], [0.5, 0.07]),
              "pendulum": ([-3.1, -8.0], [3.1, 8.0])}[env]
    return rng.uniform(lo, hi, size=(E, len(lo))).astype(F32)


# --------------------------------------------------------------------------------------------- crafted step rows
# Rows whose outcome a clip or an exact compare decides (a last-bit difference of a float64 cos cannot flip them).
# Each: (state, action, start timestep or None = 0, label).  `T` = the case's episode length.
def crafted_step_rows(env, T, physics=None):
    from warp_drive_amd.envs import classic_control as cc

    pi32 = float(F32(math.pi))
    if env in ("mountain_car", "continuous_mountain_car"):
        base = cc.MountainCarPhysics if env == "mountain_car" else cc.ContinuousMountainCarPhysics
        p = type("Physics", (base,), dict(physics or {}))
        lo, hi = (0, 2) if env == "mountain_car" else (-3.0, 3.0)
        rows = [((p.min_position, -p.max_speed), lo, None, "wall"),
                ((0.59, p.max_speed), hi, None, "goal"),
                ((0.59, p.max_speed), hi, T - 1, "goal_on_last_tick"),
                ((0.2, 0.0), hi, T - 1, "last_tick")]
        if p.goal_velocity == p.max_speed:
            rows += [((0.5, p.max_speed), hi, None, "goal_at_clipped_speed"),
                     ((0.5, 0.0), hi, None, "slow_past_goal")]
        if env == "continuous_mountain_car":
            rows += [((-0.5, 0.0), 3.0, None, "action_above"), ((-0.5, 0.0), -3.0, None, "action_below"),
                     ((-0.5, 0.0), p.min_action, None, "action_min"), ((-0.5, 0.0), p.max_action, None, "action_max")]
        return rows
    if env == "acrobot":
        near = pi32 - 5e-4
        v1, v2 = float(F32(4 * math.pi)), float(F32(9 * math.pi))
        return [((near, 0.0, 3.0, 0.0), 2, None, "wrap_theta1_up"), ((-near, 0.0, -3.0, 0.0), 0, None, "wrap_theta1_down"),
                ((0.0, near, 0.0, 4.0), 2, None, "wrap_theta2_up"), ((0.0, -near, 0.0, -4.0), 0, None, "wrap_theta2_down"),
                ((0.0, 0.0, v1, v2), 2, None, "bound_up"), ((0.0, 0.0, -v1, -v2), 0, None, "bound_down"),
                ((0.1, 0.1, v1, -v2), 1, None, "bound_mixed"), ((0.1, 0.1, -v1, v2), 1, None, "bound_mixed2"),
                ((pi32, 0.0, 0.0, 0.0), 1, T - 1, "upright_last_tick")]
    if env == "pendulum":
        rows = []
        for th in (10.0, 37.5, 90.0, pi32):
            for sg in (1.0, -1.0):
                for thdot in (8.0, -8.0):
                    rows.append(((sg * th, thdot), 2.5 * sg, None, f"theta_{sg * th:g}_{thdot:g}"))
        return rows
    return []


# ----------------------------------------------------------------------------------------------------------- cases
class StepCase:
    def __init__(self, env, E=700, ticks=40, episode_length=13, physics=None):
        self.env, self.E, self.ticks, self.T, self.physics = env, E, ticks, episode_length, physics
        self.name = f"step-{env}-E{E}" + ("-other-physics" if physics else "")

    def __repr__(self):
        return self.name

    def crafted(self):
        return crafted_step_rows(self.env, self.T, self.physics)

    def start(self):
        """(state [E, S], timestep [E]) before tick 0: spread states, the crafted rows first"""
        rng = np.random.RandomState(1)
        state = spread_states(self.env, rng, self.E)
        ts = np.zeros(self.E, np.int32)
        for i, (s, _, t0, _) in enumerate(self.crafted()):
            state[i] = np.asarray(s, F32)
            ts[i] = 0 if t0 is None else t0
        return state, ts

    def actions(self):
        """[ticks, E]: random (the continuous ones beyond the clip range too), tick 0 of the crafted rows as listed"""
        rng = np.random.RandomState(2)
        if self.env in DISCRETE:
            a = rng.randint(0, 2 if self.env == "cartpole" else 3, size=(self.ticks, self.E)).astype(np.int32)
        else:
            a = rng.uniform(-3.0, 3.0, size=(self.ticks, self.E)).astype(F32)
        for i, (_, act, _, _) in enumerate(self.crafted()):
            a[0, i] = act
        return a


STEP_CASES = [StepCase(env, E) for env in ENVS for E in (700, 1601)] + \
             [StepCase(env, 700, physics=OTHER_PHYSICS[env]) for env in OTHER_PHYSICS]


class TickCase:
    """One fused-tick scenario.  epochs: "zero" (every replica at epoch 0), "residue" (row % 4, the rows WRAP_ROWS at
    0xfffffffd) or "odd" (2 * (row % 8) + 1); in every discrete case with more than ONE_DRAW's row, that row starts two
    ticks before the epoch whose uniform is exactly 1.0.  timesteps: "zero", "spread" (row % episode_length) or "mostly-zero".
    rows: None (no batch tensors) or the number of rows of the batch tensors (>= ticks).  extra: "third" registers a
    third reset array of one float per replica (Cartpole's uncached restore)."""

    def __init__(self, name, env, E=700, T=4, ticks=11, launches=3, rows=None, pool=0, A=None, epochs="residue",
                 timesteps="spread", physics=None, extra=None, share=0.02):
        self.name, self.env, self.E, self.T, self.ticks, self.launches = f"{env}-{name}", env, E, T, ticks, launches
        self.rows, self.pool, self.epochs, self.timesteps, self.physics, self.extra = rows, pool, epochs, timesteps, physics, extra
        self.cont = env not in DISCRETE
        self.A = (2 if env == "cartpole" else 3) if A is None and not self.cont else A
        self.share = share   # the smallest share every action must reach on the host replay
        assert ticks <= 50 and E in (1, 63, 65, 700, 1501, 1601) and launches >= 3
        assert rows is None or rows >= ticks

    def __repr__(self):
        return self.name

    # ---- what the device test writes before the first launch
    def has_one_draw(self):
        return not self.cont and self.E > ONE_DRAW[0] and self.ticks >= 3

    def start_epochs(self):
        rows = np.arange(self.E, dtype=np.uint32)
        if self.epochs == "zero":
            ep = np.zeros(self.E, np.uint32)
        elif self.epochs == "odd":
            ep = (2 * (rows % 8) + 1).astype(np.uint32)
        else:
            ep = (rows % 4).astype(np.uint32)
            if self.E >= 63:
                ep[WRAP_ROWS] = WRAP_EPOCH
        if self.has_one_draw():
            ep[ONE_DRAW[0]] = ONE_DRAW[1] - 2
        return ep

    def start_pool_epochs(self):
        rows = np.arange(self.E, dtype=np.uint32)
        if self.epochs == "zero":
            return np.zeros(self.E, np.uint32)
        ep = (rows % 4).astype(np.uint32)
        if self.E >= 63:
            ep[WRAP_ROWS] = WRAP_EPOCH
        return ep

    def start_timesteps(self):
        if self.timesteps == "zero":
            return np.zeros(self.E, np.int32)
        if self.timesteps == "mostly-zero":   # four replicas in five start an episode with the first launch
            rows = np.arange(self.E)
            return np.where(rows % 5 == 0, rows % self.T, 0).astype(np.int32)
        return (np.arange(self.E) % self.T).astype(np.int32)

    def start_states(self):
        return spread_states(self.env, np.random.RandomState(11), self.E)

    def probabilities(self):
        """discrete: [E, A] float32 Dirichlet rows, then the crafted ones: one-hot at each end, a row whose float32 running
        sum ends below 1.0 (also ONE_DRAW's row: its draw of exactly 1.0 must clamp to the last action), zeros in the
        middle.  Box: the means [E] in [-1.5, 1.5]."""
        rng = np.random.RandomState(3)
        if self.cont:
            return rng.uniform(-1.5, 1.5, size=self.E).astype(F32)
        A = self.A
        p = rng.dirichlet(np.ones(A), size=self.E).astype(F32)
        short = np.full(A, F32(0.999) / F32(A), F32)
        assert np.cumsum(short, dtype=F32)[-1] < 1
        if self.E == 1:
            p[0] = short
        if self.E >= 63:
            p[0] = np.eye(A, dtype=F32)[0]
            p[1] = np.eye(A, dtype=F32)[A - 1]
            p[2] = short
            middle = np.zeros(A, F32)
            middle[0], middle[A - 1] = (0.5, 0.5) if A > 1 else (1.0, 1.0)
            p[3] = middle
            p[4, A // 2] = 0.0   # an inner zero in an otherwise dense row (no longer normalised)
            p[ONE_DRAW[0]] = short
        return p

    def actions(self):
        """discrete: the actions of every tick, [launches * ticks, E] int32, from the host's Philox replay"""
        assert not self.cont
        k0, k1 = seed_words(SAMPLER_SEED)
        p, ep = self.probabilities(), self.start_epochs()
        out = np.empty((self.launches * self.ticks, self.E), np.int32)
        for k in range(len(out)):
            u = single_head_tick_uniform(self.E, ep + np.uint32(k), k0, k1, TICK_TAG)
            out[k] = sample_actions_counting(p, u)
        return out

    def one_draw_tick(self):
        """the tick at which ONE_DRAW's row draws u == 1.0 (2), or None"""
        return 2 if self.has_one_draw() else None


class Coverage:
    def __init__(self, case):
        self.case = case
        self.restarts, self.restart_ticks, self.terminal = 0, set(), 0
        self.actions = np.zeros(case.A or 1, np.int64)
        self.pool_rows, self.residues, self.wrapped = set(), set(), 0
        self.finished_in_launch = []

    def line(self):
        c = self.case
        shares = "-" if c.cont else np.round(self.actions / max(1, self.actions.sum()), 3).tolist()
        one = "" if c.cont else (", u == 1.0 drawn" if c.has_one_draw() else ", no u == 1.0 draw (row or launch too small)")
        return (f"{self.restarts} restarts on ticks {sorted(self.restart_ticks)} ({self.terminal} terminal), action "
                f"shares {shares}, pool rows drawn {len(self.pool_rows)} of {c.pool}, start residues "
                f"{sorted(self.residues)}, {self.wrapped} replicas cross 2^32{one}")


def simulate(case):
    """the whole case on the host alone -> Coverage"""
    from warp_drive_amd.envs.classic_control import apply_done

    E, T = case.E, case.T
    env_obj = make_env(case.env, T, case.pool, case.physics)
    start = np.asarray(env_obj.get_data_dictionary()["state"]["data"], F32).reshape(-1)
    pool_states = None
    if case.pool:
        pool_states = np.asarray(env_obj.get_reset_pool_dictionary()["state_reset_pool"]["data"], F32)[:, 0]
    step = numpy_step(case.env, case.physics)
    state, ts = case.start_states(), case.start_timesteps().astype(np.int64)
    epochs, pool_epochs = case.start_epochs(), case.start_pool_epochs()
    k0, k1 = seed_words(SAMPLER_SEED)
    p0, p1 = seed_words(POOL_SEED)
    cov = Coverage(case)
    acts = None if case.cont else case.actions()
    means, ou = (case.probabilities(), np.zeros(E, F32)) if case.cont else (None, None)
    rows = np.arange(E, dtype=np.uint32)
    for launch in range(case.launches):
        ep0 = epochs + np.uint32(launch * case.ticks)
        cov.residues.update(int(r) for r in np.unique(ep0 & np.uint32(3)))
        cov.wrapped += int((ep0.astype(np.uint64) + np.uint64(case.ticks) > np.uint64(1 << 32)).sum())
        finished = np.zeros(E, bool)
        for k in range(case.ticks):
            if case.cont:
                u1, u2 = ou_uniforms(rows, ep0 + np.uint32(k), k0, k1, TICK_TAG)
                ou, a = ou_step_f32(ou, means, u1, u2, *OU_PARAMS)
            else:
                a = acts[launch * case.ticks + k]
                cov.actions += np.bincount(a, minlength=case.A)
            state, _, _, term = step(state, a)
            ts += 1
            done = apply_done(term, ts, T)
            fin = np.flatnonzero(done > 0)
            if len(fin):
                cov.restart_ticks.add(k)
            cov.restarts += len(fin)
            cov.terminal += int(((done > 0) & (ts < T)).sum())
            finished[fin] = True
            ts[fin] = 0
            if case.pool:
                pick = pool_pick(fin, pool_epochs[fin], p0, p1, case.pool)
                cov.pool_rows.update(int(r) for r in pick)
                state[fin] = pool_states[pick]
                pool_epochs[fin] += np.uint32(1)
            else:
                state[fin] = start
        cov.finished_in_launch.append(finished)
    return cov


def _tick_cases(env):
    C = lambda name, **kw: TickCase(name, env, **kw)
    cont = env not in DISCRETE
    pooled = env != "cartpole"   # Cartpole's fused tick has no pool (its pooled rollout is the unfused plan)
    out = [
        # start epochs: launches of 5 and of 7 ticks start at every residue mod 4; the wrap rows cross 2^32
        C("epochs-5", T=4, ticks=5, launches=4, rows=5, pool=7 if pooled else 0),
        C("epochs-7", T=6, ticks=7, launches=4, pool=7 if pooled else 0, E=1501),
        # launch length: restarts inside a launch; every launch ends on the restart; one tick at an odd epoch
        C("long-launch", T=4, ticks=11, rows=14, E=1601),
        C("long-launch-unrecorded", T=4, ticks=11),
        C("ends-on-restart", T=6, ticks=6, rows=6, timesteps="mostly-zero", epochs="zero"),
        C("one-tick", T=3, ticks=1, launches=7, epochs="odd", rows=1),
        # sizes: one replica, a partial wavefront, one replica into the second wavefront
        C("E1", E=1, T=3, ticks=7, rows=10), C("E63", E=63, T=4, ticks=9), C("E65", E=65, T=4, ticks=9, rows=9),
    ]
    if pooled:
        out += [C(f"pool{n}-{'recorded' if rows else 'unrecorded'}", T=4, ticks=11, rows=rows, pool=n)
                for n, rows in ((2, 14), (7, None), (16, 14), (2, None))]
        out += [C("no-pool-recorded", T=5, ticks=11, rows=14)]
    if env in OTHER_PHYSICS:
        out += [C("other-physics", T=9, ticks=11, rows=11, physics=OTHER_PHYSICS[env], pool=7)]
    counts = {"mountain_car": (1, 2, 5, 8), "acrobot": (1, 2), "cartpole": (1, 2, 3, 8, 9, 12)}.get(env, ())
    for A in counts:
        # (Dirichlet rows at A = 12: the rarest action's share on the host replay is 0.07 -- the bar stays 0.02)
        out += [C(f"A{A}-recorded", A=A, T=4, ticks=11, rows=14, pool=7 if pooled else 0)]
        if env == "cartpole":
            out += [C(f"A{A}-unrecorded", A=A, T=4, ticks=11)]
    if env == "cartpole":
        # (episodes of 30 ticks: in every launch some replicas finish and some do not)
        out += [C("third-array-recorded", T=30, ticks=11, rows=14, extra="third", E=1601),
                C("third-array-unrecorded", T=30, ticks=11, extra="third")]
    return out


TICK_CASES = [c for env in ENVS for c in _tick_cases(env)]
# action counts the host refuses (asserted refused, never launched)
REFUSED_ACTION_COUNTS = {"mountain_car": (0, 9), "acrobot": (0, 9)}


# --------------------------------------------------------------------------------------------------- rollout cases
NEAR_WINDOW = 2e-6   # the project's window around a threshold inside which the device's expf may decide otherwise
HEAD_SCALE = 6.0     # as tests/classic_control_policy.py: decisive enough that the actions occur with varied shares


class RolloutCase(TickCase):
    """...EnvRollout_H<hidden> with A actions: the policy FullyConnected(O, [A], [hidden, hidden]) under
    torch.manual_seed(5), the head's weights times HEAD_SCALE, packed by pack_rollout_policy"""

    def __init__(self, env, hidden, A):
        # (E = 1501, not 700: the grid of 3 blocks of 128 threads must take three trips)
        super().__init__(f"rollout-H{hidden}-A{A}", env, E=1501, T=4, ticks=11, launches=3, rows=11,
                         pool=0 if env == "cartpole" else 7, A=A, share=0.02)
        self.hidden = hidden

    def has_one_draw(self):
        return False   # (the probabilities are the network's: no crafted row)

    def policy(self):
        """(model, packed float32 numpy weights)"""
        import torch
        from warp_drive_amd.training.models import FullyConnected
        from warp_drive_amd.training.policy_kernel import pack_rollout_policy

        torch.manual_seed(5)
        model = FullyConnected(OBS_DIM[self.env], [self.A], [self.hidden, self.hidden])
        with torch.no_grad():
            model.policy_head[0].weight.mul_(HEAD_SCALE)
        return model, pack_rollout_policy(model).numpy()

    def near_cap(self):
        draws = self.E * self.ticks * self.launches
        return (2 + draws // 50000) * (self.A - 1)


ROLLOUT_ACTIONS = {"mountain_car": (1, 2, 8), "acrobot": (1, 2), "cartpole": (1, 3, 8)}
ROLLOUT_CASES = [RolloutCase(env, H, A) for env in DISCRETE for H in (32, 64) for A in ROLLOUT_ACTIONS[env]]
ROLLOUT_GEOMETRIES = ((64, None), (128, 3), (64, "idle"))


def rollout_probabilities(case, packed, obs):
    from tests.classic_control_policy import policy_probabilities

    return policy_probabilities(packed, case.hidden, obs, case.A)


def near_threshold(cum, u, window=NEAR_WINDOW):
    """rows whose uniform lies within `window` of one of the A - 1 thresholds (host sums and uniforms alone)"""
    cum = np.asarray(cum, F32)
    if cum.shape[1] < 2:
        return np.zeros(len(cum), bool)
    return (np.abs(cum[:, :-1].astype(np.float64) - np.asarray(u, np.float64)[:, None]) < window).any(axis=1)


def host_obs(env, state):
    from warp_drive_amd.envs import classic_control as cc

    return cc.acrobot_obs(state) if env == "acrobot" else np.asarray(state, F32).copy()


def simulate_rollout(case, packed=None):
    """the rollout on the host alone (numpy step, the restated network on `packed`, default the case's own policy, the
    Philox replay) -> (Coverage, near draws)"""
    from tests.classic_control_policy import count_below, running_sums
    from warp_drive_amd.envs.classic_control import apply_done

    E, T = case.E, case.T
    env_obj = make_env(case.env, T, case.pool)
    start = np.asarray(env_obj.get_data_dictionary()["state"]["data"], F32).reshape(-1)
    pool_states = None
    if case.pool:
        pool_states = np.asarray(env_obj.get_reset_pool_dictionary()["state_reset_pool"]["data"], F32)[:, 0]
    obs0 = host_obs(case.env, start[None])[0]
    step = numpy_step(case.env)
    if packed is None:
        _, packed = case.policy()
    state, ts = case.start_states(), case.start_timesteps().astype(np.int64)
    obs = np.broadcast_to(obs0, (E, len(obs0))).astype(F32).copy()   # (the device's observation rows before tick 0)
    if case.env == "cartpole":   # (Cartpole's observation is its state)
        obs = state.copy()
    epochs, pool_epochs = case.start_epochs(), case.start_pool_epochs()
    k0, k1 = seed_words(SAMPLER_SEED)
    p0, p1 = seed_words(POOL_SEED)
    cov, near = Coverage(case), 0
    for launch in range(case.launches):
        ep0 = epochs + np.uint32(launch * case.ticks)
        cov.residues.update(int(r) for r in np.unique(ep0 & np.uint32(3)))
        cov.wrapped += int((ep0.astype(np.uint64) + np.uint64(case.ticks) > np.uint64(1 << 32)).sum())
        for k in range(case.ticks):
            u = single_head_tick_uniform(E, ep0 + np.uint32(k), k0, k1, TICK_TAG)
            cum = running_sums(rollout_probabilities(case, packed, obs))
            near += int(near_threshold(cum, u).sum())
            a = count_below(cum, u)
            cov.actions += np.bincount(a, minlength=case.A)
            state, obs, _, term = step(state, a)
            ts += 1
            done = apply_done(term, ts, T)
            fin = np.flatnonzero(done > 0)
            if len(fin):
                cov.restart_ticks.add(k)
            cov.restarts += len(fin)
            ts[fin] = 0
            obs[fin] = obs0
            if case.pool:
                pick = pool_pick(fin, pool_epochs[fin], p0, p1, case.pool)
                cov.pool_rows.update(int(r) for r in pick)
                state[fin] = pool_states[pick]
                pool_epochs[fin] += np.uint32(1)
            else:
                state[fin] = start
    return cov, near
