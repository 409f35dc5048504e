"""Cases and a numpy model for the Cartpole rollout with a reset pool in one launch: HipClassicControlCartPoleEnvRollout_P /
_P_H<32|64> (csrc/kernels/cartpole_pool.hip).  Shared by tests/test_cartpole_pool_rollout_host.py (every case is replayed
on the host alone and must reach the coverage it is there for) and tests/test_gpu_cartpole_pool_rollout.py (the same cases
on the device, both pool placements).  Nothing here touches a GPU.

The model of a T-tick launch (`PoolModel.launch`) combines, per tick: the observation rows (recorded), the action (the
counting draw on the tick's Philox uniform, or whatever `choose` returns), oracle/cartpole_np.py's step, and for a finished
replica the pool row `oracle.core_np.pool_pick` names from the pool epoch words the model advances itself (+1 on a restart
only) as its STATE, its SAVED observation row as its observation, time step 0.  The saved observation rows differ from
replica to replica (the pooled env's reset draws: training/data_loader.py stacks one host reset per replica); the device
test writes `saved_observations()` and `pool_rows()` into the device's arrays, so host and device replay the same case."""
import numpy as np

from oracle.cartpole_np import CartPoleOracle
from oracle.core_np import pool_pick, sample_actions_counting, seed_words, single_head_tick_uniform
from tests import classic_control_cases as cc

F32 = np.float32
SAMPLER_SEED, POOL_SEED, TICK_TAG = cc.SAMPLER_SEED, cc.POOL_SEED, cc.TICK_TAG
HIDDEN = (0, 32, 64)   # 0: the fixed-probability entry
ENTRY = {0: "HipClassicControlCartPoleEnvRollout_P", 32: "HipClassicControlCartPoleEnvRollout_P_H32",
         64: "HipClassicControlCartPoleEnvRollout_P_H64"}
OBJECT = "wd_kernels_cp_pool.hsaco"

# pool rows no fast tick may see.  The first three restart straight into a terminal tick (an angle of 1.0 with no angular
# velocity, a cart beyond x_threshold): the next step ends the episode whatever its sine and cosine were.  The last two hold
# |theta| = 1.0 with an angular velocity that brings the pole back inside the threshold within ONE step (1.0 - 45 * 0.02 =
# 0.1): the replica goes on, and the velocities the next observation row records were computed from sin / cos of 1.0 --
# the small-angle polynomials give other bits there (tests/test_cartpole_pool_rollout_host.py asserts that they do).
CRAFTED_ROWS = np.array([[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, -1.0, 0.0], [3.0, 0.0, 0.0, 0.0],
                         [0.0, 0.0, 1.0, -45.0], [0.01, 0.0, -1.0, 45.0]], F32)


class PoolCase(cc.RolloutCase):
    """`hidden` 0: fixed probabilities (TickCase's crafted rows, the draw of exactly 1.0 included); 32 / 64: the policy
    FullyConnected(4, [A], [hidden, hidden]) under torch.manual_seed(seed), the head's weights times HEAD_SCALE.
    crafted: the first rows of the pool are CRAFTED_ROWS."""

    def __init__(self, name, hidden, A=2, pool=7, E=1501, T=4, ticks=11, rows=11, crafted=False, seed=5, share=0.02):
        cc.TickCase.__init__(self, name, "cartpole", E=E, T=T, ticks=ticks, launches=3, rows=rows, pool=pool, A=A,
                             epochs="residue", timesteps="spread", share=share)
        self.hidden, self.crafted, self.seed = int(hidden), bool(crafted), int(seed)
        self.name = f"cartpole-pool-H{hidden}-{name}"
        assert pool >= 2 and (not crafted or pool > len(CRAFTED_ROWS))

    def has_one_draw(self):
        return self.hidden == 0 and cc.TickCase.has_one_draw(self)

    def policy(self):
        """(model, packed float32 numpy weights)"""
        import torch
        from warp_drive_amd.training.models import FullyConnected
        from warp_drive_amd.training.policy_kernel import pack_rollout_policy

        torch.manual_seed(self.seed)
        model = FullyConnected(4, [self.A], [self.hidden, self.hidden])
        with torch.no_grad():
            model.policy_head[0].weight.mul_(cc.HEAD_SCALE)
        return model, pack_rollout_policy(model).numpy()

    def pool_rows(self):
        """float32 [pool, 4]: start states as the env draws them (+-0.05), the crafted rows first when asked for"""
        rows = np.random.RandomState(100 + self.pool).uniform(-0.05, 0.05, size=(self.pool, 4)).astype(F32)
        if self.crafted:
            rows[:len(CRAFTED_ROWS)] = CRAFTED_ROWS
        return rows

    def saved_observations(self):
        """float32 [E, 4]: the saved copy of the observation rows, different for every replica"""
        return np.random.RandomState(200).uniform(-0.05, 0.05, size=(self.E, 4)).astype(F32)


def _cases(H):
    C = lambda name, **kw: PoolCase(name, H, **kw)   # noqa: E731
    return ([C(f"A{A}", A=A, rows=14 if A == 2 else 11) for A in (1, 2, 3, 8)] +
            [C("pool2", pool=2, rows=14), C("pool16", pool=16)] +
            [C(f"E{E}", E=E) for E in (1, 63, 65)] +
            # episodes of 30 ticks: in every launch some replicas finish and some do not
            [C("T30", T=30, rows=14),
             C("crafted-pool", crafted=True, pool=9), C("ordinary-pool", pool=9)])


CASES = [c for H in HIDDEN for c in _cases(H)]
GEOMETRIES = cc.ROLLOUT_GEOMETRIES
PLACEMENTS = ("lds", "global")


class PoolModel:
    def __init__(self, case, pool_rows=None, saved_observations=None):
        self.case = case
        E = case.E
        self.pool = np.asarray(case.pool_rows() if pool_rows is None else pool_rows, F32)
        self.obs0 = np.asarray(case.saved_observations() if saved_observations is None else saved_observations, F32)
        assert self.pool.shape == (case.pool, 4) and self.obs0.shape == (E, 4)
        self.orc = CartPoleOracle(E, case.T)
        self.orc.state = case.start_states().copy()
        self.orc.obs = self.orc.state.copy()          # (the device test writes the state into the observation rows)
        self.orc.timestep = case.start_timesteps().astype(np.int32).copy()
        self.epochs, self.pool_epochs = case.start_epochs().copy(), case.start_pool_epochs().copy()
        self.k, self.pk = seed_words(SAMPLER_SEED), seed_words(POOL_SEED)
        self.last = None
        # coverage
        self.restarts = np.zeros(E, np.int64)
        self.restart_ticks, self.rows_drawn = [], set()
        self.actions = np.zeros(case.A, np.int64)
        self.finished_in_launch = []
        self.wrapped = self.pool_wrapped = self.terminal = 0
        self.crafted_survivors = 0   # restarts from a crafted row that the NEXT tick did not end

    def uniforms(self, k):
        return single_head_tick_uniform(self.case.E, self.epochs + np.uint32(k), self.k[0], self.k[1], TICK_TAG)

    def launch(self, choose):
        """case.ticks ticks -> the rows the launch records {"obs" [T, E, 4], "actions", "rewards", "done" [T, E]};
        choose(k, obs float32 [E, 4], u float32 [E]) -> int actions [E]"""
        case, orc, E = self.case, self.orc, self.case.E
        rec = {"obs": [], "actions": [], "rewards": [], "done": []}
        self.wrapped += int((self.epochs.astype(np.uint64) + np.uint64(case.ticks) > np.uint64(1 << 32)).sum())
        ticks_with_restart, finished = set(), np.zeros(E, bool)
        from_crafted = np.zeros(E, bool)
        for k in range(case.ticks):
            obs = orc.obs.copy()
            a = np.asarray(choose(k, obs, self.uniforms(k)), np.int32)
            self.actions += np.bincount(a, minlength=case.A)
            orc.done = np.zeros(E, np.int32)
            orc.step(a)
            done = orc.done.astype(np.int32).copy()
            fin = done > 0
            self.crafted_survivors += int((from_crafted & ~fin).sum())
            rec["obs"].append(obs), rec["actions"].append(a), rec["rewards"].append(orc.rewards.astype(F32).copy())
            rec["done"].append(done)
            self.last = dict(done=done, rewards=orc.rewards.astype(F32).copy(), actions=a.copy())
            self.terminal += int((fin & (orc.timestep < case.T)).sum())
            rows = np.flatnonzero(fin)
            pick = pool_pick(rows, self.pool_epochs[rows], self.pk[0], self.pk[1], case.pool)
            orc.state[rows] = self.pool[pick]
            orc.obs[rows] = self.obs0[rows]
            orc.timestep[rows] = 0
            before = self.pool_epochs[rows].astype(np.uint64)
            self.pool_epochs[rows] += np.uint32(1)
            self.pool_wrapped += int((before + np.uint64(1) > np.uint64(0xFFFFFFFF)).sum())
            from_crafted = np.zeros(E, bool)
            if case.crafted:
                from_crafted[rows] = pick >= 3   # (rows 3 and 4 of CRAFTED_ROWS are the survivors)
                from_crafted[rows] &= pick < len(CRAFTED_ROWS)
            self.restarts += fin
            self.rows_drawn |= set(int(p) for p in pick)
            finished |= fin
            if fin.any():
                ticks_with_restart.add(k)
        self.restart_ticks.append(sorted(ticks_with_restart))
        self.finished_in_launch.append(finished)
        self.epochs = (self.epochs + np.uint32(case.ticks)).astype(np.uint32)
        return {key: np.stack(v) for key, v in rec.items()}

    def state(self):
        """the arrays after a launch"""
        orc = self.orc
        return dict(state=orc.state.copy(), obs=orc.obs.copy(), timestep=orc.timestep.astype(np.int32).copy(),
                    epochs=self.epochs.copy(), pool_epochs=self.pool_epochs.copy(), **self.last)


class HostChoice:
    """the action of a tick on the host alone: the counting draw on the fixed probabilities, or on the float32 restatement
    of the in-kernel network; counts the draws within NEAR_WINDOW of a threshold"""

    def __init__(self, case, packed=None):
        self.case, self.near = case, 0
        self.packed = (case.policy()[1] if packed is None else packed) if case.hidden else None
        self.probs = None if case.hidden else case.probabilities()

    def cum(self, obs):
        from tests.classic_control_policy import running_sums

        return running_sums(cc.rollout_probabilities(self.case, self.packed, obs))

    def __call__(self, k, obs, u):
        from tests.classic_control_policy import count_below

        if not self.case.hidden:
            return sample_actions_counting(self.probs, u)
        cum = self.cum(obs)
        self.near += int(cc.near_threshold(cum, u).sum())
        return count_below(cum, u)


class FollowDevice(HostChoice):
    """tests/test_gpu_classic_control_shapes.py's rule for the live-policy entries: the device's recorded action must be
    the host's counting draw except where the uniform lies within NEAR_WINDOW of a threshold (that set comes from the
    host's sums and uniforms alone); the model follows the device's action.  Fixed probabilities: no exception."""

    def __init__(self, case, device_actions, packed=None):
        super().__init__(case, packed)
        self.got, self.differ = np.asarray(device_actions), 0

    def __call__(self, k, obs, u):
        from tests.classic_control_policy import count_below

        got = self.got[k]
        assert got.min() >= 0 and got.max() <= self.case.A - 1, k
        if not self.case.hidden:
            want = sample_actions_counting(self.probs, u)
            np.testing.assert_array_equal(got, want, err_msg=f"tick {k}")
            return got
        cum = self.cum(obs)
        near = cc.near_threshold(cum, u)
        bad = got != count_below(cum, u)
        assert not (bad & ~near).any(), (k, cum[bad & ~near], u[bad & ~near], got[bad & ~near])
        self.near, self.differ = self.near + int(near.sum()), self.differ + int(bad.sum())
        return got


def sincos_small(x):
    """csrc/kernels/cartpole_common.h::cp_sincos_small in float32 numpy (each fused multiply-add in float64, rounded once)"""
    fma = lambda a, b, c: (np.float64(a) * np.float64(b) + np.float64(c)).astype(F32)   # noqa: E731
    x = np.asarray(x, F32)
    r2 = (x * x).astype(F32)
    c = fma(F32(float.fromhex("0x1.98e616p-16")), r2, F32(float.fromhex("-0x1.6c06dcp-10")))
    c = fma(c, r2, F32(float.fromhex("0x1.55553cp-05")))
    c = fma(c, r2, F32(-0.5))
    c = fma(c, r2, F32(1.0))
    s = fma(F32(float.fromhex("0x1.7d3bbcp-19")), r2, F32(float.fromhex("-0x1.a06bbap-13")))
    s = fma(s, r2, F32(float.fromhex("0x1.11119ap-07")))
    s = fma(s, r2, F32(float.fromhex("-0x1.555556p-03")))
    s = fma(s, r2, F32(0.0))
    s = fma(s, x, x)
    return s, c
