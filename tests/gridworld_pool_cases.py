"""Cases and a numpy model for the TagGridWorld rollout with a reset pool in one launch: HipTagGridWorldRollout_N5P /
_N5P_H<32|64> and HipTagGridWorldEvaluate_N5P_H<32|64> (csrc/kernels/tag_gridworld_n5_pool.hip, the pooled variant of tag_gridworld_n5_common.h).  Shared by
tests/test_gridworld_pool_rollout_host.py (the model against single oracle ticks; every GPU case sized from the model
alone) and tests/test_gpu_gridworld_pool_rollout.py (the same cases on the device).  Nothing here touches a GPU.

The model of a T-tick launch (`PoolModel.launch`) combines, per tick: the oracle's observation rows (recorded), the
action (the counting draw on the tick's Philox uniform, or whatever `choose` returns), TagGridWorldOracle.step, the
pool row `pool_pick` names from the pool epoch words the model advances itself (+1 on a restart only), and
`reset_done_envs(x=, y=)` -- positions from the pool row, observation rows from the placeholder of the START positions,
time step 0.  After the launch: the sampler words += T, `_done_` / rewards / actions are the last tick's."""
import numpy as np

from oracle.core_np import pool_pick, sample_actions_counting, seed_words, single_head_tick_uniform
from oracle.tag_gridworld_np import TagGridWorldOracle, running_sums
from tests import gridworld_cases as gc
from tests import gridworld_evaluate as gev

F32 = np.float32
N, F, A, EPB = 5, 21, 5, 12
SAMPLER_SEED, POOL_SEED, ENV_SEED = gc.SAMPLER_SEED, 17, 27
TICK_TAG = gc.TICK_TAG
REWARDS = dict(zip(("wall_hit_penalty", "tag_reward_for_tagger", "tag_penalty_for_runner", "step_cost_for_tagger"),
                   gc.REWARD_SETS["thirds"]))
NEAR_WINDOW = 2e-6   # tests/test_gpu_gridworld_shapes.py's rule for the live-policy entries


class PoolCase:
    """E replicas on a grid of side L + 1, episodes of `T` ticks, `launches` launches of `ticks` ticks, a pool of
    `n_pool` rows; starts "default" (taggers in the centre, the runner in the corner) or "boundary" (taggers ON
    coordinate L: a tick that keeps them there reads the last used entry of the quotient table)"""

    def __init__(self, name, E, L, T, ticks, n_pool=5, launches=1, starts="default", seed=0):
        self.name, self.E, self.L, self.T, self.ticks = name, int(E), int(L), int(T), int(ticks)
        self.n_pool, self.launches, self.starts, self.seed = int(n_pool), int(launches), starts, int(seed)

    def __repr__(self):
        return self.name

    def config(self):
        cfg = dict(num_taggers=N - 1, grid_length=self.L, episode_length=self.T, use_full_observation=True, **REWARDS)
        if self.starts == "boundary":
            L = self.L
            cfg["starting_location_x"] = np.array([L, L, L - 1, L, 0], np.int32)
            cfg["starting_location_y"] = np.array([L, L - 1, L, 0, 0], np.int32)
        return cfg

    def env(self):
        """the env object (host side only: no device is touched before an EnvWrapper takes it)"""
        from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorldWithResetPool

        env = CUDATagGridWorldWithResetPool(seed=ENV_SEED, **self.config())
        env.POOL_SIZE = self.n_pool
        return env

    def pools(self):
        """(pool_x, pool_y) int32 [n_pool, 5] as the env draws them from its seed"""
        feed = self.env().get_reset_pool_dictionary()
        return (np.asarray(feed["loc_x_reset_pool"]["data"], np.int32), np.asarray(feed["loc_y_reset_pool"]["data"], np.int32))

    def probabilities(self):
        """float32 [E, 5, 5]: seeded Dirichlet rows, different for every replica and agent, none uniform"""
        return np.random.RandomState(2000 + self.seed).dirichlet(np.ones(A), size=(self.E, N)).astype(F32)

    def start_epochs(self):
        """sampler epoch word per agent row, different from row to row"""
        rows = np.arange(self.E * N, dtype=np.uint64)
        return (((rows * np.uint64(2654435761)) >> np.uint64(9)) & np.uint64(0xFFF)).astype(np.uint32)

    def start_pool_epochs(self):
        """pool epoch word per replica, different from replica to replica"""
        envs = np.arange(self.E, dtype=np.uint64)
        return (((envs * np.uint64(2246822519)) >> np.uint64(11)) & np.uint64(0xFF)).astype(np.uint32)


SMALL_CASES = [PoolCase(f"pool_E{E}", E, 7, 3, 10, seed=E) for E in (1, 11, 12, 13, 25)]
BOUNDARY_CASES = [PoolCase(f"pool_boundary_L{L}", 25, L, 6, 14, launches=2, starts="boundary", seed=L) for L in (100, 255)]
POOL_SIZE_CASES = [PoolCase(f"pool_rows{n}", 25, 7, 3, 10, n_pool=n, seed=40 + n) for n in (2, 5, 7, 64)]
TAG_CASE = PoolCase("pool_tags_L2", 25, 2, 20, 30, seed=77)
FIXED_CASES = SMALL_CASES + BOUNDARY_CASES + POOL_SIZE_CASES + [TAG_CASE]
POLICY_CASES = SMALL_CASES + BOUNDARY_CASES + POOL_SIZE_CASES   # "the first three case families"


class PoolModel:
    def __init__(self, case, pool_x=None, pool_y=None, epochs=None, pool_epochs=None):
        self.case = case
        self.orc = TagGridWorldOracle(num_envs=case.E, **case.config())
        px, py = case.pools() if pool_x is None else (pool_x, pool_y)
        self.pool_x, self.pool_y = np.asarray(px, np.int32), np.asarray(py, np.int32)
        self.epochs = (case.start_epochs() if epochs is None else np.asarray(epochs, np.uint32)).copy()
        self.pool_epochs = (case.start_pool_epochs() if pool_epochs is None else np.asarray(pool_epochs, np.uint32)).copy()
        self.k, self.pk = seed_words(SAMPLER_SEED), seed_words(POOL_SEED)
        self.restarts = np.zeros(case.E, np.int64)
        self.tags = self.timeouts = 0
        self.rows_drawn = set()
        self.max_coord = 0
        self.last = None

    def uniforms(self, k):
        E = self.case.E
        return single_head_tick_uniform(E * N, self.epochs + np.uint32(k), self.k[0], self.k[1], TICK_TAG).reshape(E, N)

    def launch(self, T, probs=None, choose=None):
        """T ticks -> {"obs" [T, E, 5, 21], "actions" [T, E, 5], "rewards" [T, E, 5], "done" [T, E]} (what the launch
        records).  probs: float32 [E, 5, 5] for the counting draw; or choose(k, obs float32, u) -> int actions [E, 5]"""
        case, orc, E = self.case, self.orc, self.case.E
        rec = {"obs": [], "actions": [], "rewards": [], "done": []}
        envs = np.arange(E)
        for k in range(T):
            obs = orc.obs.astype(F32)
            u = self.uniforms(k)
            a = sample_actions_counting(probs, u) if choose is None else np.asarray(choose(k, obs, u), np.int32)
            orc.step(a)
            self.max_coord = max(self.max_coord, int(orc.loc_x.max()), int(orc.loc_y.max()))
            fin = orc.done > 0
            tagged = ((orc.loc_x[:, :-1] == orc.loc_x[:, -1:]) & (orc.loc_y[:, :-1] == orc.loc_y[:, -1:])).any(axis=1)
            self.tags += int(tagged.sum())
            self.timeouts += int((fin & ~tagged).sum())
            rec["obs"].append(obs)
            rec["actions"].append(a.astype(np.int32))
            rec["rewards"].append(orc.rewards.astype(F32))
            rec["done"].append(orc.done.astype(np.int32).copy())
            self.last = dict(done=orc.done.astype(np.int32).copy(), rewards=orc.rewards.astype(F32), actions=a.astype(np.int32))
            pick = pool_pick(envs, self.pool_epochs, self.pk[0], self.pk[1], self.pool_x.shape[0])
            orc.reset_done_envs(x=self.pool_x[pick], y=self.pool_y[pick])
            self.pool_epochs[fin] += np.uint32(1)
            self.restarts += fin
            self.rows_drawn |= set(pick[fin].tolist())
        self.epochs = (self.epochs + np.uint32(T)).astype(np.uint32)
        return {key: np.stack(v) for key, v in rec.items()}

    def state(self):
        """the arrays after a launch"""
        orc = self.orc
        return dict(loc_x=orc.loc_x.copy(), loc_y=orc.loc_y.copy(), obs=orc.obs.astype(F32), timestep=orc.timestep.copy(),
                    epochs=self.epochs.copy(), pool_epochs=self.pool_epochs.copy(), **self.last)


def coverage_ok(case, model):
    """what the GPU test demands of every case: at least 2 * E restarts (and no replica without one), every pool row
    drawn in the pool-size cases of 2 / 5 / 7 rows, the pool words advanced by the restarts"""
    ok = int(model.restarts.sum()) >= 2 * case.E and bool((model.restarts >= 1).all())
    if case in POOL_SIZE_CASES and case.n_pool in (2, 5, 7):
        ok = ok and model.rows_drawn == set(range(case.n_pool))
    ok = ok and bool((model.pool_epochs - case.start_pool_epochs() == model.restarts.astype(np.uint32)).all())
    if case.starts == "boundary":
        ok = ok and model.max_coord == case.L
    return bool(ok)


def policies(hidden, shared, seed):
    """([models], [packed float32 numpy weights] * 2) for the kernel's (tagger, runner) arguments: one FullyConnected(21,
    [5], [H, H]) passed twice when `shared`, else two; head x 4 / x 7 and first layer x 2 as tests/gridworld_evaluate.py"""
    import torch
    from warp_drive_amd.training.models import FullyConnected
    from warp_drive_amd.training.policy_kernel import pack_gridworld_policy

    torch.manual_seed(seed)
    models = [FullyConnected(F, [A], [hidden, hidden]) for _ in range(1 if shared else 2)]
    with torch.no_grad():
        for m, scale in zip(models, gev.HEAD_SCALE):
            m.policy_head[0].weight.mul_(scale)
            m.fc["0"][0].weight.mul_(gev.FIRST_LAYER_SCALE)
    packed = [pack_gridworld_policy(m).numpy().copy() for m in models]
    return models, (packed * 2 if shared else packed)


class Judge:
    """tests/test_gpu_gridworld_shapes.py's rule for the actions of a live-policy launch: the device's action is the
    counting draw on the float32 restatement of the in-kernel forward, except where the uniform sits within 2e-6 of a
    running sum; the model follows the device's action"""

    def __init__(self, packed, hidden, device_actions):
        self.packed, self.hidden, self.got = packed, hidden, np.asarray(device_actions)
        self.near = self.draws = 0

    def __call__(self, k, obs, u):
        p = gev.probabilities(self.packed, self.hidden, obs)
        cum = running_sums(p.reshape(-1, A)).reshape(-1, N, A)
        want = np.minimum((cum < u[..., None]).sum(axis=-1), A - 1).astype(np.int32)
        got = self.got[k].reshape(want.shape)
        assert ((got >= 0) & (got < A)).all(), k
        bad = got != want
        if bad.any():   # only where the uniform sits on a threshold
            gap = np.abs(cum[bad] - u[bad][:, None]).min(axis=1)
            assert (gap < NEAR_WINDOW).all(), (k, gap.max(), np.argwhere(bad)[:5])
        self.near += int(bad.sum())
        self.draws += want.size
        return got

    def cap(self):
        return 2 + self.draws // 50000


# ------------------------------------------------------------------------------------------------------ evaluation
class PoolEvalCase(gev.GwCase):
    """one episode of every replica at grid_length 100 (tests/gridworld_evaluate.py's replay follows the device's
    trace): the agents of a replica start within a few cells of each other so that tags happen within the episode, every
    fourth replica in the far corner (coordinates up to 100, walls)"""

    # torch.manual_seed of the policies: the first seed from 1 on under which the HOST replay at E = 13 and E = 25 has
    # tags, time-outs, wall hits, an agent on coordinate 100, no decision inside the 2e-6 window and (greedy) three
    # actions with a share of at least 0.05 -- a greedy policy of this size may settle on one move
    SEEDS = {(32, "greedy"): 2, (64, "greedy"): 4, (32, "sampled"): 1, (64, "sampled"): 1}

    def __init__(self, hidden, mode, E, grid_length=100, T=12, seed=None):
        super().__init__(hidden, mode, grid_length=grid_length, T=T, E=E)
        self.seed = self.SEEDS[hidden, mode] if seed is None else seed
        self.name = "pool-" + self.name

    def policies(self, seed=None):
        return gev.GwCase.policies(self, self.seed if seed is None else seed)

    def oracle(self):
        orc = TagGridWorldOracle(num_envs=self.E, **self.env_config())
        rng = np.random.RandomState(gev.START_SEED)
        base = rng.randint(3, self.L - 6, size=(self.E, 1))
        base[np.arange(self.E) % 4 == 3] = self.L - 3
        orc.loc_x = (base + rng.randint(0, 4, size=(self.E, N))).astype(np.int32)
        orc.loc_y = (base + rng.randint(0, 4, size=(self.E, N))).astype(np.int32)
        orc.timestep = (np.arange(self.E) % 4).astype(np.int32)
        orc.obs = orc.generate_observation()
        return orc


def eval_coverage_ok(case, r):
    """what an evaluation case of 13 replicas or more must exercise: tags, time-outs, walls, coordinate L"""
    return bool(r["tagged"].any() and r["timed_out"].any() and r["wall_hits"] > 0 and r["max_coord"] == case.L)


EVAL_CASES = [PoolEvalCase(32, mode, E) for mode in gev.MODES for E in (1, 13, 25)] + \
             [PoolEvalCase(64, mode, 25) for mode in gev.MODES]
