"""The one-launch evaluation of a custom environment (include/wd_env_evaluate.h), restated on the host: the numpy model of
the network and the Philox replay of tests/custom_rollout_model.py, the greedy rule and the near-tie windows of
tests/classic_control_evaluate.py and tests/classic_control_cases.py (all by import), the envs' own host steps, and the
cases the CPU and the GPU tests share.  Nothing here touches a GPU.

A case is ONE launch: every replica runs one episode from its own start, up to its first done or `ticks` ticks.  It is
judged TICK BY TICK: the host replicas give the observation, the model gives the expected action -- the first maximum
of the probabilities (greedy) or the number of running sums below the replayed uniform (sampled) -- and the host step is
then fed the RECORDED action, so one flagged decision does not spread.  A decision is flagged only by `near_top_two`
(greedy) or `near_threshold` (sampled), computed from host values.

The Rendezvous replicas of a case do not start alike: the class draws ONE set of starting cells for all replicas, under
which every replica of a greedy evaluation would walk the same path.  Replica e starts from cells of its own (`start_cells`;
the device arrays are overwritten behind `reset_all_envs()`, the reset copies are not), so replicas finish at different
ticks in both modes -- and the end state, which must equal the reset copies, differs from every start.

"Every action occurs" is asked of a sampled case with at least 50 decisions per action on its own, and of the cases of one
kind and action count TOGETHER otherwise: a greedy evaluation of the probe sees 2 L distinct observation rows, fewer than
eight actions' worth, and the smallest Rendezvous case makes three decisions."""
import os

import numpy as np

from tests import custom_rollout_model as rollout_model
from tests.classic_control_cases import NEAR_WINDOW, near_threshold
from tests.classic_control_evaluate import first_maximum, near_top_two
from tests.classic_control_policy import count_below, policy_probabilities, running_sums
from tests.custom_rollout_model import HostReplicas, make_policy, near_cap, policy_floats, replayed_uniform

f32 = np.float32
ROOT = rollout_model.ROOT
EXAMPLE_DIR = os.path.join(ROOT, "examples", "rendezvous_evaluate")
EXAMPLE_SOURCE = os.path.join(EXAMPLE_DIR, "rendezvous_evaluate.hip")
PROBE_SOURCE = os.path.join(ROOT, "tests", "custom_envs", "evaluate_probe.hip")
HEADER = os.path.join(ROOT, "include", "wd_env_evaluate.h")
TICK_TAG = rollout_model.TICK_TAG
WIDTHS = rollout_model.WIDTHS
MODES = ("greedy", "sampled")
EXAMPLE_KERNELS = sorted(
    ["HipRendezvousEvaluateStep", "HipRendezvousEvaluateTick"]
    + [f"HipRendezvousEvaluate{kind}_H{H}" for kind in ("Rollout", "Evaluate", "PgValues", "PgGradients") for H in WIDTHS]
    + ["HipRendezvousEvaluatePgReduce", "HipRendezvousEvaluatePgApply"])
PROBE_KERNELS = sorted(["HipEvaluateProbeStep", "HipEvaluateProbeTick"]
                       + [f"HipEvaluateProbe{kind}_H{H}" for kind in ("Rollout", "Evaluate") for H in WIDTHS])

__all__ = ["NEAR_WINDOW", "near_threshold", "near_top_two", "first_maximum", "count_below", "policy_probabilities",
           "running_sums", "near_cap", "policy_floats", "replayed_uniform", "make_policy"]


def example_module():
    """examples/rendezvous_evaluate/rendezvous_evaluate.py, imported by path (the examples are not a package)"""
    import importlib.util
    import sys

    name = "rendezvous_evaluate_example"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(EXAMPLE_DIR, "rendezvous_evaluate.py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


def uniforms_at(seed, rows, epochs):
    """the uniform agent row rows[i] draws at epoch epochs[i] (mod 2^32) under sampler seed `seed`: float32 [len(rows)]"""
    from tests import custom_tick_model as tick_model

    k0, k1 = tick_model.seed_words(seed)
    e = (np.asarray(epochs, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    bits = tick_model.tick_bits(np.asarray(rows, dtype=np.uint32), e, k0, k1, TICK_TAG)
    return tick_model.uniform_of(bits[:, 0])


# ---------------------------------------------------------------------------------------------------- host replicas
class EpisodeReplicas(HostReplicas):
    """E host envs that run ONE episode each: a replica that has finished is stepped no more.  `total` [E, N] float32: the
    rewards added in tick order; `steps`, `done` [E]; `running` [E] bool.  `first`: the observation a restore leaves."""

    def __init__(self, cls, config, num_envs, cells=None):
        super().__init__(cls, config, num_envs)
        if cells is not None:
            for e, env in enumerate(self.envs):
                env.set_cells(cells[0][e], cells[1][e])
                self.obs[e] = self._rows(env._observation())
        self.running = np.ones(num_envs, dtype=bool)
        self.total = np.zeros((num_envs, self.N), dtype=f32)
        self.steps = np.zeros(num_envs, dtype=np.int32)
        self.done = np.zeros(num_envs, dtype=np.int32)
        self.last_rewards = np.zeros((num_envs, self.N), dtype=f32)

    def step(self, actions):
        """actions [E, N]: the running replicas take one tick"""
        for e, env in enumerate(self.envs):
            if not self.running[e]:
                continue
            obs, rew, d, _ = env.step({a: int(actions[e, a]) for a in range(self.N)})
            self.obs[e] = self._rows(obs)
            self.last_rewards[e] = [rew[a] for a in range(self.N)]
            self.total[e] = (self.total[e] + self.last_rewards[e]).astype(f32)
            self.steps[e] += 1
            if d["__all__"]:
                self.done[e], self.running[e] = 1, False
                self.early += env.timestep < env.episode_length
                self.timed += env.timestep == env.episode_length


# ------------------------------------------------------------------------------------------------------------ cases
class Case:
    """One evaluation: kind "rendezvous" -- the worked example (F = 5, A = 5), shape (E, N, L, T) = replicas, agents, grid
    length, episode length -- or "probe" -- tests/custom_envs/evaluate_probe.py (F = 2, A chosen), episodes of L ticks; one
    launch of `ticks` ticks (default: T; the probe's T = L + 1 is LONGER than its episode: the launch stops at the first
    done).  `seed`: the sampler's; `policy_seed`: torch's for the network; both chosen (on the host alone, SEEDS) so that
    the modelled run meets test_custom_env_evaluate_build.py's conditions."""

    def __init__(self, kind, E, N, L, T, hidden, A=5, mode="greedy", ticks=None):
        assert mode in MODES
        self.kind, self.E, self.N, self.L, self.T, self.hidden, self.A, self.mode = kind, E, N, L, T, hidden, A, mode
        self.ticks = T if ticks is None else int(ticks)
        self.greedy = mode == "greedy"
        self.F = 5 if kind == "rendezvous" else 2
        self.key = (kind, E, N, L, T, hidden, A)
        self.seed, self.policy_seed = SEEDS.get(self.key, (17, rollout_model.TORCH_SEED))
        self.name = f"{kind}-E{E}-N{N}-L{L}-T{T}-H{hidden}-A{A}-{mode}" + ("" if ticks is None else f"-ticks{ticks}")
        self._config = None

    def __repr__(self):
        return self.name

    def near_cap(self, decisions):
        return near_cap(decisions, self.A)

    def env_class(self):
        if self.kind == "rendezvous":
            return example_module().RendezvousEvaluate
        from tests.custom_envs.evaluate_probe import EvaluateProbe

        return EvaluateProbe

    def source(self):
        return EXAMPLE_SOURCE if self.kind == "rendezvous" else PROBE_SOURCE

    def policy(self):
        return make_policy(self.F, self.A, self.hidden, seed=self.policy_seed)

    def start_cells(self):
        """(x [E, N], y [E, N]) int32: the cells replica e starts from; None for the probe"""
        if self.kind != "rendezvous":
            return None
        rng = np.random.RandomState(7000 + 10 * self.N + self.E)
        return (rng.randint(0, self.L + 1, (self.E, self.N)).astype(np.int32),
                rng.randint(0, self.L + 1, (self.E, self.N)).astype(np.int32))

    def config(self):
        """the env's config; Rendezvous with more than one agent: the spread limit is the median, over the replicas of
        the modelled run of this mode with the limit off, of the smallest largest-spread a replica reaches before its last
        tick -- about half the replicas finish early, the rest at the time limit (a greedy policy gathers the agents far
        sooner than a sampled one: one limit for both modes would end every greedy replica early and no sampled one)"""
        if self._config is None:
            if self.kind == "probe":
                self._config = dict(num_agents=self.N, episode_length=self.L, n_actions=self.A)
            else:
                config = dict(num_agents=self.N, grid_length=self.L, episode_length=self.T, seed=self.N,
                              wall_penalty=0.125, spread_limit=-1)
                if self.N > 1:
                    twin = Case(self.kind, self.E, self.N, self.L, self.T, self.hidden, self.A, self.mode)
                    twin.seed, twin.policy_seed = self.seed, self.policy_seed
                    minima = simulate(twin, config)["maxima"][:max(1, self.T - 1)].min(axis=0)
                    config["spread_limit"] = int(np.floor(np.median(minima)))
                self._config = config
        return dict(self._config)

    def replicas(self, config=None):
        return EpisodeReplicas(self.env_class(), self.config() if config is None else config, self.E, self.start_cells())


def expected_actions(case, packed, obs, tick):
    """obs [E * N, F] -> (expected action [E * N], flagged [E * N]) of tick `tick` of a launch that began at epoch 0"""
    p = policy_probabilities(packed, case.hidden, obs, case.A)
    if case.greedy:
        return first_maximum(p), near_top_two(p)
    cum = running_sums(p)
    u = replayed_uniform(case.seed, case.E * case.N, tick)
    return count_below(cum, u), near_threshold(cum, u)


def simulate(case, config=None):
    """the case on the host alone -> {"actions": counts [A], "early", "timed", "near", "decisions", "steps" [E], "done" [E],
    "total" [E, N], "maxima" [ticks, E] (the largest spread of the tick; the last value where a replica has finished)}"""
    _, packed = case.policy()
    host = case.replicas(config)
    counts, near, decisions, maxima = np.zeros(case.A, dtype=np.int64), 0, 0, []
    for k in range(case.ticks):
        if not host.running.any():
            break
        want, flagged = expected_actions(case, packed, host.obs.reshape(case.E * case.N, case.F), k)
        live = np.repeat(host.running, case.N)
        near += int(flagged[live].sum())
        decisions += int(live.sum())
        counts += np.bincount(want[live], minlength=case.A)
        host.step(want.reshape(case.E, case.N))
        maxima.append(np.array([getattr(env, "last_max_spread", None) or 0 for env in host.envs]))
    return {"actions": counts, "early": int(host.early), "timed": int(host.timed), "near": near, "decisions": decisions,
            "steps": host.steps.copy(), "done": host.done.copy(), "total": host.total.copy(), "maxima": np.array(maxima)}


RENDEZVOUS_SHAPES = rollout_model.RENDEZVOUS_SHAPES   # (1, 1, 4, 3), (3, 5, 4, 4), (7, 64, 6, 5), (7, 70, 6, 9), (2, 130, 8, 6)
WIDE_SHAPE = rollout_model.WIDE_SHAPE                 # (2, 520, 4, 3): served at width 32 only
PROBE_SHAPES = [(A, N) for A in (1, 2, 8) for N in (1, 5, 70)]
# (kind, E, N, L, T, hidden, A) -> (sampler seed, policy seed) where (17, 5) does not meet the conditions of
# tests/test_custom_env_evaluate_build.py::test_the_gpu_cases_cannot_pass_vacuously: the first pair, policy seed first, found
# on the host model alone (policy seeds 5 .. 44, sampler seeds 17 .. 19; a pair is kept when both modes of the shape meet
# the per-case conditions, and preferred when it adds actions the greedy cases of its kind have not shown yet)
SEEDS = {("rendezvous", 1, 1, 4, 3, 32, 5): (18, 9), ("rendezvous", 1, 1, 4, 3, 64, 5): (19, 9),
         ("rendezvous", 3, 5, 4, 4, 32, 5): (17, 6), ("rendezvous", 3, 5, 4, 4, 64, 5): (18, 5),
         ("probe", 3, 1, 4, 5, 32, 2): (17, 12), ("probe", 3, 1, 4, 5, 32, 8): (17, 12),
         ("probe", 3, 5, 4, 5, 64, 8): (17, 10)}

RENDEZVOUS_CASES = [Case("rendezvous", *shape, hidden=H, mode=mode) for shape in RENDEZVOUS_SHAPES for H in WIDTHS
                    for mode in MODES] + [Case("rendezvous", *WIDE_SHAPE, hidden=32, mode=mode) for mode in MODES]
PROBE_CASES = [Case("probe", 3, N, 4, 5, hidden=H, A=A, mode=mode) for A, N in PROBE_SHAPES for H in WIDTHS for mode in MODES]
SHORT_CASES = [Case("rendezvous", 3, 5, 4, 4, hidden=32, mode=mode, ticks=2) for mode in MODES] + \
              [Case("probe", 3, 5, 4, 5, hidden=64, A=2, mode=mode, ticks=3) for mode in MODES]
