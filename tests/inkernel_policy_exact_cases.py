"""Cases, preset epochs and host models for the tests that hold the in-kernel policies of the in-tree rollout and evaluation
entries to tolerance 0 with NO excused draw (tests/test_gpu_inkernel_policy_exact.py on the device,
tests/test_inkernel_policy_exact_host.py on the host: no case can pass vacuously, and every planted defect is caught).
Nothing here touches a GPU.

The policies are tests/crafted_policies.py's: their probabilities are exactly 0, 0.5, 1 or 1 / A, so the action is a pure
function of the observation and the Philox uniform, with no window around a threshold.  The epoch words are preset so that
known rows draw u == 1.0 and u == 2^-24 -- on each of the four words of a Philox block -- inside the launch, two rows
cross the 2^32 wrap, and the rest start at arbitrary epochs.  The in-tree draw is wd_tick_draw: word (epoch & 3) of the
block with counter (row, epoch >> 2, tag, 4) (oracle/core_np.py::single_head_tick_uniform); a TagGridWorld row is
env * 5 + agent.

The host models of the device tests are the project's restatements, unchanged (oracle/cartpole_np.py,
tests/classic_control_policy.py, oracle/tag_gridworld_np.py and the replays of tests/classic_control_evaluate.py,
tests/gridworld_evaluate.py, tests/cartpole_pool_cases.py, tests/gridworld_pool_cases.py).  `probabilities` below is a
second statement of the same network that can carry a planted DEFECT; without one it equals the restatements bit for
bit (asserted on the host)."""
import functools

import numpy as np

from oracle.core_np import find_end_draws, pool_pick, seed_words, single_head_tick_uniform
from oracle.tag_gridworld_np import TagGridWorldOracle
from tests import cartpole_pool_cases as cpool
from tests import classic_control_cases as cc
from tests import classic_control_evaluate as ev
from tests import crafted_policies as cp
from tests import gridworld_evaluate as gev
from tests import gridworld_pool_cases as gpool

F32 = np.float32
SINGLE = ("cartpole", "acrobot", "mountain_car")
WIDTHS = cp.WIDTHS
E_SINGLE, E_GRID, N = 130, 25, 5        # two wavefronts and two lanes; two full groups of 12 replicas and a group of one
TICKS, LAUNCHES, LENGTHS = 9, 2, (7, 13)
TOTAL = TICKS * LAUNCHES
N_QUADS = 1 << 19                       # Philox blocks searched per row: 8 rows with u == 1.0 below row 125, every word hit
EVAL_SPAN = 3                           # an evaluation reaches its end draws within its first three ticks
TIE_ROW, TIE_REPLICA = 5, 0
CLAMP_SHIFTS = (0, 1, 2, 3, 4, 5)       # the random policy runs under six presets: its end rows meet other observations
CLAMP_MARGIN, CLAMP_ROWS, CLAMP_ROWS_ON_THE_HOST = 1e-3, 8, 12
# torch.manual_seed of the random policy per (env, hidden): the rollout cases' own seed 5 where the host replay alone finds
# CLAMP_ROWS_ON_THE_HOST clamp rows (see `clamp_rows`) over both episode lengths and the six presets, else the first seed
# from 1 on that does (a float32 running sum ends below 1.0 on one row in four to ten; HEAD_SCALE saturates many rows).
# `python -m tests.inkernel_policy_exact_cases` repeats the search and prints the table.
CLAMP_SEED = {
    ("cartpole", 32): 7,       # 19 clamp rows on the host
    ("cartpole", 64): 1,       # 13
    ("acrobot", 32): 1,        # 13
    ("acrobot", 64): 1,        # 13
    ("mountain_car", 32): 5,   # 12
    ("mountain_car", 64): 2,   # 20
    ("gridworld", 32): 5,      # 14
    ("gridworld", 64): 5,      # 16
}
DEFECTS = ("le", "no_clamp", "last_max", "drop_w0_last_column", "drop_last_hidden", "swap_policies", "bias_after_relu")
assert cc.SAMPLER_SEED == gev.SAMPLER_SEED and int(cc.TICK_TAG) == int(gev.TICK_TAG)
KEY = seed_words(cc.SAMPLER_SEED)


# ------------------------------------------------------------------------------------------------ epochs and the ends
@functools.lru_cache(maxsize=None)
def end_draws():
    """{(word, "hi" | "lo"): [(row, epoch), ...]}: the draws with u == 1.0 ("hi") and u == 2^-24 ("lo") of rows below 130
    within N_QUADS Philox blocks; epoch = 4 * block + word"""
    found = find_end_draws(KEY[0], KEY[1], int(cc.TICK_TAG), 4, E_SINGLE, N_QUADS, words=(0, 1, 2, 3))
    return {(w, kind): [(row, 4 * quad + w) for row, quad in rows] for (w, kind), rows in found.items()}


def uniforms(epochs, tick):
    """float32 [rows]: the uniform every row draws at `epochs + tick` (mod 2^32)"""
    e = (np.asarray(epochs, np.uint64) + np.uint64(tick)).astype(np.uint32)
    return single_head_tick_uniform(len(e), e, KEY[0], KEY[1], cc.TICK_TAG)


def preset_epochs(n_rows, span=TOTAL, shift=0):
    """(epochs uint32 [n_rows], roles {row: (word, "hi" | "lo", tick)}, wrap rows): one row per word and end, then every
    further row with a draw of 1.0 (the clamp rows), each reaching its end draw at `tick` < span of the run -- ticks 3, 8
    (the last of the first launch), 13, 0, 5, 10, 15, 2, 7, 12, 17 (the last of the second), ... shifted by `shift`; two
    other rows start at 0xFFFFFFFF and 0xFFFFFFFE; the rest at arbitrary epochs.  Fails when an end is missing."""
    ends = end_draws()
    epochs = np.random.RandomState(7).randint(0, 2 ** 32, size=n_rows, dtype=np.uint64).astype(np.uint32)
    roles, picks = {}, []
    if n_rows >= E_GRID * N:
        clamp = {r for w in range(4) for r, _ in ends[(w, "hi")]}   # (no row with a draw of 1.0 is spent on a low end)
        for w in range(4):
            for kind in ("hi", "lo"):
                found = [(r, e) for r, e in ends[(w, kind)] if r < n_rows and r not in [p[0] for p in picks]
                         and (kind == "hi" or r not in clamp)]
                assert found, f"no {kind} end on word {w} in {N_QUADS} blocks of {n_rows} rows"
                picks.append((found[0][0], found[0][1], w, kind))
        for w in range(4):
            for r, e in ends[(w, "hi")]:
                if r < n_rows and r not in [p[0] for p in picks]:
                    picks.append((r, e, w, "hi"))
    for i, (r, e, w, kind) in enumerate(picks):
        tick = min((5 * i + 3 + shift) % span, e)
        roles[r] = (w, kind, tick)
        epochs[r] = e - tick
    wrap = [r for r in range(n_rows) if r not in roles and r not in (TIE_ROW,)][:2]
    for r, start in zip(wrap, (0xFFFFFFFF, 0xFFFFFFFE)):
        epochs[r] = start
    return epochs, roles, wrap


# ------------------------------------------------------------------------------- the network, with a planted defect
def probabilities(env, packed, hidden, obs, defect=None):
    """the restated network on the packed buffer of layout `env` (tests/crafted_policies.py::LAYOUT): acc = bias, one
    fused multiply-add per input in index order (float64 product and sum, rounded once), ReLU, softmax with the maximum
    subtracted, the sum in action order, one division per action.  obs [R, I] -> [R, A] float32.
    defect: "drop_w0_last_column", "drop_last_hidden" (the last hidden unit of both layers feeds nothing),
    "bias_after_relu" (fmaxf(W . x, 0) + b in the hidden layers)"""
    parts = cp.unpack(env, packed, hidden)
    W0, W1, Wp = parts["W0"].copy(), parts["W1"].copy(), parts["Wp"].copy()
    if defect == "drop_w0_last_column":
        W0[:, -1] = 0
    if defect == "drop_last_hidden":
        W1[:, -1] = 0
        Wp[:, -1] = 0
    late = defect == "bias_after_relu"

    def layer(v, W, b, hidden_layer):
        first = np.zeros_like(b) if (late and hidden_layer) else b
        acc = np.broadcast_to(first, (v.shape[0], W.shape[0])).astype(F32).copy()
        for j in range(W.shape[1]):
            acc = (W[None, :, j].astype(np.float64) * v[:, j:j + 1].astype(np.float64) + acc.astype(np.float64)).astype(F32)
        if not hidden_layer:
            return acc
        out = np.maximum(acc, F32(0))
        return (out + b).astype(F32) if late else out

    x = np.asarray(obs, F32)
    h2 = layer(layer(x, W0, parts["b0"], True), W1, parts["b1"], True)
    logits = layer(h2, Wp, parts["bp"], False)
    e = np.exp((logits - logits.max(axis=1, keepdims=True)).astype(F32)).astype(F32)
    s = np.zeros(e.shape[0], F32)
    for a in range(e.shape[1]):
        s = (s + e[:, a]).astype(F32)
    return (e / s[:, None]).astype(F32)


def running_sums(p):
    p = np.asarray(p, F32)
    cum = np.empty_like(p)
    acc = np.zeros(p.shape[0], F32)
    for a in range(p.shape[1]):
        acc = p[:, a].copy() if a == 0 else (acc + p[:, a]).astype(F32)
        cum[:, a] = acc
    return cum


def pick(cum, u, defect=None):
    """the counting draw: the number of running sums below u, clamped to the last action.  defect "le": `<=` in the count;
    "no_clamp": the count itself"""
    cum, u = np.asarray(cum, F32), np.asarray(u, F32)[:, None]
    cnt = ((cum <= u) if defect == "le" else (cum < u)).sum(axis=1)
    return (cnt if defect == "no_clamp" else np.minimum(cnt, cum.shape[1] - 1)).astype(np.int32)


def greedy(p, defect=None):
    """the FIRST maximum (strict `<`); defect "last_max": the last one"""
    p = np.asarray(p, F32)
    best, act = p[:, 0].copy(), np.zeros(len(p), np.int32)
    for i in range(1, p.shape[1]):
        better = (best <= p[:, i]) if defect == "last_max" else (best < p[:, i])
        best = np.where(better, p[:, i], best)
        act = np.where(better, i, act).astype(np.int32)
    return act


def grid_probabilities(packed, hidden, obs, defect=None):
    """[E, 5, 21] -> [E, 5, 5]: the tagger's network on agents 0 - 3, the runner's on agent 4 ("swap_policies": the
    other way round)"""
    tagger, runner = (packed[1], packed[0]) if defect == "swap_policies" else (packed[0], packed[1])
    E = obs.shape[0]
    p = np.empty((E, N, 5), F32)
    p[:, :N - 1] = probabilities("gridworld", tagger, hidden, obs[:, :N - 1].reshape(-1, 21), defect).reshape(E, N - 1, 5)
    p[:, N - 1] = probabilities("gridworld", runner, hidden, obs[:, N - 1], defect)
    return p


# ------------------------------------------------------------------------------------------------ single-agent cases
TIE_STATE = {"cartpole": (0.1, 0.2, 0.125, -0.5),      # theta + theta_dot / 4 == 0
             "mountain_car": (-0.5, 0.0),              # at rest
             "acrobot": (0.3, -0.2, 0.0, 1.5)}         # theta_dot_1 == 0


def single_start_states(env, E):
    """spread over the state space (otherwise a deterministic policy gives every replica one trajectory); TIE_ROW at the
    exact-tie state of the env's switched policy"""
    state = cc.spread_states(env, np.random.RandomState(11), E)
    if E > TIE_ROW:
        state[TIE_ROW] = np.asarray(TIE_STATE[env], F32)
    else:
        state[0] = np.asarray(TIE_STATE[env], F32)
    return state


def single_start_obs(env, state):
    """the observation rows of the start states (the device test writes them: the policy of tick 0 sees the replica's
    own state, not the registered restart row)"""
    return state.copy() if env == "cartpole" else cc.host_obs(env, state)


class SingleCase(cc.RolloutCase):
    """...EnvRollout_H<hidden> of one single-agent env with its own action count: E replicas, episodes of T ticks, two
    launches of nine ticks from spread states and time steps row % T (replicas finish inside a launch, on its last tick
    and at the time limit), the preset epochs.  `packed`: the policy under test."""

    def __init__(self, env, hidden, T, E=E_SINGLE, geom=(64, None), shift=0):
        self.env, self.hidden, self.T, self.E, self.geom, self.shift = env, int(hidden), int(T), int(E), geom, int(shift)
        self.ticks, self.launches, self.rows = TICKS, LAUNCHES, TICKS
        self.pool = 0 if env == "cartpole" else 7
        self.A = cp.LAYOUT[env][2]
        self.cont, self.physics, self.extra, self.epochs, self.timesteps, self.share = False, None, None, "preset", "spread", 0.0
        self.packed = cp.kinds(env, self.hidden)["uniform"]
        self.name = f"{env}-exact-H{hidden}-T{T}-E{E}" + ("-idle" if geom[1] == "idle" else "")

    def has_one_draw(self):
        return False

    def preset(self):
        return preset_epochs(self.E, TOTAL, self.shift)

    def start_epochs(self):
        return self.preset()[0].copy()

    def start_states(self):
        return single_start_states(self.env, self.E)

    def policy(self):
        return None, self.packed

    def random_policy(self, seed=5):
        """the rollout cases' random policy: FullyConnected under torch.manual_seed(seed), the head times HEAD_SCALE"""
        import torch
        from warp_drive_amd.training.models import FullyConnected
        from warp_drive_amd.training.policy_kernel import pack_rollout_policy

        torch.manual_seed(seed)
        model = FullyConnected(cc.OBS_DIM[self.env], [self.A], [self.hidden, self.hidden])
        with torch.no_grad():
            model.policy_head[0].weight.mul_(cc.HEAD_SCALE)
        return pack_rollout_policy(model).numpy()


def single_cases(env, hidden):
    """both episode lengths at E = 130; one replica; the geometry with two idle blocks"""
    return [SingleCase(env, hidden, T) for T in LENGTHS] + [SingleCase(env, hidden, 7, E=1),
                                                            SingleCase(env, hidden, 13, geom=(64, "idle"))]


def simulate_single(case, packed, defect=None, ticks=TOTAL):
    """the two launches (or `ticks` ticks) on the host alone (numpy step, `probabilities`, the Philox replay) ->
    {"actions" [K, E], "probs" [K, E, A], "cum", "u" [K, E], "done" [K, E] (0, 1: time limit or termination, 2:
    MountainCar's goal), "early" [K, E] bool (finished before the time limit), "wrapped"}"""
    from warp_drive_amd.envs.classic_control import apply_done

    env, E, T = case.env, case.E, case.T
    env_obj = cc.make_env(env, T, case.pool)
    start = np.asarray(env_obj.get_data_dictionary()["state"]["data"], F32).reshape(-1)
    pool_states = None
    if case.pool:
        pool_states = np.asarray(env_obj.get_reset_pool_dictionary()["state_reset_pool"]["data"], F32)[:, 0]
    obs0 = single_start_obs(env, start[None])[0]
    step = cc.numpy_step(env)
    state, ts = case.start_states(), case.start_timesteps().astype(np.int64)
    obs = single_start_obs(env, state)
    epochs, pool_epochs = case.start_epochs(), case.start_pool_epochs()
    p0, p1 = seed_words(cc.POOL_SEED)
    out = {k: [] for k in ("actions", "probs", "cum", "u", "done", "early")}
    for k in range(ticks):
        u = uniforms(epochs, k)
        p = probabilities(env, packed, case.hidden, obs, defect)
        cum = running_sums(p)
        a = pick(cum, u, defect)
        state, obs, _, term = step(state, np.minimum(a, case.A - 1))
        ts += 1
        done = apply_done(term, ts, T)
        fin = np.flatnonzero(done > 0)
        for key, v in (("actions", a), ("probs", p), ("cum", cum), ("u", u), ("done", done.copy()),
                       ("early", (done > 0) & (ts < T))):
            out[key].append(v)
        ts[fin] = 0
        obs[fin] = obs0
        if case.pool:
            state[fin] = pool_states[pool_pick(fin, pool_epochs[fin], p0, p1, case.pool)]
            pool_epochs[fin] += np.uint32(1)
        else:
            state[fin] = start
    out = {k: np.stack(v) for k, v in out.items()}
    out["wrapped"] = int((epochs.astype(np.uint64) + np.uint64(TOTAL) > np.uint64(1 << 32)).sum())
    return out


class SingleEvalCase(ev.EvalCase):
    """...EnvEvaluate_H<hidden>, greedy or sampled, one episode of T ticks from the same spread states (time steps
    row % 4) and the preset epochs of an evaluation (the end draws within the first three ticks)"""

    def __init__(self, env, hidden, mode, T, E=E_SINGLE):
        super().__init__(env, hidden, mode, E=E)
        self.T = int(T)
        self.packed = cp.kinds(env, self.hidden)["uniform"]
        self.name = f"{env}-exact-H{hidden}-{mode}-T{T}-E{E}"

    def policy(self):
        return None, self.packed

    def start(self):
        return single_start_states(self.env, self.E), (np.arange(self.E) % 4).astype(np.int32)

    def preset(self):
        return preset_epochs(self.E, EVAL_SPAN)

    def start_epochs(self):
        return self.preset()[0].copy()

    def near_cap(self, decisions):
        return 0


# ------------------------------------------------------------------------------------------------- TagGridWorld cases
def grid_start(case_E, L, T):
    """(loc_x, loc_y int32 [E, 5], timestep int32 [E]): positions uniform on 0 .. L, time steps 3 * row % T; TIE_REPLICA at
    time step 0 with tagger 0 in the runner's column (the tagger's form is 0) and the runner on y == 0 (the runner's form
    y / L - t / T is 0), no tagger on the runner's cell"""
    rng = np.random.RandomState(gev.START_SEED)
    x = rng.randint(0, L + 1, size=(case_E, N)).astype(np.int32)
    y = rng.randint(0, L + 1, size=(case_E, N)).astype(np.int32)
    ts = ((3 * np.arange(case_E)) % T).astype(np.int32)
    x[TIE_REPLICA], y[TIE_REPLICA] = (3, 7, 1, 8, 3), (5, 2, 9, 6, 0)
    return x, y, ts


class GridCase(gev.GwCase):
    """HipTagGridWorldRollout_N5_H<hidden> (two launches of nine ticks) and HipTagGridWorldEvaluate_N5_H<hidden> (one
    episode) at E = 25 on a grid of side 11: `packed` = [tagger, runner]"""

    def __init__(self, hidden, mode, T, E=E_GRID, shift=0, span=TOTAL):
        super().__init__(hidden, mode, grid_length=10, T=T, E=E)
        self.shift, self.span = int(shift), int(span)
        self.packed = cp.kinds("gridworld", self.hidden)["uniform"]
        self.name = f"gridworld-exact-H{hidden}-{mode}-T{T}-E{E}"

    def policies(self, seed=None):
        if seed is None:
            return None, self.packed
        return gev.GwCase.policies(self, seed)

    def oracle(self):
        orc = TagGridWorldOracle(num_envs=self.E, **self.env_config())
        orc.loc_x, orc.loc_y, orc.timestep = grid_start(self.E, self.L, self.T)
        orc.obs = orc.generate_observation()
        return orc

    def preset(self):
        return preset_epochs(self.E * N, self.span, self.shift)

    def start_epochs(self):
        return self.preset()[0].copy().reshape(self.E, N)

    def near_cap(self, decisions):
        return 0


def simulate_grid(case, packed, defect=None):
    """the two launches of the rollout on the host alone -> {"actions" [K, E, 5], "probs" [K, E, 5, 5], "cum", "u"
    [K, E, 5], "done" [K, E], "tagged" [K, E] bool}"""
    orc, E = case.oracle(), case.E
    epochs = case.start_epochs().reshape(-1)
    out = {k: [] for k in ("actions", "probs", "cum", "u", "done", "tagged")}
    for k in range(TOTAL):
        u = uniforms(epochs, k).reshape(E, N)
        p = grid_probabilities(packed, case.hidden, orc.obs.astype(F32), defect)
        cum = running_sums(p.reshape(-1, 5))
        a = pick(cum, u.reshape(-1), defect).reshape(E, N)
        _, rew, done = orc.step(np.minimum(a, 4))
        for key, v in (("actions", a), ("probs", p), ("cum", cum.reshape(E, N, 5)), ("u", u), ("done", done.copy()),
                       ("tagged", (done > 0) & (rew[:, 0] > 5.0))):
            out[key].append(v)
        orc.reset_done_envs()
    return {k: np.stack(v) for k, v in out.items()}


# --------------------------------------------------------------------------------------- the pooled entries (reduced)
class CartpolePoolCase(cpool.PoolCase):
    """HipClassicControlCartPoleEnvRollout_P_H<hidden> at E = 130, T = 7, the preset epochs"""

    def __init__(self, hidden, T=7, E=E_SINGLE):
        self.env, self.hidden, self.T, self.E = "cartpole", int(hidden), int(T), int(E)
        self.ticks, self.launches, self.rows, self.pool, self.A = TICKS, LAUNCHES, TICKS, 7, 2
        self.cont, self.physics, self.extra, self.epochs, self.timesteps, self.share = False, None, None, "preset", "spread", 0.0
        self.crafted, self.seed = False, 5
        self.packed = cp.kinds("cartpole", self.hidden)["uniform"]
        self.name = f"cartpole-pool-exact-H{hidden}-T{T}-E{E}"

    def has_one_draw(self):
        return False

    def start_epochs(self):
        return preset_epochs(self.E, TOTAL)[0].copy()

    def start_states(self):
        return single_start_states("cartpole", self.E)

    def policy(self):
        return None, self.packed


class GridPoolCase(gpool.PoolCase):
    """HipTagGridWorldRollout_N5P_H<hidden> at E = 25, the preset epochs, GridCase's start"""

    def __init__(self, hidden, T=7):
        super().__init__(f"gridworld-pool-exact-H{hidden}-T{T}", E_GRID, 10, T, TICKS, launches=LAUNCHES)
        self.hidden = int(hidden)

    def start_epochs(self):
        return preset_epochs(self.E * N, TOTAL)[0].copy()

    def start_oracle(self):
        orc = TagGridWorldOracle(num_envs=self.E, **self.config())
        orc.loc_x, orc.loc_y, orc.timestep = grid_start(self.E, self.L, self.T)
        orc.obs = orc.generate_observation()
        return orc


def grid_exact_choice(packed, hidden):
    """choose(k, obs, u) of tests/gridworld_pool_cases.py::PoolModel.launch on the project's restatement, nothing excused"""
    from oracle.tag_gridworld_np import running_sums as sums

    def choose(k, obs, u):
        p = gev.probabilities(packed, hidden, obs)
        cum = sums(p.reshape(-1, 5)).reshape(-1, N, 5)
        return np.minimum((cum < u[..., None]).sum(axis=-1), 4).astype(np.int32)

    return choose


# ------------------------------------------------------------------------------------------------ what the rows show
def end_rows(roles, kind):
    """[(row, word, tick)] of the rows whose end draw is `kind`"""
    return [(r, w, t) for r, (w, k, t) in sorted(roles.items()) if k == kind]


def clamp_rows(cum, u, A, roles):
    """the (tick, row) pairs of a run with u == 1.0 where the model's last running sum is below 1.0 and the one before it
    below 1 - CLAMP_MARGIN (so is the device's, whose sums differ from the model's by a few 1e-7): all A sums are below u
    on any correct implementation, and only the clamp gives A - 1.  cum [K, rows, A], u [K, rows]."""
    out = []
    for r, w, t in end_rows(roles, "hi"):
        assert float(u[t, r]) == 1.0
        before = cum[t, r, A - 2] if A >= 2 else F32(0)
        if cum[t, r, A - 1] < 1.0 and before < 1.0 - CLAMP_MARGIN:
            out.append((t, r))
    return out


def single_clamp_rows(env, hidden, seed):
    """the clamp rows of the host replay of the random policy `seed` over both episode lengths and every preset"""
    total = 0
    for T in LENGTHS:
        for shift in CLAMP_SHIFTS:
            case = SingleCase(env, hidden, T, shift=shift)
            r = simulate_single(case, case.random_policy(seed))
            total += len(clamp_rows(r["cum"], r["u"], case.A, case.preset()[1]))
    return total


def grid_clamp_rows(hidden, seed):
    total = 0
    for T in LENGTHS:
        for shift in CLAMP_SHIFTS:
            case = GridCase(hidden, "sampled", T, shift=shift)
            r = simulate_grid(case, case.policies(seed)[1])
            total += len(clamp_rows(r["cum"].reshape(TOTAL, -1, 5), r["u"].reshape(TOTAL, -1), 5, case.preset()[1]))
    return total


if __name__ == "__main__":   # the seed search
    for env in SINGLE + ("gridworld",):
        for H in WIDTHS:
            for seed in [5] + [s for s in range(1, 40) if s != 5]:
                n = grid_clamp_rows(H, seed) if env == "gridworld" else single_clamp_rows(env, H, seed)
                if n >= CLAMP_ROWS_ON_THE_HOST:
                    print(f'    ("{env}", {H}): {seed},   # {n} clamp rows')
                    break
            else:
                print(env, H, "no seed below 40")
