"""Cases and inputs of the A2C / PPO update kernels for the TagGridWorld policies (csrc/kernels/pg_update_gridworld.hip;
training/pg_update_gridworld_kernels.py).  No GPU.

The yardstick is tests/pg_update_cases.py's, as it stands: its float64 restatement is generic in O and A.  A case with n
agents per replica IS that module's case with E * n columns (column i = replica i // n, agent i % n) whose done flags are
the replica's, repeated per agent (`as_pc_case`, `inputs`).  What this file adds:

  * `CASES`: O = 21, A = 5, the smallest shapes at which the launches can still go wrong (a tile is 128 rows): 2 rows,
    exactly one tile, a tile boundary inside a batch row, 21 tiles on 3 blocks, surplus blocks, whole tiles on 2 blocks,
    logit gaps above 110; both widths, gamma 1 and 0.98, entropy coefficients 0 and 0.05, value coefficients 0.01 and 1,
    A2C and PPO, n = 1 and n = 4;
  * done patterns per REPLICA: none, last row, one mid-batch, independent random flags (neighbouring replicas differ: a
    replica index formed wrongly from the (replica, agent) index shows);
  * observation rows drawn like the environment's in two cases (coordinates k / L, 0 / 1 type and "is me" columns, t / T
    last: exact zeros and ones among the inputs);
  * `returns_model_n`: losses.discounted_returns on [T, E, n] arrays with [T, E] done flags, operation for operation;
  * two more planted defects for the host test: "the done flag of replica i % E" and "inv_R without n".

The bound is tests/update_kernel_cases.py's: err <= max(4 * err_f32, 2e-6 * scale) per result tensor."""
import collections

import numpy as np

from tests import pg_update_cases as pc

f32, f64 = np.float32, np.float64
O, A = 21, 5
DONE_PATTERNS = ("none", "last row", "one mid-batch", "random")
GRID_CELLS = 10   # L of the environment-like observation rows

GwCase = collections.namedtuple("GwCase", "name E T n gamma H ent vf algo done grid gap envlike seed")


def _case(E, T, n, gamma, H, ent, vf, done, algo="A2C", grid=None, gap=False, envlike=False, seed=0):
    name = (f"E{E}-T{T}-n{n}-g{gamma}-H{H}-ent{ent}-vf{vf}-{algo}-{done.replace(' ', '_')}" + (f"-grid{grid}" if grid else "")
            + ("-gap" if gap else "") + ("-envlike" if envlike else ""))
    return GwCase(name, E, T, n, gamma, H, ent, vf, algo, done, grid, gap, envlike, seed)


# grid: blocks of the gradient launch (None: one per tile)
CASES = (
    _case(1, 2, 1, 1.0, 32, 0.0, 0.01, "none", seed=1),                                         # 2 rows: the smallest batch
    _case(16, 2, 4, 0.98, 64, 0.05, 1.0, "one mid-batch", "PPO", seed=2),                       # 128 rows: exactly one tile
    _case(13, 5, 4, 0.98, 32, 0.05, 0.01, "random", envlike=True, seed=3),                      # 260 rows: 2 tiles + 4 rows
    _case(65, 10, 4, 0.98, 64, 0.05, 1.0, "random", "PPO", grid=3, seed=4),                     # 2600 rows: 21 tiles on 3 blocks
    _case(33, 5, 1, 1.0, 32, 0.05, 1.0, "one mid-batch", grid=5, seed=5),                       # 165 rows: 3 surplus blocks
    _case(64, 10, 1, 0.98, 64, 0.0, 0.01, "last row", "PPO", grid=2, envlike=True, seed=6),     # 640 rows: 5 tiles on 2 blocks
    _case(16, 5, 4, 0.98, 64, 0.05, 1.0, "last row", gap=True, seed=7),                         # logit gaps above 110
)


def case_rows(case):
    return case.T * case.E * case.n


def case_tiles(case):
    return -(-case_rows(case) // pc.TILE)


def case_grid(case):
    return case.grid or case_tiles(case)


def as_pc_case(case):
    """tests/pg_update_cases.py's case with E * n columns"""
    return pc.Case(case.name, case.E * case.n, case.T, case.gamma, case.H, O, A, case.ent, case.vf, case.algo, case.done,
                   case.grid, case.gap, case.seed)


def done_flags(case, rng):
    """[T, E] int32, per replica"""
    T, E = case.T, case.E
    done = np.zeros((T, E), np.int32)
    if case.done == "last row":
        done[-1] = 1
    elif case.done == "one mid-batch":
        done[(T - 1) // 2, E // 2] = 1
    elif case.done == "random":
        done[:] = rng.random((T, E)) < 0.3
        for e in range(1, E):   # neighbours differ: an odd replica is its left neighbour's opposite, an even one in row 0
            if e % 2:
                done[:, e] = 1 - done[:, e - 1]
            else:
                done[0, e] = 1 - done[0, e - 1]
    return done


def _envlike_obs(case, rng):
    """rows like TagGridWorld's at 5 agents: 10 coordinates k / L, five 0 / 1 type flags, a one-hot "is me", t / T"""
    T, E, n = case.T, case.E, case.n
    obs = np.zeros((T, E, n, O), f32)
    coords = rng.integers(0, GRID_CELLS + 1, (T, E, 1, 10)).astype(f32) / f32(GRID_CELLS)
    obs[..., :10] = coords                                     # every agent of a replica sees the same positions
    obs[..., 10:15] = np.array([1, 1, 1, 1, 0], f32)           # taggers, the runner
    me = np.arange(n) if n > 1 else np.array([4])
    obs[..., np.arange(n), 15 + me] = 1.0
    obs[..., 20] = (np.arange(T, dtype=f32) / f32(T))[:, None, None]
    return obs


def inputs(case):
    """{obs [T, E * n, 21], actions [T, E * n] int32, rewards [T, E * n], done [T, E * n] int32 (the replica's flag
    repeated per agent), done_env [T, E] int32, theta (flat float32)}: tests/pg_update_cases.py::inputs' keys on E * n
    columns, plus the replica-level flags the returns launch is given"""
    rng = np.random.default_rng(7000 + case.seed)
    T, E, n, H = case.T, case.E, case.n, case.H
    obs = _envlike_obs(case, rng) if case.envlike else rng.standard_normal((T, E, n, O)).astype(f32)
    done_env = done_flags(case, rng)
    return {
        "obs": obs.reshape(T, E * n, O),
        "actions": rng.integers(0, A, (T, E * n)).astype(np.int32),
        "rewards": (rng.standard_normal((T, E * n)) - 1.0).astype(f32),
        "done": np.repeat(done_env, n, axis=1),
        "done_env": done_env,
        "theta": pc.flatten(pc._make_net(rng, H, O, A, 20000.0 if case.gap else 1.0)),
    }


def returns_model_n(rewards, done_env, values, gamma, dtype=f32):
    """losses.discounted_returns on rewards / values [T, E, n] and done [T, E], operation for operation in `dtype`"""
    r, v = rewards.astype(dtype), values.astype(dtype)
    d = (done_env > 0).astype(dtype)[..., None]
    one, g = dtype(1), dtype(gamma)
    out = np.zeros_like(r)
    out[-1] = d[-1] * r[-1] + (one - d[-1]) * v[-1]
    for t in range(r.shape[0] - 2, -1, -1):
        out[t] = r[t] + ((one - d[t]) * g) * out[t + 1]
    return out


# ----------------------------------------------------------------------------------------------- the planted defects
MUTATIONS = pc.MUTATIONS + ("the done flag of replica i % E", "inv_R without n")


def mutation_applies(case, mutation):
    if mutation == "the done flag of replica i % E":
        return case.n > 1 and case.E > 1 and case.done in ("random", "one mid-batch")
    if mutation == "inv_R without n":
        return case.n > 1
    return pc.mutation_applies(as_pc_case(case), mutation)


def yardstick(case, inp, mutate=None, values=None):
    """tests/pg_update_cases.py::yardstick on the E * n columns; the two defects of this file are planted around it"""
    pcase = as_pc_case(case)
    if mutate == "the done flag of replica i % E":
        wrong = inp["done_env"][:, np.arange(case.E * case.n) % case.E]
        return pc.yardstick(pcase, {**inp, "done": wrong}, values=values)
    if mutate == "inv_R without n":
        out = pc.yardstick(pcase, inp, values=values)   # (every gradient is linear in inv_R; the sums do not hold it)
        return {k: (v * case.n if k in pc.TENSOR_NAMES else v) for k, v in out.items()}
    return pc.yardstick(pcase, inp, mutate=mutate, values=values)


def framework(case, inp, dtype, device="cpu", values=None):
    return pc.framework(as_pc_case(case), inp, dtype, device, values=values)
