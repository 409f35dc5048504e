"""Cases and inputs of the A2C / PPO update kernels for a custom environment's in-kernel policy (include/wd_env_update.h;
training/pg_update_custom_kernels.py).  No GPU.

The yardstick is tests/pg_update_cases.py's, as it stands: its float64 restatement is generic in O and A.  A case with n
agents per replica IS that module's case with E * n columns (column i = replica i // n, agent i % n) whose done flags are
the replica's, repeated per agent -- tests/pg_update_gridworld_cases.py's construction, whose `done_flags` and
`returns_model_n` are used as they are.  What this file adds:

  * `CASES`: the smallest shapes at which the launches can still go wrong (a tile is 128 rows): 2 rows, exactly one tile, a
    tile boundary inside a batch row (260 rows), 20 tiles on 3 blocks, surplus blocks, whole tiles on 2 blocks, a tile
    boundary inside a REPLICA's 70 agents, logit gaps above 110; F in {1, 5, 7} (no float4 / one float4 and a tail of
    one / of three), A in {1, 2, 5, 8}, n in {1, 4, 70}, both widths, A2C and PPO, four done patterns with "random" --
    neighbouring replicas differ -- wherever n > 1;
  * `unit_of`: the device source that has a case's entries (F = 5: examples/rendezvous_update/; F = 1, 7: the probes of
    tests/custom_envs/update_probe.py);
  * the two planted defects of the gridworld cases for the host test: "the done flag of replica i % E", "inv_R without n".

The bound is tests/update_kernel_cases.py's: err <= max(4 * err_f32, 2e-6 * scale) per result tensor."""
import collections
import os

import numpy as np

from tests import pg_update_cases as pc
from tests import pg_update_gridworld_cases as gc

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE_SOURCE = os.path.join(ROOT, "examples", "rendezvous_update", "rendezvous_update.hip")
EXAMPLE_UNIT, EXAMPLE_PREFIX, EXAMPLE_OBS = "RendezvousUpdate", "HipRendezvousUpdatePg", 5

CuCase = collections.namedtuple("CuCase", "name E T n gamma H F A ent vf algo done grid gap seed")


def _case(E, T, n, gamma, H, F, A, ent, vf, done, algo="A2C", grid=None, gap=False, seed=0):
    name = (f"E{E}-T{T}-n{n}-g{gamma}-H{H}F{F}A{A}-ent{ent}-vf{vf}-{algo}-{done.replace(' ', '_')}"
            + (f"-grid{grid}" if grid else "") + ("-gap" if gap else ""))
    return CuCase(name, E, T, n, gamma, H, F, A, ent, vf, algo, done, grid, gap, seed)


# grid: blocks of the gradient launch (None: one per tile)
CASES = (
    _case(1, 2, 1, 1.0, 32, 1, 1, 0.0, 0.01, "none", seed=1),                                  # 2 rows, one action
    _case(16, 2, 4, 0.98, 64, 5, 5, 0.05, 1.0, "one mid-batch", "PPO", seed=2),                # 128 rows: exactly one tile
    _case(13, 5, 4, 0.98, 32, 7, 2, 0.05, 0.01, "random", seed=3),                             # 260 rows: 2 tiles + 4 rows
    _case(4, 9, 70, 0.98, 64, 5, 8, 0.05, 1.0, "random", "PPO", grid=3, seed=4),               # 2520 rows: 20 tiles on 3 blocks
    _case(33, 5, 1, 1.0, 32, 7, 8, 0.05, 1.0, "one mid-batch", grid=5, seed=5),                # 165 rows: 3 surplus blocks
    _case(64, 10, 1, 0.98, 64, 1, 2, 0.0, 0.01, "last row", "PPO", grid=2, seed=6),            # 640 rows: 5 tiles on 2 blocks
    _case(16, 5, 4, 0.98, 64, 7, 5, 0.05, 1.0, "last row", gap=True, seed=7),                  # logit gaps above 110
    _case(2, 3, 70, 0.98, 32, 5, 5, 0.05, 0.01, "random", seed=8),                             # 420 rows: a boundary inside a replica
)


def case_rows(case):
    return case.T * case.E * case.n


def case_tiles(case):
    return -(-case_rows(case) // pc.TILE)


def case_grid(case):
    return case.grid or case_tiles(case)


def unit_of(F):
    """(unit name, device source, entry prefix) of the code object that has the entries for observation size F"""
    if F == EXAMPLE_OBS:
        return EXAMPLE_UNIT, EXAMPLE_SOURCE, EXAMPLE_PREFIX
    from tests.custom_envs import update_probe

    name = update_probe.RUN[F]
    source, size, prefix = update_probe.UNITS[name]
    assert size == F
    return name, source, prefix


def as_pc_case(case):
    """tests/pg_update_cases.py's case with E * n columns"""
    return pc.Case(case.name, case.E * case.n, case.T, case.gamma, case.H, case.F, case.A, case.ent, case.vf, case.algo,
                   case.done, case.grid, case.gap, case.seed)


def inputs(case):
    """{obs [T, E * n, F], actions [T, E * n] int32, rewards [T, E * n], done [T, E * n] int32 (the replica's flag repeated
    per agent), done_env [T, E] int32, theta (flat float32)}: tests/pg_update_cases.py::inputs' keys on E * n columns, plus
    the replica-level flags the returns launch is given"""
    rng = np.random.default_rng(9000 + case.seed)
    T, E, n, H, F, A = case.T, case.E, case.n, case.H, case.F, case.A
    done_env = gc.done_flags(case, rng)
    return {
        "obs": rng.standard_normal((T, E * n, F)).astype(f32),
        "actions": rng.integers(0, A, (T, E * n)).astype(np.int32),
        "rewards": (rng.standard_normal((T, E * n)) - 1.0).astype(f32),
        "done": np.repeat(done_env, n, axis=1),
        "done_env": done_env,
        "theta": pc.flatten(pc._make_net(rng, H, F, A, 20000.0 if case.gap else 1.0)),
    }


returns_model_n = gc.returns_model_n

# ----------------------------------------------------------------------------------------------- the planted defects
MUTATIONS = gc.MUTATIONS


def mutation_applies(case, mutation):
    if mutation == "the done flag of replica i % E":
        return case.n > 1 and case.E > 1 and case.done in ("random", "one mid-batch")
    if mutation == "inv_R without n":
        return case.n > 1
    return pc.mutation_applies(as_pc_case(case), mutation)


def yardstick(case, inp, mutate=None, values=None):
    """tests/pg_update_cases.py::yardstick on the E * n columns; the two defects of the gridworld cases planted around it"""
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


# ------------------------------------------------------------------------------------------------- the apply stage
# tests/pg_update_cases.py::APPLY_CASES' pattern -- clip active / inactive / off at Adam steps 1, 2, 1000 -- at the new shapes
APPLY_CASES = tuple(
    pc.ApplyCase(f"H{H}F{F}A{A}-step{ac.step}-clip_{ac.clip}", H, F, A, ac.step, ac.clip, ac.max_norm, ac.lr, 80 + i)
    for i, (ac, (H, F, A)) in enumerate(zip(pc.APPLY_CASES, [(32, 1, 1), (64, 5, 5), (64, 7, 8), (64, 1, 2), (32, 7, 5),
                                                            (32, 5, 8), (64, 7, 2), (32, 5, 5), (64, 1, 8)])))
