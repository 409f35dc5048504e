"""Host side of the A2C / PPO update kernels for the TagGridWorld policies (no GPU): where the entries live and what they
cost, the wrappers' geometry with n agents in it, the admission rules (the new one, and the old one as it was), the
packed-layout model, and the yardstick of tests/test_gpu_pg_update_gridworld.py -- tests/pg_update_cases.py's float64 pass on
E * n columns agrees with float64 autograd at O = 21, A = 5, and each of eight planted defects breaks the GPU file's bound
on every case it applies to."""
import os

import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests import pg_update_gridworld_cases as gc
from tests.test_pg_update_host import _kernel_metadata, _Recorder
from warp_drive_amd.training import pg_update_gridworld_kernels as pggk
from warp_drive_amd.training import pg_update_kernels as pguk

f32, f64 = np.float32, np.float64
OBJECT = "wd_kernels_pg_gw.hsaco"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge

    ge.build()
    from warp_drive_amd.managers import hip_driver as drv

    return drv


def test_the_new_entries_are_in_a_code_object_of_their_own(built):
    from warp_drive_amd import build as wd_build

    assert wd_build.UNITS[OBJECT] == ("pg_update_gridworld.hip", []) and pggk.CODE_OBJECT == OBJECT
    manifest = built.manifest()
    names = pggk.all_kernel_names()
    assert names == ["HipPgGwApply", "HipPgGwGradients_H32", "HipPgGwGradients_H64", "HipPgGwReduce", "HipPgGwValues_H32",
                     "HipPgGwValues_H64"]
    assert sorted(k for k, v in manifest.items() if v == OBJECT) == names
    assert manifest.get(pguk.RETURNS_ENTRY) == "wd_kernels_update.hsaco"
    # ... and the single-agent object holds what it held
    assert sorted(k for k, v in manifest.items() if v == "wd_kernels_pg.hsaco") == pguk.all_kernel_names()
    assert not set(names) & set(pguk.all_kernel_names())


def test_the_update_units_and_the_two_classes_share_one_source():
    from warp_drive_amd import build as wd_build

    header = os.path.join(wd_build.KDIR, "pg_update_common.h")
    for unit in ("pg_update.hip", "pg_update_gridworld.hip", "ddpg_update.hip"):
        assert header in wd_build.unit_sources(unit), unit
    base = pguk._PgUpdateLaunches
    for cls in (pguk.PgUpdateKernels, pggk.PgGridworldUpdateKernels):
        assert issubclass(cls, base)
        for method in ("compute_values", "discounted_returns", "gradients", "reduce", "apply", "gradient_norm", "metrics",
                       "_check_batch"):
            assert method not in vars(cls) and getattr(cls, method) is getattr(base, method), (cls.__name__, method)
        own = {name for name in vars(cls) if name == "__init__" or not name.startswith("__")}
        assert own == {"__init__", "_shape_args"}, own


def test_entries_have_no_scratch_and_no_spilled_registers(built):
    from warp_drive_amd import build as wd_build

    meta = _kernel_metadata(os.path.join(wd_build.CSRC, OBJECT))
    assert sorted(meta) == pggk.all_kernel_names()
    for name, fields in meta.items():
        assert fields[".private_segment_fixed_size"] == 0, (name, fields)
        assert fields[".vgpr_spill_count"] == 0, (name, fields)
        assert 0 < fields[".vgpr_count"] <= 512, (name, fields)
        bound = (pguk.TILE if "Gradients" in name else pguk.REDUCE_THREADS if name == "HipPgGwReduce" else
                 pguk.APPLY_THREADS if name == "HipPgGwApply" else pguk.VALUES_MAX_THREADS)
        assert fields[".max_flat_workgroup_size"] == bound, (name, fields)
    assert meta["HipPgGwReduce"][".group_segment_fixed_size"] == 4 * pguk.REDUCE_THREADS


@pytest.mark.parametrize("compute_units", [256, 4])
@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_wrappers_launch_five_legal_geometries(case, compute_units):
    rec = _Recorder()
    T, E, n, H = case.T, case.E, case.n, case.H
    k = pggk.PgGridworldUpdateKernels(rec, E, T, n, H, "cpu", compute_units=compute_units)
    assert rec.initialised == pggk.kernel_names(H)
    P = pggk.gw_net_floats(H)
    rows = T * E * n
    assert P == pc.net_floats(H, 21, 5) == k.P and k.rows == rows == gc.case_rows(case)
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    theta, m, v = (z(P) for _ in range(3))
    packed = z(pggk.packed_floats(H))
    obs, actions, rewards, done = z(T, E, n, 21), z(T, E, n, 1, dtype=torch.int32), z(T, E, n), z(T, E, dtype=torch.int32)
    k.compute_values(obs, theta)
    k.discounted_returns(rewards, done, case.gamma)
    k.gradients(obs, actions, theta, case.ent, case.vf)
    k.reduce()
    k.apply(theta, m, v, 1, 1e-3, max_norm=3.0, packed=packed)
    assert [l[0] for l in rec.launches] == pggk.kernel_names(H) and len(rec.launches) == 5
    (_, a1, b1, g1, s1), (_, a2, b2, g2, s2), (_, a3, b3, g3, s3), (_, a4, b4, g4, s4), (_, a5, b5, g5, s5) = rec.launches
    assert b1[0] in (64, 128, 256) and b1[0] <= pguk.VALUES_MAX_THREADS and 1 <= g1[0] <= -(-rows // b1[0])
    assert b1[0] == 64 or -(-rows // b1[0]) >= compute_units      # no block larger than keeps every unit busy
    # the network in LDS: W0 with rows of 24 floats, b0, W1, b1, Wp, eight bias slots, Wv, bv, whole 16-byte vectors
    net_lds = (24 * H + H + H * H + H + 5 * H + 8 + H + 1 + 3) // 4 * 4
    assert s1 == pggk.values_lds_bytes(H) == 4 * net_lds and s1 % 16 == 0 and s1 <= pguk.LDS_LIMIT
    assert len(a1) == 4 and int(a1[2]) == rows and a1[3] is k.values
    # the existing returns entry on `values`: rows of width 1 whose column 0 is the value, n agents per replica
    assert a2[2] is k.values and (int(a2[3]), int(a2[4])) == (1, 0) and float(a2[5]) == float(f32(case.gamma))
    assert (int(a2[6]), int(a2[7]), int(a2[8])) == (T, E, n) and a2[9] is k.returns and a2[10] is k.advantages
    assert b2 == (256, 1, 1) and g2 == (-(-E * n // 256), 1) and s2 == 0
    tiles = -(-rows // pguk.TILE)
    assert b3 == (pguk.TILE, 1, 1) and g3[0] == min(tiles, compute_units) == k.partials.shape[0] >= 1
    assert s3 == pggk.gradients_lds_bytes(H) == s1 + 4 * pguk.LD * (2 * H + 21 + 6 + 4)
    assert s3 % 16 == 0 and s3 <= pguk.LDS_LIMIT
    assert a3[2] is k.advantages and a3[3] is k.returns and int(a3[5]) == rows
    assert float(a3[6]) == float(f32(1.0 / (T * E * n))) and float(a3[7]) == float(f32(case.ent))
    assert float(a3[8]) == float(f32(case.vf)) and a3[9] is k.partials
    assert b4 == (pguk.REDUCE_THREADS, 1, 1) and g4 == (pguk.REDUCE_BLOCKS, 1) == (9, 1) and s4 == 0
    assert (int(a4[1]), int(a4[2])) == (k.partials.shape[0], H)
    covered = g5[0] * pguk.APPLY_THREADS
    assert b5 == (pguk.APPLY_THREADS, 1, 1) and s5 == 0 and int(a5[6]) == H
    assert covered >= max(P, pggk.packed_floats(H)) > covered - pguk.APPLY_THREADS     # every float of the packed block too
    # the sizes the kernels index by
    assert k.values.shape == k.returns.shape == k.advantages.shape == (T, E, n) and k.partials.shape[1] == P + 4
    assert k.grads.numel() == P and k.sumsq.numel() == 8 and k.sums.numel() == 4
    from warp_drive_amd.envs.tag_gridworld import gridworld_policy_floats

    assert pggk.packed_floats(H) == gridworld_policy_floats(H) and pggk.packed_floats(H) > P - H - 1


def test_wrappers_refuse_what_the_kernels_do_not_take():
    rec = _Recorder()
    for bad in ((8, 4, 4, 48), (8, 4, 0, 64), (0, 4, 4, 64), (8, 4, 4, 256)):
        with pytest.raises(AssertionError):
            pggk.PgGridworldUpdateKernels(rec, *bad, "cpu", compute_units=4)
    k = pggk.PgGridworldUpdateKernels(rec, 8, 4, 4, 64, "cpu", compute_units=4)
    theta = torch.zeros(k.P)
    obs, actions = torch.zeros(4, 8, 4, 21), torch.zeros(4, 8, 4, 1, dtype=torch.int32)
    with pytest.raises(AssertionError):
        k.compute_values(torch.zeros(4, 8, 4, 24), theta)                          # another observation size
    with pytest.raises(AssertionError):
        k.compute_values(torch.zeros(4, 8, 21, 4), theta)                          # ... with the right number of floats
    with pytest.raises(AssertionError):
        k.compute_values(obs.double(), theta)                                      # another dtype
    with pytest.raises(AssertionError):
        k.compute_values(torch.zeros(4, 8, 4, 42)[..., ::2], theta)                # not contiguous
    with pytest.raises(AssertionError):
        k.compute_values(obs, theta, block=512)                                    # above the launch bound
    with pytest.raises(AssertionError):
        k.compute_values(obs, torch.zeros(pguk.net_floats(32, 21, 5)))             # another width's parameters
    with pytest.raises(AssertionError):
        k.gradients(obs, actions.float(), theta, 0.0, 0.1)                         # float actions
    with pytest.raises(AssertionError):
        k.gradients(obs, actions, theta, 0.0, 0.1, partials=torch.zeros(2, 2 * (k.P + 4))[:, ::2])
    with pytest.raises(AssertionError):
        k.discounted_returns(torch.zeros(4, 8, 4), torch.zeros(4, 8, 4, dtype=torch.int32), 0.99)   # done per agent
    with pytest.raises(AssertionError):
        k.apply(theta, theta.clone(), theta.clone(), 1, 1e-3, packed=torch.zeros(k.P - 64 - 1))     # the prefix layout
    assert not rec.launches


_OK = dict(one_launch_rollout=True, gridworld_packing=True, n_policies=2, n_agents=4, head_sizes=[5], fc_dims=[32, 32],
           obs_size=21, dtype=torch.float32, normalize_return=False, normalize_advantage=False, neg_pos_env_ratio=-1,
           world_size=1, algorithm="A2C")


@pytest.mark.parametrize("change,ok,reason", [
    ({}, True, ""),
    ({"fc_dims": [64, 64], "n_agents": 1, "algorithm": "ppo"}, True, ""),
    ({"n_policies": 1, "n_agents": 5, "neg_pos_env_ratio": 0}, True, ""),
    ({"n_policies": 3, "n_agents": 2}, True, ""),
    ({"one_launch_rollout": False}, False, "per tick"),
    ({"gridworld_packing": False}, False, "pack_gridworld_policy"),
    ({"n_agents": 0}, False, "0 agents"),
    ({"head_sizes": [5, 5]}, False, "2 action heads"),
    ({"head_sizes": [4]}, False, "4 actions"),
    ({"head_sizes": [8]}, False, "8 actions"),
    ({"fc_dims": [48, 48]}, False, "hidden width 48"),
    ({"fc_dims": [256, 256]}, False, "hidden width 256"),
    ({"fc_dims": [64, 32]}, False, "unequal widths"),
    ({"fc_dims": [64, 64, 64]}, False, "3 hidden layers"),
    ({"obs_size": 6}, False, "observation size 6"),
    ({"obs_size": 24}, False, "observation size 24"),
    ({"dtype": torch.bfloat16}, False, "float32"),
    ({"normalize_return": True}, False, "normalize_return"),
    ({"normalize_advantage": True}, False, "normalize_advantage"),
    ({"neg_pos_env_ratio": 2}, False, "neg_pos_env_ratio"),
    ({"world_size": 2}, False, "2 ranks"),
    ({"algorithm": "DDPG"}, False, "algorithm DDPG"),
])
def test_gridworld_admission(change, ok, reason):
    got, why = pggk.admitted_gridworld_shape(**{**_OK, **change})
    assert got is ok and (why == "" if ok else reason in why), (got, why)


def test_the_single_agent_admission_answers_as_before():
    ok = dict(one_launch_rollout=True, n_policies=1, n_agents=1, head_sizes=[3], fc_dims=[64, 64], obs_size=6,
              dtype=torch.float32, normalize_return=False, normalize_advantage=False, neg_pos_env_ratio=-1, world_size=1,
              algorithm="A2C")
    assert pguk.admitted_shape(**ok) == (True, "")
    for change, reason in (({"n_policies": 2}, "2 policies"), ({"n_agents": 5}, "5 agents"),
                           ({"obs_size": 3}, "observation size 3"), ({"obs_size": 21}, "observation size 21"),
                           ({"n_policies": 2, "n_agents": 4, "obs_size": 21, "head_sizes": [5]}, "2 policies")):
        got, why = pguk.admitted_shape(**{**ok, **change})
        assert got is False and reason in why, (change, why)
    assert pguk.HIDDEN == (32, 64) and pguk.OBS_SIZES == (2, 4, 6) and len(pguk.all_kernel_names()) == 14


@pytest.mark.parametrize("H", pggk.HIDDEN)
def test_the_packed_layout_model_is_pack_gridworld_policy(H):
    """pack_from_flat(theta) -- what the Apply launch must leave in the packed tensor -- equals pack_gridworld_policy of
    the module holding theta byte for byte, pad columns and tail included; FlatPolicy takes the module as it is"""
    from warp_drive_amd.training.policy_kernel import pack_gridworld_policy

    theta = gc.inputs(gc.CASES[2]._replace(H=H))["theta"]
    model = pc.build_module(H, 21, 5, theta, torch.float32, "cpu")
    want = pack_gridworld_policy(model).numpy()
    got = pggk.pack_from_flat(theta, H)
    assert got.dtype == f32 and got.shape == want.shape == (pggk.packed_floats(H),)
    assert np.array_equal(pc.bits(got), pc.bits(want))
    w0 = got[:24 * H].reshape(H, 24)
    assert not w0[:, 21:].any() and not got[pggk.packed_body_floats(H):].any() and w0[:, :21].all() is not None
    prefilled = torch.full((pggk.packed_floats(H),), float("nan"))
    assert np.array_equal(pc.bits(pack_gridworld_policy(model, out=prefilled).numpy()), pc.bits(want))
    flat = pguk.FlatPolicy(model)
    assert flat.bound() and (flat.H, flat.O, flat.A) == (H, 21, 5) and np.array_equal(flat.flat.numpy(), theta)
    assert np.array_equal(pc.bits(pack_gridworld_policy(model).numpy()), pc.bits(want))


# ------------------------------------------------------------------------------------------------ the yardsticks
@pytest.fixture(scope="module")
def references():
    """per case: inputs, the float64 yardstick, float64 and float32 autograd on the CPU (computed once, never changed)"""
    out = {}
    for case in gc.CASES:
        inp = gc.inputs(case)
        out[case.name] = (inp, gc.yardstick(case, inp), gc.framework(case, inp, torch.float64),
                          gc.framework(case, inp, torch.float32))
    return out


RESULT_KEYS = ("values", "returns", "advantages") + pc.TENSOR_NAMES + pc.SUM_NAMES


def test_cases_cover_what_the_issue_lists():
    shapes = [(c.E, c.T, c.n, gc.case_rows(c), c.grid) for c in gc.CASES]
    assert shapes == [(1, 2, 1, 2, None), (16, 2, 4, 128, None), (13, 5, 4, 260, None), (65, 10, 4, 2600, 3),
                      (33, 5, 1, 165, 5), (64, 10, 1, 640, 2), (16, 5, 4, 320, None)]
    assert [c.gap for c in gc.CASES] == [False] * 6 + [True]
    assert {c.H for c in gc.CASES} == {32, 64} and {c.gamma for c in gc.CASES} == {1.0, 0.98}
    assert {c.ent for c in gc.CASES} == {0.0, 0.05} and {c.vf for c in gc.CASES} == {0.01, 1.0}
    assert {c.algo for c in gc.CASES} == {"A2C", "PPO"} and {c.done for c in gc.CASES} == set(gc.DONE_PATTERNS)
    assert any(c.done == "random" and c.n == 4 for c in gc.CASES) and any(c.envlike for c in gc.CASES)
    by_rows = {gc.case_rows(c): c for c in gc.CASES}
    assert gc.case_tiles(by_rows[2600]) == 21 and gc.case_grid(by_rows[165]) - gc.case_tiles(by_rows[165]) == 3
    assert gc.case_tiles(by_rows[128]) == 1 and gc.case_tiles(by_rows[260]) == 3 and gc.case_tiles(by_rows[640]) == 5
    assert (13 * 4) % 128 and (2 * 13 * 4) < 128 < (3 * 13 * 4)     # the first tile boundary lies inside batch row t = 2
    assert {m for m in gc.MUTATIONS} == set(pc.MUTATIONS) | {"the done flag of replica i % E", "inv_R without n"}


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_inputs_hold_what_the_cases_promise(case, references):
    inp, want, _, _ = references[case.name]
    T, E, n, H = case.T, case.E, case.n, case.H
    net = {k: v.astype(f64) for k, v in pc.unflatten(inp["theta"], H, 21, 5).items()}
    z, _, (_, z1, _, z2, _) = pc.forward64(net, inp["obs"].astype(f64).reshape(-1, 21))
    assert (z1 < 0).any() and (z2 < 0).any() and (z1 > 0).any() and (z2 > 0).any()
    assert (z1[:, [1, H - 2]] == 0).all() and (z2[:, [2, H - 1]] == 0).all()                 # exactly 0 ...
    assert (net["W1"][:, 1] != 0).any() and (net["Wv"][0, [2, H - 1]] != 0).all()            # ... and not dead ends
    assert (net["Wp"][:, [2, H - 1]] != 0).all()
    done, rep = inp["done_env"], inp["done"]
    assert done.shape == (T, E) and rep.shape == (T, E * n)
    assert np.array_equal(rep.reshape(T, E, n), np.broadcast_to(done[..., None], (T, E, n)))
    if case.done == "none":
        assert not done.any()
    elif case.done == "last row":
        assert done[-1].all() and not done[:-1].any()
    elif case.done == "one mid-batch":
        assert done.sum() == 1 and not done[-1].any() and (T == 2 or not done[0].any())
    else:
        assert all((done[:, e] != done[:, e + 1]).any() for e in range(E - 1))               # neighbours differ
        assert done[-1].any() and not done[-1].all() and 0.2 < done.mean() < 0.8
        if n > 1:   # ... so the flags of replica i % E are not those of replica i // n
            assert not np.array_equal(done[:, np.arange(E * n) % E], rep)
    if case.envlike:
        obs = inp["obs"].reshape(T, E, n, 21)
        coords = obs[..., :10] * gc.GRID_CELLS
        assert np.array_equal(coords, np.round(coords)) and coords.min() == 0 and coords.max() == gc.GRID_CELLS
        assert set(np.unique(obs[..., 10:20])) == {0.0, 1.0} and (obs[..., 15:20].sum(-1) == 1).all()
        assert np.array_equal(obs[:, 0, 0, 20], np.arange(T, dtype=f32) / f32(T))
        assert (obs == 0).any() and (obs == 1).any()
    if case.gap:
        top = np.sort(z, axis=1)
        assert np.median(top[:, -1] - top[:, -2]) > 110 and want["probabilities"].min() < 1e-40
    else:
        assert want["probabilities"].min() > 1e-6
    assert all(np.isfinite(np.asarray(want[k])).all() for k in want)
    assert inp["actions"].min() >= 0 and inp["actions"].max() <= 4


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_written_out_float64_pass_agrees_with_float64_autograd(case, references):
    inp, want, auto64, auto32 = references[case.name]
    given = auto32["values"].astype(f32)
    for w, a in ((want, auto64), (gc.yardstick(case, inp, values=given), gc.framework(case, inp, torch.float64, values=given))):
        for key in RESULT_KEYS:
            x, y = np.asarray(w[key], f64), np.asarray(a[key], f64)
            assert x.shape == y.shape or x.size == y.size == 1, (key, x.shape, y.shape)
            scale = max(float(np.abs(y).max()), 1e-300)
            assert float(np.abs(x - y).max()) <= 1e-11 * max(scale, 1.0), (case.name, key)


@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_the_n_agent_returns_model_is_discounted_returns_bit_for_bit(case, references):
    from warp_drive_amd.training.losses import discounted_returns

    inp, _, _, auto32 = references[case.name]
    T, E, n = case.T, case.E, case.n
    v = auto32["values"].astype(f32).reshape(T, E, n)
    r = inp["rewards"].reshape(T, E, n)
    want = discounted_returns(torch.from_numpy(r), torch.from_numpy(inp["done_env"]), torch.from_numpy(v), case.gamma)
    got = gc.returns_model_n(r, inp["done_env"], v, case.gamma, f32)
    assert got.dtype == f32 and np.array_equal(pc.bits(got), pc.bits(want.numpy()))
    # ... and it is the single-agent model on E * n columns with the flags repeated
    flat = pc.returns_model(inp["rewards"], inp["done"], v.reshape(T, E * n), case.gamma, f32)
    assert np.array_equal(pc.bits(got.reshape(T, E * n)), pc.bits(flat))


# ----------------------------------------------------------------------------------------------------- the teeth
def _violations(mutated, want, yard32, keys):
    return [k for k in keys if not pc.compare(np.asarray(mutated[k], f64).reshape(-1), np.asarray(want[k], f64).reshape(-1),
                                              np.asarray(yard32[k], f64).reshape(-1))[0]]


_MUST_BREAK = {
    "relu'(0) = 1": {"b0", "b1"},
    "last tile left out": {"W0", "b0", "W1", "b1"},
    "entropy term dropped": {"Wp", "bp"},
    "inv_R = 1 / E": {"W0", "b0", "W1", "b1", "Wv", "bv"},
    "returns ignore done": {"returns", "advantages", "Wv", "bv"},
    "value gradient without the factor 2": {"Wv", "bv"},
    "the done flag of replica i % E": {"returns", "advantages", "Wv", "bv"},
    "inv_R without n": {"W0", "b0", "W1", "b1", "Wv", "bv"},
}


@pytest.mark.parametrize("mutation", gc.MUTATIONS)
def test_a_planted_defect_breaks_the_bound(mutation, references):
    cases = [c for c in gc.CASES if gc.mutation_applies(c, mutation)]
    assert len(cases) >= 3, mutation
    for case in cases:
        inp, want, _, auto32 = references[case.name]
        broken = set(_violations(gc.yardstick(case, inp, mutate=mutation), want, auto32, RESULT_KEYS))
        assert broken >= _MUST_BREAK[mutation], (mutation, case.name, sorted(broken))


def test_the_unmutated_yardstick_passes_its_own_bound(references):
    for case in gc.CASES:
        _, want, _, auto32 = references[case.name]
        rounded = {k: np.asarray(want[k], f64).astype(f32).astype(f64) for k in RESULT_KEYS}
        assert not _violations(rounded, want, auto32, RESULT_KEYS), case.name


def test_metrics_reshape_by_n():
    """`metrics` on n = 4 agents: the "over agents" standard deviations are real numbers (one agent: NaN, as the framework's)"""
    rec = _Recorder()
    T, E = 3, 5
    for n in (4, 1):
        k = pggk.PgGridworldUpdateKernels(rec, E, T, n, 32, "cpu", compute_units=4)
        g = torch.Generator().manual_seed(n)
        k.values.copy_(torch.randn(T, E, n, generator=g))
        k.returns.copy_(torch.randn(T, E, n, generator=g))
        k.advantages.copy_(k.returns - k.values)
        k.sums.copy_(torch.tensor([1.0, 2.0, 3.0, 4.0]))
        actions = torch.randint(0, 5, (T, E, n, 1), generator=g, dtype=torch.int32)
        m = k.metrics(torch.randn(T, E, n, generator=g), actions, ent_coeff=0.05, vf_coeff=0.5, ppo=False)
        R = T * E * n
        assert m["Policy loss"] == -1.0 / R and m["Mean entropy"] == 2.0 / R and m["Value function loss"] == 3.0 / R
        want = actions.float().std(dim=2).mean().item()
        assert (np.isfinite(m["Std. of action_0 over agents"]) and m["Std. of action_0 over agents"] == want) if n > 1 \
            else np.isnan(m["Std. of action_0 over agents"])
        assert np.isfinite(m["Std. of action_0 over envs"]) and np.isfinite(m["Std. of action_0 over time"])
        assert k.metrics(torch.zeros(T, E, n), actions, 0.05, 0.5, ppo=True)["Policy loss"] == -4.0 / R
