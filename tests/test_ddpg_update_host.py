"""Host side of the DDPG update kernels (no GPU): where the entries live, the wrappers' geometry, the admission rule, and
the yardsticks of tests/test_gpu_ddpg_update.py -- the written-out float64 passes agree with float64 autograd of
training/losses.py::DDPG and a float64 torch.optim.Adam on every case, the returns model equals `n_step_returns` bit for
bit, and each of six planted defects breaks the GPU file's bound on the cases' own inputs."""
import numpy as np
import pytest
import torch

from tests import ddpg_update_cases as dc
from warp_drive_amd.training import ddpg_update_kernels as duk

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge

    ge.build()
    from warp_drive_amd.managers import hip_driver as drv

    return drv


def test_every_entry_is_in_the_ddpg_code_object(built):
    from warp_drive_amd import build as wd_build

    assert wd_build.UNITS["wd_kernels_ddpg.hsaco"] == ("ddpg_update.hip", [])
    manifest = built.manifest()
    names = duk.all_kernel_names()
    assert len(names) == 2 * len(duk.HIDDEN) * len(duk.OBS_SIZES) + 2
    for name in names:
        assert manifest.get(name) == "wd_kernels_ddpg.hsaco", (name, manifest.get(name))
    assert sorted(k for k, v in manifest.items() if v == "wd_kernels_ddpg.hsaco") == names


class _Recorder:
    """stands in for the function manager: every launch is recorded instead of run"""

    def __init__(self):
        self.launches, self.initialised = [], []

    def initialize_functions(self, names):
        self.initialised += list(names)

    def get_function(self, name):
        def launch(*args, block, grid, shared):
            from warp_drive_amd.managers.hip_driver import _pack_args

            _pack_args(args)   # (every argument is something the driver can pass)
            self.launches.append((name, args, block, grid, shared))

        return launch


@pytest.mark.parametrize("compute_units", [256, 4])
@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_wrappers_launch_four_legal_geometries(case, compute_units):
    rec = _Recorder()
    k = duk.DdpgUpdateKernels(rec, case.E, case.T, case.n_step, case.H, case.O, "cpu", compute_units=compute_units)
    assert rec.initialised == duk.kernel_names(case.H, case.O)
    T, E, O, PT = case.T, case.E, case.O, duk.total_floats(case.H, case.O)
    V = T - case.n_step + 1
    assert PT == dc.net_floats(case.H, O) + dc.net_floats(case.H, O + 1) and k.rows == V * E
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    theta, target, m, v = (z(PT) for _ in range(4))
    packed = z(duk.net_floats(case.H, O) + case.H * ((O + 1) // 2 * 2 - O))
    k.targets(z(T, E, 1, O), target, case.scale, case.bias)
    k.gradients(z(T, E, 1, O), z(T, E, 1, 1), z(T, E, 1), z(T, E, dtype=torch.int32), k.next_values, theta, case.gamma,
                case.scale, case.bias)
    k.reduce()
    k.apply(theta, target, m, v, 1, 1e-3, 1e-3, 0.05, max_norm=3.0, packed=packed)
    assert [l[0] for l in rec.launches] == duk.kernel_names(case.H, O) and len(rec.launches) <= 4
    (_, _, b1, g1, s1), (_, _, b2, g2, s2), (_, _, b3, g3, s3), (_, _, b4, g4, s4) = rec.launches
    rows1 = (T - 1) * E
    assert b1[0] in (64, 128, 256) and b1[0] <= duk.TARGETS_MAX_THREADS and 1 <= g1[0] <= -(-rows1 // b1[0])
    assert b1[0] == 64 or -(-rows1 // b1[0]) >= compute_units      # no block larger than keeps every unit busy
    assert s1 == duk.targets_lds_bytes(case.H, O) and s1 % 16 == 0 and s1 <= duk.LDS_LIMIT
    tiles = -(-V * E // duk.TILE)
    assert b2 == (duk.TILE, 1, 1) and g2[0] == min(tiles, compute_units) == k.partials.shape[0] >= 1
    assert s2 == duk.gradients_lds_bytes(case.H, O) and s2 % 16 == 0 and s2 <= duk.LDS_LIMIT
    assert s2 == s1 + 4 * (2 * case.H * duk.LD + 4 * duk.LD + 2 * duk.TILE)
    assert b3 == (duk.REDUCE_THREADS, 1, 1) and g3 == (duk.REDUCE_BLOCKS, 1) and s3 == 0
    assert b4 == (duk.APPLY_THREADS, 1, 1) and (g4[0] - 1) * duk.APPLY_THREADS < PT <= g4[0] * duk.APPLY_THREADS and s4 == 0
    # the sizes the kernels index by
    assert k.next_values.shape == (T - 1, E) and k.returns.shape == (V, E) and k.partials.shape[1] == PT + 2
    assert k.grads.numel() == PT and k.sumsq.numel() == 12 and k.losses.numel() == 2
    offsets = [at for at, _ in duk.tensor_slices(case.H, O)]
    assert offsets == [lo for lo, _ in dc.tensor_bounds(case.H, O)]


def test_wrappers_refuse_what_the_kernels_do_not_take():
    rec = _Recorder()
    with pytest.raises(AssertionError):
        duk.DdpgUpdateKernels(rec, 8, 4, 5, 64, 3, "cpu", compute_units=4)      # T < n_step
    with pytest.raises(AssertionError):
        duk.DdpgUpdateKernels(rec, 8, 4, 2, 48, 3, "cpu", compute_units=4)      # no entry of that width
    k = duk.DdpgUpdateKernels(rec, 8, 4, 2, 64, 3, "cpu", compute_units=4)
    with pytest.raises(AssertionError):
        k.targets(torch.zeros(4, 8, 1, 2), torch.zeros(k.PT), 1.0, 0.0)         # another observation size
    with pytest.raises(AssertionError):
        k.targets(torch.zeros(4, 8, 1, 3), torch.zeros(k.PT), 1.0, 0.0, block=512)   # above the launch bound
    assert not rec.launches


@pytest.mark.parametrize("args,ok,reason", [
    ((1, 1, 3, 1, [64, 64], [64, 64], False), True, ""),
    ((1, 1, 2, 1, [32, 32], [32, 32], False), True, ""),
    ((1, 1, 3, 1, [48, 48], [48, 48], False), False, "hidden width 48"),
    ((1, 1, 3, 1, [64, 32], [64, 32], False), False, "unequal widths"),
    ((1, 1, 3, 1, [64, 64], [32, 32], False), False, "is not the critic's"),
    ((1, 1, 3, 1, [64, 64, 64], [64, 64, 64], False), False, "3 hidden layers"),
    ((1, 1, 3, 1, [64, 64], [64, 64], True), False, "normalize_return"),
    ((2, 1, 3, 1, [64, 64], [64, 64], False), False, "2 policies"),
    ((1, 5, 3, 1, [64, 64], [64, 64], False), False, "5 agents"),
    ((1, 1, 6, 1, [64, 64], [64, 64], False), False, "observation size 6"),
    ((1, 1, 3, 2, [64, 64], [64, 64], False), False, "2 action dimensions"),
])
def test_admission(args, ok, reason):
    got, why = duk.admitted_shape(*args)
    assert got is ok and (why == "" if ok else reason in why), (got, why)


def test_flat_networks_are_views_the_modules_keep_using():
    case = dc.CASES[2]
    inp = dc.inputs(case)
    actor, critic = dc.build_modules(case, inp["theta"], torch.float32, "cpu")
    before = [p.detach().clone() for p in dc.module_parameters(actor, critic)]
    state_keys = list(actor.state_dict())
    flat = duk.FlatNetworks(actor, critic)
    assert flat.bound() and (flat.H, flat.O) == (case.H, case.O)
    assert np.array_equal(flat.flat.numpy(), inp["theta"])                 # the kernels' layout is the cases' layout
    assert all(torch.equal(p, q) for p, q in zip(dc.module_parameters(actor, critic), before))
    assert list(actor.state_dict()) == state_keys
    flat.flat.add_(1.0)                                                    # what a kernel does
    assert all(torch.equal(p, q + 1.0) for p, q in zip(dc.module_parameters(actor, critic), before))
    other, _ = dc.build_modules(case, inp["target"], torch.float32, "cpu")
    actor.load_state_dict(other.state_dict())                              # ... and what a checkpoint load does
    assert flat.bound() and np.array_equal(flat.flat.numpy()[:duk.net_floats(case.H, case.O)],
                                           inp["target"][:duk.net_floats(case.H, case.O)])


# ------------------------------------------------------------------------------------------------ the yardsticks
@pytest.fixture(scope="module")
def references():
    """per case: inputs, the float64 yardstick, float64 and float32 autograd on the CPU (computed once, never changed)"""
    out = {}
    for case in dc.CASES:
        inp = dc.inputs(case)
        out[case.name] = (inp, dc.yardstick(case, inp), dc.framework(case, inp, torch.float64),
                          dc.framework(case, inp, torch.float32))
    return out


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_written_out_float64_passes_agree_with_float64_autograd(case, references):
    _, want, auto64, _ = references[case.name]
    for key in ("next_values", "returns", "critic_loss", "actor_loss") + dc.TENSOR_NAMES:
        a, b = np.asarray(want[key], f64), np.asarray(auto64[key], f64)
        assert a.shape == b.shape or a.size == b.size == 1, (key, a.shape, b.shape)
        scale = max(float(np.abs(b).max()), 1e-300)
        assert float(np.abs(a - b).max()) <= 1e-11 * max(scale, 1.0), (case.name, key)


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_inputs_hold_what_the_cases_promise(case, references):
    inp, want, _, _ = references[case.name]
    actor, critic = dc.unflatten(inp["theta"], case.H, case.O)
    V = case.T - case.n_step + 1
    x = inp["obs"][:V].reshape(-1, case.O).astype(f64)
    z, (_, z1, _, z2, _) = dc._forward({k: v.astype(f64) for k, v in actor.items()}, x)
    assert (z1 < 0).any() and (z2 < 0).any() and (z1 > 0).any() and (z2 > 0).any()
    assert (z1[:, [1, case.H - 2]] == 0).all() and (z2[:, [2, case.H - 1]] == 0).all()       # exactly 0 ...
    assert (actor["W1"][:, 1] != 0).any() and (actor["Wo"][0, [2, case.H - 1]] != 0).all()   # ... and not dead ends
    saturated = np.tanh(z.astype(f32)).astype(f32)
    assert (np.abs(saturated) == 1.0).mean() > (0.5 if case.saturate else -1)
    done = inp["done"]
    if case.done == "none":
        assert not done.any()
    elif case.done == "last row":
        assert done[-1].all() and not done[:-1].any()
    elif case.done == "every row":
        assert (done > 0).all()
    else:
        assert (done > 0).any() and not (done > 0).all()
    assert dc.case_grid(case) >= 1
    assert all(np.isfinite(np.asarray(want[k])).all() for k in want)


def test_cases_cover_what_the_issue_lists():
    assert {c.E for c in dc.CASES} == {1, 63, 64, 65, 257}
    assert {(c.T, c.n_step) for c in dc.CASES} == {(2, 1), (2, 2), (5, 5), (6, 3), (10, 5)}
    assert {c.gamma for c in dc.CASES} == {1.0, 0.99} and {c.H for c in dc.CASES} == {32, 64}
    assert {(c.O, c.scale, c.bias) for c in dc.CASES} == {(2, 1.0, 0.0), (3, 2.0, 0.25)}
    assert {c.done for c in dc.CASES} == set(dc.DONE_PATTERNS) and any(c.saturate for c in dc.CASES)
    tiles = lambda c: -(-(c.T - c.n_step + 1) * c.E // dc.TILE)
    assert any(dc.case_grid(c) < tiles(c) for c in dc.CASES) and any(dc.case_grid(c) > tiles(c) for c in dc.CASES)
    assert {(a.step, a.clip) for a in dc.APPLY_CASES} == {(s, c) for s in (1, 2, 1000) for c in ("active", "inactive", "off")}
    assert all(a.lr_actor != a.lr_critic for a in dc.APPLY_CASES)


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_returns_model_is_n_step_returns_bit_for_bit(case, references):
    from warp_drive_amd.training.losses import DDPG

    inp, _, _, auto32 = references[case.name]
    nv = auto32["next_values"].astype(f32)
    want = DDPG(discount_factor_gamma=case.gamma, n_step=case.n_step).n_step_returns(
        torch.from_numpy(inp["rewards"])[..., None], torch.from_numpy(inp["done"]), torch.from_numpy(nv)[..., None])
    got = dc.returns_model(inp["rewards"], inp["done"], nv, case.n_step, case.gamma, f32)
    assert got.dtype == f32 and np.array_equal(dc.bits(got), dc.bits(want.numpy()[..., 0]))


@pytest.mark.parametrize("ac", dc.APPLY_CASES, ids=lambda a: a.name)
def test_apply_model_agrees_with_float64_torch(ac):
    inp = dc.apply_inputs(ac)
    want, auto64 = dc.apply_model(ac, inp), dc.framework_apply(ac, inp, torch.float64)
    for key in want:
        assert float(np.abs(want[key] - auto64[key]).max()) <= 1e-12, (ac.name, key)
    pa = dc.net_floats(ac.H, ac.O)
    norms = [float(np.sqrt(np.sum(inp["grads"][lo:hi].astype(f64) ** 2))) for lo, hi in ((0, pa), (pa, inp["grads"].size))]
    if ac.clip == "inactive":
        assert max(norms) < 0.5 * ac.max_norm
    else:
        assert min(norms) > 2 * ac.max_norm                      # (clip "off": it WOULD have clipped)
    zero = slice(0, None, dc.ZERO_EVERY)
    # a gradient of exactly 0 on moments of exactly 0, at every step: Adam leaves the parameter and the moments alone
    assert np.array_equal(want["theta"][zero], inp["theta"][zero].astype(f64))
    assert not want["exp_avg"][zero].any() and not want["exp_avg_sq"][zero].any()


# ----------------------------------------------------------------------------------------------------- the teeth
def _violations(case, mutated, want, yard32, keys):
    return [k for k in keys if not dc.compare(np.asarray(mutated[k], f64), want[k], yard32[k])[0]]


@pytest.mark.parametrize("mutation", dc.RETURNS_MUTATIONS)
def test_a_mutated_returns_expression_breaks_the_bound(mutation, references):
    cases = [c for c in dc.CASES if dc.returns_mutation_applies(c, mutation)]
    assert len(cases) >= 3, mutation
    for case in cases:
        inp, want, _, auto32 = references[case.name]
        mutated = dc.yardstick(case, inp, mutate=mutation)
        assert _violations(case, mutated, want, auto32, ["returns"]) == ["returns"], (mutation, case.name)
        # ... and what is built on the returns goes with it
        assert _violations(case, mutated, want, auto32, ["critic.bo", "critic.Wo"]), (mutation, case.name)


@pytest.mark.parametrize("mutation", dc.GRADIENT_MUTATIONS)
@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_a_mutated_gradient_breaks_the_bound(case, mutation, references):
    inp, want, _, auto32 = references[case.name]
    mutated = dc.yardstick(case, inp, mutate=mutation)
    broken = _violations(case, mutated, want, auto32, dc.TENSOR_NAMES)
    if mutation == "critic leak":
        assert set(broken) >= {"critic.W1", "critic.b1", "critic.Wo"} and not [k for k in broken if k.startswith("actor")]
    elif mutation == "relu'(0) = 1":
        assert set(broken) >= {"critic.b0", "critic.b1"}, broken
        if not case.saturate:
            assert set(broken) >= {"actor.b0", "actor.b1"}, broken
    else:
        assert set(broken) >= {"critic.W1", "critic.b1", "critic.W0"}, broken


def test_the_unmutated_yardstick_passes_its_own_bound(references):
    """(the float32 autograd results sit inside the bound by construction; the written-out passes at float32 precision
    -- the yardstick rounded to float32 -- do too: the bound is not so tight that only autograd itself can pass)"""
    for case in dc.CASES:
        _, want, _, auto32 = references[case.name]
        rounded = {k: np.asarray(want[k], f64).astype(f32).astype(f64) for k in dc.TENSOR_NAMES}
        assert not _violations(case, rounded, want, auto32, dc.TENSOR_NAMES), case.name
