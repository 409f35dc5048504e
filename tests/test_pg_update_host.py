"""Host side of the A2C / PPO update kernels (no GPU): where the entries live and what they cost, the wrappers' geometry,
the admission rule, the flat holder, the `"all"` switch, the repack skip, and the yardsticks of
tests/test_gpu_pg_update.py -- the written-out float64 pass agrees with float64 autograd of training/losses.py's A2C and
PPO and with a float64 torch.optim.Adam, and each of six planted defects breaks the GPU file's bound on the cases' own
inputs."""
import re

import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from warp_drive_amd.training import pg_update_kernels as pguk

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge

    ge.build()
    from warp_drive_amd.managers import hip_driver as drv

    return drv


def test_every_entry_is_in_the_pg_code_object(built):
    from warp_drive_amd import build as wd_build

    assert wd_build.UNITS["wd_kernels_pg.hsaco"] == ("pg_update.hip", [])
    manifest = built.manifest()
    names = pguk.all_kernel_names()
    assert len(names) == 2 * len(pguk.HIDDEN) * len(pguk.OBS_SIZES) + 2
    for name in names:
        assert manifest.get(name) == "wd_kernels_pg.hsaco", (name, manifest.get(name))
    assert sorted(k for k, v in manifest.items() if v == "wd_kernels_pg.hsaco") == names
    assert manifest.get(pguk.RETURNS_ENTRY) == "wd_kernels_update.hsaco"      # the existing entry, where it was


def _kernel_metadata(hsaco):
    """{kernel: {field: int}} from the code object's metadata note"""
    import os
    import subprocess
    import tempfile
    from warp_drive_amd import build as wd_build

    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "pg.elf")
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={hsaco}", f"--output={elf}"],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                               text=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        name = re.search(r"^\s{4}\.name:\s+(\S+)$", block, re.M)
        if name is None:
            continue
        out[name.group(1)] = {"." + key: int(re.search(r"^\s{4}\." + key + r":\s+(\d+)$", block, re.M).group(1))
                              for key in ("private_segment_fixed_size", "vgpr_spill_count", "vgpr_count",
                                          "group_segment_fixed_size", "max_flat_workgroup_size")}
    return out


def test_entries_have_no_scratch_and_no_spilled_registers(built):
    import os
    from warp_drive_amd import build as wd_build

    meta = _kernel_metadata(os.path.join(wd_build.CSRC, "wd_kernels_pg.hsaco"))
    assert sorted(meta) == pguk.all_kernel_names()
    for name, fields in meta.items():
        assert fields[".private_segment_fixed_size"] == 0, (name, fields)
        assert fields[".vgpr_spill_count"] == 0, (name, fields)
        assert 0 < fields[".vgpr_count"] <= 512, (name, fields)
        bound = (pguk.TILE if "Gradients" in name else pguk.REDUCE_THREADS if name == "HipPgReduce" else 256)
        assert fields[".max_flat_workgroup_size"] == bound, (name, fields)
    assert meta["HipPgReduce"][".group_segment_fixed_size"] == 4 * pguk.REDUCE_THREADS


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
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_wrappers_launch_five_legal_geometries(case, compute_units):
    rec = _Recorder()
    k = pguk.PgUpdateKernels(rec, case.E, case.T, case.H, case.O, case.A, "cpu", compute_units=compute_units)
    assert rec.initialised == pguk.kernel_names(case.H, case.O)
    T, E, H, O, A = case.T, case.E, case.H, case.O, case.A
    P = pguk.net_floats(H, O, A)
    assert P == pc.net_floats(H, O, A) and k.rows == T * E and k.P == P
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    theta, m, v = (z(P) for _ in range(3))
    packed = z(pguk.packed_floats(H, O, A))
    obs, actions, rewards, done = z(T, E, 1, O), z(T, E, 1, 1, dtype=torch.int32), z(T, E, 1), z(T, E, dtype=torch.int32)
    k.compute_values(obs, theta)
    k.discounted_returns(rewards, done, case.gamma)
    k.gradients(obs, actions, theta, case.ent, case.vf)
    k.reduce()
    k.apply(theta, m, v, 1, 1e-3, max_norm=3.0, packed=packed)
    assert [l[0] for l in rec.launches] == pguk.kernel_names(H, O) and len(rec.launches) == 5
    (_, a1, b1, g1, s1), (_, a2, b2, g2, s2), (_, a3, b3, g3, s3), (_, a4, b4, g4, s4), (_, a5, b5, g5, s5) = rec.launches
    rows = T * E
    assert b1[0] in (64, 128, 256) and b1[0] <= pguk.VALUES_MAX_THREADS and 1 <= g1[0] <= -(-rows // b1[0])
    assert b1[0] == 64 or -(-rows // b1[0]) >= compute_units      # no block larger than keeps every unit busy
    assert s1 == pguk.values_lds_bytes(H, O) and s1 % 16 == 0 and s1 <= pguk.LDS_LIMIT
    assert s1 == 4 * ((pc.net_floats(H, O, 8) + 3) // 4 * 4)
    assert (int(a1[2]), int(a1[3]), int(a1[4]), int(a1[5])) == (rows, H, O, A)
    # the existing returns entry on `values`: rows of width 1 whose column 0 is the value, one "agent"
    assert a2[2] is k.values and (int(a2[3]), int(a2[4])) == (1, 0) and float(a2[5]) == float(f32(case.gamma))
    assert (int(a2[6]), int(a2[7]), int(a2[8])) == (T, E, 1) and a2[9] is k.returns and a2[10] is k.advantages
    assert b2 == (256, 1, 1) and g2 == (-(-E // 256), 1) and s2 == 0
    tiles = -(-rows // pguk.TILE)
    assert b3 == (pguk.TILE, 1, 1) and g3[0] == min(tiles, compute_units) == k.partials.shape[0] >= 1
    assert s3 == pguk.gradients_lds_bytes(H, O) and s3 % 16 == 0 and s3 <= pguk.LDS_LIMIT
    assert s3 == s1 + 4 * pguk.LD * (2 * H + O + 9 + 4)
    assert a3[2] is k.advantages and a3[3] is k.returns
    assert (int(a3[5]), int(a3[6]), int(a3[7]), int(a3[8])) == (rows, H, O, A)
    assert float(a3[9]) == float(f32(1.0 / rows)) and float(a3[10]) == float(f32(case.ent)) and float(a3[11]) == float(f32(case.vf))
    assert b4 == (pguk.REDUCE_THREADS, 1, 1) and g4 == (pguk.REDUCE_BLOCKS, 1) == (9, 1) and s4 == 0
    assert b5 == (pguk.APPLY_THREADS, 1, 1) and (g5[0] - 1) * pguk.APPLY_THREADS < P <= g5[0] * pguk.APPLY_THREADS and s5 == 0
    # the sizes the kernels index by
    assert k.values.shape == k.returns.shape == k.advantages.shape == (T, E) and k.partials.shape[1] == P + 4
    assert k.grads.numel() == P and k.sumsq.numel() == 8 and k.sums.numel() == 4
    assert [at for at, _ in pguk.tensor_slices(H, O, A)] == [lo for lo, _ in pc.tensor_bounds(H, O, A)]
    assert pguk.packed_floats(H, O, A) == pc.tensor_bounds(H, O, A)[5][1]
    assert pguk.gradients_lds_bytes(64, 6) <= pguk.LDS_LIMIT and pguk.TILE == pc.TILE


def test_wrappers_refuse_what_the_kernels_do_not_take():
    rec = _Recorder()
    for bad in ((8, 4, 48, 4, 2), (8, 4, 64, 3, 2), (8, 4, 64, 4, 9), (8, 4, 64, 4, 0)):
        with pytest.raises(AssertionError):
            pguk.PgUpdateKernels(rec, *bad, "cpu", compute_units=4)
    k = pguk.PgUpdateKernels(rec, 8, 4, 64, 4, 2, "cpu", compute_units=4)
    with pytest.raises(AssertionError):
        k.compute_values(torch.zeros(4, 8, 1, 6), torch.zeros(k.P))             # another observation size
    with pytest.raises(AssertionError):
        k.compute_values(torch.zeros(4, 8, 1, 4), torch.zeros(k.P), block=512)  # above the launch bound
    with pytest.raises(AssertionError):
        k.gradients(torch.zeros(4, 8, 1, 4), torch.zeros(4, 8, 1, 1), torch.zeros(k.P), 0.0, 0.1)   # float actions
    assert not rec.launches


_OK = dict(one_launch_rollout=True, n_policies=1, n_agents=1, head_sizes=[3], fc_dims=[64, 64], obs_size=6,
           dtype=torch.float32, normalize_return=False, normalize_advantage=False, neg_pos_env_ratio=-1, world_size=1,
           algorithm="A2C")


@pytest.mark.parametrize("change,ok,reason", [
    ({}, True, ""),
    ({"fc_dims": [32, 32], "obs_size": 2, "head_sizes": [8], "algorithm": "ppo"}, True, ""),
    ({"obs_size": 4, "head_sizes": [1], "neg_pos_env_ratio": 0}, True, ""),
    ({"one_launch_rollout": False}, False, "per tick"),
    ({"n_policies": 2}, False, "2 policies"),
    ({"n_agents": 5}, False, "5 agents"),
    ({"head_sizes": [3, 3]}, False, "2 action heads"),
    ({"head_sizes": [9]}, False, "9 actions"),
    ({"fc_dims": [48, 48]}, False, "hidden width 48"),
    ({"fc_dims": [64, 32]}, False, "unequal widths"),
    ({"fc_dims": [64, 64, 64]}, False, "3 hidden layers"),
    ({"obs_size": 3}, False, "observation size 3"),
    ({"dtype": torch.bfloat16}, False, "float32"),
    ({"normalize_return": True}, False, "normalize_return"),
    ({"normalize_advantage": True}, False, "normalize_advantage"),
    ({"neg_pos_env_ratio": 2}, False, "neg_pos_env_ratio"),
    ({"world_size": 2}, False, "2 ranks"),
    ({"algorithm": "DDPG"}, False, "algorithm DDPG"),
])
def test_admission(change, ok, reason):
    got, why = pguk.admitted_shape(**{**_OK, **change})
    assert got is ok and (why == "" if ok else reason in why), (got, why)


def test_flat_policy_is_views_the_module_keeps_using(tmp_path):
    case = pc.CASES[2]
    inp = pc.inputs(case)
    model = pc.build_module(case.H, case.O, case.A, inp["theta"], torch.float32, "cpu")
    before = [p.detach().clone() for p in pc.module_parameters(model)]
    state_keys = list(model.state_dict())
    flat = pguk.FlatPolicy(model)
    assert flat.bound() and (flat.H, flat.O, flat.A) == (case.H, case.O, case.A)
    assert np.array_equal(flat.flat.numpy(), inp["theta"])                 # the kernels' layout is the cases' layout
    assert all(torch.equal(p, q) for p, q in zip(pc.module_parameters(model), before))
    assert list(model.state_dict()) == state_keys
    # the packed policy of the rollout is a prefix of the flat buffer
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    assert torch.equal(pack_rollout_policy(model), flat.flat[:pguk.packed_floats(case.H, case.O, case.A)])
    flat.flat.add_(1.0)                                                    # what a kernel does
    assert all(torch.equal(p, q + 1.0) for p, q in zip(pc.module_parameters(model), before))
    # a checkpoint round trip: out of the flat module, into a plain one, and back
    path = tmp_path / "shared_7.state_dict"
    torch.save(type(model.state_dict())((k, v.detach().clone()) for k, v in model.state_dict().items()), path)
    plain = pc.build_module(case.H, case.O, case.A, np.zeros_like(inp["theta"]), torch.float32, "cpu")
    plain.load_state_dict(torch.load(path))
    assert all(torch.equal(p, q + 1.0) for p, q in zip(pc.module_parameters(plain), before))
    other = pc.inputs(pc.CASES[2]._replace(seed=99))["theta"]
    versions = [int(p._version) for p in model.parameters()]
    model.load_state_dict(pc.build_module(case.H, case.O, case.A, other, torch.float32, "cpu").state_dict())
    assert flat.bound() and np.array_equal(flat.flat.numpy(), other)
    assert all(int(p._version) > v for p, v in zip(model.parameters(), versions))   # ... which the repack skip sees


# ------------------------------------------------------------------------------------------------ the yardsticks
@pytest.fixture(scope="module")
def references():
    """per case: inputs, the float64 yardstick, float64 and float32 autograd on the CPU (computed once, never changed)"""
    out = {}
    for case in pc.CASES:
        inp = pc.inputs(case)
        out[case.name] = (inp, pc.yardstick(case, inp), pc.framework(case, inp, torch.float64),
                          pc.framework(case, inp, torch.float32))
    return out


RESULT_KEYS = ("values", "returns", "advantages") + pc.TENSOR_NAMES + pc.SUM_NAMES


def test_cases_cover_what_the_issue_lists():
    assert {c.E for c in pc.CASES} == {1, 63, 64, 65, 257} and {c.T for c in pc.CASES} == {2, 5, 10}
    assert {c.H for c in pc.CASES} == {32, 64} and {c.O for c in pc.CASES} == {2, 4, 6} and {c.A for c in pc.CASES} == {1, 2, 3, 8}
    assert {c.gamma for c in pc.CASES} == {1.0, 0.99} and {c.ent for c in pc.CASES} == {0.0, 0.1}
    assert {c.vf for c in pc.CASES} == {0.01, 0.1} and {c.algo for c in pc.CASES} == {"A2C", "PPO"}
    assert {c.done for c in pc.CASES} == set(pc.DONE_PATTERNS) and sum(c.gap for c in pc.CASES) == 1
    assert min(c.E * c.T for c in pc.CASES) == 2
    assert any(c.E * c.T == 2570 and pc.case_tiles(c) == 21 and c.grid == 3 for c in pc.CASES)
    assert {pc.case_grid(c) - pc.case_tiles(c) for c in pc.CASES if c.grid and c.grid > pc.case_tiles(c)} == {1, 2, 3}
    assert any((c.E * c.T) % pc.TILE for c in pc.CASES) and any((c.E * c.T) % pc.TILE == 0 for c in pc.CASES)
    assert {(a.step, a.clip) for a in pc.APPLY_CASES} == {(s, c) for s in (1, 2, 1000) for c in ("active", "inactive", "off")}


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_inputs_hold_what_the_cases_promise(case, references):
    inp, want, _, _ = references[case.name]
    net = {k: v.astype(f64) for k, v in pc.unflatten(inp["theta"], case.H, case.O, case.A).items()}
    z, _, (_, z1, _, z2, _) = pc.forward64(net, inp["obs"].astype(f64).reshape(-1, case.O))
    assert (z1 < 0).any() and (z2 < 0).any() and (z1 > 0).any() and (z2 > 0).any()
    assert (z1[:, [1, case.H - 2]] == 0).all() and (z2[:, [2, case.H - 1]] == 0).all()       # exactly 0 ...
    assert (net["W1"][:, 1] != 0).any() and (net["Wv"][0, [2, case.H - 1]] != 0).all()       # ... and not dead ends
    assert (net["Wp"][:, [2, case.H - 1]] != 0).all()
    done = inp["done"]
    if case.done == "none":
        assert not done.any()
    elif case.done == "last row":
        assert done[-1].all() and not done[:-1].any()
    elif case.done == "value 2":
        assert set(np.unique(done)) == {0, 2}
    else:
        assert done.sum() == 1 and not done[-1].any() and (case.T == 2 or not done[0].any())
    if case.gap:   # the gap between the largest logit and the next exceeds 110 on most rows, on some it does not
        top = np.sort(z, axis=1)
        assert np.median(top[:, -1] - top[:, -2]) > 110 and (top[:, -1] - top[:, 0] > 110).all()
        assert want["probabilities"].min() < 1e-40
    else:          # ... and everywhere else every probability is far above Categorical's clamp at float32 eps
        assert want["probabilities"].min() > 1e-6
    assert all(np.isfinite(np.asarray(want[k])).all() for k in want)
    assert inp["actions"].min() >= 0 and inp["actions"].max() <= case.A - 1


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_written_out_float64_pass_agrees_with_float64_autograd(case, references):
    """training/losses.py's A2C and PPO objects, end to end, and the same objective on GIVEN values (what the GPU file
    hands the gradient stage)"""
    inp, want, auto64, auto32 = references[case.name]
    given = auto32["values"].astype(f32)
    for w, a in ((want, auto64), (pc.yardstick(case, inp, values=given), pc.framework(case, inp, torch.float64, values=given))):
        for key in RESULT_KEYS:
            x, y = np.asarray(w[key], f64), np.asarray(a[key], f64)
            assert x.shape == y.shape or x.size == y.size == 1, (key, x.shape, y.shape)
            scale = max(float(np.abs(y).max()), 1e-300)
            assert float(np.abs(x - y).max()) <= 1e-11 * max(scale, 1.0), (case.name, key)
        assert abs(pc.loss_terms(case, w)[0] - a["loss"]) <= 1e-11 * max(1.0, abs(a["loss"])), case.name


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_returns_model_is_discounted_returns_bit_for_bit(case, references):
    from warp_drive_amd.training.losses import discounted_returns

    inp, _, _, auto32 = references[case.name]
    v = auto32["values"].astype(f32)
    want = discounted_returns(torch.from_numpy(inp["rewards"])[..., None], torch.from_numpy(inp["done"]),
                              torch.from_numpy(v)[..., None], case.gamma)
    got = pc.returns_model(inp["rewards"], inp["done"], v, case.gamma, f32)
    assert got.dtype == f32 and np.array_equal(pc.bits(got), pc.bits(want.numpy()[..., 0]))


@pytest.mark.parametrize("ac", pc.APPLY_CASES, ids=lambda a: a.name)
def test_apply_model_agrees_with_float64_torch(ac):
    inp = pc.apply_inputs(ac)
    want, auto64 = pc.apply_model(ac, inp), pc.framework_apply(ac, inp, torch.float64)
    for key in want:
        assert float(np.abs(want[key] - auto64[key]).max()) <= 1e-12, (ac.name, key)
    norm = float(np.sqrt(np.sum(inp["grads"].astype(f64) ** 2)))
    if ac.clip == "inactive":
        assert norm < 0.5 * ac.max_norm
    else:
        assert norm > 2 * ac.max_norm                      # (clip "off": it WOULD have clipped)
    zero = slice(0, None, pc.ZERO_EVERY)
    # a gradient of exactly 0 on moments of exactly 0, at every step: Adam leaves the parameter and the moments alone
    assert np.array_equal(want["theta"][zero], inp["theta"][zero].astype(f64))
    assert not want["exp_avg"][zero].any() and not want["exp_avg_sq"][zero].any()


# ----------------------------------------------------------------------------------------------------- the teeth
def _violations(mutated, want, yard32, keys):
    return [k for k in keys if not pc.compare(np.asarray(mutated[k], f64).reshape(-1), np.asarray(want[k], f64).reshape(-1),
                                              np.asarray(yard32[k], f64).reshape(-1))[0]]


_MUST_BREAK = {
    "relu'(0) = 1": {"b0", "b1"},
    "last tile left out": {"W0", "b0", "W1", "b1"},   # (the value head's share of the last tile can be exactly 0: ret = v)
    "entropy term dropped": {"Wp", "bp"},
    "inv_R = 1 / E": {"W0", "b0", "W1", "b1", "Wv", "bv"},
    "returns ignore done": {"returns", "advantages", "Wv", "bv"},
    "value gradient without the factor 2": {"Wv", "bv"},
}


@pytest.mark.parametrize("mutation", pc.MUTATIONS)
def test_a_planted_defect_breaks_the_bound(mutation, references):
    cases = [c for c in pc.CASES if pc.mutation_applies(c, mutation)]
    assert len(cases) >= 5, mutation
    for case in cases:
        inp, want, _, auto32 = references[case.name]
        broken = set(_violations(pc.yardstick(case, inp, mutate=mutation), want, auto32, RESULT_KEYS))
        assert broken >= _MUST_BREAK[mutation], (mutation, case.name, sorted(broken))


def test_the_unmutated_yardstick_passes_its_own_bound(references):
    """(the float32 autograd results sit inside the bound by construction; the written-out pass at float32 precision --
    the yardstick rounded to float32 -- does too: the bound is not so tight that only autograd itself can pass)"""
    for case in pc.CASES:
        _, want, _, auto32 = references[case.name]
        rounded = {k: np.asarray(want[k], f64).astype(f32).astype(f64) for k in RESULT_KEYS}
        assert not _violations(rounded, want, auto32, RESULT_KEYS), case.name


# ------------------------------------------------------------------------------------- the switch and the repack skip
class _StubTrainer:
    """what Trainer._generate_rollout_batch_in_one_launch touches before the launch, on the CPU"""

    def __init__(self, model):
        from warp_drive_amd.training.policy_kernel import pack_rollout_policy

        self.policies, self.models = ["shared"], {"shared": model}
        self.packs = 0

        def pack(m, out=None):
            self.packs += 1
            return pack_rollout_policy(m, out=out)

        self._batch_rollout = {"packed": {"shared": pack_rollout_policy(model)}, "pack": pack, "split": None}

        class _Stop(Exception):
            pass

        class _Engine:
            def run(self, n):
                raise _Stop

        self.engine, self.stop = _Engine(), _Stop

    def rollout(self):
        from warp_drive_amd.training.trainer import Trainer

        with pytest.raises(self.stop):
            Trainer._generate_rollout_batch_in_one_launch(self)


def test_the_repack_is_skipped_after_a_refill_and_not_after_a_framework_side_change():
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy, parameter_versions

    case = pc.CASES[2]
    model = pc.build_module(case.H, case.O, case.A, pc.inputs(case)["theta"], torch.float32, "cpu")
    flat = pguk.FlatPolicy(model)
    tr = _StubTrainer(model)
    packed = tr._batch_rollout["packed"]["shared"]
    tr.rollout()
    assert tr.packs == 1                                           # nothing was refilled yet: the framework's repack
    # what an Apply launch does: the parameters and the packed tensor change together, no version counter moves
    flat.flat.data.mul_(0.5)
    packed.copy_(flat.flat[:packed.numel()])
    tr._batch_rollout["refilled"] = {"shared": parameter_versions(model)}
    tr.rollout()
    tr.rollout()
    assert tr.packs == 1 and torch.equal(packed, pack_rollout_policy(model))   # skipped; the bytes are the repack's
    other = pc.inputs(case._replace(seed=77))["theta"]
    model.load_state_dict(pc.build_module(case.H, case.O, case.A, other, torch.float32, "cpu").state_dict())
    assert not torch.equal(packed, pack_rollout_policy(model))
    tr.rollout()
    assert tr.packs == 2 and torch.equal(packed, pack_rollout_policy(model))   # a framework-side change: repacked
    assert "shared" not in tr._batch_rollout["refilled"]
    tr.rollout()
    assert tr.packs == 3                                           # ... and it stays so until the next refill
    with torch.no_grad():
        model.vf_head.bias.add_(1.0)                               # a manual edit after a refill
    tr._batch_rollout["refilled"] = {"shared": tuple(v - (i == 7) for i, v in enumerate(parameter_versions(model)))}
    tr.rollout()
    assert tr.packs == 4
    # an edit through `.data` moves no counter: the skip does not see it until it is announced
    from warp_drive_amd.training.trainer import Trainer

    tr._batch_rollout["refilled"] = {"shared": parameter_versions(model)}
    tr._fused_forward = {"shared": None}
    model.vf_head.weight.data.mul_(2.0)
    model.fc["0"][0].weight.data.mul_(2.0)
    assert tr._batch_rollout["refilled"]["shared"] == parameter_versions(model)
    tr.rollout()
    assert tr.packs == 4 and not torch.equal(packed, pack_rollout_policy(model))
    model._inference_cache["x"] = None
    Trainer.mark_parameters_changed(tr)
    assert model._inference_cache == {}
    tr.rollout()
    assert tr.packs == 5 and torch.equal(packed, pack_rollout_policy(model))


class _NoDevice:
    """an env wrapper that says "hip" and has nothing else: whatever touches it beyond that raises AttributeError"""
    env_backend = "hip"


@pytest.mark.parametrize("algorithm", ["A2C", "DDPG"])
def test_another_string_is_refused_before_anything_touches_the_device(algorithm):
    from warp_drive_amd.training.trainer import Trainer
    from warp_drive_amd.training.trainer_ddpg import TrainerDDPG

    cls = TrainerDDPG if algorithm == "DDPG" else Trainer
    config = lambda value: {"trainer": {"fused_update": value, "num_envs": 4, "train_batch_size": 8, "num_episodes": 1},
                            "policy": {"shared": {"algorithm": algorithm}}}
    for value in ("everything", "ALL", "true", ""):
        with pytest.raises(ValueError, match="trainer.fused_update: True, False or \"all\""):
            cls(env_wrapper=_NoDevice(), config=config(value))
    for value in ("all", True, False):   # accepted: the constructor goes on to the wrapper, which this one does not have
        with pytest.raises(AttributeError):
            cls(env_wrapper=_NoDevice(), config=config(value))


def test_the_shipped_default_is_what_it_was():
    import yaml
    from warp_drive_amd.training import trainer

    defaults = yaml.safe_load(open(trainer._DEFAULT_CONFIG))
    assert defaults["trainer"]["fused_update"] is True
    assert not isinstance(getattr(trainer.Trainer, "update_path", None), dict)   # per trainer, set in __init__
