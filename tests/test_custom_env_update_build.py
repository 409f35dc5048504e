"""The update kernels of a custom environment without a GPU (include/wd_env_update.h;
training/pg_update_custom_kernels.py; utils/custom_tick.py::FusedUpdateMixin): the worked example and the probes compile to
exactly their entries, without scratch memory or spilled vector registers and with the launch bounds the wrappers launch
by -- the largest observation size at both widths included; the wrappers pack exactly the kernarg layout the compiled
entries declare; the host's LDS formulas equal the literals the probe sources assert; admission accepts what is served and
names every refusal; and the yardstick of tests/test_gpu_custom_env_update.py -- tests/pg_update_cases.py's float64 pass on
E * n columns at the new F and A -- agrees with float64 autograd, holds float32 autograd under the bound, and catches each of
eight planted defects on every case it applies to.  hipcc cross-compiles gfx950, so no GPU is needed."""
import os
import re

import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests import pg_update_custom_cases as cc
from tests.custom_envs import update_probe
from tests.test_custom_env_rollout_build import _metadata, _sha
from tests.test_pg_update_host import _Recorder
from warp_drive_amd import build as wd_build
from warp_drive_amd.training import pg_update_custom_kernels as pgck
from warp_drive_amd.training import pg_update_kernels as pguk

f32, f64 = np.float32, np.float64
ROOT = cc.ROOT
HEADER = os.path.join(ROOT, "include", "wd_env_update.h")
COMMON = os.path.join(wd_build.KDIR, "pg_update_common.h")
ROLLOUT_ENTRIES = ["HipRendezvousUpdateRollout_H32", "HipRendezvousUpdateRollout_H64", "HipRendezvousUpdateStep",
                   "HipRendezvousUpdateTick"]
# unit -> (source, F, entry prefix, the entries besides the update's)
UNITS = {cc.EXAMPLE_UNIT: (cc.EXAMPLE_SOURCE, cc.EXAMPLE_OBS, cc.EXAMPLE_PREFIX, ROLLOUT_ENTRIES)}
UNITS.update({name: (*spec, []) for name, spec in update_probe.UNITS.items()})

_CACHE = []


@pytest.fixture(autouse=True)
def cache(tmp_path_factory, monkeypatch):
    """one cache directory for the module: each unit compiles once"""
    if not _CACHE:
        _CACHE.append(str(tmp_path_factory.mktemp("env_cache")))
    monkeypatch.setenv("WD_ENV_CACHE", _CACHE[0])
    return _CACHE[0]


def _update_entries(prefix):
    return [f"{prefix}Apply", f"{prefix}Gradients_H32", f"{prefix}Gradients_H64", f"{prefix}Reduce", f"{prefix}Values_H32",
            f"{prefix}Values_H64"]


def _example_class():
    import importlib.util
    import sys

    name = "rendezvous_update_example"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(cc.EXAMPLE_SOURCE),
                                                                         "rendezvous_update.py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name].RendezvousUpdate


# ------------------------------------------------------------------------------------------------------ the build
@pytest.mark.parametrize("unit", sorted(UNITS))
def test_the_units_build_to_exactly_their_entries_without_scratch(cache, unit):
    source, F, prefix, others = UNITS[unit]
    manifest_before = _sha(wd_build.MANIFEST)
    in_tree_before = sorted(os.listdir(wd_build.CSRC))
    path = wd_build.build_env_unit(unit, source)
    assert pgck.all_kernel_names(prefix) == _update_entries(prefix)
    assert os.path.dirname(path) == cache and wd_build.kernels_in(path) == sorted(_update_entries(prefix) + others)
    assert _sha(wd_build.MANIFEST) == manifest_before and sorted(os.listdir(wd_build.CSRC)) == in_tree_before
    # the kit and the one statement of the parity contract it includes are part of the unit's content hash
    sources = wd_build.unit_sources(source, [f[2:] for f in wd_build.env_unit_flags(source) if f.startswith("-I")])
    assert HEADER in sources and COMMON in sources
    meta = _metadata(path)
    assert sorted(meta) == sorted(_update_entries(prefix) + others)
    for H in pgck.HIDDEN:
        names = pgck.kernel_names(prefix, H)
        bounds = dict(zip((names[0], names[2], names[3], names[4]),
                          (pguk.VALUES_MAX_THREADS, pguk.TILE, pguk.REDUCE_THREADS, pguk.APPLY_THREADS)))
        assert list(bounds.values()) == [256, 128, 1024, 256]
        for name, bound in bounds.items():
            m = meta[name]
            print(f"{name}: {m['vgprs']} VGPRs, private {m['private']}, spills {m['vgpr_spills']} (vector) / "
                  f"{m['sgpr_spills']} (scalar, to vector registers), static LDS {m['lds']}, at most {m['max_threads']} threads")
            assert (m["private"], m["vgpr_spills"]) == (0, 0), name
            assert m["max_threads"] == bound and 0 < m["vgprs"] <= 512 // max(1, bound // 128), name
        assert meta[names[3]]["lds"] == 4 * pguk.REDUCE_THREADS
        assert meta[names[0]]["lds"] == meta[names[2]]["lds"] == meta[names[4]]["lds"] == 0    # all of theirs is dynamic


def test_the_kit_restates_nothing_and_the_rest_of_the_tree_is_as_it_was():
    text = open(HEADER).read()
    assert set(re.findall(r"^\s*#include\s+(\S+)", text, re.M)) == {'"pg_update_common.h"'}
    code = re.sub(r"//.*", "", text)
    assert code.count("asm") == 1 and 'asm volatile("" ::: "memory")' in code      # the empty compiler barrier alone
    assert "atomic" not in code.lower() and "shfl" not in code
    for shared in ("upd_layer1_and_value", "upd_positive_mask", "upd_stage", "upd_layer1_backward", "upd_acc_w1", "upd_acc_w0",
                   "upd_pg_reduce", "upd_clip_adam", "upd_pg_net_floats", "upd_pad4"):
        assert shared in code and not re.search(r"(void|float|int|uint64_t)\s+" + shared + r"\s*\(", code), shared
    assert "static_assert(F >= 1 && F <= WD_UPD_MAX_OBS" in code and "#define WD_UPD_MAX_OBS 32" in code
    assert pgck.MAX_OBS == 32
    # not part of the in-tree build; the trainer names no class of a custom environment
    assert not any("rendezvous" in unit.lower() or "probe" in unit.lower() for unit, _ in wd_build.UNITS.values())
    owners = wd_build.in_tree_kernel_owners()
    assert not [k for _, _, prefix, others in UNITS.values() for k in _update_entries(prefix) + others if k in owners]
    trainer = open(os.path.join(ROOT, "warp_drive_amd", "training", "trainer.py")).read()
    assert "Rendezvous" not in trainer and "FusedUpdateMixin" not in trainer and "PgCustomUpdateKernels" not in trainer
    assert sorted(f for f in os.listdir(os.path.dirname(cc.EXAMPLE_SOURCE)) if f != "__pycache__") == [
        "rendezvous_update.hip", "rendezvous_update.py"]
    source = open(cc.EXAMPLE_SOURCE).read()
    assert "WD_PG_UPDATE_ENTRIES(RendezvousUpdate, 5)" in source and "rendezvous_policy" not in re.sub(r"//.*", "", source)


# --------------------------------------------------------------------------------------- LDS: literals and formulas
def test_the_lds_formulas_are_the_literals_the_sources_assert():
    for (H, F), (values, gradients) in update_probe.LDS_FLOATS.items():
        assert pgck.values_lds_bytes(H, F) == 4 * values and pgck.gradients_lds_bytes(H, F) == 4 * gradients, (H, F)
        assert gradients - values == pguk.LD * (2 * H + F + 9 + 4) and values % 4 == 0 and gradients % 4 == 0
        assert 4 * gradients <= pguk.LDS_LIMIT
    assert {F for _, F in update_probe.LDS_FLOATS} == {F for _, F, _ in update_probe.UNITS.values()} == {1, 7, 32}
    for source, F, _ in update_probe.UNITS.values():
        text = open(source).read()
        for H in (32, 64):
            values, gradients = update_probe.LDS_FLOATS[(H, F)]
            assert f"wd_pg_values_lds_floats({H}, {F}) == {values}" in text, (source, H)
            assert f"wd_pg_gradients_lds_floats({H}, {F}) == {gradients}" in text, (source, H)
        assert f", {F})" in text.split("WD_PG_UPDATE_ENTRIES(")[-1]
    # the network's copy, written out: W0 with rows of pad4(F), b0, W1, b1, eight head rows, eight bias slots, Wv, bv
    for H in (32, 64):
        for F in range(1, 33):
            net = ((F + 3) // 4 * 4) * H + H + H * H + H + 8 * H + 8 + H + 1
            assert pgck.values_lds_bytes(H, F) == 4 * ((net + 3) // 4 * 4)
            assert pgck.gradients_lds_bytes(H, F) <= pguk.LDS_LIMIT
    # at an even observation size without pad columns the network's copy is pg_update.hip's
    for H in (32, 64):
        assert pgck.values_lds_bytes(H, 4) == pguk.values_lds_bytes(H, 4)
        assert pgck.gradients_lds_bytes(H, 4) == pguk.gradients_lds_bytes(H, 4)


# ------------------------------------------------------------------------------------- the wrappers and the kernargs
@pytest.mark.parametrize("compute_units,blocks_per_cu", [(256, None), (4, None), (4, 2)])
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_wrappers_launch_five_legal_geometries(case, compute_units, blocks_per_cu):
    rec = _Recorder()
    T, E, n, H, F, A = case.T, case.E, case.n, case.H, case.F, case.A
    _, _, prefix = cc.unit_of(F)
    k = pgck.PgCustomUpdateKernels(rec, prefix, E, T, n, H, F, A, "cpu", compute_units=compute_units,
                                   blocks_per_cu=blocks_per_cu)
    assert rec.initialised == pgck.kernel_names(prefix, H)
    P, rows = pc.net_floats(H, F, A), T * E * n
    assert k.P == P and k.rows == rows == cc.case_rows(case) and k.packed_floats == P - H - 1
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)   # noqa: E731
    theta, m, v, packed = z(P), z(P), z(P), z(P - H - 1)
    obs, actions, rewards, done = z(T, E, n, F), z(T, E, n, 1, dtype=torch.int32), z(T, E, n), z(T, E, dtype=torch.int32)
    k.compute_values(obs, theta)
    k.discounted_returns(rewards, done, case.gamma)
    k.gradients(obs, actions, theta, case.ent, case.vf)
    k.reduce()
    k.apply(theta, m, v, 1, 1e-3, max_norm=3.0, packed=packed)
    assert [l[0] for l in rec.launches] == pgck.kernel_names(prefix, H)
    (_, a1, b1, g1, s1), (_, a2, b2, g2, s2), (_, a3, b3, g3, s3), (_, a4, b4, g4, s4), (_, a5, b5, g5, s5) = rec.launches
    assert b1[0] in (64, 128, 256) and 1 <= g1[0] <= -(-rows // b1[0]) and s1 == pgck.values_lds_bytes(H, F)
    assert len(a1) == 5 and int(a1[2]) == rows and int(a1[3]) == A and a1[4] is k.values
    assert a2[2] is k.values and (int(a2[6]), int(a2[7]), int(a2[8])) == (T, E, n) and b2 == (256, 1, 1)
    assert g2 == (-(-E * n // 256), 1) and s2 == 0
    tiles = -(-rows // pguk.TILE)
    per_cu = {32: 2, 64: 1}[H] if blocks_per_cu is None else blocks_per_cu
    assert b3 == (pguk.TILE, 1, 1) and g3[0] == min(tiles, per_cu * compute_units) == k.partials.shape[0] >= 1
    assert k.partials.shape == (g3[0], P + 4) and s3 == pgck.gradients_lds_bytes(H, F) <= pguk.LDS_LIMIT and s3 % 16 == 0
    assert len(a3) == 11 and a3[2] is k.advantages and a3[3] is k.returns and int(a3[5]) == rows and int(a3[6]) == A
    assert float(a3[7]) == float(f32(1.0 / rows)) and float(a3[8]) == float(f32(case.ent)) and a3[10] is k.partials
    assert b4 == (1024, 1, 1) and g4 == (9, 1) and s4 == 0 and (int(a4[1]), int(a4[2]), int(a4[3])) == (g3[0], H, A)
    assert b5 == (256, 1, 1) and s5 == 0 and (int(a5[6]), int(a5[7])) == (H, A) and a5[5] is packed
    assert g5[0] * 256 >= P > (g5[0] - 1) * 256


def test_the_default_grid_is_what_was_measured():
    """docs/rounds/r39.md: two blocks per compute unit where two are resident in its LDS (width 32, whatever F), one
    elsewhere (width 64: `_setup`'s geometry as it is)"""
    rec = _Recorder()
    for F in (1, 5, 7, 32):
        assert pgck.default_blocks_per_cu(32, F) == 2 and 2 * pgck.gradients_lds_bytes(32, F) <= pguk.LDS_LIMIT
        assert pgck.default_blocks_per_cu(64, F) == 1 and 2 * pgck.gradients_lds_bytes(64, F) > pguk.LDS_LIMIT
    k = pgck.PgCustomUpdateKernels(rec, "HipXPg", 2000, 20, 100, 32, 5, 5, "cpu", compute_units=256)
    assert k.rows == 4_000_000 and k.gradients_grid == 512 and k.partials.shape[0] == 512 and k.blocks_per_cu == 2
    k1 = pgck.PgCustomUpdateKernels(rec, "HipXPg", 2000, 20, 100, 32, 5, 5, "cpu", compute_units=256, blocks_per_cu=1)
    assert k1.gradients_grid == 256 == k1.partials.shape[0]
    k64 = pgck.PgCustomUpdateKernels(rec, "HipXPg", 2000, 20, 100, 64, 5, 5, "cpu", compute_units=256)
    assert k64.gradients_grid == 256 == k64.partials.shape[0] and k64.blocks_per_cu == 1
    for bad in ((48, 5, 5), (32, 0, 5), (32, 33, 5), (32, 5, 0), (32, 5, 9)):
        with pytest.raises(AssertionError):
            pgck.PgCustomUpdateKernels(rec, "HipXPg", 4, 4, 4, *bad, "cpu", compute_units=4)
    with pytest.raises(AssertionError):
        pgck.PgCustomUpdateKernels(rec, "HipXPg", 4, 4, 4, 32, 5, 5, "cpu", compute_units=4, blocks_per_cu=0)
    with pytest.raises(AssertionError):
        k.compute_values(torch.zeros(20, 2000, 100, 6), torch.zeros(k.P))          # another observation size


@pytest.mark.parametrize("unit,H,A", [(cc.EXAMPLE_UNIT, 32, 5), (cc.EXAMPLE_UNIT, 64, 8), ("UpdateProbeF1", 64, 1),
                                      ("UpdateProbe", 32, 2)])
def test_the_wrappers_pack_the_kernarg_layout_of_the_compiled_entries(unit, H, A):
    from warp_drive_amd.managers import hip_driver as drv

    source, F, prefix, _ = UNITS[unit]
    meta = _metadata(wd_build.build_env_unit(unit, source))
    rec = _Recorder()
    E, T, n = 3, 4, 5
    k = pgck.PgCustomUpdateKernels(rec, prefix, E, T, n, H, F, A, "cpu", compute_units=4)
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)   # noqa: E731
    theta, m, v, packed = z(k.P), z(k.P), z(k.P), z(k.packed_floats)
    k.compute_values(z(T, E, n, F), theta)
    k.discounted_returns(z(T, E, n), z(T, E, dtype=torch.int32), 0.98)
    k.gradients(z(T, E, n, F), z(T, E, n, 1, dtype=torch.int32), theta, 0.05, 1.0)
    k.reduce()
    k.apply(theta, m, v, 1, 1e-3, max_norm=3.0, packed=packed)
    k.apply(theta, m, v, 2, 1e-3, packed=None)                          # a null packed pointer is a pointer too
    checked = 0
    for name, args, _, _, _ in rec.launches:
        if name == pguk.RETURNS_ENTRY:
            continue
        explicit = [a for a in meta[name]["args"] if not a[2].startswith("hidden_")]
        offset, layout = 0, []
        for a in args:
            pointer = hasattr(a, "data_ptr") or isinstance(a, (drv.DevicePtr, np.uint64))
            size = 8 if pointer else a.dtype.itemsize
            offset += (-offset) % size
            layout.append((offset, size, "global_buffer" if pointer else "by_value"))
            offset += size
        assert layout == explicit, (name, layout, explicit)
        assert len(drv._pack_args(args)) == max(o + s for o, s, _ in explicit)
        checked += 1
    assert checked == 5
    # the entries' own argument counts: (obs, theta, rows, A, values), eleven, seven, fifteen
    counts = [len([a for a in meta[nm]["args"] if not a[2].startswith("hidden_")]) for nm in
              (pgck.kernel_names(prefix, H)[i] for i in (0, 2, 3, 4))]
    assert counts == [5, 11, 7, 15]


# ------------------------------------------------------------------------------------------------------ admission
_OK = dict(one_launch_rollout=True, rollout_packing=True, n_policies=1, n_agents=100, head_sizes=[5], fc_dims=[32, 32],
           obs_size=5, dtype=torch.float32, normalize_return=False, normalize_advantage=False, neg_pos_env_ratio=-1,
           world_size=1, algorithm="A2C")


@pytest.mark.parametrize("change,ok,reason", [
    ({}, True, ""),
    ({"fc_dims": [64, 64], "n_agents": 1, "algorithm": "ppo", "head_sizes": [8], "obs_size": 32}, True, ""),
    ({"obs_size": 1, "head_sizes": [1], "neg_pos_env_ratio": 0}, True, ""),
    ({"n_policies": 2}, False, "2 policies"),
    ({"n_agents": 0}, False, "0 agents"),
    ({"head_sizes": [5, 5]}, False, "2 action heads"),
    ({"head_sizes": [0]}, False, "0 actions"),
    ({"head_sizes": [9]}, False, "9 actions"),
    ({"obs_size": 0}, False, "observation size 0"),
    ({"obs_size": 33}, False, "observation size 33"),
    ({"fc_dims": [48, 48]}, False, "hidden width 48"),
    ({"fc_dims": [64, 32]}, False, "unequal widths"),
    ({"fc_dims": [64, 64, 64]}, False, "3 hidden layers"),
    ({"dtype": torch.bfloat16}, False, "float32"),
    ({"normalize_return": True}, False, "normalize_return"),
    ({"normalize_advantage": True}, False, "normalize_advantage"),
    ({"neg_pos_env_ratio": 2}, False, "neg_pos_env_ratio"),
    ({"world_size": 2}, False, "2 ranks"),
    ({"algorithm": "DDPG"}, False, "algorithm DDPG"),
    ({"one_launch_rollout": False}, False, "per tick"),
    ({"rollout_packing": False}, False, "pack_rollout_policy"),
])
def test_custom_admission(change, ok, reason):
    got, why = pgck.admitted_custom_shape(**{**_OK, **change})
    assert got is ok and (why == "" if ok else reason in why), (got, why)


def test_an_lds_size_over_the_limit_is_refused_by_name(monkeypatch):
    monkeypatch.setattr(pgck, "LDS_LIMIT", pgck.gradients_lds_bytes(64, 5) - 1)
    assert pgck.admitted_custom_shape(**_OK) == (True, "")
    got, why = pgck.admitted_custom_shape(**{**_OK, "fc_dims": [64, 64]})
    assert got is False and "bytes of LDS" in why


class _Functions:
    def __init__(self, missing=()):
        self.missing = set(missing)

    def has_function(self, name):
        return name not in self.missing

    def initialize_functions(self, names):
        pass

    def get_function(self, name):
        return name


def test_the_mixin_answers_for_the_entries_of_its_code_object():
    from warp_drive_amd.rollout import UnsupportedRolloutShape
    from warp_drive_amd.utils.custom_tick import FusedRolloutMixin, FusedUpdateMixin

    cls = _example_class()
    assert issubclass(cls, FusedUpdateMixin) and issubclass(FusedUpdateMixin, FusedRolloutMixin)
    assert (cls.UPDATE_KERNEL_PREFIX, cls.UPDATE_OBS_SIZE) == (cc.EXAMPLE_PREFIX, 5)
    assert FusedUpdateMixin.UPDATE_KERNEL_PREFIX is None
    env = cls(num_agents=5, grid_length=4, episode_length=4)
    env.cuda_function_manager = _Functions()
    assert env.update_kernels_refusal(32, 5, 5) == (True, "") and env.update_kernels_refusal(64, 5, 1) == (True, "")
    for args, reason in (((48, 5, 5), "hidden width 48"), ((32, 5, 0), "0 actions"), ((32, 5, 9), "9 actions"),
                         ((32, 6, 5), "compiled for 5"), ((32, 4, 5), "observation size 4")):
        ok, why = env.update_kernels_refusal(*args)
        assert ok is False and reason in why, (args, why)
    for missing in pgck.all_kernel_names(cc.EXAMPLE_PREFIX):
        env.cuda_function_manager = _Functions([missing])
        ok, why = env.update_kernels_refusal(32, 5, 5)
        assert ok is False and missing in why
        with pytest.raises(UnsupportedRolloutShape, match=missing):
            env.update_kernels(4, 6, 5, 32, 5, 5, "cpu", compute_units=4)
    env.cuda_function_manager = _Functions()
    k = env.update_kernels(4, 6, 5, 32, 5, 5, "cpu", compute_units=4)
    assert isinstance(k, pgck.PgCustomUpdateKernels) and (k.E, k.T, k.n, k.H, k.O, k.A) == (4, 6, 5, 32, 5, 5)
    assert k.names == pgck.kernel_names(cc.EXAMPLE_PREFIX, 32) and k.blocks_per_cu == pgck.default_blocks_per_cu(32, 5)

    class Nameless(FusedUpdateMixin):
        cuda_function_manager = _Functions()

    ok, why = Nameless().update_kernels_refusal(32, 5, 5)
    assert ok is False and "UPDATE_KERNEL_PREFIX" in why
    # an env with the rollout mixin alone offers nothing: the trainer's third branch finds no such method
    assert not hasattr(FusedRolloutMixin, "update_kernels_refusal")


# ------------------------------------------------------------------------------------------------ the yardsticks
@pytest.fixture(scope="module")
def references():
    """per case: inputs, the float64 yardstick, float64 and float32 autograd on the CPU (computed once, never changed)"""
    out = {}
    for case in cc.CASES:
        inp = cc.inputs(case)
        out[case.name] = (inp, cc.yardstick(case, inp), cc.framework(case, inp, torch.float64),
                          cc.framework(case, inp, torch.float32))
    return out


RESULT_KEYS = ("values", "returns", "advantages") + pc.TENSOR_NAMES + pc.SUM_NAMES


def test_cases_cover_what_the_issue_lists():
    rows = {cc.case_rows(c): c for c in cc.CASES}
    assert sorted(rows) == [2, 128, 165, 260, 320, 420, 640, 2520]
    assert cc.case_tiles(rows[128]) == 1 and cc.case_tiles(rows[260]) == 3 and (13 * 4) % 128 and 2 * 52 < 128 < 3 * 52
    assert cc.case_tiles(rows[2520]) == 20 and rows[2520].grid == 3
    assert cc.case_grid(rows[165]) - cc.case_tiles(rows[165]) == 3 and cc.case_tiles(rows[640]) == 5 and rows[640].grid == 2
    assert rows[420].n == 70 and 128 % 70 and rows[320].gap and [c.gap for c in cc.CASES].count(True) == 1
    assert {c.F for c in cc.CASES} == {1, 5, 7} and {c.A for c in cc.CASES} == {1, 2, 5, 8}
    assert {c.n for c in cc.CASES} == {1, 4, 70} and {c.H for c in cc.CASES} == {32, 64}
    assert {(c.H, c.F) for c in cc.CASES} == {(H, F) for H in (32, 64) for F in (1, 5, 7)}
    assert {c.algo for c in cc.CASES} == {"A2C", "PPO"} and {c.done for c in cc.CASES} == {"none", "last row",
                                                                                          "one mid-batch", "random"}
    assert sum(c.done == "random" and c.n > 1 for c in cc.CASES) >= 3
    assert set(cc.MUTATIONS) == set(pc.MUTATIONS) | {"the done flag of replica i % E", "inv_R without n"}
    assert {(a.step, a.clip) for a in cc.APPLY_CASES} == {(a.step, a.clip) for a in pc.APPLY_CASES}
    assert {a.O for a in cc.APPLY_CASES} == {1, 5, 7} and {a.H for a in cc.APPLY_CASES} == {32, 64}
    assert all(cc.unit_of(c.F)[2] for c in cc.CASES)


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_inputs_hold_what_the_cases_promise(case, references):
    inp, want, _, _ = references[case.name]
    T, E, n, H, F, A = case.T, case.E, case.n, case.H, case.F, case.A
    net = {k: v.astype(f64) for k, v in pc.unflatten(inp["theta"], H, F, A).items()}
    z, _, (_, z1, _, z2, _) = pc.forward64(net, inp["obs"].astype(f64).reshape(-1, F))
    assert (z1 < 0).any() and (z2 < 0).any() and (z1 > 0).any() and (z2 > 0).any()
    assert (z1[:, [1, H - 2]] == 0).all() and (z2[:, [2, H - 1]] == 0).all()                 # exactly 0 ...
    assert (net["W1"][:, 1] != 0).any() and (net["Wv"][0, [2, H - 1]] != 0).all()            # ... and not dead ends
    done, rep = inp["done_env"], inp["done"]
    assert done.shape == (T, E) and rep.shape == (T, E * n)
    assert np.array_equal(rep.reshape(T, E, n), np.broadcast_to(done[..., None], (T, E, n)))
    if case.done == "random":
        assert all((done[:, e] != done[:, e + 1]).any() for e in range(E - 1))               # neighbours differ
        if n > 1:   # ... so the flags of replica i % E are not those of replica i // n
            assert not np.array_equal(done[:, np.arange(E * n) % E], rep)
    if case.gap:
        top = np.sort(z, axis=1)
        assert np.median(top[:, -1] - top[:, -2]) > 110
    elif A > 1:
        assert want["probabilities"].min() > 1e-6
    assert all(np.isfinite(np.asarray(want[k])).all() for k in want)
    assert inp["actions"].min() >= 0 and inp["actions"].max() <= A - 1


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_written_out_float64_pass_agrees_with_float64_autograd(case, references):
    inp, want, auto64, auto32 = references[case.name]
    given = auto32["values"].astype(f32)
    for w, a in ((want, auto64), (cc.yardstick(case, inp, values=given), cc.framework(case, inp, torch.float64, values=given))):
        for key in RESULT_KEYS:
            x, y = np.asarray(w[key], f64), np.asarray(a[key], f64)
            assert x.shape == y.shape or x.size == y.size == 1, (key, x.shape, y.shape)
            scale = max(float(np.abs(y).max()), 1e-300)
            assert float(np.abs(x - y).max()) <= 1e-11 * max(scale, 1.0), (case.name, key)


def _violations(got, want, yard32, keys):
    return [k for k in keys if not pc.compare(np.asarray(got[k], f64).reshape(-1), np.asarray(want[k], f64).reshape(-1),
                                              np.asarray(yard32[k], f64).reshape(-1))[0]]


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_the_float32_framework_model_is_within_the_bound_of_the_yardstick(case, references):
    """the float32 framework computation -- what the GPU test takes err_f32 from -- judged as a result itself: its error
    is err_f32, so it passes the bound by construction of the bound, and stays within 5e-6 relative of the yardstick (what
    the issue measured at these F and A); the n-agent returns model is losses.discounted_returns bit for bit"""
    from warp_drive_amd.training.losses import discounted_returns

    inp, want, _, auto32 = references[case.name]
    assert not _violations(auto32, want, auto32, RESULT_KEYS), case.name
    for key in RESULT_KEYS:
        w, g = np.asarray(want[key], f64).reshape(-1), np.asarray(auto32[key], f64).reshape(-1)
        assert np.isfinite(g).all(), (case.name, key)
        # (not the gap case: its logits are of the order of 1e3, where one float32 ulp is 1e-4 -- every log-probability
        # moves by more than this figure whoever computes it in float32)
        if not case.gap:
            assert float(np.abs(w - g).max()) <= 5e-6 * max(float(np.abs(w).max()), 1.0), (case.name, key)
    T, E, n = case.T, case.E, case.n
    v = auto32["values"].astype(f32).reshape(T, E, n)
    r = inp["rewards"].reshape(T, E, n)
    ref = discounted_returns(torch.from_numpy(r), torch.from_numpy(inp["done_env"]), torch.from_numpy(v), case.gamma)
    got = cc.returns_model_n(r, inp["done_env"], v, case.gamma, f32)
    assert got.dtype == f32 and np.array_equal(pc.bits(got), pc.bits(ref.numpy()))


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


@pytest.mark.parametrize("mutation", cc.MUTATIONS)
def test_a_planted_defect_breaks_the_bound(mutation, references):
    cases = [c for c in cc.CASES if cc.mutation_applies(c, mutation)]
    assert len(cases) >= 3, mutation
    for case in cases:
        inp, want, _, auto32 = references[case.name]
        broken = set(_violations(cc.yardstick(case, inp, mutate=mutation), want, auto32, RESULT_KEYS))
        assert broken >= _MUST_BREAK[mutation], (mutation, case.name, sorted(broken))


def test_the_unmutated_yardstick_passes_its_own_bound(references):
    for case in cc.CASES:
        _, want, _, auto32 = references[case.name]
        rounded = {k: np.asarray(want[k], f64).astype(f32).astype(f64) for k in RESULT_KEYS}
        assert not _violations(rounded, want, auto32, RESULT_KEYS), case.name
