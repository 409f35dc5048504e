"""The matrix-core gradient launch of the update kit without a GPU (include/wd_env_update_matrix.h;
training/pg_update_custom_kernels.py; utils/custom_tick.py::FusedUpdateMixin): the example and the four probes build to the
kit's entries plus the two Mx entries, without scratch memory or spilled vector registers and within the register share of
their blocks per compute unit; the host's LDS formula equals the literals the probe sources assert; the wrapper's geometry
for "matrix"; the mixin names a missing Mx entry."""
import importlib.util
import os
import sys

import pytest

from tests import pg_update_custom_cases as cc
from tests.test_custom_env_rollout_build import _metadata
from tests.test_custom_env_update_build import ROLLOUT_ENTRIES, _Functions, _update_entries, cache  # noqa: F401
from tests.test_pg_update_host import _Recorder
from warp_drive_amd import build as wd_build
from warp_drive_amd.training import pg_update_custom_kernels as pgck
from warp_drive_amd.training import pg_update_kernels as pguk

_PROBES = os.path.join(cc.ROOT, "tests", "custom_envs")
EXAMPLE_SOURCE = os.path.join(cc.ROOT, "examples", "rendezvous_update_matrix", "rendezvous_update_matrix.hip")
# unit -> (device source, F, entry prefix)
UNITS = {"RendezvousUpdateMatrix": (EXAMPLE_SOURCE, 5, cc.EXAMPLE_PREFIX)}
UNITS.update({f"UpdateMatrixProbeF{F}": (os.path.join(_PROBES, f"update_matrix_probe_f{F}.hip"), F, f"HipUpdateMatrixProbeF{F}Pg")
              for F in (1, 16, 17, 32)})
# the LDS sizes the probe sources assert, in floats: {F: (width 32, width 64)}
LDS_FLOATS = {1: (12364, 29996), 16: (14828, 33356), 17: (15180, 33836), 32: (17644, 37196)}


def example_class():
    """(class, device source) of examples/rendezvous_update_matrix/, imported by path"""
    spec = importlib.util.spec_from_file_location("rendezvous_update_matrix_example", EXAMPLE_SOURCE[:-3] + "py")
    if spec.name not in sys.modules:
        sys.modules[spec.name] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(sys.modules[spec.name])
    return sys.modules[spec.name].RendezvousUpdateMatrix, EXAMPLE_SOURCE


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_the_units_build_to_the_kits_entries_and_the_two_mx_entries_without_scratch(unit):
    source, F, prefix = UNITS[unit]
    mx = pgck.matrix_kernel_names(prefix)
    assert mx == [f"{prefix}GradientsMx_H32", f"{prefix}GradientsMx_H64"]
    others = ROLLOUT_ENTRIES if unit == "RendezvousUpdateMatrix" else []
    meta = _metadata(wd_build.build_env_unit(unit, source))
    assert sorted(meta) == sorted(_update_entries(prefix) + mx + others)
    for H, name in zip(pgck.HIDDEN, mx):
        m, per_cu = meta[name], pguk.MATRIX_BLOCKS_PER_CU[H]
        assert (m["private"], m["vgpr_spills"], m["lds"], m["max_threads"]) == (0, 0, 0, 256), name
        assert 0 < m["vgprs"] <= 512 // per_cu, name
        lds = pgck.gradients_matrix_lds_bytes(H, F)
        assert lds % 16 == 0 and per_cu * lds <= pguk.LDS_LIMIT, (H, F)
        if F in LDS_FLOATS:
            floats = LDS_FLOATS[F][H // 64]
            assert lds == 4 * floats and f"wd_pg_gradients_mx_lds_floats({H}, {F}) == {floats}" in open(source).read()
    sources = wd_build.unit_sources(source, [f[2:] for f in wd_build.env_unit_flags(source) if f.startswith("-I")])
    assert {os.path.basename(s) for s in sources} >= {"wd_env_update.h", "wd_env_update_matrix.h", "pg_update_matrix_common.h",
                                                      "pg_update_common.h"}


@pytest.mark.parametrize("compute_units", [256, 4])
@pytest.mark.parametrize("H,F", [(32, 32), (64, 17), (32, 5)])
def test_the_wrapper_sizes_the_matrix_launch(H, F, compute_units):
    E, T, n, A, prefix = 2000, 20, 100, 5, "HipXPg"
    lanes, default, k = (pgck.PgCustomUpdateKernels(_Recorder(), prefix, E, T, n, H, F, A, "cpu", compute_units=compute_units, **kw)
                         for kw in ({"gradients_entry": "lanes"}, {}, {"gradients_entry": "matrix"}))
    for a in ("names", "gradients_block", "gradients_grid", "gradients_lds", "blocks_per_cu"):
        assert getattr(default, a) == getattr(lanes, a), a
    assert lanes.names == pgck.kernel_names(prefix, H) and lanes.gradients_block == pguk.TILE
    assert k.names == pgck.kernel_names(prefix, H, "matrix") and k.names[2] == f"{prefix}GradientsMx_H{H}"
    assert [a == b for a, b in zip(k.names, lanes.names)] == [True, True, False, True, True]
    per_cu = {32: 2, 64: 1}[H]
    assert (k.gradients_block, k.blocks_per_cu, k.gradients_lds) == (256, per_cu, pgck.gradients_matrix_lds_bytes(H, F))
    assert k.gradients_grid == per_cu * compute_units == k.partials.shape[0] and k.partials.shape[1] == k.P + 4
    with pytest.raises(AssertionError):
        pgck.PgCustomUpdateKernels(_Recorder(), prefix, E, T, n, H, F, A, "cpu", compute_units=4, gradients_entry="mfma")


def test_the_mixin_names_a_missing_mx_entry():
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    env = example_class()[0](num_agents=5, grid_length=4, episode_length=4)
    env.cuda_function_manager = _Functions()
    assert env.update_kernels_refusal(32, 5, 5, gradients_entry="matrix") == (True, "")
    assert env.update_kernels(4, 6, 5, 64, 5, 5, "cpu", compute_units=4, gradients_entry="matrix").gradients_entry == "matrix"
    assert env.update_kernels(4, 6, 5, 64, 5, 5, "cpu", compute_units=4).gradients_entry == "lanes"
    for missing in pgck.matrix_kernel_names(cc.EXAMPLE_PREFIX):
        env.cuda_function_manager = _Functions([missing])
        assert env.update_kernels_refusal(32, 5, 5) == (True, "")                       # "lanes" does not ask for them
        ok, why = env.update_kernels_refusal(32, 5, 5, gradients_entry="matrix")
        assert ok is False and missing in why
        with pytest.raises(UnsupportedRolloutShape, match=missing):
            env.update_kernels(4, 6, 5, 32, 5, 5, "cpu", compute_units=4, gradients_entry="matrix")
