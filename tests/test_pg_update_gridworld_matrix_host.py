"""Host side of the TagGridWorld gradient launch on the float32 matrix cores (csrc/kernels/pg_update_gridworld_matrix.hip,
wd_kernels_pg_gw_mx.hsaco; `trainer.fused_update_gradients: "matrix"`), no GPU: where the two entries live, what they cost,
and the wrapper's geometry."""
import os

import pytest
import torch

from tests.test_pg_update_host import _kernel_metadata, _Recorder, built  # noqa: F401  (`built` is a fixture)
from warp_drive_amd.training import pg_update_gridworld_kernels as pggk
from warp_drive_amd.training import pg_update_kernels as pguk

OBJECT = "wd_kernels_pg_gw_mx.hsaco"


@pytest.mark.parametrize("H", pggk.HIDDEN)
def test_the_entry_is_in_the_new_unit_without_scratch_or_spills(built, H):  # noqa: F811
    from warp_drive_amd import build as wd_build

    assert wd_build.UNITS[OBJECT] == ("pg_update_gridworld_matrix.hip", wd_build.UNITS["wd_kernels_pg_mx.hsaco"][1])
    assert pggk.MATRIX_CODE_OBJECT == OBJECT
    names = pggk.matrix_kernel_names()
    assert names == ["HipPgGwGradientsMatrix_H32", "HipPgGwGradientsMatrix_H64"]
    assert sorted(k for k, v in built.manifest().items() if v == OBJECT) == names
    assert not set(names) & set(pggk.all_kernel_names())
    meta = _kernel_metadata(os.path.join(wd_build.CSRC, OBJECT))
    assert sorted(meta) == names
    fields = meta[f"HipPgGwGradientsMatrix_H{H}"]
    assert fields[".private_segment_fixed_size"] == 0 and fields[".vgpr_spill_count"] == 0, fields
    assert fields[".max_flat_workgroup_size"] == pguk.MATRIX_THREADS == 256, fields
    assert fields[".group_segment_fixed_size"] == 0, fields                       # all LDS is the launch's
    # four wavefronts, one per SIMD: a compute unit holds 512 // registers blocks of them
    assert 0 < fields[".vgpr_count"] <= 512 // pguk.MATRIX_BLOCKS_PER_CU[H], fields
    assert pguk.MATRIX_BLOCKS_PER_CU[H] * pggk.gradients_matrix_lds_bytes(H) <= pguk.LDS_LIMIT == 160 * 1024


@pytest.mark.parametrize("compute_units", [256, 1])
@pytest.mark.parametrize("H", pggk.HIDDEN)
def test_the_wrapper_launches_the_matrix_entry_with_its_geometry(H, compute_units):
    E, T, n = 637, 8, 4                       # 20 384 rows: 160 tiles
    rec = _Recorder()
    k = pggk.PgGridworldUpdateKernels(rec, E, T, n, H, "cpu", compute_units=compute_units, gradients_entry="matrix")
    assert rec.initialised == pggk.kernel_names(H, "matrix") and rec.initialised[2] == f"HipPgGwGradientsMatrix_H{H}"
    assert [x for i, x in enumerate(rec.initialised) if i != 2] == [x for i, x in enumerate(pggk.kernel_names(H)) if i != 2]
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)  # noqa: E731
    k.gradients(z(T, E, n, 21), z(T, E, n, 1, dtype=torch.int32), z(k.P), 0.05, 1.0)
    (name, args, block, grid, shared), = rec.launches
    blocks = pguk.MATRIX_BLOCKS_PER_CU[H]
    assert name == rec.initialised[2] and block == (256, 1, 1) and (k.rows, k.tiles) == (20384, 160)
    assert grid[0] == min(160, blocks * compute_units) == k.partials.shape[0] and k.partials.shape[1] == k.P + 4
    # the kernel's gwm_lds_floats(H), written out
    net = (22 * (32 if H == 32 else 96) + 2 * H + 5 * H + 8 + H + 1 + 3) // 4 * 4 + 2 * H * (H + 8)
    assert shared == pggk.gradients_matrix_lds_bytes(H) == 4 * (net + 4 * (2 * H * 36 + 22 * 36 + 6 * 32)) and shared % 16 == 0
    assert len(args) == 10 and int(args[5]) == 20384 and args[2] is k.advantages and args[9] is k.partials


def test_the_default_is_the_lanes_entry():
    rec = _Recorder()
    k = pggk.PgGridworldUpdateKernels(rec, 8, 4, 4, 32, "cpu", compute_units=4)
    assert k.gradients_entry == "lanes" and (k.gradients_block, k.gradients_lds) == (128, pggk.gradients_lds_bytes(32))
    assert rec.initialised == pggk.kernel_names(32) == pggk.kernel_names(32, "lanes")
    assert "HipPgGwGradients_H32" in rec.initialised and not set(pggk.matrix_kernel_names()) & set(pggk.all_kernel_names())
