"""Host side of the gradient launch on the float32 matrix cores (csrc/kernels/pg_update_matrix.hip, wd_kernels_pg_mx.hsaco;
`trainer.fused_update_gradients: "matrix"`), no GPU: where the six entries live and what they cost, the wrapper's geometry
for every case of tests/pg_update_cases.py, and the key's values."""
import os

import pytest
import torch

from tests import pg_update_cases as pc
from tests.test_pg_update_host import _kernel_metadata, _NoDevice, _Recorder, built  # noqa: F401  (`built` is a fixture)
from warp_drive_amd.training import pg_update_kernels as pguk

OBJECT = "wd_kernels_pg_mx.hsaco"


def test_the_six_entries_are_in_their_own_code_object(built):
    manifest = built.manifest()
    names = pguk.matrix_kernel_names()
    assert names == sorted(f"HipPgGradientsMx_H{H}_O{O}" for H in (32, 64) for O in (2, 4, 6))
    assert sorted(k for k, v in manifest.items() if v == OBJECT) == names
    assert not [k for k, v in manifest.items() if "GradientsMx" in k and v != OBJECT]
    assert not set(names) & set(pguk.all_kernel_names())


def test_entries_have_no_scratch_no_spills_and_the_block_they_are_launched_with(built):
    from warp_drive_amd import build as wd_build

    meta = _kernel_metadata(os.path.join(wd_build.CSRC, OBJECT))
    assert sorted(meta) == pguk.matrix_kernel_names()
    for name, fields in meta.items():
        H = int(name.split("_H")[1].split("_")[0])
        assert fields[".private_segment_fixed_size"] == 0 and fields[".vgpr_spill_count"] == 0, (name, fields)
        assert fields[".max_flat_workgroup_size"] == pguk.MATRIX_THREADS == 256, (name, fields)
        assert fields[".group_segment_fixed_size"] == 0, (name, fields)               # all LDS is the launch's
        # four wavefronts, one per SIMD: a compute unit holds 512 // registers blocks of them
        assert 0 < fields[".vgpr_count"] <= 512 // pguk.MATRIX_BLOCKS_PER_CU[H], (name, fields)


@pytest.mark.parametrize("compute_units", [256, 4])
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_the_wrapper_launches_a_legal_geometry(case, compute_units):
    rec = _Recorder()
    T, E, H, O, A = case.T, case.E, case.H, case.O, case.A
    k = pguk.PgUpdateKernels(rec, E, T, H, O, A, "cpu", compute_units=compute_units, gradients_entry="matrix")
    assert rec.initialised == pguk.kernel_names(H, O, "matrix") and rec.initialised[2] == f"HipPgGradientsMx_H{H}_O{O}"
    assert [n for i, n in enumerate(rec.initialised) if i != 2] == [n for i, n in enumerate(pguk.kernel_names(H, O)) if i != 2]
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)  # noqa: E731
    k.gradients(z(T, E, 1, O), z(T, E, 1, 1, dtype=torch.int32), z(k.P), case.ent, case.vf)
    (name, args, block, grid, shared), = rec.launches
    blocks = pguk.MATRIX_BLOCKS_PER_CU[H]
    assert name == rec.initialised[2] and block == (256, 1, 1) and k.tiles == pc.case_tiles(case)
    assert grid[0] == min(k.tiles, blocks * compute_units) == k.partials.shape[0] >= 1 and k.partials.shape[1] == k.P + 4
    net = (H * O + 2 * H + 8 * H + 8 + H + 1 + 3) // 4 * 4 + H * (H + 8)
    assert shared == pguk.gradients_matrix_lds_bytes(H, O) == 4 * (net + 4 * (2 * H * 36 + 15 * 32)) and shared % 16 == 0
    assert blocks * shared <= pguk.LDS_LIMIT and pguk.gradients_matrix_lds_bytes(64, 6) <= pguk.LDS_LIMIT == 160 * 1024
    assert (int(args[5]), int(args[6]), int(args[7]), int(args[8])) == (T * E, H, O, A) and args[2] is k.advantages


def test_the_key_takes_lanes_or_matrix_and_absent_means_lanes():
    from warp_drive_amd.training.trainer import Trainer

    config = lambda **tr: {"trainer": dict(fused_update="all", num_envs=4, train_batch_size=8, num_episodes=1, **tr),  # noqa: E731
                           "policy": {"shared": {"algorithm": "A2C"}}}
    for value in ("Matrix", "mfma", "", True, None):
        with pytest.raises(ValueError, match='trainer.fused_update_gradients: "lanes" or "matrix"'):
            Trainer(env_wrapper=_NoDevice(), config=config(fused_update_gradients=value))
    for tr in ({}, {"fused_update_gradients": "lanes"}, {"fused_update_gradients": "matrix"}):
        with pytest.raises(AttributeError):   # accepted: the constructor goes on to the wrapper, which this one does not have
            Trainer(env_wrapper=_NoDevice(), config=config(**tr))
    rec = _Recorder()
    assert pguk.PgUpdateKernels(rec, 8, 4, 32, 4, 2, "cpu", compute_units=4).gradients_entry == "lanes"
    assert rec.initialised == pguk.kernel_names(32, 4) == pguk.kernel_names(32, 4, "lanes")
