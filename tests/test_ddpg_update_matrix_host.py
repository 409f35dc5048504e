"""Host side of the DDPG gradient launch on the float32 matrix cores (csrc/kernels/ddpg_update_matrix.hip,
wd_kernels_ddpg_mx.hsaco; `trainer.fused_update_gradients: "matrix"`), no GPU: where the four entries live, what they cost,
the wrapper's geometry, and the key's validation in TrainerDDPG."""
import os

import pytest
import torch

from tests.test_ddpg_update_host import _Recorder, built  # noqa: F401  (`built` is a fixture)
from tests.test_pg_update_host import _kernel_metadata, _NoDevice
from warp_drive_amd.training import ddpg_update_kernels as duk

OBJECT = "wd_kernels_ddpg_mx.hsaco"
SHAPES = [(H, O) for H in duk.HIDDEN for O in duk.OBS_SIZES]


def _lds_floats(H, O):
    """dgm_lds_floats(H, O) of the kernel, written out"""
    small = (H * O + 3 * H + 1 + 3) // 4 * 4 + (H * (O + 1) + 3 * H + 1 + 3) // 4 * 4
    return small + 4 * H * (H + 8) + 4 * (2 * H * 36 + (O + 3) * 32)


@pytest.mark.parametrize("H,O", SHAPES)
def test_the_entry_is_in_the_new_unit_without_scratch_or_spills(built, H, O):  # noqa: F811
    from warp_drive_amd import build as wd_build

    assert wd_build.UNITS[OBJECT] == ("ddpg_update_matrix.hip", wd_build.UNITS["wd_kernels_pg_mx.hsaco"][1])
    assert duk.MATRIX_CODE_OBJECT == OBJECT and duk.GRADIENTS_ENTRIES == ("lanes", "matrix")
    names = duk.matrix_kernel_names()
    assert names == [f"HipDdpgGradientsMatrix_H{h}_O{o}" for h, o in SHAPES]
    assert sorted(k for k, v in built.manifest().items() if v == OBJECT) == names
    assert not set(names) & set(duk.all_kernel_names())
    meta = _kernel_metadata(os.path.join(wd_build.CSRC, OBJECT))
    assert sorted(meta) == names
    fields = meta[f"HipDdpgGradientsMatrix_H{H}_O{O}"]
    assert fields[".private_segment_fixed_size"] == 0 and fields[".vgpr_spill_count"] == 0, fields
    assert fields[".max_flat_workgroup_size"] == duk.MATRIX_THREADS == 256, fields
    assert fields[".group_segment_fixed_size"] == 0, fields                       # all LDS is the launch's
    assert 0 < fields[".vgpr_count"] <= 512, fields                               # one block of four wavefronts per compute unit
    assert duk.gradients_matrix_lds_bytes(H, O) == 4 * _lds_floats(H, O) <= duk.LDS_LIMIT == 160 * 1024
    assert duk.gradients_matrix_lds_bytes(H, O) % 16 == 0


@pytest.mark.parametrize("compute_units", [256, 1])
@pytest.mark.parametrize("H,O", SHAPES)
def test_the_wrapper_launches_the_matrix_entry_with_its_geometry(H, O, compute_units):
    E, T, n_step = 5100, 6, 3                 # 20 400 rows: 160 tiles
    rec = _Recorder()
    k = duk.DdpgUpdateKernels(rec, E, T, n_step, H, O, "cpu", compute_units=compute_units, gradients_entry="matrix")
    assert rec.initialised == duk.kernel_names(H, O, "matrix") and rec.initialised[1] == f"HipDdpgGradientsMatrix_H{H}_O{O}"
    assert [x for i, x in enumerate(rec.initialised) if i != 1] == [x for i, x in enumerate(duk.kernel_names(H, O)) if i != 1]
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)  # noqa: E731
    k.gradients(z(T, E, 1, O), z(T, E, 1, 1), z(T, E, 1), z(T, E, dtype=torch.int32), k.next_values, z(k.PT), 0.99, 2.0, 0.25)
    (name, args, block, grid, shared), = rec.launches
    assert name == rec.initialised[1] and block == (256, 1, 1) and (k.rows, k.tiles) == (20400, 160)
    assert grid[0] == min(160, compute_units) == k.partials.shape[0] and k.partials.shape[1] == k.PT + 2
    assert shared == duk.gradients_matrix_lds_bytes(H, O) == 4 * _lds_floats(H, O)
    assert len(args) == 14 and args[12] is k.returns and args[13] is k.partials


def test_the_default_is_the_lanes_entry_and_another_is_refused():
    rec = _Recorder()
    k = duk.DdpgUpdateKernels(rec, 8, 4, 2, 32, 3, "cpu", compute_units=4)
    assert k.gradients_entry == "lanes" and (k.gradients_block, k.gradients_lds) == (128, duk.gradients_lds_bytes(32, 3))
    assert rec.initialised == duk.kernel_names(32, 3) == duk.kernel_names(32, 3, "lanes")
    with pytest.raises(AssertionError):
        duk.DdpgUpdateKernels(rec, 8, 4, 2, 32, 3, "cpu", compute_units=4, gradients_entry="Matrix")
    with pytest.raises(AssertionError):
        duk.kernel_names(32, 3, "mfma")


@pytest.mark.parametrize("value", ["Matrix", "", True])
def test_another_value_is_refused_before_anything_touches_the_device(value):
    from warp_drive_amd.training.trainer_ddpg import TrainerDDPG

    config = {"trainer": {"fused_update": True, "fused_update_gradients": value, "num_envs": 4, "train_batch_size": 8,
                          "num_episodes": 1}, "policy": {"shared": {"algorithm": "DDPG"}}}
    with pytest.raises(ValueError, match='trainer.fused_update_gradients: "lanes" or "matrix"'):
        TrainerDDPG(env_wrapper=_NoDevice(), config=config)
