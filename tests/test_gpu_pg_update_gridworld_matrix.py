"""The TagGridWorld gradient launch on the float32 matrix cores on the device (HipPgGwGradientsMatrix_H<H>,
wd_kernels_pg_gw_mx.hsaco): the body, inputs, yardstick and bound of
tests/test_gpu_pg_update_gridworld.py::test_gradients_and_reduce, as they are, on the matrix entry and the existing Reduce;
then composed in Trainer on `tag_gridworld` under `fused_update_gradients: "matrix"`."""
import pytest
import torch

from tests import pg_update_gridworld_cases as gc
from tests import test_gpu_pg_update_gridworld as gw
from tests.test_gpu_pg_update import DEV, _same_bytes, _sentinel, _untouched
from tests.test_gpu_pg_update_gridworld import _counts, _launched_since as _stages_since, fm  # noqa: F401  (`fm` is a fixture)

pytestmark = pytest.mark.gpu
MX_STAGES = tuple(s + "Matrix" if s == "HipPgGwGradients" else s for s in gw.GW_STAGES)

# 20 384 rows = 160 tiles, the last of 32 rows, on ONE compute unit (grid = its blocks): 80 trips per block at width 32, 160
# at width 64.  The seeds are the first from 11 + H on at which no nonzero hidden preactivation of the float64 yardstick
# (pc.forward64's z1, z2 on gc.inputs) lies within 4e-7 of zero: nearer, the order of a float32 sum decides the side of
# relu'(0) and one row's delta appears in or vanishes from a gradient whoever computes it.
DEPTH = tuple(gc._case(637, 8, 4, 0.98, H, 0.05, 1.0, "random", algo, grid=64 // H, seed=seed)
              for H, algo, seed in ((32, "A2C", 43), (64, "PPO", 85)))
CASES = gc.CASES + (gc._case(33, 1, 1, 0.98, 64, 0.05, 1.0, "last row", "PPO", seed=8),) + DEPTH   # 33 rows: a wavefront of one


def _kernels(fm, case, entry="matrix"):  # noqa: F811
    from warp_drive_amd.training.pg_update_gridworld_kernels import PgGridworldUpdateKernels

    k = PgGridworldUpdateKernels(fm, case.E, case.T, case.n, case.H, DEV, gradients_entry=entry,
                                 compute_units=1 if case in DEPTH else None)
    assert case not in DEPTH or (k.rows, k.tiles, k.gradients_grid) == (20384, 160, case.grid)
    return k


def _launched_since(before):
    """the launches with the matrix entry under the lanes entry's name -- and no launch of the lanes entry"""
    out = _stages_since(before)
    assert "HipPgGwGradients" not in out, out
    return {stage.replace("GradientsMatrix", "Gradients"): n for stage, n in out.items()}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_matrix_gradients_and_reduce(fm, monkeypatch, case):  # noqa: F811
    monkeypatch.setattr(gw, "_kernels", _kernels)
    monkeypatch.setattr(gw, "_launched_since", _launched_since)
    gw.test_gradients_and_reduce(fm, {case.name: (gc.inputs(case), None)}, case)


@pytest.mark.parametrize("fc,ppo", [((32, 32), "tagger"), ((64, 64), "runner")])
def test_matrix_composed_in_the_trainer(fc, ppo, tmp_path):
    """three iterations: five launches per policy with the matrix entry third; parameters and Adam moments byte for byte
    those of the stages launched directly on a snapshot; the packed policies are pack_gridworld_policy's.  Without the key:
    "lanes" twice and never a matrix launch."""
    from warp_drive_amd.training import pg_update_gridworld_kernels as pggk
    from warp_drive_amd.training.policy_kernel import pack_gridworld_policy

    E, T, H = 25, 6, fc[0]
    extra = {ppo: {"algorithm": "PPO", "clip_param": 0.1}}
    tr = gw._trainer(tmp_path / "m", fc=fc, policy_extra=extra, trainer_extra={"fused_update_gradients": "matrix"})
    assert tr.update_path == {"tagger": "kernels", "runner": "kernels"}
    assert tr.update_gradients_path == {"tagger": "matrix", "runner": "matrix"}
    direct = {}
    for pol, n in gw.POLICIES.items():
        k = tr._pg_kernels[pol]
        assert k.names == pggk.kernel_names(H, "matrix") and k.names[2] == f"HipPgGwGradientsMatrix_H{H}"
        assert (k.gradients_block, k.gradients_lds) == (256, pggk.gradients_matrix_lds_bytes(H))
        direct[pol] = _kernels(tr.w.cuda_function_manager, gc._case(E, T, n, 0.98, H, 0.05, 1.0, "none"))
    for it in range(3):
        tr._generate_rollout_batch()
        torch.cuda.synchronize()
        snaps = {pol: {"theta": tr._pg_flat[pol].flat.clone(), "m": tr._pg_adam[pol]["exp_avg"].clone(),
                       "v": tr._pg_adam[pol]["exp_avg_sq"].clone()} for pol in gw.POLICIES}
        before = _counts()
        tr._update_model_params(it, False)
        torch.cuda.synchronize()
        assert _stages_since(before) == {s: 2 for s in MX_STAGES}, it
        for pol in gw.POLICIES:
            pcfg, flat, adam, st, dk, b = tr.config["policy"][pol], tr._pg_flat[pol], tr._pg_adam[pol], snaps[pol], direct[pol], tr.batch[pol]
            whole_k, packed = _sentinel((pggk.packed_floats(H),))
            dk.compute_values(b["obs"][:T], st["theta"])
            dk.discounted_returns(b["rewards"][:T], tr.done_batch[:T], pcfg["gamma"])
            dk.gradients(b["obs"][:T], b["actions"][:T], st["theta"], pcfg["entropy_coeff"], pcfg["vf_loss_coeff"])
            dk.reduce()
            dk.apply(st["theta"], st["m"], st["v"], it + 1, pcfg["lr"], max_norm=pcfg["max_grad_norm"], packed=packed)
            torch.cuda.synchronize()
            assert _same_bytes(st["theta"], flat.flat) and _same_bytes(st["m"], adam["exp_avg"]), (it, pol)
            assert _same_bytes(st["v"], adam["exp_avg_sq"]) and bool(torch.isfinite(flat.flat).all()), (it, pol)
            assert _untouched(whole_k, packed) and _same_bytes(packed, pack_gridworld_policy(tr.models[pol])), (it, pol)
            assert _same_bytes(packed, tr._batch_rollout["packed"][pol]), (it, pol)
    tr.graceful_close()
    plain = gw._trainer(tmp_path / "l", fc=fc, policy_extra=extra)
    assert plain.update_gradients_path == {"tagger": "lanes", "runner": "lanes"}
    plain._generate_rollout_batch()
    before = _counts()
    plain._update_model_params(0, False)
    torch.cuda.synchronize()
    assert _stages_since(before) == {s: 2 for s in gw.GW_STAGES}
    plain.graceful_close()
