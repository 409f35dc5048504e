"""The DDPG gradient launch on the float32 matrix cores on the device (HipDdpgGradientsMatrix_H<H>_O<O>,
wd_kernels_ddpg_mx.hsaco): the body, inputs, yardstick and bound of tests/test_gpu_ddpg_update.py::test_gradients_after_reduce,
as they are, on the matrix entry and the existing Reduce -- plus the returns bit for bit -- then composed in TrainerDDPG
under `fused_update_gradients: "matrix"`."""
import numpy as np
import pytest
import torch

from tests import ddpg_update_cases as dc
from tests import test_gpu_ddpg_update as dd
from tests.test_gpu_ddpg_update import DEV, _counts, _launched_since as _stages_since, _same_bytes, fm  # noqa: F401  (`fm` is a fixture)

pytestmark = pytest.mark.gpu
MX_STAGES = tuple(s + "Matrix" if s == "HipDdpgGradients" else s for s in dd.STAGES)

# 20 400 rows = 160 tiles, the last of 48 rows, on ONE block: 160 trips.  The seeds are the first from 11 + H on at which no
# nonzero hidden preactivation of the float64 yardstick (dc._forward's z1, z2 of the three passes on dc.inputs) lies within
# 4e-7 of zero: nearer, the order of a float32 sum decides the side of relu'(0) and one row's delta appears in or vanishes
# from a gradient whoever computes it.
DEPTH = tuple(dc._case(5100, 6, 3, 0.99, H, O, "inside window", grid=1, seed=seed) for H, O, seed in ((32, 2, 89), (64, 3, 2738)))
CASES = dc.CASES + DEPTH


def _kernels(fm, case):  # noqa: F811
    from warp_drive_amd.training.ddpg_update_kernels import DdpgUpdateKernels

    k = DdpgUpdateKernels(fm, case.E, case.T, case.n_step, case.H, case.O, DEV, gradients_entry="matrix")
    assert case not in DEPTH or (k.rows, k.tiles, dc.case_grid(case)) == (20400, 160, 1)
    return k


def _launched_since(before):
    """the launches with the matrix entry under the lanes entry's name -- and no launch of the lanes entry"""
    out = _stages_since(before)
    assert "HipDdpgGradients" not in out, out
    return {stage.replace("GradientsMatrix", "Gradients"): n for stage, n in out.items()}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_matrix_gradients_after_reduce(fm, monkeypatch, case):  # noqa: F811
    monkeypatch.setattr(dd, "_kernels", _kernels)
    monkeypatch.setattr(dd, "_launched_since", _launched_since)
    inp = dc.inputs(case)
    dd.test_gradients_after_reduce(fm, {case.name: (inp, None)}, case)
    # the returns, bit for bit, from the kernel's own next values
    k, d = _kernels(fm, case), dd._device_inputs(inp)
    nv = k.targets(d["obs"], d["target"], case.scale, case.bias).clone()
    whole_r, returns = dd._sentinel((k.V, case.E))
    k.gradients(d["obs"], d["actions"], d["rewards"], d["done"], nv, d["theta"], case.gamma, case.scale, case.bias,
                returns_out=returns, partials=torch.zeros((dc.case_grid(case), k.PT + 2), device=DEV))
    torch.cuda.synchronize()
    model = dc.returns_model(inp["rewards"], inp["done"], nv.cpu().numpy(), case.n_step, case.gamma, np.float32)
    assert dd._untouched(whole_r, returns) and np.array_equal(dc.bits(returns.cpu().numpy()), dc.bits(model))


@pytest.mark.parametrize("fc", [(64, 64), (32, 32)])
def test_matrix_composed_in_the_trainer(fc, monkeypatch, tmp_path):
    """tests/test_gpu_ddpg_update.py::test_composed_in_the_trainer as it is, on Pendulum's one-launch rollout, with the key:
    four launches per update, the matrix entry second, byte for byte the stages launched directly.  Without the key:
    "lanes"."""
    from warp_drive_amd.training import ddpg_update_kernels as duk
    from warp_drive_amd.training.scripts import train

    trainer, direct, setup = dd._trainer, duk.DdpgUpdateKernels, train.setup_trainer
    seen = []

    def setup_with_the_key(name, ov, **kw):
        if "fused_update" in ov["trainer"]:
            ov["trainer"]["fused_update_gradients"] = "matrix"
        seen.append(setup(name, ov, **kw))
        return seen[-1]

    # (the body builds its direct launches for width 64 and the lanes entry: this test's width and entry instead)
    monkeypatch.setattr(train, "setup_trainer", setup_with_the_key)
    monkeypatch.setattr(dd, "_trainer", lambda *a, **kw: trainer(*a, fc=fc, **kw))
    monkeypatch.setattr(dd, "_launched_since", _launched_since)
    monkeypatch.setattr(duk, "DdpgUpdateKernels", lambda f, E, T, n, H, O, dev, gradients_entry="matrix":
                        direct(f, E, T, n, fc[0], O, dev, gradients_entry=gradients_entry))
    dd.test_composed_in_the_trainer("pendulum", "one launch", tmp_path)
    with_key, without = seen
    assert (with_key.update_path, with_key.update_gradients_path) == ("kernels", "matrix")
    assert with_key._update_kernels.names[1] == f"HipDdpgGradientsMatrix_H{fc[0]}_O3"
    assert (without.update_path, without.update_gradients_path) == ("framework", None)
    monkeypatch.undo()
    plain = dd._trainer(tmp_path / "l", fc=fc)
    assert (plain.update_path, plain.update_gradients_path) == ("kernels", "lanes")
    plain.graceful_close()
