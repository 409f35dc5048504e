"""The gradient launch on the float32 matrix cores on the device (HipPgGradientsMx_H<H>_O<O>, wd_kernels_pg_mx.hsaco): the
cases, inputs, yardsticks, conventions and bound of tests/test_gpu_pg_update.py, whose helpers these are."""
import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests.test_gpu_pg_update import (DEV, ENVS, _counts, _device_inputs, _launched_since, _same_bytes, _sentinel,  # noqa: F401
                                      _trainer, fm, gradients_after_reduce, references)

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
MX_STAGES = ("HipPgValues", "HipDiscountedReturns", "HipPgGradientsMx", "HipPgReduce", "HipPgApply")


def _kernels(fm, case):
    from warp_drive_amd.training.pg_update_kernels import PgUpdateKernels

    return PgUpdateKernels(fm, case.E, case.T, case.H, case.O, case.A, DEV, gradients_entry="matrix")


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_matrix_gradients_after_reduce(fm, references, case):
    """from the kernels' own values, returns and advantages: HipPgGradientsMx, then the existing HipPgReduce -- the eight
    gradients and the four sums under the bound against float64, the sums of squares against those of the kernel's own
    gradients; surplus blocks write zeros; fences intact; inputs unchanged; a second run gives the same bytes"""
    gradients_after_reduce(fm, case, references[case.name][0], "matrix")


def test_a_matrix_entry_launched_for_another_shape_touches_nothing(fm):
    """another width, another observation size, A = 0 and A = 9: the partials keep the sentinel"""
    case = pc.CASES[2]
    k, d = _kernels(fm, case), _device_inputs(pc.inputs(case))
    rows, H, O, A = case.T * case.E, case.H, case.O, case.A
    adv, ret = torch.zeros(rows, device=DEV), torch.zeros(rows, device=DEV)
    for h, o, a in ((32, O, A), (H, 4, A), (H, O, 0), (H, O, 9)):
        whole, partials = _sentinel((k.gradients_grid, k.P + 4))
        k.fn_gradients(d["obs"], d["actions"], adv, ret, d["theta"], np.int64(rows), np.int32(h), np.int32(o), np.int32(a),
                       f32(1.0), f32(0.1), f32(0.1), partials, block=(k.gradients_block, 1, 1), grid=(k.gradients_grid, 1),
                       shared=k.gradients_lds)
        torch.cuda.synchronize()
        assert bool((whole == pc.SENTINEL_BITS).all()), (h, o, a)


@pytest.mark.parametrize("env,fc,algo", [("cartpole", (32, 32), "A2C"), ("acrobot", (64, 64), "PPO")])
def test_matrix_composed_in_the_trainer(env, fc, algo, tmp_path):
    """three iterations at E = 64, T = 6 with `fused_update_gradients: "matrix"`: the update is five launches, the third
    the Mx entry; parameters and moments equal, byte for byte, the stages launched directly on a snapshot; the packed policy
    is pack_rollout_policy of the module.  Without the key the lanes entry is launched and the Mx entry never is."""
    from warp_drive_amd.training import pg_update_kernels as pguk
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    pol, extra = "shared", {"algorithm": algo, "clip_param": 0.1}
    tr = _trainer(tmp_path / "m", env, fc=fc, policy_extra=extra, trainer_extra={"fused_update_gradients": "matrix"})
    assert tr.update_path == {pol: "kernels"} and tr.update_gradients_path == {pol: "matrix"}
    O, A = ENVS[env]
    direct = pguk.PgUpdateKernels(tr.w.cuda_function_manager, 64, 6, fc[0], O, A, DEV, gradients_entry="matrix")
    model, pcfg = tr.models[pol], tr.config["policy"][pol]
    for it in range(3):
        tr._generate_rollout_batch()
        torch.cuda.synchronize()
        flat, adam = tr._pg_flat[pol], tr._pg_adam[pol]
        st = {"theta": flat.flat.clone(), "m": adam["exp_avg"].clone(), "v": adam["exp_avg_sq"].clone()}
        step, before = adam["step"], _counts()
        tr._update_model_params(it, False)
        torch.cuda.synchronize()
        assert _launched_since(before) == {s: 1 for s in MX_STAGES}, (it, _launched_since(before))
        b, packed = tr.batch[pol], torch.zeros_like(pack_rollout_policy(model))
        direct.compute_values(b["obs"][:6], st["theta"])
        direct.discounted_returns(b["rewards"][:6], tr.done_batch[:6], pcfg["gamma"])
        direct.gradients(b["obs"][:6], b["actions"][:6], st["theta"], pcfg["entropy_coeff"], pcfg["vf_loss_coeff"])
        direct.reduce()
        direct.apply(st["theta"], st["m"], st["v"], step + 1, pcfg["lr"], max_norm=pcfg["max_grad_norm"], packed=packed)
        torch.cuda.synchronize()
        assert _same_bytes(st["theta"], flat.flat) and _same_bytes(st["m"], adam["exp_avg"]) and _same_bytes(st["v"], adam["exp_avg_sq"]), it
        assert _same_bytes(packed, pack_rollout_policy(model)) and _same_bytes(tr._batch_rollout["packed"][pol], packed)
        assert bool(torch.isfinite(flat.flat).all()) and flat.bound()
    tr.graceful_close()
    plain = _trainer(tmp_path / "l", env, fc=fc, policy_extra=extra)
    assert plain.update_path == {pol: "kernels"} and plain.update_gradients_path == {pol: "lanes"}
    plain._generate_rollout_batch()
    before = _counts()
    plain._update_model_params(0, False)
    torch.cuda.synchronize()
    assert _launched_since(before) == {s.replace("Mx", ""): 1 for s in MX_STAGES}
    plain.graceful_close()
