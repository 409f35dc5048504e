"""The matrix-core gradient launch of a custom environment on the device (include/wd_env_update_matrix.h): the body, cases'
inputs, yardstick and bound of tests/test_gpu_custom_env_update.py::test_gradients_and_reduce, as they are, on the Mx entry
and the existing Reduce; then composed in Trainer on examples/rendezvous_update_matrix/.  One compile per unit and module."""
import logging

import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests import pg_update_custom_cases as cc
from tests import test_gpu_custom_env_update as cu
from tests.test_custom_env_update_matrix_build import UNITS, example_class
from tests.test_gpu_custom_env_update import E_, N_, T_, _counts, _launched_since, env_cache  # noqa: F401
from tests.test_gpu_pg_update import DEV, _same_bytes, _sentinel, _untouched

pytestmark = pytest.mark.gpu
f32 = np.float32


def _case(E, T, n, H, F, A, done, algo="A2C", grid=None, gap=False, seed=0):
    return cc._case(E, T, n, 0.98, H, F, A, 0.05, 1.0, done, algo, grid, gap, seed)


CASES = (
    _case(1, 2, 1, 32, 1, 1, "none", seed=1),                                # 2 rows: three wavefronts empty
    _case(33, 1, 1, 64, 16, 2, "last row", "PPO", seed=2),                   # 33 rows: a wavefront holding one row
    _case(16, 2, 4, 64, 5, 5, "one mid-batch", "PPO", seed=3),               # 128 rows: exactly one tile
    _case(13, 5, 4, 32, 17, 2, "random", seed=4),                            # 260 rows
    _case(4, 9, 70, 64, 32, 8, "random", "PPO", grid=3, seed=5),             # 2520 rows on 3 blocks: trips, 70 agents
    _case(33, 5, 1, 32, 32, 8, "one mid-batch", grid=5, seed=6),             # 165 rows on 5 blocks: surplus blocks
    _case(16, 5, 4, 64, 17, 5, "last row", gap=True, seed=7),                # logit gaps above 110
    _case(13, 5, 4, 32, 16, 5, "random", "PPO", seed=8),                     # the vector dW0 at its largest, width 32
    _case(2, 3, 70, 32, 5, 5, "random", seed=9),                             # 420 rows, the example's entries at width 32
    _case(16, 2, 4, 64, 1, 8, "none", seed=10),                              # one first-layer step at width 64
)
# 20 385 rows on ONE compute unit (grid = its blocks): 160 trips per block at width 64, 80 at width 32.  The seeds are the
# first from 11 + H on at which no nonzero hidden preactivation of the float64 yardstick lies within 4e-7 of zero (64 terms
# of float32 rounding at the activations' scale): nearer, the order of a float32 sum decides the side of relu'(0).
DEPTH = tuple(_case(4077, 5, 1, H, 17, 5, "random", grid=64 // H, seed=seed) for H, seed in ((32, 43), (64, 90)))


@pytest.fixture(scope="module")
def managers(env_cache):  # noqa: F811
    """F -> a function manager whose custom code object has the update entries and the Mx entries for F"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd import build as wd_build
    from warp_drive_amd.managers.function_manager import HIPFunctionManager

    require_gpu()
    made = {}

    def get(F):
        if F not in made:
            unit, (source, _, _) = next((u, s) for u, s in UNITS.items() if s[1] == F)
            made[F] = HIPFunctionManager(num_agents=1, num_envs=1)
            made[F].load_hip_from_binary_file()
            made[F].load_custom_hip_from_binary_file(wd_build.build_env_unit(unit, source), source)
        return made[F]

    return get


def _kernels(managers, case):  # noqa: F811
    from warp_drive_amd.training.pg_update_custom_kernels import PgCustomUpdateKernels

    prefix = next(s[2] for s in UNITS.values() if s[1] == case.F)
    k = PgCustomUpdateKernels(managers(case.F), prefix, case.E, case.T, case.n, case.H, case.F, case.A, DEV,
                              gradients_entry="matrix", compute_units=1 if case in DEPTH else None)
    assert case not in DEPTH or (k.rows, k.tiles, k.gradients_grid) == (20385, 160, case.grid)
    return k


@pytest.mark.parametrize("case", CASES + DEPTH, ids=lambda c: c.name)
def test_matrix_gradients_and_reduce(managers, monkeypatch, case):  # noqa: F811
    """the existing test's body with the kernels built for "matrix": exactly one PgGradientsMx launch and no PgGradients"""
    def launched(before):
        out = _launched_since(before)
        assert "PgGradients" not in out, out
        return {stage.replace("PgGradientsMx", "PgGradients"): n for stage, n in out.items()}

    monkeypatch.setattr(cu, "_case_kernels", _kernels)
    monkeypatch.setattr(cu, "_launched_since", launched)
    cu.test_gradients_and_reduce(managers, {case.name: (cc.inputs(case), None)}, case)


@pytest.mark.parametrize("H", [32, 64])
def test_a_matrix_entry_launched_with_a_bad_action_count_touches_nothing(managers, H):
    k = _kernels(managers, _case(16, 2, 4, H, 17, 5, "none"))
    obs, theta = torch.zeros((k.rows, 17), device=DEV), torch.zeros(k.P, device=DEV)
    actions, flat = torch.zeros(k.rows, dtype=torch.int32, device=DEV), torch.zeros(k.rows, device=DEV)
    for bad_a in (0, 9):
        whole, partials = _sentinel((1, k.P + 4))
        k.fn_gradients(obs, actions, flat, flat, theta, np.int64(k.rows), np.int32(bad_a), f32(1.0 / k.rows), f32(0.0), f32(1.0),
                       partials, block=(k.gradients_block, 1, 1), grid=(1, 1), shared=k.gradients_lds)
        torch.cuda.synchronize()
        assert bool((whole == pc.SENTINEL_BITS).all()), (H, bad_a)


def _trainer(tmp_path, cls, source, fc, algo, entry):
    from tests.rendezvous_helpers import registrar_for
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.training.trainer import Trainer

    w = EnvWrapper(env_name=cls.name, env_config=dict(num_agents=N_, grid_length=6, episode_length=5, seed=9), num_envs=E_,
                   env_backend="hip", env_registrar=registrar_for(cls, source))
    tcfg = {"num_envs": E_, "train_batch_size": E_ * T_, "num_episodes": 10 ** 6, "seed": 5, "fused_rollout_policy": "all",
            "fused_update": "all", **({"fused_update_gradients": entry} if entry else {})}
    pcfg = {"to_train": True, "algorithm": algo, "lr": 0.01, "vf_loss_coeff": 1, "entropy_coeff": 0.05, "gamma": 0.98,
            "clip_grad_norm": True, "max_grad_norm": 3, "normalize_advantage": False, "normalize_return": False,
            "clip_param": 0.1, "model": {"type": "fully_connected", "fc_dims": list(fc), "model_ckpt_filepath": ""}}
    config = {"name": "rdv", "trainer": tcfg, "policy": {"shared": pcfg},
              "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0, "basedir": str(tmp_path), "name": "rdv", "tag": "t"}}
    torch.manual_seed(3)
    return Trainer(env_wrapper=w, config=config, policy_tag_to_agent_id_map={"shared": list(range(N_))},
                   results_dir=str(tmp_path), verbose=False)


@pytest.mark.parametrize("fc,algo", [((32, 32), "A2C"), ((64, 64), "PPO")])
def test_matrix_composed_in_the_trainer(fc, algo, tmp_path, caplog):
    """five launches with the Mx entry third; parameters and moments byte for byte those of the stages launched directly on
    a snapshot; the packed policy is pack_rollout_policy.  RendezvousUpdate under the key: one log line, the lanes entry.
    Without the key: never an Mx launch."""
    from tests.hip_harness import require_gpu
    from tests.test_custom_env_update_build import _example_class
    from warp_drive_amd.training import pg_update_custom_kernels as pgck
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    require_gpu()
    pol, H, prefix = "shared", fc[0], "HipRendezvousUpdatePg"
    cls, source = example_class()
    tr = _trainer(tmp_path / "m", cls, source, fc, algo, "matrix")
    assert tr.update_path == {pol: "kernels"} and tr.update_gradients_path == {pol: "matrix"}
    k = tr._pg_kernels[pol]
    assert k.names == pgck.kernel_names(prefix, H, "matrix") and k.gradients_block == 256
    tr._generate_rollout_batch()
    torch.cuda.synchronize()
    flat, adam, pcfg, b = tr._pg_flat[pol], tr._pg_adam[pol], tr.config["policy"][pol], tr.batch[pol]
    st = {"theta": flat.flat.clone(), "m": adam["exp_avg"].clone(), "v": adam["exp_avg_sq"].clone()}
    before = _counts()
    tr._update_model_params(0, False)
    torch.cuda.synchronize()
    assert _launched_since(before) == {"PgValues": 1, "HipDiscountedReturns": 1, "PgGradientsMx": 1, "PgReduce": 1, "PgApply": 1}
    dk = pgck.PgCustomUpdateKernels(tr.w.cuda_function_manager, prefix, E_, T_, N_, H, 5, 5, DEV, gradients_entry="matrix")
    whole_k, packed = _sentinel((k.packed_floats,))
    obs, actions = b["obs"][:T_], b["actions"][:T_]
    dk.compute_values(obs, st["theta"])
    dk.discounted_returns(b["rewards"][:T_], tr.done_batch[:T_], pcfg["gamma"])
    dk.gradients(obs, actions, st["theta"], pcfg["entropy_coeff"], pcfg["vf_loss_coeff"])
    dk.reduce()
    dk.apply(st["theta"], st["m"], st["v"], 1, pcfg["lr"], max_norm=pcfg["max_grad_norm"], packed=packed)
    torch.cuda.synchronize()
    assert _same_bytes(st["theta"], flat.flat) and _same_bytes(st["m"], adam["exp_avg"]) and _same_bytes(st["v"], adam["exp_avg_sq"])
    assert _untouched(whole_k, packed) and _same_bytes(packed, pack_rollout_policy(tr.models[pol]).reshape(-1))
    assert _same_bytes(packed, tr._batch_rollout["packed"][pol].reshape(-1)) and bool(torch.isfinite(flat.flat).all())
    tr.graceful_close()
    for i, (env, entry, said) in enumerate((((_example_class(), cc.EXAMPLE_SOURCE), "matrix", 1), ((cls, source), None, 0))):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            plain = _trainer(tmp_path / str(i), *env, fc, algo, entry)
        lines = [r.getMessage() for r in caplog.records if "fused_update_gradients" in r.getMessage()]
        assert len(lines) == said and all(f"{prefix}GradientsMx_H32" in line for line in lines), lines
        assert plain.update_path == {pol: "kernels"} and plain.update_gradients_path == {pol: "lanes"}
        plain._generate_rollout_batch()
        before = _counts()
        plain._update_model_params(0, False)
        torch.cuda.synchronize()
        assert _launched_since(before) == {"PgValues": 1, "HipDiscountedReturns": 1, "PgGradients": 1, "PgReduce": 1, "PgApply": 1}
        plain.graceful_close()
