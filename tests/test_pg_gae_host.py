"""Host side of the policy key `gae_lambda` (csrc/kernels/pg_gae.hip), no GPU: the float64 loop of the definition (`gae64`, which
tests/test_gpu_pg_gae.py holds the launch to) against losses.py's form, the key's validation, the host's S, the unit."""
import os

import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests.test_pg_update_host import _kernel_metadata, _NoDevice, built  # noqa: F401  (`built` is a fixture)
from warp_drive_amd.training import losses
from warp_drive_amd.training import pg_update_kernels as pguk

OBJECT = "wd_kernels_pg_gae.hsaco"
DONE_PATTERNS = ("none", "all", "last row", "random")


def inputs(T, E, n, pattern, seed=54):
    """rewards, values [T, E, n] float32 and done [T, E] int32 from {0, 1, 2}"""
    rng = np.random.default_rng(seed + 1000 * T + E * n)
    done = np.full((T, E), pattern == "all", np.int32)
    done[-1] |= pattern == "last row"
    if pattern == "random":
        done = rng.choice(np.array([0, 0, 0, 1, 2], np.int32), (T, E))
    return {"rewards": (rng.standard_normal((T, E, n)) - 1.0).astype(np.float32),
            "values": (5.0 * rng.standard_normal((T, E, n))).astype(np.float32), "done": done}


def gae64(rewards, done, values, gamma, lam, dtype=np.float64):
    """the definition, row by row in `dtype`: (returns, advantages) [T, E, n]"""
    r, v = rewards.astype(dtype), values.astype(dtype)
    nd = (done <= 0).astype(dtype)[..., None]
    g, gl = dtype(gamma), dtype(dtype(gamma) * dtype(lam))
    A = np.zeros_like(r)
    A[-1] = (1 - nd[-1]) * (r[-1] - v[-1])
    for t in range(r.shape[0] - 2, -1, -1):
        A[t] = (r[t] + g * nd[t] * v[t + 1] - v[t]) + gl * nd[t] * A[t + 1]
    return A + v, A


def _framework(inp, objective):
    t = {k: torch.from_numpy(a) for k, a in inp.items()}
    return objective._returns(t["rewards"], t["done"], t["values"]).numpy()


@pytest.mark.parametrize("pattern", DONE_PATTERNS)
@pytest.mark.parametrize("T,E,n,gamma,lam", [(1, 3, 1, 0.99, 1.0), (2, 5, 2, 1.0, 0.0), (17, 7, 5, 0.99, 0.95), (60, 4, 2, 0.99, 1.0)])
def test_the_framework_form_is_the_definition(T, E, n, gamma, lam, pattern):
    """losses.gae_returns (float32) through A2C / PPO against the float64 loop under tests/pg_update_cases.py's bound, the
    float32 loop as yardstick; lambda = 0: A is delta; lambda = 1: today's returns_batch (float64: 1e-12 of the scale)"""
    inp = inputs(T, E, n, pattern)
    want, A = gae64(**inp, gamma=gamma, lam=lam)
    got, yard = _framework(inp, losses.A2C(gamma, gae_lambda=lam)), gae64(**inp, gamma=gamma, lam=lam, dtype=np.float32)[0]
    assert pc.within_bound(*pc.judge(got, want, yard)), pc.judge(got, want, yard)
    assert np.array_equal(_framework(inp, losses.PPO(discount_factor_gamma=gamma, gae_lambda=lam)), got)
    if lam == 0.0:
        r, v, nd = inp["rewards"].astype(np.float64), inp["values"].astype(np.float64), (inp["done"] <= 0)[..., None]
        assert np.array_equal(A[:-1], r[:-1] + gamma * nd[:-1] * v[1:] - v[:-1])
    if lam == 1.0:
        today64 = np.stack([pc.returns_model(inp["rewards"][..., a], inp["done"], inp["values"][..., a], gamma, np.float64)
                            for a in range(n)], axis=-1)
        assert np.abs(want - today64).max() <= 1e-12 * max(1.0, np.abs(today64).max())
        assert pc.within_bound(*pc.judge(got, today64, _framework(inp, losses.A2C(gamma))))


@pytest.mark.parametrize("value", ["0.95", True, -0.1, 1.5, [0.9]])
def test_anything_but_a_number_in_the_unit_interval_is_refused_before_anything_touches_the_device(value):
    from warp_drive_amd.training.trainer import Trainer

    config = lambda v: {"trainer": {"fused_update": "all", "num_envs": 4, "train_batch_size": 8, "num_episodes": 1},  # noqa: E731
                        "policy": {"shared": {"algorithm": "PPO", "gae_lambda": v}}}
    with pytest.raises(ValueError, match=r"policy.shared.gae_lambda: None or a number in \[0, 1\]"):
        Trainer(env_wrapper=_NoDevice(), config=config(value))
    for accepted in (None, 0, 1, 0.95):   # the constructor goes on to the wrapper, which this one does not have
        with pytest.raises(AttributeError):
            Trainer(env_wrapper=_NoDevice(), config=config(accepted))


@pytest.mark.parametrize("columns,T,cus,want", [
    (100, 500, 256, 16), (100, 128, 256, 16), (100, 127, 256, 8), (100, 16, 256, 2), (100, 15, 256, 1), (1, 1, 256, 1),
    (100000, 10, 256, 1), (100000, 500, 256, 1), (64 * 1024, 500, 256, 1), (64 * 1023, 500, 256, 16), (65, 64, 1, 8), (257, 64, 1, 1)])
def test_the_hosts_choice_of_wavefronts(columns, T, cus, want):
    assert pguk.gae_wavefronts(columns, T, cus) == want and want in pguk.GAE_WAVEFRONTS


def test_the_entry_is_the_new_unit_without_scratch_or_spills(built):  # noqa: F811
    from warp_drive_amd import build as wd_build

    assert wd_build.UNITS[OBJECT] == ("pg_gae.hip", wd_build.UNITS["wd_kernels_pg.hsaco"][1])
    assert pguk.GAE_CODE_OBJECT == OBJECT and pguk.gae_kernel_names() == ["HipPgGaeReturns"]
    assert pguk.GAE_ENTRY not in pguk.all_kernel_names()
    meta = _kernel_metadata(os.path.join(wd_build.CSRC, OBJECT))
    assert sorted(k for k, v in built.manifest().items() if v == OBJECT) == pguk.gae_kernel_names() == sorted(meta)
    fields = meta[pguk.GAE_ENTRY]
    assert fields[".private_segment_fixed_size"] == 0 and fields[".vgpr_spill_count"] == 0, fields
    assert fields[".max_flat_workgroup_size"] == max(pguk.GAE_WAVEFRONTS) * pguk.GAE_TILE == 1024, fields
    assert fields[".group_segment_fixed_size"] == 0 and fields[".vgpr_count"] <= 128, fields   # (LDS is dynamic; 16 wavefronts a CU)
