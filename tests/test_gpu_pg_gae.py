"""GAE(lambda) on the update kernels' path (csrc/kernels/pg_gae.hip; the policy key `gae_lambda`): HipPgGaeReturns with S forced
against the float64 loop of the definition (tests/test_pg_gae_host.py::gae64), then inside Trainer.  Conventions and bound are
tests/test_gpu_pg_update.py's, with the same loop in float32 as the float32 yardstick."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests.test_gpu_pg_update import DEV, _counts, _fenced, _judge, _launched_since, _same_bytes, _sentinel, _trainer, _untouched, fm  # noqa: F401
from tests.test_gpu_pg_normalize import COMPARED
from tests.test_pg_gae_host import DONE_PATTERNS, gae64, inputs

pytestmark = pytest.mark.gpu
TICKS = (1, 2, 3, 17, 500)           # one row, S > T, T no multiple of S, kept segments (<= 32 rows) and re-read ones
SHAPES = ((1, 1), (63, 1), (64, 1), (65, 1), (200, 1), (13, 5), (40, 5))   # (E, n): C = 1, 63, 64, 65, 200; 65, 200 with n = 5
SETTINGS = tuple(itertools.product((0.0, 0.95, 1.0), (0.99, 1.0), DONE_PATTERNS))   # (lambda, gamma, done)


@functools.lru_cache(maxsize=None)
def reference(T, E, n, pattern, gamma, lam):   # once per case, shared by every S: inputs, float64, the float32 loop
    inp = inputs(T, E, n, pattern)
    (ret, adv), ret32 = gae64(**inp, gamma=gamma, lam=lam), gae64(**inp, gamma=gamma, lam=lam, dtype=np.float32)[0]
    return inp, {"returns": ret, "advantages": adv}, {"returns": ret32, "advantages": ret32 - inp["values"]}


def _launch(k, d, gamma, lam, S):
    (whole_r, returns), (whole_a, adv) = _sentinel((k.T, k.E, k.n)), _sentinel((k.T, k.E, k.n))
    before = _counts()
    k.gae_returns(d["rewards"], d["done"], gamma, lam, values=d["values"], returns=returns, advantages=adv, wavefronts=S)
    torch.cuda.synchronize()
    assert _launched_since(before) == {"HipPgGaeReturns": 1}
    assert _untouched(whole_r, returns) and _untouched(whole_a, adv)   # nothing past [T][C]
    return {"returns": returns, "advantages": adv}


@pytest.mark.parametrize("S", (1, 2, 16))
@pytest.mark.parametrize("E,n", SHAPES)
@pytest.mark.parametrize("T", TICKS)
def test_the_entry_against_float64(fm, T, E, n, S):  # noqa: F811
    """every (lambda, gamma, done pattern): both outputs under the bound, the inputs as they were, a second launch the same bytes"""
    from warp_drive_amd.training.pg_update_gridworld_kernels import PgGridworldUpdateKernels
    from warp_drive_amd.training.pg_update_kernels import PgUpdateKernels

    k = PgUpdateKernels(fm, E, T, 32, 4, 2, DEV) if n == 1 else PgGridworldUpdateKernels(fm, E, T, n, 32, DEV)
    for lam, gamma, pattern in SETTINGS:
        inp, want, yard = reference(T, E, n, pattern, gamma, lam)
        d = {key: _fenced(a, torch.int32 if key == "done" else torch.float32) for key, a in inp.items()}
        first, second = _launch(k, d, gamma, lam, S), _launch(k, d, gamma, lam, S)
        assert all(_same_bytes(first[key], second[key]) for key in first)
        assert all(np.array_equal(pc.bits(view.cpu().numpy()), pc.bits(inp[key])) for key, view in d.items())
        _judge(f"T{T} E{E} n{n} S{S} lambda {lam} gamma {gamma} {pattern}", {key: v.cpu().numpy() for key, v in first.items()},
               want, yard, ("returns", "advantages"))


def test_composed_in_the_trainer(tmp_path):
    """one logging iteration on Acrobot (E = 64, T = 16: two wavefronts a block) with `gae_lambda: 0.95` against a
    framework-path trainer on the same weights and batch, under test_gpu_pg_update.py::test_composed_in_the_trainer's bound"""
    pol, extra = "shared", {"algorithm": "PPO", "clip_param": 0.1, "gae_lambda": 0.95}
    tr = _trainer(tmp_path / "k", "acrobot", T=16, policy_extra=extra)
    ref = _trainer(tmp_path / "f", "acrobot", T=16, policy_extra=extra, fused_update=None)
    assert tr.update_path == {pol: "kernels"} and ref.update_path == {pol: "framework"}
    tr._generate_rollout_batch()
    ref._generate_rollout_batch()
    torch.cuda.synchronize()
    before = _counts()
    metrics = tr._update_model_params(0, True)[pol]
    torch.cuda.synchronize()
    launched = _launched_since(before)   # (the new entry once, HipDiscountedReturns not at all)
    assert launched == {s: 1 for s in ("HipPgValues", "HipPgGaeReturns", "HipPgGradients", "HipPgReduce", "HipPgApply")}, launched
    want = ref._update_model_params(0, True)[pol]
    assert set(metrics) == set(want)
    for key in COMPARED:
        assert np.isfinite(metrics[key]) and abs(metrics[key] - want[key]) <= 2e-2 * max(1.0, abs(want[key])), (key, metrics[key], want[key])
    for t in (tr, ref):
        t.graceful_close()
