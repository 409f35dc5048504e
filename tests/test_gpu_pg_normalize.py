"""normalize_return / normalize_advantage on the update kernels' path (csrc/kernels/pg_normalize.hip,
wd_kernels_pg_norm.hsaco; `trainer.fused_update_normalize`): the two or three launches of `_PgUpdateLaunches.normalize`
against numpy float64 of losses._normalise in A2C.compute_loss_and_metrics' order, then inside Trainer.  Conventions and
bound are tests/test_gpu_pg_update.py's, with losses._normalise in CPU float32 as the float32 yardstick.  Per tick the
returns and the values lie about fifty standard deviations from zero; no tick is constant."""
import functools

import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests.test_gpu_pg_update import (DEV, _counts, _fenced, _judge, _launched_since, _same_bytes, _sentinel, _trainer,  # noqa: F401
                                      _untouched, fm)
from tests.test_gpu_pg_update_gridworld import _trainer as _gridworld_trainer
from warp_drive_amd.training.losses import _normalise

pytestmark = pytest.mark.gpu
# (T, E, n): C = E * n = 2, 5, one column short of a block, a block, one over, a chunk, one over, three chunks and one
SHAPES = [(1, 2, 1), (3, 1, 5), (2, 51, 5), (2, 256, 1), (1, 257, 1), (2, 1024, 4), (2, 4097, 1), (3, 12289, 1)]
SWITCHES = [(True, False), (False, True), (True, True)]   # (normalize_return, normalize_advantage)
SEED = 52


def inputs(shape, seed=SEED):
    T, E, n = shape
    rng = np.random.default_rng(seed + 1000 * T + E * n)
    sigma = rng.uniform(0.5, 2.0, size=(T, 1, 1))
    returns = (50.0 * sigma + sigma * rng.standard_normal((T, E, n))).astype(np.float32)
    values = (50.0 * sigma + sigma * rng.standard_normal((T, E, n))).astype(np.float32)
    return {"returns": returns, "values": values, "advantages": returns - values}   # (float32, as HipDiscountedReturns leaves it)


def _normalise64(x):
    return (x - x.mean(axis=(1, 2), keepdims=True)) / (x.std(axis=(1, 2), ddof=1, keepdims=True) + 1e-10)


def yardstick(inp, normalize_return, normalize_advantage, normalise=_normalise64, cast=lambda a: a.astype(np.float64)):
    """A2C.compute_loss_and_metrics' order; the advantages without normalize_return are the launch's float32 input"""
    out = {}
    adv = cast(inp["advantages"])
    if normalize_return:
        out["norm_returns"] = normalise(cast(inp["returns"]))
        adv = out["advantages"] = out["norm_returns"] - cast(inp["values"])
    if normalize_advantage:
        out["norm_advantages"] = normalise(adv)
    return {k: np.asarray(v) for k, v in out.items()}


framework32 = functools.partial(yardstick, normalise=_normalise, cast=torch.from_numpy)   # losses._normalise, CPU float32


def _run(fm, shape, normalize_return, normalize_advantage):
    """one `normalize` on fenced inputs into sentinel outputs -> (inputs, those on the device, {output: (whole, view)})"""
    from warp_drive_amd.training.pg_update_gridworld_kernels import PgGridworldUpdateKernels
    from warp_drive_amd.training.pg_update_kernels import PgUpdateKernels

    (T, E, n), inp = shape, inputs(shape)
    k = PgUpdateKernels(fm, E, T, 32, 4, 2, DEV) if n == 1 else PgGridworldUpdateKernels(fm, E, T, n, 32, DEV)
    d = {key: _fenced(inp[key]) for key in (("returns", "values") if normalize_return else ("advantages",))}
    outs = {key: _sentinel(inp["returns"].shape) for key in ("norm_returns", "advantages", "norm_advantages") if key not in d}
    before = _counts()
    k.normalize(normalize_return, normalize_advantage, **d, **{key: view for key, (_, view) in outs.items()})
    torch.cuda.synchronize()
    assert sum(_launched_since(before).values()) == 2 + (normalize_return and normalize_advantage)
    return inp, d, outs


@pytest.mark.parametrize("normalize_return,normalize_advantage", SWITCHES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_normalize_against_float64(fm, shape, normalize_return, normalize_advantage):  # noqa: F811
    inp, d, outs = _run(fm, shape, normalize_return, normalize_advantage)
    want, yard = (f(inp, normalize_return, normalize_advantage) for f in (yardstick, framework32))
    assert all(np.ptp(inp[key], axis=(1, 2)).min() > 0 for key in d)          # no constant tick
    for key, (whole, view) in outs.items():
        assert _untouched(whole, view), key                                    # nothing past [T][C]
        if key not in want:                                                    # ... and an output not asked for: nothing at all
            assert bool((whole == pc.SENTINEL_BITS).all()), key
    for key, view in d.items():                                                # the inputs are as they were
        assert np.array_equal(pc.bits(view.cpu().numpy()), pc.bits(inp[key])), key
    _judge(f"{shape} {normalize_return, normalize_advantage}", {key: outs[key][1].cpu().numpy() for key in want}, want, yard,
           tuple(want))


@pytest.mark.parametrize("shape", [(2, 51, 5), (3, 12289, 1)], ids=str)
def test_the_same_launches_twice_give_the_same_bytes(fm, shape):  # noqa: F811
    (_, _, first), (_, _, second) = _run(fm, shape, True, True), _run(fm, shape, True, True)
    for key in first:
        assert _same_bytes(first[key][0], second[key][0]), key


NORMALIZED = {"normalize_return": True, "normalize_advantage": True}
COMPARED = ("Mean rewards", "Value function loss", "Mean entropy", "Policy loss", "Total loss", "Mean advantages",
            "Mean (norm.) advantages", "Mean (discounted) returns", "Mean normalized returns")


MAKE = {   # env -> (trainer, its normalising policy); the runner beside the tagger trains on the kernels without normalisation
    "cartpole": lambda path, **kw: (_trainer(path, "cartpole", policy_extra=NORMALIZED,
                                             env_cfg={"episode_length": 50, "seed": 11}, **kw), "shared"),
    "tag_gridworld": lambda path, **kw: (_gridworld_trainer(path, policy_extra={"tagger": NORMALIZED},
                                                            env_extra={"episode_length": 50}, **kw), "tagger")}


@pytest.mark.parametrize("make", MAKE.values(), ids=list(MAKE))
def test_composed_in_the_trainer(make, tmp_path):
    """one logging iteration with the key and both switches against a framework-path trainer on the same weights and
    batch (episodes longer than the batch: no tick whose returns are one constant): the policy is on the kernels and its
    metric dict is the framework's -- its keys, its values within test_gpu_pg_update.py::test_composed_in_the_trainer's"""
    tr, pol = make(tmp_path / "k", trainer_extra={"fused_update_normalize": True})
    ref, _ = make(tmp_path / "f", fused_update=None)
    assert tr.update_path[pol] == "kernels" and ref.update_path[pol] == "framework"
    assert set(tr.update_path.values()) == {"kernels"} and tr._pg_normalize == {pol: (True, True)}
    tr._generate_rollout_batch()
    ref._generate_rollout_batch()
    torch.cuda.synchronize()
    before = _counts()
    metrics = tr._update_model_params(0, True)[pol]
    torch.cuda.synchronize()
    launched = _launched_since(before)
    assert [launched.get(s) for s in ("HipPgTickMoments", "HipPgNormalizeReturns", "HipPgNormalizeAdvantages")] == [1, 1, 1], launched
    want = ref._update_model_params(0, True)[pol]
    assert set(metrics) == set(want)
    for key in COMPARED:
        assert np.isfinite(metrics[key]) and abs(metrics[key] - want[key]) <= 2e-2 * max(1.0, abs(want[key])), (key, metrics[key], want[key])
    for t in (tr, ref):
        t.graceful_close()
