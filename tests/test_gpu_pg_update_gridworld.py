"""The A2C / PPO update kernels for the TagGridWorld policies on the device (wd_kernels_pg_gw.hsaco; cases and inputs:
tests/pg_update_gridworld_cases.py, yardstick: tests/pg_update_cases.py), stage by stage from each stage's own inputs, then
composed inside Trainer on `tag_gridworld` (`fused_rollout_policy: "all"` + `fused_update: "all"`).

Conventions: those of tests/test_gpu_pg_update.py (sentinel-filled outputs with surplus rows, NaN-fenced inputs, every
launch through the wrappers and counted in hip_driver.LAUNCH_COUNTS, per result tensor
err <= max(4 * err_f32, 2e-6 * scale), err / err_f32 printed per tensor under pytest -s)."""
import copy
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests import pg_update_gridworld_cases as gc
from tests.test_gpu_pg_update import DEV, _fenced, _judge, _same_bytes, _sentinel, _untouched

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
GW_STAGES = ("HipPgGwValues", "HipDiscountedReturns", "HipPgGwGradients", "HipPgGwReduce", "HipPgGwApply")
POLICIES = {"tagger": 4, "runner": 1}


@pytest.fixture(scope="module")
def fm():
    from tests.hip_harness import require_gpu
    from warp_drive_amd.managers.function_manager import HIPFunctionManager

    require_gpu()
    m = HIPFunctionManager(num_agents=1, num_envs=1)
    m.load_hip_from_binary_file()
    return m


@pytest.fixture(scope="module")
def references():
    """per case: the inputs and the float64 yardstick from them (computed once, never changed)"""
    out = {}
    for case in gc.CASES:
        inp = gc.inputs(case)
        out[case.name] = (inp, gc.yardstick(case, inp))
    return out


def _kernels(fm, case):
    from warp_drive_amd.training.pg_update_gridworld_kernels import PgGridworldUpdateKernels

    return PgGridworldUpdateKernels(fm, case.E, case.T, case.n, case.H, DEV)


def _counts():
    from warp_drive_amd.managers import hip_driver as drv

    return {k: v for k, v in drv.LAUNCH_COUNTS.items() if k.startswith("HipPg") or k == "HipDiscountedReturns"}


def _launched_since(before):
    """{stage: launches} of the update's kernels since `before`"""
    out = {}
    for name, n in _counts().items():
        d = n - before.get(name, 0)
        if d:
            stage = name.split("_H")[0]
            out[stage] = out.get(stage, 0) + d
    return out


def _device_inputs(case, inp):
    T, E, n = case.T, case.E, case.n
    return {"obs": _fenced(inp["obs"].reshape(T, E, n, 21)), "actions": _fenced(inp["actions"].reshape(T, E, n, 1), torch.int32),
            "rewards": _fenced(inp["rewards"].reshape(T, E, n)), "done_env": _fenced(inp["done_env"], torch.int32),
            "theta": _fenced(inp["theta"])}


def _inputs_as_they_were(d, inp):
    for key in d:
        assert np.array_equal(pc.bits(d[key].cpu().numpy().reshape(-1)), pc.bits(np.ascontiguousarray(inp[key]).reshape(-1))), key


# ================================================================================================ 1 + 2. values, returns
@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_values_and_returns(fm, references, case):
    """values under the bound against float64 -- at the wrapper's geometry, and bit-identical at one block of 64 threads
    (grid-stride trips) and with surplus blocks; the returns the existing entry forms from them with n agents per replica
    equal the float32 returns model and losses.discounted_returns bit for bit, the advantages are returns - values"""
    from warp_drive_amd.training.losses import discounted_returns

    inp, want = references[case.name]
    k, d = _kernels(fm, case), _device_inputs(case, inp)
    T, E, n = case.T, case.E, case.n
    results = []
    for block, grid in ((None, None), (64, 1), (128, -(-T * E * n // 128) + 3)):
        whole, out = _sentinel((T, E, n))
        before = _counts()
        k.compute_values(d["obs"], d["theta"], out=out, block=block, grid=grid)
        torch.cuda.synchronize()
        assert _launched_since(before) == {"HipPgGwValues": 1}
        assert _untouched(whole, out), (case.name, block, grid)
        results.append(out)
    assert _same_bytes(results[0], results[1]) and _same_bytes(results[0], results[2])
    yard = gc.framework(case, inp, torch.float32, DEV)
    _judge(f"values {case.name}", {"values": results[0].cpu().numpy().reshape(T, E * n)}, want, yard, ["values"])

    whole_r, returns = _sentinel((T, E, n))
    whole_a, adv = _sentinel((T, E, n))
    before = _counts()
    k.discounted_returns(d["rewards"], d["done_env"], case.gamma, values=results[0], returns=returns, advantages=adv)
    torch.cuda.synchronize()
    assert _launched_since(before) == {"HipDiscountedReturns": 1}
    assert _untouched(whole_r, returns) and _untouched(whole_a, adv)
    v_host = results[0].cpu().numpy()
    model = gc.returns_model_n(inp["rewards"].reshape(T, E, n), inp["done_env"], v_host, case.gamma, f32)
    assert np.array_equal(pc.bits(returns.cpu().numpy()), pc.bits(model)), case.name
    ref = discounted_returns(d["rewards"], d["done_env"], results[0], case.gamma)
    assert _same_bytes(returns, ref) and _same_bytes(adv, ref - results[0]), case.name
    _inputs_as_they_were(d, inp)


# ============================================================================================ 3 + 4. gradients, reduce
@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: c.name)
def test_gradients_and_reduce(fm, references, case):
    """gradients, from the kernel's own values, returns and advantages: the per-block partials summed in block order in
    float64 -- the eight tensors and the four sums -- under the bound against the yardstick; blocks without rows write zeros.
    reduce, from the partials it was given: the flat gradient, the four sums and the per-tensor sums of squares under the
    bound against their float64 sums.  Nothing outside the written regions changes; a second run gives the same bytes."""
    inp, _ = references[case.name]
    k, d = _kernels(fm, case), _device_inputs(case, inp)
    T, E, n = case.T, case.E, case.n
    values = k.compute_values(d["obs"], d["theta"]).clone()
    returns, adv = k.discounted_returns(d["rewards"], d["done_env"], case.gamma, values=values)
    returns, adv = returns.clone(), adv.clone()
    v_host = values.cpu().numpy().reshape(T, E * n)
    want = gc.yardstick(case, inp, values=v_host)
    yard = gc.framework(case, inp, torch.float32, DEV, values=v_host)
    grid = gc.case_grid(case)
    P = k.P
    runs = []
    for _ in range(2):
        whole_p, partials = _sentinel((grid, P + 4))
        whole_g, grads = _sentinel((P,))
        whole_s, sumsq = _sentinel((8,))
        whole_l, sums = _sentinel((4,))
        before = _counts()
        k.gradients(d["obs"], d["actions"], d["theta"], case.ent, case.vf, advantages=_fenced(adv.cpu().numpy()),
                    returns=_fenced(returns.cpu().numpy()), partials=partials)
        k.reduce(partials=partials, grads=grads, sumsq=sumsq, sums=sums)
        torch.cuda.synchronize()
        assert _launched_since(before) == {"HipPgGwGradients": 1, "HipPgGwReduce": 1}
        for whole, view in ((whole_p, partials), (whole_g, grads), (whole_s, sumsq), (whole_l, sums)):
            assert _untouched(whole, view), case.name
        runs.append((partials, grads, sumsq, sums))
    for a, b in zip(*runs):
        assert _same_bytes(a, b), case.name
    partials, grads, sumsq, sums = runs[0]
    assert bool(torch.isfinite(partials).all())
    assert grid == k.tiles or case.grid
    if grid > k.tiles:
        assert not partials[k.tiles:].any(), "a block without rows writes zeros"
    bounds = pc.tensor_bounds(case.H, 21, 5)
    # ---- the gradient stage by itself: its partials, summed in block order in float64
    p_host = partials.cpu().numpy().astype(f64)
    summed = np.zeros(P + 4, f64)
    for b in range(grid):
        summed += p_host[b]
    got = {name: summed[lo:hi] for name, (lo, hi) in zip(pc.TENSOR_NAMES, bounds)}
    got.update({name: summed[P + i] for i, name in enumerate(pc.SUM_NAMES)})
    _judge(f"gradients {case.name}", got, want, yard, pc.TENSOR_NAMES + pc.SUM_NAMES)
    # ---- the reduce stage by itself: against the float64 sum of the partials it was given (the float32 computation of the
    # same quantity: torch's sum over the block axis on the device)
    g_host = grads.cpu().numpy()
    f32_sum = partials.sum(dim=0).cpu().numpy()
    got_r = {name: g_host[lo:hi] for name, (lo, hi) in zip(pc.TENSOR_NAMES, bounds)}
    got_r.update({name: sums[i].item() for i, name in enumerate(pc.SUM_NAMES)})
    want_r, yard_r = dict(got), {name: f32_sum[lo:hi] for name, (lo, hi) in zip(pc.TENSOR_NAMES, bounds)}
    yard_r.update({name: f32_sum[P + i] for i, name in enumerate(pc.SUM_NAMES)})
    _judge(f"reduce {case.name}", got_r, want_r, yard_r, pc.TENSOR_NAMES + pc.SUM_NAMES)
    ss_got = {name: sumsq[i].item() for i, name in enumerate(pc.TENSOR_NAMES)}
    ss_want = {name: float(np.sum(g_host[lo:hi].astype(f64) ** 2)) for name, (lo, hi) in zip(pc.TENSOR_NAMES, bounds)}
    ss_yard = {name: float((grads[lo:hi] * grads[lo:hi]).sum()) for name, (lo, hi) in zip(pc.TENSOR_NAMES, bounds)}
    _judge(f"sums of squares {case.name}", ss_got, ss_want, ss_yard, pc.TENSOR_NAMES)
    assert abs(k.gradient_norm(sumsq) - np.sqrt(sum(ss_want.values()))) <= 1e-5 * max(k.gradient_norm(sumsq), 1e-30)
    _inputs_as_they_were(d, inp)


def test_reduce_and_apply_launched_for_another_width_touch_nothing(fm):
    """the two entries that take the width as an argument, launched with 48 and with 0: every output keeps the sentinel"""
    case = gc.CASES[1]
    k = _kernels(fm, case)
    P = k.P
    for h in (48, 0):
        whole_g, grads = _sentinel((P,))
        whole_s, sumsq = _sentinel((8,))
        whole_l, sums = _sentinel((4,))
        whole_k, packed = _sentinel((k.packed_floats,))
        state = [_sentinel((P,)) for _ in range(3)]
        partials, g_in, ss_in = torch.zeros((2, P + 4), device=DEV), torch.zeros(P, device=DEV), torch.ones(8, device=DEV)
        k.fn_reduce(partials, np.int32(2), np.int32(h), grads, sumsq, sums, block=(1024, 1, 1), grid=(9, 1), shared=0)
        k.fn_apply(state[0][1], state[1][1], state[2][1], g_in, ss_in, packed, np.int32(h), f32(0.0), f32(1e-3), f32(1.0),
                   f32(0.1), f32(0.999), f32(0.001), f32(1e-8), block=(256, 1, 1), grid=(k.apply_grid, 1), shared=0)
        torch.cuda.synchronize()
        for whole in [whole_g, whole_s, whole_l, whole_k] + [w for w, _ in state]:
            assert bool((whole == pc.SENTINEL_BITS).all()), h


# ===================================================================================================== 5. apply
APPLY_CASES = tuple(pc.ApplyCase(f"H{H}-step{ac.step}-clip_{ac.clip}", H, 21, 5, ac.step, ac.clip, ac.max_norm, ac.lr, 60 + i)
                    for i, (ac, H) in enumerate(zip(pc.APPLY_CASES, (32, 64, 64, 64, 32, 32, 64, 32, 64))))


@pytest.mark.parametrize("ac", APPLY_CASES, ids=lambda a: a.name)
def test_apply_and_refill(fm, ac):
    """tests/pg_update_cases.py::APPLY_CASES' kinds of input -- clip active / inactive / off, Adam steps 1, 2, 1000 -- at
    O = 21, A = 5: parameters and both moments under the bound per tensor; a gradient of exactly 0 on fresh moments leaves
    its parameter and moments as they were; the packed tensor, PRE-FILLED WITH THE SENTINEL, equals pack_gridworld_policy of
    the updated module byte for byte afterwards (pad columns and tail written too); nothing else changes"""
    from warp_drive_amd.training import pg_update_gridworld_kernels as pggk
    from warp_drive_amd.training.policy_kernel import pack_gridworld_policy

    assert {(a.step, a.clip) for a in APPLY_CASES} == {(a.step, a.clip) for a in pc.APPLY_CASES}
    inp = pc.apply_inputs(ac)
    k = _kernels(fm, gc.CASES[1]._replace(H=ac.H))
    state = {}
    for key in ("theta", "exp_avg", "exp_avg_sq"):
        whole, view = _sentinel((k.P,))
        view.copy_(torch.from_numpy(inp[key]))
        state[key] = (whole, view)
    grads = _fenced(inp["grads"])
    # the sums of squares from the reduce launch itself, on one "block" whose partial is the gradient
    partial = _fenced(np.concatenate([inp["grads"], np.zeros(4, f32)])[None])
    whole_s, sumsq = _sentinel((8,))
    scratch_g, scratch_l = torch.zeros(k.P, device=DEV), torch.zeros(4, device=DEV)
    k.reduce(partials=partial, grads=scratch_g, sumsq=sumsq, sums=scratch_l)
    assert _same_bytes(scratch_g, grads)
    whole_k, packed = _sentinel((pggk.packed_floats(ac.H),))
    before = _counts()
    k.apply(state["theta"][1], state["exp_avg"][1], state["exp_avg_sq"][1], ac.step, ac.lr, max_norm=pc.apply_max_norm(ac),
            packed=packed, grads=grads, sumsq=sumsq)
    torch.cuda.synchronize()
    assert _launched_since(before) == {"HipPgGwApply": 1}
    for whole, view in list(state.values()) + [(whole_s, sumsq), (whole_k, packed)]:
        assert _untouched(whole, view), ac.name
    assert np.array_equal(pc.bits(grads.cpu().numpy()), pc.bits(inp["grads"]))
    want, yard = pc.apply_model(ac, inp), pc.framework_apply(ac, inp, torch.float32, DEV)
    got = {key: state[key][1].cpu().numpy() for key in state}
    flat = lambda res: {f"{key} {name}": np.asarray(res[key])[lo:hi] for key in state
                        for name, (lo, hi) in zip(pc.TENSOR_NAMES, pc.tensor_bounds(ac.H, 21, 5))}
    for key in state:
        keys = [name for name in flat(want) if name.startswith(key + " ")]
        _judge(f"apply {ac.name} {key}", flat(got), flat(want), flat(yard), keys, worst_only=True)
    zero = slice(0, None, pc.ZERO_EVERY)   # gradient and both moments exactly 0 there, at every step of the cases
    for key in ("theta", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(pc.bits(got[key][zero]), pc.bits(inp[key][zero])), key
    assert not np.array_equal(got["theta"], inp["theta"])
    model = pc.build_module(ac.H, 21, 5, got["theta"], torch.float32, DEV)
    assert _same_bytes(packed, pack_gridworld_policy(model)), ac.name
    assert np.array_equal(pc.bits(packed.cpu().numpy()), pc.bits(pggk.pack_from_flat(got["theta"], ac.H)))


# ============================================================================================== inside the trainer
def _trainer(tmp_path, E=25, T=6, fc=(32, 32), seed=3, log_freq=1, fused_update="all", rollout="all", policy_extra=None,
             env_extra=None, trainer_extra=None):
    """tag_gridworld at E = 25 (the rollout's groups of 12 replicas leave one over), T = 6"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    policies = {}
    for pol, lr in (("tagger", 0.002), ("runner", 0.005)):
        policies[pol] = {"to_train": True, "algorithm": "A2C", "clip_grad_norm": True, "max_grad_norm": 3, "gamma": 0.98,
                         "lr": lr, "vf_loss_coeff": 1, "entropy_coeff": 0.05, "normalize_advantage": False,
                         "normalize_return": False,
                         "model": {"type": "fully_connected", "fc_dims": list(fc), "model_ckpt_filepath": ""}}
        policies[pol].update((policy_extra or {}).get(pol, {}))
    trainer = {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": seed, "fused_rollout_policy": rollout}
    if fused_update is not None:
        trainer["fused_update"] = fused_update
    trainer.update(trainer_extra or {})
    ov = {"trainer": trainer, "policy": policies, "saving": {"metrics_log_freq": log_freq, "model_params_save_freq": 0},
          "env": {"episode_length": 5, "seed": 11, **(env_extra or {})}}
    torch.manual_seed(seed)
    return setup_trainer("tag_gridworld", ov, results_dir=str(tmp_path), verbose=False)


def _counting_pack(tr):
    packs = {}
    real_pack = tr._batch_rollout["pack"]

    def counting_pack(model, out=None):
        pol = next(p for p in tr.policies if tr.models[p] is model)
        packs[pol] = packs.get(pol, 0) + 1
        return real_pack(model, out=out)

    tr._batch_rollout["pack"] = counting_pack
    return packs


@pytest.mark.parametrize("fc,ppo", [((32, 32), "tagger"), ((64, 64), "runner")])
def test_composed_in_the_trainer(fc, ppo, tmp_path):
    """three iterations at E = 25, T = 6, both policies trained, one of them with PPO: both are on the kernels; every
    update is one launch of each of the five stages PER POLICY; its results are byte-identical to launching the stages
    directly on a snapshot; the framework's pack runs once per policy before the first update and never after; a logging
    iteration returns the framework path's keys, finite, within 2e-2 of a framework-path twin on the same seeds;
    forward_inference after an update equals forward; checkpoints of both policies go to a framework-path trainer and back"""
    from warp_drive_amd.training import pg_update_gridworld_kernels as pggk
    from warp_drive_amd.training.policy_kernel import pack_gridworld_policy

    E, T = 25, 6
    extra = {ppo: {"algorithm": "PPO", "clip_param": 0.1}}
    tr = _trainer(tmp_path / "k", fc=fc, policy_extra=extra)
    ref = _trainer(tmp_path / "f", fc=fc, policy_extra=extra, fused_update=None)
    assert tr.update_path == {"tagger": "kernels", "runner": "kernels"}
    assert ref.update_path == {"tagger": "framework", "runner": "framework"}
    assert tr._batch_rollout is not None and ref._batch_rollout is not None
    assert tr.engine.step_kernel_name == f"HipTagGridWorldRollout_N5_H{fc[0]}"
    direct = {}
    for pol, n in POLICIES.items():
        k = tr._pg_kernels[pol]
        assert isinstance(k, pggk.PgGridworldUpdateKernels) and (k.E, k.T, k.n, k.H) == (E, T, n, fc[0])
        assert tr.batch[pol]["obs"][:T].shape == (T, E, n, 21) and tr.batch[pol]["actions"].dtype == torch.int32
        direct[pol] = pggk.PgGridworldUpdateKernels(tr.w.cuda_function_manager, E, T, n, fc[0], DEV)
    packs = _counting_pack(tr)
    probes = {pol: tr.batch[pol]["obs"][0].clone().normal_() for pol in POLICIES}
    for it in range(3):
        log = it == 1
        tr._generate_rollout_batch()
        ref._generate_rollout_batch()
        assert packs == {"tagger": 1, "runner": 1}, "the framework's pack runs before the first update only"
        for pol in POLICIES:
            tr.models[pol].forward_inference(probes[pol])     # (fills the cache an update must not leave stale)
        torch.cuda.synchronize()
        snaps, coeffs = {}, {}
        for pol in POLICIES:
            flat, adam, objective = tr._pg_flat[pol], tr._pg_adam[pol], tr.trainers[pol]
            snaps[pol] = {"theta": flat.flat.clone(), "m": adam["exp_avg"].clone(), "v": adam["exp_avg_sq"].clone(),
                          "step": adam["step"]}
            ts = tr.current_timestep[pol]
            coeffs[pol] = (objective.entropy_coeff_schedule.get_param_value(ts), objective.vf_loss_coeff_schedule.get_param_value(ts))
        before = _counts()
        metrics = tr._update_model_params(it, log)
        torch.cuda.synchronize()
        assert _launched_since(before) == {s: 2 for s in GW_STAGES}, (it, _launched_since(before))
        ref_metrics = ref._update_model_params(it, log)
        if log:
            for pol in POLICIES:
                assert set(metrics[pol]) == set(ref_metrics[pol])
                bad = {key: v for key, v in metrics[pol].items() if not np.isfinite(v) and not (pol == "runner" and "over agents" in key)}
                assert not bad, (pol, bad)
                for key in ("Mean rewards", "Value function loss", "Mean entropy", "Policy loss", "Total loss"):
                    assert abs(metrics[pol][key] - ref_metrics[pol][key]) <= 2e-2 * max(1.0, abs(ref_metrics[pol][key])), (pol, key)
        else:
            assert metrics == {}
        for pol in POLICIES:
            model, pcfg, flat, adam, snap = tr.models[pol], tr.config["policy"][pol], tr._pg_flat[pol], tr._pg_adam[pol], snaps[pol]
            assert adam["step"] == snap["step"] + 1 and tr.current_timestep[pol] == (it + 1) * E * T
            b, st, dk = tr.batch[pol], {key: v.clone() for key, v in snap.items() if key != "step"}, direct[pol]
            whole_k, packed = _sentinel((pggk.packed_floats(fc[0]),))
            ent_c, vf_c = coeffs[pol]
            dk.compute_values(b["obs"][:T], st["theta"])
            dk.discounted_returns(b["rewards"][:T], tr.done_batch[:T], pcfg["gamma"])
            dk.gradients(b["obs"][:T], b["actions"][:T], st["theta"], ent_c, vf_c)
            dk.reduce()
            dk.apply(st["theta"], st["m"], st["v"], snap["step"] + 1, pcfg["lr"], max_norm=pcfg["max_grad_norm"], packed=packed)
            torch.cuda.synchronize()
            assert _same_bytes(st["theta"], flat.flat) and _same_bytes(st["m"], adam["exp_avg"]), (it, pol)
            assert _same_bytes(st["v"], adam["exp_avg_sq"]), (it, pol)
            assert _untouched(whole_k, packed) and _same_bytes(packed, pack_gridworld_policy(model))
            assert _same_bytes(tr._batch_rollout["packed"][pol], packed)
            k = tr._pg_kernels[pol]
            assert _same_bytes(dk.values, k.values) and _same_bytes(dk.returns, k.returns) and _same_bytes(dk.grads, k.grads)
            assert not _same_bytes(snap["theta"], flat.flat) and flat.bound()
            with torch.no_grad():
                probs_i, values_i = model.forward_inference(probes[pol])
                probs_f, values_f = model(probes[pol])
            assert torch.allclose(probs_i[0], probs_f[0], rtol=0, atol=1e-6) and torch.allclose(values_i, values_f, rtol=0, atol=1e-6)
    # the modules are the source of truth: state_dict, save, load, and a framework-path trainer loads the files; and back
    tr.save_model_checkpoint()
    for pol in POLICIES:
        path = os.path.join(tr.save_dir, f"{pol}_{tr.current_timestep[pol]}.state_dict")
        saved = copy.deepcopy(tr.models[pol].state_dict())
        ref.load_model_checkpoint({pol: path})
        for key, v in saved.items():
            assert torch.equal(ref.models[pol].state_dict()[key], v), (pol, key)
    ref._generate_rollout_batch()
    ref._update_model_params(3, False)
    for pol in POLICIES:
        ref.current_timestep[pol] = 777
    ref.save_model_checkpoint()
    for pol in POLICIES:
        tr.load_model_checkpoint({pol: os.path.join(ref.save_dir, f"{pol}_777.state_dict")})
        assert tr.current_timestep[pol] == 777 and tr._pg_flat[pol].bound()
        for key, v in ref.models[pol].state_dict().items():
            assert torch.equal(tr.models[pol].state_dict()[key], v), (pol, key)
    tr._generate_rollout_batch()          # a framework-side change: the rollout repacks, with the loaded weights
    assert packs == {"tagger": 2, "runner": 2}
    for pol in POLICIES:
        assert _same_bytes(tr._batch_rollout["packed"][pol], pack_gridworld_policy(tr.models[pol]))
    tr._update_model_params(3, False)     # ... and the update goes on from the loaded state
    tr._generate_rollout_batch()
    torch.cuda.synchronize()
    assert packs == {"tagger": 2, "runner": 2}
    assert all(bool(torch.isfinite(tr._pg_flat[pol].flat).all()) for pol in POLICIES)
    for t in (tr, ref):
        t.graceful_close()


def _said(caplog):
    return [r.getMessage() for r in caplog.records if "trainer.fused_update" in r.getMessage()]


def test_a_policy_that_is_not_trained_is_never_touched(tmp_path, caplog):
    import logging

    with caplog.at_level(logging.INFO):
        tr = _trainer(tmp_path, policy_extra={"runner": {"to_train": False}})
    assert tr.update_path == {"tagger": "kernels", "runner": "framework"} and set(tr._pg_kernels) == {"tagger"}
    assert _said(caplog) == []
    runner = [p.detach().clone() for p in tr.models["runner"].parameters()]
    tagger = tr._pg_flat["tagger"].flat.clone()
    for it in range(3):
        tr._generate_rollout_batch()
        before = _counts()
        tr._update_model_params(it, it == 1)
        torch.cuda.synchronize()
        assert _launched_since(before) == {s: 1 for s in GW_STAGES}
    assert all(_same_bytes(p, q) for p, q in zip(tr.models["runner"].parameters(), runner))
    assert not _same_bytes(tagger, tr._pg_flat["tagger"].flat)
    tr.graceful_close()


def test_a_refused_policy_stays_on_the_framework_path_beside_one_on_the_kernels(tmp_path, caplog):
    import logging

    with caplog.at_level(logging.INFO):
        tr = _trainer(tmp_path, policy_extra={"runner": {"normalize_advantage": True}})
    assert tr.update_path == {"tagger": "kernels", "runner": "framework"} and set(tr._pg_kernels) == {"tagger"}
    said = _said(caplog)
    assert len(said) == 1 and "'runner'" in said[0] and "normalize_advantage" in said[0] and "framework path" in said[0], said
    first = {pol: [p.detach().clone() for p in tr.models[pol].parameters()] for pol in POLICIES}
    for it in range(3):
        tr._generate_rollout_batch()
        before = _counts()
        metrics = tr._update_model_params(it, True)
        torch.cuda.synchronize()
        launched = _launched_since(before)   # (the runner's framework path may launch the returns entry as well)
        assert {s: launched.get(s) for s in GW_STAGES if s.startswith("HipPgGw")} == {s: 1 for s in GW_STAGES if s.startswith("HipPgGw")}
        assert launched.get("HipDiscountedReturns", 0) >= 1 and set(launched) <= set(GW_STAGES), launched
        assert all(np.isfinite(metrics[pol]["Total loss"]) for pol in POLICIES)
    for pol in POLICIES:
        assert all(not torch.equal(p, q) for p, q in zip(tr.models[pol].parameters(), first[pol])), pol
    tr.graceful_close()


def test_three_taggers_train_on_the_framework_path(tmp_path, caplog):
    import logging

    with caplog.at_level(logging.INFO):
        tr = _trainer(tmp_path, env_extra={"num_taggers": 3})
    assert tr._batch_rollout is None                                    # the one-launch rollout exists for 5 agents
    assert tr.update_path == {"tagger": "framework", "runner": "framework"} and tr._pg_kernels == {}
    said = _said(caplog)
    assert len(said) == 2 and all("framework path" in s for s in said), said
    before = _counts()
    for it in range(2):
        tr._generate_rollout_batch()
        metrics = tr._update_model_params(it, True)
        assert all(np.isfinite(metrics[pol]["Total loss"]) for pol in POLICIES)
    assert not [s for s in _launched_since(before) if s.startswith("HipPg")]
    tr.graceful_close()


# Recorded on the MI355X with the PARENT commit's (6e67eb9) training/trainer.py and training/pg_update_kernels.py in place of
# this tree's, and on this tree: `_parameter_checksum` after three iterations of the two trainers below, same seeds.
DEFAULT_PATH_CHECKSUM = "0657c2daf751bc5412a1e44beda1088fa3f4df19060a7e67edfda00d11a171c8"


def _parameter_checksum(trainers):
    h = hashlib.sha256()
    for tr in trainers:
        for pol in ("tagger", "runner"):
            for p in tr.models[pol].parameters():
                h.update(p.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def default_path_run(tmp_path):
    """tag_gridworld on the one-launch rollout WITHOUT `fused_update` and with `fused_update: True`, three iterations each
    at E = 25, T = 6 -> ({policy: path} of each, the sha256 of the bytes of every parameter)"""
    trainers = [_trainer(os.path.join(str(tmp_path), name), fused_update=value) for name, value in (("none", None), ("true", True))]
    for tr in trainers:
        assert tr._batch_rollout is not None
        for it in range(3):
            tr._generate_rollout_batch()
            tr._update_model_params(it, it == 2)
    torch.cuda.synchronize()
    paths = [getattr(tr, "update_path", None) for tr in trainers]
    checksum = _parameter_checksum(trainers)
    for tr in trainers:
        tr.graceful_close()
    return paths, checksum


def test_default_path_is_the_parent_commits(tmp_path):
    paths, checksum = default_path_run(tmp_path)
    print("default path checksum", checksum)
    assert all(p == {"tagger": "framework", "runner": "framework"} for p in paths) and checksum == DEFAULT_PATH_CHECKSUM


# ------------------------------------------------------------------------------------------------------- learning
def test_gridworld_taggers_learn_with_the_update_kernels(tmp_path):
    """tests/test_gpu_learning.py::test_gridworld_taggers_learn_to_catch_a_random_runner's "one launch per batch" settings
    and its bar (the last 10 of 60 iterations at least 3 above the first 3; measured there as -0.3 -> 6.2) with
    `fused_update: "all"` added: every update of the taggers is five launches, the runner keeps its random initial policy."""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    pol = {p: {"to_train": p == "tagger", "algorithm": "A2C", "vf_loss_coeff": 1, "entropy_coeff": 0.05, "gamma": 0.98,
               "lr": 0.001, "model": {"type": "fully_connected", "fc_dims": [32, 32], "model_ckpt_filepath": ""}}
           for p in ("runner", "tagger")}
    ov = {"trainer": {"num_envs": 600, "train_batch_size": 600 * 100, "num_episodes": 10 ** 6, "seed": 7, "fused_update": "all"},
          "policy": pol, "env": {"grid_length": 20}, "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0}}
    torch.manual_seed(0)
    tr = setup_trainer("tag_gridworld", ov, results_dir=str(tmp_path), verbose=False)
    assert tr._batch_rollout is not None and tr.update_path["tagger"] == "kernels"
    tr.train(60)
    tr.graceful_close()
    curve = [json.loads(line)["tagger"]["Mean episodic reward"] for line in open(os.path.join(str(tmp_path), "results.json"))]
    assert len(curve) == 60 and all(np.isfinite(curve))
    first, last = float(np.mean(curve[:3])), float(np.mean(curve[-10:]))
    print(f"gridworld taggers, one launch per batch, update kernels: mean episodic reward {first:.2f} -> {last:.2f}")
    assert last >= first + 3.0, (first, last, curve[::5])
