"""The A2C / PPO update kernels on the device (wd_kernels_pg.hsaco; cases, inputs and yardsticks: tests/pg_update_cases.py),
stage by stage from each stage's own inputs, then composed inside Trainer (`trainer.fused_update: "all"`).

Conventions (those of tests/test_gpu_ddpg_update.py):
  * an output lies inside an allocation filled with a sentinel NaN, with surplus rows / blocks, and everything outside the
    region the launch must write is compared byte for byte afterwards; the region itself starts as the sentinel too;
  * a float input is a view that ENDS inside a larger allocation that goes on with NaN;
  * every launch goes through the wrappers of training/pg_update_kernels.py and is counted in hip_driver.LAUNCH_COUNTS;
  * per result tensor err <= max(4 * err_f32, 2e-6 * scale): err against the float64 yardstick, err_f32 the error of the
    framework's float32 computation of the same quantity from the same inputs on the device, scale the largest float64
    magnitude; err / err_f32 is printed per tensor (pytest -s)."""
import copy
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DEV = torch.device("cuda:0")
STAGES = ("HipPgValues", "HipDiscountedReturns", "HipPgGradients", "HipPgReduce", "HipPgApply")


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
    for case in pc.CASES:
        inp = pc.inputs(case)
        out[case.name] = (inp, pc.yardstick(case, inp))
    return out


def _kernels(fm, case):
    from warp_drive_amd.training.pg_update_kernels import PgUpdateKernels

    return PgUpdateKernels(fm, case.E, case.T, case.H, case.O, case.A, DEV)


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


def _fenced(a, dtype=torch.float32):
    """numpy array -> a device view of its shape that ends inside an allocation going on with NaN (int32: with -1)"""
    a = np.ascontiguousarray(a)
    fill = float("nan") if dtype == torch.float32 else -1
    base = torch.full((a.size + 72,), fill, dtype=dtype, device=DEV)
    view = base[:a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _sentinel(shape, surplus=3):
    """(whole allocation as int32, the float32 view of `shape` a launch is given): everything holds the sentinel;
    `surplus` more leading rows follow the view"""
    n = int(np.prod(shape))
    extra = surplus * int(np.prod(shape[1:])) if len(shape) > 1 else surplus
    whole = torch.full((n + extra,), pc.SENTINEL_BITS, dtype=torch.int32, device=DEV)
    return whole, whole[:n].view(torch.float32).view(shape)


def _untouched(whole, view):
    return bool((whole[view.numel():] == pc.SENTINEL_BITS).all())


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _judge(tag, got, want, yard, keys, worst_only=False):
    ratios, failures = {}, []
    for k in keys:
        g = np.asarray(got[k], f64)
        assert np.isfinite(g).all(), (tag, k, "not finite")
        ok, err, err_f32, scale, ratio = pc.compare(g.reshape(-1), np.asarray(want[k], f64).reshape(-1),
                                                    np.asarray(yard[k], f64).reshape(-1))
        ratios[k] = ratio
        if not ok:
            failures.append((k, err, err_f32, scale))
    if worst_only:
        worst = max(ratios, key=ratios.get)
        ratios = {f"worst of {len(ratios)}: {worst}": ratios[worst]}
    print(f"{tag}: err / err_f32 " + ", ".join(f"{k} {v:.2f}" for k, v in ratios.items()))
    assert not failures, (tag, failures)


def _device_inputs(inp):
    T, E, O = inp["obs"].shape
    return {"obs": _fenced(inp["obs"].reshape(T, E, 1, O)), "actions": _fenced(inp["actions"].reshape(T, E, 1, 1), torch.int32),
            "rewards": _fenced(inp["rewards"].reshape(T, E, 1)), "done": _fenced(inp["done"], torch.int32),
            "theta": _fenced(inp["theta"])}


def _inputs_as_they_were(d, inp):
    for key in d:
        assert np.array_equal(pc.bits(d[key].cpu().numpy().reshape(-1)), pc.bits(np.ascontiguousarray(inp[key]).reshape(-1))), key


# ================================================================================================ 1 + 2. values, returns
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_values_and_returns(fm, references, case):
    """values under the bound against float64 -- at the wrapper's geometry, and bit-identical at one block of 64 threads
    (grid-stride trips) and with surplus blocks; the returns the existing entry forms from them equal
    losses.discounted_returns on the kernel's own values bit for bit, the advantages are returns - values"""
    from warp_drive_amd.training.losses import discounted_returns

    inp, want = references[case.name]
    k, d = _kernels(fm, case), _device_inputs(inp)
    T, E = case.T, case.E
    results = []
    for block, grid in ((None, None), (64, 1), (128, -(-T * E // 128) + 3)):
        whole, out = _sentinel((T, E))
        before = _counts()
        k.compute_values(d["obs"], d["theta"], out=out, block=block, grid=grid)
        torch.cuda.synchronize()
        assert _launched_since(before) == {"HipPgValues": 1}
        assert _untouched(whole, out), (case.name, block, grid)
        results.append(out)
    assert _same_bytes(results[0], results[1]) and _same_bytes(results[0], results[2])
    yard = pc.framework(case, inp, torch.float32, DEV)
    _judge(f"values {case.name}", {"values": results[0].cpu().numpy()}, want, yard, ["values"])

    whole_r, returns = _sentinel((T, E))
    whole_a, adv = _sentinel((T, E))
    before = _counts()
    k.discounted_returns(d["rewards"], d["done"], case.gamma, values=results[0], returns=returns, advantages=adv)
    torch.cuda.synchronize()
    assert _launched_since(before) == {"HipDiscountedReturns": 1}
    assert _untouched(whole_r, returns) and _untouched(whole_a, adv)
    ref = discounted_returns(d["rewards"], d["done"], results[0].reshape(T, E, 1), case.gamma).reshape(T, E)
    assert _same_bytes(returns, ref), case.name
    assert _same_bytes(adv, ref - results[0]), case.name
    model = pc.returns_model(inp["rewards"], inp["done"], results[0].cpu().numpy(), case.gamma, f32)
    assert np.array_equal(pc.bits(returns.cpu().numpy()), pc.bits(model))
    _inputs_as_they_were(d, inp)


# ============================================================================================ 3 + 4. gradients, reduce
@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_gradients_after_reduce(fm, references, case):
    """from the kernel's own values, returns and advantages: the eight gradients and the four sums under the bound against
    float64, the per-tensor sums of squares against those of the kernel's own gradients; blocks without rows write zeros;
    nothing outside the written regions changes; a second run gives the same bytes"""
    from warp_drive_amd.training import pg_update_kernels as pguk

    inp, _ = references[case.name]
    k, d = _kernels(fm, case), _device_inputs(inp)
    values = k.compute_values(d["obs"], d["theta"]).clone()
    returns, adv = k.discounted_returns(d["rewards"], d["done"], case.gamma, values=values)
    returns, adv = returns.clone(), adv.clone()
    v_host = values.cpu().numpy()
    want = pc.yardstick(case, inp, values=v_host)
    yard = pc.framework(case, inp, torch.float32, DEV, values=v_host)
    grid = pc.case_grid(case)
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
        assert _launched_since(before) == {"HipPgGradients": 1, "HipPgReduce": 1}
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
    g_host = grads.cpu().numpy()
    bounds = pc.tensor_bounds(case.H, case.O, case.A)
    got = {name: g_host[lo:hi] for name, (lo, hi) in zip(pc.TENSOR_NAMES, bounds)}
    got.update({name: sums[i].item() for i, name in enumerate(pc.SUM_NAMES)})
    _judge(f"gradients {case.name}", got, want, yard, pc.TENSOR_NAMES + pc.SUM_NAMES)
    ss_got = {n: sumsq[i].item() for i, n in enumerate(pc.TENSOR_NAMES)}
    ss_want = {n: float(np.sum(g_host[lo:hi].astype(f64) ** 2)) for n, (lo, hi) in zip(pc.TENSOR_NAMES, bounds)}
    ss_yard = {n: float((grads[lo:hi] * grads[lo:hi]).sum()) for n, (lo, hi) in zip(pc.TENSOR_NAMES, bounds)}
    _judge(f"sums of squares {case.name}", ss_got, ss_want, ss_yard, pc.TENSOR_NAMES)
    assert abs(k.gradient_norm(sumsq) - np.sqrt(sum(ss_want.values()))) <= 1e-5 * max(k.gradient_norm(sumsq), 1e-30)
    assert pguk.TILE == pc.TILE
    _inputs_as_they_were(d, inp)


def test_an_entry_launched_for_another_shape_touches_nothing(fm):
    """another width, another observation size, A = 0 and A = 9, for all four entries: every output keeps the sentinel"""
    case = pc.CASES[2]
    inp = pc.inputs(case)
    k, d = _kernels(fm, case), _device_inputs(inp)
    T, E, H, O, A = case.T, case.E, case.H, case.O, case.A
    P = k.P
    for h, o, a in ((32, O, A), (H, 4, A), (H, O, 0), (H, O, 9)):
        whole_v, values = _sentinel((T, E))
        whole_p, partials = _sentinel((k.gradients_grid, P + 4))
        whole_g, grads = _sentinel((P,))
        whole_s, sumsq = _sentinel((8,))
        whole_l, sums = _sentinel((4,))
        state = [_sentinel((P,)) for _ in range(3)]
        shape = (np.int32(h), np.int32(o), np.int32(a))
        adv, ret = torch.zeros(T * E, device=DEV), torch.zeros(T * E, device=DEV)
        k.fn_values(d["obs"], d["theta"], np.int64(T * E), *shape, values, block=(64, 1, 1), grid=(2, 1), shared=k.values_lds)
        k.fn_gradients(d["obs"], d["actions"], adv, ret, d["theta"], np.int64(T * E), *shape, f32(1.0), f32(0.1), f32(0.1),
                       partials, block=(128, 1, 1), grid=(k.gradients_grid, 1), shared=k.gradients_lds)
        if (h, o) == (H, O):   # (the two shape-free entries refuse A outside 1 .. 8)
            k.fn_reduce(partials, np.int32(k.gradients_grid), *shape, grads, sumsq, sums, block=(1024, 1, 1), grid=(9, 1), shared=0)
            k.fn_apply(state[0][1], state[1][1], state[2][1], d["theta"], sumsq, np.uint64(0), *shape, f32(0.0), f32(1e-3),
                       f32(1.0), f32(0.1), f32(0.999), f32(0.001), f32(1e-8), block=(256, 1, 1), grid=(k.apply_grid, 1), shared=0)
        torch.cuda.synchronize()
        for whole in [whole_v, whole_p, whole_g, whole_s, whole_l] + [w for w, _ in state]:
            assert bool((whole == pc.SENTINEL_BITS).all()), (h, o, a)


# ===================================================================================================== 5. apply
@pytest.mark.parametrize("ac", pc.APPLY_CASES, ids=lambda a: a.name)
def test_apply(fm, ac):
    """clip (active / inactive / off) + Adam (steps 1, 2, 1000) from given float32 gradients: parameters and both moments
    under the bound per tensor; a gradient of exactly 0 on fresh moments leaves its parameter and moments as they were; the
    packed policy equals pack_rollout_policy of the updated module byte for byte; nothing outside the three buffers and the
    packed policy changes"""
    from warp_drive_amd.training import pg_update_kernels as pguk
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    inp = pc.apply_inputs(ac)
    case = pc.CASES[0]._replace(E=64, T=2, H=ac.H, O=ac.O, A=ac.A)
    k = _kernels(fm, case)
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
    whole_k, packed = _sentinel((pguk.packed_floats(ac.H, ac.O, ac.A),))
    before = _counts()
    k.apply(state["theta"][1], state["exp_avg"][1], state["exp_avg_sq"][1], ac.step, ac.lr, max_norm=pc.apply_max_norm(ac),
            packed=packed, grads=grads, sumsq=sumsq)
    torch.cuda.synchronize()
    assert _launched_since(before) == {"HipPgApply": 1}
    for whole, view in list(state.values()) + [(whole_s, sumsq), (whole_k, packed)]:
        assert _untouched(whole, view), ac.name
    assert np.array_equal(pc.bits(grads.cpu().numpy()), pc.bits(inp["grads"]))
    want, yard = pc.apply_model(ac, inp), pc.framework_apply(ac, inp, torch.float32, DEV)
    got = {key: state[key][1].cpu().numpy() for key in state}
    flat = lambda res: {f"{key} {name}": np.asarray(res[key])[lo:hi] for key in state
                        for name, (lo, hi) in zip(pc.TENSOR_NAMES, pc.tensor_bounds(ac.H, ac.O, ac.A))}
    for key in state:
        keys = [n for n in flat(want) if n.startswith(key + " ")]
        _judge(f"apply {ac.name} {key}", flat(got), flat(want), flat(yard), keys, worst_only=True)
    zero = slice(0, None, pc.ZERO_EVERY)   # gradient and both moments exactly 0 there, at every step of the cases
    for key in ("theta", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(pc.bits(got[key][zero]), pc.bits(inp[key][zero])), key
    assert not np.array_equal(got["theta"], inp["theta"])
    model = pc.build_module(ac.H, ac.O, ac.A, got["theta"], torch.float32, DEV)
    assert _same_bytes(packed, pack_rollout_policy(model)), ac.name


# ============================================================================================== inside the trainer
ENVS = {"cartpole": (4, 2), "acrobot": (6, 3), "mountain_car": (2, 3)}   # env -> (observation size, actions)


def _trainer(tmp_path, env="cartpole", E=64, T=6, fc=(32, 32), seed=3, log_freq=1, fused_update="all", rollout="all",
             policy_extra=None, env_cfg=None, trainer_extra=None):
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    policy = {"to_train": True, "algorithm": "A2C", "clip_grad_norm": True, "max_grad_norm": 3, "gamma": 0.99, "lr": 0.001,
              "vf_loss_coeff": 0.1, "entropy_coeff": 0.05, "normalize_advantage": False, "normalize_return": False,
              "model": {"type": "fully_connected", "fc_dims": list(fc), "model_ckpt_filepath": ""}}
    policy.update(policy_extra or {})
    trainer = {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": seed, "fused_rollout_policy": rollout}
    if fused_update is not None:
        trainer["fused_update"] = fused_update
    trainer.update(trainer_extra or {})
    ov = {"trainer": trainer, "policy": {"shared": policy},
          "saving": {"metrics_log_freq": log_freq, "model_params_save_freq": 0},
          "env": env_cfg or {"episode_length": 5, "seed": 11}}
    torch.manual_seed(seed)
    return setup_trainer(f"single_{env}", ov, results_dir=str(tmp_path), verbose=False)


@pytest.mark.parametrize("env,fc,algo", [("cartpole", (32, 32), "A2C"), ("acrobot", (64, 64), "PPO"), ("mountain_car", (32, 32), "A2C")])
def test_composed_in_the_trainer(env, fc, algo, tmp_path):
    """three iterations at E = 64, T = 6 under `fused_rollout_policy: "all"` + `fused_update: "all"`: `_update_model_params`
    is the five launches; its results are byte-identical to launching the stages directly on a snapshot of the same state;
    the rollout repacks once (before the first update) and never after; a logging iteration returns the framework path's
    keys, finite; forward_inference after an update equals forward; checkpoints go to a framework-path trainer and back"""
    from warp_drive_amd.training import pg_update_kernels as pguk
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    pol = "shared"
    extra = {"algorithm": algo, "clip_param": 0.1}
    tr = _trainer(tmp_path / "k", env, fc=fc, policy_extra=extra)
    ref = _trainer(tmp_path / "f", env, fc=fc, policy_extra=extra, fused_update=None)
    assert tr.update_path == {pol: "kernels"} and ref.update_path == {pol: "framework"}
    assert tr._batch_rollout is not None and ref._batch_rollout is not None
    O, A = ENVS[env]
    k = tr._pg_kernels[pol]
    assert (k.E, k.T, k.H, k.O, k.A) == (64, 6, fc[0], O, A)
    direct = pguk.PgUpdateKernels(tr.w.cuda_function_manager, 64, 6, fc[0], O, A, DEV)
    packs = {"n": 0}
    real_pack = tr._batch_rollout["pack"]

    def counting_pack(model, out=None):
        packs["n"] += 1
        return real_pack(model, out=out)

    tr._batch_rollout["pack"] = counting_pack
    model, pcfg = tr.models[pol], tr.config["policy"][pol]
    probe = tr.batch[pol]["obs"][0].clone()
    for it in range(3):
        log = it == 1
        tr._generate_rollout_batch()
        ref._generate_rollout_batch()
        assert packs["n"] == 1, "the framework's repack runs before the first update only"
        model.forward_inference(probe)     # (fills the cache an update must not leave stale)
        torch.cuda.synchronize()
        flat, adam = tr._pg_flat[pol], tr._pg_adam[pol]
        snap = {"theta": flat.flat.clone(), "m": adam["exp_avg"].clone(), "v": adam["exp_avg_sq"].clone(), "step": adam["step"]}
        before = _counts()
        metrics = tr._update_model_params(it, log)
        torch.cuda.synchronize()
        assert _launched_since(before) == {s: 1 for s in STAGES}, (it, _launched_since(before))
        ref_metrics = ref._update_model_params(it, log)
        if log:
            assert set(metrics[pol]) == set(ref_metrics[pol])
            bad = {key: v for key, v in metrics[pol].items() if not np.isfinite(v) and "over agents" not in key}
            assert not bad, bad
            # (the two trainers have seen the same batches with the same weights up to float32 rounding of the update; a sampled
            # action that flips on that rounding moves a mean over 384 rows by a fraction of a percent)
            for key in ("Mean rewards", "Value function loss", "Mean entropy", "Policy loss", "Total loss"):
                assert abs(metrics[pol][key] - ref_metrics[pol][key]) <= 2e-2 * max(1.0, abs(ref_metrics[pol][key])), key
        else:
            assert metrics == {}
        assert adam["step"] == snap["step"] + 1 and tr.current_timestep[pol] == (it + 1) * 64 * 6
        b = tr.batch[pol]
        st = {key: v.clone() for key, v in snap.items() if key != "step"}
        packed = torch.zeros_like(pack_rollout_policy(model))
        direct.compute_values(b["obs"][:6], st["theta"])
        direct.discounted_returns(b["rewards"][:6], tr.done_batch[:6], pcfg["gamma"])
        direct.gradients(b["obs"][:6], b["actions"][:6], st["theta"], pcfg["entropy_coeff"], pcfg["vf_loss_coeff"])
        direct.reduce()
        direct.apply(st["theta"], st["m"], st["v"], snap["step"] + 1, pcfg["lr"], max_norm=pcfg["max_grad_norm"], packed=packed)
        torch.cuda.synchronize()
        assert _same_bytes(st["theta"], flat.flat) and _same_bytes(st["m"], adam["exp_avg"]) and _same_bytes(st["v"], adam["exp_avg_sq"]), it
        assert _same_bytes(packed, pack_rollout_policy(model)) and _same_bytes(tr._batch_rollout["packed"][pol], packed)
        assert _same_bytes(direct.values, k.values) and _same_bytes(direct.returns, k.returns)
        assert not _same_bytes(snap["theta"], flat.flat) and flat.bound()
        with torch.no_grad():
            probs_i, values_i = model.forward_inference(probe)
            probs_f, values_f = model(probe)
        assert torch.allclose(probs_i[0], probs_f[0], rtol=0, atol=1e-6) and torch.allclose(values_i, values_f, rtol=0, atol=1e-6)
    # the module is the source of truth: state_dict, save, load, and a framework-path trainer loads the file; and back
    tr.save_model_checkpoint()
    path = os.path.join(tr.save_dir, f"{pol}_{tr.current_timestep[pol]}.state_dict")
    saved = copy.deepcopy(model.state_dict())
    ref.load_model_checkpoint({pol: path})
    for key, v in saved.items():
        assert torch.equal(ref.models[pol].state_dict()[key], v), key
    ref._generate_rollout_batch()
    ref._update_model_params(3, False)
    ref.current_timestep[pol] = 777
    ref.save_model_checkpoint()
    tr.load_model_checkpoint({pol: os.path.join(ref.save_dir, f"{pol}_777.state_dict")})
    assert tr.current_timestep[pol] == 777 and tr._pg_flat[pol].bound()
    for key, v in ref.models[pol].state_dict().items():
        assert torch.equal(model.state_dict()[key], v), key
    tr._generate_rollout_batch()          # a framework-side change: the rollout repacks, with the loaded weights
    assert packs["n"] == 2 and _same_bytes(tr._batch_rollout["packed"][pol], pack_rollout_policy(model))
    tr._update_model_params(3, False)     # ... and the update goes on from the loaded state
    tr._generate_rollout_batch()
    torch.cuda.synchronize()
    assert packs["n"] == 2 and bool(torch.isfinite(tr._pg_flat[pol].flat).all())
    for t in (tr, ref):
        t.graceful_close()


def test_the_per_tick_forward_kernel_follows_the_update_kernels(tmp_path):
    """A [64, 64] policy on at least `fused_policy_forward_min_rows` rows also has a FusedPolicyForward, whose packed copy of
    the weights `_policy_probabilities` -- the per-tick evaluation, `fetch_episode_states` -- reads.  After updates on the
    kernels path it gives the CURRENT network's probabilities (the forward kernel's arithmetic is float32-accurate: 1e-5),
    which are far from those of the weights it was packed from at construction; so does a per-tick `evaluate_episodes`'
    first forward, and a checkpoint load in between changes nothing about that."""
    pol = "shared"
    tr = _trainer(tmp_path, "cartpole", fc=(64, 64), trainer_extra={"fused_policy_forward_min_rows": 0},
                  policy_extra={"lr": 0.01})
    assert tr.update_path == {pol: "kernels"} and tr._fused_forward[pol] is not None
    model = tr.models[pol]
    first = copy.deepcopy(model.state_dict())
    old = pc.build_module(64, 4, 2, np.zeros(pc.net_floats(64, 4, 2), f32), torch.float32, DEV)
    old.load_state_dict(first)

    def compare():
        obs = tr.obs.reshape(tr.num_envs, 1, -1)
        got = tr._policy_probabilities()[pol][0].clone()
        with torch.no_grad():
            want, stale = model(obs)[0][0], old(obs)[0][0]
        assert tr._pg_stale_forward == set()
        return float((got - want).abs().max()), float((stale - want).abs().max())

    err, moved = compare()
    assert err <= 1e-5 and moved == 0.0
    for it in range(5):
        tr._generate_rollout_batch()
        tr._update_model_params(it, False)
        assert tr._pg_stale_forward == {pol}
    err, moved = compare()
    print(f"per-tick forward kernel after 5 updates: {err:.2e} from forward, the construction-time weights {moved:.2e}")
    assert moved > 1e-3 and err <= 1e-5, (err, moved)
    tr._generate_rollout_batch()
    tr._update_model_params(5, False)
    assert tr._pg_stale_forward == {pol}
    _, _, _, probabilities = tr.fetch_episode_states([], include_probabilities=True, include_rewards_actions=True)
    assert tr._pg_stale_forward == set()
    probs0 = probabilities[0][pol][0]                 # tick 0, replica 0
    err, moved = compare()
    assert moved > 1e-3 and err <= 1e-5 and np.isfinite(probs0).all(), (err, moved)
    tr.graceful_close()


@pytest.mark.parametrize("change,why", [({"fc": (48, 48)}, "hidden width 48"),
                                        ({"fc": (32, 32, 32)}, "3 hidden layers"),
                                        ({"policy_extra": {"normalize_advantage": True}}, "normalize_advantage"),
                                        ({"rollout": False}, "per tick")])
def test_refused_shapes_train_on_the_framework_path(change, why, tmp_path, caplog):
    import logging

    with caplog.at_level(logging.INFO):
        tr = _trainer(tmp_path, "cartpole", **change)
    assert tr.update_path == {"shared": "framework"} and tr._pg_kernels == {}
    said = [r.getMessage() for r in caplog.records if "trainer.fused_update" in r.getMessage()]
    assert len(said) == 1 and why in said[0] and "framework path" in said[0], said
    before_counts = _counts()
    first = [p.detach().clone() for p in tr.models["shared"].parameters()]
    for it in range(3):
        tr._generate_rollout_batch()
        metrics = tr._update_model_params(it, True)
        assert np.isfinite(metrics["shared"]["Total loss"])
    assert not [s for s in _launched_since(before_counts) if s.startswith("HipPg")]
    assert all(not torch.equal(p, q) for p, q in zip(tr.models["shared"].parameters(), first))
    tr.graceful_close()


def test_another_string_is_refused(tmp_path):
    with pytest.raises(ValueError, match="fused_update"):
        _trainer(tmp_path, "cartpole", fused_update="everything")


def test_all_means_true_for_ddpg(tmp_path):
    from tests.test_gpu_ddpg_update import _trainer as ddpg_trainer

    tr = ddpg_trainer(tmp_path, "one launch", fused_update="all")
    assert tr.update_path == "kernels"
    packs = {"n": 0}
    real_pack = tr._batch_rollout["pack"]

    def counting_pack(model, out=None):
        packs["n"] += 1
        return real_pack(model, out=out)

    tr._batch_rollout["pack"] = counting_pack
    from warp_drive_amd.training.policy_kernel import pack_rollout_actor

    for it in range(3):
        tr._generate_rollout_batch()
        tr._update_model_params(it, False)
        torch.cuda.synchronize()
        assert _same_bytes(tr._batch_rollout["packed"]["shared"], pack_rollout_actor(tr.actors["shared"]))
    assert packs["n"] == 1                 # the repack is skipped after the Apply launch's refill here as well
    tr.graceful_close()


# Recorded on the MI355X with the PARENT commit's (48c5bcb) training/trainer.py in place of this tree's, in two processes, and
# on this tree: `_parameter_checksum` after three iterations of the three trainers below WITHOUT the key, same seeds.
DEFAULT_PATH_CHECKSUM = "a0fcd2903a1220510f4838ab4c0fd4585e7de52e8554af022bda8102ee66728e"


def _parameter_checksum(trainers):
    h = hashlib.sha256()
    for tr in trainers:
        for p in tr.models["shared"].parameters():
            h.update(p.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def default_path_run(tmp_path):
    """Cartpole, Acrobot and MountainCar WITHOUT `fused_update`, three iterations each at E = 64, T = 6 on the one-launch
    rollout -> ({policy: path} of each, the sha256 of the bytes of every parameter)"""
    trainers = [_trainer(os.path.join(str(tmp_path), env), env, fused_update=None) for env in ENVS]
    for tr in trainers:
        for it in range(3):
            tr._generate_rollout_batch()
            tr._update_model_params(it, it == 2)
    torch.cuda.synchronize()
    paths, checksum = [getattr(tr, "update_path", {"shared": "framework"}) for tr in trainers], _parameter_checksum(trainers)
    for tr in trainers:
        tr.graceful_close()
    return paths, checksum


def test_default_path_is_the_parent_commits(tmp_path):
    paths, checksum = default_path_run(tmp_path)
    print("default path checksum", checksum)
    assert all(p == {"shared": "framework"} for p in paths) and checksum == DEFAULT_PATH_CHECKSUM


# ------------------------------------------------------------------------------------------------------- learning
def test_acrobot_learns_with_the_update_kernels(tmp_path):
    """tests/test_gpu_classic_control_policy.py::test_acrobot_learns_on_the_one_launch_path's settings and its bar (first
    100 iterations below -180, last 100 above -150) with `fused_update: "all"` added: every update five launches.
    Measured on the MI355X, once: -197.4 -> -86.1 (docs/rounds/r19.md §6)."""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    ov = {"trainer": {"num_envs": 1000, "train_batch_size": 1000 * 50, "num_episodes": 10 ** 6, "seed": 7,
                      "fused_rollout_policy": "all", "fused_update": "all"},
          "env": {"episode_length": 200, "seed": 11}, "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0}}
    torch.manual_seed(0)
    tr = setup_trainer("single_acrobot", ov, results_dir=str(tmp_path), verbose=False)
    assert tr._batch_rollout is not None and tr.engine.step_kernel_name == "HipClassicControlAcrobotEnvRollout_H32"
    assert tr.update_path == {"shared": "kernels"}
    tr.train(1500)
    tr.graceful_close()
    curve = np.array([json.loads(line)["shared"]["Mean episodic reward"] for line in open(tmp_path / "results.json")])
    first, last = np.nanmean(curve[:100]), np.nanmean(curve[-100:])
    print(f"acrobot, one launch per batch, update kernels: mean episodic reward {first:.1f} -> {last:.1f}; every 100th: "
          + " ".join(f"{v:.0f}" for v in curve[::100]))
    assert first < -180 and last > -150
