"""The DDPG update kernels on the device (wd_kernels_ddpg.hsaco; cases, inputs and yardsticks: tests/ddpg_update_cases.py),
stage by stage from each stage's own inputs, then composed inside TrainerDDPG (`trainer.fused_update: true`).

Conventions (those of tests/test_gpu_update_kernel_entries.py):
  * an output lies inside an allocation filled with a sentinel NaN, with surplus rows / blocks, and everything outside the
    region the launch must write is compared byte for byte afterwards; the region itself starts as the sentinel too;
  * a float input is a view that ENDS inside a larger allocation that goes on with NaN;
  * every launch goes through the wrappers of training/ddpg_update_kernels.py and is counted in hip_driver.LAUNCH_COUNTS;
  * per result tensor err <= max(4 * err_f32, 2e-6 * scale): err against the float64 yardstick, err_f32 the error of the
    framework's float32 computation of the same quantity from the same inputs on the device, scale the largest float64
    magnitude; err / err_f32 is printed per tensor (pytest -s)."""
import copy
import hashlib

import numpy as np
import pytest
import torch

from tests import ddpg_update_cases as dc

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
DEV = torch.device("cuda:0")
STAGES = ("HipDdpgTargets", "HipDdpgGradients", "HipDdpgReduce", "HipDdpgApply")


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
    for case in dc.CASES:
        inp = dc.inputs(case)
        out[case.name] = (inp, dc.yardstick(case, inp))
    return out


def _kernels(fm, case):
    from warp_drive_amd.training.ddpg_update_kernels import DdpgUpdateKernels

    return DdpgUpdateKernels(fm, case.E, case.T, case.n_step, case.H, case.O, DEV)


def _counts():
    from warp_drive_amd.managers import hip_driver as drv

    return {k: v for k, v in drv.LAUNCH_COUNTS.items() if k.startswith("HipDdpg")}


def _launched_since(before):
    """{stage: launches} of the update kernels since `before`"""
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
    whole = torch.full((n + extra,), dc.SENTINEL_BITS, dtype=torch.int32, device=DEV)
    return whole, whole[:n].view(torch.float32).view(shape)


def _untouched(whole, view):
    return bool((whole[view.numel():] == dc.SENTINEL_BITS).all())


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _judge(tag, got, want, yard, keys, worst_only=False):
    ratios, failures = {}, []
    for k in keys:
        g = np.asarray(got[k], f64)
        assert np.isfinite(g).all(), (tag, k, "not finite")
        ok, err, err_f32, scale, ratio = dc.compare(g.reshape(-1), np.asarray(want[k], f64).reshape(-1),
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
    return {"obs": _fenced(inp["obs"].reshape(T, E, 1, O)), "actions": _fenced(inp["actions"].reshape(T, E, 1, 1)),
            "rewards": _fenced(inp["rewards"].reshape(T, E, 1)), "done": _fenced(inp["done"], torch.int32),
            "theta": _fenced(inp["theta"]), "target": _fenced(inp["target"])}


# ============================================================================================ 1. next values, returns
@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_next_values_and_returns(fm, references, case):
    """next values under the bound against float64 -- at the wrapper's geometry, and bit-identical at one block of 64
    threads (grid-stride trips) and with surplus blocks; the returns the gradient launch forms from them equal
    losses.DDPG.n_step_returns on the kernel's next values bit for bit"""
    from warp_drive_amd.training.losses import DDPG

    inp, want = references[case.name]
    k, d = _kernels(fm, case), _device_inputs(inp)
    T, E = case.T, case.E
    results = []
    rows1 = (T - 1) * E
    for block, grid in ((None, None), (64, 1), (128, -(-rows1 // 128) + 3)):
        whole, out = _sentinel((T - 1, E))
        before = _counts()
        k.targets(d["obs"], d["target"], case.scale, case.bias, out=out, block=block, grid=grid)
        torch.cuda.synchronize()
        assert _launched_since(before) == {"HipDdpgTargets": 1}
        assert _untouched(whole, out), (case.name, block, grid)
        results.append(out)
    assert _same_bytes(results[0], results[1]) and _same_bytes(results[0], results[2])
    yard = dc.framework(case, inp, torch.float32, DEV)
    _judge(f"next values {case.name}", {"next_values": results[0].cpu().numpy()}, want, yard, ["next_values"])

    whole_r, returns = _sentinel((k.V, E))
    whole_p, partials = _sentinel((dc.case_grid(case), k.PT + 2))
    before = _counts()
    k.gradients(d["obs"], d["actions"], d["rewards"], d["done"], results[0], d["theta"], case.gamma, case.scale, case.bias,
                returns_out=returns, partials=partials)
    torch.cuda.synchronize()
    assert _launched_since(before) == {"HipDdpgGradients": 1}
    assert _untouched(whole_r, returns) and _untouched(whole_p, partials)
    objective = DDPG(discount_factor_gamma=case.gamma, n_step=case.n_step)
    ref = objective.n_step_returns(d["rewards"], d["done"], results[0].reshape(T - 1, E, 1))
    assert _same_bytes(returns, ref.reshape(k.V, E)), case.name
    model = dc.returns_model(inp["rewards"], inp["done"], results[0].cpu().numpy(), case.n_step, case.gamma, f32)
    assert np.array_equal(dc.bits(returns.cpu().numpy()), dc.bits(model))
    for key in d:   # the inputs are as they were
        src = inp[key]
        assert np.array_equal(dc.bits(d[key].cpu().numpy().reshape(-1)), dc.bits(np.ascontiguousarray(src).reshape(-1))), key


# ============================================================================================ 2 + 3. gradients, reduce
@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_gradients_after_reduce(fm, references, case):
    """from the kernel's own next values: the twelve gradients and the two losses under the bound against float64, the
    per-tensor sums of squares against those of the kernel's own gradients; blocks without rows write zeros; nothing
    outside the written regions changes; a second run gives the same bytes"""
    from warp_drive_amd.training import ddpg_update_kernels as duk

    inp, _ = references[case.name]
    k, d = _kernels(fm, case), _device_inputs(inp)
    nv = k.targets(d["obs"], d["target"], case.scale, case.bias).clone()
    nv_host = nv.cpu().numpy()
    want = dc.yardstick(case, inp, next_values=nv_host)
    yard = dc.framework(case, inp, torch.float32, DEV, next_values=nv_host)
    grid = dc.case_grid(case)
    runs = []
    for _ in range(2):
        whole_r, returns = _sentinel((k.V, case.E))
        whole_p, partials = _sentinel((grid, k.PT + 2))
        whole_g, grads = _sentinel((k.PT,))
        whole_s, sumsq = _sentinel((12,))
        whole_l, losses = _sentinel((2,))
        before = _counts()
        k.gradients(d["obs"], d["actions"], d["rewards"], d["done"], nv, d["theta"], case.gamma, case.scale, case.bias,
                    returns_out=returns, partials=partials)
        k.reduce(partials=partials, grads=grads, sumsq=sumsq, losses=losses)
        torch.cuda.synchronize()
        assert _launched_since(before) == {"HipDdpgGradients": 1, "HipDdpgReduce": 1}
        for whole, view in ((whole_r, returns), (whole_p, partials), (whole_g, grads), (whole_s, sumsq), (whole_l, losses)):
            assert _untouched(whole, view), case.name
        runs.append((partials, grads, sumsq, losses))
    for a, b in zip(*runs):
        assert _same_bytes(a, b), case.name
    partials, grads, sumsq, losses = runs[0]
    assert bool(torch.isfinite(partials).all())
    if grid > k.tiles:
        assert not partials[k.tiles:].any(), "a block without rows writes zeros"
    got = {"critic_loss": losses[0].item(), "actor_loss": losses[1].item()}
    g_host = grads.cpu().numpy()
    bounds = dc.tensor_bounds(case.H, case.O)
    for name, (lo, hi) in zip(dc.TENSOR_NAMES, bounds):
        got[name] = g_host[lo:hi]
    _judge(f"gradients {case.name}", got, want, yard, dc.TENSOR_NAMES + ("critic_loss", "actor_loss"))
    ss_got = {n: sumsq[i].item() for i, n in enumerate(dc.TENSOR_NAMES)}
    ss_want = {n: float(np.sum(g_host[lo:hi].astype(f64) ** 2)) for n, (lo, hi) in zip(dc.TENSOR_NAMES, bounds)}
    ss_yard = {n: float((grads[lo:hi] * grads[lo:hi]).sum()) for n, (lo, hi) in zip(dc.TENSOR_NAMES, bounds)}
    _judge(f"sums of squares {case.name}", ss_got, ss_want, ss_yard, dc.TENSOR_NAMES)
    norms = k.gradient_norms(sumsq)
    for norm, nets in zip(norms, (dc.TENSOR_NAMES[:6], dc.TENSOR_NAMES[6:])):
        assert abs(norm - sum(np.sqrt(ss_want[n]) for n in nets)) <= 1e-5 * max(norm, 1e-30)
    assert duk.TILE == dc.TILE


# ===================================================================================================== 4. apply
@pytest.mark.parametrize("ac", dc.APPLY_CASES, ids=lambda a: a.name)
def test_apply(fm, ac):
    """clip (active / inactive / off) + Adam (steps 1, 2, 1000; two learning rates) + soft update from given float32
    gradients: parameters, both moments and targets under the bound per tensor; a gradient of exactly 0 on fresh moments
    leaves its parameter and moments as they were; the packed actor equals pack_rollout_actor of the updated actor byte
    for byte; nothing outside the four buffers and the packed actor changes"""
    from warp_drive_amd.training import ddpg_update_kernels as duk
    from warp_drive_amd.training.policy_kernel import pack_rollout_actor

    inp = dc.apply_inputs(ac)
    case = dc.Case("apply", 64, 2, 1, 0.99, ac.H, ac.O, 1.0, 0.0, "none", None, False, 0)
    k = _kernels(fm, case)
    state = {}
    for key in ("theta", "target", "exp_avg", "exp_avg_sq"):
        whole, view = _sentinel((k.PT,))
        view.copy_(torch.from_numpy(inp[key]))
        state[key] = (whole, view)
    grads = _fenced(inp["grads"])
    # the sums of squares from the reduce launch itself, on one "block" whose partial is the gradient
    partial = _fenced(np.concatenate([inp["grads"], np.zeros(2, f32)])[None])
    whole_s, sumsq = _sentinel((12,))
    scratch_g, scratch_l = torch.zeros(k.PT, device=DEV), torch.zeros(2, device=DEV)
    k.reduce(partials=partial, grads=scratch_g, sumsq=sumsq, losses=scratch_l)
    assert _same_bytes(scratch_g, grads)
    OP = (ac.O + 1) // 2 * 2
    whole_k, packed = _sentinel((duk.net_floats(ac.H, ac.O) + ac.H * (OP - ac.O),))
    packed.zero_()   # (the pad column is zero from the start: pack_rollout_actor's layout)
    before = _counts()
    k.apply(state["theta"][1], state["target"][1], state["exp_avg"][1], state["exp_avg_sq"][1], ac.step, ac.lr_actor,
            ac.lr_critic, ac.tau, max_norm=dc.apply_max_norm(ac), packed=packed, grads=grads, sumsq=sumsq)
    torch.cuda.synchronize()
    assert _launched_since(before) == {"HipDdpgApply": 1}
    for whole, view in list(state.values()) + [(whole_s, sumsq), (whole_k, packed)]:
        assert _untouched(whole, view), ac.name
    assert np.array_equal(dc.bits(grads.cpu().numpy()), dc.bits(inp["grads"]))
    want, yard = dc.apply_model(ac, inp), dc.framework_apply(ac, inp, torch.float32, DEV)
    got = {key: state[key][1].cpu().numpy() for key in state}
    flat = lambda res: {f"{key} {name}": np.asarray(res[key])[lo:hi] for key in state
                        for name, (lo, hi) in zip(dc.TENSOR_NAMES, dc.tensor_bounds(ac.H, ac.O))}
    for key in state:
        keys = [k for k in flat(want) if k.startswith(key + " ")]
        _judge(f"apply {ac.name} {key}", flat(got), flat(want), flat(yard), keys, worst_only=True)
    zero = slice(0, None, dc.ZERO_EVERY)   # gradient and both moments exactly 0 there, at every step of the cases
    for key in ("theta", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(dc.bits(got[key][zero]), dc.bits(inp[key][zero])), key
    assert not np.array_equal(got["theta"], inp["theta"])
    actor, _ = dc.build_modules(case, got["theta"], torch.float32, DEV)
    assert _same_bytes(packed, pack_rollout_actor(actor)), ac.name


# ============================================================================================== inside the trainer
def _trainer(tmp_path, path="one launch", env="pendulum", E=64, T=6, n_step=3, fc=(64, 64), seed=3, log_freq=1,
             fused_update=True, policy_extra=None, env_cfg=None, lr=(0.001, 0.0005)):
    from tests import classic_control_cases as cc
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    net = {"type": "fully_connected", "fc_dims": list(fc), "model_ckpt_filepath": ""}
    policy = {"to_train": True, "algorithm": "DDPG", "clip_grad_norm": True, "max_grad_norm": 3, "gamma": 0.99, "tau": 0.05,
              "lr": {"actor": lr[0], "critic": lr[1]}, "model": {"actor": dict(net), "critic": dict(net)}}
    policy.update(policy_extra or {})
    trainer = {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": seed, "n_step": n_step,
               "fused_rollout_policy": "all" if path == "one launch" else False}
    if fused_update is not None:
        trainer["fused_update"] = fused_update
    ov = {"trainer": trainer, "policy": {"shared": policy},
          "sampler": {"params": {"damping": 0.15, "stddev": 0.2, "scale": 1.0}},
          "saving": {"metrics_log_freq": log_freq, "model_params_save_freq": 0},
          "env": env_cfg or {"episode_length": 4, "reset_pool_size": 0, "seed": cc.ENV_SEED}}
    torch.manual_seed(seed)
    return setup_trainer(f"single_{env}", ov, results_dir=str(tmp_path), verbose=False)


def _all_parameters(tr, pol="shared"):
    return [p for net in tr._networks(pol).values() for p in net.parameters()]


@pytest.mark.parametrize("env", ["pendulum", "continuous_mountain_car"])
@pytest.mark.parametrize("path", ["per tick", "one launch"])
def test_composed_in_the_trainer(env, path, tmp_path):
    """three iterations at E = 64, T = 6, n_step 3 with `fused_update: true` on both rollout paths: `_update_model_params`
    is the four launches and nothing else of the update object; its results are byte-identical to launching the stages
    directly on a snapshot of the same state, twice; a logging iteration returns the framework path's keys, finite;
    checkpoints round-trip all four networks and load into a framework-path trainer"""
    from warp_drive_amd.training import ddpg_update_kernels as duk
    from warp_drive_amd.training.policy_kernel import pack_rollout_actor

    pol = "shared"
    tr = _trainer(tmp_path / "k", path, env)
    ref = _trainer(tmp_path / "f", path, env, fused_update=None)
    assert tr.update_path == "kernels" and ref.update_path == "framework" and tr.rollout_path == ref.rollout_path == path
    k = tr._update_kernels
    direct = duk.DdpgUpdateKernels(tr.w.cuda_function_manager, 64, 6, 3, 64, k.O, DEV)
    for it in range(3):
        log = it == 1
        tr._generate_rollout_batch()
        ref._generate_rollout_batch()
        torch.cuda.synchronize()
        snap = {"theta": tr._flat.flat.clone(), "target": tr._flat_target.flat.clone(),
                "m": tr._adam["exp_avg"].clone(), "v": tr._adam["exp_avg_sq"].clone(), "step": tr._adam["step"]}
        before = _counts()
        metrics = tr._update_model_params(it, log)
        torch.cuda.synchronize()
        assert _launched_since(before) == {s: 1 for s in STAGES}, (it, _launched_since(before))
        ref_metrics = ref._update_model_params(it, log)
        if log:
            assert set(metrics[pol]) == set(ref_metrics[pol])
            bad = {key: v for key, v in metrics[pol].items() if not np.isfinite(v) and "over agents" not in key}
            assert not bad, bad
            assert metrics[pol]["Gradient norm (Actor)"] > 0 and metrics[pol]["Gradient norm (Critic)"] > 0
        else:
            assert metrics == {}
        assert tr._adam["step"] == snap["step"] + 1 and tr.current_timestep[pol] == (it + 1) * 64 * 6
        b = tr.batch[pol]
        scale, bias = tr._actor_range
        for _ in range(2):
            st = {key: v.clone() for key, v in snap.items() if key != "step"}
            packed = torch.zeros_like(pack_rollout_actor(tr.actors[pol]))
            direct.targets(b["obs"][:6], st["target"], scale, bias)
            direct.gradients(b["obs"][:6], b["actions"][:6], b["rewards"][:6], tr.done_batch[:6], direct.next_values,
                             st["theta"], 0.99, scale, bias)
            direct.reduce()
            direct.apply(st["theta"], st["target"], st["m"], st["v"], snap["step"] + 1, 0.001, 0.0005, 0.05, max_norm=3,
                         packed=packed)
            torch.cuda.synchronize()
            assert _same_bytes(st["theta"], tr._flat.flat) and _same_bytes(st["target"], tr._flat_target.flat), it
            assert _same_bytes(st["m"], tr._adam["exp_avg"]) and _same_bytes(st["v"], tr._adam["exp_avg_sq"]), it
            assert _same_bytes(packed, pack_rollout_actor(tr.actors[pol]))
            if path == "one launch":
                assert _same_bytes(tr._batch_rollout["packed"][pol], packed)
        assert not _same_bytes(snap["theta"], tr._flat.flat) and tr._flat.bound() and tr._flat_target.bound()
    # the modules are the source of truth: state_dict, save, load, and a framework-path trainer loads the files
    paths = tr.save_model_checkpoint()
    saved = {name: copy.deepcopy(net.state_dict()) for name, net in tr._networks(pol).items()}
    with torch.no_grad():
        for p in _all_parameters(tr):
            p.add_(1.0)
    tr.current_timestep[pol] = 0
    tr.load_model_checkpoint(paths)
    assert tr.current_timestep[pol] == 3 * 64 * 6 and tr._flat.bound() and tr._flat_target.bound()
    ref.load_model_checkpoint(paths)
    for name in saved:
        for key, v in saved[name].items():
            assert torch.equal(tr._networks(pol)[name].state_dict()[key], v), (name, key)
            assert torch.equal(ref._networks(pol)[name].state_dict()[key], v), (name, key)
    # a load without the targets' files: the hard copy
    tr.load_model_checkpoint({pol: {"actor": paths[pol]["actor"], "critic": paths[pol]["critic"]}})
    for t, p in zip(tr.target_actors[pol].parameters(), tr.actors[pol].parameters()):
        assert torch.equal(t, p)
    assert _same_bytes(tr._flat.flat, tr._flat_target.flat)
    tr._generate_rollout_batch()
    tr._update_model_params(3, False)    # ... and the update goes on from the loaded state
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tr._flat.flat).all())
    for t in (tr, ref):
        t.graceful_close()


@pytest.mark.parametrize("change,why", [({"fc": (48, 48)}, "hidden width 48"),
                                        ({"fc": (64, 32)}, "unequal widths"),
                                        ({"fc": (32, 32, 32)}, "3 hidden layers"),
                                        ({"policy_extra": {"normalize_return": True}}, "normalize_return")])
def test_refused_shapes_train_on_the_framework_path(change, why, tmp_path, caplog):
    import logging

    with caplog.at_level(logging.INFO):
        tr = _trainer(tmp_path, "per tick", **change)
    assert tr.update_path == "framework" and tr._update_kernels is None
    assert any(why in r.getMessage() and "framework path" in r.getMessage() for r in caplog.records)
    before_counts = _counts()
    first = [p.detach().clone() for p in _all_parameters(tr)]
    for it in range(3):
        tr._generate_rollout_batch()
        metrics = tr._update_model_params(it, True)
        assert np.isfinite(metrics["shared"]["Total loss"])
    assert _launched_since(before_counts) == {}
    assert all(not torch.equal(p, q) for p, q in zip(_all_parameters(tr), first))
    tr.graceful_close()


# Recorded on the MI355X with the PARENT commit's (7a7b8ef) trainer_ddpg.py and build.py in place of this tree's -- the only
# files of the parent that this change touches; the commit before `trainer.fused_update` existed for DDPG: `_parameter_checksum` after three iterations of the trainer below, same seeds.
DEFAULT_PATH_CHECKSUM = "f6dddfd87a3fdcdde01cc0989714c64f0829e34e188b9e6df27a13d88369b09f"


def _parameter_checksum(tr):
    h = hashlib.sha256()
    for p in _all_parameters(tr):
        h.update(p.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def default_path_run(tmp_path):
    """a trainer WITHOUT the key, three iterations on the one-launch rollout -> the sha256 of the bytes of every
    parameter of the four networks"""
    tr = _trainer(tmp_path, "one launch", fused_update=None)
    for it in range(3):
        tr._generate_rollout_batch()
        tr._update_model_params(it, it == 2)
    torch.cuda.synchronize()
    path, checksum = getattr(tr, "update_path", "framework"), _parameter_checksum(tr)
    tr.graceful_close()
    return path, checksum


def test_default_path_is_the_parent_commits(tmp_path):
    path, checksum = default_path_run(tmp_path)
    print("default path checksum", checksum)
    assert path == "framework" and checksum == DEFAULT_PATH_CHECKSUM


# ------------------------------------------------------------------------------------------------------- learning
# Seeds 0, 1 and 2 at 1000, 2000 and 4000 iterations, once, on the MI355X (docs/rounds/r18.md, profiles/r18_pendulum_ddpg_fused.txt):
#   1000: +42.6, -39.9, +19.3 standard errors;  2000: +124.1, +9.7, +61.1;  4000: +35.5, +30.0, +124.4.
# The smallest count at which all three seeds exceed 5 standard errors is 2000 (1.75 s of training per seed).
LEARNING_ITERATIONS = 2000
LEARNING_SEED = 0


def pendulum_fused_learning_run(seed, iterations, tmp_path):
    """tests/test_gpu_classic_control_actor.py::pendulum_learning_run's shape -- Pendulum, E = 1000, T = 5, n_step 5, lr 1e-3
    for both [64, 64] networks, the one-launch rollout -- with the update on the kernels: greedy per-replica returns
    before and after `iterations` training iterations, and the seconds the training took"""
    import time

    tr = _trainer(tmp_path, "one launch", "pendulum", E=1000, T=5, n_step=5, fc=(64, 64), seed=seed, log_freq=100,
                  env_cfg={"seed": seed}, lr=(0.001, 0.001))
    assert tr.rollout_path == "one launch" and tr.update_path == "kernels" and (tr.batch_len, tr.n_step) == (5, 5)
    before = tr.evaluate_episodes(use_argmax=True)[0]["shared"].reshape(-1).astype(np.float64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.train(iterations)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    after = tr.evaluate_episodes(use_argmax=True)[0]["shared"].reshape(-1).astype(np.float64)
    tr.graceful_close()
    return before, after, seconds


def test_pendulum_learns_with_the_update_kernels(tmp_path):
    """tests/test_gpu_classic_control_actor.py's criterion: the greedy policy's mean episodic reward rises by more than 5
    standard errors of the difference.  Measured on the MI355X, seed 0, 2000 iterations: -1367.2 -> -369.4, +124.1
    standard errors, 1.75 s of training."""
    from tests.test_gpu_classic_control_actor import standard_errors_of_the_gain

    before, after, seconds = pendulum_fused_learning_run(LEARNING_SEED, LEARNING_ITERATIONS, tmp_path)
    gain = standard_errors_of_the_gain(before, after)
    print(f"pendulum DDPG, update kernels, seed {LEARNING_SEED}: greedy mean episodic reward {before.mean():.1f} -> "
          f"{after.mean():.1f} after {LEARNING_ITERATIONS} iterations ({seconds:.2f} s), {gain:.1f} standard errors")
    assert len(before) == len(after) == 1000 and np.isfinite(before).all() and np.isfinite(after).all()
    assert gain > 5.0, (before.mean(), after.mean(), gain)
