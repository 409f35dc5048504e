"""The update kernels of a custom environment on the device (include/wd_env_update.h; cases and inputs:
tests/pg_update_custom_cases.py, yardstick: tests/pg_update_cases.py), stage by stage from each stage's own inputs -- on the
entries of examples/rendezvous_update/ (F = 5) and of the probes of tests/custom_envs/ (F = 1, 7) -- then composed inside
Trainer on RendezvousUpdate (`fused_rollout_policy: "all"` + `fused_update: "all"`).

Conventions: those of tests/test_gpu_pg_update.py (sentinel-filled outputs with surplus rows, NaN-fenced inputs, every
launch through the wrappers and counted in hip_driver.LAUNCH_COUNTS, per result tensor
err <= max(4 * err_f32, 2e-6 * scale), err / err_f32 printed per tensor under pytest -s).  Every device source is compiled
once per module, on its first use."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import pg_update_cases as pc
from tests import pg_update_custom_cases as cc
from tests.test_gpu_pg_update import DEV, _fenced, _judge, _same_bytes, _sentinel, _untouched

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module", autouse=True)
def env_cache(tmp_path_factory):
    """one cache directory for the module: each unit compiles once, every later user finds it"""
    path = str(tmp_path_factory.mktemp("env_cache"))
    saved = os.environ.get("WD_ENV_CACHE")
    os.environ["WD_ENV_CACHE"] = path
    yield path
    if saved is None:
        os.environ.pop("WD_ENV_CACHE", None)
    else:
        os.environ["WD_ENV_CACHE"] = saved


_MANAGERS = {}


@pytest.fixture(scope="module")
def managers(env_cache):
    """F -> a function manager whose custom code object has the update entries for F observation floats"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd import build as wd_build
    from warp_drive_amd.managers.function_manager import HIPFunctionManager

    require_gpu()
    _MANAGERS.clear()

    def get(F):
        if F not in _MANAGERS:
            unit, source, _ = cc.unit_of(F)
            fm = HIPFunctionManager(num_agents=1, num_envs=1)
            fm.load_hip_from_binary_file()
            fm.load_custom_hip_from_binary_file(wd_build.build_env_unit(unit, source), source)
            _MANAGERS[F] = fm
        return _MANAGERS[F]

    return get


@pytest.fixture(scope="module")
def references():
    """per case: the inputs and the float64 yardstick from them (computed once, never changed)"""
    out = {}
    for case in cc.CASES:
        inp = cc.inputs(case)
        out[case.name] = (inp, cc.yardstick(case, inp))
    return out


def _kernels(managers, H, F, A, E=16, T=2, n=4):
    from warp_drive_amd.training.pg_update_custom_kernels import PgCustomUpdateKernels

    return PgCustomUpdateKernels(managers(F), cc.unit_of(F)[2], E, T, n, H, F, A, DEV)


def _case_kernels(managers, case):
    return _kernels(managers, case.H, case.F, case.A, case.E, case.T, case.n)


def _counts():
    from warp_drive_amd.managers import hip_driver as drv

    return {k: v for k, v in drv.LAUNCH_COUNTS.items() if "Pg" in k or k == "HipDiscountedReturns"}


def _launched_since(before):
    """{stage without its prefix and width: launches} of the update's kernels since `before`"""
    out = {}
    for name, n in _counts().items():
        d = n - before.get(name, 0)
        if d:
            stage = name.split("_H")[0]
            stage = stage[stage.index("Pg"):] if "Pg" in stage else stage
            out[stage] = out.get(stage, 0) + d
    return out


FIVE = {"PgValues": 1, "HipDiscountedReturns": 1, "PgGradients": 1, "PgReduce": 1, "PgApply": 1}


def _device_inputs(case, inp):
    T, E, n, F = case.T, case.E, case.n, case.F
    return {"obs": _fenced(inp["obs"].reshape(T, E, n, F)), "actions": _fenced(inp["actions"].reshape(T, E, n, 1), torch.int32),
            "rewards": _fenced(inp["rewards"].reshape(T, E, n)), "done_env": _fenced(inp["done_env"], torch.int32),
            "theta": _fenced(inp["theta"])}


def _inputs_as_they_were(d, inp):
    for key in d:
        assert np.array_equal(pc.bits(d[key].cpu().numpy().reshape(-1)), pc.bits(np.ascontiguousarray(inp[key]).reshape(-1))), key


# ================================================================================================ 1 + 2. values, returns
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_values_and_returns(managers, references, case):
    """values under the bound against float64 -- at the wrapper's geometry, and bit-identical at one block of 64 threads
    (grid-stride trips) and with surplus blocks; the returns the existing entry forms from them with n agents per replica
    equal the float32 returns model and losses.discounted_returns bit for bit, the advantages are returns - values"""
    from warp_drive_amd.training.losses import discounted_returns

    inp, want = references[case.name]
    k, d = _case_kernels(managers, case), _device_inputs(case, inp)
    T, E, n = case.T, case.E, case.n
    results = []
    for block, grid in ((None, None), (64, 1), (128, -(-T * E * n // 128) + 3)):
        whole, out = _sentinel((T, E, n))
        before = _counts()
        k.compute_values(d["obs"], d["theta"], out=out, block=block, grid=grid)
        torch.cuda.synchronize()
        assert _launched_since(before) == {"PgValues": 1}
        assert _untouched(whole, out), (case.name, block, grid)
        results.append(out)
    assert _same_bytes(results[0], results[1]) and _same_bytes(results[0], results[2])
    yard = cc.framework(case, inp, torch.float32, DEV)
    _judge(f"values {case.name}", {"values": results[0].cpu().numpy().reshape(T, E * n)}, want, yard, ["values"])

    whole_r, returns = _sentinel((T, E, n))
    whole_a, adv = _sentinel((T, E, n))
    before = _counts()
    k.discounted_returns(d["rewards"], d["done_env"], case.gamma, values=results[0], returns=returns, advantages=adv)
    torch.cuda.synchronize()
    assert _launched_since(before) == {"HipDiscountedReturns": 1}
    assert _untouched(whole_r, returns) and _untouched(whole_a, adv)
    v_host = results[0].cpu().numpy()
    model = cc.returns_model_n(inp["rewards"].reshape(T, E, n), inp["done_env"], v_host, case.gamma, f32)
    assert np.array_equal(pc.bits(returns.cpu().numpy()), pc.bits(model)), case.name
    ref = discounted_returns(d["rewards"], d["done_env"], results[0], case.gamma)
    assert _same_bytes(returns, ref) and _same_bytes(adv, ref - results[0]), case.name
    _inputs_as_they_were(d, inp)


# ============================================================================================ 3 + 4. gradients, reduce
@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.name)
def test_gradients_and_reduce(managers, references, case):
    """gradients, from the kernel's own values, returns and advantages: the per-block partials summed in block order in
    float64 -- the eight tensors and the four sums -- under the bound against the yardstick; blocks without rows write zeros.
    reduce, from the partials it was given: the flat gradient, the four sums and the per-tensor sums of squares under the
    bound against their float64 sums.  Nothing outside the written regions changes; a second run gives the same bytes."""
    inp, _ = references[case.name]
    k, d = _case_kernels(managers, case), _device_inputs(case, inp)
    T, E, n, H, F, A = case.T, case.E, case.n, case.H, case.F, case.A
    values = k.compute_values(d["obs"], d["theta"]).clone()
    returns, adv = k.discounted_returns(d["rewards"], d["done_env"], case.gamma, values=values)
    returns, adv = returns.clone(), adv.clone()
    v_host = values.cpu().numpy().reshape(T, E * n)
    want = cc.yardstick(case, inp, values=v_host)
    yard = cc.framework(case, inp, torch.float32, DEV, values=v_host)
    grid = cc.case_grid(case)
    P = k.P
    assert P == pc.net_floats(H, F, A)
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
        assert _launched_since(before) == {"PgGradients": 1, "PgReduce": 1}
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
    bounds = pc.tensor_bounds(H, F, A)
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


@pytest.mark.parametrize("F", [5, 7])
def test_an_entry_launched_with_a_bad_width_or_action_count_touches_nothing(managers, F):
    """Values and Gradients (both widths) with A = 0 and 9, Reduce and Apply with H = 48 / 0 and with A = 0 / 9: every
    output keeps the sentinel"""
    for H in (32, 64):
        k = _kernels(managers, H, F, 5)
        P, rows = k.P, k.rows
        obs, theta = torch.zeros((rows, F), device=DEV), torch.zeros(P, device=DEV)
        actions, flat = torch.zeros(rows, dtype=torch.int32, device=DEV), torch.zeros(rows, device=DEV)
        for bad_a in (0, 9, -1):
            whole_v, values = _sentinel((rows,))
            whole_p, partials = _sentinel((1, P + 4))
            k.fn_values(obs, theta, np.int64(rows), np.int32(bad_a), values, block=(64, 1, 1), grid=(1, 1), shared=k.values_lds)
            k.fn_gradients(obs, actions, flat, flat, theta, np.int64(rows), np.int32(bad_a), f32(1.0 / rows), f32(0.0), f32(1.0),
                           partials, block=(128, 1, 1), grid=(1, 1), shared=k.gradients_lds)
            torch.cuda.synchronize()
            assert bool((whole_v == pc.SENTINEL_BITS).all()) and bool((whole_p == pc.SENTINEL_BITS).all()), (H, bad_a)
        for h, a in ((48, 5), (0, 5), (H, 0), (H, 9)):
            whole_g, grads = _sentinel((P,))
            whole_s, sumsq = _sentinel((8,))
            whole_l, sums = _sentinel((4,))
            whole_k, packed = _sentinel((k.packed_floats,))
            state = [_sentinel((P,)) for _ in range(3)]
            partials, g_in, ss_in = torch.zeros((2, P + 4), device=DEV), torch.zeros(P, device=DEV), torch.ones(8, device=DEV)
            k.fn_reduce(partials, np.int32(2), np.int32(h), np.int32(a), grads, sumsq, sums, block=(1024, 1, 1), grid=(9, 1),
                        shared=0)
            k.fn_apply(state[0][1], state[1][1], state[2][1], g_in, ss_in, packed, np.int32(h), np.int32(a), f32(0.0),
                       f32(1e-3), f32(1.0), f32(0.1), f32(0.999), f32(0.001), f32(1e-8), block=(256, 1, 1),
                       grid=(k.apply_grid, 1), shared=0)
            torch.cuda.synchronize()
            for whole in [whole_g, whole_s, whole_l, whole_k] + [w for w, _ in state]:
                assert bool((whole == pc.SENTINEL_BITS).all()), (H, h, a)


# ===================================================================================================== 5. apply
@pytest.mark.parametrize("ac", cc.APPLY_CASES, ids=lambda a: a.name)
def test_apply_and_refill(managers, ac):
    """tests/pg_update_cases.py::APPLY_CASES' kinds of input -- clip active / inactive / off, Adam steps 1, 2, 1000 -- at the
    new shapes: parameters and both moments under the bound per tensor; a gradient of exactly 0 on fresh moments leaves its
    parameter and moments as they were; the packed tensor, PRE-FILLED WITH THE SENTINEL, equals the first P - H - 1 floats
    of the updated flat parameters bit for bit, which is pack_rollout_policy of the updated module; nothing else changes"""
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    H, F, A = ac.H, ac.O, ac.A
    inp = pc.apply_inputs(ac)
    k = _kernels(managers, H, F, A)
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
    assert k.packed_floats == k.P - H - 1
    whole_k, packed = _sentinel((k.packed_floats,))
    before = _counts()
    k.apply(state["theta"][1], state["exp_avg"][1], state["exp_avg_sq"][1], ac.step, ac.lr, max_norm=pc.apply_max_norm(ac),
            packed=packed, grads=grads, sumsq=sumsq)
    torch.cuda.synchronize()
    assert _launched_since(before) == {"PgApply": 1}
    for whole, view in list(state.values()) + [(whole_s, sumsq), (whole_k, packed)]:
        assert _untouched(whole, view), ac.name
    assert np.array_equal(pc.bits(grads.cpu().numpy()), pc.bits(inp["grads"]))
    want, yard = pc.apply_model(ac, inp), pc.framework_apply(ac, inp, torch.float32, DEV)
    got = {key: state[key][1].cpu().numpy() for key in state}
    flat = lambda res: {f"{key} {name}": np.asarray(res[key])[lo:hi] for key in state   # noqa: E731
                        for name, (lo, hi) in zip(pc.TENSOR_NAMES, pc.tensor_bounds(H, F, A))}
    for key in state:
        keys = [name for name in flat(want) if name.startswith(key + " ")]
        _judge(f"apply {ac.name} {key}", flat(got), flat(want), flat(yard), keys, worst_only=True)
    zero = slice(0, None, pc.ZERO_EVERY)   # gradient and both moments exactly 0 there, at every step of the cases
    for key in ("theta", "exp_avg", "exp_avg_sq"):
        assert np.array_equal(pc.bits(got[key][zero]), pc.bits(inp[key][zero])), key
    assert not np.array_equal(got["theta"], inp["theta"])
    assert np.array_equal(pc.bits(packed.cpu().numpy()), pc.bits(got["theta"][:k.P - H - 1])), ac.name
    model = pc.build_module(H, F, A, got["theta"], torch.float32, DEV)
    assert _same_bytes(packed, pack_rollout_policy(model).reshape(-1)), ac.name
    # ... and without a packed policy the launch updates the parameters alone
    again = {key: torch.from_numpy(inp[key]).to(DEV) for key in state}
    k.apply(again["theta"], again["exp_avg"], again["exp_avg_sq"], ac.step, ac.lr, max_norm=pc.apply_max_norm(ac),
            packed=None, grads=grads, sumsq=sumsq)
    torch.cuda.synchronize()
    assert all(_same_bytes(again[key], state[key][1]) for key in state)


# ============================================================================================== inside the trainer
E_, N_, T_ = 6, 5, 8   # 240 rows per batch: two tiles, the boundary inside a batch row


def _example(policy=False):
    """the class and source of examples/rendezvous_update/ (or of examples/rendezvous_policy/: the rollout mixin alone)"""
    if policy:
        from tests import custom_rollout_model as model

        return model.policy_module().RendezvousPolicy, model.POLICY_SOURCE
    from tests.test_custom_env_update_build import _example_class

    return _example_class(), cc.EXAMPLE_SOURCE


def _trainer(tmp_path, fc=(32, 32), fused_update="all", rollout="all", algo="A2C", policy=False, extra=None, log_freq=1):
    from tests.hip_harness import require_gpu
    from tests.rendezvous_helpers import registrar_for
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.training.trainer import Trainer

    require_gpu()
    cls, source = _example(policy)
    w = EnvWrapper(env_name=cls.name, env_config=dict(num_agents=N_, grid_length=6, episode_length=5, seed=9), num_envs=E_,
                   env_backend="hip", env_registrar=registrar_for(cls, source))
    trainer_config = {"num_envs": E_, "train_batch_size": E_ * T_, "num_episodes": 10 ** 6, "seed": 5}
    if rollout is not None:
        trainer_config["fused_rollout_policy"] = rollout
    if fused_update is not None:
        trainer_config["fused_update"] = fused_update
    pcfg = {"to_train": True, "algorithm": algo, "lr": 0.01, "vf_loss_coeff": 1, "entropy_coeff": 0.05, "gamma": 0.98,
            "clip_grad_norm": True, "max_grad_norm": 3, "normalize_advantage": False, "normalize_return": False,
            "model": {"type": "fully_connected", "fc_dims": list(fc), "model_ckpt_filepath": ""}}
    if algo == "PPO":
        pcfg["clip_param"] = 0.1
    pcfg.update(extra or {})
    config = {"name": "rendezvous_update", "trainer": trainer_config, "policy": {"shared": pcfg},
              "saving": {"metrics_log_freq": log_freq, "model_params_save_freq": 0, "basedir": str(tmp_path),
                         "name": "rendezvous_update", "tag": "test"}}
    torch.manual_seed(3)
    return Trainer(env_wrapper=w, config=config, policy_tag_to_agent_id_map={"shared": list(range(N_))},
                   results_dir=str(tmp_path), verbose=False)


def _said(caplog):
    return [r.getMessage() for r in caplog.records if "trainer.fused_update" in r.getMessage()]


@pytest.mark.parametrize("fc,algo", [((32, 32), "A2C"), ((64, 64), "PPO")])
def test_composed_in_the_trainer(fc, algo, tmp_path):
    """RendezvousUpdate with both keys: the rollout is one launch and the update five; ONE iteration's parameters, against
    a framework-path trainer (`fused_update` unset: the parent commit's path) loaded from the same state dict and given the
    same batch, are under the bound per tensor -- err against a float64 restatement of the iteration (the yardstick's
    gradient, clip and Adam in float64), err_f32 the framework-path trainer's error against the same; the update's bytes
    are those of the stages launched directly; the packed policy is the flat prefix; a checkpoint goes to the framework-path
    trainer and back"""
    from warp_drive_amd.training import pg_update_custom_kernels as pgck
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    H = fc[0]
    tr = _trainer(tmp_path / "k", fc=fc, algo=algo)
    ref = _trainer(tmp_path / "f", fc=fc, algo=algo, fused_update=None)
    pol = "shared"
    assert tr.update_path == {pol: "kernels"} and tr.rollout_path == "one launch"
    assert ref.update_path == {pol: "framework"} and ref.rollout_path == "one launch"
    assert tr.engine.entry_names == [f"HipRendezvousUpdateRollout_H{H}"]
    k = tr._pg_kernels[pol]
    assert isinstance(k, pgck.PgCustomUpdateKernels) and (k.E, k.T, k.n, k.H, k.O, k.A) == (E_, T_, N_, H, 5, 5)
    assert k.names == pgck.kernel_names("HipRendezvousUpdatePg", H) and k.blocks_per_cu == pgck.default_blocks_per_cu(H, 5)
    # the same state dict, the same batch
    ref.models[pol].load_state_dict(copy.deepcopy(tr.models[pol].state_dict()))
    tr._generate_rollout_batch()
    torch.cuda.synchronize()
    for key in ("obs", "actions", "rewards"):
        ref.batch[pol][key].copy_(tr.batch[pol][key])
    ref.done_batch.copy_(tr.done_batch)
    flat, adam, objective, pcfg = tr._pg_flat[pol], tr._pg_adam[pol], tr.trainers[pol], tr.config["policy"][pol]
    theta0 = flat.flat.clone()
    assert _same_bytes(tr._batch_rollout["packed"][pol].reshape(-1), theta0[:k.P - H - 1])
    b = tr.batch[pol]
    obs, actions, rewards, done = b["obs"][:T_], b["actions"][:T_], b["rewards"][:T_], tr.done_batch[:T_]
    assert obs.shape == (T_, E_, N_, 5) and actions.dtype == torch.int32 and done.shape == (T_, E_)
    ent_c = objective.entropy_coeff_schedule.get_param_value(0)
    vf_c = objective.vf_loss_coeff_schedule.get_param_value(0)
    # ---- the float64 restatement of this iteration, from the recorded batch
    case = cc.CuCase("trainer", E_, T_, N_, pcfg["gamma"], H, 5, 5, ent_c, vf_c, algo, "recorded", None, False, 0)
    done_env = done.cpu().numpy()
    inp = {"obs": obs.cpu().numpy().reshape(T_, E_ * N_, 5), "actions": actions.cpu().numpy().reshape(T_, E_ * N_),
           "rewards": rewards.cpu().numpy().reshape(T_, E_ * N_), "done": np.repeat(done_env, N_, axis=1),
           "done_env": done_env, "theta": theta0.cpu().numpy()}
    assert done_env.any() and not done_env.all()       # episodes of 5 ticks in a batch of 8: the flags matter
    grad64 = pc.flat_gradient(cc.yardstick(case, inp))
    step = pc.ApplyCase("trainer", H, 5, 5, 1, "active", float(pcfg["max_grad_norm"]), pcfg["lr"], 0)
    zeros = np.zeros(k.P, f64)
    want = pc.apply_model(step, {"grads": grad64, "theta": inp["theta"], "exp_avg": zeros, "exp_avg_sq": zeros})["theta"]
    # ---- the update, and the same stages launched directly on a snapshot
    before = _counts()
    metrics = tr._update_model_params(0, True)
    torch.cuda.synchronize()
    assert _launched_since(before) == FIVE
    ref_metrics = ref._update_model_params(0, True)
    torch.cuda.synchronize()
    assert set(metrics[pol]) == set(ref_metrics[pol])
    for key in ("Mean rewards", "Value function loss", "Mean entropy", "Policy loss", "Total loss"):
        assert np.isfinite(metrics[pol][key]), key
        assert abs(metrics[pol][key] - ref_metrics[pol][key]) <= 1e-4 * max(1.0, abs(ref_metrics[pol][key])), key
    dk = pgck.PgCustomUpdateKernels(tr.w.cuda_function_manager, "HipRendezvousUpdatePg", E_, T_, N_, H, 5, 5, DEV)
    st = {"theta": theta0.clone(), "m": torch.zeros_like(theta0), "v": torch.zeros_like(theta0)}
    whole_k, packed = _sentinel((k.packed_floats,))
    dk.compute_values(obs, st["theta"])
    dk.discounted_returns(rewards, done, pcfg["gamma"])
    dk.gradients(obs, actions, st["theta"], ent_c, vf_c)
    dk.reduce()
    dk.apply(st["theta"], st["m"], st["v"], 1, pcfg["lr"], max_norm=pcfg["max_grad_norm"], packed=packed)
    torch.cuda.synchronize()
    assert _same_bytes(st["theta"], flat.flat) and _same_bytes(st["m"], adam["exp_avg"]) and _same_bytes(st["v"], adam["exp_avg_sq"])
    assert _untouched(whole_k, packed) and _same_bytes(packed, tr._batch_rollout["packed"][pol].reshape(-1))
    assert _same_bytes(packed, flat.flat[:k.P - H - 1]) and _same_bytes(packed, pack_rollout_policy(tr.models[pol]).reshape(-1))
    assert adam["step"] == 1 and flat.bound() and not _same_bytes(theta0, flat.flat)
    # ---- under the bound, per tensor
    got = flat.flat.cpu().numpy()
    yard = np.concatenate([p.detach().cpu().numpy().reshape(-1) for p in pc.module_parameters(ref.models[pol])])
    bounds = pc.tensor_bounds(H, 5, 5)
    split = lambda a: {name: np.asarray(a)[lo:hi] for name, (lo, hi) in zip(pc.TENSOR_NAMES, bounds)}   # noqa: E731
    _judge(f"one iteration H{H} {algo}", split(got), split(want), split(yard), pc.TENSOR_NAMES)
    # ---- a checkpoint goes to the framework-path trainer and back
    tr.save_model_checkpoint()
    path = os.path.join(tr.save_dir, f"{pol}_{tr.current_timestep[pol]}.state_dict")
    saved = copy.deepcopy(tr.models[pol].state_dict())
    ref.load_model_checkpoint({pol: path})
    for key, v in saved.items():
        assert torch.equal(ref.models[pol].state_dict()[key], v), key
    ref._generate_rollout_batch()
    ref._update_model_params(1, False)
    ref.current_timestep[pol] = 777
    ref.save_model_checkpoint()
    tr.load_model_checkpoint({pol: os.path.join(ref.save_dir, f"{pol}_777.state_dict")})
    assert tr.current_timestep[pol] == 777 and flat.bound()
    for key, v in ref.models[pol].state_dict().items():
        assert torch.equal(tr.models[pol].state_dict()[key], v), key
    tr._generate_rollout_batch()          # a framework-side change: the rollout repacks, with the loaded weights
    assert _same_bytes(tr._batch_rollout["packed"][pol].reshape(-1), pack_rollout_policy(tr.models[pol]).reshape(-1))
    tr._update_model_params(1, False)     # ... and the update goes on from the loaded state
    torch.cuda.synchronize()
    assert bool(torch.isfinite(flat.flat).all()) and adam["step"] == 2
    for t in (tr, ref):
        t.graceful_close()


def test_a_non_logging_iteration_synchronises_nothing_back(tmp_path, monkeypatch):
    """the update of a non-logging iteration: no synchronising torch call (the sync debug mode raises on one) and no
    call of the driver's own synchronize or device-to-host copy"""
    from warp_drive_amd.managers import hip_driver as drv

    tr = _trainer(tmp_path, log_freq=1000)
    tr._generate_rollout_batch()
    tr._update_model_params(0, False)      # (first use: the launches' functions are looked up)
    torch.cuda.synchronize()
    before_theta = tr._pg_flat["shared"].flat.clone()
    calls = []
    for name in ("synchronize", "device_synchronize", "memcpy_dtoh"):
        real = getattr(drv, name)
        monkeypatch.setattr(drv, name, lambda *a, _n=name, _r=real, **kw: (calls.append(_n), _r(*a, **kw))[1])
    tr._generate_rollout_batch()
    torch.cuda.synchronize()
    calls.clear()
    before = _counts()
    torch.cuda.set_sync_debug_mode("error")
    try:
        metrics = tr._update_model_params(1, False)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert metrics == {} and calls == [] and _launched_since(before) == FIVE
    assert not _same_bytes(before_theta, tr._pg_flat["shared"].flat)
    tr.graceful_close()


def test_an_env_with_the_rollout_mixin_alone_stays_on_the_framework_path(tmp_path, caplog):
    import logging

    with caplog.at_level(logging.INFO):
        tr = _trainer(tmp_path, policy=True)
    assert tr.rollout_path == "one launch" and tr.update_path == {"shared": "framework"} and tr._pg_kernels == {}
    said = _said(caplog)
    assert len(said) == 1 and "'shared'" in said[0] and "framework path" in said[0], said
    before = _counts()
    tr._generate_rollout_batch()
    metrics = tr._update_model_params(0, True)
    assert np.isfinite(metrics["shared"]["Total loss"])
    assert not [s for s in _launched_since(before) if s.startswith("Pg")]
    tr.graceful_close()


@pytest.mark.parametrize("change,reason", [
    (dict(extra={"normalize_advantage": True}), "normalize_advantage"),
    (dict(fc=(48, 48)), "hidden width 48"),
    (dict(rollout=None), "per tick"),
])
def test_a_listed_refusal_is_logged_once_and_the_policy_stays_on_the_framework_path(tmp_path, caplog, change, reason):
    import logging

    with caplog.at_level(logging.INFO):
        tr = _trainer(tmp_path, **change)
    assert tr.update_path == {"shared": "framework"} and tr._pg_kernels == {}
    said = _said(caplog)
    assert len(said) == 1 and reason in said[0] and "framework path" in said[0], said
    tr.graceful_close()


def test_without_the_key_the_update_is_the_parent_commits(tmp_path, caplog):
    """`fused_update` unset or True: nothing is asked of the env, nothing is said, the update runs in framework ops"""
    import logging

    for i, value in enumerate((None, True)):
        with caplog.at_level(logging.INFO):
            tr = _trainer(tmp_path / str(i), fused_update=value)
        assert tr.rollout_path == "one launch" and tr.update_path == {"shared": "framework"} and tr._pg_kernels == {}
        assert _said(caplog) == []
        before = _counts()
        tr._generate_rollout_batch()
        tr._update_model_params(0, True)
        assert not [s for s in _launched_since(before) if s.startswith("Pg")]
        tr.graceful_close()
