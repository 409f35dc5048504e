"""DDPG for the Box envs, on the host: the code object of the four HipClassicControl<X>EnvRollout_A<width> entries, which
env classes admit them, the launch `tick_launch(actor=...)` builds (fakes for the managers, those of
tests/test_classic_control_policy_host.py), the packed actor, the restatement of its arithmetic
(tests/classic_control_actor.py) against the PyTorch module, the sizing of the GPU parity test, the DDPG objective against
the reference's recorded results (tests/golden/ddpg_loss_fixtures.npz, scripts/gen_ddpg_golden.py), the targets' soft
update and one update step of TrainerDDPG on CPU tensors."""
import json
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import classic_control_actor as ca
from tests import classic_control_cases as cc
from tests.test_classic_control_policy_host import (_FakeFM, _FakeResetter, _classes, _fake_managed, _manifest, _tensor)

ACTOR_KERNELS = [f"{ca.ENTRY[env]}Rollout_A{h}" for env in ca.BOX_ENVS for h in (32, 64)]
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_actor_kernels_in_the_code_object_without_scratch_or_spills():
    """all four entries are in wd_kernels_cc.hsaco with no private segment, no spilled VGPR and a workgroup of 256"""
    from warp_drive_amd import build as wd_build

    manifest = _manifest()
    for k in ACTOR_KERNELS:
        assert manifest.get(k) == "wd_kernels_cc.hsaco", k
    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "cc.elf")
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={os.path.join(wd_build.CSRC, 'wd_kernels_cc.hsaco')}", f"--output={elf}"],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                               text=True).stdout
    found = re.findall(r"\.max_flat_workgroup_size:\s+(\d+)\n\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                       r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", notes)
    found = {n: (int(wg), int(p), int(v)) for wg, n, p, v in found if n in ACTOR_KERNELS}
    assert set(found) == set(ACTOR_KERNELS)
    for name, (workgroup, private, spills) in found.items():
        assert (workgroup, private, spills) == (256, 0, 0), (name, workgroup, private, spills)


def test_which_envs_admit_a_live_actor():
    """true exactly for (ContinuousMountainCar | Pendulum) x {32, 64} with the entry in the manifest"""
    manifest = _manifest()
    for name, (cls, _, x) in _classes().items():
        box = name in ca.BOX_ENVS
        assert getattr(cls, "ROLLOUT_ACTOR_WIDTHS", None) == ((32, 64) if box else None), name
        env = _fake_managed(name, 1000, manifest)
        for width in (8, 16, 31, 32, 33, 48, 64, 128, 256):
            assert env.has_live_actor_rollout(width) is (box and width in (32, 64)), (name, width)
        # ... and only while the code object has the entry
        env.cuda_function_manager = _FakeFM({k: v for k, v in manifest.items() if "Rollout_A32" not in k})
        assert not env.has_live_actor_rollout(32) and env.has_live_actor_rollout(64) is box


@pytest.mark.parametrize("env_name", ca.BOX_ENVS)
@pytest.mark.parametrize("width", [32, 64])
def test_tick_launch_with_an_actor(env_name, width):
    """the Rollout_A<width> entry; the tick's arguments unchanged, then (packed, width, action_scale, action_bias,
    mean_batch or null); 4 n_w bytes of LDS; anything else is UnsupportedRolloutShape"""
    import torch
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    E, T = 1000, 5
    O, x = cc.OBS_DIM[env_name], _classes()[env_name][2]
    env = _fake_managed(env_name, E, _manifest())
    env.cuda_data_manager.device_data = lambda name: ("device", name)
    env.ticks_per_launch = T
    probs = _tensor((E, 1, 1), torch.float32)
    sampler = types.SimpleNamespace(rng_state="rng")
    OP = O + O % 2
    n_w = OP * width + width + width * width + width + width + 1   # W0 [H][OP], b0, W1 [H][H], b1, Wa [H], ba
    assert n_w == ca.actor_weight_count(O, width)
    if (env_name, width) == ("pendulum", 64):
        assert 4 * n_w == 18180   # 4 * (4 * 64 + 64 + 64 * 64 + 64 + 64 + 1)
    packed = _tensor((n_w,), torch.float32)
    means = _tensor((T + 2, E), torch.float32)
    plain = env.tick_launch(sampler, [probs], _FakeResetter(), ou_params=(0.1, 0.3, 0.5))
    for mean_batch in (None, means):
        fn, args, block, grid, shared = env.tick_launch(sampler, [probs], _FakeResetter(), ou_params=(0.1, 0.3, 0.5),
                                                        actor=(packed, width, 1.25, 0.75), mean_batch=mean_batch)
        assert fn.name == f"HipClassicControl{x}EnvRollout_A{width}" and shared == 4 * n_w <= 65536
        assert (block, grid) == (plain[2], plain[3])
        assert len(args) == len(plain[1]) + 5
        for g, w in zip(args[:-5], plain[1]):
            assert type(g) is type(w) and g == w
        assert args[-5] is packed
        assert type(args[-4]) is np.int32 and args[-4] == width
        assert type(args[-3]) is np.float32 and args[-3] == np.float32(1.25)
        assert type(args[-2]) is np.float32 and args[-2] == np.float32(0.75)
        if mean_batch is None:
            assert type(args[-1]) is np.uint64 and args[-1] == 0
        else:
            assert args[-1] is means
    bad = [(_tensor((n_w + 1,), torch.float32), width, 1.0, 0.0), (_tensor((n_w,), torch.float64), width, 1.0, 0.0),
           (_tensor((n_w,), torch.float32, cuda=False), width, 1.0, 0.0),
           (_tensor((n_w,), torch.float32, contiguous=False), width, 1.0, 0.0),
           (packed, 48, 1.0, 0.0), (packed, 96 - width, 1.0, 0.0), (packed, width), packed, (packed, width, "x", 0.0)]
    for actor in bad:
        with pytest.raises(UnsupportedRolloutShape):
            env.tick_launch(sampler, [probs], _FakeResetter(), actor=actor)
    for mean_batch in (_tensor((T - 1, E), torch.float32), _tensor((T, E + 1), torch.float32),
                       _tensor((T, E), torch.float64), _tensor((T, E), torch.float32, cuda=False)):
        with pytest.raises(UnsupportedRolloutShape):
            env.tick_launch(sampler, [probs], _FakeResetter(), actor=(packed, width, 1.0, 0.0), mean_batch=mean_batch)
    with pytest.raises(UnsupportedRolloutShape):   # the record of the means belongs to the actor's launch
        env.tick_launch(sampler, [probs], _FakeResetter(), mean_batch=means)


@pytest.mark.parametrize("env_name", ["acrobot", "mountain_car"])
def test_discrete_envs_refuse_an_actor(env_name):
    import torch
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    env = _fake_managed(env_name, 1000, _manifest())
    with pytest.raises(UnsupportedRolloutShape):
        env.tick_launch(types.SimpleNamespace(rng_state="rng"), [_tensor((1000, 1, 3), torch.float32)], _FakeResetter(),
                        actor=(_tensor((100,), torch.float32), 32, 1.0, 0.0))


@pytest.mark.parametrize("O", [3, 2])
@pytest.mark.parametrize("hidden", [32, 64])
def test_pack_rollout_actor_against_a_hand_built_layout(O, hidden):
    """W0 [H][OP] with Pendulum's zero pad column, b0, W1, b1, Wa, ba; the refill is in place"""
    import torch
    from warp_drive_amd.envs.classic_control import rollout_actor_floats
    from warp_drive_amd.training.models_ddpg import FullyConnectedActor
    from warp_drive_amd.training.policy_kernel import pack_rollout_actor, rollout_actor_width

    torch.manual_seed(3)
    model = FullyConnectedActor(O, [hidden, hidden], 2.0, 0.5)
    packed = pack_rollout_actor(model)
    OP = 4 if O == 3 else 2
    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    w0 = np.zeros((hidden, OP), np.float32)
    w0[:, :O] = sd["fc.0.0.weight"]
    want = np.concatenate([w0.reshape(-1), sd["fc.0.0.bias"], sd["fc.1.0.weight"].reshape(-1), sd["fc.1.0.bias"],
                           sd["action_head.weight"].reshape(-1), sd["action_head.bias"]])
    assert packed.dtype == torch.float32 and packed.is_contiguous()
    assert packed.numel() == want.size == ca.actor_weight_count(O, hidden) == rollout_actor_floats(O, hidden)
    np.testing.assert_array_equal(packed.numpy(), want)
    if O == 3:
        assert (packed.numpy()[:hidden * OP].reshape(hidden, OP)[:, 3] == 0).all()
    # in place: the launch plan holds the tensor's address
    with torch.no_grad():
        model.fc["1"][0].weight.add_(1.0)
        model.action_head.bias.fill_(7.0)
    ptr = packed.data_ptr()
    packed.fill_(-3.0)   # (the pad column too: the refill must restore its zeros)
    again = pack_rollout_actor(model, out=packed)
    assert again is packed and packed.data_ptr() == ptr
    want2 = want.copy()
    o = hidden * OP + hidden
    want2[o:o + hidden * hidden] += 1.0
    want2[-1] = 7.0
    np.testing.assert_array_equal(packed.numpy(), want2)
    # widths
    assert rollout_actor_width(model, O) == hidden and rollout_actor_width(model, O + 1) is None
    assert rollout_actor_width(model, O, widths=(16,)) is None
    assert rollout_actor_width(FullyConnectedActor(O, [hidden], 1.0, 0.0), O) is None
    assert rollout_actor_width(FullyConnectedActor(O, [hidden, 32 if hidden == 64 else 64], 1.0, 0.0), O) is None
    assert rollout_actor_width(FullyConnectedActor(O, [48, 48], 1.0, 0.0), O) is None


@pytest.mark.parametrize("env", ca.BOX_ENVS)
@pytest.mark.parametrize("hidden", [32, 64])
def test_actor_restatement_matches_the_torch_module(env, hidden):
    """actor_mean_f32 within float32 accuracy of the module: against its float64 copy, at most 4 x the float32 module's
    own error with a floor of 8 float32 ulps of the largest mean (the bound of the GPU test); actor_mean_f64 agrees with
    the float64 copy to 1e-12"""
    import copy

    import torch
    from warp_drive_amd.training.models_ddpg import FullyConnectedActor
    from warp_drive_amd.training.policy_kernel import pack_rollout_actor

    O = cc.OBS_DIM[env]
    torch.manual_seed(7)
    scale, bias = (2.0, 0.0) if env == "pendulum" else (1.25, 0.75)
    model = FullyConnectedActor(O, [hidden, hidden], scale, bias)
    with torch.no_grad():
        model.action_head.weight.mul_(6.0)
    packed = pack_rollout_actor(model).numpy()
    rng = np.random.RandomState(O * 100 + hidden)
    obs = rng.uniform(-3, 3, size=(20000, O)).astype(np.float32)
    with torch.no_grad():
        want64 = copy.deepcopy(model).double()(torch.from_numpy(obs).double())[:, 0].numpy()
        torch32 = model(torch.from_numpy(obs))[:, 0].numpy()
    got32 = ca.actor_mean_f32(packed, hidden, obs, scale, bias)
    got64 = ca.actor_mean_f64(packed, hidden, obs, scale, bias)
    assert got32.dtype == np.float32 and got64.dtype == np.float64
    assert np.abs(got64 - want64).max() <= 1e-12
    err, err_torch = np.abs(got32 - want64).max(), np.abs(torch32.astype(np.float64) - want64).max()
    print(f"{env} H={hidden}: restatement {err:.2e}, float32 module {err_torch:.2e}")
    assert err <= max(4.0 * err_torch, 8.0 * 2.0 ** -24 * np.abs(want64).max())
    assert np.ptp(want64) > 0.5 * scale   # the means vary with the observation: not one constant


@pytest.mark.parametrize("case", ca.CASES, ids=repr)
def test_parity_case_is_not_vacuous_on_the_host(case):
    """the GPU parity test's actor, seeds and sizes replayed on the host alone: at least a tenth of the means in tanh's
    linear range, at least a tenth in its saturated range, restarts happen (and every pool row is drawn)"""
    r = ca.simulate(case)
    t = r["tanh"]
    assert t.shape == (case.launches * case.ticks, case.E)
    linear, saturated = float((t < 0.5).mean()), float((t > 0.99).mean())
    print(f"{case.name}: |tanh z| < 0.5 {linear:.3f}, > 0.99 {saturated:.3f}, {r['restarts']} restarts, pool rows "
          f"{len(r['pool_rows'])} of {case.pool}")
    assert linear >= 0.1 and saturated >= 0.1
    assert r["restarts"] >= (case.launches * case.ticks // case.T) * case.E
    assert not case.pool or len(r["pool_rows"]) == case.pool


def test_parity_geometries_take_their_trips():
    """block 256 x grid 1: three trips, the last partial; block 64 x grid 3: more than three; a grid with idle blocks"""
    assert cc.geometry(700, (256, 1)) == (256, 1, 3) and 700 % 256 != 0
    assert cc.geometry(700, (64, 3)) == (64, 3, 4)
    assert cc.geometry(700, (64, "idle"))[1] == 11 + 2
    assert cc.geometry(1, (256, 1)) is None and cc.geometry(1, (64, 3)) is None   # (E = 1: the host's and the idle grid)


# ------------------------------------------------------------------------------------------------------ objective
def test_ddpg_objective_matches_the_reference_fixtures():
    """tests/golden/ddpg_loss_fixtures.npz = the reference's DDPG.compute_loss_and_metrics on seeded random batches: n_step
    1, 3 and T, done flags mid-batch and on the last row, with and without the normalisations.  Both losses, every logged
    metric and the gradients w.r.t. the value and J inputs agree to the tolerances tests/test_trainer_cpu.py uses for the
    A2C / PPO fixtures (1e-6; gradients rtol 1e-5, atol 1e-7)."""
    import torch
    from warp_drive_amd.training.losses import DDPG

    g = np.load(os.path.join(_GOLDEN, "ddpg_loss_fixtures.npz"))
    meta = json.loads(str(g["meta"]))
    assert set(meta) == {f"n{n}_{k}" for n in (1, 3, 9) for k in ("plain", "norm")}
    for name, m in meta.items():
        values = torch.tensor(g[f"{name}.values"], requires_grad=True)
        j_values = torch.tensor(g[f"{name}.j_values"], requires_grad=True)
        done = g[f"{name}.done"]
        assert values.shape == (9, 6, 1) and done[-1].any() and not done[-1].all() and done[:-1].any()
        actor_loss, critic_loss, metrics = DDPG(**m["kwargs"]).compute_loss_and_metrics(
            timestep=m["timestep"], actions_batch=torch.tensor(g[f"{name}.actions"]),
            rewards_batch=torch.tensor(g[f"{name}.rewards"]), done_flags_batch=torch.tensor(done),
            value_functions_batch=values, next_value_functions_batch=torch.tensor(g[f"{name}.next_values"]),
            j_functions_batch=j_values, perform_logging=True)
        for got, key in ((actor_loss, "actor_loss"), (critic_loss, "critic_loss")):
            want = float(g[f"{name}.{key}"])
            assert abs(got.item() - want) <= 1e-6 * max(1.0, abs(want)), (name, key, got.item(), want)
        assert set(metrics) == set(m["metrics"]), name
        for k, want in m["metrics"].items():
            if np.isnan(want):   # (the standard deviation over one agent)
                assert np.isnan(metrics[k]), (name, k)
            else:
                assert abs(float(metrics[k]) - want) <= 1e-6 * max(1.0, abs(want)), (name, k, metrics[k], want)
        critic_loss.backward()
        actor_loss.backward()
        np.testing.assert_allclose(values.grad.numpy(), g[f"{name}.grad_values"], rtol=1e-5, atol=1e-7, err_msg=name)
        np.testing.assert_allclose(j_values.grad.numpy(), g[f"{name}.grad_j_values"], rtol=1e-5, atol=1e-7, err_msg=name)
        V = 9 - m["kwargs"]["n_step"] + 1
        assert (values.grad[V:] == 0).all() and (j_values.grad[V:] == 0).all()   # only the valid rows count


def test_soft_update_follows_the_tau_rule():
    """t <- t * (1 - tau) + p * tau: within 2 float32 ulps of the float32 expression (it IS the expression: each product
    and the sum round once), and within float32 rounding of its float64 value"""
    import torch
    from tests.hip_harness import ulp_diff
    from warp_drive_amd.training.models_ddpg import FullyConnectedActor
    from warp_drive_amd.training.trainer_ddpg import hard_update, soft_update

    torch.manual_seed(1)
    target, source = FullyConnectedActor(3, [32, 32]), FullyConnectedActor(3, [32, 32])
    for tau in (0.05, 0.5, 0.0, 1.0):
        before = [t.detach().clone() for t in target.parameters()]
        soft_update(target, source, tau)
        for t, t0, p in zip(target.parameters(), before, source.parameters()):
            want = t0 * (1.0 - tau) + p.detach() * tau
            assert ulp_diff(t.detach().numpy(), want.numpy()).max() <= 2, tau
            want64 = t0.double() * (1.0 - tau) + p.detach().double() * tau
            scale = float(torch.maximum(t0.abs(), p.detach().abs()).max())
            assert float((t.detach().double() - want64).abs().max()) <= 2 * 2.0 ** -24 * scale, tau
        if tau == 0.0:   # nothing moved
            assert all(torch.equal(t, t0) for t, t0 in zip(target.parameters(), before))
    with torch.no_grad():
        for p in source.parameters():
            p.add_(1.0)
    hard_update(target, source)
    for t, p in zip(target.parameters(), source.parameters()):
        assert torch.equal(t, p) and t.data_ptr() != p.data_ptr()


def test_trainer_refuses_ddpg_and_train_script_knows_the_configs():
    import yaml
    from warp_drive_amd.training.scripts import train

    for name in ("single_pendulum", "single_continuous_mountain_car"):
        assert name in train._ENVS
        cfg = yaml.safe_load(open(os.path.join(train._CONFIGS, f"{name}.yaml")))
        pol = cfg["policy"]["shared"]
        assert cfg["name"] == name and cfg["env"]["reset_pool_size"] > 1
        assert pol["algorithm"] == "DDPG" and (pol["gamma"], pol["tau"], cfg["trainer"]["n_step"]) == (0.99, 0.05, 5)
        assert pol["model"]["actor"]["fc_dims"] == pol["model"]["critic"]["fc_dims"] == [64, 64]
        assert cfg["sampler"]["params"] == {"damping": 0.15, "stddev": 0.2, "scale": 1.0}
        assert cfg["trainer"]["train_batch_size"] // cfg["trainer"]["num_envs"] >= cfg["trainer"]["n_step"]


def test_one_update_step_on_cpu_tensors():
    """TrainerDDPG._update_model_params on CPU tensors (the object assembled by hand: its constructor needs a device env):
    the critic moves by the critic loss alone -- its step is the step of a copy trained on that loss only --, the actor
    moves, the targets follow by tau, nothing happens with fewer rows than n_step"""
    import copy

    import torch
    from warp_drive_amd.training.losses import DDPG
    from warp_drive_amd.training.models_ddpg import FullyConnectedActionValueCritic, FullyConnectedActor
    from warp_drive_amd.training.param_scheduler import ParamScheduler
    from warp_drive_amd.training.trainer_ddpg import TrainerDDPG

    torch.manual_seed(0)
    T, E, O, n_step, tau, pol = 6, 8, 3, 5, 0.05, "shared"
    tr = TrainerDDPG.__new__(TrainerDDPG)
    tr.policies, tr.batch_len, tr.n_step, tr.tau, tr.train_batch_size = [pol], T, n_step, tau, T * E
    tr.config = {"policy": {pol: {"to_train": True, "clip_grad_norm": True, "max_grad_norm": 3.0}}}
    tr.actors = {pol: FullyConnectedActor(O, [32, 32], 2.0, 0.0)}
    tr.critics = {pol: FullyConnectedActionValueCritic(O + 1, [32, 32])}
    tr.target_actors, tr.target_critics = copy.deepcopy(tr.actors), copy.deepcopy(tr.critics)
    tr.actor_optimizers = {pol: torch.optim.Adam(tr.actors[pol].parameters(), lr=1e-3)}
    tr.critic_optimizers = {pol: torch.optim.Adam(tr.critics[pol].parameters(), lr=1e-3)}
    tr.lr_schedules = {pol: (ParamScheduler(1e-3), ParamScheduler([[0, 1e-2], [T * E, 5e-3]]))}
    tr.trainers = {pol: DDPG(discount_factor_gamma=0.99, n_step=n_step)}
    tr.current_timestep = {pol: 0}
    tr.batch = {pol: {"obs": torch.randn(T, E, 1, O), "actions": torch.randn(T, E, 1, 1), "rewards": torch.randn(T, E, 1)}}
    tr.done_batch = (torch.rand(T, E) < 0.2).to(torch.int32)
    tr._ep_sum, tr._ep_cnt = {pol: torch.ones(E)}, torch.ones(E)
    actor0, critic0 = copy.deepcopy(tr.actors[pol]), copy.deepcopy(tr.critics[pol])
    # the critic's expected step: the critic loss alone
    twin = copy.deepcopy(critic0)
    opt = torch.optim.Adam(twin.parameters(), lr=5e-3)
    b = tr.batch[pol]
    with torch.no_grad():
        nv = critic0(b["obs"][1:], actor0(b["obs"][1:]))
    _, loss, _ = tr.trainers[pol].compute_loss_and_metrics(0, b["actions"], b["rewards"], tr.done_batch,
                                                          twin(b["obs"], b["actions"]), nv, nv.new_zeros(T, E, 1))
    loss.backward()
    torch.nn.utils.clip_grad_norm_(twin.parameters(), 3.0)
    opt.step()
    metrics = tr._update_model_params(0, True)[pol]
    for p, q in zip(tr.critics[pol].parameters(), twin.parameters()):
        torch.testing.assert_close(p, q, rtol=0, atol=1e-7)
    assert any(not torch.equal(p, q) for p, q in zip(tr.actors[pol].parameters(), actor0.parameters()))
    for net, net0, target in ((tr.actors[pol], actor0, tr.target_actors[pol]),
                              (tr.critics[pol], critic0, tr.target_critics[pol])):
        for p, p0, t in zip(net.parameters(), net0.parameters(), target.parameters()):
            torch.testing.assert_close(t, p0 * (1 - tau) + p.detach() * tau, rtol=0, atol=1e-7)
    assert tr.current_timestep[pol] == T * E and metrics["Learning rate (Critic)"] == 5e-3
    assert all(np.isfinite(metrics[k]) for k in ("Total loss", "Actor loss", "Critic loss", "Gradient norm (Actor)",
                                                 "Gradient norm (Critic)", "Mean episodic reward"))
    # fewer rows than n_step: no valid row, no update
    tr.batch_len = n_step - 1
    before = copy.deepcopy(tr.actors[pol])
    m = tr._update_model_params(1, True)[pol]
    assert np.isnan(m["Total loss"]) and tr.current_timestep[pol] == T * E
    assert all(torch.equal(p, q) for p, q in zip(tr.actors[pol].parameters(), before.parameters()))
