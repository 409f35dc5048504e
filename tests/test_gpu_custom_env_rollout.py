"""The one-launch rollout of a custom environment on the MI355X (include/wd_env_rollout.h,
warp_drive_amd/utils/custom_tick.py::FusedRolloutMixin): examples/rendezvous_policy/ and the probe of tests/custom_envs/ are
registered with their device sources, compiled on first use and driven through RolloutEngine and Trainer.  Everything is
compared at tolerance 0, and every recorded tick is judged from its own inputs (tests/custom_rollout_model.py): the
recorded observation row goes through the numpy model of the network, the replayed uniform gives the expected action; the
host step is fed the RECORDED actions and must reproduce what the kernel recorded and left behind.

What was seen on the MI355X: one draw flagged near a threshold in all the cases together (the probe at N = 70, width 32,
two actions: 1 of 3150, cap 2), none elsewhere; every action that is not flagged equals the model's."""
import os

import numpy as np
import pytest

from tests import custom_rollout_model as model
from tests.classic_control_cases import near_threshold
from tests.classic_control_policy import count_below
from tests.rendezvous_helpers import registrar_for

pytestmark = pytest.mark.gpu

F_SENTINEL = np.float32(-77.25)
I_SENTINEL = 0x5EA7F00D


@pytest.fixture(scope="module", autouse=True)
def env_cache(tmp_path_factory):
    """one cache directory for the module: each unit compiles once, every later wrapper finds it"""
    path = str(tmp_path_factory.mktemp("env_cache"))
    saved = os.environ.get("WD_ENV_CACHE")
    os.environ["WD_ENV_CACHE"] = path
    yield path
    if saved is None:
        os.environ.pop("WD_ENV_CACHE", None)
    else:
        os.environ["WD_ENV_CACHE"] = saved


def _wrapper(case, reset=True):
    """(EnvWrapper by name through the registrar, reset, placeholders pushed, sampler)"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

    require_gpu()
    cls = case.env_class()
    w = EnvWrapper(env_name=cls.name, env_config=case.config(), num_envs=case.E, env_backend="hip",
                   env_registrar=registrar_for(cls, case.source()))
    if not reset:
        return w
    w.reset_all_envs()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=case.seed)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    return w, sampler


def _rng_words(sampler):
    from warp_drive_amd.managers import hip_driver as drv

    drv.synchronize()
    rng = np.zeros(4 + int(sampler._n_threads), dtype=np.uint32)
    drv.memcpy_dtoh(rng, sampler.rng_state)
    drv.synchronize()
    return rng


def _same_bits(got, want, what):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want, dtype=got.dtype).reshape(got.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {np.argwhere(got != want)[:5].tolist()}"


def _batch(case, rows, dev):
    """the four batch tensors, `rows` rows each, every word a sentinel"""
    import torch

    E, N, F = case.E, case.N, case.F
    return {"obs": torch.full((rows, E, N, F), float(F_SENTINEL), dtype=torch.float32, device=dev),
            "actions": torch.full((rows, E, N, 1), I_SENTINEL, dtype=torch.int32, device=dev),
            "rewards": torch.full((rows, E, N), float(F_SENTINEL), dtype=torch.float32, device=dev),
            "done": torch.full((rows, E), I_SENTINEL, dtype=torch.int32, device=dev)}


def _engine(case, w, sampler, ticks, rows=None):
    """(RolloutEngine on the Rollout entry of the case's width, its batch tensors, the packed policy)"""
    import torch

    from tests.hip_harness import ACT
    from warp_drive_amd.rollout import RolloutEngine

    dev = w.cuda_data_manager.data_on_device_via_torch(ACT).device
    _, packed = case.policy()
    weights = torch.from_numpy(packed).to(dev)
    batch = _batch(case, ticks + 1 if rows is None else rows, dev)
    engine = RolloutEngine(w, sampler, rollout_batch=batch, rollout_policy=(weights, case.hidden), ticks_per_launch=ticks)
    assert engine.fused and engine.entry_names == [w.env.ROLLOUT_KERNEL.format(width=case.hidden)]
    assert engine.ticks_per_launch == ticks and w.env.ticks_per_launch == 1 and len(engine.plan) == 1
    return engine, batch, packed


def _state(case, w):
    from tests.hip_harness import ACT, OBS, REW, pull

    names = [OBS, REW, ACT, "_done_", "_timestep_"] + (["loc_x", "loc_y"] if case.kind == "rendezvous" else [])
    return {name: pull(w, name) for name in names}


def _run_against_the_model(case):
    """LAUNCHES launches of `case.ticks` ticks; returns the number of near-threshold draws"""
    from tests.hip_harness import ACT, OBS, REW
    from warp_drive_amd.managers import hip_driver as drv

    E, N, F, T, A = case.E, case.N, case.F, case.ticks, case.A
    w, sampler = _wrapper(case)
    engine, batch, packed = _engine(case, w, sampler, T)
    host = model.HostReplicas(case.env_class(), case.config(), E)
    before = _rng_words(sampler)
    assert before[:2].tolist() == list(model.tick_model.seed_words(case.seed))
    assert (before[4:4 + E * N] == 0).all()
    near = 0
    seen = np.zeros(A, dtype=np.int64)
    for launch in range(case.launches):
        engine.run(1)
        drv.synchronize()
        got = {k: v.cpu().numpy() for k, v in batch.items()}
        for key, sentinel in (("obs", F_SENTINEL), ("rewards", F_SENTINEL), ("actions", I_SENTINEL), ("done", I_SENTINEL)):
            assert (got[key][T] == sentinel).all(), f"the row behind the last tick of {key}, launch {launch}"
        for k in range(T):
            where = f"launch {launch}, tick {k}"
            # the observation this tick's action was drawn on: what the previous tick (or its restart) left
            _same_bits(got["obs"][k], host.obs, f"obs_batch, {where}")
            obs = got["obs"][k].reshape(E * N, F)
            cum = model.model_sums(packed, case.hidden, obs, A)
            u = model.replayed_uniform(case.seed, E * N, launch * T + k)
            flagged = near_threshold(cum, u)
            near += int(flagged.sum())
            want = count_below(cum, u)
            actions = got["actions"][k].reshape(E * N)
            assert actions.min() >= 0 and actions.max() < A, where
            assert (actions[~flagged] == want[~flagged]).all(), \
                f"actions, {where}: rows {np.flatnonzero((actions != want) & ~flagged)[:5].tolist()}"
            seen += np.bincount(actions, minlength=A)
            rewards, done = host.step(actions.reshape(E, N))
            _same_bits(got["rewards"][k], rewards, f"reward_batch, {where}")
            _same_bits(got["done"][k], done, f"done_batch, {where}")
        # what the launch left behind
        state = _state(case, w)
        _same_bits(state[OBS], host.obs, f"observations after launch {launch}")
        _same_bits(state[REW], rewards, f"rewards after launch {launch}")
        _same_bits(state[ACT], actions, f"actions after launch {launch}")
        _same_bits(state["_done_"], done, f"_done_ after launch {launch}")
        _same_bits(state["_timestep_"], host.timesteps(), f"_timestep_ after launch {launch}")
        if case.kind == "rendezvous":
            _same_bits(state["loc_x"], host.array("loc_x"), f"loc_x after launch {launch}")
            _same_bits(state["loc_y"], host.array("loc_y"), f"loc_y after launch {launch}")
        rng = _rng_words(sampler)
        assert rng[:4].tolist() == before[:4].tolist()
        assert (rng[4:4 + E * N] == (launch + 1) * T).all()
        assert rng[4 + E * N:].tobytes() == before[4 + E * N:].tobytes()
    print(f"{case}: {near} near-threshold draws of {case.draws} (cap {case.near_cap()}), actions {seen.tolist()}, "
          f"{host.early} early and {host.timed} timed finishes")
    assert near <= case.near_cap()
    if A > 1:
        assert (seen > 0).all()
    return host


# ------------------------------------------------------------------------------------------ rollout against the model
@pytest.mark.parametrize("case", model.RENDEZVOUS_CASES, ids=repr)
def test_rollout_against_the_model(case):
    host = _run_against_the_model(case)
    assert host.timed >= 1 and (host.early >= 1 or case.N == 1)


def test_a_block_over_the_launch_bound_is_refused():
    """N = 520 is a block of 576 threads: the width-32 entry (bound 1024) serves it, the width-64 entry (bound 512) is
    asked for by nobody -- the env says no, RolloutEngine refuses, nothing is launched"""
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    case = model.Case("rendezvous", *model.WIDE_SHAPE, hidden=64)
    w, sampler = _wrapper(case)
    assert w.env.has_live_policy_rollout(32, 5) and not w.env.has_live_policy_rollout(64, 5)
    with pytest.raises(UnsupportedRolloutShape, match="hidden width 64"):
        _engine(case, w, sampler, case.ticks)
    import torch

    from tests.hip_harness import ACT

    dev = w.cuda_data_manager.data_on_device_via_torch(ACT).device
    weights = torch.from_numpy(case.policy()[1]).to(dev)
    w.env.ticks_per_launch = case.ticks
    try:
        with pytest.raises(UnsupportedRolloutShape, match="576 threads"):
            w.env.tick_launch(sampler, [None], w.env_resetter, batch=_batch(case, case.ticks + 1, dev),
                              policy=(weights, 64))
    finally:
        w.env.ticks_per_launch = 1


# --------------------------------------------------------------------------------------- one launch against T launches
@pytest.mark.parametrize("hidden", model.WIDTHS)
@pytest.mark.parametrize("shape", model.ONE_LAUNCH_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_launch_of_T_ticks_equals_T_launches_of_one(shape, hidden):
    """two wrappers from the same seeds: ONE launch of T ticks on the first; on the second T launches of one tick
    (`ticks_per_launch = 1`, a batch of one row and one sentinel row), row 0 copied out after each.  Every env array,
    every batch row and the RNG state are equal bit for bit; replicas finish and restart inside the launch."""
    from warp_drive_amd.managers import hip_driver as drv

    case = model.Case("rendezvous", *shape, hidden=hidden)
    T = case.ticks
    (w1, s1), (w2, s2) = _wrapper(case), _wrapper(case)
    multi, batch_multi, _ = _engine(case, w1, s1, T)
    single, batch_single, _ = _engine(case, w2, s2, 1)
    multi.run(1)
    rows = {k: [] for k in batch_single}
    for _ in range(T):
        single.run(1)
        drv.synchronize()
        for k, v in batch_single.items():
            assert (v[1].cpu().numpy() == (F_SENTINEL if v.dtype.is_floating_point else I_SENTINEL)).all()
            rows[k].append(v[0].cpu().numpy().copy())
    drv.synchronize()
    for k, v in batch_multi.items():
        _same_bits(v[:T].cpu().numpy(), np.stack(rows[k]), f"batch {k}")
    got, want = _state(case, w1), _state(case, w2)
    for k in want:
        _same_bits(got[k], want[k], f"{k} after the launch")
    rng1, rng2 = _rng_words(s1), _rng_words(s2)
    assert rng1.tobytes() == rng2.tobytes() and (rng1[4:4 + case.E * case.N] == T).all()
    done = np.stack(rows["done"])
    assert done.sum() >= 1 and done[:-1].sum() >= 1   # a restart inside the launch, not only on its last tick


# ------------------------------------------------------------------------------------------------------- the probe
@pytest.mark.parametrize("case", model.PROBE_CASES, ids=repr)
def test_the_probe_against_the_model(case):
    """F = 2 and a run-time action count: A = 1, 2, 8 at one agent, a partial wavefront and two wavefronts.  The rewards
    are action + 1: the step was handed the action that was recorded."""
    host = _run_against_the_model(case)
    assert host.timed == case.E * (case.ticks * case.launches // case.L) and host.early == 0


# ---------------------------------------------------------------------------------------- the Step entry on its own
@pytest.mark.parametrize("N,L", [(5, 4), (70, 6)])
def test_consistency_checker_on_the_policy_example(N, L):
    """HipRendezvousPolicyStep (the `__device__` step behind an entry that reads the action array) against the host step:
    the checker of tests/test_gpu_custom_env.py, tolerance 0 -- so it agrees with HipRendezvousStep and
    HipRendezvousFusedStep, held to the same host step there"""
    from tests.hip_harness import require_gpu
    from tests.rendezvous_helpers import host_run, spread_limit_for
    from warp_drive_amd.env_cpu_gpu_consistency_checker import EnvironmentCPUvsGPU

    require_gpu()
    E, episodes, T, seed = 3, 2, 12, 11
    config = dict(num_agents=N, grid_length=L, episode_length=T, seed=N, wall_penalty=0.125)
    config["spread_limit"] = spread_limit_for(config, E, episodes * T, seed, percentile=10)
    _, early, timed = host_run(config, E, episodes * T, seed)
    assert timed >= 1 and early >= 1
    cls = model.policy_module().RendezvousPolicy
    checker = EnvironmentCPUvsGPU(dual_mode_env_class=cls, env_configs={"policy": config}, num_envs=E,
                                  num_episodes=episodes, env_registrar=registrar_for(cls, model.POLICY_SOURCE))
    checker.test_env_reset_and_step(seed=seed, atol=0)


# ------------------------------------------------------------------------------------------------------- the trainer
def _trainer(tmp_path, fc_dims, fused):
    from warp_drive_amd.training.trainer import Trainer

    E, N, T = 4, 5, 12
    case = model.Case("rendezvous", E, N, 6, T, hidden=32)
    case._config = dict(num_agents=N, grid_length=6, episode_length=T, seed=9)
    w = _wrapper(case, reset=False)
    trainer_config = {"num_envs": E, "train_batch_size": E * 6, "num_episodes": 100, "seed": 5}
    if fused is not None:
        trainer_config["fused_rollout_policy"] = fused
    config = {"name": "rendezvous_policy", "trainer": trainer_config,
              "policy": {"shared": {"to_train": True, "algorithm": "A2C", "lr": 0.01, "vf_loss_coeff": 1, "gamma": 0.98,
                                    "model": {"type": "fully_connected", "fc_dims": list(fc_dims)}}},
              "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0, "basedir": str(tmp_path),
                         "name": "rendezvous_policy", "tag": "test"}}
    return Trainer(env_wrapper=w, config=config, policy_tag_to_agent_id_map={"shared": list(range(N))},
                   results_dir=str(tmp_path), verbose=False), w, (E, N, T)


def test_trainer_takes_the_one_launch_when_asked(tmp_path):
    import torch

    trainer, w, (E, N, T) = _trainer(tmp_path, [32, 32], "all")
    assert trainer.rollout_path == "one launch" and trainer.update_path == {"shared": "framework"}
    assert trainer.engine.fused and trainer.engine.entry_names == ["HipRendezvousPolicyRollout_H32"]
    assert trainer.engine.ticks_per_launch == 6 and w.env.ticks_per_launch == 1
    before = [p.detach().clone() for p in trainer.models["shared"].parameters()]
    metrics = trainer.train(2)
    assert torch.isfinite(torch.tensor(metrics["shared"]["Total loss"]))
    after = list(trainer.models["shared"].parameters())
    assert any((a != b).any() for a, b in zip(before, after)) and all(torch.isfinite(p).all() for p in after)
    rewards, steps = trainer.evaluate_episodes(use_argmax=False)
    trainer.graceful_close()
    assert trainer.evaluation_path == "per tick"
    assert steps["shared"].shape == (E,) and (steps["shared"] >= 1).all() and (steps["shared"] <= T).all()
    assert rewards["shared"].shape == (E, N) and np.isfinite(rewards["shared"]).all()


@pytest.mark.parametrize("fc_dims,fused", [([32, 32], None), ([48, 48], "all")], ids=["opt-in", "width-48"])
def test_trainer_stays_per_tick_otherwise(tmp_path, fc_dims, fused):
    """without the key the path is not taken (it is opt-in); a [48, 48] model has no entry"""
    trainer, _, _ = _trainer(tmp_path, fc_dims, fused)
    assert trainer.rollout_path == "per tick" and trainer.update_path == {"shared": "framework"}
    assert trainer.engine.fused and trainer.engine.entry_names == ["HipRendezvousPolicyTick"]
    trainer.train(1)
    trainer.graceful_close()
