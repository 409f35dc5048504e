"""The fused tick of a custom environment on the MI355X (include/wd_env_tick.h, warp_drive_amd/utils/custom_tick.py):
examples/rendezvous_fused/ and the several-heads probe of tests/custom_envs/ are registered with their device sources,
compiled on first use and driven through RolloutEngine and Trainer.  Everything is exact (tolerance 0) and every expected
value comes from the host: tests/custom_tick_model.py draws the actions from the seed and the probability tensors, the
host env is stepped with them, finished replicas restart."""
import os

import numpy as np
import pytest

from tests import custom_tick_model as model
from tests.rendezvous_helpers import ROOT, registrar_for

pytestmark = pytest.mark.gpu

FUSED_DIR = os.path.join(ROOT, "examples", "rendezvous_fused")
FUSED_SOURCE = os.path.join(FUSED_DIR, "rendezvous_fused.hip")
TICK, STEP = "HipRendezvousFusedTick", "HipRendezvousFusedStep"
CHECK_SEED = 11
SENTINEL = 0x5EA7F00D


def fused_module():
    import importlib.util
    import sys

    name = "rendezvous_fused_example"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(FUSED_DIR, "rendezvous_fused.py"))
        module = importlib.util.module_from_spec(spec)
        sys.modules[name] = module
        spec.loader.exec_module(module)
    return sys.modules[name]


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


def _fused_registrar(cls=None):
    return registrar_for(cls or fused_module().RendezvousFused, FUSED_SOURCE)


def _wrapper(config, num_envs, sampler_seed, registrar=None, name="RendezvousFused", reset=True):
    """(EnvWrapper by name through the registrar, reset, placeholders pushed, sampler)"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

    require_gpu()
    w = EnvWrapper(env_name=name, env_config=config, num_envs=num_envs, env_backend="hip",
                   env_registrar=registrar or _fused_registrar())
    if not reset:
        return w
    w.reset_all_envs()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=sampler_seed)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    return w, sampler


def _tick_tag():
    from warp_drive_amd.managers.function_manager import _stream_tag

    return int(_stream_tag("tick"))


def _rng_words(w, sampler):
    from warp_drive_amd.managers import hip_driver as drv

    drv.synchronize()
    rng = np.zeros(4 + w.n_envs * w.n_agents, dtype=np.uint32)
    drv.memcpy_dtoh(rng, sampler.rng_state)
    drv.synchronize()
    return rng


def _same_bits(got, want, what):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want, dtype=got.dtype).reshape(got.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {np.argwhere(got != want)[:5].tolist()}"


def _probabilities(seed, E, N, A=5):
    """seeded Dirichlet rows [E, N, A]; agent 1 (agent 0 of a one-agent replica) one-hot, agent 0 of a replica of
    several agents with probability 0 on its first two actions"""
    rng = np.random.RandomState(seed)
    p = rng.dirichlet(np.ones(A), size=(E, N)).astype(np.float32)
    hot = rng.randint(0, A, E)
    p[:, 1 % N] = np.eye(A, dtype=np.float32)[hot]
    if N > 1:
        tail = rng.dirichlet(np.ones(A - 2), size=E).astype(np.float32)
        p[:, 0, :2] = 0
        p[:, 0, 2:] = tail
    return np.ascontiguousarray(p)


def _host_envs(config, num_envs):
    envs = [fused_module().RendezvousFused(**config) for _ in range(num_envs)]
    for env in envs:
        env.reset()
    return envs


def _modelled_run(config, E, ticks, seed, probs):
    """the host replicas driven by the model's draws, restarted when they finish: per tick (actions [E, N, 1], obs,
    rewards, done, loc_x, loc_y, time steps) as the device must leave them AFTER the tick, + the largest spread per tick
    and replica, + the numbers of early finishes and of finishes at the time limit"""
    N, T = config["num_agents"], config["episode_length"]
    envs = _host_envs(config, E)
    first = np.stack([np.stack([env._observation()[a] for a in range(N)]) for env in envs])
    draws = model.TickDraws(seed, E, N, _tick_tag())
    out, maxima, early, timed = [], np.zeros((ticks, E), dtype=np.int64), 0, 0
    for t in range(ticks):
        actions = draws.draw([probs])
        steps = [envs[e].step({a: actions[e, a, 0] for a in range(N)}) for e in range(E)]
        obs = np.stack([np.stack([s[0][a] for a in range(N)]) for s in steps])
        rew = np.array([[s[1][a] for a in range(N)] for s in steps], dtype=np.float32)
        done = np.array([s[2]["__all__"] for s in steps])
        for e in range(E):
            maxima[t, e] = envs[e].last_max_spread
            if done[e]:
                early += envs[e].timestep < T
                timed += envs[e].timestep == T
                envs[e].reset()
                obs[e] = first[e]
        out.append(dict(actions=actions, obs=obs, rewards=rew, done=done.astype(np.int32),
                        loc_x=np.stack([env.loc_x for env in envs]), loc_y=np.stack([env.loc_y for env in envs]),
                        timestep=np.array([env.timestep for env in envs], dtype=np.int32)))
    return out, maxima, int(early), int(timed), draws


# -------------------------------------------------------------------------------------------- tick against the model
@pytest.mark.parametrize("E,N,L,T", [(1, 1, 4, 3), (3, 5, 4, 4), (7, 64, 6, 5), (7, 70, 6, 9), (2, 130, 8, 6)])
def test_tick_against_the_model(E, N, L, T):
    """3 T + 2 single-tick runs of HipRendezvousFusedTick, every array compared after every tick.  The spread limit is the
    10th percentile of the largest spread over the modelled run with the limit off; the seed is the first (tried on the
    host alone) whose modelled run holds an early finish and a finish at the time limit."""
    import torch

    from tests.hip_harness import ACT, OBS, REW, pull
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.rollout import RolloutEngine

    ticks = 3 * T + 2
    base = dict(num_agents=N, grid_length=L, episode_length=T, seed=N, wall_penalty=0.125)
    for seed in range(17, 17 + 50):
        probs = _probabilities(seed, E, N)
        config = dict(base, spread_limit=-1)
        if N > 1:
            _, maxima, _, _, _ = _modelled_run(config, E, ticks, seed, probs)
            config["spread_limit"] = int(np.floor(np.percentile(maxima, 10)))
        want, _, early, timed, draws = _modelled_run(config, E, ticks, seed, probs)
        if timed >= 1 and (early >= 1 if N > 1 else early == 0):
            break
    else:
        raise AssertionError("no seed gives a modelled run with an early finish and a finish at the time limit")
    print(f"({E}, {N}, {L}, {T}): seed {seed}, spread limit {config['spread_limit']}, {early} early and {timed} timed "
          "finishes")
    w, sampler = _wrapper(config, E, seed)
    dev = w.cuda_data_manager.data_on_device_via_torch(ACT).device
    engine = RolloutEngine(w, sampler, probabilities=[torch.from_numpy(probs).to(dev)])
    assert engine.fused and engine.entry_names == [TICK] and engine.ticks_per_launch == 1
    header = _rng_words(w, sampler)[:4].tolist()
    assert header == draws.header()
    for t in range(ticks):
        engine.run(1)
        drv.synchronize()
        for name, key in ((ACT, "actions"), ("loc_x", "loc_x"), ("loc_y", "loc_y"), (REW, "rewards"),
                          (OBS, "obs"), ("_done_", "done"), ("_timestep_", "timestep")):
            _same_bits(pull(w, name), want[t][key], f"{name} at tick {t}")
    rng = _rng_words(w, sampler)
    assert rng[:4].tolist() == header and (rng[4:] == ticks).all() and (draws.epochs == ticks).all()


# ---------------------------------------------------------------------------------------- the two Step entries agree
@pytest.mark.parametrize("N,L", [(5, 4), (70, 6)])
def test_consistency_checker_on_the_fused_example(N, L):
    """HipRendezvousFusedStep (the `__device__` step behind an entry that reads the action array) against the host step:
    the checker of tests/test_gpu_custom_env.py, tolerance 0 -- so it agrees with HipRendezvousStep, held to the same
    host step there"""
    from tests.hip_harness import require_gpu
    from tests.rendezvous_helpers import host_run, spread_limit_for
    from warp_drive_amd.env_cpu_gpu_consistency_checker import EnvironmentCPUvsGPU

    require_gpu()
    E, episodes, T = 3, 2, 12
    config = dict(num_agents=N, grid_length=L, episode_length=T, seed=N, wall_penalty=0.125)
    config["spread_limit"] = spread_limit_for(config, E, episodes * T, CHECK_SEED, percentile=10)
    _, early, timed = host_run(config, E, episodes * T, CHECK_SEED)
    assert timed >= 1 and early >= 1
    checker = EnvironmentCPUvsGPU(dual_mode_env_class=fused_module().RendezvousFused, env_configs={"fused": config},
                                  num_envs=E, num_episodes=episodes, env_registrar=_fused_registrar())
    checker.test_env_reset_and_step(seed=CHECK_SEED, atol=0)


# -------------------------------------------------------------------------------------------- one launch for n ticks
def _fused_state(w, sampler):
    from tests.hip_harness import ACT, OBS, REW, pull

    out = {k: pull(w, k) for k in ("loc_x", "loc_y", OBS, REW, ACT, "_done_", "_timestep_")}
    out["rng_state"] = _rng_words(w, sampler)
    return out


@pytest.mark.parametrize("n", [2, 5, 13])
@pytest.mark.parametrize("E,N,L,T", [(7, 70, 6, 4), (3, 5, 4, 4)])
def test_one_launch_for_n_ticks_equals_n_launches(E, N, L, T, n):
    """run(n) -- ONE launch of HipRendezvousFusedTick whose blocks loop over n ticks -- against n calls of run(1) on a
    second wrapper with the same seeds, from the same start: T - 1 single ticks, so that every replica's episode ends
    INSIDE the launch, on its first tick at the latest, and the loop goes on with the restarted replica"""
    from tests.rendezvous_helpers import spread_limit_for
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.rollout import RolloutEngine

    config = dict(num_agents=N, grid_length=L, episode_length=T, seed=6, wall_penalty=0.125)
    config["spread_limit"] = spread_limit_for(config, E, 30, seed=1, percentile=10)
    sides = []
    for _ in range(2):
        w, sampler = _wrapper(config, E, 23)
        engine = RolloutEngine(w, sampler)
        assert engine.fused and engine.rollout_kernel_name == TICK and engine.cohorts == 1 and len(engine.plan) == 1
        for _ in range(T - 1):
            engine.run(1)
        sides.append((w, sampler, engine))
    (w1, s1, multi), (w2, s2, single) = sides
    start = _fused_state(w1, s1)
    for k, v in _fused_state(w2, s2).items():
        _same_bits(v, start[k], f"{k} at the start")
    multi.run(n)
    for _ in range(n):
        single.run(1)
    drv.synchronize()
    got, want = _fused_state(w1, s1), _fused_state(w2, s2)
    for k in want:
        _same_bits(got[k], want[k], f"{k} after run({n})")
    assert (want["rng_state"][4:] == T - 1 + n).all()
    assert (want["_timestep_"] < T - 1 + n).all() and (want["_timestep_"] <= T).all()  # every replica restarted inside
    assert not np.array_equal(want["rng_state"], start["rng_state"])


# --------------------------------------------------------------------------------------------------- several heads
def _probe_registrar():
    from tests.custom_envs.heads_probe import SOURCE, HeadsProbe

    return registrar_for(HeadsProbe, SOURCE)


@pytest.mark.parametrize("N", [1, 5, 70])
@pytest.mark.parametrize("head_sizes", [(3,), (2, 7), (4, 1, 9, 71)], ids=lambda s: "x".join(map(str, s)))
def test_several_heads(head_sizes, N):
    """the probe env: counts[env, agent, h] += action_h + 1.  Ten single ticks through RolloutEngine (episodes of four
    ticks: the counts restart with the replica), the action tensor and the counts against the model after every tick;
    then ONE launch of ten ticks writing into an action tensor and a count array of the test's own, each between two
    fences of sentinel words."""
    import torch

    from tests.hip_harness import ACT, pull
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.rollout import RolloutEngine
    from warp_drive_amd.utils.custom_tick import custom_tick_launch

    E, T, H, seed = 3, 4, len(head_sizes), 29
    config = dict(num_agents=N, episode_length=T, head_sizes=head_sizes)
    w, sampler = _wrapper(config, E, seed, registrar=_probe_registrar(), name="HeadsProbe")
    dev = w.cuda_data_manager.data_on_device_via_torch(ACT).device
    rng = np.random.RandomState(3)
    probs = [np.ascontiguousarray(rng.dirichlet(np.ones(a), size=(E, N)).astype(np.float32)) for a in head_sizes]
    tensors = [torch.from_numpy(p).to(dev) for p in probs]
    engine = RolloutEngine(w, sampler, probabilities=tensors)
    assert engine.fused and engine.entry_names == ["HipHeadsProbeTick"] and engine.rollout_kernel_name == "HipHeadsProbeTick"
    draws = model.TickDraws(seed, E, N, _tick_tag())
    counts = np.zeros((E, N, H), dtype=np.int32)
    seen = [set() for _ in head_sizes]
    for t in range(1, 11):
        engine.run(1)
        drv.synchronize()
        actions = draws.draw(probs)
        counts += actions + 1
        finished = t % T == 0
        if finished:
            counts[:] = 0
        _same_bits(pull(w, ACT), actions, f"actions at tick {t}")
        _same_bits(pull(w, "counts"), counts, f"counts at tick {t}")
        assert (pull(w, "_done_") == int(finished)).all() and (pull(w, "_timestep_") == t % T).all()
        for h in range(H):
            assert actions[..., h].min() >= 0 and actions[..., h].max() < head_sizes[h]
            seen[h] |= set(actions[..., h].reshape(-1).tolist())
    if N >= 5:  # (the model's own draws: at least 150 per head, so every head of two or more actions shows two)
        assert all(len(s) >= min(a, 2) for s, a in zip(seen, head_sizes))
    # ---- one launch of ten ticks into fenced arrays of the test's own (the reset table still lists the data manager's
    # `counts`, so these counts are never restarted: they are the sum over the ten ticks)
    pad, n = 64, E * N * H
    fenced = {k: torch.full((pad + n + pad,), SENTINEL, dtype=torch.int32, device=dev) for k in ("counts", "actions")}
    fenced["counts"][pad:pad + n] = 0
    fn, args, block, grid, shared = custom_tick_launch(w.env, w.env.TICK_KERNEL, w.env.TICK_STEP_ARGS, sampler, tensors,
                                                       w.env_resetter, ticks=10)
    assert block == ((N + 63) // 64 * 64, 1, 1) and tuple(grid)[0] == E
    args = list(args)
    args[0], args[1] = fenced["counts"][pad:pad + n], fenced["actions"][pad:pad + n]
    fn(*args, block=block, grid=grid, shared=shared)
    drv.synchronize()
    total = np.zeros((E, N, H), dtype=np.int32)
    for _ in range(10):
        actions = draws.draw(probs)
        total += actions + 1
    got = {k: v.cpu().numpy() for k, v in fenced.items()}
    for k, want in (("counts", total), ("actions", actions)):
        assert (got[k][:pad] == SENTINEL).all() and (got[k][pad + n:] == SENTINEL).all(), f"the fence around {k}"
        _same_bits(got[k][pad:pad + n].reshape(E, N, H), want, f"fenced {k}")
    assert (_rng_words(w, sampler)[4:] == 20).all()


# ----------------------------------------------------------------------------------------------------- engine shape
def test_engine_shape_and_the_fallback_with_a_reset_pool():
    from tests.hip_harness import pull
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.rollout import RolloutEngine
    from warp_drive_amd.utils.data_feed import DataFeed

    config = dict(num_agents=5, grid_length=4, episode_length=6, seed=2)
    w, sampler = _wrapper(config, 3, 5)
    engine = RolloutEngine(w, sampler)
    assert engine.fused and engine.entry_names == [TICK] and len(engine.plan) == 1
    assert engine.step_kernel_name == TICK and engine.rollout_kernel_name == TICK and engine.cohorts == 1
    assert w.cuda_function_manager.has_function(TICK) and w.env.cuda_step.name == STEP
    plain = RolloutEngine(w, sampler, fused=False)
    assert not plain.fused and plain.entry_names == ["sample_actions[0]", STEP, "reset_when_done_fused"]

    class Pooled(fused_module().RendezvousFused):
        """the same class with one more array that restarts from a pool: nothing the fused tick knows how to do"""

        def get_data_dictionary(self):
            feed = super().get_data_dictionary()
            feed.add_data(name="mood", data=np.zeros(self.num_agents, dtype=np.int32))
            return feed

        def get_reset_pool_dictionary(self):
            pool = DataFeed()
            pool.add_pool_for_reset(name="mood_reset_pool", reset_target="mood",
                                    data=np.arange(4 * self.num_agents, dtype=np.int32).reshape(4, self.num_agents))
            return pool

    assert Pooled.name == "RendezvousFused"
    wp, sp = _wrapper(config, 3, 5, registrar=_fused_registrar(Pooled))
    wp.init_reset_pool(seed=7)
    pooled = RolloutEngine(wp, sp)
    assert not pooled.fused and pooled.rollout_kernel_name is None
    assert pooled.entry_names == ["sample_actions[0]", STEP, "reset_when_done_fused", "reset_when_done_from_pool",
                                  "undo_done_flag_and_reset_timestep"]
    pooled.run(7)  # past the time limit: the per-tick plan restarts the replicas, the pooled array included
    drv.synchronize()
    assert (pull(wp, "_timestep_") == 1).all() and (pull(wp, "_done_") == 0).all()
    mood = pull(wp, "mood")
    assert all(row.tolist() in np.arange(20).reshape(4, 5).tolist() for row in mood)


# ---------------------------------------------------------------------------------------------------------- Trainer
def test_trainer_drives_the_fused_example(tmp_path):
    import torch

    from warp_drive_amd.training.trainer import Trainer

    E, N, T = 4, 5, 12
    w = _wrapper(dict(num_agents=N, grid_length=6, episode_length=T, seed=9), E, None, reset=False)
    config = {"name": "rendezvous_fused",
              "trainer": {"num_envs": E, "train_batch_size": E * 6, "num_episodes": 100, "seed": 5},
              "policy": {"shared": {"to_train": True, "algorithm": "A2C", "lr": 0.01, "vf_loss_coeff": 1, "gamma": 0.98,
                                    "model": {"type": "fully_connected", "fc_dims": [32, 32]}}},
              "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0, "basedir": str(tmp_path),
                         "name": "rendezvous_fused", "tag": "test"}}
    trainer = Trainer(env_wrapper=w, config=config, policy_tag_to_agent_id_map={"shared": list(range(N))},
                      results_dir=str(tmp_path), verbose=False)
    assert trainer.engine.fused and trainer.engine.entry_names == [TICK]
    assert trainer.rollout_path == "per tick" and trainer.update_path == {"shared": "framework"}
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


# ------------------------------------------------------------------------------------------ TagContinuous unchanged
def test_tag_continuous_takes_the_path_it_took(monkeypatch):
    """E = 33 of tests/test_gpu_tick_rollout.py's sizes.  The values are the parent commit's, read off its rollout.py:
    cohort_bounds(33, 2) is [(0, 32), (32, 33)], one replica per block, and a cohort of 32 blocks covers fewer than half of
    the compute units, so _add_cohorts adds none (`cohorts` stays 1); the multi-tick entry is attached all the same."""
    from tests.test_gpu_tick_cohorts import CFG
    from tests.hip_harness import require_gpu
    from warp_drive_amd import rollout
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.envs.tag_continuous import TagContinuous
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

    require_gpu()
    monkeypatch.setattr(rollout, "TICK_COHORTS", 2)
    monkeypatch.setattr(rollout, "TICK_ROLLOUT", 1)
    w = EnvWrapper(env_obj=TagContinuous(**CFG), num_envs=33, env_backend="hip")
    w.reset_all_envs()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=4242)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    engine = rollout.RolloutEngine(w, sampler)
    assert engine.entry_names == ["HipTagContinuousTick_K10_N105A21"] and engine.fused
    assert engine.rollout_kernel_name == "HipTagContinuousRollout_K10_N105A21"
    assert engine.cohorts == 1 and engine.plan.cohorts == 1 and len(engine.plan) == 1
    monkeypatch.setattr(rollout, "TICK_ROLLOUT", 0)
    off = rollout.RolloutEngine(w, sampler)
    assert off.rollout_kernel_name is None and off.cohorts == 1
