"""A custom environment end to end on the MI355X: the example of examples/rendezvous/ is registered with its device
source, compiled on first use into a cache directory, loaded next to the in-tree code objects and driven by the
consistency checker, the custom reset, RolloutEngine's per-tick plan and Trainer.  Everything is exact: the env's state
path is integer and its float32 results are single divisions."""
import os

import numpy as np
import pytest

from tests.rendezvous_helpers import SOURCE, example_module, host_run, registrar_for, spread_limit_for

pytestmark = pytest.mark.gpu

CHECK_SEED = 11   # of the checker's action stream


@pytest.fixture(scope="module")
def env_cache(tmp_path_factory):
    """one cache directory for the module: the example compiles once (about 2 s), every later wrapper finds it"""
    path = str(tmp_path_factory.mktemp("env_cache"))
    saved = os.environ.get("WD_ENV_CACHE")
    os.environ["WD_ENV_CACHE"] = path
    yield path
    if saved is None:
        os.environ.pop("WD_ENV_CACHE", None)
    else:
        os.environ["WD_ENV_CACHE"] = saved


def _wrapper(config, num_envs, registrar=None, name="Rendezvous", sampler_seed=None):
    """(EnvWrapper by name through the registrar, reset, placeholders pushed[, sampler])"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

    require_gpu()
    w = EnvWrapper(env_name=name, env_config=config, num_envs=num_envs, env_backend="hip",
                   env_registrar=registrar or registrar_for())
    w.reset_all_envs()
    sampler = None
    if sampler_seed is not None:
        sampler = HIPSampler(w.cuda_function_manager)
        sampler.init_random(seed=sampler_seed)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    return (w, sampler) if sampler_seed is not None else w


def _host_envs(config, num_envs):
    envs = [example_module().Rendezvous(**config) for _ in range(num_envs)]
    for env in envs:
        env.reset()
    return envs


def _host_tick(envs, actions):
    """step every host replica with its row of `actions` [E, N(, 1)]; -> (obs [E, N, 5], rewards [E, N], done [E])"""
    E, N = len(envs), envs[0].num_agents
    acts = np.asarray(actions).reshape(E, N)
    outs = [envs[e].step({a: acts[e, a] for a in range(N)}) for e in range(E)]
    obs = np.stack([np.stack([o[0][a] for a in range(N)]) for o in outs])
    rew = np.array([[o[1][a] for a in range(N)] for o in outs], dtype=np.float32)
    return obs, rew, np.array([o[2]["__all__"] for o in outs])


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want, dtype=got.dtype).reshape(got.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {np.argwhere(got != want)[:5].tolist()}"


# ------------------------------------------------------------------------------------------------ the checker
@pytest.mark.parametrize("N,L", [(1, 4), (5, 4), (64, 6), (70, 6), (130, 8), (1024, 10)])
def test_consistency_checker_on_the_example(env_cache, N, L):
    """EnvironmentCPUvsGPU with the registrar, 3 replicas, 2 episodes of 12 ticks, atol = 0: observations, rewards and
    done exact.  The spread limit is the 10th percentile of the largest spread over a dry host run of the same action
    stream with the limit off, so that the checked run holds replicas that finish early AND at the time limit (one
    agent: its spread is 0 whatever it does, the limit is off and every finish is at the time limit)."""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.env_cpu_gpu_consistency_checker import EnvironmentCPUvsGPU

    require_gpu()
    E, episodes, T = 3, 2, 12
    config = dict(num_agents=N, grid_length=L, episode_length=T, seed=N, wall_penalty=0.125)
    limit = spread_limit_for(config, E, episodes * T, CHECK_SEED, percentile=10) if N > 1 else -1
    config["spread_limit"] = limit
    _, early, timed = host_run(config, E, episodes * T, CHECK_SEED)
    print(f"N = {N}, L = {L}: spread limit {limit}, {early} early and {timed} timed finishes")
    assert timed >= 1 and (early >= 1 if N > 1 else early == 0)
    checker = EnvironmentCPUvsGPU(dual_mode_env_class=example_module().Rendezvous, env_configs={"rendezvous": config},
                                  num_envs=E, num_episodes=episodes, env_registrar=registrar_for())
    checker.test_env_reset_and_step(seed=CHECK_SEED, atol=0)


# ---------------------------------------------------------------------------------------------- the path itself
def test_registered_source_is_built_loaded_and_reused(env_cache, monkeypatch):
    import subprocess

    from tests.hip_harness import require_gpu
    from warp_drive_amd import build as wd_build
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.utils.env_registrar import EnvironmentRegistrar

    require_gpu()
    config = dict(num_agents=5, grid_length=4, episode_length=6)
    w = _wrapper(config, 2)
    fm = w.cuda_function_manager
    path = fm.code_object_path_of("HipRendezvousStep")
    assert os.path.dirname(path) == env_cache and path == wd_build.env_unit_path("Rendezvous", SOURCE)
    assert fm.code_object_path_of("HipRendezvousReset") == path
    assert fm.has_function("HipRendezvousStep") and not fm.has_function("HipRendezvousTick")
    assert w.env.cuda_step.name == "HipRendezvousStep" and w.env_resetter._cuda_custom_reset.name == "HipRendezvousReset"
    # in-tree kernels are found where they were
    assert fm.code_object_path_of("reset_when_done_fused") == fm._module.path
    assert os.path.dirname(fm.code_object_path_of("HipTagContinuousStep")) == wd_build.CSRC
    # a second wrapper in the process: its own manager, its own module, no compiler run
    runs = []
    real = subprocess.run
    monkeypatch.setattr(subprocess, "run", lambda cmd, *a, **k: (runs.append(list(cmd)), real(cmd, *a, **k))[1])
    w2 = _wrapper(config, 3)
    assert runs == [] and w2.cuda_function_manager.code_object_path_of("HipRendezvousStep") == path
    assert w2.cuda_function_manager._custom_module is not fm._custom_module
    monkeypatch.undo()
    # without a registered path the wrapper fails the way an unknown kernel fails: the step function is not found
    bare = EnvironmentRegistrar()
    bare.add(env_backend=["cpu", "hip"])(example_module().Rendezvous)
    with pytest.raises(AssertionError, match="failed to initialize the HIP step function"):
        EnvWrapper(env_name="Rendezvous", env_config=config, num_envs=2, env_backend="hip", env_registrar=bare)
    # ... and a manager without a custom module knows nothing of the example
    from tests.hip_harness import make_wrapper
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorld

    plain = make_wrapper(CUDATagGridWorld(num_taggers=4, grid_length=10, episode_length=10, seed=3), 2)
    assert not plain.cuda_function_manager.has_function("HipRendezvousStep")
    assert plain.cuda_function_manager.code_object_path_of("HipRendezvousStep") is None


def test_cuda_spelled_entries_are_found(env_cache, tmp_path):
    """a source whose entries keep the reference's spelling -- Cuda<Name>Step / Cuda<Name>Reset -- registered under
    another env name (the entry names follow the env's name): it steps and resets as the example does"""
    from tests.hip_harness import ACT, OBS, REW, pull, push_actions

    ported = tmp_path / "rendezvous_port_step.cu"
    text = open(SOURCE).read()
    assert text.count("HipRendezvousStep") == 1 and text.count("HipRendezvousReset(") == 1
    ported.write_text(text.replace("HipRendezvousStep", "CudaRendezvousPortStep")
                      .replace("HipRendezvousReset", "CudaRendezvousPortReset"))
    cls = type("RendezvousPort", (example_module().Rendezvous,), {"name": "RendezvousPort"})
    config = dict(num_agents=70, grid_length=6, episode_length=9, seed=2, spread_limit=400, reset_cell=(1, 5))
    port = _wrapper(config, 4, registrar=registrar_for(cls, str(ported)), name="RendezvousPort")
    ours = _wrapper(config, 4)
    assert port.env.cuda_step.name == "CudaRendezvousPortStep" and ours.env.cuda_step.name == "HipRendezvousStep"
    assert port.env_resetter._cuda_custom_reset.name == "CudaRendezvousPortReset"
    assert os.path.basename(port.cuda_function_manager.code_object_path_of("CudaRendezvousPortStep")).startswith(
        "RendezvousPort-")
    rng = np.random.RandomState(5)
    for t in range(12):
        if t == 6:
            for w in (port, ours):
                w.custom_reset_all_envs(args=["loc_x", "loc_y", "reset_cell_x", "reset_cell_y"])
        actions = rng.randint(0, 5, (4, 70, 1))
        for w in (port, ours):
            push_actions(w, actions)
            w.step_all_envs()
        for name in ("loc_x", "loc_y", OBS, REW, "_done_", "_timestep_", ACT):
            _same_bits(pull(port, name), pull(ours, name), f"{name} at tick {t}")
        for w in (port, ours):
            w.reset_only_done_envs()


# ---------------------------------------------------------------------------------------------- constant lookup
def test_shared_constants_land_in_the_custom_module_and_in_tree_uploads_in_the_main_object(env_cache):
    from oracle.tag_gridworld_np import TagGridWorldOracle
    from tests.hip_harness import OBS, REW, make_wrapper, pull, push_actions
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorld
    from warp_drive_amd.managers import hip_driver as drv

    mod = example_module()
    config = dict(num_agents=5, grid_length=6, episode_length=6, seed=4)
    permutation = [3, 0, 4, 2, 1]
    plain = _wrapper(config, 2)
    permuted = _wrapper(dict(config, moves=[mod.DEFAULT_MOVES[p] for p in permutation]), 2)
    fm = permuted.cuda_function_manager
    assert fm.constant_module_of("kRendezvousMoves") is fm._custom_module
    assert fm.constant_module_of("kIndexToActionArr") is fm._module
    table = np.zeros(10, dtype=np.int32)
    drv.synchronize()
    drv.memcpy_dtoh(table, fm._custom_module.get_global("kRendezvousMoves")[0])
    drv.synchronize()
    assert table.reshape(5, 2).tolist() == [list(mod.DEFAULT_MOVES[p]) for p in permutation]
    # action a under the permuted table moves as action permutation[a] under the plain one, and as the host env says
    actions = np.random.RandomState(1).randint(0, 5, (2, 5, 1))
    push_actions(permuted, actions)
    push_actions(plain, np.asarray(permutation)[actions])
    permuted.step_all_envs()
    plain.step_all_envs()
    host = _host_envs(dict(config, moves=[mod.DEFAULT_MOVES[p] for p in permutation]), 2)
    obs, rew, _ = _host_tick(host, actions)
    for name, want in ((OBS, obs), (REW, rew), ("loc_x", pull(plain, "loc_x")), ("loc_y", pull(plain, "loc_y"))):
        _same_bits(pull(permuted, name), want, name)
    assert not np.array_equal(pull(permuted, "loc_x"), np.tile(host[0].starting_x, (2, 1))) or \
        not np.array_equal(pull(permuted, "loc_y"), np.tile(host[0].starting_y, (2, 1)))
    # an in-tree table uploaded through a manager WITH a custom module lands in that manager's main object
    swapped = np.array([[0, 0], [-1, 0], [1, 0], [0, -1], [0, 1]], dtype=np.int32)
    permuted.cuda_data_manager.add_shared_constants({"kIndexToActionArr": swapped})
    fm.initialize_shared_constants(permuted.cuda_data_manager, ["kIndexToActionArr"])
    back = np.zeros((5, 2), dtype=np.int32)
    drv.synchronize()
    drv.memcpy_dtoh(back, fm._module.get_global("kIndexToActionArr")[0])
    drv.synchronize()
    assert np.array_equal(back, swapped)
    # ... and TagGridWorld, on a manager of its own, steps against its oracle with the table it uploads
    cfg = dict(num_taggers=4, grid_length=10, episode_length=10, seed=3)
    w = make_wrapper(CUDATagGridWorld(**cfg), 3)
    w.cuda_data_manager.add_shared_constants({"kIndexToActionArr": w.env.step_actions})
    w.cuda_function_manager.initialize_shared_constants(w.cuda_data_manager, ["kIndexToActionArr"])
    assert w.cuda_function_manager._custom_module is None
    orc = TagGridWorldOracle(num_envs=3, **cfg)
    acts = np.random.RandomState(2).randint(0, 5, (3, 5))
    push_actions(w, acts)
    w.step_all_envs()
    orc.step(acts)
    for name, want in (("loc_x", orc.loc_x), ("loc_y", orc.loc_y), ("_done_", orc.done),
                       (OBS, orc.obs.astype(np.float32)), (REW, orc.rewards.astype(np.float32))):
        np.testing.assert_array_equal(pull(w, name), want, err_msg=name)


# ------------------------------------------------------------------------------------------------ custom reset
def test_custom_reset_puts_every_agent_on_the_cell(env_cache):
    from tests.hip_harness import OBS, REW, pull, push_actions

    config = dict(num_agents=70, grid_length=6, episode_length=9, seed=8, reset_cell=(2, 5))
    w = _wrapper(config, 3)
    w.custom_reset_all_envs(args=["loc_x", "loc_y", "reset_cell_x", "reset_cell_y"])
    assert (pull(w, "loc_x") == 2).all() and (pull(w, "loc_y") == 5).all()
    assert pull(w, "loc_x").shape == (3, 70)
    host = _host_envs(config, 3)
    for env in host:
        env.set_cells(2, 5)
    actions = np.random.RandomState(3).randint(0, 5, (3, 70, 1))
    push_actions(w, actions)
    w.step_all_envs()
    obs, rew, done = _host_tick(host, actions)
    _same_bits(pull(w, OBS), obs, "observations")
    _same_bits(pull(w, REW), rew, "rewards")
    _same_bits(pull(w, "loc_x"), np.stack([e.loc_x for e in host]), "loc_x")
    assert np.array_equal(pull(w, "_done_") > 0, done)


# --------------------------------------------------------------------------------------------- RolloutEngine
def test_rollout_engine_per_tick_plan_replays_through_the_host_env(env_cache):
    """E = 7, N = 70, 30 ticks of sampler -> HipRendezvousStep -> fused reset, one run(1) per tick: the actions read back
    each tick drive the host replicas, finished replicas restart on both sides (the plan's reset has cleared their
    flags, so a finish shows as time step 0 and the restored rows)"""
    from tests.hip_harness import ACT, OBS, REW, pull
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.rollout import RolloutEngine

    E, N, T = 7, 70, 9
    config = dict(num_agents=N, grid_length=6, episode_length=T, seed=6, wall_penalty=0.125)
    # (from the host env alone: a tenth of the ticks of a random walk lie at or below this spread, so some replicas end
    # early; which ones depends on the sampler's draws, so only the number of restarts is asserted below)
    config["spread_limit"] = spread_limit_for(config, E, 30, seed=1, percentile=10)
    w, sampler = _wrapper(config, E, sampler_seed=17)
    engine = RolloutEngine(w, sampler)
    assert not engine.fused and engine.ticks_per_launch == 1
    assert engine.entry_names == ["sample_actions[0]", "HipRendezvousStep", "reset_when_done_fused"]
    assert engine.step_kernel_name == "HipRendezvousStep"
    host = _host_envs(config, E)
    first = np.stack([np.stack([env._observation()[a] for a in range(N)]) for env in host])
    early = timed = 0
    for t in range(30):
        engine.run(1)
        drv.synchronize()
        actions = pull(w, ACT)
        assert actions.min() >= 0 and actions.max() <= 4
        obs, rew, done = _host_tick(host, actions)
        for e in np.flatnonzero(done):
            early += host[e].timestep < T
            timed += host[e].timestep == T
            host[e].reset()
            obs[e] = first[e]
        _same_bits(pull(w, REW), rew, f"rewards at tick {t}")
        _same_bits(pull(w, OBS), obs, f"observations at tick {t}")
        _same_bits(pull(w, "loc_x"), np.stack([env.loc_x for env in host]), f"loc_x at tick {t}")
        _same_bits(pull(w, "loc_y"), np.stack([env.loc_y for env in host]), f"loc_y at tick {t}")
        _same_bits(pull(w, "_timestep_"), np.array([env.timestep for env in host]), f"time steps at tick {t}")
        assert pull(w, "_done_").sum() == 0
    print(f"{early} early and {timed} timed finishes")
    assert early + timed >= E * (30 // T)   # an episode lasts at most T ticks


# ---------------------------------------------------------------------------------------------------- Trainer
def test_trainer_runs_the_example_on_the_per_tick_and_framework_paths(env_cache, tmp_path):
    import torch

    from warp_drive_amd.training.trainer import Trainer

    E, N = 8, 5
    w = _wrapper_for_trainer(dict(num_agents=N, grid_length=6, episode_length=12, seed=9), E)
    config = {"name": "rendezvous",
              "trainer": {"num_envs": E, "train_batch_size": E * 6, "num_episodes": 100, "seed": 5},
              "policy": {"shared": {"to_train": True, "algorithm": "A2C", "lr": 0.01, "vf_loss_coeff": 1, "gamma": 0.98,
                                    "model": {"type": "fully_connected", "fc_dims": [32, 32]}}},
              "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0, "basedir": str(tmp_path), "name": "rendezvous",
                         "tag": "test"}}
    trainer = Trainer(env_wrapper=w, config=config, policy_tag_to_agent_id_map={"shared": list(range(N))},
                      results_dir=str(tmp_path), verbose=False)
    assert trainer.batch_len == 6
    assert trainer.rollout_path == "per tick" and trainer.update_path == {"shared": "framework"}
    assert not trainer.engine.fused and trainer.engine.step_kernel_name == "HipRendezvousStep"
    before = [p.detach().clone() for p in trainer.models["shared"].parameters()]
    metrics = trainer.train(2)
    trainer.graceful_close()
    assert torch.isfinite(torch.tensor(metrics["shared"]["Total loss"]))
    after = list(trainer.models["shared"].parameters())
    assert any((a != b).any() for a, b in zip(before, after)) and all(torch.isfinite(p).all() for p in after)


def _wrapper_for_trainer(config, num_envs):
    """the wrapper as Trainer wants it: not reset yet, no placeholders"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.env_wrapper import EnvWrapper

    require_gpu()
    return EnvWrapper(env_name="Rendezvous", env_config=config, num_envs=num_envs, env_backend="hip",
                      env_registrar=registrar_for())
