"""ClassicControl Acrobot / MountainCar / ContinuousMountainCar / Pendulum on the MI355X: the step kernels against the
numpy steps (envs/classic_control.py) and against the reference's kernel sources (tests/golden/cc_<env>_traj.npz), the
fused tick against the step + reset kernels with the draws replayed, the reset pool in the rollout plan, and the trainer
on the two pooled configs."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ENVS = ("acrobot", "mountain_car", "continuous_mountain_car", "pendulum")


def _spec(env):
    from warp_drive_amd.envs import classic_control as cc

    return {"acrobot": (cc.CUDAClassicControlAcrobotEnv, cc.acrobot_step, False),
            "mountain_car": (cc.CUDAClassicControlMountainCarEnv, cc.mountain_car_step, False),
            "continuous_mountain_car": (cc.CUDAClassicControlContinuousMountainCarEnv,
                                        cc.continuous_mountain_car_step, True),
            "pendulum": (cc.CUDAClassicControlPendulumEnv, cc.pendulum_step, True)}[env]


def _push(w, name, arr):
    t = w.cuda_data_manager.data_on_device_via_torch(name)
    t.copy_(torch.from_numpy(np.ascontiguousarray(arr)).reshape(t.shape).to(t.device))


def _push_raw(w, name, arr):
    from warp_drive_amd.managers import hip_driver as drv

    drv.memcpy_htod(w.cuda_data_manager.device_data(name), np.ascontiguousarray(arr))


def _words(ptr, n):
    from warp_drive_amd.managers import hip_driver as drv

    out = np.zeros(4 + n, dtype=np.uint32)
    drv.memcpy_dtoh(out, ptr)
    torch.cuda.synchronize()
    return out


def _pool_pick(words, envs, n_pool):
    """the pool row reset_when_done_from_pool draws for each replica in `envs` (host replay of its Philox draw,
    oracle/core_np.py::pool_pick, from the device's own header and epoch words)"""
    from oracle.core_np import pool_pick

    return pool_pick(envs, words[4 + envs], words[0], words[1], n_pool)


def _spread_states(env, rng, E):
    lo, hi = {"acrobot": ([-3.1, -3.1, -12.0, -28.0], [3.1, 3.1, 12.0, 28.0]),
              "mountain_car": ([-1.2, -0.07], [0.58, 0.07]), "continuous_mountain_car": ([-1.2, -0.07], [0.5, 0.07]),
              "pendulum": ([-3.1, -8.0], [3.1, 8.0])}[env]
    return rng.uniform(lo, hi, size=(E, 1, len(lo))).astype(np.float32)


def _actions(rng, E, cont):
    if cont:  # values outside the clip range included
        return rng.uniform(-3.0, 3.0, size=(E, 1, 1)).astype(np.float32)
    return rng.randint(0, 3, size=(E, 1, 1)).astype(np.int32)


def _count_ulp(a, b):
    from tests.hip_harness import ulp_diff

    d = ulp_diff(a, b)
    assert d.max(initial=0) <= 1, int(d.max())
    return int((d.reshape(len(d), -1) > 0).any(axis=1).sum())


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("E,n_ticks,pool", [(5000, 200, 0), (5000, 200, 64), (100000, 40, 0)])
def test_step_vs_numpy(env, E, n_ticks, pool):
    """Each tick: the numpy step on the device's own pre-step state (Acrobot is chaotic: a float64 cos that differs in its
    last bit must not grow); float outputs within 1 float32 ulp (rows counted and printed), float32-only outputs
    (Acrobot's observation, reward and terminal test of the device state) bit-exact, discrete outputs exact; through
    terminations, time-outs and restarts from the fixed start or from a pool."""
    from tests.hip_harness import OBS, REW, make_wrapper, pull, require_gpu
    from warp_drive_amd.envs.classic_control import acrobot_obs, apply_done

    require_gpu()
    cls, step, cont = _spec(env)
    T = 30
    w = make_wrapper(cls(episode_length=T, seed=5, reset_pool_size=pool), E)
    if pool:
        w.init_reset_pool(seed=17)
        pool_states = pull(w, "state_reset_pool")[:, 0]
    start = pull(w, "state")[0, 0].copy()
    rng = np.random.RandomState(1)
    _push_raw(w, "state", _spread_states(env, rng, E))  # first episodes from all over the state space: terminal states
    ulp_rows = restarts = terminal = 0
    for t in range(n_ticks):
        s0, ts0 = pull(w, "state")[:, 0].copy(), pull(w, "_timestep_").copy()
        a = _actions(rng, E, cont)
        _push(w, "sampled_actions", a)
        w.step_all_envs()
        st, ob, rw, dn = pull(w, "state")[:, 0], pull(w, OBS)[:, 0], pull(w, REW)[:, 0], pull(w, "_done_")
        es, eo, er, term = step(s0, a.reshape(-1))
        np.testing.assert_array_equal(pull(w, "_timestep_"), ts0 + 1)
        np.testing.assert_array_equal(dn, apply_done(term, ts0 + 1, T), err_msg=f"t={t}")
        ulp_rows += _count_ulp(st, es) + _count_ulp(ob, eo) + _count_ulp(rw, er)
        if env == "acrobot":  # float32 flow from the device's own state: bit for bit
            np.testing.assert_array_equal(ob, acrobot_obs(st))
            c = np.ascontiguousarray
            term_dev = (-np.cos(c(st[:, 0])) - np.cos(c(st[:, 1] + st[:, 0]))) > np.float32(1.0)
            np.testing.assert_array_equal(rw, np.where(term_dev, 0.0, -1.0).astype(np.float32))
            np.testing.assert_array_equal(dn, apply_done(term_dev.astype(np.int32), ts0 + 1, T))
        if env == "mountain_car":
            np.testing.assert_array_equal(rw, -1.0)
        fin = np.flatnonzero(dn > 0)
        words = _words(w.env_resetter._pool_rng, E) if pool else None
        w.reset_only_done_envs()
        s1 = pull(w, "state")[:, 0]
        if pool:
            pick = _pool_pick(words, fin, pool_states.shape[0])
            np.testing.assert_array_equal(s1[fin], pool_states[pick])
            after = _words(w.env_resetter._pool_rng, E)
            np.testing.assert_array_equal(after[4:] - words[4:], (dn > 0).astype(np.uint32))
        else:
            np.testing.assert_array_equal(s1[fin], np.broadcast_to(start, s1[fin].shape))
        restarts += len(fin)
        terminal += int(((dn > 0) & (ts0 + 1 < T)).sum())
    print(f"{env} E={E} pool={pool}: {ulp_rows} rows 1 ulp apart (float64 flow), {restarts} restarts, "
          f"{terminal} terminal")
    assert restarts > E // 2 and (terminal > 0 or env == "pendulum")


@pytest.mark.parametrize("env", ENVS)
def test_step_vs_reference_kernel_source(env):
    """The device step replays tests/golden/cc_<env>_traj.npz tick by tick (each tick starts from the fixture's recorded
    state and timestep): floats within 1e-5 abs, discrete exact (MountainCar's done == 2 included)."""
    from tests.hip_harness import OBS, REW, make_wrapper, pull, require_gpu

    require_gpu()
    cls, _, cont = _spec(env)
    g = np.load(os.path.join(GOLDEN, f"cc_{env}_traj.npz"))
    ticks, E = g["actions"].shape[:2]
    w = make_wrapper(cls(episode_length=int(g["episode_length"]), seed=1), E)
    for t in range(ticks):
        _push_raw(w, "state", g["state_in"][t].astype(np.float32))
        _push_raw(w, "_timestep_", g["timestep_in"][t].astype(np.int32))
        _push_raw(w, "_done_", np.zeros(E, np.int32))
        _push(w, "sampled_actions", g["actions"][t].astype(np.float32 if cont else np.int32))
        w.step_all_envs()
        np.testing.assert_allclose(pull(w, "state")[:, 0], g["state"][t], rtol=0, atol=1e-5, err_msg=f"t={t}")
        np.testing.assert_allclose(pull(w, OBS)[:, 0], g["obs"][t], rtol=0, atol=1e-5, err_msg=f"t={t}")
        np.testing.assert_allclose(pull(w, REW)[:, 0], g["rewards"][t], rtol=0, atol=1e-5, err_msg=f"t={t}")
        np.testing.assert_array_equal(pull(w, "_done_"), g["done"][t], err_msg=f"t={t}")
        np.testing.assert_array_equal(pull(w, "_timestep_"), g["timestep"][t])


def _ou_actions(w, sampler, words, ou, probs, ticks, damping=0.15, stddev=0.2, scale=1.0):
    """what `ticks` sample_ou_process launches with the tick's stream tag draw on copies of the RNG words and OU state"""
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.managers.function_manager import _stream_tag

    E = probs.shape[0]
    rng_copy = drv.mem_alloc(words.nbytes)
    drv.memcpy_htod(rng_copy, words)
    ou_copy = torch.from_numpy(ou.copy()).cuda()
    out = []
    try:
        for _ in range(ticks):
            act = torch.zeros(E, dtype=torch.float32, device="cuda")
            sampler.sample_ou_process(rng_copy, probs, act, ou_copy, np.float32(damping), np.float32(stddev),
                                      np.float32(scale), np.int32(E), _stream_tag("tick"), block=(256, 1, 1),
                                      grid=(max(1, min(4096, (E + 255) // 256)), 1))
            torch.cuda.synchronize()
            out.append(act.cpu().numpy())
    finally:
        rng_copy.free()
    return out


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("ticks,batch,pool", [(1, False, 0), (8, False, 0), (8, False, 16), (8, True, 16)])
def test_fused_tick(env, ticks, batch, pool):
    """HipClassicControl<X>EnvTick through the RolloutEngine (one entry, fused) against a second wrapper driven by the
    step kernel and reset_when_done with the tick's draws replayed: discrete actions from the host's Philox replay
    (single_head_tick_uniform + the counting sampler), continuous ones from direct sample_ou_process launches on copies
    of the RNG words and OU state.  State, observation, reward, done, timestep and the RNG words match exactly; with a
    pool every restart is the row the host replay of the pool key picks; with the batch tensors row k is tick k."""
    from oracle.core_np import sample_actions_counting, single_head_tick_uniform
    from tests.hip_harness import OBS, REW, make_wrapper, pull, require_gpu
    from warp_drive_amd.managers.function_manager import HIPSampler, _stream_tag
    from warp_drive_amd.rollout import RolloutEngine

    require_gpu()
    cls, _, cont = _spec(env)
    E, T = 3001, 20
    wa = make_wrapper(cls(episode_length=T, seed=5, reset_pool_size=pool), E)
    wb = make_wrapper(cls(episode_length=T, seed=5, reset_pool_size=pool), E)
    if pool:
        wa.init_reset_pool(seed=23)
        wb.init_reset_pool(seed=23)
        pool_states = pull(wa, "state_reset_pool")[:, 0]
    sampler = HIPSampler(wa.cuda_function_manager)
    sampler.init_random(seed=9)
    if cont:
        wa.cuda_data_manager.push_data_to_device(_ou_feed(E))
    rng = np.random.RandomState(2)
    if cont:
        probs = torch.from_numpy(rng.uniform(-1.5, 1.5, size=(E, 1, 1)).astype(np.float32)).cuda()
    else:
        probs = torch.from_numpy(rng.dirichlet(np.ones(3), size=(E, 1)).astype(np.float32)).cuda()
    rb = None
    if batch:
        O = int(pull(wa, OBS).shape[-1])
        rb = {"obs": torch.zeros((ticks, E, 1, O), dtype=torch.float32, device="cuda"),
              "actions": torch.zeros((ticks, E, 1, 1), dtype=torch.float32 if cont else torch.int32, device="cuda"),
              "rewards": torch.zeros((ticks, E, 1), dtype=torch.float32, device="cuda"),
              "done": torch.zeros((ticks, E), dtype=torch.int32, device="cuda")}
    engine = RolloutEngine(wa, sampler, probabilities=[probs], ticks_per_launch=ticks, rollout_batch=rb)
    assert engine.fused and engine.ticks_per_launch == ticks and len(engine.entry_names) == 1
    assert engine.entry_names[0].endswith("EnvTick")
    probs_host = probs.cpu().numpy()
    restarts = 0
    for launch in range(6 if ticks > 1 else 45):
        words = _words(sampler.rng_state, E)
        if cont:
            ou = pull(wa, "sampled_actions_ou_state").reshape(-1).astype(np.float32)
            acts = _ou_actions(wa, sampler, words, ou, probs.reshape(-1), ticks)
        else:
            assert (words[4:] == launch * ticks).all()
        engine.run(1)
        torch.cuda.synchronize()
        for k in range(ticks):
            if cont:
                a = acts[k].reshape(E, 1, 1)
            else:
                u = single_head_tick_uniform(E, words[4:] + np.uint32(k), words[0], words[1], _stream_tag("tick"))
                a = sample_actions_counting(probs_host, u.reshape(E, 1)).reshape(E, 1, 1).astype(np.int32)
            obs_before = pull(wb, OBS).copy()
            _push(wb, "sampled_actions", a)
            wb.step_all_envs()
            done_k, rew_k = pull(wb, "_done_").copy(), pull(wb, REW).copy()
            if batch:
                np.testing.assert_array_equal(rb["obs"][k].cpu().numpy(), obs_before)
                np.testing.assert_array_equal(rb["actions"][k].cpu().numpy().reshape(-1), a.reshape(-1))
                np.testing.assert_array_equal(rb["rewards"][k].cpu().numpy(), rew_k)
                np.testing.assert_array_equal(rb["done"][k].cpu().numpy(), done_k)
            fin = np.flatnonzero(done_k > 0)
            pw = _words(wb.env_resetter._pool_rng, E) if pool else None
            if k == ticks - 1:
                np.testing.assert_array_equal(pull(wa, "sampled_actions").reshape(-1), a.reshape(-1))
                np.testing.assert_array_equal(pull(wa, "_done_"), done_k)
                np.testing.assert_array_equal(pull(wa, REW), rew_k)
            wb.reset_only_done_envs()
            if pool:
                pick = _pool_pick(pw, fin, pool_states.shape[0])
                np.testing.assert_array_equal(pull(wb, "state")[fin, 0], pool_states[pick])
            restarts += len(fin)
        np.testing.assert_array_equal(pull(wa, "state"), pull(wb, "state"), err_msg=f"launch {launch}")
        np.testing.assert_array_equal(pull(wa, OBS), pull(wb, OBS))
        np.testing.assert_array_equal(pull(wa, "_timestep_"), pull(wb, "_timestep_"))
        if pool:
            np.testing.assert_array_equal(_words(wa.env_resetter._pool_rng, E), _words(wb.env_resetter._pool_rng, E))
        if cont:
            np.testing.assert_array_equal(_words(sampler.rng_state, E)[4:], words[4:] + np.uint32(ticks))
    assert restarts > E // 2


def _ou_feed(E):
    from warp_drive_amd.utils.data_feed import DataFeed

    f = DataFeed()
    f.add_data(name="sampled_actions_ou_state", data=np.zeros((E, 1, 1), np.float32))
    return f


@pytest.mark.parametrize("env", ["continuous_mountain_car", "pendulum"])
def test_box_actions_unfused_plan(env):
    """The unfused plan of a Box env: sample_ou_process (HIPSampler.sample's stream tag and defaults), step, reset --
    the actions equal a direct HIPSampler.sample on copies, and the env arrays equal a step_all_envs of those actions."""
    from tests.hip_harness import OBS, make_wrapper, pull, require_gpu
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.rollout import RolloutEngine

    require_gpu()
    cls, _, _ = _spec(env)
    E = 2048
    wa = make_wrapper(cls(episode_length=15, seed=5), E)
    wb = make_wrapper(cls(episode_length=15, seed=5), E)
    sa, sb = HIPSampler(wa.cuda_function_manager), HIPSampler(wb.cuda_function_manager)
    sa.init_random(seed=3)
    sb.init_random(seed=3)
    wa.cuda_data_manager.push_data_to_device(_ou_feed(E))
    wb.cuda_data_manager.push_data_to_device(_ou_feed(E))
    means = torch.from_numpy(np.random.RandomState(4).uniform(-1, 1, size=(E, 1, 1)).astype(np.float32)).cuda()
    engine = RolloutEngine(wa, sa, probabilities=[means], fused=False)
    assert not engine.fused and engine.entry_names[0] == "sample_ou_process"
    for t in range(40):
        engine.run(1)
        sb.sample(wb.cuda_data_manager, means, "sampled_actions")
        wb.step_all_envs()
        wb.reset_only_done_envs()
        torch.cuda.synchronize()
        for name in ("sampled_actions", "sampled_actions_ou_state", "state", OBS, "_timestep_", "_done_"):
            np.testing.assert_array_equal(pull(wa, name), pull(wb, name), err_msg=f"{name} t={t}")


def test_cartpole_pool_reset_in_rollout_plan():
    """A RolloutEngine run of Cartpole with a reset pool restarts every finished replica at the pool row the host replay
    of reset_when_done_from_pool's key picks (the plan used to restore only the arrays with a saved copy: the state kept
    its terminal value)."""
    from tests.hip_harness import make_wrapper, pull, require_gpu
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.rollout import RolloutEngine

    require_gpu()
    E = 2000
    w = make_wrapper(CUDAClassicControlCartPoleEnv(episode_length=25, seed=5, reset_pool_size=8), E)
    w.init_reset_pool(seed=31)
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=4)
    engine = RolloutEngine(w, sampler)
    assert not engine.fused and "reset_when_done_from_pool" in engine.entry_names
    pool_states = pull(w, "state_reset_pool")[:, 0]
    restarts = 0
    for t in range(60):
        words = _words(w.env_resetter._pool_rng, E)
        engine.run(1)
        torch.cuda.synchronize()
        fin = np.flatnonzero(pull(w, "_timestep_") == 0)
        pick = _pool_pick(words, fin, 8)
        np.testing.assert_array_equal(pull(w, "state")[fin, 0], pool_states[pick], err_msg=f"t={t}")
        np.testing.assert_array_equal(pull(w, "_done_"), 0)
        restarts += len(fin)
    assert restarts > E


@pytest.mark.parametrize("name", ["single_acrobot", "single_mountain_car"])
def test_trainer_on_pooled_configs(name, tmp_path):
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    ov = {"trainer": {"num_envs": 200, "train_batch_size": 200 * 20, "num_episodes": 1000, "seed": 3},
          "env": {"episode_length": 60, "reset_pool_size": 50}, "saving": {"metrics_log_freq": 1}}
    torch.manual_seed(0)
    tr = setup_trainer(name, ov, results_dir=str(tmp_path), verbose=False)
    assert tr.w.env_resetter._random_initialized
    metrics = tr.train(3)
    tr.graceful_close()
    for pol in metrics:
        assert np.isfinite(metrics[pol]["Total loss"])


def test_acrobot_learns(tmp_path):
    """A2C on run_configs/single_acrobot.yaml's [32, 32] policy (1000 replicas, 50-tick batches, 200-tick episodes, the
    config's reset pool): the mean episodic reward is minus the mean episode length, -200 while the tip never swings up.
    scripts/learning_curves.py (profiles/acrobot_learning_curve.txt) reaches -85 after 1500 iterations (~9 s); the bar
    here is -150 over the last 100 iterations, with every restart drawn from the pool by the fused tick."""
    import json

    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    ov = {"trainer": {"num_envs": 1000, "train_batch_size": 1000 * 50, "num_episodes": 10 ** 6, "seed": 7},
          "env": {"episode_length": 200, "seed": 11}, "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0}}
    torch.manual_seed(0)
    tr = setup_trainer("single_acrobot", ov, results_dir=str(tmp_path), verbose=False)
    assert tr.engine.fused and tr.w.env_resetter._random_initialized
    tr.train(1500)
    tr.graceful_close()
    curve = np.array([json.loads(line)["shared"]["Mean episodic reward"] for line in open(tmp_path / "results.json")])
    first, last = np.nanmean(curve[:100]), np.nanmean(curve[-100:])
    print(f"acrobot: mean episodic reward {first:.1f} -> {last:.1f}")
    assert first < -180 and last > -150
