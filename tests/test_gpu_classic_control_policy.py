"""HipClassicControl<Acrobot|MountainCar>EnvRollout_H<32|64> on the MI355X: a batch of ticks in one launch with the policy
network evaluated by the kernel on every tick's observation -- against the step + reset kernels with the recorded actions
replayed, the host restatement of the network (tests/classic_control_policy.py) and the host's Philox replay; and the
trainer on the one-launch path these entries open (`trainer.fused_rollout_policy: "all"`)."""
import json

import numpy as np
import pytest
import torch

from tests import classic_control_policy as ccp

pytestmark = pytest.mark.gpu

ENTRY = {"acrobot": "HipClassicControlAcrobotEnv", "mountain_car": "HipClassicControlMountainCarEnv"}


def _words(ptr, n):
    from warp_drive_amd.managers import hip_driver as drv

    out = np.zeros(4 + n, dtype=np.uint32)
    drv.memcpy_dtoh(out, ptr)
    torch.cuda.synchronize()
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("env", ["acrobot", "mountain_car"])
@pytest.mark.parametrize("hidden", [32, 64])
@pytest.mark.parametrize("pool", [0, 16])
def test_rollout_with_the_policy_inside_the_kernel(env, hidden, pool):
    """E = 1501, episodes of 23 ticks, 12 ticks per launch, 5 launches, batch tensors pre-filled with 7.0 / -1.  A second
    wrapper is driven by the step kernel and reset_when_done with the device's recorded action replayed tick by tick (the
    numpy step may differ from the device's by an ulp: the step kernel is the yardstick).  At tolerance 0: row k of obs /
    rewards / done, the final state, the observation, `_timestep_`, the sampler's RNG words and the pool's; every pool
    restart is the row oracle.core_np.pool_pick names.  The recorded action is the number of host running sums (the
    restated network on the second wrapper's observation) below the host's Philox uniform, except where the uniform lies
    within 2e-6 of one of the two thresholds (device expf against numpy's): the replay then follows the device; such draws
    are capped at 2 + draws // 50000.  T single-tick launches of the same entry record the same rows, byte for byte."""
    from oracle.core_np import pool_pick, single_head_tick_uniform
    from tests.hip_harness import OBS, REW, make_wrapper, pull, require_gpu
    from warp_drive_amd.managers.function_manager import HIPSampler, _stream_tag
    from warp_drive_amd.rollout import RolloutEngine
    from warp_drive_amd.training.policy_kernel import rollout_policy_width

    require_gpu()
    c = ccp.PARITY
    E, T, ticks, launches = c["E"], c["episode_length"], c["ticks"], c["launches"]
    cls, O = ccp.device_class(env), ccp.OBS_SIZE[env]
    model, packed_host = ccp.make_policy(env, hidden)
    assert rollout_policy_width(model, O, cls.ROLLOUT_POLICY_WIDTHS) == hidden
    assert packed_host.numel() == ccp.policy_weight_count(O, hidden, 3)
    packed = packed_host.cuda()
    packed_np = packed_host.numpy()

    def wrapper():
        w = make_wrapper(cls(episode_length=T, seed=c["env_seed"], reset_pool_size=pool), E)
        if pool:
            w.init_reset_pool(seed=c["pool_seed"])
        return w

    def make(tpl):
        w = wrapper()
        sampler = HIPSampler(w.cuda_function_manager)
        sampler.init_random(seed=c["sampler_seed"])
        probs = torch.full((E, 1, 3), 1.0 / 3.0, device="cuda")  # (not read: the kernel evaluates the policy)
        batch = {"obs": torch.full((tpl, E, 1, O), 7.0, device="cuda"),
                 "actions": torch.full((tpl, E, 1, 1), -1, dtype=torch.int32, device="cuda"),
                 "rewards": torch.full((tpl, E, 1), 7.0, device="cuda"),
                 "done": torch.full((tpl, E), -1, dtype=torch.int32, device="cuda")}
        eng = RolloutEngine(w, sampler, probabilities=[probs], rollout_batch=batch, rollout_policy=(packed, hidden),
                            ticks_per_launch=tpl)
        assert eng.fused and eng.ticks_per_launch == tpl and eng.entry_names == [f"{ENTRY[env]}Rollout_H{hidden}"]
        assert eng.step_kernel_name == f"{ENTRY[env]}Rollout_H{hidden}"
        return w, sampler, batch, eng

    wa, sampler, batch, eng = make(ticks)
    w1, sampler1, batch1, eng1 = make(1)
    wb = wrapper()
    pool_states = pull(wa, "state_reset_pool")[:, 0] if pool else None
    start = pull(wa, "state")[0, 0].copy()
    tag = _stream_tag("tick")
    near = draws = finished = 0
    counts, rows_drawn = np.zeros(3, np.int64), set()
    for launch in range(launches):
        words = _words(sampler.rng_state, E)
        assert (words[4:] == launch * ticks).all()
        eng.run(1)
        torch.cuda.synchronize()
        b = {k: v.cpu().numpy() for k, v in batch.items()}
        for k in range(ticks):
            eng1.run(1)  # the same tick as its own launch
            torch.cuda.synchronize()
            for key in b:
                np.testing.assert_array_equal(_bits(batch1[key][0].cpu().numpy()), _bits(b[key][k]),
                                              err_msg=f"{key} row {k} of launch {launch}")
            obs_before = pull(wb, OBS)[:, 0].copy()
            np.testing.assert_array_equal(_bits(b["obs"][k, :, 0]), _bits(obs_before), err_msg=f"obs row {k} of launch {launch}")
            cum = ccp.running_sums(ccp.policy_probabilities(packed_np, hidden, obs_before, 3))
            u = single_head_tick_uniform(E, words[4:] + np.uint32(k), words[0], words[1], tag)
            want = ccp.count_below(cum, u)
            got = b["actions"][k, :, 0, 0]
            assert got.min() >= 0 and got.max() <= 2
            bad = got != want
            gap = np.abs(cum[bad, :2] - u[bad, None]).min(axis=1) if bad.any() else np.zeros(0, np.float32)
            assert (gap < 2e-6).all(), (launch, k, cum[bad], u[bad], got[bad], want[bad])
            near += int(bad.sum())
            draws += E
            counts += np.bincount(got, minlength=3)
            # ---- the replay follows the device's action: step kernel + reset_when_done on the second wrapper
            t = wb.cuda_data_manager.data_on_device_via_torch("sampled_actions")
            t.copy_(torch.from_numpy(got.astype(np.int32)).reshape(t.shape).to(t.device))
            wb.step_all_envs()
            done_k, rew_k = pull(wb, "_done_").copy(), pull(wb, REW).copy()
            np.testing.assert_array_equal(_bits(b["rewards"][k]), _bits(rew_k), err_msg=f"rewards row {k} of launch {launch}")
            np.testing.assert_array_equal(b["done"][k], done_k, err_msg=f"done row {k} of launch {launch}")
            if k == ticks - 1:  # the per-tick arrays report the launch's last tick
                np.testing.assert_array_equal(pull(wa, "sampled_actions").reshape(-1), got)
                np.testing.assert_array_equal(pull(wa, "_done_"), done_k)
                np.testing.assert_array_equal(_bits(pull(wa, REW)), _bits(rew_k))
            fin = np.flatnonzero(done_k > 0)
            finished += len(fin)
            pw = _words(wb.env_resetter._pool_rng, E) if pool else None
            wb.reset_only_done_envs()
            s1 = pull(wb, "state")[:, 0]
            if pool:
                pick = pool_pick(fin, pw[4 + fin], pw[0], pw[1], pool)
                np.testing.assert_array_equal(_bits(s1[fin]), _bits(pool_states[pick]))
                rows_drawn.update(int(r) for r in pick)
            else:
                np.testing.assert_array_equal(_bits(s1[fin]), _bits(np.broadcast_to(start, s1[fin].shape)))
        for w in (wa, w1):
            np.testing.assert_array_equal(_bits(pull(w, "state")), _bits(pull(wb, "state")), err_msg=f"launch {launch}")
            np.testing.assert_array_equal(_bits(pull(w, OBS)), _bits(pull(wb, OBS)), err_msg=f"launch {launch}")
            np.testing.assert_array_equal(pull(w, "_timestep_"), pull(wb, "_timestep_"), err_msg=f"launch {launch}")
            if pool:
                np.testing.assert_array_equal(_words(w.env_resetter._pool_rng, E), _words(wb.env_resetter._pool_rng, E))
        after = _words(sampler.rng_state, E)
        np.testing.assert_array_equal(after[:4], words[:4])
        np.testing.assert_array_equal(after[4:], words[4:] + np.uint32(ticks))
        np.testing.assert_array_equal(_words(sampler1.rng_state, E), after)
    frac = counts / draws
    print(f"{env} H={hidden} pool={pool}: {draws} draws, {near} within 2e-6 of a threshold, {finished} finished episodes, "
          f"action shares {np.round(frac, 3)}, {len(rows_drawn)} pool rows drawn")
    assert draws == 90060 and near <= 2 + draws // 50000, near
    assert finished >= 2 * E and (frac >= 0.05).all(), (finished, frac)
    assert not pool or len(rows_drawn) >= 8


def _overrides(extra_trainer=None):
    ov = {"trainer": {"num_envs": 200, "train_batch_size": 200 * 20, "num_episodes": 1000, "seed": 3},
          "env": {"episode_length": 60, "reset_pool_size": 50}, "saving": {"metrics_log_freq": 1}}
    ov["trainer"].update(extra_trainer or {})
    return ov


@pytest.mark.parametrize("name", ["single_acrobot", "single_mountain_car"])
def test_trainer_takes_the_one_launch_path_when_asked(name, tmp_path):
    """the sizes of test_trainer_on_pooled_configs with `fused_rollout_policy: "all"`: the engine is the Rollout_H32
    entry, the whole batch is one launch, three iterations give finite losses"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    torch.manual_seed(0)
    tr = setup_trainer(name, _overrides({"fused_rollout_policy": "all"}), results_dir=str(tmp_path), verbose=False)
    env = "acrobot" if name == "single_acrobot" else "mountain_car"
    assert tr.engine.step_kernel_name == f"{ENTRY[env]}Rollout_H32"
    assert tr._batch_rollout is not None and tr.w.env_resetter._random_initialized
    metrics = tr.train(3)
    tr.graceful_close()
    assert metrics
    for pol in metrics:
        assert np.isfinite(metrics[pol]["Total loss"])


@pytest.mark.parametrize("name", ["single_acrobot", "single_mountain_car"])
@pytest.mark.parametrize("value", [None, True])
def test_trainer_keeps_the_per_tick_path_by_default(name, value, tmp_path):
    """without the key (and with its default, True) the shipped behaviour: the fixed-probability tick, one launch per tick"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    torch.manual_seed(0)
    tr = setup_trainer(name, _overrides({} if value is None else {"fused_rollout_policy": value}),
                       results_dir=str(tmp_path), verbose=False)
    assert tr.engine.step_kernel_name.endswith("EnvTick") and tr._batch_rollout is None
    tr.graceful_close()


def test_batch_bookkeeping_with_goal_flags_and_a_pool(tmp_path):
    """What the one-launch path reads from the recorded rows, with done == 2 (MountainCar's goal) and a reset pool, neither
    of which Cartpole's batch path ever had: the done rows keep the value 2 (A2C's positive replicas are exactly those),
    and episodic reward sums / counts / the carried-over partial sums equal a tick-by-tick host loop over the rows."""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.losses import A2C
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    torch.manual_seed(0)
    tr = setup_trainer("single_mountain_car", _overrides({"fused_rollout_policy": "all"}), results_dir=str(tmp_path),
                       verbose=False)
    assert tr._batch_rollout is not None
    E, T = tr.num_envs, tr.batch_len
    # every third replica one push away from the goal: it gets there on the first tick
    from warp_drive_amd.managers import hip_driver as drv

    dm = tr.w.cuda_data_manager
    state = dm.pull_data_from_device("state").astype(np.float32)   # [E, 1, 2]
    near_goal = np.arange(E) % 3 == 0
    state[near_goal] = np.array([0.49, 0.06], np.float32)
    drv.memcpy_htod(dm.device_data("state"), np.ascontiguousarray(state))
    torch.cuda.synchronize()
    pol = tr.policies[0]
    ep_reward = np.zeros(E)
    ep_sum, ep_cnt, timed_out = np.zeros(E), np.zeros(E), False
    for it in range(4):  # 80 ticks: time-outs (60-tick episodes) as well
        tr._generate_rollout_batch()
        torch.cuda.synchronize()
        done = tr.done_batch[:T].cpu().numpy()
        rew = tr.batch[pol]["rewards"][:T, :, 0].cpu().numpy().astype(np.float64)
        assert set(np.unique(done)) <= {0, 1, 2}
        timed_out |= bool((done == 1).any())
        if it == 0:
            np.testing.assert_array_equal(done[0] == 2, near_goal)
            positives, _, _ = A2C._sample_positive_negative_env_ids(tr.done_batch[:T], 1000)
            assert set(np.flatnonzero((done == 2).any(axis=0))) == set(positives) and len(positives) >= E // 3
        for t in range(T):
            ep_reward += rew[t]
            fin = done[t] > 0
            ep_sum += ep_reward * fin
            ep_cnt += fin
            ep_reward[fin] = 0.0
        np.testing.assert_allclose(tr._ep_sum[pol].cpu().numpy(), ep_sum, rtol=1e-6)
        np.testing.assert_array_equal(tr._ep_cnt.cpu().numpy(), ep_cnt)
        np.testing.assert_allclose(tr._ep_reward[pol][:, 0].cpu().numpy(), ep_reward, rtol=1e-6)
    assert timed_out and ep_cnt.min() >= 1
    tr.graceful_close()


def test_acrobot_learns_on_the_one_launch_path(tmp_path):
    """tests/test_gpu_classic_control.py::test_acrobot_learns with `fused_rollout_policy: "all"`: the same settings and
    the same bar (first 100 iterations below -180, last 100 above -150), every batch one launch of
    HipClassicControlAcrobotEnvRollout_H32"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    ov = {"trainer": {"num_envs": 1000, "train_batch_size": 1000 * 50, "num_episodes": 10 ** 6, "seed": 7,
                      "fused_rollout_policy": "all"},
          "env": {"episode_length": 200, "seed": 11}, "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0}}
    torch.manual_seed(0)
    tr = setup_trainer("single_acrobot", ov, results_dir=str(tmp_path), verbose=False)
    assert tr._batch_rollout is not None and tr.engine.step_kernel_name == "HipClassicControlAcrobotEnvRollout_H32"
    assert tr.w.env_resetter._random_initialized
    tr.train(1500)
    tr.graceful_close()
    curve = np.array([json.loads(line)["shared"]["Mean episodic reward"] for line in open(tmp_path / "results.json")])
    first, last = np.nanmean(curve[:100]), np.nanmean(curve[-100:])
    print(f"acrobot, one launch per batch: mean episodic reward {first:.1f} -> {last:.1f}")
    assert first < -180 and last > -150
