"""Cartpole with a reset pool on the device: HipClassicControlCartPoleEnvRollout_P / _P_H32 / _P_H64
(csrc/kernels/cartpole_pool.hip) against the numpy model of tests/cartpole_pool_cases.py, bit for bit -- every case under
three launch geometries and both pool placements (staged in LDS, read from global memory) --, the entries' guard, what
RolloutEngine and the Trainer build for a pooled Cartpole, and whether it still learns.  The yardstick is
oracle/cartpole_np.py for the step and the host's Philox replay for every draw and every pool pick; tolerance 0; for the
live-policy entries the rule of tests/test_gpu_classic_control_shapes.py (a recorded action may differ from the host's
only where the uniform lies within NEAR_WINDOW of a threshold, the model follows the device's action, the count of such
draws stays under the case's cap).  `pytest -s` prints one line per case."""
import json
import os

import numpy as np
import pytest

from tests import cartpole_pool_cases as cp
from tests import classic_control_cases as cc

pytestmark = pytest.mark.gpu

F32 = np.float32
FENCE_ROWS = 2   # rows of the batch tensors behind the case's own: never written


def _shapes():
    from tests import test_gpu_classic_control_shapes as shapes   # (its plumbing: _wrapper, _put, _words, _tick_start, EQ)

    return shapes


def _device(case, placement="auto"):
    """the wrapper of a case with the case's pool rows and saved observation rows written into the device's arrays, the
    sampler, the batch tensors (FENCE_ROWS surplus rows) and the launch `tick_launch` builds"""
    import torch
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.managers.function_manager import HIPSampler

    sh = _shapes()
    w = sh._wrapper(case)
    dm, E = w.cuda_data_manager, case.E
    assert tuple(dm.get_shape("state_reset_pool")) == (case.pool, 1, 4) and sorted(dm.reset_data_list) == ["observations"]
    sh._put(w, "state_reset_pool", case.pool_rows().reshape(case.pool, 1, 4))
    drv.memcpy_htod(dm.device_data("observations_at_reset"), np.ascontiguousarray(case.saved_observations().reshape(E, 1, 4)))
    torch.cuda.synchronize()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=cc.SAMPLER_SEED)
    R = case.rows + FENCE_ROWS
    batch = {"obs": torch.full((R, E, 1, 4), 7.0, device="cuda"),
             "actions": torch.full((R, E, 1, 1), -1, dtype=torch.int32, device="cuda"),
             "rewards": torch.full((R, E, 1), 7.0, device="cuda"),
             "done": torch.full((R, E), -1, dtype=torch.int32, device="cuda")}
    if case.hidden:
        packed = torch.from_numpy(case.policy()[1]).cuda()
        probs = torch.full((E, 1, case.A), 1.0 / case.A, device="cuda")   # (not read: the kernel evaluates the policy)
    else:
        packed = None
        probs = torch.from_numpy(case.probabilities().reshape(E, 1, -1)).cuda()
    w.env.ticks_per_launch = case.ticks
    dev = dict(w=w, sampler=sampler, batch=batch, packed=packed, probs=probs, start=sh._start_arrays(w, case))
    dev["launch"] = _launch(dev, case, placement)
    return dev


def _launch(dev, case, placement):
    w = dev["w"]
    w.env.pool_placement = placement
    policy = (dev["packed"], case.hidden) if case.hidden else None
    return w.env.tick_launch(dev["sampler"], [dev["probs"]], w.env_resetter, batch=dev["batch"], policy=policy)


def _snapshot(dev, case):
    """every byte a launch may write"""
    from tests.hip_harness import ACT, OBS, REW, pull

    sh, w = _shapes(), dev["w"]
    out = {n: pull(w, n).copy() for n in ("state", OBS, "_timestep_", "_done_", REW, ACT)}
    out.update({f"batch_{k}": v.cpu().numpy() for k, v in dev["batch"].items()})
    out["rng"] = sh._words(dev["sampler"].rng_state, case.E)
    out["pool_rng"] = sh._words(w.env_resetter._pool_rng, case.E)
    out["pool"] = pull(w, "state_reset_pool").copy()
    return out


@pytest.mark.parametrize("case", cp.CASES, ids=repr)
def test_entries_against_the_model(case):
    """after every launch: the batch rows (obs, actions, rewards, done; the fence rows untouched), `state`,
    `observations`, `_timestep_`, `_done_`, `rewards`, `sampled_actions`, the sampler's and the pool generator's words
    against the model.  The first placement and geometry is replayed on the model; every other one must leave the same
    bytes in every array after every launch (and so agrees with the model too).  The crafted-pool case is the one that
    fails when the fast ticks ignore the pool rows; its twin with an ordinary pool runs them."""
    from tests.hip_harness import ACT, OBS, REW

    sh = _shapes()
    E, T = case.E, case.ticks
    dev = _device(case)
    first, combos = None, 0
    for placement in cp.PLACEMENTS:
        fn, args, block, grid, shared = _launch(dev, case, placement)
        staged = placement == "lds"
        assert fn.name == cp.ENTRY[case.hidden] and int(args[-1]) == (1 if staged else 0) and int(args[-2]) == case.pool
        assert shared == dev["w"].env.pool_rollout_lds_bytes(case.hidden, case.A, case.pool, staged)
        for geom in cp.GEOMETRIES:
            g = cc.geometry(E, geom)
            if g is None:
                continue
            threads, blocks, trips = g
            assert threads <= cc.LAUNCH_BOUND
            words0 = sh._tick_start(dev["w"], case, dev["sampler"], dev["start"])
            snaps = []
            for li in range(case.launches):
                for key, fill in (("obs", 7.0), ("actions", -1), ("rewards", 7.0), ("done", -1)):
                    dev["batch"][key].fill_(fill)
                fn(*args, block=(threads, 1, 1), grid=(blocks, 1), shared=shared)
                sh._sync()
                snaps.append(_snapshot(dev, case))
            combos += 1
            if first is not None:
                for li, (a, b) in enumerate(zip(first, snaps)):
                    for key in a:
                        assert a[key].tobytes() == b[key].tobytes(), (case.name, placement, geom, li, key)
                continue
            first = snaps
            model = cp.PoolModel(case)
            near = differ = 0
            for li, snap in enumerate(snaps):
                tag = f"{case.name} {placement} {geom} launch {li}"
                choice = cp.FollowDevice(case, snap["batch_actions"][:T, :, 0, 0])
                rows = model.launch(choice)
                near, differ = near + choice.near, differ + choice.differ
                sh.EQ(snap["batch_obs"][:T, :, 0], rows["obs"], f"{tag} obs rows")
                sh.EQ(snap["batch_actions"][:T, :, 0, 0], rows["actions"], f"{tag} action rows")
                sh.EQ(snap["batch_rewards"][:T, :, 0], rows["rewards"], f"{tag} reward rows")
                sh.EQ(snap["batch_done"][:T], rows["done"], f"{tag} done rows")
                assert (snap["batch_obs"][T:] == 7.0).all() and (snap["batch_actions"][T:] == -1).all(), tag
                assert (snap["batch_rewards"][T:] == 7.0).all() and (snap["batch_done"][T:] == -1).all(), tag
                st = model.state()
                sh.EQ(snap["state"][:, 0], st["state"], f"{tag} state")
                sh.EQ(snap[OBS][:, 0], st["obs"], f"{tag} observation")
                sh.EQ(snap["_timestep_"], st["timestep"], f"{tag} timestep")
                sh.EQ(snap["_done_"], st["done"], f"{tag} done")          # the launch's last tick, still set
                sh.EQ(snap[REW][:, 0], st["rewards"], f"{tag} reward")
                sh.EQ(snap[ACT].reshape(-1), st["actions"], f"{tag} sampled_actions")
                sh.EQ(snap["rng"][:4], words0[:4], f"{tag} RNG header")
                sh.EQ(snap["rng"][4:], st["epochs"], f"{tag} RNG epochs")
                sh.EQ(snap["pool_rng"][:2], np.array(model.pk, np.uint32), f"{tag} pool RNG key")
                sh.EQ(snap["pool_rng"][4:], st["pool_epochs"], f"{tag} pool epochs")
                sh.EQ(snap["pool"][:, 0], case.pool_rows(), f"{tag} the pool itself")
            restarts = int(model.restarts.sum())
            print(f"{case.name} [{fn.name}] {placement} {geom}: {threads} threads x {blocks} blocks, {trips} trips; "
                  f"{restarts} restarts ({model.terminal} terminal), pool rows {sorted(model.rows_drawn)}, {near} draws "
                  f"within {cc.NEAR_WINDOW} of a threshold (cap {case.near_cap()}), {differ} decided otherwise by the "
                  f"device, {model.crafted_survivors} restarts from a crafted row survived a tick")
            assert near <= case.near_cap() and restarts >= E
            assert not case.crafted or model.crafted_survivors >= 10
    assert combos == len(cp.PLACEMENTS) * (3 if E == 1501 else 2)


@pytest.mark.parametrize("hidden", [0, 32])
def test_guard_cases_write_nothing(hidden):
    """every shape the entries do not serve, launched once with valid pointers everywhere else (weights, probabilities and
    dynamic LDS sized for the widest variant): afterwards every byte of every array, of the batch tensors, of the pool
    and of both generators' words is unchanged"""
    import torch

    sh = _shapes()
    case = cp.PoolCase("guard", hidden, A=3, E=65)
    dev = _device(case)
    fn, args, block, grid, shared = dev["launch"]
    assert fn.name == cp.ENTRY[hidden]
    n_w = lambda H, A: 4 * H + H + H * H + H + A * H + A   # noqa: E731
    big = torch.full((n_w(64, 9),), 0.01, device="cuda")
    probs9 = torch.full((case.E, 1, 9), 1.0 / 9, device="cuda")
    i_probs = next(i for i, a in enumerate(args) if a is dev["probs"])
    i_policy = len(args) - 7          # policy, hidden, invariant_divide_ok, pool_rng, pool, n_pool, pool_in_lds
    assert int(args[i_probs + 1]) == 3 and int(args[i_policy + 1]) == hidden and int(args[-2]) == case.pool
    null = np.uint64(0)

    def variant(**changes):
        a = list(args)
        a[i_policy] = big   # (a valid pointer to enough floats whatever the variant reads)
        for key, v in changes.items():
            a[{"probs": i_probs, "n_actions": i_probs + 1, "policy": i_policy, "hidden": i_policy + 1,
               "pool_rng": len(args) - 4, "pool": len(args) - 3, "n_pool": len(args) - 2}[key]] = v
        return a

    variants = [("hidden is another width", variant(hidden=np.int32(64 if hidden else 32))),
                ("n_actions = 9", variant(probs=probs9, n_actions=np.int32(9))),
                ("n_actions = 0", variant(n_actions=np.int32(0))),
                ("n_pool = 0", variant(n_pool=np.int32(0))),
                ("n_pool = -3", variant(n_pool=np.int32(-3))),
                ("pool is null", variant(pool=null)),
                ("pool_rng is null", variant(pool_rng=null))]
    if hidden:
        variants.append(("policy is null", variant(policy=null)))
    lds = 4 * n_w(64, 9) + 16 * case.pool
    for name, a in variants:
        sh._tick_start(dev["w"], case, dev["sampler"], dev["start"])
        before = _snapshot(dev, case)
        fn(*a, block=block, grid=grid, shared=lds)
        sh._sync()
        after = _snapshot(dev, case)
        for key in before:
            assert before[key].tobytes() == after[key].tobytes(), (fn.name, name, key)
    # ... and the arguments as the host built them do write
    sh._tick_start(dev["w"], case, dev["sampler"], dev["start"])
    before = _snapshot(dev, case)
    fn(*args, block=block, grid=grid, shared=shared)
    sh._sync()
    after = _snapshot(dev, case)
    assert all(before[k].tobytes() != after[k].tobytes() for k in ("state", "batch_obs", "rng", "pool_rng"))
    print(f"{fn.name}: {len(variants)} guard cases, {len(before)} arrays unchanged each")


def test_engine_fuses_the_pooled_rollout_only():
    """RolloutEngine on a pooled Cartpole: unfused as before; with the batch tensors and ticks_per_launch > 1 one launch
    of the ..._P entry (fixed probabilities) or ..._P_H32 (a policy); with ticks_per_launch = 1 unfused"""
    import torch
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.rollout import RolloutEngine

    sh = _shapes()
    case = cp.PoolCase("engine", 32, E=65)
    w = sh._wrapper(case)
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=3)
    E, T = case.E, 5
    batch = {"obs": torch.zeros((T, E, 1, 4), device="cuda"), "actions": torch.zeros((T, E, 1, 1), dtype=torch.int32, device="cuda"),
             "rewards": torch.zeros((T, E, 1), device="cuda"), "done": torch.zeros((T, E), dtype=torch.int32, device="cuda")}
    packed = torch.from_numpy(case.policy()[1]).cuda()
    plain = RolloutEngine(w, sampler)
    assert not plain.fused and plain.step_kernel_name == "HipClassicControlCartPoleEnvStep"
    assert len(plain.entry_names) == 5   # sample, step, table reset, pool launch, undo
    live = RolloutEngine(w, sampler, rollout_batch=batch, rollout_policy=(packed, 32), ticks_per_launch=T)
    assert live.fused and live.ticks_per_launch == T
    assert live.step_kernel_name == "HipClassicControlCartPoleEnvRollout_P_H32" and live.entry_names == [live.step_kernel_name]
    fixed = RolloutEngine(w, sampler, rollout_batch=batch, ticks_per_launch=T)
    assert fixed.fused and fixed.entry_names == ["HipClassicControlCartPoleEnvRollout_P"]
    one = RolloutEngine(w, sampler, rollout_batch=batch, ticks_per_launch=1)
    assert not one.fused and one.step_kernel_name == "HipClassicControlCartPoleEnvStep"
    assert w.env.ticks_per_launch == 1   # (the env object keeps its own setting)
    live.run(1)
    torch.cuda.synchronize()
    assert float(batch["rewards"].min()) == 1.0 and int(batch["done"].sum()) >= 0


# --------------------------------------------------------------------------------------------------- the trainer
ALL = {"fused_rollout_policy": "all", "fused_update": "all"}


def _trainer(tmp_path, keys, E=200, T=20, seed=3):
    import torch
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    ov = {"trainer": {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": seed, **keys},
          "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0},
          "env": {"episode_length": 60, "reset_pool_size": 50, "seed": 11}}
    torch.manual_seed(seed)
    return setup_trainer("single_cartpole_with_reset_pool", ov, results_dir=str(tmp_path), verbose=False)


def _finite_losses(metrics):
    """the losses and every other metric but the spread of the actions over the agents (one agent: its std is undefined)"""
    keys = [k for k in metrics if "over agents" not in k]
    return {"Total loss", "Policy loss", "Value function loss", "Mean entropy"} <= set(keys) and \
        all(np.isfinite(metrics[k]) for k in keys)


def _params(tr):
    return {k: v.detach().cpu().clone() for k, v in tr._unwrap(tr.models["shared"]).state_dict().items()}


def test_composed_in_the_trainer(tmp_path):
    """single_cartpole_with_reset_pool at E = 200, T = 20, episode length 60, a pool of 50 rows, with
    fused_rollout_policy / fused_update "all": one launch of ..._P_H32 per batch, the five-launch update, a one-launch
    evaluation, finite losses; every restart the batch records starts at a pool row -- the row after a done row is the
    replica's saved observation copy, and the row after that is one Euler step from one of the 50 pool rows.  With
    fused_rollout_policy True: today's per-tick plan.  A checkpoint of either trainer loads into the other."""
    import torch
    from oracle.cartpole_np import CartPoleOracle
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    E, T = 200, 20
    tr = _trainer(tmp_path / "all", ALL)
    assert tr._batch_rollout is not None and tr.engine.fused
    assert tr.engine.step_kernel_name == "HipClassicControlCartPoleEnvRollout_P_H32"
    assert tr.engine.entry_names == [tr.engine.step_kernel_name]
    assert tr.update_path == {"shared": "kernels"}
    saved = tr.obs.detach().cpu().numpy().reshape(E, 4).copy()       # before the first tick: the saved copy itself
    pool = tr.w.cuda_data_manager.pull_data_from_device("state_reset_pool").reshape(50, 4).astype(F32)
    assert len({r.tobytes() for r in saved}) > E // 2               # (one host reset per replica: the rows differ)
    checked = restarts = 0
    for it in range(3):
        tr._generate_rollout_batch()
        torch.cuda.synchronize()
        b = tr.batch["shared"]
        obs = b["obs"][:T].cpu().numpy().reshape(T, E, 4)
        act = b["actions"][:T].cpu().numpy().reshape(T, E)
        done = tr.done_batch[:T].cpu().numpy().reshape(T, E)
        assert (b["rewards"][:T].cpu().numpy() == 1.0).all() and set(np.unique(done)) <= {0, 1}
        restarts += int(done.sum())
        for t in range(T - 2):
            envs = np.flatnonzero((done[t] > 0) & (done[t + 1] == 0))
            if not len(envs):
                continue
            np.testing.assert_array_equal(obs[t + 1][envs], saved[envs], err_msg=f"iteration {it} tick {t}")
            for a in (0, 1):   # one Euler step of every pool row under this action
                sel = envs[act[t + 1][envs] == a]
                orc = CartPoleOracle(50, 10 ** 9)
                orc.state = pool.copy()
                orc.step(np.full(50, a))
                nxt = {r.tobytes() for r in orc.state}
                assert all(obs[t + 2][e].tobytes() in nxt for e in sel), (it, t, a)
                checked += len(sel)
        m = tr._update_model_params(it, True)
        torch.cuda.synchronize()
        assert _finite_losses(m["shared"]), m["shared"]
        assert torch.equal(tr._batch_rollout["packed"]["shared"].cpu(), pack_rollout_policy(tr.models["shared"]).cpu()), it
    assert restarts >= E and checked >= E // 2, (restarts, checked)
    rewards, steps = tr.evaluate_episodes(use_argmax=True)
    assert tr.evaluation_path == "one launch"
    assert np.isfinite(rewards["shared"]).all() and (steps["shared"] >= 1).all() and (steps["shared"] <= 60).all()
    # ---- the same config on today's path
    plain = _trainer(tmp_path / "plain", {"fused_rollout_policy": True})
    assert plain._batch_rollout is None and not plain.engine.fused
    assert plain.engine.step_kernel_name == "HipClassicControlCartPoleEnvStep" and plain.update_path == {"shared": "framework"}
    plain._generate_rollout_batch()
    assert np.isfinite(plain._update_model_params(0, True)["shared"]["Total loss"])
    plain.evaluate_episodes(use_argmax=True)
    assert plain.evaluation_path == "per tick"
    # ---- checkpoints, both ways
    tr.current_timestep["shared"] = 600
    tr.save_model_checkpoint()
    plain.load_model_checkpoint({"shared": os.path.join(tr.save_dir, "shared_600.state_dict")})
    for k, v in _params(tr).items():
        assert torch.equal(v, _params(plain)[k]), k
    plain._generate_rollout_batch()
    assert np.isfinite(plain._update_model_params(1, True)["shared"]["Total loss"])
    plain.current_timestep["shared"] = 700
    plain.save_model_checkpoint()
    tr.load_model_checkpoint({"shared": os.path.join(plain.save_dir, "shared_700.state_dict")})
    for k, v in _params(plain).items():
        assert torch.equal(v, _params(tr)[k]), k
    tr._generate_rollout_batch()   # (the packed policy is refilled from the loaded weights before the launch)
    torch.cuda.synchronize()
    assert torch.equal(tr._batch_rollout["packed"]["shared"].cpu(), pack_rollout_policy(tr.models["shared"]).cpu())
    assert _finite_losses(tr._update_model_params(3, True)["shared"]) and tr.update_path == {"shared": "kernels"}
    tr.graceful_close()
    plain.graceful_close()


# ------------------------------------------------------------------------------------------------------- learning
@pytest.mark.parametrize("path", ["per tick", "one launch"])
def test_pooled_cartpole_learns(path, tmp_path):
    """tests/test_gpu_learning.py's Cartpole shape (E = 1000, T = 50, episode length 200) with reset_pool_size 1000 and
    that file's bar: the first mean episode length in 15 .. 30, the last ten of 300 iterations at least 3 x the first --
    on the per-tick plan and on the one launch with the update kernels.
    (Recorded curves: docs/rounds/r26.md.)"""
    import torch
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    ov = {"trainer": {"num_envs": 1000, "train_batch_size": 1000 * 50, "num_episodes": 10 ** 6, "seed": 7,
                      **(ALL if path == "one launch" else {})},
          "env": {"episode_length": 200, "reset_pool_size": 1000},
          "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0}}
    torch.manual_seed(0)
    tr = setup_trainer("single_cartpole_with_reset_pool", ov, results_dir=str(tmp_path), verbose=False)
    assert (tr._batch_rollout is not None) == (path == "one launch")
    assert tr.update_path == {"shared": "kernels" if path == "one launch" else "framework"}
    tr.train(300)
    tr.graceful_close()
    curve = [json.loads(line)["shared"]["Mean episodic reward"] for line in open(os.path.join(str(tmp_path), "results.json"))]
    assert len(curve) == 300 and all(np.isfinite(curve))
    first, last = float(np.mean(curve[:3])), float(np.mean(curve[-10:]))
    print(f"pooled cartpole, {path}: mean episode length {first:.1f} -> {last:.1f}; every 20th: {np.round(curve[::20], 1).tolist()}")
    assert 15.0 <= first <= 30.0, first
    assert last >= 3.0 * first, (first, last, curve[::10])
