"""TagGridWorld with a reset pool on the MI355X, one launch per batch: HipTagGridWorldRollout_N5P (fixed probabilities),
_N5P_H32 / _N5P_H64 (live policies, shared or two distinct ones), HipTagGridWorldEvaluate_N5P_H<32|64>
(csrc/kernels/tag_gridworld_n5_pool.hip) launched directly with the arguments the env builds, against the numpy model of
tests/gridworld_pool_cases.py at tolerance 0; then the trainer on `tag_gridworld_with_reset_pool` with the three opt-in
keys, and a learning run on both paths.  The cases are sized on the host by tests/test_gridworld_pool_rollout_host.py.
`pytest -s` prints one line per case."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests import gridworld_evaluate as gev
from tests import gridworld_pool_cases as gp

pytestmark = pytest.mark.gpu

F32 = np.float32
N, F = gp.N, gp.F
SURPLUS = 2                      # batch rows behind the launch's, which keep their sentinels
SENT_F, SENT_I = -7.5, -1


# ------------------------------------------------------------------------------------------------------- plumbing
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def EQ(got, want, tag=""):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(tag))


def _put(w, name, arr):
    from warp_drive_amd.managers import hip_driver as drv

    dm = w.cuda_data_manager
    arr = np.ascontiguousarray(arr)
    assert arr.size == int(np.prod(dm.get_shape(name))) and str(arr.dtype) in str(dm.get_dtype(name)), (name, arr.dtype)
    drv.memcpy_htod(dm.device_data(name), arr)
    torch.cuda.synchronize()


def _words(ptr, n):
    from warp_drive_amd.managers import hip_driver as drv

    out = np.zeros(4 + n, dtype=np.uint32)
    drv.memcpy_dtoh(out, ptr)
    torch.cuda.synchronize()
    return out


def _put_words(ptr, words):
    from warp_drive_amd.managers import hip_driver as drv

    drv.memcpy_htod(ptr, np.ascontiguousarray(words, dtype=np.uint32))
    torch.cuda.synchronize()


def _image(w, skip=()):
    """the byte image of every device array of the env's data manager except `skip`"""
    from warp_drive_amd.managers import hip_driver as drv

    out = {}
    for name, p in w.cuda_data_manager._device_data_pointer.items():
        if int(p.nbytes) > 0 and name not in skip:
            buf = np.zeros(int(p.nbytes), np.uint8)
            drv.memcpy_dtoh(buf, p)
            out[name] = buf
    torch.cuda.synchronize()
    return out


def _same_image(a, b, tag):
    assert set(a) == set(b)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), (tag, name)


class _Device:
    """a case's env on the device: wrapper, pool generator, sampler, the start state and both generators' words written"""

    def __init__(self, env, E, start, epochs, pool_epochs):
        from tests.hip_harness import OBS, make_wrapper, require_gpu
        from warp_drive_amd.managers.function_manager import HIPSampler

        require_gpu()
        self.E, self.OBS = E, OBS
        self.w = w = make_wrapper(env, E)
        w.init_reset_pool(seed=gp.POOL_SEED)
        self.pool_x, self.pool_y = self.pull("loc_x_reset_pool"), self.pull("loc_y_reset_pool")
        self.sampler = HIPSampler(w.cuda_function_manager)
        self.sampler.init_random(seed=gp.SAMPLER_SEED)
        self.words0 = _words(self.sampler.rng_state, E * N)
        self.pool_words0 = _words(w.env_resetter._pool_rng, E)
        assert (int(self.words0[0]), int(self.words0[1])) == gp.seed_words(gp.SAMPLER_SEED) and (self.words0[4:] == 0).all()
        assert (int(self.pool_words0[0]), int(self.pool_words0[1])) == gp.seed_words(gp.POOL_SEED)
        assert (self.pool_words0[4:] == 0).all()
        self.words0[4:] = np.asarray(epochs, np.uint32).reshape(-1)
        self.pool_words0[4:] = pool_epochs
        self.start = start
        self.rewind()

    def pull(self, name):
        return self.w.cuda_data_manager.pull_data_from_device(name)

    def rewind(self):
        orc, w = self.start, self.w
        _put(w, "loc_x", orc.loc_x)
        _put(w, "loc_y", orc.loc_y)
        _put(w, "_timestep_", orc.timestep)
        _put(w, "_done_", np.zeros(self.E, np.int32))
        _put(w, self.OBS, orc.obs.astype(F32))
        _put_words(self.sampler.rng_state, self.words0)
        _put_words(w.env_resetter._pool_rng, self.pool_words0)

    def words(self):
        return _words(self.sampler.rng_state, self.E * N), _words(self.w.env_resetter._pool_rng, self.E)


def _rollout_device(case):
    from oracle.tag_gridworld_np import TagGridWorldOracle

    dev = _Device(case.env(), case.E, TagGridWorldOracle(num_envs=case.E, **case.config()), case.start_epochs(),
                  case.start_pool_epochs())
    px, py = case.pools()
    EQ(dev.pool_x, px, "the pool the env pushed is the one the host cases are sized on")
    EQ(dev.pool_y, py)
    return dev


def _batch(T, E):
    return {"obs": torch.full((T + SURPLUS, E, N, F), SENT_F, device="cuda"),
            "actions": torch.full((T + SURPLUS, E, N, 1), SENT_I, dtype=torch.int32, device="cuda"),
            "rewards": torch.full((T + SURPLUS, E, N), SENT_F, device="cuda"),
            "done": torch.full((T + SURPLUS, E), SENT_I, dtype=torch.int32, device="cuda")}


def _refill(batch):
    for key, t in batch.items():
        t.fill_(SENT_F if t.dtype == torch.float32 else SENT_I)


WRITTEN = ("loc_x", "loc_y", "_timestep_", "_done_")   # + observations, rewards, actions (hip_harness names)


def _check_state(dev, st, tag):
    from tests.hip_harness import ACT, OBS, REW

    EQ(dev.pull("loc_x"), st["loc_x"], (tag, "loc_x"))
    EQ(dev.pull("loc_y"), st["loc_y"], (tag, "loc_y"))
    EQ(dev.pull(OBS), st["obs"], (tag, "observations"))
    EQ(dev.pull("_timestep_"), st["timestep"], (tag, "_timestep_"))
    EQ(dev.pull("_done_"), st["done"], (tag, "_done_"))
    EQ(dev.pull(REW), st["rewards"], (tag, "rewards"))
    EQ(dev.pull(ACT)[..., 0], st["actions"], (tag, "actions"))
    words, pool_words = dev.words()
    EQ(words[:4], dev.words0[:4], tag)
    EQ(words[4:], st["epochs"], (tag, "sampler words"))
    EQ(pool_words[:4], dev.pool_words0[:4], tag)
    EQ(pool_words[4:], st["pool_epochs"], (tag, "pool words"))


def _check_rows(b, rows, T, tag):
    EQ(b["obs"][:T], rows["obs"], (tag, "obs rows"))
    EQ(b["actions"][:T, :, :, 0], rows["actions"], (tag, "action rows"))
    EQ(b["rewards"][:T], rows["rewards"], (tag, "reward rows"))
    EQ(b["done"][:T], rows["done"], (tag, "done rows"))
    for key in b:   # the fence
        sent = SENT_F if b[key].dtype == np.float32 else SENT_I
        assert (b[key][T:] == sent).all(), (tag, key, "a row behind the launch's was written")


def _unwritten(dev):
    from tests.hip_harness import ACT, OBS, REW

    return _image(dev.w, skip=WRITTEN + (ACT, OBS, REW))


# ------------------------------------------------------------------------------------------- fixed probabilities
@pytest.mark.parametrize("case", gp.FIXED_CASES, ids=repr)
def test_fixed_probabilities_against_the_model(case):
    """HipTagGridWorldRollout_N5P under the host's grid and under a grid of ONE block (E = 13: two trips of the stride
    loop, E = 25: three): batch rows, fence, every array the launch leaves, both generators' words -- bit for bit the
    model's; nothing else in the data manager changes; restarts, pool rows and pool words as the host test sized them"""
    dev = _rollout_device(case)
    env, E, T = dev.w.env, case.E, case.ticks
    env.ticks_per_launch = T
    probs = torch.from_numpy(case.probabilities()).cuda()
    batch = _batch(T, E)
    assert env.has_pool_rollout(5)
    fn, args, block, grid, shared = env.tick_launch(dev.sampler, [probs], dev.w.env_resetter, batch=batch)
    assert fn.name == "HipTagGridWorldRollout_N5P" and block == (64, 1, 1) and grid == (-(-E // gp.EPB), 1)
    assert shared == env.pool_rollout_lds_bytes(0) <= 64 * 1024
    for blocks in sorted({grid[0], 1}, reverse=True):
        dev.rewind()
        model = gp.PoolModel(case, dev.pool_x, dev.pool_y)
        other = _unwritten(dev)
        for launch in range(case.launches):
            tag = (case.name, f"grid {blocks}", f"launch {launch}")
            _refill(batch)
            fn(*args, block=block, grid=(blocks, 1), shared=shared)
            torch.cuda.synchronize()
            rows = model.launch(T, probs=case.probabilities())
            _check_rows({k: v.cpu().numpy() for k, v in batch.items()}, rows, T, tag)
            _check_state(dev, model.state(), tag)
        _same_image(other, _unwritten(dev), case.name)
        assert gp.coverage_ok(case, model), (int(model.restarts.sum()), sorted(model.rows_drawn))
        EQ(model.pool_epochs - case.start_pool_epochs(), model.restarts.astype(np.uint32))
    print(f"{case.name}: {int(model.restarts.sum())} restarts ({model.tags} tags), pool rows {len(model.rows_drawn)} of "
          f"{case.n_pool}, largest coordinate {model.max_coord}, {shared} bytes of LDS")


# ------------------------------------------------------------------------------------------------- live policies
@pytest.mark.parametrize("shared_policy", [True, False], ids=["shared", "distinct"])
@pytest.mark.parametrize("hidden", [32, 64])
@pytest.mark.parametrize("case", gp.POLICY_CASES, ids=repr)
def test_live_policies_against_the_model(case, hidden, shared_policy):
    """HipTagGridWorldRollout_N5P_H32 / _H64 with one policy passed twice and with two: actions by
    tests/test_gpu_gridworld_shapes.py's rule (the counting draw on the float32 restatement of the in-kernel forward; a
    mismatch only where the uniform is within 2e-6 of a running sum; at most 2 + draws // 50000 of them; the model
    follows the device), everything downstream at tolerance 0"""
    dev = _rollout_device(case)
    env, E, T = dev.w.env, case.E, case.ticks
    env.ticks_per_launch = T
    _, packed_np = gp.policies(hidden, shared_policy, seed=hidden + case.seed)
    tensors = [torch.from_numpy(p).cuda() for p in (packed_np[:1] if shared_policy else packed_np)]
    packed = tensors * 2 if shared_policy else tensors
    assert (packed[0] is packed[1]) == shared_policy
    probs = torch.full((E, N, 5), 0.2, device="cuda")
    batch = _batch(T, E)
    assert env.has_live_policy_rollout(hidden, 5)
    fn, args, block, grid, shared = env.tick_launch(dev.sampler, [probs], dev.w.env_resetter, batch=batch,
                                                    policy=(packed, hidden))
    assert fn.name == f"HipTagGridWorldRollout_N5P_H{hidden}" and block == (64, 1, 1) and grid == (-(-E // gp.EPB), 1)
    assert shared == env.pool_rollout_lds_bytes(hidden) <= 64 * 1024
    model = gp.PoolModel(case, dev.pool_x, dev.pool_y)
    near = draws = 0
    counts = np.zeros(5, np.int64)
    for launch in range(case.launches):
        tag = (case.name, hidden, f"launch {launch}")
        _refill(batch)
        fn(*args, block=block, grid=grid, shared=shared)
        torch.cuda.synchronize()
        b = {k: v.cpu().numpy() for k, v in batch.items()}
        judge = gp.Judge(packed_np, hidden, b["actions"][:T, :, :, 0])
        rows = model.launch(T, choose=judge)
        _check_rows(b, rows, T, tag)
        _check_state(dev, model.state(), tag)
        near, draws = near + judge.near, draws + judge.draws
        counts += np.bincount(rows["actions"].ravel(), minlength=5)
    hist = counts / counts.sum()
    print(f"{case.name} H{hidden} {'shared' if shared_policy else 'distinct'}: {int(model.restarts.sum())} restarts, "
          f"{near} draws on a threshold of {draws}, action shares {np.round(hist, 2).tolist()}")
    assert near <= 2 + draws // 50000 and hist.max() < 0.95, (near, draws, hist)
    # (which rows are drawn follows from the restarts, and those from the policy's actions: only the count is demanded)
    assert int(model.restarts.sum()) >= 2 * E and (model.restarts >= 1).all()
    EQ(model.pool_epochs - case.start_pool_epochs(), model.restarts.astype(np.uint32))


# ------------------------------------------------------------------------------------------------------ evaluation
@pytest.mark.parametrize("case", gp.EVAL_CASES, ids=repr)
def test_one_launch_evaluation_against_the_replay(case):
    """HipTagGridWorldEvaluate_N5P_H<width> at grid_length 100, greedy and sampled: reward sums, steps, done and the
    action trace equal the per-tick replay that follows the device's trace (tests/gridworld_evaluate.py: a decision may
    differ only inside the 2e-6 window); the sampler words advance by the steps (sampled) or not at all (greedy); the env
    arrays and the pool words are unchanged"""
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorldWithResetPool

    E, T = case.E, case.T
    dev = _Device(CUDATagGridWorldWithResetPool(seed=gp.ENV_SEED, **case.env_config()), E, case.oracle(),
                  case.start_epochs(), np.arange(E, dtype=np.uint32) * 3 + 1)
    env = dev.w.env
    packed_np = case.policies()[1]
    packed = [torch.from_numpy(p).cuda() for p in packed_np]
    out = {"reward_sum": torch.full((E + SURPLUS, N), SENT_F, device="cuda"),
           "steps": torch.full((E + SURPLUS,), SENT_I, dtype=torch.int32, device="cuda"),
           "done": torch.full((E + SURPLUS,), SENT_I, dtype=torch.int32, device="cuda")}
    trace = torch.full((T + SURPLUS, E, N), SENT_I, dtype=torch.int32, device="cuda")
    assert env.has_live_policy_evaluate(case.hidden, 5)
    fn, args, block, grid, shared = env.evaluate_launch(dev.sampler, policy=(packed, case.hidden), use_argmax=case.greedy,
                                                        outputs=out, action_trace=trace, ticks=T)
    assert fn.name == f"HipTagGridWorldEvaluate_N5P_H{case.hidden}" and (block, grid) == ((64, 1, 1), (-(-E // gp.EPB), 1))
    assert shared == env.live_policy_evaluate_lds_bytes(case.hidden) <= 64 * 1024
    before = _image(dev.w)
    fn(*args, block=block, grid=grid, shared=shared)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    got_trace = trace.cpu().numpy()
    r = gev.replay(case, ticks=T, trace=got_trace, packed=packed_np)
    for key in ("reward_sum", "steps", "done"):
        EQ(got[key][:E], r[key], (case.name, key))
        assert (got[key][E:] == (SENT_F if key == "reward_sum" else SENT_I)).all(), key
    want_trace = np.full(got_trace.shape, SENT_I, np.int32)
    want_trace[:T] = r["actions"]
    EQ(got_trace, want_trace, (case.name, "trace"))
    words, pool_words = dev.words()
    want_words = dev.words0.copy()
    want_words[4:] = r["epochs"].reshape(-1)
    EQ(words, want_words, "sampler words")
    EQ(pool_words, dev.pool_words0, "pool words")
    _same_image(before, _image(dev.w), case.name)
    assert r["near"] <= case.near_cap(r["decisions"]) and (r["done"] == 1).all()
    print(f"{case.name}: steps {int(r['steps'].min())} .. {int(r['steps'].max())}, {int(r['tagged'].sum())} tagged, "
          f"{r['wall_hits']} wall hits, largest coordinate {r['max_coord']}, {r['followed']} decisions followed the device")
    if E >= 13:
        assert gp.eval_coverage_ok(case, r)


# --------------------------------------------------------------------------------------------------- the trainer
GW_STAGES = ("HipPgGwValues", "HipDiscountedReturns", "HipPgGwGradients", "HipPgGwReduce", "HipPgGwApply")
OPT_IN = {"fused_rollout_policy": "all", "fused_update": "all", "fused_evaluation": True}


def _trainer(tmp_path, keys, E=25, T=6, seed=3):
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    ov = {"trainer": {"num_envs": E, "train_batch_size": E * T, "num_episodes": 10 ** 6, "seed": seed, **keys},
          "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0}, "env": {"episode_length": 5, "seed": 11}}
    torch.manual_seed(seed)
    return setup_trainer("tag_gridworld_with_reset_pool", ov, results_dir=str(tmp_path), verbose=False)


def _counts():
    from warp_drive_amd.managers import hip_driver as drv

    return dict(drv.LAUNCH_COUNTS)


def _since(before, prefix=("HipPg", "HipDiscountedReturns", "HipTagGridWorld")):
    out = {}
    for name, n in _counts().items():
        d = n - before.get(name, 0)
        if d and name.startswith(prefix):
            stage = name.split("_H")[0] if name.startswith("HipPg") else name
            out[stage] = out.get(stage, 0) + d
    return out


def test_composed_in_the_trainer(tmp_path, caplog):
    """tag_gridworld_with_reset_pool at E = 25, T = 6, episode_length 5 with the three opt-in keys: the rollout is the
    _N5P_H32 entry, the shared policy (n = 5) is updated by five launches per iteration, the packed tensor equals
    pack_gridworld_policy(model) after every Apply, a logging iteration's metrics are finite, evaluate_episodes is one
    launch in both modes.  Without the keys: today's per-tick plan, the framework update, nothing logged."""
    from warp_drive_amd.training import pg_update_gridworld_kernels as pggk
    from warp_drive_amd.training.policy_kernel import pack_gridworld_policy

    E, T = 25, 6
    tr = _trainer(tmp_path / "k", OPT_IN)
    assert tr._batch_rollout is not None and tr.engine.fused
    assert tr.engine.step_kernel_name == "HipTagGridWorldRollout_N5P_H32" and tr.engine.entry_names == [tr.engine.step_kernel_name]
    assert tr.update_path == {"shared": "kernels"} and tr.policy_map == {"shared": [0, 1, 2, 3, 4]}
    k = tr._pg_kernels["shared"]
    assert isinstance(k, pggk.PgGridworldUpdateKernels) and (k.E, k.T, k.n, k.H) == (E, T, 5, 32)
    pool_before = _words(tr.w.env_resetter._pool_rng, E)[4:].copy()
    for it in range(3):
        log = it == 1
        tr._generate_rollout_batch()
        torch.cuda.synchronize()
        done = tr.done_batch[:T].cpu().numpy()
        pool_now = _words(tr.w.env_resetter._pool_rng, E)[4:]
        EQ(pool_now - pool_before, (done > 0).sum(axis=0).astype(np.uint32), "pool words advance by the restarts")
        pool_before = pool_now.copy()
        assert (done > 0).sum() >= E   # episode_length 5 of 6 ticks: every replica restarts in every batch
        before = _counts()
        metrics = tr._update_model_params(it, log)
        torch.cuda.synchronize()
        assert _since(before, ("HipPg", "HipDiscountedReturns")) == {s: 1 for s in GW_STAGES}, (it, _since(before))
        packed = tr._batch_rollout["packed"]["shared"]
        assert torch.equal(packed.cpu(), pack_gridworld_policy(tr.models["shared"]).cpu()), it
        if log:
            bad = {key: v for key, v in metrics["shared"].items() if not np.isfinite(v)}
            assert metrics["shared"] and not bad, bad
        else:
            assert metrics == {}
    for use_argmax in (True, False):
        before = _counts()
        rewards, steps = tr.evaluate_episodes(use_argmax=use_argmax)
        assert tr.evaluation_path == "one launch"
        assert _since(before, ("HipTagGridWorld", "HipEvaluate")) == {"HipTagGridWorldEvaluate_N5P_H32": 1}, _since(before)
        assert rewards["shared"].shape == (E, 5) and np.isfinite(rewards["shared"]).all()
        assert steps["shared"].shape == (E,) and (steps["shared"] >= 1).all() and (steps["shared"] <= 5).all()
    tr.graceful_close()
    # ---- without the keys: the plan tests/test_gpu_gridworld_shapes.py pins, the framework's update, no new message
    with caplog.at_level(logging.INFO):
        plain = _trainer(tmp_path / "p", {})
    assert plain._batch_rollout is None and not plain.engine.fused and plain.engine.step_kernel_name == "HipTagGridWorldStep"
    assert plain.update_path == {"shared": "framework"} and plain._pg_kernels == {}
    said = [r.getMessage() for r in caplog.records if "fused" in r.getMessage() or "whole-batch" in r.getMessage()]
    assert said == [], said
    before = _counts()
    plain._generate_rollout_batch()
    m = plain._update_model_params(0, True)
    assert np.isfinite(m["shared"]["Total loss"]) and not [s for s in _since(before) if s.startswith(("HipPg", "HipTagGridWorldRollout"))]
    plain.evaluate_episodes(use_argmax=True)
    assert plain.evaluation_path == "per tick"
    plain.graceful_close()


# ------------------------------------------------------------------------------------------------------- learning
# Recorded on the MI355X in one session (docs/rounds/r24.md has both curves): the per-tick framework path -- what this
# env trained on before the one-launch rollout existed -- gains PER_TICK_GAIN in mean episodic reward from the mean of
# its first 3 to the mean of its last 10 of 60 iterations.  The bar is half of it: seed noise does not fail it, a rollout
# that does not learn does.
PER_TICK_GAIN = 4.63    # 0.539 -> 5.169 (profiles/r24_learning_curves.json; the one-launch path in that session: 0.531 -> 5.055)
LEARNING_BAR = 0.5 * PER_TICK_GAIN


def learning_curve(tmp_path, keys):
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    ov = {"trainer": {"num_envs": 600, "train_batch_size": 600 * 100, "num_episodes": 10 ** 6, "seed": 7, **keys},
          "env": {"grid_length": 20}, "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0}}
    torch.manual_seed(0)
    tr = setup_trainer("tag_gridworld_with_reset_pool", ov, results_dir=str(tmp_path), verbose=False)
    tr.train(60)
    tr.graceful_close()
    curve = [json.loads(line)["shared"]["Mean episodic reward"] for line in open(os.path.join(str(tmp_path), "results.json"))]
    assert len(curve) == 60 and all(np.isfinite(curve))
    return tr, curve


def _gain(curve):
    return float(np.mean(curve[-10:]) - np.mean(curve[:3]))


def test_the_shared_policy_learns_on_both_paths(tmp_path):
    """the shared [32, 32] policy on a 20 x 20 grid, E = 600, T = 100, 60 iterations, seeded: on the per-tick framework
    path and on the one-launch rollout with the update kernels the mean episodic reward gains at least LEARNING_BAR"""
    gains = {}
    for name, keys in (("per tick", {}), ("one launch", {"fused_rollout_policy": "all", "fused_update": "all"})):
        tr, curve = learning_curve(tmp_path / name.replace(" ", "_"), keys)
        assert (tr._batch_rollout is not None) == (name == "one launch")
        assert tr.update_path == {"shared": "kernels" if name == "one launch" else "framework"}
        gains[name] = _gain(curve)
        print(f"{name}: mean episodic reward {np.mean(curve[:3]):.3f} -> {np.mean(curve[-10:]):.3f}, every 5th: "
              f"{np.round(curve[::5], 2).tolist()}")
    assert gains["per tick"] >= LEARNING_BAR and gains["one launch"] >= LEARNING_BAR, (gains, LEARNING_BAR)
