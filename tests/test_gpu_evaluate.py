"""Trainer.evaluate_episodes on the MI355X: the six HipClassicControl<CartPole|Acrobot|MountainCar>EnvEvaluate_H<32|64>
entries launched directly (parity with the host replay of tests/classic_control_evaluate.py that follows the device's
recorded actions, under several geometries; nothing but the outputs is written; only the first episode counts; the
guard), HipEvaluateAccumulate against its numpy model, the trainer on both paths, and a trained Cartpole policy scored
greedily.  The cases are sized on the host by tests/test_classic_control_evaluate_host.py.  `pytest -s` prints one line
per case."""
import json
import os

import numpy as np
import pytest
import torch

from tests import classic_control_cases as cc
from tests import classic_control_evaluate as ev

pytestmark = pytest.mark.gpu

F32 = np.float32
N_TAIL = 11   # arguments of an Evaluate entry after the step's: rng, n_actions, tag, ticks, packed, width, use_argmax,
#               reward_sum, steps, done, trace


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


def _wrapper(case):
    from tests.hip_harness import make_wrapper, require_gpu

    require_gpu()
    w = make_wrapper(cc.make_env(case.env, case.T, case.pool), case.E)
    if case.pool:
        w.init_reset_pool(seed=cc.POOL_SEED)
    return w


def _image(w, extra=()):
    """the byte image of every device array of the env's data manager (env arrays, their reset copies, the pool, the
    placeholders), of the pool's RNG words and of `extra` tensors"""
    from warp_drive_amd.managers import hip_driver as drv

    out = {}
    for name, p in w.cuda_data_manager._device_data_pointer.items():
        if int(p.nbytes) > 0:
            buf = np.zeros(int(p.nbytes), np.uint8)
            drv.memcpy_dtoh(buf, p)
            out[name] = buf
    torch.cuda.synchronize()
    if getattr(w.env_resetter, "_pool_rng", None) is not None:
        out["<pool rng>"] = _words(w.env_resetter._pool_rng, w.n_envs)
    for i, t in enumerate(extra):
        out[f"<extra {i}>"] = t.cpu().numpy().copy()
    return out


def _same_image(a, b, tag):
    assert set(a) == set(b)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), (tag, name)


_STEPPERS = {}


def _device_step(case):
    """(state [E, S], action [E]) -> (state, obs, reward, terminal code) through the env's Step kernel on a second
    wrapper (timestep 0 before the step: no time-out; `_done_` cleared: the flag is this step's terminal code)"""
    from tests.hip_harness import ACT, OBS, REW, pull

    key = (case.env, case.E)
    if key not in _STEPPERS:
        _STEPPERS[key] = _wrapper(case)
    w, E = _STEPPERS[key], case.E
    zeros = np.zeros(E, np.int32)

    def step(state, action):
        _put(w, "state", np.asarray(state, F32))
        _put(w, "_timestep_", zeros)
        _put(w, "_done_", zeros)
        _put(w, ACT, np.asarray(action, np.int32))
        w.step_all_envs()
        torch.cuda.synchronize()
        return pull(w, "state")[:, 0].copy(), pull(w, OBS)[:, 0].copy(), pull(w, REW)[:, 0].copy(), pull(w, "_done_").copy()

    return step


class _Launch:
    """one case set up on the device: the start state, observation, timestep and epoch words written, the outputs and
    the trace pre-filled with sentinels (three surplus rows each)"""

    def __init__(self, case, ticks=None, trace_rows=None):
        from tests.hip_harness import OBS
        from warp_drive_amd.managers.function_manager import HIPSampler

        self.case, E = case, case.E
        self.ticks = case.T if ticks is None else int(ticks)
        self.w = w = _wrapper(case)
        state, ts = case.start()
        self.obs0 = cc.host_obs(case.env, state) if case.env != "cartpole" else state.copy()
        _put(w, "state", state)
        _put(w, OBS, self.obs0)
        _put(w, "_timestep_", ts)
        _put(w, "_done_", np.zeros(E, np.int32))
        self.sampler = HIPSampler(w.cuda_function_manager)
        self.sampler.init_random(seed=cc.SAMPLER_SEED)
        self.words0 = _words(self.sampler.rng_state, E)
        assert (self.words0[:2] == np.array(ev.seed_words(cc.SAMPLER_SEED), np.uint32)).all()
        self.words0[4:] = case.start_epochs()
        self.packed_np = case.policy()[1]
        self.packed = torch.from_numpy(self.packed_np).cuda()
        rows = (self.ticks if trace_rows is None else trace_rows) + ev.SURPLUS
        self.out = {"reward_sum": torch.empty(E + ev.SURPLUS, dtype=torch.float32, device="cuda"),
                    "steps": torch.empty(E + ev.SURPLUS, dtype=torch.int32, device="cuda"),
                    "done": torch.empty(E + ev.SURPLUS, dtype=torch.int32, device="cuda")}
        self.trace = torch.empty((rows, E), dtype=torch.int32, device="cuda")
        self.fn, self.args, self.block, self.grid, self.shared = w.env.evaluate_launch(
            self.sampler, policy=(self.packed, case.hidden), use_argmax=case.greedy, outputs=self.out,
            action_trace=self.trace, ticks=self.ticks)
        assert self.fn.name == f"{cc.ENTRY[case.env]}Evaluate_H{case.hidden}"
        assert self.shared == 4 * self.packed_np.size and self.block[0] <= cc.LAUNCH_BOUND

    def rewind(self):
        self.out["reward_sum"].fill_(float(ev.SENTINEL_F))
        self.out["steps"].fill_(int(ev.SENTINEL_I))
        self.out["done"].fill_(int(ev.SENTINEL_I))
        self.trace.fill_(int(ev.SENTINEL_I))
        _put_words(self.sampler.rng_state, self.words0)

    def run(self, geom="product", args=None):
        """-> {"reward_sum", "steps", "done", "trace", "words"} pulled after one launch from the rewound start"""
        self.rewind()
        threads, blocks, _ = cc.geometry(self.case.E, geom, product=(self.block[0], self.grid[0]))
        assert threads <= cc.LAUNCH_BOUND
        self.fn(*(self.args if args is None else args), block=(threads, 1, 1), grid=(blocks, 1), shared=self.shared)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in self.out.items()}
        got["trace"] = self.trace.cpu().numpy()
        got["words"] = _words(self.sampler.rng_state, self.case.E)
        return got

    def check_against_replay(self, got, tag):
        """the replay follows the recorded actions (each the host's or inside the near-tie set); then bit for bit:
        the three outputs, the trace rows up to each replica's end (sentinels after it and in the surplus rows), the RNG
        words (sampled: epoch += steps; greedy: untouched)"""
        case, E = self.case, self.case.E
        r = ev.replay(case, ticks=self.ticks, step=_device_step(case), trace=got["trace"], packed=self.packed_np)
        for key in ("reward_sum", "steps", "done"):
            EQ(got[key][:E], r[key], (tag, key))
        EQ(got["reward_sum"][E:], np.full(ev.SURPLUS, ev.SENTINEL_F), tag)
        EQ(got["steps"][E:], np.full(ev.SURPLUS, ev.SENTINEL_I), tag)
        EQ(got["done"][E:], np.full(ev.SURPLUS, ev.SENTINEL_I), tag)
        want_trace = np.full(got["trace"].shape, ev.SENTINEL_I, np.int32)
        want_trace[: self.ticks] = np.where(r["actions"] >= 0, r["actions"], ev.SENTINEL_I)
        EQ(got["trace"], want_trace, (tag, "trace"))
        want_words = self.words0.copy()
        want_words[4:] = r["epochs"]
        EQ(got["words"], want_words, (tag, "rng words"))
        assert r["near"] <= case.near_cap(r["decisions"]), (tag, r["near"])
        return r


def _line(case, r, extra=""):
    share = np.round(r["counts"] / max(1, r["counts"].sum()), 3).tolist()
    print(f"{case.name}: {r['decisions']} decisions, {r['near']} near a tie ({r['followed']} followed the device), "
          f"terminations on {len(r['end_ticks'])} ticks, {r['timeouts']} time-outs, done values "
          f"{np.unique(r['done']).tolist()}, action shares {share}{extra}")


# --------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("case", ev.PARITY_CASES, ids=repr)
def test_one_launch_evaluation_against_the_replay(case):
    """E = 1501 under the host's geometry: outputs, trace and RNG words equal the replay bit for bit; nothing else is
    written (the byte image of every env array, reset copy, pool, pool RNG and the packed policy is unchanged; the
    surplus rows of the outputs and the trace rows after a replica's end keep their sentinels; greedy: the RNG words
    too).  (64, None), (128, 3) (three trips of the grid-stride loop) and the idle-block geometry are byte-identical to
    the host's."""
    L = _Launch(case)
    before = _image(L.w, extra=[L.packed])
    got = L.run("product")
    _same_image(before, _image(L.w, extra=[L.packed]), case.name)
    r = L.check_against_replay(got, case.name)
    if case.greedy:
        EQ(got["words"], L.words0, "a greedy evaluation leaves the RNG words alone")
    else:
        assert (got["words"][4:] != L.words0[4:]).all()
    assert (r["done"] > 0).all() and len(r["end_ticks"]) >= 3 and r["timeouts"] > 0
    assert case.env != "mountain_car" or (r["done"] == 2).sum() >= 50
    for geom in ev.GEOMETRIES:
        threads, blocks, trips = cc.geometry(case.E, geom)
        assert geom != (128, 3) or trips >= 3
        other = L.run(geom)
        for key in got:
            assert other[key].tobytes() == got[key].tobytes(), (case.name, geom, key)
    _line(case, r)


@pytest.mark.parametrize("case", ev.SMALL_CASES + ev.RESIDUE_CASES, ids=repr)
def test_small_sizes_and_start_timesteps(case):
    """E = 1 and E = 65 under the host's own geometry; and E = 1501 with per-replica start timesteps row % 4: the
    time-out arrives that much sooner"""
    L = _Launch(case)
    got = L.run("product")
    r = L.check_against_replay(got, case.name)
    assert (r["done"] > 0).all()
    if case.timesteps == "residue":
        rows = np.arange(case.E) % 4
        assert (((r["steps"] + rows == case.T) & (r["done"] == 1))[rows > 0]).sum() >= 20
    _line(case, r)


@pytest.mark.parametrize("case", [c for c in ev.PARITY_CASES if c.hidden == 32], ids=repr)
def test_only_the_first_episode_counts(case):
    """`ticks = episode_length + 7` gives byte-identical outputs to `ticks = episode_length` (no second episode); with
    `ticks = episode_length - 5` the unfinished replicas report done 0 and steps == ticks, the finished ones what the
    full launch reports"""
    E, T = case.E, case.T
    rows = T + 7
    full = _Launch(case, ticks=T, trace_rows=rows).run()
    long = _Launch(case, ticks=T + 7, trace_rows=rows).run()
    for key in full:
        assert long[key].tobytes() == full[key].tobytes(), (case.name, key)
    L = _Launch(case, ticks=T - 5, trace_rows=rows)
    short = L.run()
    r = L.check_against_replay(short, case.name)
    unfinished = short["done"][:E] == 0
    assert 20 <= unfinished.sum() < E and (short["steps"][:E][unfinished] == T - 5).all()
    assert (full["steps"][:E][unfinished] > T - 5).all()
    for key in ("reward_sum", "steps", "done"):
        EQ(short[key][:E][~unfinished], full[key][:E][~unfinished], (case.name, key))
    EQ(short["trace"][: T - 5], full["trace"][: T - 5], case.name)
    _line(case, r, f"; {int(unfinished.sum())} replicas unfinished after {T - 5} ticks")


@pytest.mark.parametrize("case", [c for c in ev.PARITY_CASES if c.mode == "sampled"], ids=repr)
@pytest.mark.parametrize("what", ["other width", "nine actions", "null policy"])
def test_guard_returns_without_touching_memory(case, what):
    """`hidden` of the other width, n_actions = 9, or a null policy: every byte, the outputs, the trace and the RNG words
    included, is unchanged"""
    L = _Launch(case)
    args = list(L.args)
    tail = len(args) - N_TAIL
    assert args[tail] is L.sampler.rng_state and args[tail + 4] is L.packed and args[-1] is L.trace
    if what == "other width":
        args[tail + 5] = np.int32(96 - case.hidden)
    elif what == "nine actions":
        args[tail + 1] = np.int32(9)
    else:
        args[tail + 4] = np.uint64(0)
    before = _image(L.w, extra=[L.packed])
    got = L.run("product", args=args)
    _same_image(before, _image(L.w, extra=[L.packed]), (case.name, what))
    E = case.E
    EQ(got["reward_sum"], np.full(E + ev.SURPLUS, ev.SENTINEL_F), what)
    EQ(got["steps"], np.full(E + ev.SURPLUS, ev.SENTINEL_I), what)
    EQ(got["done"], np.full(E + ev.SURPLUS, ev.SENTINEL_I), what)
    EQ(got["trace"], np.full(got["trace"].shape, ev.SENTINEL_I), what)
    EQ(got["words"], L.words0, what)


# -------------------------------------------------------------------------------------------- HipEvaluateAccumulate
@pytest.mark.parametrize("N", ev.ACC_AGENTS)
@pytest.mark.parametrize("threads,blocks", [(64, 3), (256, None)])
def test_accumulate_kernel_against_its_numpy_model(N, threads, blocks):
    """E = 130, 12 ticks, one launch per tick on synthetic rewards / done flags (done on tick 0, never done, done twice,
    done value 2): reward sums and end ticks equal the numpy model bit for bit; blocks of 64 threads on a grid of 3
    (many trips, replicas split across blocks and trips at N = 105) and blocks of 256"""
    from tests.hip_harness import make_wrapper, require_gpu
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv

    require_gpu()
    fm = make_wrapper(CUDAClassicControlCartPoleEnv(episode_length=10, seed=1), 4).cuda_function_manager
    fm.initialize_functions(["HipEvaluateAccumulate"])
    fn = fm.get_function("HipEvaluateAccumulate")
    E, ticks = ev.ACC_E, ev.ACC_TICKS
    rewards, done = ev.accumulate_inputs(N)
    want_sum, want_end = ev.accumulate_model(rewards, done)
    total = torch.zeros((E + ev.SURPLUS, N), dtype=torch.float32, device="cuda")
    total[E:] = float(ev.SENTINEL_F)
    end = torch.full((E + ev.SURPLUS,), -1, dtype=torch.int32, device="cuda")
    end[E:] = int(ev.SENTINEL_I)
    grid = blocks if blocks is not None else -(-E * N // threads)
    for k in range(ticks):
        r_k, d_k = torch.from_numpy(rewards[k]).cuda(), torch.from_numpy(done[k]).cuda()
        fn(r_k, d_k, total, end, np.int32(k), np.int32(N), np.int32(E), block=(threads, 1, 1), grid=(grid, 1), shared=0)
        torch.cuda.synchronize()
    EQ(total[:E].cpu().numpy(), want_sum)
    EQ(end[:E].cpu().numpy(), want_end)
    EQ(total[E:].cpu().numpy(), np.full((ev.SURPLUS, N), ev.SENTINEL_F))
    EQ(end[E:].cpu().numpy(), np.full(ev.SURPLUS, ev.SENTINEL_I))


# --------------------------------------------------------------------------------------------------------- trainer
def _trainer(name, overrides, tmp_path):
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    overrides = json.loads(json.dumps(overrides))
    overrides.setdefault("saving", {"metrics_log_freq": 1, "model_params_save_freq": 0})
    torch.manual_seed(0)
    return setup_trainer(name, overrides, results_dir=str(tmp_path), verbose=False)


def _env_image(tr):
    from warp_drive_amd.managers import hip_driver as drv

    out = {}
    for name, p in tr.w.cuda_data_manager._device_data_pointer.items():
        if "_batch" not in name and int(p.nbytes) > 0:
            buf = np.zeros(int(p.nbytes), np.uint8)
            drv.memcpy_dtoh(buf, p)
            out[name] = buf.tobytes()
    torch.cuda.synchronize()
    return out


def _check_state_after(tr, ep_sum, ep_cnt):
    """the envs as reset_all_envs() leaves them, `_ep_reward` zero, `_ep_sum` / `_ep_cnt` untouched"""
    after = _env_image(tr)
    tr.w.reset_all_envs()
    torch.cuda.synchronize()
    reset = _env_image(tr)
    for name in after:   # (a second reset changes nothing: every array a reset restores already held its start value)
        assert after[name] == reset[name], name
    for pol in tr.policies:
        assert float(tr._ep_reward[pol].abs().max()) == 0.0
        EQ(tr._ep_sum[pol].cpu().numpy(), ep_sum[pol])
    EQ(tr._ep_cnt.cpu().numpy(), ep_cnt)


def test_trainer_evaluates_cartpole_in_one_launch(tmp_path):
    """single_cartpole, [32, 32], 70 replicas, after two training iterations: the path is "one launch"; two greedy calls
    return identical arrays; a greedy call leaves the sampler's RNG words alone and a sampled one advances every epoch
    word by the replica's steps; shapes and dtypes; the state after the call"""
    E, T = 70, 40
    tr = _trainer("single_cartpole", {"trainer": {"num_envs": E, "train_batch_size": E * 10, "num_episodes": 500, "seed": 3},
                                      "env": {"episode_length": T}}, tmp_path)
    assert tr._batch_rollout is not None
    tr.train(2)
    ep_sum = {p: tr._ep_sum[p].cpu().numpy().copy() for p in tr.policies}
    ep_cnt = tr._ep_cnt.cpu().numpy().copy()
    words = _words(tr.sampler.rng_state, E)
    r1, s1 = tr.evaluate_episodes(use_argmax=True)
    assert tr.evaluation_path == "one launch"
    EQ(_words(tr.sampler.rng_state, E), words)
    _check_state_after(tr, ep_sum, ep_cnt)
    r2, s2 = tr.evaluate_episodes(use_argmax=True)
    assert set(r1) == set(s1) == {"shared"}
    assert r1["shared"].dtype == np.float32 and r1["shared"].shape == (E, 1)
    assert s1["shared"].dtype == np.int32 and s1["shared"].shape == (E,)
    EQ(r1["shared"], r2["shared"]), EQ(s1["shared"], s2["shared"])
    EQ(r1["shared"][:, 0], s1["shared"].astype(F32))   # Cartpole pays 1 per tick, the terminal tick included
    assert (s1["shared"] >= 1).all() and (s1["shared"] <= T).all()
    r3, s3 = tr.evaluate_episodes()
    assert tr.evaluation_path == "one launch"
    after = _words(tr.sampler.rng_state, E)
    EQ(after[:4], words[:4]), EQ(after[4:], words[4:] + s3["shared"].astype(np.uint32))
    EQ(r3["shared"][:, 0], s3["shared"].astype(F32))
    _check_state_after(tr, ep_sum, ep_cnt)
    tr.train(1)   # training goes on afterwards
    tr.graceful_close()


_GW_SMALL_POLICIES = {p: {"to_train": True, "algorithm": "A2C", "vf_loss_coeff": 1, "entropy_coeff": 0.05, "gamma": 0.98,
                          "lr": 0.001, "model": {"type": "fully_connected", "fc_dims": [32, 32], "model_ckpt_filepath": ""}}
                      for p in ("runner", "tagger")}
_PER_TICK = {
    # (training is one launch per batch of HipTagGridWorldRollout_N5_H32, which has no Evaluate entry: the single-tick
    # engine is built on first use)
    "tag_gridworld_n5_rollout": ("tag_gridworld", {"trainer": {"num_envs": 50, "train_batch_size": 50 * 25, "num_episodes": 50},
                                                   "env": {"episode_length": 30}, "policy": _GW_SMALL_POLICIES}),
    "tag_gridworld": ("tag_gridworld", {"trainer": {"num_envs": 50, "train_batch_size": 50 * 25, "num_episodes": 50},
                                        "env": {"episode_length": 30}}),
    "tag_continuous": ("tag_continuous", {"trainer": {"num_envs": 64, "train_batch_size": 64 * 20, "num_episodes": 200},
                                          "env": {"num_runners": 20, "episode_length": 30, "num_other_agents_observed": 6}}),
    # (no fused tick: sampler, step and reset_only_done_envs() as separate launches)
    "tag_gridworld_unfused": ("tag_gridworld", {"trainer": {"num_envs": 50, "train_batch_size": 50 * 25, "num_episodes": 50,
                                                            "fused_rollout": False}, "env": {"episode_length": 30}}),
    "cartpole": ("single_cartpole", {"trainer": {"num_envs": 70, "train_batch_size": 70 * 10, "num_episodes": 500,
                                                 "fused_rollout_policy": False}, "env": {"episode_length": 40}}),
}


@pytest.mark.parametrize("config", sorted(_PER_TICK))
@pytest.mark.parametrize("mode", ev.MODES)
def test_trainer_evaluates_per_tick(config, mode, tmp_path):
    """the path is "per tick", and the result equals, bit for bit, a host loop in the reference's form from the same seed:
    per tick the same launches, rewards and done flags pulled and accumulated in numpy under the first-episode mask.
    Greedy: the pulled `sampled_actions` are np.argmax of the pulled probabilities on every tick."""
    name, ov = _PER_TICK[config]
    tr = _trainer(name, ov, tmp_path)
    greedy = mode == "greedy"
    E, N, T = tr.num_envs, tr.w.n_agents, int(tr.w.episode_length)
    assert N == (5 if config.startswith("tag_gridworld") else N)
    assert tr._evaluation_engine().fused == (config != "tag_gridworld_unfused")
    assert (tr._batch_rollout is not None) == (config == "tag_gridworld_n5_rollout")
    assert (tr._evaluation_engine() is tr.engine) == (config != "tag_gridworld_n5_rollout")
    ep_sum = {p: tr._ep_sum[p].cpu().numpy().copy() for p in tr.policies}
    ep_cnt = tr._ep_cnt.cpu().numpy().copy()
    seed = 1234
    tr.sampler.init_random(seed=seed)
    rewards, steps = tr.evaluate_episodes(use_argmax=greedy)
    assert tr.evaluation_path == "per tick"
    _check_state_after(tr, ep_sum, ep_cnt)
    # ---- the reference's form: pull per tick, accumulate on the host
    tr.sampler.init_random(seed=seed)
    tr.w.reset_all_envs()
    engine = tr._evaluation_engine()
    total, count, live = np.zeros((E, N), F32), np.zeros(E, np.int32), np.ones(E, bool)
    for k in range(T):
        tr._policy_probabilities()
        pulled = [p.cpu().numpy().copy() for p in tr.probs]
        if greedy:
            tr._greedy_probabilities_()
        engine.run(1)
        torch.cuda.synchronize()
        rew, done = tr.rewards.cpu().numpy().reshape(E, N), tr.done.cpu().numpy()
        if greedy:
            acts = tr.actions.cpu().numpy().reshape(E, N, -1)
            for h, p in enumerate(pulled):
                EQ(acts[:, :, h], np.argmax(p, axis=-1).astype(acts.dtype), (config, "tick", k, "head", h))
        total[live] = (total[live] + rew[live]).astype(F32)
        count[live] += 1
        live &= ~(done != 0)
        if not engine.fused:
            tr.w.reset_only_done_envs()
    assert not live.any()   # the time-out ends every episode
    for pol in tr.policies:
        ids = tr.policy_map[pol]
        assert rewards[pol].dtype == np.float32 and rewards[pol].shape == (E, len(ids))
        assert steps[pol].dtype == np.int32 and steps[pol].shape == (E,)
        EQ(rewards[pol], total[:, ids], (config, pol))
        EQ(steps[pol], count, (config, pol))
    print(f"{config} {mode}: steps {count.min()} .. {count.max()}, mean reward per policy "
          f"{ {p: round(float(rewards[p].mean()), 3) for p in tr.policies} }")
    tr.graceful_close()


def test_greedy_evaluation_of_a_trained_cartpole_policy(tmp_path):
    """the settings of tests/test_gpu_learning.py::test_cartpole_learns["one launch per batch"]: after 300 iterations the
    greedy evaluation's mean episodic reward is at least 3 x the first iterations' training value (that test's own bar)"""
    ov = {"trainer": {"num_envs": 1000, "train_batch_size": 1000 * 50, "num_episodes": 10 ** 6, "seed": 7},
          "env": {"episode_length": 200}, "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0}}
    tr = _trainer("single_cartpole", ov, tmp_path)
    assert tr._batch_rollout is not None
    tr.train(300)
    curve = [json.loads(line)["shared"]["Mean episodic reward"] for line in open(os.path.join(str(tmp_path), "results.json"))]
    first = float(np.mean(curve[:3]))
    greedy, gsteps = tr.evaluate_episodes(use_argmax=True)
    assert tr.evaluation_path == "one launch"
    sampled, _ = tr.evaluate_episodes()
    tr.graceful_close()
    g, s = float(greedy["shared"].mean()), float(sampled["shared"].mean())
    print(f"cartpole after 300 iterations: training value {first:.1f} (first iteration {curve[0]:.1f}) -> {np.mean(curve[-10:]):.1f}; "
          f"evaluate_episodes greedy {g:.1f}, sampled {s:.1f} (episodes of at most 200 ticks)")
    assert 15.0 <= first <= 30.0, first
    assert g >= 3.0 * first and g >= 3.0 * curve[0], (g, first, curve[0])
    EQ(greedy["shared"][:, 0], gsteps["shared"].astype(F32))
