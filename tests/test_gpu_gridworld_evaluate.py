"""TagGridWorld's one-launch evaluation on the MI355X: HipTagGridWorldEvaluate_N5_H<32|64> launched directly (parity with
the host replay of tests/gridworld_evaluate.py that follows the device's recorded actions, under three grids; nothing but
the outputs is written; small sizes and the last entry of the quotient table; only the first episode counts; the guard)
and the trainer on that path under `fused_rollout_policy: "all"`.  The cases are sized on the host by
tests/test_gridworld_evaluate_host.py.  `pytest -s` prints one line per case."""
import json

import numpy as np
import pytest
import torch

from tests import gridworld_evaluate as gev

pytestmark = pytest.mark.gpu

F32 = np.float32
N = gev.N
N_TAIL = 11   # arguments of an Evaluate entry after the step's: rng, tag, ticks, action table, tagger, runner, use_argmax,
#               reward_sum, steps, done, trace
I_FULL_OBS, I_BOUNDARY, I_AGENTS = 10, 11, 14   # positions of three scalars among the step's arguments


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


def _image(w, extra=()):
    """the byte image of every device array of the env's data manager (env arrays, their reset copies, the
    placeholders) and of `extra` tensors"""
    from warp_drive_amd.managers import hip_driver as drv

    out = {}
    for name, p in w.cuda_data_manager._device_data_pointer.items():
        if int(p.nbytes) > 0:
            buf = np.zeros(int(p.nbytes), np.uint8)
            drv.memcpy_dtoh(buf, p)
            out[name] = buf
    torch.cuda.synchronize()
    for i, t in enumerate(extra):
        out[f"<extra {i}>"] = t.cpu().numpy().copy()
    return out


def _same_image(a, b, tag):
    assert set(a) == set(b)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), (tag, name)


class _Launch:
    """one case set up on the device: per-replica start positions, observation rows, timesteps and epoch words written,
    the outputs and the trace pre-filled with sentinels (three surplus rows each)"""

    def __init__(self, case, ticks=None, trace_rows=None):
        from tests.hip_harness import OBS, make_wrapper, require_gpu
        from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorld
        from warp_drive_amd.managers.function_manager import HIPSampler

        require_gpu()
        self.case, E = case, case.E
        self.ticks = case.T if ticks is None else int(ticks)
        self.w = w = make_wrapper(CUDATagGridWorld(seed=27, **case.env_config()), E)
        orc = case.oracle()
        _put(w, "loc_x", orc.loc_x)
        _put(w, "loc_y", orc.loc_y)
        _put(w, "_timestep_", orc.timestep)
        _put(w, "_done_", np.zeros(E, np.int32))
        _put(w, OBS, orc.obs.astype(F32))
        self.sampler = HIPSampler(w.cuda_function_manager)
        self.sampler.init_random(seed=gev.SAMPLER_SEED)
        self.words0 = _words(self.sampler.rng_state, E * N)
        assert (self.words0[:2] == np.array(gev.seed_words(gev.SAMPLER_SEED), np.uint32)).all()
        self.words0[4:] = case.start_epochs().reshape(-1)
        self.packed_np = case.policies()[1]
        self.packed = [torch.from_numpy(p).cuda() for p in self.packed_np]
        rows = (self.ticks if trace_rows is None else trace_rows) + gev.SURPLUS
        self.out = {"reward_sum": torch.empty((E + gev.SURPLUS, N), dtype=torch.float32, device="cuda"),
                    "steps": torch.empty(E + gev.SURPLUS, dtype=torch.int32, device="cuda"),
                    "done": torch.empty(E + gev.SURPLUS, dtype=torch.int32, device="cuda")}
        self.trace = torch.empty((rows, E, N), dtype=torch.int32, device="cuda")
        assert w.env.has_live_policy_evaluate(case.hidden, 5)
        self.fn, self.args, self.block, self.grid, self.shared = w.env.evaluate_launch(
            self.sampler, policy=(self.packed, case.hidden), use_argmax=case.greedy, outputs=self.out,
            action_trace=self.trace, ticks=self.ticks)
        assert self.fn.name == f"HipTagGridWorldEvaluate_N5_H{case.hidden}"
        assert self.block == (64, 1, 1) and self.grid == (-(-E // gev.EPB), 1)
        assert self.shared == w.env.live_policy_evaluate_lds_bytes(case.hidden) <= 64 * 1024

    def rewind(self):
        self.out["reward_sum"].fill_(float(gev.SENTINEL_F))
        self.out["steps"].fill_(int(gev.SENTINEL_I))
        self.out["done"].fill_(int(gev.SENTINEL_I))
        self.trace.fill_(int(gev.SENTINEL_I))
        _put_words(self.sampler.rng_state, self.words0)

    def run(self, geom="product", args=None):
        """-> {"reward_sum", "steps", "done", "trace", "words"} pulled after one launch from the rewound start"""
        self.rewind()
        blocks = gev.grid_blocks(self.case.E, geom)
        self.fn(*(self.args if args is None else args), block=(64, 1, 1), grid=(blocks, 1), shared=self.shared)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in self.out.items()}
        got["trace"] = self.trace.cpu().numpy()
        got["words"] = _words(self.sampler.rng_state, self.case.E * N)
        return got

    def check_against_replay(self, got, tag):
        """the replay follows the recorded actions (each the host's, or its decision's margin below 2e-6); then bit for
        bit: the three outputs, the trace rows up to each replica's end (-1 after it and in the surplus rows), the RNG
        words (sampled: every agent's epoch += its replica's steps; greedy: untouched); the surplus output rows keep their
        sentinels; at most 2 + decisions // 50000 decisions lie inside the window"""
        case, E = self.case, self.case.E
        r = gev.replay(case, ticks=self.ticks, trace=got["trace"], packed=self.packed_np)
        for key in ("reward_sum", "steps", "done"):
            EQ(got[key][:E], r[key], (tag, key))
        EQ(got["reward_sum"][E:], np.full((gev.SURPLUS, N), gev.SENTINEL_F), tag)
        EQ(got["steps"][E:], np.full(gev.SURPLUS, gev.SENTINEL_I), tag)
        EQ(got["done"][E:], np.full(gev.SURPLUS, gev.SENTINEL_I), tag)
        want_trace = np.full(got["trace"].shape, gev.SENTINEL_I, np.int32)
        want_trace[: self.ticks] = r["actions"]   # (-1 where the replica no longer ran: the sentinel)
        EQ(got["trace"], want_trace, (tag, "trace"))
        want_words = self.words0.copy()
        want_words[4:] = r["epochs"].reshape(-1)
        EQ(got["words"], want_words, (tag, "rng words"))
        assert r["near"] <= case.near_cap(r["decisions"]), (tag, r["near"], r["decisions"])
        return r


def _line(case, r, extra=""):
    ok, fig = gev.vacuity(case, r)
    print(f"{case.name}: {fig}, {r['followed']} decisions followed the device{extra}")


# --------------------------------------------------------------------------------------------------------- parity
@pytest.mark.parametrize("case", gev.PARITY_CASES, ids=repr)
def test_one_launch_evaluation_against_the_replay(case):
    """E = 257 under the host's geometry: outputs, trace and RNG words equal the replay bit for bit; nothing else is
    written (the byte image of every env array, reset copy and placeholder and of the two packed policies is unchanged;
    the surplus rows of the outputs and the trace rows after a replica's end keep their sentinels; greedy: the RNG words
    too).  A grid of 3 blocks (8 trips of the stride loop) and a grid with two idle blocks are byte-identical to the
    host's."""
    L = _Launch(case)
    before = _image(L.w, extra=L.packed)
    got = L.run("product")
    _same_image(before, _image(L.w, extra=L.packed), case.name)
    r = L.check_against_replay(got, case.name)
    if case.greedy:
        EQ(got["words"], L.words0, "a greedy evaluation leaves the RNG words alone")
    else:
        assert (got["words"][4:] != L.words0[4:]).all()
    assert (r["done"] == 1).all() and gev.vacuity(case, r)[0], gev.vacuity(case, r)[1]
    for geom in gev.GEOMETRIES[1:]:
        blocks = gev.grid_blocks(case.E, geom)
        assert geom != 3 or -(-case.E // (blocks * gev.EPB)) == 8
        other = L.run(geom)
        for key in got:
            assert other[key].tobytes() == got[key].tobytes(), (case.name, geom, key)
    _line(case, r)


@pytest.mark.parametrize("case", gev.SMALL_CASES + gev.BOUND_CASES, ids=repr)
def test_small_sizes_and_the_table_bound(case):
    """E = 1, E = 13 (a second group of one replica) and grid_length = 63 with T = 12 (live agents stand on coordinate
    63: the last entry of the quotient table) under the host's own geometry"""
    L = _Launch(case)
    before = _image(L.w, extra=L.packed)
    got = L.run("product")
    _same_image(before, _image(L.w, extra=L.packed), case.name)
    r = L.check_against_replay(got, case.name)
    assert (r["done"] == 1).all()
    assert case.L != 63 or gev.reaches_bound(case, r)
    _line(case, r)


@pytest.mark.parametrize("case", [c for c in gev.PARITY_CASES if c.hidden == 32 and c.L == 10], ids=repr)
def test_only_the_first_episode_counts(case):
    """`ticks = episode_length + 7` gives byte-identical outputs to `ticks = episode_length` (no second episode); with
    `ticks = episode_length - 5` the unfinished replicas report done 0 and steps == ticks, the finished ones what the
    full launch reports"""
    E, T = case.E, case.T
    rows = T + 7
    full = _Launch(case, ticks=T, trace_rows=rows).run()
    L = _Launch(case, ticks=T + 7, trace_rows=rows)
    long = L.run()
    for key in full:
        assert long[key].tobytes() == full[key].tobytes(), (case.name, key)
    L.check_against_replay(long, (case.name, "T + 7"))
    L = _Launch(case, ticks=T - 5, trace_rows=rows)
    short = L.run()
    r = L.check_against_replay(short, (case.name, "T - 5"))
    unfinished = short["done"][:E] == 0
    assert 20 <= unfinished.sum() < E and (short["steps"][:E][unfinished] == T - 5).all()
    assert (full["steps"][:E][unfinished] > T - 5).all()
    for key in ("reward_sum", "steps", "done"):
        EQ(short[key][:E][~unfinished], full[key][:E][~unfinished], (case.name, key))
    EQ(short["trace"][: T - 5], full["trace"][: T - 5], case.name)
    _line(case, r, f"; {int(unfinished.sum())} replicas unfinished after {T - 5} ticks")


@pytest.mark.parametrize("case", [c for c in gev.PARITY_CASES if c.mode == "sampled" and c.L == 10], ids=repr)
@pytest.mark.parametrize("what", ["null policy", "four agents", "partial observations", "boundary 64"])
def test_guard_returns_without_touching_memory(case, what):
    """a null policy pointer, n_agents = 4, use_full_observation = 0 or world_boundary = 64: every byte, the outputs, the
    trace and the RNG words included, is unchanged"""
    L = _Launch(case)
    args = list(L.args)
    tail = len(args) - N_TAIL
    assert args[tail] is L.sampler.rng_state and args[tail + 4] is L.packed[0] and args[tail + 5] is L.packed[1]
    assert args[-1] is L.trace
    assert int(args[I_FULL_OBS]) == 1 and int(args[I_BOUNDARY]) == case.L and int(args[I_AGENTS]) == N
    if what == "null policy":
        args[tail + 5 if case.hidden == 64 else tail + 4] = np.uint64(0)
    elif what == "four agents":
        args[I_AGENTS] = np.int32(4)
    elif what == "partial observations":
        args[I_FULL_OBS] = np.int32(0)
    else:
        args[I_BOUNDARY] = np.int32(64)
    before = _image(L.w, extra=L.packed)
    got = L.run("product", args=args)
    _same_image(before, _image(L.w, extra=L.packed), (case.name, what))
    E = case.E
    EQ(got["reward_sum"], np.full((E + gev.SURPLUS, N), gev.SENTINEL_F), what)
    EQ(got["steps"], np.full(E + gev.SURPLUS, gev.SENTINEL_I), what)
    EQ(got["done"], np.full(E + gev.SURPLUS, gev.SENTINEL_I), what)
    EQ(got["trace"], np.full(got["trace"].shape, gev.SENTINEL_I), what)
    EQ(got["words"], L.words0, what)


# --------------------------------------------------------------------------------------------------------- trainer
_GW_SMALL_POLICIES = {p: {"to_train": True, "algorithm": "A2C", "vf_loss_coeff": 1, "entropy_coeff": 0.05, "gamma": 0.98,
                          "lr": 0.001, "model": {"type": "fully_connected", "fc_dims": [32, 32], "model_ckpt_filepath": ""}}
                      for p in ("runner", "tagger")}


def _trainer(trainer_overrides, tmp_path):
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    E, T = 50, 30
    overrides = {"trainer": dict({"num_envs": E, "train_batch_size": E * 25, "num_episodes": 50}, **trainer_overrides),
                 "env": {"episode_length": T}, "policy": json.loads(json.dumps(_GW_SMALL_POLICIES)),
                 "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0}}
    torch.manual_seed(0)
    return setup_trainer("tag_gridworld", overrides, results_dir=str(tmp_path), verbose=False)


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


def _direct(tr, use_argmax, words):
    """a direct evaluate_launch from the RNG words `words` with the trainer's packed weights, after reset_all_envs():
    (reward_sum [E, 5], steps [E], done [E])"""
    E = tr.num_envs
    _put_words(tr.sampler.rng_state, words)
    tr.w.reset_all_envs()
    br = tr._batch_rollout
    packed = [br["packed"]["tagger"], br["packed"]["runner"]]
    out = {"reward_sum": torch.zeros((E, N), dtype=torch.float32, device="cuda"),
           "steps": torch.zeros(E, dtype=torch.int32, device="cuda"), "done": torch.zeros(E, dtype=torch.int32, device="cuda")}
    fn, args, block, grid, shared = tr.w.env.evaluate_launch(tr.sampler, policy=(packed, 32), use_argmax=use_argmax,
                                                             outputs=out)
    fn(*args, block=block, grid=grid, shared=shared)
    torch.cuda.synchronize()
    return tuple(out[k].cpu().numpy() for k in ("reward_sum", "steps", "done"))


def test_trainer_evaluates_gridworld_in_one_launch(tmp_path):
    """tag_gridworld, [32, 32] policies, `fused_rollout_policy: "all"`, 50 replicas, T = 30, after two training
    iterations: the path is "one launch"; the result equals a direct evaluate_launch with the same packed weights from
    the same RNG words bit for bit; keys, shapes and dtypes; two greedy calls are identical; a greedy call leaves the
    sampler's RNG words alone and a sampled one advances every agent's word by its replica's steps; the state after the
    call; training goes on afterwards"""
    E, T = 50, 30
    tr = _trainer({"fused_rollout_policy": "all"}, tmp_path)
    assert tr._batch_rollout is not None and tr.engine.step_kernel_name == "HipTagGridWorldRollout_N5_H32"
    assert list(tr.policy_map["tagger"]) == [0, 1, 2, 3] and list(tr.policy_map["runner"]) == [4]
    tr.train(2)
    ep_sum = {p: tr._ep_sum[p].cpu().numpy().copy() for p in tr.policies}
    ep_cnt = tr._ep_cnt.cpu().numpy().copy()
    words = _words(tr.sampler.rng_state, E * N)
    r1, s1 = tr.evaluate_episodes(use_argmax=True)
    assert tr.evaluation_path == "one launch"
    assert getattr(tr, "_eval_engine", None) is None   # no second engine is built just to evaluate
    EQ(_words(tr.sampler.rng_state, E * N), words)
    _check_state_after(tr, ep_sum, ep_cnt)
    r2, s2 = tr.evaluate_episodes(use_argmax=True)
    assert set(r1) == set(s1) == {"tagger", "runner"}
    for pol, n in (("tagger", 4), ("runner", 1)):
        assert r1[pol].dtype == np.float32 and r1[pol].shape == (E, n)
        assert s1[pol].dtype == np.int32 and s1[pol].shape == (E,)
        EQ(r1[pol], r2[pol]), EQ(s1[pol], s2[pol])
        assert (s1[pol] >= 1).all() and (s1[pol] <= T).all()
    want, want_steps, want_done = _direct(tr, True, words)
    assert (want_done == 1).all()
    EQ(r1["tagger"], want[:, :4]), EQ(r1["runner"], want[:, 4:]), EQ(s1["tagger"], want_steps), EQ(s1["runner"], want_steps)
    EQ(_words(tr.sampler.rng_state, E * N), words)
    r3, s3 = tr.evaluate_episodes()
    assert tr.evaluation_path == "one launch"
    after = _words(tr.sampler.rng_state, E * N)
    EQ(after[:4], words[:4])
    EQ(after[4:], words[4:] + np.repeat(s3["tagger"].astype(np.uint32), N))
    _check_state_after(tr, ep_sum, ep_cnt)
    want, want_steps, want_done = _direct(tr, False, words)
    EQ(r3["tagger"], want[:, :4]), EQ(r3["runner"], want[:, 4:]), EQ(s3["tagger"], want_steps), EQ(s3["runner"], want_steps)
    EQ(_words(tr.sampler.rng_state, E * N), after)
    print(f"greedy: steps {s1['tagger'].min()} .. {s1['tagger'].max()}, mean reward tagger {r1['tagger'].mean():.3f} runner "
          f"{r1['runner'].mean():.3f}; sampled: steps {s3['tagger'].min()} .. {s3['tagger'].max()}, "
          f"{len(np.unique(s3['tagger']))} distinct")
    tr.train(1)   # training goes on afterwards
    tr.graceful_close()


def test_trainer_without_all_keeps_the_per_tick_evaluation(tmp_path):
    """the same config without `fused_rollout_policy: "all"`: the training rollout is one launch all the same, the
    evaluation is "per tick" """
    tr = _trainer({}, tmp_path)
    assert tr._batch_rollout is not None and tr.engine.step_kernel_name == "HipTagGridWorldRollout_N5_H32"
    assert tr.w.env.has_live_policy_evaluate(32, 5) and tr.w.env.EVALUATE_POLICY_OPT_IN
    tr.evaluate_episodes(use_argmax=True)
    assert tr.evaluation_path == "per tick"
    tr.graceful_close()
