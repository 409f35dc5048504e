"""One-launch evaluation of the Box envs on the device: the HipClassicControl<Pendulum|ContinuousMountainCar>
EnvEvaluate_A32 / _A64 entries (one episode of every replica in one launch with the deterministic actor inside the kernel,
csrc/kernels/classic_control.hip::cc_evaluate_actor_impl) against the pinned ...EnvTick entry, the kernel's guard, and
TrainerDDPG.evaluate_episodes / the evaluator metric on top of them.

Yardstick.  The entry records its means and actions; from the same start a second wrapper runs the Tick at one tick per
launch whose `probs` is row k of the recorded means (0 where the replica had already ended).  The host adds the Tick's
float32 rewards in tick order up to each replica's first done and keeps `ou_state` and the epoch word as they were right
after that tick.  Reward sum, steps, done code, every live row of the action trace, `ou_state` and the epoch words are
compared at tolerance 0; the recorded means, on the observations the yardstick held, are within the bound of
tests/test_gpu_classic_control_actor.py::_within_bound.  The cases live in tests/classic_control_actor_evaluate.py;
tests/test_classic_control_actor_evaluate_host.py sizes them on the host.  `pytest -s` prints one line per case.
(Written in round 16, in which no GPU could be had: docs/rounds/r16.md section 4.)"""
import json
import os

import numpy as np
import pytest

from tests import classic_control_actor as ca
from tests import classic_control_actor_evaluate as ae
from tests import classic_control_cases as cc
from tests import test_gpu_classic_control_actor as ta
from tests import test_gpu_classic_control_shapes as sh
from tests import test_gpu_evaluate as te

pytestmark = pytest.mark.gpu

F32 = np.float32
EQ = sh.EQ
OU = "sampled_actions_ou_state"
N_TAIL = 16   # rng, tag, ticks, packed, width, action_scale, action_bias, ou_state, damping, stddev, scale, reward_sum,
#               steps, done, mean_trace, action_trace


def ae_seed_words():
    from oracle.core_np import seed_words

    return seed_words(cc.SAMPLER_SEED)


class _Side:
    """one wrapper with its sampler and OU state, at the case's start"""

    def __init__(self, case):
        from warp_drive_amd.managers.function_manager import HIPSampler

        self.case, self.w = case, sh._wrapper(case)
        self.sampler = HIPSampler(self.w.cuda_function_manager)
        self.sampler.init_random(seed=cc.SAMPLER_SEED)
        self.w.cuda_data_manager.push_data_to_device(sh._ou_feed(case.E))
        self.state0, self.ts0 = case.start()
        self.obs0 = ca.host_obs(case.env, self.state0)
        self.words0 = sh._words(self.sampler.rng_state, case.E)
        assert (int(self.words0[0]), int(self.words0[1])) == ae_seed_words()
        self.words0[4:] = case.start_epochs()

    def start(self):
        from tests.hip_harness import ACT, OBS, REW

        w, E = self.w, self.case.E
        sh._put(w, "state", self.state0)
        sh._put(w, OBS, self.obs0)
        sh._put(w, "_timestep_", self.ts0)
        sh._put(w, "_done_", np.zeros(E, np.int32))
        sh._put(w, REW, np.full(E, -7.0, F32))
        sh._put(w, ACT, np.full(E, -1.0, F32))
        sh._put(w, OU, self.case.start_ou())
        sh._put_words(self.sampler.rng_state, self.words0)

    def ou(self):
        from tests.hip_harness import pull

        return pull(self.w, OU).reshape(-1).copy()

    def words(self):
        return sh._words(self.sampler.rng_state, self.case.E)


class _Launch(_Side):
    """the entry under test: outputs and traces with surplus elements / rows, pre-filled with sentinels"""

    def __init__(self, case):
        import torch

        super().__init__(case)
        E, T = case.E, case.ticks
        self.packed_np = case.actor()[1]
        self.packed = torch.from_numpy(self.packed_np).cuda()
        self.out = {"reward_sum": torch.empty(E + ae.SURPLUS, dtype=torch.float32, device="cuda"),
                    "steps": torch.empty(E + ae.SURPLUS, dtype=torch.int32, device="cuda"),
                    "done": torch.empty(E + ae.SURPLUS, dtype=torch.int32, device="cuda")}
        self.mean_trace = torch.empty((T + ae.SURPLUS, E), dtype=torch.float32, device="cuda")
        self.action_trace = torch.empty((T + ae.SURPLUS, E), dtype=torch.float32, device="cuda")
        assert self.w.env.has_live_actor_evaluate(case.hidden)
        actor = (self.packed, case.hidden, case.action_scale, case.action_bias)
        kw = dict(actor=actor, ou=case.ou_params, outputs=self.out, ticks=T)
        self.launch = self.w.env.evaluate_actor_launch(self.sampler, mean_trace=self.mean_trace,
                                                       action_trace=self.action_trace, **kw)
        self.launch_untraced = self.w.env.evaluate_actor_launch(self.sampler, **kw)
        fn, args, block, grid, shared = self.launch
        assert fn.name == f"{ca.ENTRY[case.env]}Evaluate_A{case.hidden}"
        assert shared == 4 * self.packed_np.size == 4 * ca.actor_weight_count(cc.OBS_DIM[case.env], case.hidden)
        assert block[0] <= cc.LAUNCH_BOUND and args[-1] is self.action_trace and args[-2] is self.mean_trace

    def run(self, geom="product", launch=None, args=None):
        """-> the outputs, traces, OU state and RNG words pulled after one launch from the case's start"""
        import torch

        self.start()
        self.out["reward_sum"].fill_(float(ae.SENTINEL_F))
        self.out["steps"].fill_(int(ae.SENTINEL_I))
        self.out["done"].fill_(int(ae.SENTINEL_I))
        self.mean_trace.fill_(float(ae.SENTINEL_F))
        self.action_trace.fill_(float(ae.SENTINEL_F))
        fn, largs, block, grid, shared = self.launch if launch is None else launch
        threads, blocks, _ = cc.geometry(self.case.E, geom, product=(block[0], grid[0]))
        assert threads <= cc.LAUNCH_BOUND
        fn(*(largs if args is None else args), block=(threads, 1, 1), grid=(blocks, 1), shared=shared)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in self.out.items()}
        got.update(mean_trace=self.mean_trace.cpu().numpy(), action_trace=self.action_trace.cpu().numpy(),
                   ou=self.ou(), words=self.words())
        return got

    def image(self):
        """every device array of the env's data manager but the OU state (env arrays, reset copies, the pool, the
        placeholders), the pool's RNG words and the packed actor"""
        img = te._image(self.w, extra=[self.packed])
        img.pop(OU, None)
        return img


def _yardstick(case, fed_means):
    """the Tick, one tick per launch at the host's geometry, on `fed_means` [ticks, E] -> reward_sum, steps, done,
    actions [ticks, E], live [ticks, E] (the replica ran tick k), obs [ticks, E, O] (the observation tick k's mean belongs
    to), ou and epoch words as right after each replica's last counted tick"""
    import torch
    from tests.hip_harness import ACT, OBS, REW, pull

    E, T = case.E, case.ticks
    y = _Side(case)
    y.w.env.ticks_per_launch = 1
    probs = torch.from_numpy(np.ascontiguousarray(fed_means, F32).reshape(T, E, 1, 1)).cuda()
    launches = [y.w.env.tick_launch(y.sampler, [probs[k]], y.w.env_resetter, ou_params=case.ou_params) for k in range(T)]
    assert all(l[0].name == ca.ENTRY[case.env] + "Tick" and l[4] == 0 for l in launches)
    y.start()
    running = np.ones(E, bool)
    total, steps, done = np.zeros(E, F32), np.zeros(E, np.int32), np.zeros(E, np.int32)
    ou_end, words_end = case.start_ou(), y.words0.copy()
    actions, live, obs = np.zeros((T, E), F32), np.zeros((T, E), bool), []
    for k, (fn, args, block, grid, shared) in enumerate(launches):
        obs.append(pull(y.w, OBS).reshape(E, -1).copy())
        fn(*args, block=block, grid=grid, shared=shared)
        torch.cuda.synchronize()
        rew, d = pull(y.w, REW).reshape(E), pull(y.w, "_done_").reshape(E)
        live[k], actions[k] = running, pull(y.w, ACT).reshape(E)
        total[running] = (total[running] + rew[running]).astype(F32)
        steps[running] += 1
        ou_end[running] = y.ou()[running]
        words_end[4:][running] = y.words()[4:][running]
        fin = running & (d > 0)
        done[fin] = d[fin]
        running = running & ~fin
    return {"reward_sum": total, "steps": steps, "done": done, "actions": actions, "live": live, "obs": np.stack(obs),
            "ou": ou_end, "words": words_end}


@pytest.mark.parametrize("case", ae.CASES, ids=repr)
def test_one_launch_evaluation_against_the_tick(case):
    """every case under the host's geometry against the yardstick at tolerance 0 (reward sum, steps, done code, the live
    rows of the action trace, `ou_state`, the epoch words); greedy: the RNG words and the non-zero `ou_state` pattern are
    unchanged and the actions are the means; trace rows after a replica's end, surplus rows and surplus output elements
    keep their sentinels; the env's arrays, the pool, its RNG words and the packed actor are byte-identical before and
    after; the live means are within round 15's bound.  The E = 700 parity cases also under 256 x 1 (three trips, the last
    partial), 64 x 3 and 64 threads with two idle blocks, byte-identical, and with null traces (the same outputs)."""
    E, T, H = case.E, case.ticks, case.hidden
    L = _Launch(case)
    L.start()
    before = L.image()
    got = L.run("product")
    te._same_image(before, L.image(), case.name)
    # ---- the sentinels
    for key, sentinel in (("reward_sum", ae.SENTINEL_F), ("steps", ae.SENTINEL_I), ("done", ae.SENTINEL_I)):
        EQ(got[key][E:], np.full(ae.SURPLUS, sentinel), (case.name, key, "surplus"))
    steps = got["steps"][:E]
    assert (steps >= 1).all() and (steps <= T).all()
    live = np.arange(T)[:, None] < steps[None, :]
    for key in ("mean_trace", "action_trace"):
        EQ(got[key][T:], np.full((ae.SURPLUS, E), ae.SENTINEL_F), (case.name, key, "surplus rows"))
        EQ(got[key][:T][~live], np.full(int((~live).sum()), ae.SENTINEL_F), (case.name, key, "rows after the end"))
        assert np.isfinite(got[key][:T][live]).all() and (got[key][:T][live] != ae.SENTINEL_F).all()
    # ---- the yardstick
    y = _yardstick(case, np.where(live, got["mean_trace"][:T], F32(0)))
    EQ(live, y["live"], (case.name, "live rows"))
    for key in ("reward_sum", "steps", "done"):
        EQ(got[key][:E], y[key], (case.name, key))
    EQ(got["action_trace"][:T][live], y["actions"][live], (case.name, "action trace"))
    EQ(got["ou"], y["ou"], (case.name, "ou_state"))
    EQ(got["words"], y["words"], (case.name, "RNG words"))
    if case.greedy:
        EQ(got["words"], L.words0, (case.name, "a greedy launch leaves the RNG words alone"))
        EQ(got["ou"], case.start_ou(), (case.name, "... and the OU state"))
        EQ(got["action_trace"][:T][live], got["mean_trace"][:T][live], (case.name, "the actions are the means"))
    else:
        EQ(got["words"][:4], L.words0[:4], case.name)
        EQ(got["words"][4:], L.words0[4:] + steps.astype(np.uint32), (case.name, "epoch += steps"))
        assert (got["ou"] != case.start_ou()).any()
        assert (got["action_trace"][:T][live] != got["mean_trace"][:T][live]).mean() > 0.9
    if T < case.T:
        unfinished = got["done"][:E] == 0
        assert unfinished.sum() >= E // 2 and (steps[unfinished] == T).all()
    else:
        assert (got["done"][:E] > 0).all()
    # ---- the means, on the observations the yardstick held
    ta._within_bound(got["mean_trace"][:T][live], L.packed_np, H, y["obs"][live], case.action_scale, case.action_bias,
                     case.name)
    ends = np.unique(steps[got["done"][:E] > 0])
    print(f"{case.name}: {int(live.sum())} live ticks, episodes end after {ends.min() if len(ends) else '-'} .. "
          f"{ends.max() if len(ends) else '-'} ticks ({len(ends)} different counts), done values "
          f"{np.unique(got['done'][:E]).tolist()}")
    if case not in ae.PARITY_CASES:
        return
    # ---- geometries, and null traces
    fn, args, block, grid, shared = L.launch
    for geom in ae.GEOMETRIES[1:]:
        threads, blocks, trips = cc.geometry(E, geom, product=(block[0], grid[0]))
        assert geom != (256, 1) or (trips == 3 and E % 256)
        other = L.run(geom)
        for key in got:
            assert other[key].tobytes() == got[key].tobytes(), (case.name, geom, key)
    fn2, args2, _, _, shared2 = L.launch_untraced
    assert fn2.name == fn.name and shared2 == shared and args2[-1] == 0 and args2[-2] == 0
    untraced = L.run("product", launch=L.launch_untraced)
    for key in ("reward_sum", "steps", "done", "ou", "words"):
        assert untraced[key].tobytes() == got[key].tobytes(), (case.name, "null traces", key)
    for key in ("mean_trace", "action_trace"):
        assert (untraced[key] == ae.SENTINEL_F).all(), (case.name, "null traces", key)


@pytest.mark.parametrize("env", ae.ENVS)
@pytest.mark.parametrize("what", ["other width", "null actor"])
def test_guard_returns_without_touching_memory(env, what):
    """the A32 entry launched with hidden = 64, or with a null actor (sampled mode): every output and trace keeps its
    sentinels, the RNG words, the OU state and every other array are unchanged"""
    case = ae.ActorEvalCase(env, 32, "sampled")
    L = _Launch(case)
    args = list(L.launch[1])
    tail = len(args) - N_TAIL
    assert args[tail] is L.sampler.rng_state and args[tail + 3] is L.packed and int(args[tail + 4]) == 32
    if what == "other width":
        args[tail + 4] = np.int32(64)
    else:
        args[tail + 3] = np.uint64(0)
    L.start()
    before = L.image()
    got = L.run("product", args=args)
    te._same_image(before, L.image(), (env, what))
    E = case.E
    EQ(got["reward_sum"], np.full(E + ae.SURPLUS, ae.SENTINEL_F), what)
    EQ(got["steps"], np.full(E + ae.SURPLUS, ae.SENTINEL_I), what)
    EQ(got["done"], np.full(E + ae.SURPLUS, ae.SENTINEL_I), what)
    for key in ("mean_trace", "action_trace"):
        EQ(got[key], np.full(got[key].shape, ae.SENTINEL_F), (what, key))
    EQ(got["words"], L.words0, what)
    EQ(got["ou"], case.start_ou(), what)


# -------------------------------------------------------------------------------------------------------- trainer
E_TR, T_EP = 64, 8


def _trainer(env, tmp_path, fused_evaluation=None, evaluator=None, scale=1.0):
    import torch
    from tests.hip_harness import require_gpu
    from warp_drive_amd.training.scripts.train import setup_trainer

    require_gpu()
    net = {"type": "fully_connected", "fc_dims": [32, 32], "model_ckpt_filepath": ""}
    policy = {"to_train": True, "algorithm": "DDPG", "clip_grad_norm": True, "max_grad_norm": 3, "gamma": 0.99, "tau": 0.05,
              "lr": {"actor": 0.001, "critic": 0.001}, "model": {"actor": dict(net), "critic": dict(net)}}
    trainer = {"num_envs": E_TR, "train_batch_size": E_TR * 6, "num_episodes": 10 ** 6, "seed": 3, "n_step": 5,
               "fused_rollout_policy": "all"}
    if fused_evaluation is not None:
        trainer["fused_evaluation"] = fused_evaluation
    if evaluator is not None:
        trainer["evaluator"] = evaluator
    ov = {"trainer": trainer, "policy": {"shared": policy},
          "sampler": {"params": {"damping": 0.15, "stddev": 0.2, "scale": scale}},
          "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0},
          "env": {"episode_length": T_EP, "reset_pool_size": 0, "seed": cc.ENV_SEED}}
    torch.manual_seed(3)
    return setup_trainer(f"single_{env}", ov, results_dir=str(tmp_path), verbose=False)


@pytest.mark.parametrize("env", ae.ENVS)
def test_trainer_evaluates_in_one_launch(env, tmp_path):
    """E = 64, a [32, 32] actor, `fused_rollout_policy: "all"`, `fused_evaluation: true`, episodes of 8 ticks, after two
    training iterations: the path is "one launch"; keys, shapes and dtypes as on the per-tick path; two greedy calls are
    identical and equal, at tolerance 0, a direct `evaluate_actor_launch` with pack_rollout_actor of the trainer's actor
    after reset_all_envs(); a greedy call leaves the sampler's words and `ou_state` alone; a sampled one advances each
    epoch word by the replica's steps; afterwards the envs are as reset_all_envs() leaves them"""
    import torch
    from tests.hip_harness import pull
    from warp_drive_amd.training.policy_kernel import pack_rollout_actor
    from warp_drive_amd.training.trainer_ddpg import TrainerDDPG

    pol, E = "shared", E_TR
    tr = _trainer(env, tmp_path, fused_evaluation=True)
    assert type(tr) is TrainerDDPG and tr.rollout_path == "one launch"
    tr.train(2)
    ep_sum = {p: tr._ep_sum[p].cpu().numpy().copy() for p in tr.policies}
    ep_cnt = tr._ep_cnt.cpu().numpy().copy()
    words = te._words(tr.sampler.rng_state, E)
    ou = pull(tr.w, OU).copy()
    assert np.abs(ou).max() > 0   # (training drew: the pattern a greedy call must keep is not zero)
    greedy = [tr.evaluate_episodes(use_argmax=True) for _ in range(2)]
    assert tr.evaluation_path == "one launch"
    EQ(te._words(tr.sampler.rng_state, E), words, "greedy: RNG words")
    EQ(pull(tr.w, OU), ou, "greedy: OU state")
    te._check_state_after(tr, ep_sum, ep_cnt)
    for rewards, steps in greedy:
        assert set(rewards) == set(steps) == {pol}
        assert rewards[pol].dtype == np.float32 and rewards[pol].shape == (E, 1)
        assert steps[pol].dtype == np.int32 and steps[pol].shape == (E,)
        assert (steps[pol] >= 1).all() and (steps[pol] <= T_EP).all() and np.isfinite(rewards[pol]).all()
    EQ(greedy[0][0][pol], greedy[1][0][pol], "two greedy evaluations: rewards")
    EQ(greedy[0][1][pol], greedy[1][1][pol], "two greedy evaluations: steps")
    # ---- the same launch, built by the test
    tr.w.reset_all_envs()
    actor = tr.actors[pol]
    packed = pack_rollout_actor(actor).cuda()
    out = {"reward_sum": torch.full((E,), -7.5, device="cuda"), "steps": torch.full((E,), -77, dtype=torch.int32, device="cuda"),
           "done": torch.full((E,), -77, dtype=torch.int32, device="cuda")}
    fn, args, block, grid, shared = tr.w.env.evaluate_actor_launch(
        tr.sampler, actor=(packed, 32, actor.action_scale, actor.action_bias), ou=(0.15, 0.2, 0.0), outputs=out, ticks=T_EP)
    fn(*args, block=block, grid=grid, shared=shared)
    torch.cuda.synchronize()
    EQ(greedy[0][0][pol][:, 0], out["reward_sum"].cpu().numpy(), "direct launch: rewards")
    EQ(greedy[0][1][pol], out["steps"].cpu().numpy(), "direct launch: steps")
    assert (out["done"].cpu().numpy() > 0).all()
    # ---- sampled
    rewards, steps = tr.evaluate_episodes()
    assert tr.evaluation_path == "one launch"
    assert rewards[pol].dtype == np.float32 and rewards[pol].shape == (E, 1) and steps[pol].shape == (E,)
    after = te._words(tr.sampler.rng_state, E)
    EQ(after[:4], words[:4]), EQ(after[4:], words[4:] + steps[pol].astype(np.uint32), "sampled: epoch += steps")
    assert np.ptp(rewards[pol]) > 0 and np.ptp(greedy[0][0][pol]) == 0   # one start state: only the noise differs
    te._check_state_after(tr, ep_sum, ep_cnt)
    tr.train(1)   # training goes on afterwards
    tr.graceful_close()


@pytest.mark.parametrize("env", ae.ENVS)
def test_trainer_without_the_key_stays_per_tick(env, tmp_path):
    """no `trainer.fused_evaluation` (or false): "per tick", also on the one-launch rollout"""
    for key in (None, False):
        tr = _trainer(env, tmp_path / str(key), fused_evaluation=key)
        assert tr.rollout_path == "one launch" and tr._one_launch_evaluation() is None
        rewards, steps = tr.evaluate_episodes(use_argmax=True)
        assert tr.evaluation_path == "per tick"
        assert rewards["shared"].shape == (E_TR, 1) and steps["shared"].shape == (E_TR,)
        tr.graceful_close()


@pytest.mark.parametrize("env", ae.ENVS)
@pytest.mark.parametrize("fused", [True, False])
def test_evaluator_logs_the_test_metrics(env, fused, tmp_path):
    """`trainer.evaluator: true` at a log frequency of 1: two training iterations put both "(test)" metrics, finite, into
    every record of results.json, on the one-launch path when it is available and per tick otherwise; without the key
    they are absent"""
    names = ("Mean episodic reward (test)", "Mean episodic steps (test)")
    for evaluator in (True, None):
        out = tmp_path / f"evaluator-{evaluator}"
        tr = _trainer(env, out, fused_evaluation=fused, evaluator=evaluator)
        tr.train(2)
        records = [json.loads(line) for line in open(os.path.join(str(out), "results.json"))]
        assert [r["Iterations Completed"] for r in records] == [1, 2]
        for r in records:
            if evaluator:
                assert all(np.isfinite(r["shared"][n]) for n in names), r["shared"]
                assert 1 <= r["shared"][names[1]] <= T_EP
            else:
                assert not any(n in r["shared"] for n in names)
        if evaluator:
            assert tr.evaluation_path == ("one launch" if fused else "per tick")
            assert all(n in tr.metrics["shared"] for n in names)
        else:
            assert not hasattr(tr, "evaluation_path")
        tr.graceful_close()
