"""The contract clauses of the custom-environment kits (include/wd_env.h, wd_env_tick.h, wd_env_rollout.h) that no worked
example reaches, on the MI355X, with tests/custom_envs/contract_probe.{hip,py} and the several-heads probe:

* the network on the device against tests/custom_rollout_model.py::policy_logits, through the Logits entries: logits at
  tolerance 0 for every (F, H) of the probe, -inf past A; running sums within NEAR_WINDOW, bit for bit where no expf
  result can differ (uniform, saturated, masked policies);
* the draw at preset epochs: arbitrary ones, the 2^32 wrap inside a launch, u == 1.0 and u == 2^-24 on every word, with
  probability rows crafted around the known uniforms (tick kit) and crafted policies (rollout kit), tolerance 0;
* a step that READS the done flag (wd_tick_begin's barrier), and a restart of a per-replica word, a row that is not
  agent-shaped, a row longer than the block and the rewards array itself.

Every expected value comes from tests/custom_contract_model.py (the host alone); tests/test_custom_env_contract_build.py
shows there that no case passes vacuously.  docs/rounds/r37.md has what was measured."""
import os

import numpy as np
import pytest

from tests import custom_contract_model as model
from tests.classic_control_cases import NEAR_WINDOW, near_threshold
from tests.classic_control_policy import count_below
from tests.custom_rollout_model import near_cap
from tests.rendezvous_helpers import registrar_for

pytestmark = pytest.mark.gpu

F_SENTINEL = np.float32(-77.25)
I_SENTINEL = 0x5EA7F00D
FENCE = 16   # sentinel words behind the last epoch word of the test's own RNG state


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


# ----------------------------------------------------------------------------------------------------------- helpers
class _Rng:
    """an RNG state of the test's own: the sampler's four header words, the given epochs, FENCE sentinel words"""

    def __init__(self, sampler, n_rows, dev):
        import torch

        from warp_drive_amd.managers import hip_driver as drv

        drv.synchronize()
        header = np.zeros(4, dtype=np.uint32)
        drv.memcpy_dtoh(header, sampler.rng_state)
        drv.synchronize()
        self.header, self.n_rows = header, n_rows
        words = np.concatenate([header, np.zeros(n_rows, np.uint32), np.full(FENCE, I_SENTINEL, np.uint32)])
        self.tensor = torch.from_numpy(words.view(np.int32).copy()).to(dev)

    def set_epochs(self, epochs):
        import torch

        e = np.ascontiguousarray(epochs, dtype=np.uint32)
        assert e.shape == (self.n_rows,)
        self.tensor[4:4 + self.n_rows] = torch.from_numpy(e.view(np.int32).copy()).to(self.tensor.device)

    def check(self, epochs_after, what):
        words = self.tensor.cpu().numpy().view(np.uint32)
        assert words[:4].tolist() == self.header.tolist(), f"{what}: the header words"
        assert (words[4 + self.n_rows:] == I_SENTINEL).all(), f"{what}: the words behind the last row"
        _same_bits(words[4:4 + self.n_rows], epochs_after, f"{what}: the epoch words")


def _same_bits(got, want, what):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want, dtype=got.dtype).reshape(got.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {np.argwhere(got != want)[:5].tolist()}"


def _sampler(w, seed):
    from warp_drive_amd.managers.function_manager import HIPSampler

    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=seed)
    return sampler


def _probe(N, F, L, seed, A=model.RESTART_A, E=3):
    """(EnvWrapper of ContractProbe, sampler).  The placeholders are pushed by hand: `rewards` WITH a reset copy (a value
    no step stores), which create_and_push_data_placeholders does not offer."""
    from tests.hip_harness import ACT, OBS, REW, require_gpu
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.utils.data_feed import DataFeed

    require_gpu()
    config = dict(num_agents=N, episode_length=L, n_actions=A, features=F, num_envs=E)
    w = EnvWrapper(env_name=model.ContractProbe.name, env_config=config, num_envs=E, env_backend="hip",
                   env_registrar=registrar_for(model.ContractProbe, model.SOURCE))
    w.reset_all_envs()
    feed = DataFeed()
    feed.add_data(name=OBS, data=np.repeat(model.probe_observation(0, N, F)[None], E, axis=0),
                  save_copy_and_apply_at_reset=True)
    feed.add_data(name=ACT, data=np.zeros((E, N, 1), dtype=np.int32))
    feed.add_data(name=REW, data=np.full((E, N), model.REWARD_AT_RESET, dtype=np.float32), save_copy_and_apply_at_reset=True)
    w.cuda_data_manager.push_data_to_device(feed, torch_accessible=True)
    assert list(w.cuda_data_manager.reset_data_list) == ["per_env", "odd", "wide", OBS, REW]
    return w, _sampler(w, seed)


def _device(w):
    from tests.hip_harness import ACT

    return w.cuda_data_manager.data_on_device_via_torch(ACT).device


def _tick(w, sampler, probs, ticks, rng=None):
    """one launch of the env's Tick entry for `ticks` ticks (on the RNG state `rng` when given)"""
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.utils.custom_tick import custom_tick_launch

    fn, args, block, grid, shared = custom_tick_launch(w.env, w.env.TICK_KERNEL, w.env.TICK_STEP_ARGS, sampler, probs,
                                                       w.env_resetter, ticks=ticks)
    args = list(args)
    if rng is not None:
        args[len(w.env.TICK_STEP_ARGS)] = rng.tensor
    fn(*args, block=block, grid=grid, shared=shared)
    drv.synchronize()


def _batch(E, N, F, rows, dev):
    import torch

    return {"obs": torch.full((rows, E, N, F), float(F_SENTINEL), dtype=torch.float32, device=dev),
            "actions": torch.full((rows, E, N, 1), I_SENTINEL, dtype=torch.int32, device=dev),
            "rewards": torch.full((rows, E, N), float(F_SENTINEL), dtype=torch.float32, device=dev),
            "done": torch.full((rows, E), I_SENTINEL, dtype=torch.int32, device=dev)}


def _rollout(w, sampler, packed, H, A, ticks, rng=None, rows=None):
    """one launch of the Rollout entry of width H for `ticks` ticks into fresh batch tensors (one sentinel row behind
    the last tick) -> the batch as numpy arrays"""
    import torch

    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.utils.custom_tick import custom_rollout_launch

    env, dev = w.env, _device(w)
    E, N, F = w.n_envs, env.num_agents, env.features
    batch = _batch(E, N, F, ticks + 1 if rows is None else rows, dev)
    weights = torch.from_numpy(np.ascontiguousarray(packed, dtype=np.float32)).to(dev)
    fn, args, block, grid, shared = custom_rollout_launch(env, env.ROLLOUT_KERNEL.format(width=H), env.TICK_STEP_ARGS,
                                                          sampler, A, weights, H, w.env_resetter, batch, ticks)
    assert block == ((N + 63) // 64 * 64, 1, 1) and tuple(grid)[0] == E and block[0] <= env.ROLLOUT_MAX_THREADS[H]
    args = list(args)
    if rng is not None:
        args[len(env.TICK_STEP_ARGS)] = rng.tensor
    fn(*args, block=block, grid=grid, shared=shared)
    drv.synchronize()
    got = {k: v.cpu().numpy() for k, v in batch.items()}
    for key, sentinel in (("obs", F_SENTINEL), ("rewards", F_SENTINEL), ("actions", I_SENTINEL), ("done", I_SENTINEL)):
        assert (got[key][ticks:] == sentinel).all(), f"the rows behind the last tick of {key}"
    return got


def _rng_words(sampler):
    from warp_drive_amd.managers import hip_driver as drv

    drv.synchronize()
    rng = np.zeros(4 + int(sampler._n_threads), dtype=np.uint32)
    drv.memcpy_dtoh(rng, sampler.rng_state)
    drv.synchronize()
    return rng


# ------------------------------------------------------------------------------- 2. the device network against the model
def _device_logits(w, H, A, packed, obs):
    """(logits [R, 8], running sums [R, 8]) of the Logits entry: two blocks of 64 threads, one thread per row"""
    import torch

    from warp_drive_amd.managers import hip_driver as drv

    dev, fm = _device(w), w.cuda_function_manager
    name = w.env.logits_kernel(H)
    fm.initialize_functions([name])
    R, F = obs.shape
    assert len(packed) == model.rollout_model.policy_floats(F, H, A)
    weights = torch.from_numpy(np.ascontiguousarray(packed, dtype=np.float32)).to(dev)
    rows = torch.from_numpy(np.ascontiguousarray(obs, dtype=np.float32)).to(dev)
    out = [torch.full((R + 1, 8), float(F_SENTINEL), dtype=torch.float32, device=dev) for _ in range(2)]
    fm.get_function(name)(weights, np.int32(A), rows, np.int32(R), out[0], out[1], block=(64, 1, 1), grid=(2, 1),
                          shared=(4 * len(packed) + 15) // 16 * 16)
    drv.synchronize()
    logits, cum = (t.cpu().numpy() for t in out)
    assert (logits[R] == F_SENTINEL).all() and (cum[R] == F_SENTINEL).all(), "the row behind the last one"
    return logits[:R], cum[:R]


@pytest.mark.parametrize("F,H", model.SHAPES, ids=lambda v: str(v))
def test_device_logits_and_running_sums_against_the_model(F, H):
    """every crafted policy of tests/custom_contract_model.py::logit_cases at A = 1, 2, 5, 8 (uniform: 2, 3, 5, 7, 8) on
    70 rows: the probe's signed observations, an all-zero row and a row of -0.0.  Logits: tolerance 0, the contract;
    -inf past A.  Running sums: NEAR_WINDOW (the project's window for two different expf), tolerance 0 where every expf
    term is expf(0) or underflows to 0; the last sum repeated past A."""
    w, _ = _probe(5, F, 4, seed=3)
    obs = model.logit_rows(F)
    worst = {}
    for name, A, packed, exact in model.logit_cases(F, H):
        logits, cum = _device_logits(w, H, A, packed, obs)
        want_logits, want_cum = model.model_logits_and_sums(packed, H, obs, A)
        _same_bits(logits[:, :A], want_logits, f"logits of {name}")
        assert np.isneginf(logits[:, A:]).all(), f"{name}: logits past A"
        _same_bits(cum[:, A:], np.repeat(cum[:, A - 1:A], 8 - A, axis=1), f"{name}: sums past A")
        diff = float(np.abs(cum[:, :A].astype(np.float64) - want_cum.astype(np.float64)).max())
        kind = name.split("-")[0].rstrip("0123456789")
        worst[kind] = max(worst.get(kind, 0.0), diff)
        if exact:
            _same_bits(cum[:, :A], want_cum, f"running sums of {name}")
        else:
            assert diff < NEAR_WINDOW, f"running sums of {name}: {diff}"
    print(f"F {F} H {H}: largest difference of a running sum per policy kind {worst}")


def test_non_finite_weights_still_draw_an_action_in_range():
    """a NaN and a +inf planted in W1: what the device returns is printed (docs/rounds/r37.md records it); asserted is
    only what the pick guarantees by construction, every drawn action in [0, A)"""
    F, H, A, N = 7, 32, 5, 70
    w, sampler = _probe(N, F, 50, seed=3)
    packed = model.non_finite_policy(F, H, A)
    obs = model.logit_rows(F)
    logits, cum = _device_logits(w, H, A, packed, obs)
    with np.errstate(all="ignore"):
        want_logits, want_cum = model.model_logits_and_sums(packed, H, obs, A)
    print(f"device logits, row 0: {logits[0].tolist()}; running sums: {cum[0].tolist()}")
    print(f"model  logits, row 0: {want_logits[0].tolist()}; running sums: {want_cum[0].tolist()}")
    print(f"rows with a NaN logit: device {int(np.isnan(logits[:, :A]).any(axis=1).sum())}, "
          f"model {int(np.isnan(want_logits).any(axis=1).sum())} of {len(obs)}; "
          f"NaN at the same places: {bool((np.isnan(logits[:, :A]) == np.isnan(want_logits)).all())}")
    fmax = model.policy_logits_fmax(packed, F, H, A, obs)   # the ReLU as C's fmaxf: a NaN activation becomes 0
    print(f"device logits equal the model's with fmaxf for its ReLU (what the host build of the header gives), bit for "
          f"bit: {model.same_bits_or_both_nan(logits[:, :A], fmax)}")
    got = _rollout(w, sampler, packed, H, A, 3)
    actions = got["actions"][:3]
    print(f"actions drawn under the non-finite policy: {np.bincount(actions.reshape(-1), minlength=A).tolist()}")
    assert actions.min() >= 0 and actions.max() < A


# ------------------------------------------------------------------------------------ 3. the draw at preset epochs
def _check_roles(plan, want_last, head_sizes, variant):
    """the crafted rows give what they are there for (the model's own values; the device is compared with them)"""
    flat = want_last.reshape(len(plan["epochs"]), -1)
    for row, (word, kind) in plan["roles"].items():
        A = head_sizes[word]
        _, k = model._plateau(A)
        if kind == "hi":
            assert flat[row, word] == (k - 1 if variant == 0 else A - 1)
        else:
            assert flat[row, word] == (A - k if variant == 0 else min(1, A - 1))


@pytest.mark.parametrize("variant", [0, 1], ids=["plateau-and-leading-zeros", "clamp"])
def test_tick_kit_draws_at_preset_epochs_four_heads(variant):
    """HipHeadsProbeTick with four heads at E = 3, N = 70: one launch of three ticks from preset epochs.  The action
    tensor holds the LAST tick's actions (where every end is drawn), the counts the sum of action + 1 over the ticks."""
    from tests.custom_envs.heads_probe import SOURCE, HeadsProbe
    from tests.hip_harness import ACT, pull, require_gpu
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

    import torch

    require_gpu()
    E, N, T, sizes = model.END_E, model.END_N, model.END_TICKS, (3, 2, 7, 5)
    w = EnvWrapper(env_name="HeadsProbe", env_config=dict(num_agents=N, episode_length=50, head_sizes=sizes), num_envs=E,
                   env_backend="hip", env_registrar=registrar_for(HeadsProbe, SOURCE))
    w.reset_all_envs()
    sampler = _sampler(w, model.END_SEED)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    dev = _device(w)
    rng = _Rng(sampler, E * N, dev)
    plan = model.tick_plan(int(rng.header[0]), int(rng.header[1]), sizes, variant)   # searched from the device's words
    assert sorted(plan["roles"].values()) == sorted((h, k) for h in range(4) for k in ("hi", "lo"))
    _check_roles(plan, plan["want"][-1], sizes, variant)
    rng.set_epochs(plan["epochs"])
    _tick(w, sampler, [torch.from_numpy(p).to(dev) for p in plan["probs"]], T, rng)
    _same_bits(pull(w, ACT), plan["want"][-1], "actions of the last tick")
    _same_bits(pull(w, "counts"), (plan["want"] + 1).sum(axis=0), "counts over the launch")
    rng.check(plan["epochs_after"], "after the launch")
    assert plan["epochs_after"][plan["wrap"]].tolist() == [2, 1]   # wrapped inside the launch
    assert (_rng_words(sampler)[4:] == 0).all()                     # the sampler's own state was not the one in use


@pytest.mark.parametrize("variant", [0, 1], ids=["plateau-and-leading-zeros", "clamp"])
def test_tick_kit_draws_at_preset_epochs_one_head(variant):
    """HipContractProbeTick (one head of five actions) at E = 3, N = 70, episodes longer than the launch: rewards are
    action + 1, so the step was handed the action that was stored"""
    import torch

    from tests.hip_harness import ACT, REW, pull

    E, N, T, A = model.END_E, model.END_N, model.END_TICKS, 5
    w, sampler = _probe(N, 4, 50, seed=model.END_SEED, A=A)
    dev = _device(w)
    rng = _Rng(sampler, E * N, dev)
    plan = model.tick_plan(int(rng.header[0]), int(rng.header[1]), (A,), variant)
    assert sorted(plan["roles"].values()) == [(0, "hi"), (0, "lo")]
    _check_roles(plan, plan["want"][-1], (A,), variant)
    rng.set_epochs(plan["epochs"])
    _tick(w, sampler, [torch.from_numpy(plan["probs"][0]).to(dev)], T, rng)
    _same_bits(pull(w, ACT), plan["want"][-1], "actions of the last tick")
    _same_bits(pull(w, REW), (plan["want"][-1][..., 0] + 1).astype(np.float32), "rewards of the last tick")
    assert (pull(w, "seen_done") == 0).all() and (pull(w, "_timestep_") == T).all()
    rng.check(plan["epochs_after"], "after the launch")


@pytest.mark.parametrize("F,H", [(4, 32), (7, 64)], ids=lambda v: str(v))
def test_rollout_kit_draws_at_preset_epochs(F, H):
    """the Rollout entry at E = 3, N = 70 from the same preset epochs under the masked, saturated and uniform policies:
    NO excused draw (the model's near-threshold count is 0, shown on the CPU), every recorded action is the model's; at
    u == 2^-24 an action of probability 0 in front is never drawn, at u == 1.0 the action is what the model's sums and the
    clamp give.  One random policy under near_cap's rule."""
    E, N, T = model.END_E, model.END_N, model.END_TICKS
    w, sampler = _probe(N, F, 50, seed=model.END_SEED, A=8)
    rng = _Rng(sampler, E * N, _device(w))
    for name, A, packed, crafted in model.end_policies(F, H):
        w.reset_all_envs()
        plan = model.rollout_plan(int(rng.header[0]), int(rng.header[1]), F, H, A, packed, crafted)
        assert sorted(plan["roles"].values()) == [(0, "hi"), (0, "lo")]
        rng.set_epochs(plan["epochs"])
        got = _rollout(w, sampler, packed, H, A, T, rng)
        near = 0
        for k in range(T):
            _same_bits(got["obs"][k], plan["obs"][k], f"{name}: obs_batch, tick {k}")
            actions = got["actions"][k].reshape(E * N)
            assert actions.min() >= 0 and actions.max() < A
            flagged = plan["near"][k] if not crafted else np.zeros(E * N, bool)
            near += int(plan["near"][k].sum())
            bad = np.flatnonzero((actions != plan["want"][k]) & ~flagged)
            assert bad.size == 0, f"{name}: actions, tick {k}: rows {bad[:5].tolist()}"
            _same_bits(got["rewards"][k], (actions + 1).astype(np.float32), f"{name}: reward_batch, tick {k}")
        print(f"F {F} H {H} {name}: {near} near-threshold draws of {E * N * T} (cap {0 if crafted else near_cap(E * N * T, A)})")
        assert near <= (0 if crafted else near_cap(E * N * T, A))
        for row, (_, kind) in plan["roles"].items():
            u, a, cum = plan["u"][-1][row], int(got["actions"][T - 1].reshape(-1)[row]), plan["cum"][-1][row]
            assert u == (np.float32(1.0) if kind == "hi" else np.float32(2.0 ** -24))
            if kind == "lo" and crafted:
                assert (np.diff(np.concatenate([[0], cum]))[a] > 0), f"{name}: an action of probability 0 was drawn"
            if kind == "hi":
                assert a == min(int((cum < u).sum()), A - 1)
        rng.check(plan["epochs_after"], f"{name}: after the launch")
        assert plan["epochs_after"][plan["wrap"]].tolist() == [2, 1]


# --------------------------------------------------------------------------------- 4. the done flag and the restart
def _state(w):
    from tests.hip_harness import ACT, OBS, REW, pull

    return {k: pull(w, k) for k in (OBS, REW, ACT, "_done_", "_timestep_", "seen_done", "per_env", "odd", "wide")}


def _check_state(w, host, actions, what):
    from tests.hip_harness import ACT, OBS, REW

    want = dict(host.state(), **{OBS: host.obs, REW: host.rewards, ACT: actions})
    got = _state(w)
    for k, v in want.items():
        _same_bits(got[k], v, f"{k} {what}")


@pytest.mark.parametrize("N", model.RESTART_AGENTS)
def test_tick_entry_reads_the_done_flag_and_restarts_every_array(N):
    """HipContractProbeTick, E = 3, episodes of 4 ticks under launches of 5, 9 and 6 ticks: a flag set at tick k stands
    when tick k + 1 begins, inside a launch and across launches, and the step must never see it (`seen_done` stays 0).
    After every launch every array holds the host model's values: restored on the tick a replica finishes (the rewards
    array too, to a value no step stores), mutated otherwise; `_done_` stays 1 behind a finish on the last tick."""
    import torch

    E, A = model.RESTART_E, model.RESTART_A
    w, sampler = _probe(N, 7, model.RESTART_L, seed=model.RESTART_SEED)
    probs = model.restart_probabilities(N)
    tensors = [torch.from_numpy(probs).to(_device(w))]
    host = model.HostProbe(model.restart_config(N, 7))
    draws = model.tick_model.TickDraws(model.RESTART_SEED, E, N, model.TICK_TAG)
    assert _rng_words(sampler)[:4].tolist() == draws.header()
    total = 0
    for launch, T in enumerate(model.RESTART_LAUNCHES):
        _tick(w, sampler, tensors, T)
        for k in range(T):
            actions = draws.draw([probs])
            host.step(actions[..., 0], last_tick=k == T - 1)
        total += T
        _check_state(w, host, actions, f"after launch {launch}")
        assert (_rng_words(sampler)[4:] == total).all()
    assert host.inside >= 1 and host.on_last == E and (host.done == 1).all() and (host.timesteps() == 0).all()


@pytest.mark.parametrize("N", model.RESTART_AGENTS)
@pytest.mark.parametrize("F,H", [(1, 4), (7, 32)], ids=lambda v: str(v))
def test_rollout_entry_records_rewards_before_it_restores_them(F, H, N):
    """the Rollout entries of the smallest network (F = 1, H = 4) and of (7, 32) on the same launches: every recorded
    tick is judged from its own inputs; reward_batch[k] holds action + 1 on a finishing tick as well, the rewards array
    the reference value behind it"""
    from tests.hip_harness import REW, pull

    E, A = model.RESTART_E, model.RESTART_A
    w, sampler = _probe(N, F, model.RESTART_L, seed=model.RESTART_SEED)
    packed = model.policies(F, H, A)["random2"][0]
    host = model.HostProbe(model.restart_config(N, F))
    near = tick = draws = 0
    for launch, T in enumerate(model.RESTART_LAUNCHES):
        got = _rollout(w, sampler, packed, H, A, T)
        for k in range(T):
            where = f"launch {launch}, tick {k}"
            _same_bits(got["obs"][k], host.obs, f"obs_batch, {where}")
            cum = model.model_logits_and_sums(packed, H, got["obs"][k].reshape(E * N, F), A)[1]
            u = model.rollout_model.replayed_uniform(model.RESTART_SEED, E * N, tick)
            flagged = near_threshold(cum, u)
            near += int(flagged.sum())
            actions = got["actions"][k].reshape(E * N)
            assert actions.min() >= 0 and actions.max() < A, where
            assert (actions[~flagged] == count_below(cum, u)[~flagged]).all(), f"actions, {where}"
            rewards, done = host.step(actions.reshape(E, N), last_tick=k == T - 1)
            _same_bits(got["rewards"][k], (actions + 1).astype(np.float32), f"reward_batch, {where}")
            _same_bits(got["rewards"][k], rewards, f"reward_batch against the host step, {where}")
            _same_bits(got["done"][k], done, f"done_batch, {where}")
            tick, draws = tick + 1, draws + E * N
        _check_state(w, host, actions, f"after launch {launch}")
        assert (_rng_words(sampler)[4:] == tick).all()
    print(f"F {F} H {H} N {N}: {near} near-threshold draws of {draws} (cap {near_cap(draws, A)})")
    assert near <= near_cap(draws, A)
    assert host.inside >= 1 and host.on_last == E and (pull(w, REW) == model.REWARD_AT_RESET).all()


@pytest.mark.parametrize("kit", ["tick", "rollout"])
@pytest.mark.parametrize("N", [5, 130])
def test_one_launch_of_T_ticks_equals_T_launches_of_one(N, kit):
    """two wrappers from the same seeds: ONE launch of 9 ticks (two finishes inside) on the first, 9 launches of one tick
    on the second; every array, every batch row and the RNG state are equal bit for bit"""
    import torch

    F, H, A, T = 7, 32, model.RESTART_A, 9
    sides = [_probe(N, F, model.RESTART_L, seed=model.RESTART_SEED) for _ in range(2)]
    packed = model.policies(F, H, A)["random3"][0]
    probs = model.restart_probabilities(N)

    def run(side, ticks):
        w, sampler = side
        if kit == "tick":
            return _tick(w, sampler, [torch.from_numpy(probs).to(_device(w))], ticks)
        return _rollout(w, sampler, packed, H, A, ticks)

    multi = run(sides[0], T)
    singles = [run(sides[1], 1) for _ in range(T)]
    if kit == "rollout":
        for key in multi:
            _same_bits(multi[key][:T], np.stack([s[key][0] for s in singles]), f"batch {key}")
        assert multi["done"][:T].sum() == 2 * model.RESTART_E
    got, want = _state(sides[0][0]), _state(sides[1][0])
    for k in want:
        _same_bits(got[k], want[k], f"{k} after the launch")
    assert (want["_timestep_"] == T % model.RESTART_L).all() and (want["seen_done"] == 0).all()
    rng1, rng2 = _rng_words(sides[0][1]), _rng_words(sides[1][1])
    assert rng1.tobytes() == rng2.tobytes() and (rng1[4:] == T).all()
