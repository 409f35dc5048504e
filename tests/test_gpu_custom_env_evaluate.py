"""The one-launch evaluation of a custom environment on the MI355X (include/wd_env_evaluate.h,
warp_drive_amd/utils/custom_tick.py::FusedEvaluateMixin): examples/rendezvous_evaluate/ and the probe of tests/custom_envs/
are registered with their device sources, compiled on first use and driven through `evaluate_launch` and Trainer.

Against the model (tests/custom_evaluate_model.py), with the action trace: every tick of every replica is judged from host
values -- the host replicas give the observation, the numpy model the expected action (the first maximum of the
probabilities, or the count of running sums below the replayed uniform); the host step is fed the RECORDED action.  A
decision is excused only where `near_top_two` / `near_threshold` flag it, the flagged count is printed and capped by the
project's rule; reward sums (float32 adds in tick order), steps, done, trace rows, sentinels and the end state are held at
tolerance 0.  The crafted policies of tests/custom_crafted_policies.py excuse nothing at all.

What was seen on the MI355X: one decision flagged near a threshold in all the cases together (the probe at N = 70, width 32,
two actions, sampled: 1 of 840, cap 2 -- the host model flags the same one), none elsewhere; every decision that is not
flagged equals the model's (docs/rounds/r42.md)."""
import os

import numpy as np
import pytest

from tests import custom_crafted_policies as crafted
from tests import custom_evaluate_model as model
from tests.rendezvous_helpers import registrar_for

pytestmark = pytest.mark.gpu

f32 = np.float32
F_SENTINEL = f32(-77.25)
I_SENTINEL = 0x5EA7F00D
PAD = 64   # sentinel words behind the last element of reward_sum / steps / done


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


# ------------------------------------------------------------------------------------------------------- the device
def _wrapper(case, config=None, seed=None, cls=None):
    """(EnvWrapper by name through the registrar, reset, placeholders pushed, sampler)"""
    from tests.hip_harness import require_gpu
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

    require_gpu()
    cls = case.env_class() if cls is None else cls
    w = EnvWrapper(env_name=cls.name, env_config=case.config() if config is None else config, num_envs=case.E,
                   env_backend="hip", env_registrar=registrar_for(cls, case.source()))
    w.reset_all_envs()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=case.seed if seed is None else seed)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    return w, sampler


def _write(w, name, array):
    """overwrite the device array `name` (not its reset copy) with `array`: same shape, same dtype"""
    from warp_drive_amd.managers import hip_driver as drv

    dm = w.cuda_data_manager
    array = np.ascontiguousarray(array)
    assert tuple(dm.get_shape(name)) == array.shape and dm.get_dtype(name) == array.dtype.name, (name, array.shape)
    drv.memcpy_htod(dm.device_data(name), array)
    drv.synchronize()


def _start(case, w, host):
    """put the replicas on the device where the host replicas stand (behind reset_all_envs())"""
    from tests.hip_harness import OBS

    cells = case.start_cells()
    if cells is not None:
        _write(w, "loc_x", cells[0])
        _write(w, "loc_y", cells[1])
        _write(w, OBS, host.obs.astype(f32))


def _rng_words(sampler, words=None):
    """the sampler's whole state; with `words`: write it back first"""
    from warp_drive_amd.managers import hip_driver as drv

    drv.synchronize()
    n = 4 + int(sampler._n_threads)
    if words is not None:
        assert words.dtype == np.uint32 and words.shape == (n,)
        drv.memcpy_htod(sampler.rng_state, words)
        drv.synchronize()
    rng = np.zeros(n, dtype=np.uint32)
    drv.memcpy_dtoh(rng, sampler.rng_state)
    drv.synchronize()
    return rng


def _same_bits(got, want, what):
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(want, dtype=got.dtype).reshape(got.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {np.argwhere(got != want)[:5].tolist()}"


def _device(w):
    from tests.hip_harness import ACT

    return w.cuda_data_manager.data_on_device_via_torch(ACT).device


def _launch(case, w, sampler, packed, ticks, traced=True):
    """one launch of the case's Evaluate entry -> (outputs as numpy, sentinel pads included; trace [ticks + 1, E, N] or
    None)"""
    import torch

    from warp_drive_amd.managers import hip_driver as drv

    dev, E, N = _device(w), case.E, case.N
    weights = torch.from_numpy(np.ascontiguousarray(packed)).to(dev)
    out = {"reward_sum": torch.full((E * N + PAD,), float(F_SENTINEL), dtype=torch.float32, device=dev),
           "steps": torch.full((E + PAD,), I_SENTINEL, dtype=torch.int32, device=dev),
           "done": torch.full((E + PAD,), I_SENTINEL, dtype=torch.int32, device=dev)}
    trace = torch.full((ticks + 1, E, N), I_SENTINEL, dtype=torch.int32, device=dev) if traced else None
    assert w.env.has_live_policy_evaluate(case.hidden, case.A) and w.env.cuda_env_resetter is w.env_resetter
    fn, args, block, grid, shared = w.env.evaluate_launch(sampler, policy=(weights, case.hidden), use_argmax=case.greedy,
                                                          outputs=out, action_trace=trace, ticks=ticks)
    assert fn.name == w.env.EVALUATE_KERNEL.format(width=case.hidden) and grid[0] == E and block[0] == (N + 63) // 64 * 64
    fn(*args, block=block, grid=grid, shared=shared)
    drv.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}, (None if trace is None else trace.cpu().numpy())


def _judge(case, host, packed, out, trace, ticks, uniforms=None, excuse=True):
    """the launch's outputs and trace against the host replicas, tick by tick; returns (flagged decisions, decisions,
    action counts [A], the last recorded action of every agent [E, N]).  `uniforms(k)`: the uniform of every agent row at
    tick k (default: the replay from epoch 0); excuse=False: no decision is excused"""
    E, N, A = case.E, case.N, case.A
    near = decisions = 0
    seen = np.zeros(A, dtype=np.int64)
    last = np.zeros((E, N), dtype=np.int32)
    for k in range(ticks):
        running = host.running.copy()
        if not running.any():
            break
        obs = host.obs.reshape(E * N, case.F)
        p = model.policy_probabilities(packed, case.hidden, obs, A)
        if case.greedy:
            want, flagged = model.first_maximum(p), model.near_top_two(p)
        else:
            cum = model.running_sums(p)
            u = model.replayed_uniform(case.seed, E * N, k) if uniforms is None else uniforms(k)
            want, flagged = model.count_below(cum, u), model.near_threshold(cum, u)
        if not excuse:
            flagged = np.zeros(E * N, dtype=bool)
        live = np.repeat(running, N)
        got = trace[k].reshape(E * N)
        assert (got[live] >= 0).all() and (got[live] < A).all(), f"{case}, tick {k}"
        assert (got[~live] == I_SENTINEL).all(), f"{case}, tick {k}: a trace row behind a replica's last tick was written"
        bad = live & ~flagged & (got != want)
        assert not bad.any(), f"{case}, tick {k}: rows {np.flatnonzero(bad)[:5].tolist()} got {got[bad][:5]} want {want[bad][:5]}"
        near += int((flagged & live).sum())
        decisions += int(live.sum())
        seen += np.bincount(got[live], minlength=A)
        last[running] = got.reshape(E, N)[running]
        host.step(np.where(live, got, 0).reshape(E, N))
    assert (trace[host.steps.max():] == I_SENTINEL).all(), f"{case}: rows behind the last tick"
    _same_bits(out["reward_sum"][:E * N], host.total, f"{case}: reward_sum")
    _same_bits(out["steps"][:E], host.steps, f"{case}: steps")
    _same_bits(out["done"][:E], host.done, f"{case}: done")
    assert (out["reward_sum"][E * N:] == F_SENTINEL).all() and (out["steps"][E:] == I_SENTINEL).all() and \
        (out["done"][E:] == I_SENTINEL).all(), f"{case}: a sentinel behind the outputs was overwritten"
    return near, decisions, seen, last


def _end_state(case, w, sampler, host, last, rng_before):
    """what a launch leaves: every array with a reset copy equals it, `_timestep_` and `_done_` are zero, `rewards` and the
    action array keep the last tick's values, the RNG words are untouched (greedy) or advanced by the replica's steps"""
    from tests.hip_harness import ACT, OBS, REW, pull

    dm = w.cuda_data_manager
    names = list(dm.reset_data_list)
    assert OBS in names and (case.kind != "rendezvous" or {"loc_x", "loc_y"} <= set(names))
    for name in names:
        _same_bits(pull(w, name), pull(w, f"{name}_at_reset"), f"{case}: {name} against its reset copy")
    _same_bits(pull(w, OBS), host.first, f"{case}: observations")
    assert (pull(w, "_timestep_") == 0).all() and (pull(w, "_done_") == 0).all()
    assert REW not in names and ACT not in names
    _same_bits(pull(w, REW), host.last_rewards, f"{case}: rewards keep the last tick's values")
    _same_bits(pull(w, ACT), last, f"{case}: the action array keeps the last tick's values")
    rng = _rng_words(sampler)
    want = rng_before.copy()
    if not case.greedy:
        want[4:4 + case.E * case.N] += np.repeat(host.steps.astype(np.uint32), case.N)
    _same_bits(rng, want, f"{case}: the sampler's state")


def _run_against_the_model(case, ticks=None):
    ticks = case.ticks if ticks is None else ticks
    w, sampler = _wrapper(case)
    _, packed = case.policy()
    host = case.replicas()
    _start(case, w, host)
    before = _rng_words(sampler)
    assert before[:2].tolist() == list(model.rollout_model.tick_model.seed_words(case.seed))
    assert (before[4:4 + case.E * case.N] == 0).all()
    out, trace = _launch(case, w, sampler, packed, ticks)
    near, decisions, seen, last = _judge(case, host, packed, out, trace, ticks)
    print(f"{case}: {near} flagged decisions of {decisions} (cap {case.near_cap(decisions)}), actions {seen.tolist()}, "
          f"steps {host.steps.tolist()}, {host.early} early and {host.timed} timed finishes")
    assert near <= case.near_cap(decisions)
    _end_state(case, w, sampler, host, last, before)
    # without the trace, from the same start: the same bytes
    _start(case, w, case.replicas())
    _rng_words(sampler, before)
    again, none = _launch(case, w, sampler, packed, ticks, traced=False)
    assert none is None
    for key in out:
        _same_bits(again[key], out[key], f"{case}: {key} without the trace")
    _end_state(case, w, sampler, host, last, before)
    return host


# --------------------------------------------------------------------------------------------------- against the model
@pytest.mark.parametrize("case", model.RENDEZVOUS_CASES, ids=repr)
def test_rendezvous_against_the_model(case):
    """replicas finish at different ticks within one launch: at least two distinct step counts wherever N > 1"""
    host = _run_against_the_model(case)
    assert host.done.all() and host.early + host.timed == case.E
    if case.N > 1:
        assert host.early >= 1 and host.timed >= 1 and len(set(host.steps.tolist())) >= 2, host.steps.tolist()


@pytest.mark.parametrize("case", model.PROBE_CASES, ids=repr)
def test_the_probe_against_the_model(case):
    """F = 2 and a run-time action count: A = 1, 2, 8 at one agent, a partial wavefront and two wavefronts.  `ticks` is
    LONGER than the episode: the launch stops at the first done.  The rewards are action + 1: the sums show that the step
    was handed the recorded actions."""
    host = _run_against_the_model(case)
    assert case.ticks == case.L + 1 and (host.steps == case.L).all() and host.done.all() and host.timed == case.E


@pytest.mark.parametrize("case", model.SHORT_CASES, ids=repr)
def test_ticks_shorter_than_the_episode(case):
    """done == 0 and steps == ticks for whoever is still running, and the replica is restored all the same (the end state
    is checked for every replica)"""
    host = _run_against_the_model(case)
    still = host.done == 0
    assert still.any() and (host.steps[still] == case.ticks).all() and host.running[still].all()


def test_a_block_over_the_launch_bound_is_refused_and_nothing_is_launched():
    """N = 520 is a block of 576 threads: the width-32 entry (bound 1024) serves it, the width-64 entry (bound 512) does
    not -- the env says no, `evaluate_launch` refuses, nothing is launched: outputs, env arrays and RNG state keep their
    bytes"""
    import torch

    from tests.hip_harness import OBS, pull
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    case = model.Case("rendezvous", *model.WIDE_SHAPE, hidden=64, mode="greedy")
    w, sampler = _wrapper(case, config=dict(num_agents=case.N, grid_length=case.L, episode_length=case.T, seed=case.N))
    assert w.env.has_live_policy_evaluate(32, 5) and not w.env.has_live_policy_evaluate(64, 5)
    dev = _device(w)
    weights = torch.from_numpy(case.policy()[1]).to(dev)
    out = {"reward_sum": torch.full((case.E, case.N), float(F_SENTINEL), dtype=torch.float32, device=dev),
           "steps": torch.full((case.E,), I_SENTINEL, dtype=torch.int32, device=dev),
           "done": torch.full((case.E,), I_SENTINEL, dtype=torch.int32, device=dev)}
    before, obs = _rng_words(sampler), pull(w, OBS)
    for greedy in (True, False):
        with pytest.raises(UnsupportedRolloutShape, match="576 threads"):
            w.env.evaluate_launch(sampler, policy=(weights, 64), use_argmax=greedy, outputs=out, ticks=case.T)
    assert (out["reward_sum"].cpu().numpy() == F_SENTINEL).all() and (out["steps"].cpu().numpy() == I_SENTINEL).all()
    assert _rng_words(sampler).tobytes() == before.tobytes() and pull(w, OBS).tobytes() == obs.tobytes()
    assert (pull(w, "_timestep_") == 0).all()


# ------------------------------------------------------------------------------------------------ no excused decision
CRAFTED_SHAPES = [("rendezvous", 2, 130, 8, 7, 5), ("probe", 3, 70, 7, 7, 2), ("probe", 3, 70, 7, 7, 8)]


def _crafted_case(kind, E, N, L, T, A, hidden, mode):
    case = model.Case(kind, E, N, L, T, hidden=hidden, A=A, mode=mode)
    case.seed = crafted.END_SEED
    if kind == "rendezvous":
        case._config = dict(num_agents=N, grid_length=L, episode_length=T, seed=N, wall_penalty=0.125, spread_limit=-1)
    return case


def _crafted_policies(case):
    """{name: (packed, expected greedy action of a row of observations, or None)}"""
    F, H, A = case.F, case.hidden, case.A
    above, below = (2, 1) if A >= 3 else (0, 1)
    out = {"uniform": (crafted.uniform(F, H, A), lambda obs: np.zeros(len(obs), np.int32)),
           "switched": (crafted.switched(F, H, A, 0, 0.5, above, below),
                        lambda obs: crafted.switched_winner(obs[:, 0], 0.5, above, below))}
    if A >= 5:
        out["tied"] = (crafted.constant(F, H, A, (1, 3)), lambda obs: np.ones(len(obs), np.int32))
    return out


@pytest.mark.parametrize("hidden", model.WIDTHS)
@pytest.mark.parametrize("shape", CRAFTED_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_crafted_policies_greedy_excuse_nothing(shape, hidden):
    """uniform: action 0 on every tick; two tied winners: the lower index; switched on the sign of (column 0 - 0.5): the
    expected winner, the lower index AT the threshold.  Probabilities exactly 0, 0.5, 1 or 1 / A: no window, no cap."""
    case = _crafted_case(*shape, hidden=hidden, mode="greedy")
    w, sampler = _wrapper(case)
    before = _rng_words(sampler)
    for name, (packed, expected) in _crafted_policies(case).items():
        host = case.replicas()
        _start(case, w, host)
        first_obs = host.obs.reshape(case.E * case.N, case.F).copy()
        out, trace = _launch(case, w, sampler, packed, case.ticks)
        _same_bits(trace[0].reshape(-1), expected(first_obs), f"{case}, {name}: tick 0 against the helper's winner")
        near, decisions, seen, last = _judge(case, host, packed, out, trace, case.ticks, excuse=False)
        assert near == 0 and decisions == case.E * case.N * case.ticks and (host.steps == case.ticks).all()
        if name == "uniform":
            assert seen[0] == decisions
        if name == "tied":
            assert seen[1] == decisions
        if name == "switched" and case.kind == "rendezvous":
            assert (first_obs[:, 0] == 0.5).any() and (first_obs[:, 0] < 0.5).any() and (first_obs[:, 0] > 0.5).any()
            assert seen[1] > 0 and seen[2] > 0 and seen[1] + seen[2] == decisions
        _end_state(case, w, sampler, host, last, before)


@pytest.mark.parametrize("hidden", model.WIDTHS)
@pytest.mark.parametrize("shape", CRAFTED_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_crafted_policies_sampled_at_preset_epochs_excuse_nothing(shape, hidden):
    """the epoch words are preset so that known rows draw u == 1.0 (the clamp: the last action with a positive
    probability ... or the last action) and u == 2^-24 (the first action with a positive probability) inside the launch;
    every action of every row equals the count of the model's exact running sums below the replayed uniform"""
    case = _crafted_case(*shape, hidden=hidden, mode="sampled")
    w, sampler = _wrapper(case)
    rows = case.E * case.N
    epochs, roles = crafted.preset_epochs(rows, case.ticks)
    assert {kind for kind, _ in roles.values()} == {"hi", "lo"}
    start = _rng_words(sampler)
    start[4:4 + rows] = epochs
    uniforms = lambda k: model.uniforms_at(case.seed, np.arange(rows), epochs.astype(np.uint64) + np.uint64(k))  # noqa: E731
    for row, (kind, tick) in roles.items():
        assert uniforms(tick)[row] == f32(1.0 if kind == "hi" else 2.0 ** -24)
    for name, (packed, _) in _crafted_policies(case).items():
        host = case.replicas()
        _start(case, w, host)
        before = _rng_words(sampler, start)
        out, trace = _launch(case, w, sampler, packed, case.ticks)
        near, decisions, seen, last = _judge(case, host, packed, out, trace, case.ticks, uniforms=uniforms, excuse=False)
        assert decisions == rows * case.ticks and (host.steps == case.ticks).all()
        for row, (kind, tick) in roles.items():
            got = int(trace[tick].reshape(-1)[row])
            if name == "uniform":
                assert got == (case.A - 1 if kind == "hi" else 0), (name, row, kind, got)
            if name == "tied":                       # running sums 0, 0.5, 0.5, 1, 1: below 1.0 three, below 2^-24 one
                assert got == (3 if kind == "hi" else 1), (name, row, kind, got)
        if name == "uniform":
            assert (seen > 0).all()
        _end_state(case, w, sampler, host, last, before)


# ------------------------------------------------------------------------------------------------------- the trainer
E_T, N_T, T_T, L_T = 4, 5, 12, 6


def _trainer(tmp_path, fc_dims=(32, 32), rollout="all", fused_update=None, cls=None, pool_seed=None):
    import torch

    from tests.hip_harness import require_gpu
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.training.trainer import Trainer

    require_gpu()
    cls = model.example_module().RendezvousEvaluate if cls is None else cls
    w = EnvWrapper(env_name=cls.name, env_config=dict(num_agents=N_T, grid_length=L_T, episode_length=T_T, seed=9),
                   num_envs=E_T, env_backend="hip", env_registrar=registrar_for(cls, model.EXAMPLE_SOURCE))
    if pool_seed is not None:
        w.init_reset_pool(seed=pool_seed)
    trainer_config = {"num_envs": E_T, "train_batch_size": E_T * 6, "num_episodes": 10 ** 6, "seed": 5}
    if rollout is not None:
        trainer_config["fused_rollout_policy"] = rollout
    if fused_update is not None:
        trainer_config["fused_update"] = fused_update
    pcfg = {"to_train": True, "algorithm": "A2C", "lr": 0.01, "vf_loss_coeff": 1, "entropy_coeff": 0.05, "gamma": 0.98,
            "clip_grad_norm": True, "max_grad_norm": 3, "normalize_advantage": False, "normalize_return": False,
            "model": {"type": "fully_connected", "fc_dims": list(fc_dims), "model_ckpt_filepath": ""}}
    config = {"name": "rendezvous_evaluate", "trainer": trainer_config, "policy": {"shared": pcfg},
              "saving": {"metrics_log_freq": 1, "model_params_save_freq": 0, "basedir": str(tmp_path),
                         "name": "rendezvous_evaluate", "tag": "test"}}
    torch.manual_seed(3)
    return Trainer(env_wrapper=w, config=config, policy_tag_to_agent_id_map={"shared": list(range(N_T))},
                   results_dir=str(tmp_path), verbose=False)


def _documented(rewards, steps):
    assert set(rewards) == set(steps) == {"shared"}
    assert rewards["shared"].shape == (E_T, N_T) and rewards["shared"].dtype == np.float32
    assert steps["shared"].shape == (E_T,) and steps["shared"].dtype == np.int32
    assert (steps["shared"] >= 1).all() and (steps["shared"] <= T_T).all() and np.isfinite(rewards["shared"]).all()


@pytest.mark.parametrize("hidden", model.WIDTHS)
def test_trainer_evaluates_in_one_launch_and_agrees_with_the_per_tick_path(tmp_path, hidden):
    """under `fused_rollout_policy: "all"` the evaluation is one launch, greedy and sampled; with a crafted exact policy
    (switched on column 0: the agents walk towards x = L / 2) a greedy evaluation returns the same bytes as a second trainer
    on the per-tick path with the same weights, and leaves the envs as `reset_all_envs()` leaves them"""
    from tests.hip_harness import OBS, pull

    one = _trainer(tmp_path / "one", fc_dims=(hidden, hidden))
    per = _trainer(tmp_path / "per", fc_dims=(hidden, hidden), rollout=None)
    assert one.rollout_path == "one launch" and per.rollout_path == "per tick"
    packed = crafted.switched(5, hidden, 5, 0, 0.5, 2, 1)
    for tr in (one, per):
        crafted.load_into(tr.models["shared"], packed, 5, hidden, 5)
    r1, s1 = one.evaluate_episodes(use_argmax=True)
    r2, s2 = per.evaluate_episodes(use_argmax=True)
    assert one.evaluation_path == "one launch" and per.evaluation_path == "per tick"
    _documented(r1, s1)
    _documented(r2, s2)
    _same_bits(r1["shared"], r2["shared"], "reward sums of the two paths")
    _same_bits(s1["shared"], s2["shared"], "step counts of the two paths")
    case = model.Case("rendezvous", E_T, N_T, L_T, T_T, hidden=hidden, mode="greedy")
    case._config = dict(num_agents=N_T, grid_length=L_T, episode_length=T_T, seed=9)
    host = model.EpisodeReplicas(case.env_class(), case._config, E_T)
    for k in range(T_T):
        want, _ = model.expected_actions(case, packed, host.obs.reshape(E_T * N_T, 5), k)   # (exact: a tie is no excuse)
        host.step(want.reshape(E_T, N_T))
    _same_bits(r1["shared"], host.total, "reward sums against the host replicas")
    _same_bits(s1["shared"], host.steps, "step counts against the host replicas")
    for tr in (one, per):
        _same_bits(pull(tr.w, OBS), host.first, "observations after evaluate_episodes")
        assert (pull(tr.w, "_timestep_") == 0).all() and (pull(tr.w, "_done_") == 0).all()
    r3, s3 = one.evaluate_episodes(use_argmax=False)
    assert one.evaluation_path == "one launch"
    _documented(r3, s3)
    one.graceful_close()
    per.graceful_close()


def test_trainer_evaluation_sees_the_weights_the_apply_launch_wrote(tmp_path):
    """two iterations with rollout and update in kernels (`fused_update: "all"`), then a greedy evaluation: judged against
    the model fed pack_rollout_policy of the CURRENT parameters -- and not what the parameters before training give"""
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    tr = _trainer(tmp_path, fused_update="all")
    assert tr.rollout_path == "one launch" and tr.update_path == {"shared": "kernels"}
    initial = pack_rollout_policy(tr.models["shared"]).cpu().numpy().astype(f32).copy()
    tr.train(2)
    packed = pack_rollout_policy(tr.models["shared"]).cpu().numpy().astype(f32)
    assert packed.shape == initial.shape and (packed != initial).any() and np.isfinite(packed).all()
    rewards, steps = tr.evaluate_episodes(use_argmax=True)
    assert tr.evaluation_path == "one launch"
    _documented(rewards, steps)
    case = model.Case("rendezvous", E_T, N_T, L_T, T_T, hidden=32, mode="greedy")
    case._config = dict(num_agents=N_T, grid_length=L_T, episode_length=T_T, seed=9)
    host, flagged_total = model.EpisodeReplicas(case.env_class(), case._config, E_T), 0
    for k in range(T_T):
        want, flagged = model.expected_actions(case, packed, host.obs.reshape(E_T * N_T, 5), k)
        flagged_total += int(flagged.sum())
        host.step(want.reshape(E_T, N_T))
    print(f"{flagged_total} flagged decisions of {E_T * N_T * T_T} on the host")
    assert flagged_total == 0, "a condition on the case (host values): choose another seed"
    _same_bits(rewards["shared"], host.total, "reward sums against the model on the current parameters")
    _same_bits(steps["shared"], host.steps, "step counts")
    tr.graceful_close()


def test_trainer_stays_per_tick_without_the_key_and_asks_nothing_of_the_mixin(tmp_path, monkeypatch):
    cls = model.example_module().RendezvousEvaluate
    asked = []
    monkeypatch.setattr(cls, "has_live_policy_evaluate", lambda self, *a: asked.append(a) or True)
    monkeypatch.setattr(cls, "evaluate_launch", lambda self, *a, **k: asked.append(("launch", a)))
    tr = _trainer(tmp_path, rollout=None)
    assert tr.rollout_path == "per tick"
    rewards, steps = tr.evaluate_episodes(use_argmax=True)
    assert tr.evaluation_path == "per tick" and asked == []
    _documented(rewards, steps)
    tr.graceful_close()


def test_trainer_with_a_reset_pool_stays_per_tick(tmp_path):
    from warp_drive_amd.utils.data_feed import DataFeed

    class Pooled(model.example_module().RendezvousEvaluate):
        """the same class with one more array that restarts from a pool: nothing the kits know how to do"""

        def get_data_dictionary(self):
            feed = super().get_data_dictionary()
            feed.add_data(name="mood", data=np.zeros(self.num_agents, dtype=np.int32))
            return feed

        def get_reset_pool_dictionary(self):
            pool = DataFeed()
            pool.add_pool_for_reset(name="mood_reset_pool", reset_target="mood",
                                    data=np.arange(4 * self.num_agents, dtype=np.int32).reshape(4, self.num_agents))
            return pool

    assert Pooled.name == "RendezvousEvaluate"
    tr = _trainer(tmp_path, cls=Pooled, pool_seed=7)
    assert not tr.w.env.has_live_policy_evaluate(32, 5) and not tr.w.env.has_live_policy_rollout(32, 5)
    assert tr.rollout_path == "per tick"
    rewards, steps = tr.evaluate_episodes(use_argmax=True)
    assert tr.evaluation_path == "per tick"
    _documented(rewards, steps)
    tr.graceful_close()
