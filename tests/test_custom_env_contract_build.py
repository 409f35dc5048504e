"""tests/custom_envs/contract_probe.hip without a GPU: the unit compiles to the expected entries without scratch memory,
the host helpers pack the kernarg layouts the entries declare, the host build of include/wd_env_rollout.h computes what
the numpy model computes on every crafted policy, and the cases of tests/test_gpu_custom_env_contract.py -- replayed here
on the host alone -- reach what they are there for.  hipcc cross-compiles gfx950, so no GPU is needed."""
import time

import numpy as np
import pytest

from tests import custom_contract_model as model
from tests.classic_control_cases import NEAR_WINDOW
from tests.custom_rollout_model import near_cap
from tests.test_custom_env_rollout_build import (_batch, _DeviceTensor, _metadata, _StubData, _StubFunctions,  # noqa: F401
                                                 _StubResetter, _StubSampler, cache, policy_check)
from warp_drive_amd import build as wd_build

ROLLOUTS = [f"HipContractProbeRollout_F{F}_H{H}" for F, H in model.SHAPES]
LOGITS = [f"HipContractProbeLogits_F{F}_H{H}" for F, H in model.SHAPES]
KERNELS = sorted(ROLLOUTS + LOGITS + ["HipContractProbeStep", "HipContractProbeTick"])


@pytest.fixture(scope="module")
def unit(tmp_path_factory):
    import os

    saved = os.environ.get("WD_ENV_CACHE")
    os.environ["WD_ENV_CACHE"] = str(tmp_path_factory.mktemp("contract_cache"))
    try:
        start = time.time()
        path = wd_build.build_env_unit("ContractProbe", model.SOURCE)
        print(f"ContractProbe compiled in {time.time() - start:.1f} s")
        return path, _metadata(path)
    finally:
        if saved is None:
            os.environ.pop("WD_ENV_CACHE", None)
        else:
            os.environ["WD_ENV_CACHE"] = saved


# ------------------------------------------------------------------------------------------------------ the build
def test_the_unit_builds_to_the_expected_entries_without_scratch(unit):
    path, meta = unit
    assert wd_build.kernels_in(path) == KERNELS and sorted(meta) == KERNELS
    for kernel, m in sorted(meta.items()):
        print(f"{kernel}: {m['vgprs']} VGPRs, private {m['private']}, spills {m['vgpr_spills']} / {m['sgpr_spills']}, "
              f"static LDS {m['lds']}, at most {m['max_threads']} threads")
        assert (m["private"], m["vgpr_spills"], m["sgpr_spills"]) == (0, 0, 0), kernel
    for (F, H), name in zip(model.SHAPES, ROLLOUTS):
        bound = model.ContractProbe.ROLLOUT_MAX_THREADS[H]
        assert meta[name]["max_threads"] == bound and meta[name]["vgprs"] <= 512 // (bound // 256)
    for name in ROLLOUTS + LOGITS:
        # `int pad[3]`: static LDS that is no multiple of 16 bytes in front of the staged policy (the linker may round the
        # segment up to the dynamic array's alignment)
        assert meta[name]["lds"] in (12, 16), name
    assert meta["HipContractProbeTick"]["lds"] == 0 and meta["HipContractProbeStep"]["lds"] == 0
    assert not any("contractprobe" in u.lower() for u, _ in wd_build.UNITS.values())
    owners = wd_build.in_tree_kernel_owners()
    assert not [k for k in KERNELS if k in owners]


def _stubbed(F, A=5, num_agents=5):
    from warp_drive_amd.managers.function_manager import CUDAFunctionFeed

    env = model.ContractProbe(num_agents=num_agents, episode_length=4, n_actions=A, features=F, num_envs=3)
    env.cuda_function_manager = _StubFunctions(missing=[f"HipContractProbeRollout_F{f}_H{h}" for f in (1, 4, 7)
                                                        for h in (4, 32, 64) if (f, h) not in model.SHAPES])
    env.cuda_data_manager = _StubData({"n_features": np.int32(F)}, num_agents, F)
    env.cuda_step_function_feed = CUDAFunctionFeed(env.cuda_data_manager)
    return env


def _layout(args):
    from warp_drive_amd.managers import hip_driver as drv

    offset, layout = 0, []
    for a in args:
        size = 8 if isinstance(a, drv.DevicePtr) or hasattr(a, "data_ptr") else a.dtype.itemsize
        offset += (-offset) % size
        layout.append((offset, size))
        offset += size
    return layout


@pytest.mark.parametrize("F,H", model.SHAPES, ids=lambda v: str(v))
def test_the_helpers_pack_the_kernarg_layout_of_the_compiled_entries(unit, F, H):
    import torch

    from warp_drive_amd.managers import hip_driver as drv

    _, meta = unit
    A, ticks = 5, 9
    env = _stubbed(F, A)
    widths = sorted(h for f, h in model.SHAPES if f == F)
    assert [h for h in (4, 32, 64) if env.has_live_policy_rollout(h, A)] == widths
    resetter, sampler = _StubResetter(), _StubSampler()
    packed = _DeviceTensor((model.rollout_model.policy_floats(F, H, A),), torch.float32, 0xE0000)
    env.ticks_per_launch = ticks
    fn, args, block, grid, shared = env.tick_launch(sampler, [None], resetter, batch=_batch(3, 5, F, ticks), policy=(packed, H))
    entry = f"HipContractProbeRollout_F{F}_H{H}"
    assert fn.name == entry and block == (64, 1, 1) and grid == (3, 1) and shared % 16 == 0
    assert 0 <= shared - 4 * packed.numel() < 16
    explicit = [a for a in meta[entry]["args"] if not a[2].startswith("hidden_")]
    assert _layout(args) == [(o, s) for o, s, _ in explicit] and len(args) == len(env.TICK_STEP_ARGS) + 11
    assert ["global_buffer" if s == 8 else "by_value" for _, s in _layout(args)] == [k for _, _, k in explicit]
    assert len(drv._pack_args(args)) == max(o + s for o, s, _ in explicit) and int(args[-1]) == ticks
    # the Tick entry: the step's arguments + the 14 trailing ones of wd_env_tick.h
    env.ticks_per_launch = 1
    probs = [_DeviceTensor((3, 5, A), torch.float32, 0xF0000)]
    fn, args, block, _, shared = env.tick_launch(sampler, probs, resetter)
    explicit = [a for a in meta["HipContractProbeTick"]["args"] if not a[2].startswith("hidden_")]
    assert fn.name == "HipContractProbeTick" and shared == 0 and len(args) == len(env.TICK_STEP_ARGS) + 14
    assert _layout(args) == [(o, s) for o, s, _ in explicit]
    # the Logits entry, as the GPU test calls it: policy, A, observation rows, row count, logits, running sums
    explicit = [a for a in meta[env.logits_kernel(H)]["args"] if not a[2].startswith("hidden_")]
    call = [packed, np.int32(A), packed, np.int32(70), packed, packed]
    assert _layout(call) == [(o, s) for o, s, _ in explicit] == [(0, 8), (8, 4), (16, 8), (24, 4), (32, 8), (40, 8)]


# ------------------------------------------------------------------------------------------------ the host program
@pytest.mark.parametrize("F,H", model.SHAPES, ids=lambda v: str(v))
def test_the_host_build_computes_the_models_policy_on_the_crafted_policies(policy_check, F, H):
    """every policy the GPU test hands the Logits entries, on the same 70 rows: logits bit for bit, running sums within
    NEAR_WINDOW, and bit for bit on the uniform, saturated and masked policies"""
    obs = model.logit_rows(F)
    u = np.linspace(2.0 ** -24, 1.0, len(obs)).astype(np.float32)
    names = set()
    for name, A, packed, exact in model.logit_cases(F, H):
        logits, cum, picks = policy_check(H, F, A, packed, obs, u)
        want_logits, want_cum = model.model_logits_and_sums(packed, H, obs, A)
        assert logits.tobytes() == want_logits.tobytes(), (name, np.argwhere(logits != want_logits)[:5].tolist())
        if exact:
            assert cum.tobytes() == want_cum.tobytes(), (name, np.argwhere(cum != want_cum)[:5].tolist())
        else:
            assert float(np.abs(cum.astype(np.float64) - want_cum.astype(np.float64)).max()) < NEAR_WINDOW, name
        assert picks.min() >= 0 and picks.max() <= A - 1
        names.add(name.split("-")[0].rstrip("0123456789"))
    assert names == {"random", "dead", "saturated", "masked", "uniform"}


# --------------------------------------------------------------------------------- the GPU cases, on the host alone
def test_the_logit_cases_cannot_pass_vacuously():
    for F, H in model.SHAPES:
        obs = model.logit_rows(F)
        assert (obs[-2:] == 0).all() and np.signbit(obs[-1]).all() and not np.signbit(obs[-2]).any()
        assert obs.min() <= -7 and obs.max() >= 7 and np.abs(obs).max() <= 8
        if F >= 3:
            assert (np.abs(obs * 2) % 2 == 1).any()   # a half
        probe = obs[:-2]
        assert (probe == 0).any() and (np.signbit(probe) & (probe == 0)).any()   # 0.0 and -0.0 among the probe's own rows
        for A in model.ACTIONS:
            pol = model.policies(F, H, A)
            live = model.first_layer(pol["random1"][0], F, H, A, obs) > 0
            assert live.any(axis=1).sum() >= 10, (F, H, A)   # rows whose first layer is not dead
            assert (model.first_layer(pol["dead"][0], F, H, A, obs) < 0).all(), (F, H, A)
            logits, _ = model.model_logits_and_sums(pol["dead"][0], H, obs, A)
            assert (logits == logits[0]).all()   # the biases alone: one row of logits for every observation
            logits, _ = model.model_logits_and_sums(pol["random1"][0], H, obs, A)
            assert len({row.tobytes() for row in logits}) > len({row.tobytes() for row in obs}) // 2
            if A >= 2:
                for w in model.saturated_winners(A):
                    logits, cum = model.model_logits_and_sums(pol[f"saturated{w}"][0], H, obs, A)
                    assert (logits[:, w] - np.delete(logits, w, axis=1).max(axis=1) > 110).all()
                    assert (cum[:, :w] == 0).all() and (cum[:, w:] == 1).all()
                logits, cum = model.model_logits_and_sums(pol["masked"][0], H, obs, A)
                assert np.isneginf(logits[:, 0]).all() and (cum[:, 0] == 0).all() and (A < 3 or np.isneginf(logits[:, -1]).all())
        for A in model.UNIFORM_ACTIONS:
            logits, cum = model.model_logits_and_sums(model.uniform_policy(F, H, A), H, obs, A)
            assert (logits == np.float32(0.75)).all() and (cum[:, 0] == np.float32(1) / np.float32(A)).all()


def _seed_words():
    return tuple(int(v) for v in model.tick_model.seed_words(model.END_SEED))


@pytest.mark.parametrize("variant", [0, 1])
def test_the_tick_plans_reach_both_ends_the_wrap_and_the_clamp(variant):
    for sizes in ((3, 2, 7, 5), (5,)):
        plan = model.tick_plan(*_seed_words(), sizes, variant)
        H = len(sizes)
        assert sorted(plan["roles"].values()) == sorted((h, k) for h in range(H) for k in ("hi", "lo"))
        last, want = plan["u"][-1], plan["want"][-1].reshape(-1, H)
        for row, (h, kind) in plan["roles"].items():
            assert last[row, h] == (np.float32(1.0) if kind == "hi" else np.float32(2.0 ** -24))   # both ends are drawn
            p = plan["probs"][h].reshape(-1, sizes[h])[row]
            unclamped, with_le = model.pick_variants(p, last[row, h])
            if kind == "hi" and variant == 1:
                assert unclamped == sizes[h] and want[row, h] == sizes[h] - 1    # only the clamp keeps it in range
            if kind == "hi" and variant == 0:
                assert with_le != want[row, h] and p[want[row, h]] > 0 and (p[want[row, h] + 1:] == 0).all()
            if kind == "lo":
                assert p[0] == 0 and p[want[row, h]] > 0 and (p[:want[row, h]] == 0).all()
        # a wrap happens inside the launch
        assert plan["epochs"][plan["wrap"]].tolist() == [0xFFFFFFFF, 0xFFFFFFFE]
        assert plan["epochs_after"][plan["wrap"]].tolist() == [2, 1]
        # the one-ulp rows: below picks 1, equal and above pick 0, for every head of two or more actions
        rows = np.array([r for r in range(len(last)) if r not in plan["roles"]])
        for h, A in enumerate(sizes):
            assert (want[rows[rows % 4 == 0], h] == 1).all() and (want[rows[(rows % 4 == 1) | (rows % 4 == 2)], h] == 0).all()
            p = plan["probs"][h].reshape(-1, A)
            _, with_le = model.pick_variants(p, last[:, h])
            assert (with_le != want[:, h]).sum() >= len(rows) // 4 - 1   # `<=` for `<` changes every "equal" row


@pytest.mark.parametrize("F,H", [(4, 32), (7, 64)], ids=lambda v: str(v))
def test_the_rollout_plans_need_no_excused_draw(F, H):
    """the modelled near-threshold count is 0 for every crafted policy (so the GPU test excuses nothing there) and within
    near_cap's rule for the random one; both ends are drawn, and mean something"""
    draws = model.END_E * model.END_N * model.END_TICKS
    seen = set()
    for name, A, packed, crafted in model.end_policies(F, H):
        plan = model.rollout_plan(*_seed_words(), F, H, A, packed, crafted)
        near = int(plan["near"].sum())
        print(f"F {F} H {H} {name}: {near} modelled near-threshold draws of {draws}")
        assert near <= (0 if crafted else near_cap(draws, A)), name
        assert sorted(plan["roles"].values()) == [(0, "hi"), (0, "lo")]
        for row, (_, kind) in plan["roles"].items():
            u, cum, want = plan["u"][-1][row], plan["cum"][-1][row], plan["want"][-1][row]
            assert u == (np.float32(1.0) if kind == "hi" else np.float32(2.0 ** -24))
            if kind == "lo" and name.startswith("masked"):
                assert cum[0] == 0 and want >= 1            # a zero-probability leading action is not drawn
            if kind == "hi" and name == "saturated0-A5":
                assert want == 0 and (cum == 1).all()       # `<=` for `<` would give A - 1
        seen |= set(plan["want"].reshape(-1).tolist())
        assert plan["epochs_after"][plan["wrap"]].tolist() == [2, 1]
    assert len(seen) >= 5


def test_the_restart_cases_finish_inside_a_launch_and_on_its_last_tick():
    for N in model.RESTART_AGENTS:
        host = model.HostProbe(model.restart_config(N, 7))
        draws = model.tick_model.TickDraws(model.RESTART_SEED, model.RESTART_E, N, model.TICK_TAG)
        probs = model.restart_probabilities(N)
        changed = set()
        for T in model.RESTART_LAUNCHES:
            assert T <= 9
            for k in range(T):
                before = host.state()
                rewards, done = host.step(draws.draw([probs])[..., 0], last_tick=k == T - 1)
                assert (rewards != model.REWARD_AT_RESET).all()   # no step stores the reference value
                after = host.state()
                changed |= {k2 for k2 in ("per_env", "odd", "wide") if not np.array_equal(before[k2], after[k2])}
                if done.all():
                    assert (after["per_env"] == model.PER_ENV_AT_RESET).all() and (host.rewards == model.REWARD_AT_RESET).all()
                    assert after["odd"].tobytes() == np.tile(model.ODD_AT_RESET, model.RESTART_E).tobytes()
        assert host.inside == 4 * model.RESTART_E and host.on_last == model.RESTART_E and changed == {"per_env", "odd", "wide"}
        assert 7 * N > (N + 63) // 64 * 64 or N < 64   # `wide`: a row longer than the block wherever the block is full
    assert sum(model.RESTART_LAUNCHES) % model.RESTART_L == 0


@pytest.mark.parametrize("F,H", [(1, 4), (7, 32)], ids=lambda v: str(v))
def test_the_restart_rollouts_stay_within_near_cap_and_draw_every_action(F, H):
    """the Rollout cases of the restart test on the host alone (host step, the model, the Philox replay): the modelled
    near-threshold count is within near_cap's rule -- a condition on the cases, not a measurement of the device"""
    from tests.classic_control_cases import near_threshold
    from tests.classic_control_policy import count_below

    E, A = model.RESTART_E, model.RESTART_A
    packed = model.policies(F, H, A)["random2"][0]
    for N in model.RESTART_AGENTS:
        host = model.HostProbe(model.restart_config(N, F))
        near, seen, ticks = 0, np.zeros(A, np.int64), sum(model.RESTART_LAUNCHES)
        for tick in range(ticks):
            cum = model.model_logits_and_sums(packed, H, host.obs.reshape(E * N, F), A)[1]
            u = model.rollout_model.replayed_uniform(model.RESTART_SEED, E * N, tick)
            near += int(near_threshold(cum, u).sum())
            actions = count_below(cum, u)
            seen += np.bincount(actions, minlength=A)
            host.step(actions.reshape(E, N))
        print(f"F {F} H {H} N {N}: {near} modelled near-threshold draws of {E * N * ticks}, actions {seen.tolist()}")
        assert near <= near_cap(E * N * ticks, A)
        if N >= 70:
            assert (seen > 0).sum() >= 3


def test_the_host_build_takes_a_nan_activation_for_zero(policy_check):
    """a NaN and a +inf planted in W1: the header's ReLU is C's fmaxf(acc, 0), which returns 0 for a NaN, so the host build
    of the header gives the logits of the model WITH np.fmax for its ReLU -- not the numpy model's, whose np.maximum hands
    the NaN on to every logit.  (What the device returns is printed by the GPU test and recorded in docs/rounds/r37.md.)"""
    F, H, A = 7, 32, 5
    packed, obs = model.non_finite_policy(F, H, A), model.logit_rows(F)
    u = np.linspace(2.0 ** -24, 1.0, len(obs)).astype(np.float32)
    logits, cum, picks = policy_check(H, F, A, packed, obs, u)
    want = model.policy_logits_fmax(packed, F, H, A, obs)
    print(f"host build, row 0: logits {logits[0].tolist()}, running sums {cum[0].tolist()}; "
          f"rows with a NaN logit {int(np.isnan(logits).any(axis=1).sum())} of {len(obs)}")
    assert model.same_bits_or_both_nan(logits, want)
    assert np.isnan(model.model_logits_and_sums(packed, H, obs, A)[0]).all()
    assert picks.min() >= 0 and picks.max() <= A - 1
