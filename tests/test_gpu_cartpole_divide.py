"""Cartpole's division shortcut on the device, where it is used: wd_test_cartpole_divide (the test-only code object) calls
the shipping cp_div_invariant and cp_div_in_window for every float32 dividend it is given and counts; the counts are judged
by the host model of tests/cartpole_divide_cases.py -- the whole window per named divisor, and one binade exhaustively where
the model says the shortcut fails.  Then the verdict the env acts on (the proof flag AND the kernels' mass predicate must
imply a clean window) and recorded rollouts through the Tick, Rollout_H32 and Rollout_P entries with a total mass and a
force whose every force quotient overflows: the oracle records infinities, the shortcut would record NaN.
Tolerance 0 everywhere.  `pytest -s` prints the counts and the launch times."""
import time

import numpy as np
import pytest

from tests import cartpole_divide_cases as cd

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32
ALL_MAGNITUDES = (0, 1 << 31)   # every magnitude pattern, each with its negation: all 2^32 float32
_counts = {}                    # (divisor bits, first, n) -> (inside, differ, seconds): one launch per key and session


def _fm():
    from tests.hip_harness import make_wrapper, require_gpu
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv

    require_gpu()
    if "fm" not in _counts:
        _counts["fm"] = make_wrapper(CUDAClassicControlCartPoleEnv(episode_length=20, seed=1), 8)
    return _counts["fm"].cuda_function_manager


def _count(c, first, n, y=None):
    """(dividends inside the window, mismatches among them, seconds) of one launch over the magnitude patterns
    first .. first + n - 1 and their negations"""
    import torch
    from warp_drive_amd.managers import hip_driver as drv

    key = (int(F32(c).view(U32)), first, n, None if y is None else int(F32(y).view(U32)))
    if key not in _counts:
        _fm()
        if "fn" not in _counts:
            _counts["fn"] = drv.Module(drv.code_object_of("wd_test_cartpole_divide")).get_function("wd_test_cartpole_divide")
        fn = _counts["fn"]
        out = torch.zeros(2, dtype=torch.int64, device="cuda")
        with np.errstate(all="ignore"):
            recip = F32(1.0) / F32(c) if y is None else F32(y)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(F32(c), recip, U32(first), U32(n), out, block=(256, 1, 1), grid=(8192, 1))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        inside, differ = (int(v) for v in out.cpu().numpy())
        _counts[key] = (inside, differ, dt)
    return _counts[key]


def _env_verdict(d):
    """invariant_divide_ok() of an env with the divisor's masses (what tick_launch hands to the kernels)"""
    from tests.hip_harness import make_wrapper
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv

    _fm()
    env = CUDAClassicControlCartPoleEnv(episode_length=20, seed=1)
    env.physics = type("Physics", (env.physics,), d.physics())
    make_wrapper(env, 8)
    assert F32(env.physics.masspole + env.physics.masscart) == d.c
    return env.invariant_divide_ok()


# ------------------------------------------------------------------------------------------------ part 2: the counts
@pytest.mark.parametrize("d", cd.DIVISORS, ids=repr)
def test_device_counts_over_the_whole_window(d):
    """all 2^32 dividends in one launch: the count inside the window is the one its bounds give; the mismatch count is
    zero exactly where the host model's verdict is clean; where it is not, one failing binade, both signs, counted again
    on its own, equals the host model's exhaustive count (tests/cartpole_divide_cases.py's table, pinned by the host
    test).  The underflow-side counts also say whether these three instructions keep float32 subnormals under this
    build: they do iff the counts agree."""
    inside, differ, dt = _count(d.c, *ALL_MAGNITUDES)
    print(f"{d.name}: {inside} dividends inside the window, {differ} mismatches, {dt * 1e3:.1f} ms")
    assert dt < 2.0, "split the launch: a single one was to stay under two seconds"
    assert inside == cd.window_count(*ALL_MAGNITUDES) == 2 * cd.WINDOW_SPAN
    assert (differ == 0) == d.clean, (d.name, differ)
    if not d.clean:
        first = (d.binade + 127) << 23
        b_inside, b_differ, b_dt = _count(d.c, first, 1 << 23)
        print(f"{d.name}: binade 2^{d.binade}: {b_differ} of {b_inside} differ (host model: {d.count}), {b_dt * 1e3:.1f} ms")
        assert b_inside == cd.window_count(first, 1 << 23) == 1 << 24
        assert b_differ == d.count and differ >= b_differ


def test_the_count_sees_a_wrong_reciprocal_and_the_window_edges():
    """the entry is no rubber stamp: with a reciprocal some places off the classic divisor fails in its own binade exactly as
    often as the host model says (the correction step forgives ONE place, 0 mismatches: which is why the verifier compares
    the reciprocal itself); patterns outside the window are not counted, whatever they would give"""
    c = cd.BY_NAME["classic-1.1"].c
    y = F32(1.0) / c
    one = (0 + 127) << 23
    assert _count(c, one, 1 << 23)[:2] == (1 << 24, 0)
    seen = []
    for places in (1, 8, 64):
        wrong = np.array([int(y.view(U32)) + places], U32).view(F32)[0]
        inside, differ, _ = _count(c, one, 1 << 23, y=wrong)
        assert inside == 1 << 24 and differ == cd.binade_mismatches(c, 0, y=wrong), (places, differ)
        seen.append(differ)
    assert seen[0] == 0 and 0 < seen[1] < seen[2], seen
    below, above = cd.WINDOW_FIRST - 1000, cd.WINDOW_FIRST + cd.WINDOW_SPAN - 1000
    assert _count(c, below, 2000)[:2] == (cd.window_count(below, 2000), 0) == (2000, 0)
    assert _count(c, above, 2000)[:2] == (cd.window_count(above, 2000), 0) == (2000, 0)
    assert _count(cd.BY_NAME["1.5*2^126"].c, 0, cd.WINDOW_FIRST)[:2] == (0, 0)           # zero and everything below 2^-90
    assert _count(c, cd.WINDOW_FIRST + cd.WINDOW_SPAN, (1 << 31) - cd.WINDOW_FIRST - cd.WINDOW_SPAN)[:2] == (0, 0)   # 2^90 .. NaN


# ------------------------------------------------------------------------------------------------ part 3: the verdict
@pytest.mark.parametrize("d", cd.DIVISORS, ids=repr)
def test_what_the_env_acts_on_implies_a_clean_window(d):
    """invariant_divide_ok() == 1 and the kernels' mass predicate (host model of cp_fast_masses_ok, constants read out of
    the source by the host test) => the device finds no mismatch in the window.  Without a bound on the total mass every
    out-of-band divisor of the table breaks this: the two-binade proof passes for all of them."""
    ok = _env_verdict(d)
    fast = cd.fast_predicate(d.masspole, d.c)
    differ = _count(d.c, *ALL_MAGNITUDES)[1]
    print(f"{d.name}: invariant_divide_ok {ok}, mass predicate {fast}, {differ} mismatches in the window")
    assert ok in (0, 1)
    assert not (ok == 1 and fast) or differ == 0, (d.name, ok, fast, differ)
    if d.name in ("classic-1.1", "masspole-0.25", "masscart-2^20"):
        assert ok == 1 and fast   # (the fix does not switch the fast ticks off)


def test_verdicts_are_kept_per_total_mass():
    """the verifier still notices a reciprocal one place off and still passes the classic mass; replacing `physics` on one
    env object launches it again and gives that mass's verdict, asking twice does not"""
    import torch
    from tests.hip_harness import make_wrapper
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv
    from warp_drive_amd.managers import hip_driver as drv

    fm = _fm()
    fm.initialize_functions(["HipCartPoleVerifyInvariantDivide"])
    verify = fm.get_function("HipCartPoleVerifyInvariantDivide")
    ok = torch.ones(1, dtype=torch.int32, device="cuda")
    for d in (cd.BY_NAME["classic-1.1"], cd.BY_NAME["masscart-2^20"], cd.BY_NAME["sqrt3*2^-60"]):
        y = F32(1.0) / d.c
        for recip, want in ((y, 1), (np.nextafter(y, F32(np.inf)), 0), (np.nextafter(y, F32(0.0)), 0)):
            ok.fill_(1)
            verify(d.c, recip, ok, block=(256, 1, 1), grid=(4096, 1), shared=0)
            assert int(ok.item()) == want, (d, recip)
    env = CUDAClassicControlCartPoleEnv(episode_length=20, seed=1)
    make_wrapper(env, 8)
    name = "HipCartPoleVerifyInvariantDivide"
    before = drv.LAUNCH_COUNTS[name]
    assert env.invariant_divide_ok() == 1 and env.invariant_divide_ok() == 1
    assert drv.LAUNCH_COUNTS[name] == before + 1
    classic = env.physics
    env.physics = type("Physics", (classic,), cd.BY_NAME["masscart-2^20"].physics())
    assert env.invariant_divide_ok() == 1 and drv.LAUNCH_COUNTS[name] == before + 2
    env.physics = classic
    assert env.invariant_divide_ok() == 1 and drv.LAUNCH_COUNTS[name] == before + 2   # a mass seen before: no launch
    assert sorted(env._inv_div_verdicts) == sorted(F32(v).tobytes() for v in (F32(1.1), cd.BY_NAME["masscart-2^20"].c))
    # two more masses, each verdict the host model's of the two proof binades (the table's `proof`, pinned by the host
    # test); the reciprocal of the first is subnormal -- the kernel compares it with its own 1.0f / c
    for d in (cd.BY_NAME["1.5*2^126"], cd.BY_NAME["1.25*2^60"]):
        env.physics = type("Physics", (classic,), d.physics())
        assert env.invariant_divide_ok() == int(d.proof), d
    assert drv.LAUNCH_COUNTS[name] == before + 4


# ------------------------------------------------------------------------------------------------ part 3: the rollouts
def test_overflow_rollout_through_the_tick_entry():
    """tests/test_gpu_core.py's recorded rollout (every row against the oracle, NaN equal to NaN only) with the overflow
    physics: row 1 of every launch holds +-inf in both velocities.  The proof flag is 1 (the proof passes); the kernels
    must not take the fast ticks all the same."""
    from tests.test_gpu_core import _cartpole_recorded_rollout

    d = cd.BY_NAME["sqrt3*2^-60"]
    with np.errstate(all="ignore"):
        flag = _cartpole_recorded_rollout(cd.ROLLOUT_E, cd.ROLLOUT_LAUNCHES, dict(cd.OVERFLOW_PHYSICS))
    assert flag == int(cd.proof_passes(d.c)) == 1 and not cd.fast_predicate(d.masspole, d.c)


def test_in_band_rollout_off_the_tested_masses_stays_fast():
    """a cart of 2^20: proof flag 1, mass predicate true -- the middle ticks run cp_euler<true> -- and every row is the oracle's"""
    from tests.test_gpu_core import _cartpole_recorded_rollout

    d = cd.BY_NAME["masscart-2^20"]
    assert _cartpole_recorded_rollout(cd.ROLLOUT_E, cd.ROLLOUT_LAUNCHES, dict(cd.IN_BAND_PHYSICS)) == 1
    assert cd.fast_predicate(d.masspole, d.c) and d.clean


def test_overflow_rollout_through_the_live_policy_entry():
    """HipClassicControlCartPoleEnvRollout_H32 with the overflow physics, 16 ticks, 3 launches: observation, reward and done
    rows and the state against the oracle (NaN equal to NaN only).  The action: on a finite observation the rule of
    test_cartpole_rollout_with_the_policy_inside_the_kernel (the host's draw, except within 2e-6 of the threshold); on an
    observation that holds an infinity the network has no host restatement (0 * inf, max(NaN, 0)) -- any action of the
    two; the oracle follows the device's action either way."""
    import torch
    from oracle.cartpole_np import CartPoleOracle, policy_probabilities
    from oracle.core_np import single_head_tick_uniform
    from tests.hip_harness import make_wrapper, pull, require_gpu
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.managers.function_manager import HIPSampler, _stream_tag
    from warp_drive_amd.rollout import RolloutEngine
    from warp_drive_amd.training.models import FullyConnected
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    require_gpu()
    E, T, ticks, hidden = cd.ROLLOUT_E, 23, cd.ROLLOUT_TICKS, 32
    torch.manual_seed(5)
    model = FullyConnected(4, [2], [hidden, hidden])
    with torch.no_grad():
        model.policy_head[0].weight.mul_(6.0)
    packed = pack_rollout_policy(model).cuda()
    env = CUDAClassicControlCartPoleEnv(episode_length=T, seed=32145)
    env.physics = type("Physics", (env.physics,), dict(cd.OVERFLOW_PHYSICS))
    env.ticks_per_launch = ticks
    w = make_wrapper(env, E)
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=4)
    probs = torch.full((E, 1, 2), 0.5, device="cuda")
    batch = {"obs": torch.full((ticks, E, 1, 4), 7.0, device="cuda"),
             "actions": torch.full((ticks, E, 1, 1), -1, dtype=torch.int32, device="cuda"),
             "rewards": torch.full((ticks, E, 1), -1.0, device="cuda"),
             "done": torch.full((ticks, E), -1, dtype=torch.int32, device="cuda")}
    eng = RolloutEngine(w, sampler, probabilities=[probs], rollout_batch=batch, rollout_policy=(packed, hidden))
    assert eng.step_kernel_name == "HipClassicControlCartPoleEnvRollout_H32" and eng.ticks_per_launch == ticks
    orc = type("Oracle", (CartPoleOracle,), dict(cd.OVERFLOW_PHYSICS))(E, T, initial_state=pull(w, "state")[0, 0])
    rng_words = np.zeros(4 + E, dtype=np.uint32)
    finished = infinite_rows = judged = 0
    with np.errstate(all="ignore"):
        for launch in range(cd.ROLLOUT_LAUNCHES):
            drv.memcpy_dtoh(rng_words, sampler.rng_state)
            torch.cuda.synchronize()
            eng.run(1)
            torch.cuda.synchronize()
            b = {k: v.cpu().numpy() for k, v in batch.items()}
            for k in range(ticks):
                np.testing.assert_array_equal(b["obs"][k, :, 0], orc.obs, err_msg=f"obs row {k} of launch {launch}")
                got = b["actions"][k, :, 0, 0]
                assert set(np.unique(got)) <= {0, 1}
                finite = np.isfinite(orc.obs).all(axis=1)
                p = policy_probabilities(packed.cpu().numpy(), hidden, orc.obs[finite])
                u = single_head_tick_uniform(E, rng_words[4:] + np.uint32(k), rng_words[0], rng_words[1], _stream_tag("tick"))[finite]
                bad = got[finite] != (p[:, 0] < u).astype(np.int32)
                assert (np.abs(p[bad, 0] - u[bad]) < 2e-6).all(), (launch, k, p[bad, 0], u[bad])
                judged += int(finite.sum())
                infinite_rows += int((~finite).sum())
                orc.step(got.reshape(E, 1, 1))
                np.testing.assert_array_equal(b["rewards"][k, :, 0], orc.rewards)
                np.testing.assert_array_equal(b["done"][k], orc.done, err_msg=f"done row {k} of launch {launch}")
                finished += int((orc.done > 0).sum())
                orc.reset_done_envs()
            np.testing.assert_array_equal(pull(w, "state")[:, 0], orc.state)
            np.testing.assert_array_equal(pull(w, "_timestep_"), orc.timestep)
    assert env.invariant_divide_ok() == 1
    assert finished >= E and infinite_rows >= E and judged >= E, (finished, infinite_rows, judged)


def test_overflow_rollout_through_the_pool_entry():
    """HipClassicControlCartPoleEnvRollout_P (its `fast` predicate is cartpole_pool.hip's own line), the smallest pool the
    pool tests use, staged in LDS so that the launch may be fast at all: tests/cartpole_pool_cases.py's model with the
    overflow physics, every array after every launch, bit for bit"""
    from oracle.cartpole_np import CartPoleOracle
    from tests import cartpole_pool_cases as cp
    from tests import test_gpu_cartpole_pool_rollout as pool
    from tests.hip_harness import OBS

    sh = pool._shapes()
    case = cp.PoolCase("overflow", 0, pool=2, E=1501, T=23, ticks=cd.ROLLOUT_TICKS, rows=cd.ROLLOUT_TICKS)
    case.E = cd.ROLLOUT_E          # (the case class lists the replica counts of ITS cases; nothing in it depends on the list)
    case.physics = dict(cd.OVERFLOW_PHYSICS)
    assert case.launches == cd.ROLLOUT_LAUNCHES and case.pool == min(c.pool for c in cp.CASES)
    dev = pool._device(case, "lds")
    fn, args, block, grid, shared = dev["launch"]
    assert fn.name == "HipClassicControlCartPoleEnvRollout_P" and int(args[-1]) == 1 and int(args[-5]) == 1   # staged; proof flag
    words0 = sh._tick_start(dev["w"], case, dev["sampler"], dev["start"])
    model = cp.PoolModel(case)
    model.orc.__class__ = type("Oracle", (CartPoleOracle,), dict(cd.OVERFLOW_PHYSICS))
    T, infinite = case.ticks, 0
    with np.errstate(all="ignore"):
        for li in range(case.launches):
            fn(*args, block=block, grid=grid, shared=shared)
            sh._sync()
            snap = pool._snapshot(dev, case)
            tag = f"launch {li}"
            rows = model.launch(cp.FollowDevice(case, snap["batch_actions"][:T, :, 0, 0]))
            infinite += int(np.isinf(rows["obs"]).any(axis=2).sum())
            sh.EQ(snap["batch_obs"][:T, :, 0], rows["obs"], f"{tag} obs rows")
            sh.EQ(snap["batch_actions"][:T, :, 0, 0], rows["actions"], f"{tag} action rows")
            sh.EQ(snap["batch_rewards"][:T, :, 0], rows["rewards"], f"{tag} reward rows")
            sh.EQ(snap["batch_done"][:T], rows["done"], f"{tag} done rows")
            st = model.state()
            sh.EQ(snap["state"][:, 0], st["state"], f"{tag} state")
            sh.EQ(snap[OBS][:, 0], st["obs"], f"{tag} observation")
            sh.EQ(snap["_timestep_"], st["timestep"], f"{tag} timestep")
            sh.EQ(snap["_done_"], st["done"], f"{tag} done")
            sh.EQ(snap["rng"][:4], words0[:4], f"{tag} RNG header")
            sh.EQ(snap["rng"][4:], st["epochs"], f"{tag} RNG epochs")
            sh.EQ(snap["pool_rng"][4:], st["pool_epochs"], f"{tag} pool epochs")
    assert not np.isnan(rows["obs"]).any() and infinite >= case.E and int(model.restarts.sum()) >= case.E
