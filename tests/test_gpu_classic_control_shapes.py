"""The Step, Tick and Rollout_H32 / _H64 entries of Cartpole (csrc/kernels/cartpole.hip) and of Acrobot, MountainCar,
ContinuousMountainCar and Pendulum (csrc/kernels/classic_control.hip) off their one tested shape: launched directly with
the arguments `step_launch()` / `tick_launch()` build at other blocks and grids than the host picks (several trips of the
grid-stride loop, partial wavefronts, blocks without a replica), with launches that start in the middle of a Philox quad
and cross the 2^32 wrap, launches longer than an episode, batch tensors with surplus rows, pools of 2 / 7 / 16 rows and
none, 1 .. 12 actions, crafted probability rows, a third reset array (Cartpole's uncached restore) and other physics.
The cases live in tests/classic_control_cases.py; tests/test_classic_control_shapes_logic.py asserts on the host that each
reaches what it is there for.  The yardstick of the tick is a second wrapper driven by the Step kernel at the host's
geometry and reset_when_done with the draws replayed (Cartpole: oracle/cartpole_np.py, bit for bit); every comparison is
at tolerance 0 except the float64-flow floats of the Step entries against numpy (1 float32 ulp) and the rollout's
near-threshold draws.  `pytest -s` prints one line per case and geometry."""
import numpy as np
import pytest

from tests import classic_control_cases as cc

pytestmark = pytest.mark.gpu

F32 = np.float32


# ------------------------------------------------------------------------------------------------------- plumbing
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def EQ(got, want, tag=""):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(tag))


def _put(w, name, arr):
    import torch
    from warp_drive_amd.managers import hip_driver as drv

    dm = w.cuda_data_manager
    arr = np.ascontiguousarray(arr)
    assert arr.size == int(np.prod(dm.get_shape(name))) and str(arr.dtype) in str(dm.get_dtype(name)), (name, arr.dtype)
    drv.memcpy_htod(dm.device_data(name), arr)
    torch.cuda.synchronize()


def _sync():
    import torch

    torch.cuda.synchronize()


def _words(ptr, n):
    import torch
    from warp_drive_amd.managers import hip_driver as drv

    out = np.zeros(4 + n, dtype=np.uint32)
    drv.memcpy_dtoh(out, ptr)
    torch.cuda.synchronize()
    return out


def _put_words(ptr, words):
    import torch
    from warp_drive_amd.managers import hip_driver as drv

    drv.memcpy_htod(ptr, np.ascontiguousarray(words, dtype=np.uint32))
    torch.cuda.synchronize()


def _wrapper(case):
    from tests.hip_harness import make_wrapper, require_gpu

    require_gpu()
    w = make_wrapper(cc.make_env(case.env, case.T, getattr(case, "pool", 0), case.physics), case.E)
    if getattr(case, "pool", 0):
        w.init_reset_pool(seed=cc.POOL_SEED)
    return w


def _count_ulp(a, b):
    from tests.hip_harness import ulp_diff

    d = ulp_diff(a, b)
    assert d.max(initial=0) <= 1, int(d.max())
    return int((d.reshape(len(d), -1) > 0).any(axis=1).sum())


def _act_dtype(env):
    return np.int32 if env in cc.DISCRETE else np.float32


# ----------------------------------------------------------------------------------------------------------- Step
@pytest.mark.parametrize("case", cc.STEP_CASES, ids=repr)
def test_step_geometries(case):
    """Every geometry leaves byte-identical state, observation, reward, `_done_` and `_timestep_` to the host's own after
    every tick; the host's geometry is compared per tick with the numpy step on the device's own pre-step state
    (test_step_vs_numpy's rule: float64-flow floats within 1 float32 ulp, float32-flow and discrete outputs exact;
    Cartpole bit for bit against CartPoleOracle), the crafted rows (wall, goal, clipped speed, the time-out that
    coincides with the goal, wraps and bounds, unwrapped angles) among them."""
    from tests.hip_harness import ACT, OBS, REW, pull
    from warp_drive_amd.envs.classic_control import acrobot_obs, apply_done

    env, E, T = case.env, case.E, case.T
    w = _wrapper(case)
    fn, args, block, grid, shared = w.env.step_launch()
    assert fn.name == cc.ENTRY[env] + "Step" and shared == 0
    step = cc.numpy_step(env, case.physics)
    state0, ts0 = case.start()
    acts = case.actions()
    names = ("state", OBS, REW, "_done_", "_timestep_")
    product = []
    for geom in cc.geometries(E):
        threads, blocks, trips = cc.geometry(E, geom, product=(block[0], grid[0]))
        assert threads <= cc.LAUNCH_BOUND and (geom == "product" or not isinstance(geom[1], int) or trips >= 3)
        _put(w, "state", state0)
        _put(w, "_timestep_", ts0)
        _put(w, "_done_", np.zeros(E, np.int32))
        _put(w, OBS, np.full((E, cc.OBS_DIM[env]), 7.0, F32))
        ulp_rows = restarts = terminal = 0
        for t in range(case.ticks):
            s_pre, ts_pre = pull(w, "state")[:, 0].copy(), pull(w, "_timestep_").copy()
            _put(w, ACT, acts[t].astype(_act_dtype(env)))
            _put(w, REW, np.full(E, -7.0, F32))
            fn(*args, block=(threads, 1, 1), grid=(blocks, 1), shared=0)
            _sync()
            got = {n: pull(w, n) for n in names}
            tag = f"{case.name} {geom} tick {t}"
            if geom == "product":
                st, ob, rw, dn = got["state"][:, 0], got[OBS][:, 0], got[REW][:, 0], got["_done_"]
                es, eo, er, term = step(s_pre, acts[t])
                EQ(got["_timestep_"], ts_pre + 1, tag)
                EQ(dn, apply_done(term, ts_pre + 1, T), tag)
                if env == "cartpole":
                    EQ(st, es, tag), EQ(ob, eo, tag), EQ(rw, er, tag)
                else:
                    ulp_rows += _count_ulp(st, es) + _count_ulp(ob, eo) + _count_ulp(rw, er)
                if env == "acrobot":   # float32 flow from the device's own state: bit for bit
                    EQ(ob, acrobot_obs(st), tag)
                    c = np.ascontiguousarray
                    term_dev = (-np.cos(c(st[:, 0])) - np.cos(c(st[:, 1] + st[:, 0]))) > F32(1.0)
                    EQ(rw, np.where(term_dev, 0.0, -1.0).astype(F32), tag)
                    EQ(dn, apply_done(term_dev.astype(np.int32), ts_pre + 1, T), tag)
                if env == "mountain_car":
                    EQ(rw, np.full(E, -1.0, F32), tag)
                product.append(got)
            else:
                for n in names:
                    assert got[n].tobytes() == product[t][n].tobytes(), (tag, n)
            restarts += int((got["_done_"] > 0).sum())
            terminal += int(((got["_done_"] > 0) & (ts_pre + 1 < T)).sum())
            w.reset_only_done_envs()
        print(f"{case.name} [{fn.name}] geometry {geom}: {threads} threads x {blocks} blocks, {trips} trips; {restarts} "
              f"restarts ({terminal} terminal), {len(case.crafted())} crafted rows, {ulp_rows} rows 1 ulp apart")
        assert restarts >= E


# ----------------------------------------------------------------------------------------------------------- Tick
class _DeviceYardstick:
    """a second wrapper: the Step kernel at the host's geometry + reset_when_done"""

    def __init__(self, case, state0, ts0):
        from tests.hip_harness import OBS, pull

        self.case, self.w = case, _wrapper(case)
        self.obs0 = pull(self.w, OBS).copy()
        self.state0, self.ts0 = state0, ts0
        self.pool_words0 = _words(self.w.env_resetter._pool_rng, case.E) if case.pool else None
        self.rewind()

    def rewind(self):
        """back to the case's start (a rollout case replays once per geometry)"""
        from tests.hip_harness import OBS

        case = self.case
        _put(self.w, "state", self.state0)
        _put(self.w, "_timestep_", self.ts0)
        _put(self.w, "_done_", np.zeros(case.E, np.int32))
        _put(self.w, OBS, self.obs0)
        if case.pool:
            words = self.pool_words0.copy()
            words[4:] = case.start_pool_epochs()
            _put_words(self.w.env_resetter._pool_rng, words)

    def obs(self):
        from tests.hip_harness import OBS, pull

        return pull(self.w, OBS)[:, 0].copy()

    def step(self, a):
        from tests.hip_harness import ACT, REW, pull

        _put(self.w, ACT, np.asarray(a, _act_dtype(self.case.env)))
        self.w.step_all_envs()
        return pull(self.w, "_done_").copy(), pull(self.w, REW)[:, 0].copy()

    def restart(self):
        self.w.reset_only_done_envs()

    def final(self):
        from tests.hip_harness import pull

        out = {"state": pull(self.w, "state")[:, 0].copy(), "obs": self.obs(), "ts": pull(self.w, "_timestep_").copy()}
        if self.case.pool:
            out["pool_words"] = _words(self.w.env_resetter._pool_rng, self.case.E)
        return out


class _CartpoleYardstick:
    """oracle/cartpole_np.py::CartPoleOracle, bit for bit"""

    def __init__(self, case, state0, ts0, start, obs0):
        from oracle.cartpole_np import CartPoleOracle

        self.orc = CartPoleOracle(case.E, case.T, initial_state=start)
        self.orc.state = state0.copy()
        self.orc.obs = obs0.copy()
        self.orc.timestep = ts0.astype(np.int32).copy()

    def obs(self):
        return self.orc.obs.copy()

    def step(self, a):
        self.orc.step(a)
        return self.orc.done.copy(), self.orc.rewards.copy()

    def restart(self):
        self.orc.reset_done_envs()

    def final(self):
        return {"state": self.orc.state.copy(), "obs": self.orc.obs.copy(), "ts": self.orc.timestep.copy()}


def _ou_feed(E):
    from warp_drive_amd.utils.data_feed import DataFeed

    f = DataFeed()
    f.add_data(name="sampled_actions_ou_state", data=np.zeros((E, 1, 1), F32))
    return f


def _box_actions(case, sampler, words, means):
    """the actions of every tick of a Box case and the OU state after every launch: direct sample_ou_process launches
    with the tick's stream tag on copies of the RNG words and of the OU state"""
    import torch
    from warp_drive_amd.managers import hip_driver as drv

    E = case.E
    rng_copy = drv.mem_alloc(words.nbytes)
    drv.memcpy_htod(rng_copy, words)
    ou = torch.zeros(E, dtype=torch.float32, device="cuda")
    damping, stddev, scale = cc.OU_PARAMS
    acts, ou_after = [], []
    try:
        for k in range(case.launches * case.ticks):
            act = torch.zeros(E, dtype=torch.float32, device="cuda")
            sampler.sample_ou_process(rng_copy, means, act, ou, F32(damping), F32(stddev), F32(scale), np.int32(E),
                                      cc.TICK_TAG, block=(256, 1, 1), grid=(max(1, min(4096, (E + 255) // 256)), 1))
            torch.cuda.synchronize()
            acts.append(act.cpu().numpy())
            if (k + 1) % case.ticks == 0:
                ou_after.append(ou.cpu().numpy().copy())
    finally:
        rng_copy.free()
    return np.stack(acts), ou_after


def _expected(case, yard, acts):
    """the yardstick's trajectory, launch by launch"""
    out = []
    for launch in range(case.launches):
        rec = {k: [] for k in ("obs_rows", "actions", "rewards", "done")}
        finished = np.zeros(case.E, bool)
        for k in range(case.ticks):
            a = acts[launch * case.ticks + k]
            rec["obs_rows"].append(yard.obs())
            done, rew = yard.step(a)
            rec["actions"].append(a), rec["rewards"].append(rew), rec["done"].append(done)
            finished |= done > 0
            yard.restart()
        rec = {k: np.stack(v) for k, v in rec.items()}
        rec.update(yard.final())
        rec["finished"] = finished
        out.append(rec)
    return out


def _batch(case):
    import torch

    if case.rows is None:
        return None
    R, E, O = case.rows, case.E, cc.OBS_DIM[case.env]
    return {"obs": torch.full((R, E, 1, O), 7.0, device="cuda"),
            "actions": torch.full((R, E, 1, 1), -1, dtype=torch.float32 if case.cont else torch.int32, device="cuda"),
            "rewards": torch.full((R, E, 1), 7.0, device="cuda"),
            "done": torch.full((R, E), -1, dtype=torch.int32, device="cuda")}


def _refill(batch):
    if batch is not None:
        batch["obs"].fill_(7.0), batch["actions"].fill_(-1), batch["rewards"].fill_(7.0), batch["done"].fill_(-1)


def _check_batch(case, batch, rec, tag):
    if batch is None:
        return
    T = case.ticks
    b = {k: v.cpu().numpy() for k, v in batch.items()}
    EQ(b["obs"][:T, :, 0], rec["obs_rows"], f"{tag} obs rows")
    EQ(b["actions"][:T, :, 0, 0], rec["actions"].astype(b["actions"].dtype), f"{tag} action rows")
    EQ(b["rewards"][:T, :, 0], rec["rewards"], f"{tag} reward rows")
    EQ(b["done"][:T], rec["done"], f"{tag} done rows")
    # the surplus rows stay untouched
    assert (b["obs"][T:] == 7.0).all() and (b["actions"][T:] == -1).all(), tag
    assert (b["rewards"][T:] == 7.0).all() and (b["done"][T:] == -1).all(), tag


EXTRA, EXTRA_BASE, EXTRA_DIRTY = "restored_flag", 3.5, 9.0


def _start_arrays(w, case):
    """the arrays before the first launch: spread states and timesteps; the observation rows are the wrapper's own (the
    registered restart rows) -- Cartpole's observation IS its state (its kernels record and evaluate the state)"""
    from tests.hip_harness import OBS, pull

    state = case.start_states()
    obs = state.reshape(case.E, 1, -1).copy() if case.env == "cartpole" else pull(w, OBS).copy()
    return {"state": state, "ts": case.start_timesteps(), "obs": obs, "row": pull(w, "state")[0, 0].copy()}


def _tick_setup(case):
    """(wrapper under test, sampler, probabilities tensor, batch, launch, the start arrays)"""
    import torch
    from tests.hip_harness import OBS, pull
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.utils.data_feed import DataFeed

    w = _wrapper(case)
    E = case.E
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=cc.SAMPLER_SEED)
    if case.cont:
        w.cuda_data_manager.push_data_to_device(_ou_feed(E))
    if case.extra == "third":
        feed = DataFeed()
        feed.add_data(name=EXTRA, data=np.full((E,), EXTRA_BASE, F32), save_copy_and_apply_at_reset=True)
        w.cuda_data_manager.push_data_to_device(feed)
        assert len(w.cuda_data_manager.reset_data_list) == 3
    p = case.probabilities()
    probs = torch.from_numpy(p.reshape(E, 1, -1)).cuda()
    batch = _batch(case)
    w.env.ticks_per_launch = case.ticks
    launch = w.env.tick_launch(sampler, [probs], w.env_resetter, batch=batch)
    start = _start_arrays(w, case)
    return w, sampler, probs, batch, launch, start


def _tick_start(w, case, sampler, start):
    from oracle.core_np import seed_words
    from tests.hip_harness import ACT, OBS, REW

    E = case.E
    _put(w, "state", start["state"])
    _put(w, "_timestep_", start["ts"])
    _put(w, "_done_", np.zeros(E, np.int32))
    _put(w, OBS, start["obs"])
    _put(w, REW, np.full(E, -7.0, F32))
    _put(w, ACT, np.full(E, -1, _act_dtype(case.env)))
    sampler.init_random(seed=cc.SAMPLER_SEED)
    words = _words(sampler.rng_state, E)
    assert (int(words[0]), int(words[1])) == seed_words(cc.SAMPLER_SEED) and (words[4:] == 0).all()
    words[4:] = case.start_epochs()
    _put_words(sampler.rng_state, words)
    if case.pool:
        pw = _words(w.env_resetter._pool_rng, E)
        assert (int(pw[0]), int(pw[1])) == seed_words(cc.POOL_SEED)
        pw[4:] = case.start_pool_epochs()
        _put_words(w.env_resetter._pool_rng, pw)
    if case.cont:
        _put(w, "sampled_actions_ou_state", np.zeros(E, F32))
    return words


@pytest.mark.parametrize("case", cc.TICK_CASES, ids=repr)
def test_tick_cases_and_geometries(case):
    """HipClassicControl<X>EnvTick, every case under every geometry that takes its trips: after every launch the state,
    the observation, `_timestep_`, `_done_`, the reward, `sampled_actions`, the sampler's RNG words, the pool's RNG
    words and every batch row k against tick k of the yardstick, at tolerance 0"""
    from tests.hip_harness import ACT, OBS, REW, pull

    env, E = case.env, case.E
    w, sampler, probs, batch, launch, start = _tick_setup(case)
    fn, args, block, grid, shared = launch
    assert fn.name == cc.ENTRY[env] + "Tick" and shared == 0
    words0 = _tick_start(w, case, sampler, start)
    ou_after = None
    if case.cont:
        acts, ou_after = _box_actions(case, sampler, words0, probs.reshape(-1))
    else:
        acts = case.actions()
        assert acts.min() >= 0 and acts.max() == case.A - 1
        if case.has_one_draw():   # the draw of exactly 1.0 on a row whose sums stay below it: the clamp
            assert acts[case.one_draw_tick(), cc.ONE_DRAW[0]] == case.A - 1
    if env == "cartpole":
        yard = _CartpoleYardstick(case, start["state"], start["ts"], start["row"], start["obs"][:, 0])
    else:
        yard = _DeviceYardstick(case, start["state"], start["ts"])
        EQ(yard.obs0, start["obs"])   # (both wrappers hold the registered restart rows)
    expected = _expected(case, yard, acts)
    cov = cc.simulate(case)
    restarts = sum(int((r["done"] > 0).sum()) for r in expected)
    results = []
    for geom in cc.geometries(E):
        threads, blocks, trips = cc.geometry(E, geom, product=(block[0], grid[0]))
        assert threads <= cc.LAUNCH_BOUND and (geom == "product" or not isinstance(geom[1], int) or trips >= 3)
        _tick_start(w, case, sampler, start)
        out = {}
        for li, rec in enumerate(expected):
            tag = f"{case.name} {geom} launch {li}"
            _refill(batch)
            if case.extra:
                _put(w, EXTRA, np.full(E, EXTRA_DIRTY, F32))
            fn(*args, block=(threads, 1, 1), grid=(blocks, 1), shared=0)
            _sync()
            _check_batch(case, batch, rec, tag)
            out = {n: pull(w, n) for n in ("state", OBS, "_timestep_", "_done_", REW, ACT)}
            EQ(out["state"][:, 0], rec["state"], f"{tag} state")
            EQ(out[OBS][:, 0], rec["obs"], f"{tag} observation")
            EQ(out["_timestep_"], rec["ts"], f"{tag} timestep")
            EQ(out["_done_"], rec["done"][-1], f"{tag} done")          # the launch's last tick, still set
            EQ(out[REW][:, 0], rec["rewards"][-1], f"{tag} reward")
            EQ(out[ACT].reshape(-1), rec["actions"][-1].astype(out[ACT].dtype), f"{tag} sampled_actions")
            out["rng"] = _words(sampler.rng_state, E)
            EQ(out["rng"][:4], words0[:4], f"{tag} RNG header")
            EQ(out["rng"][4:], words0[4:] + np.uint32((li + 1) * case.ticks), f"{tag} RNG epochs")
            if case.pool:
                out["pool_rng"] = _words(w.env_resetter._pool_rng, E)
                EQ(out["pool_rng"], rec["pool_words"], f"{tag} pool RNG words")
            if case.cont:
                out["ou"] = pull(w, "sampled_actions_ou_state").reshape(-1)
                EQ(out["ou"], ou_after[li], f"{tag} OU state")
            if case.extra:   # restored for exactly the replicas that finished in this launch
                out["extra"] = pull(w, EXTRA)
                EQ(out["extra"], np.where(rec["finished"], EXTRA_BASE, EXTRA_DIRTY).astype(F32), f"{tag} third array")
        results.append(out)
        print(f"{case.name} [{fn.name}] geometry {geom}: {threads} threads x {blocks} blocks, {trips} trips; device "
              f"restarts {restarts}; host replay: {cov.line()}")
    for other in results[1:]:
        for key in results[0]:
            assert results[0][key].tobytes() == other[key].tobytes(), (case.name, key)
    assert restarts >= E


@pytest.mark.parametrize("env", sorted(cc.REFUSED_ACTION_COUNTS))
def test_action_counts_the_host_refuses(env):
    """the host admits 1 .. 8 actions for the classic-control ticks and rollouts: other counts are refused, not launched"""
    import torch
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    case = cc.TickCase("refused", env, E=63)
    w = _wrapper(case)
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=1)
    for A in cc.REFUSED_ACTION_COUNTS[env]:
        probs = torch.zeros((case.E, 1, A), device="cuda")
        with pytest.raises(AssertionError):
            w.env.tick_launch(sampler, [probs], w.env_resetter)
        assert not w.env.has_live_policy_rollout(32, A)
        with pytest.raises(UnsupportedRolloutShape):
            w.env.tick_launch(sampler, [probs], w.env_resetter, policy=(torch.zeros(8, device="cuda"), 32))
    for A in (1, 8):
        assert w.env.has_live_policy_rollout(32, A) and w.env.has_live_policy_rollout(64, A)


# -------------------------------------------------------------------------------------------------------- Rollout
def _rollout_setup(case):
    import torch
    from tests.hip_harness import OBS, pull
    from warp_drive_amd.managers.function_manager import HIPSampler

    w = _wrapper(case)
    E = case.E
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=cc.SAMPLER_SEED)
    _, packed_np = case.policy()
    packed = torch.from_numpy(packed_np).cuda()
    probs = torch.full((E, 1, case.A), 1.0 / case.A, device="cuda")   # (not read: the kernel evaluates the policy)
    batch = _batch(case)
    w.env.ticks_per_launch = case.ticks
    assert w.env.has_live_policy_rollout(case.hidden, case.A)
    launch = w.env.tick_launch(sampler, [probs], w.env_resetter, batch=batch, policy=(packed, case.hidden))
    start = _start_arrays(w, case)
    return w, sampler, packed, packed_np, probs, batch, launch, start


@pytest.mark.parametrize("case", cc.ROLLOUT_CASES, ids=repr)
def test_rollout_action_counts_and_geometries(case):
    """...EnvRollout_H32 / _H64 at 1, 2, 3, 8 actions under three geometries, launches of 11 ticks over 4-tick episodes that
    start in the middle of a Philox quad, a 7-row pool: the yardstick replays the device's recorded action (rows, final
    arrays, RNG and pool words at tolerance 0); the recorded action is the number of host running sums below the host's
    uniform except where the uniform lies within 2e-6 of a threshold -- that set is computed from the host's sums and
    uniforms alone and capped at (2 + draws // 50000) * (A - 1); with one action every action is 0."""
    from oracle.core_np import seed_words, single_head_tick_uniform
    from tests.classic_control_policy import count_below, running_sums
    from tests.hip_harness import ACT, OBS, REW, pull

    env, E = case.env, case.E
    w, sampler, packed, packed_np, probs, batch, launch, start = _rollout_setup(case)
    fn, args, block, grid, shared = launch
    O, H, A = cc.OBS_DIM[env], case.hidden, case.A
    n_w = O * H + H + H * H + H + A * H + A
    assert fn.name == cc.ENTRY[env] + f"Rollout_H{H}" and shared == 4 * n_w
    k0, k1 = seed_words(cc.SAMPLER_SEED)
    results, yard = [], None
    for geom in cc.ROLLOUT_GEOMETRIES:
        threads, blocks, trips = cc.geometry(E, geom)
        assert threads <= cc.LAUNCH_BOUND and (not isinstance(geom[1], int) or trips >= 3)
        words0 = _tick_start(w, case, sampler, start)
        if env == "cartpole":
            yard = _CartpoleYardstick(case, start["state"], start["ts"], start["row"], start["obs"][:, 0])
        elif yard is None:
            yard = _DeviceYardstick(case, start["state"], start["ts"])
        else:
            yard.rewind()
        near = differ = draws = restarts = 0
        counts = np.zeros(A, np.int64)
        out = {}
        for li in range(case.launches):
            tag = f"{case.name} {geom} launch {li}"
            _refill(batch)
            fn(*args, block=(threads, 1, 1), grid=(blocks, 1), shared=shared)   # (shared = 4 * n_w at every geometry)
            _sync()
            b = {k: v.cpu().numpy() for k, v in batch.items()}
            acts = b["actions"][:case.ticks, :, 0, 0]
            assert acts.min() >= 0 and acts.max() <= A - 1, tag
            ep0 = words0[4:] + np.uint32(li * case.ticks)
            for k in range(case.ticks):
                obs_k = yard.obs()
                cum = running_sums(cc.rollout_probabilities(case, packed_np, obs_k))
                u = single_head_tick_uniform(E, ep0 + np.uint32(k), k0, k1, cc.TICK_TAG)
                near_k = cc.near_threshold(cum, u)
                bad = acts[k] != count_below(cum, u)
                assert not (bad & ~near_k).any(), (tag, k, cum[bad & ~near_k], u[bad & ~near_k], acts[k][bad & ~near_k])
                near, differ, draws = near + int(near_k.sum()), differ + int(bad.sum()), draws + E
                counts += np.bincount(acts[k], minlength=A)
                EQ(b["obs"][k, :, 0], obs_k, f"{tag} obs row {k}")
                done_k, rew_k = yard.step(acts[k])   # the replay follows the device's action
                EQ(b["rewards"][k, :, 0], rew_k, f"{tag} reward row {k}")
                EQ(b["done"][k], done_k, f"{tag} done row {k}")
                restarts += int((done_k > 0).sum())
                yard.restart()
            out = {n: pull(w, n) for n in ("state", OBS, "_timestep_", "_done_", REW, ACT)}
            fin = yard.final()
            EQ(out["state"][:, 0], fin["state"], f"{tag} state")
            EQ(out[OBS][:, 0], fin["obs"], f"{tag} observation")
            EQ(out["_timestep_"], fin["ts"], f"{tag} timestep")
            EQ(out["_done_"], done_k, f"{tag} done")
            EQ(out[REW][:, 0], rew_k, f"{tag} reward")
            EQ(out[ACT].reshape(-1), acts[-1], f"{tag} sampled_actions")
            out["rng"] = _words(sampler.rng_state, E)
            EQ(out["rng"][:4], words0[:4], f"{tag} RNG header")
            EQ(out["rng"][4:], words0[4:] + np.uint32((li + 1) * case.ticks), f"{tag} RNG epochs")
            if case.pool:
                out["pool_rng"] = _words(w.env_resetter._pool_rng, E)
                EQ(out["pool_rng"], fin["pool_words"], f"{tag} pool RNG words")
            out.update({f"batch_{k}": v for k, v in b.items()})
        results.append(out)
        shares = np.round(counts / draws, 3).tolist()
        print(f"{case.name} [{fn.name}] geometry {geom}: {threads} threads x {blocks} blocks, {trips} trips; {restarts} "
              f"restarts, action shares {shares}, {near} of {draws} draws within {cc.NEAR_WINDOW} of a threshold "
              f"(cap {case.near_cap()}), {differ} of them decided otherwise by the device")
        assert near <= case.near_cap() and restarts >= E
        assert A > 1 or (counts[0] == draws and near == 0)
    for other in results[1:]:
        for key in results[0]:
            assert results[0][key].tobytes() == other[key].tobytes(), (case.name, key)


@pytest.mark.parametrize("env", cc.DISCRETE)
def test_rollout_entry_refuses_another_width_and_nine_actions(env):
    """The H32 entry launched with hidden = 64, and a launch with n_actions = 9 (both beyond what the host builds: the
    kernel's own guard).  Every argument is a valid pointer, the weights and the dynamic LDS have the H64 / nine-action
    size, every array is pre-filled: afterwards every byte of every array, of the batch tensors and of both RNG word
    blocks is unchanged."""
    import torch
    from tests.hip_harness import ACT, OBS, REW, pull

    GUARD_ARRAYS = ("state", ACT, "_done_", REW, OBS, "_timestep_")
    case = cc.RolloutCase(env, 32, 3)
    w, sampler, packed, packed_np, probs, batch, launch, start = _rollout_setup(case)
    fn, args, block, grid, shared = launch
    assert fn.name == cc.ENTRY[env] + "Rollout_H32"
    E, O = case.E, cc.OBS_DIM[env]
    n_w = lambda H, A: O * H + H + H * H + H + A * H + A
    i_probs = next(i for i, a in enumerate(args) if a is probs)
    i_packed = next(i for i, a in enumerate(args) if a is packed)
    assert int(args[i_probs + 1]) == 3 and int(args[i_packed + 1]) == 32
    big = torch.full((max(n_w(64, 9), n_w(32, 9)),), 0.01, device="cuda")
    probs9 = torch.full((E, 1, 9), 1.0 / 9, device="cuda")
    wide = list(args)
    wide[i_packed], wide[i_packed + 1] = big, np.int32(64)
    nine = list(args)
    nine[i_probs], nine[i_probs + 1], nine[i_packed] = probs9, np.int32(9), big
    for name, a, lds in (("hidden = 64", wide, 4 * n_w(64, 3)), ("n_actions = 9", nine, 4 * n_w(32, 9))):
        _tick_start(w, case, sampler, start)
        _refill(batch)
        before = {n: pull(w, n).tobytes() for n in GUARD_ARRAYS}
        before.update({f"batch_{k}": v.cpu().numpy().tobytes() for k, v in batch.items()})
        before["rng"] = _words(sampler.rng_state, E).tobytes()
        if case.pool:
            before["pool_rng"] = _words(w.env_resetter._pool_rng, E).tobytes()
        fn(*a, block=block, grid=grid, shared=lds)
        _sync()
        after = {n: pull(w, n).tobytes() for n in GUARD_ARRAYS}
        after.update({f"batch_{k}": v.cpu().numpy().tobytes() for k, v in batch.items()})
        after["rng"] = _words(sampler.rng_state, E).tobytes()
        if case.pool:
            after["pool_rng"] = _words(w.env_resetter._pool_rng, E).tobytes()
        for key in before:
            assert before[key] == after[key], (env, name, key)
        print(f"{fn.name} with {name}: {len(before)} arrays unchanged")
