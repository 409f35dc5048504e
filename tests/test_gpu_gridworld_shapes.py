"""TagGridWorld's five device entries off the 5-agent shape: HipTagGridWorldStep / Tick / Rollout
(csrc/kernels/tag_gridworld.hip) and HipTagGridWorldRollout_N5 / _N5_H32 / _N5_H64 (tag_gridworld_n5.hip) at other
agent counts, grids, episode lengths, reward scalars and -- launched directly with the arguments `step_launch()` /
`tick_launch()` build -- at other blocks and grids than the host picks: the reference geometry, blocks that are no
multiple of N, grids of 1 and 3 blocks (several trips of the grid-stride loop), with and without the LDS restore
cache.  Everything is replayed through oracle/tag_gridworld_np.py with the kernels' own draws and compared at
tolerance 0.  The cases and their expected trajectories live in tests/gridworld_cases.py; the host file
tests/test_gridworld_shapes_logic.py asserts, from the oracle alone, that every case reaches tags, time-outs, restarts
and all eight reward sums.  `pytest -s` prints what every case ran."""
import numpy as np
import pytest

from tests import gridworld_cases as gc

pytestmark = pytest.mark.gpu

IMAGE_MAX_BYTES = 60000
EQ = np.testing.assert_array_equal


# ------------------------------------------------------------------------------------------------------- plumbing
def _wrapper(case, cls=None):
    from tests.hip_harness import make_wrapper, require_gpu
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorld

    require_gpu()
    return make_wrapper((cls or CUDATagGridWorld)(seed=27, **case.config()), case.E)


def _words(ptr, n):
    import torch
    from warp_drive_amd.managers import hip_driver as drv

    out = np.zeros(4 + n, dtype=np.uint32)
    drv.memcpy_dtoh(out, ptr)
    torch.cuda.synchronize()
    return out


def _start(w, case, sampler, obs0):
    """bring the wrapper to the case's initial state (a case runs once per geometry on one wrapper) and check it"""
    import torch
    from oracle.core_np import seed_words
    from tests.hip_harness import OBS, pull
    from warp_drive_amd.managers import hip_driver as drv

    w.reset_all_envs()
    t0 = case.start_timesteps()
    if t0 is not None:
        drv.memcpy_htod(w.cuda_data_manager.device_data("_timestep_"), np.ascontiguousarray(t0))
        torch.cuda.synchronize()
    orc = gc.make_oracle(case)
    EQ(pull(w, "loc_x"), orc.loc_x)
    EQ(pull(w, "loc_y"), orc.loc_y)
    EQ(pull(w, "_timestep_"), orc.timestep)
    EQ(pull(w, "_done_"), 0)
    EQ(pull(w, OBS), obs0)
    if sampler is not None:
        sampler.init_random(seed=gc.SAMPLER_SEED)
        words = _words(sampler.rng_state, case.E * case.N)
        assert (int(words[0]), int(words[1])) == seed_words(gc.SAMPLER_SEED) and (words[4:] == 0).all()
        words[4:] = case.start_epochs()   # (row-dependent epochs: see gridworld_cases.Case.start_epochs)
        drv.memcpy_htod(sampler.rng_state, words)
        torch.cuda.synchronize()


def _cache_dwords(w):
    dm = w.cuda_data_manager
    return sum(int(np.prod(dm.get_shape(k)[1:])) for k in dm.reset_data_list)


def _regeometry(w, case, launch, geom, rollout=False):
    """the launch `step_launch()` / `tick_launch()` built, with another block and grid.  geom: "product", or
    (threads, blocks or None for one trip, optional "nocache").  The kernels derive replicas-per-block from blockDim.x;
    dynamic LDS by the host rule lds_bytes(epb) (+ the restore cache; `reset_cache_dwords` is the rollout's last
    argument).  A rollout geometry without the LDS image is refused here, on the host, and never launched."""
    fn, args, block, grid, shared = launch
    env, N, E = w.env, case.N, case.E
    if geom == "product":
        epb = max(1, block[0] // N)
        cd = int(args[-1]) if rollout else 0
        return fn, args, block, grid, shared, dict(threads=block[0], blocks=grid[0], epb=epb, cache=cd,
                                                   trips=-(-(-(-E // epb)) // grid[0]), image=env.image_fits(epb))
    threads, blocks = geom[0], geom[1]
    assert N <= threads <= 1024
    epb = max(1, threads // N)
    lds = env.lds_bytes(epb)
    args = list(args)
    cd = 0
    if rollout:
        assert fn.name == "HipTagGridWorldRollout" and env.image_fits(epb), (case, geom)
        cd = _cache_dwords(w)
        if "nocache" in geom or lds + 4 * epb * cd > IMAGE_MAX_BYTES:
            cd = 0
        lds += 4 * epb * cd
        args[-1] = np.int32(cd)
    groups = -(-E // epb)
    blocks = groups if blocks is None else blocks
    assert 1 <= blocks <= groups and lds <= 65536
    return fn, args, (threads, 1, 1), (blocks, 1), lds, dict(threads=threads, blocks=blocks, epb=epb, cache=cd,
                                                             trips=-(-groups // blocks), image=env.image_fits(epb))


def _geometries(case, env, kind):
    """the product's geometry; the reference geometry block = (N, 1, 1), grid = (E, 1) (Step); blocks of 64 / 128 /
    256 / 512 threads (no multiple of N wherever N does not divide them: idle tail lanes) with one trip, grids of 3
    and of 1 block (>= 3 trips, asserted), for the rollout only sizes whose image fits by the host rule, plus the same
    block without the restore cache where it has one"""
    N, E = case.N, case.E
    out = ["product"]
    if kind == "step":
        out.append((N, E))
    sizes = [b for b in (64, 128, 256, 512) if b >= N]
    if kind == "rollout":
        sizes = [b for b in sizes if env.image_fits(max(1, b // N))]
    for b, g in zip(sizes, (3, None, 1, 3)):
        out.append((b, g))
    if len(sizes) == 1:
        out.append((sizes[0], 1))
    if kind == "rollout":
        cd = 2 * N + N * case.F
        with_cache = [b for b in sizes if env.lds_bytes(b // N) + 4 * (b // N) * cd <= IMAGE_MAX_BYTES]
        if with_cache:
            out.append((with_cache[-1], None, "nocache"))
    return out


def _report(case, kind, geom, info, cov, fn):
    print(f"{case.name} [{kind} {fn.name}] geometry {geom}: {info['threads']} threads x {info['blocks']} blocks, "
          f"{info['epb']} replicas per block, {info['trips']} trips, LDS image {'yes' if info['image'] else 'no'}, "
          f"restore cache {info['cache']} dwords; {cov.line()}")


def _same(results, tag):
    """every geometry of a case left the same bytes"""
    first = results[0]
    for other in results[1:]:
        assert first.keys() == other.keys()
        for key in first:
            assert first[key].tobytes() == other[key].tobytes(), (tag, key)


# ---------------------------------------------------------------------------------------------------------- Step
@pytest.mark.parametrize("case", gc.STEP_CASES, ids=repr)
def test_step_shapes_and_geometries(case):
    """HipTagGridWorldStep with pushed random actions, every tick against the oracle (positions, done, timestep,
    observations, rewards), then the reset of finished replicas; same bytes under every geometry"""
    from tests.hip_harness import OBS, REW, pull, push_actions

    obs0, ticks, cov = gc.simulate(case, sampled=False, keep_obs_step=True)
    w = _wrapper(case)
    results = []
    for geom in _geometries(case, w.env, "step"):
        _start(w, case, None, obs0)
        fn, args, block, grid, shared, info = _regeometry(w, case, w.env.step_launch(), geom)
        assert fn.name == "HipTagGridWorldStep"
        if geom != "product" and geom[1] in (1, 3):
            assert info["trips"] >= 3, (case, geom, info)
        out = {}
        for k, rec in enumerate(ticks):
            push_actions(w, rec["actions"])
            w.cuda_data_manager.data_on_device_via_torch(REW).fill_(-1.0)
            fn(*args, block=block, grid=grid, shared=shared)
            tag = f"{case.name} {geom} tick {k}"
            got = {n: pull(w, n) for n in ("loc_x", "loc_y", "_done_", "_timestep_", OBS, REW)}
            EQ(got["loc_x"], rec["step_x"], err_msg=tag)
            EQ(got["loc_y"], rec["step_y"], err_msg=tag)
            EQ(got["_done_"], rec["done"], err_msg=tag)
            EQ(got["_timestep_"], rec["step_t"], err_msg=tag)
            EQ(got[OBS], rec["obs_step"], err_msg=tag)
            EQ(got[REW], rec["rewards"], err_msg=tag)
            w.reset_only_done_envs()
            if k % 8 == 7 or k == len(ticks) - 1:
                EQ(pull(w, "loc_x"), rec["loc_x"], err_msg=tag)
                EQ(pull(w, "_timestep_"), rec["timestep"], err_msg=tag)
                EQ(pull(w, OBS), rec["obs"], err_msg=tag)
            if k == len(ticks) - 1:
                out = got
        results.append(out)
        _report(case, "step", geom, info, cov, fn)
    _same(results, case.name)


# ---------------------------------------------------------------------------------------------------------- Tick
@pytest.mark.parametrize("case", gc.TICK_CASES, ids=repr)
def test_tick_shapes_and_geometries(case):
    """HipTagGridWorldTick: the sampled actions draw for draw, then the step and the in-kernel restore of finished
    replicas (`_done_` still set), the RNG words after every launch; same bytes under every geometry"""
    import torch
    from tests.hip_harness import ACT, OBS, REW, pull
    from warp_drive_amd.managers.function_manager import HIPSampler

    obs0, ticks, cov = gc.simulate(case)
    cov.check(case.E)
    w = _wrapper(case)
    E, N = case.E, case.N
    sampler = HIPSampler(w.cuda_function_manager)
    probs = torch.from_numpy(case.probabilities()).cuda()
    results = []
    for geom in _geometries(case, w.env, "tick"):
        _start(w, case, sampler, obs0)
        launch = w.env.tick_launch(sampler, [probs], w.env_resetter)
        fn, args, block, grid, shared, info = _regeometry(w, case, launch, geom)
        assert fn.name == "HipTagGridWorldTick"
        if geom != "product" and geom[1] in (1, 3):
            assert info["trips"] >= 3, (case, geom, info)
        out = {}
        for k, rec in enumerate(ticks):
            w.cuda_data_manager.data_on_device_via_torch(REW).fill_(-1.0)
            w.cuda_data_manager.data_on_device_via_torch(ACT).fill_(-1)
            fn(*args, block=block, grid=grid, shared=shared)
            tag = f"{case.name} {geom} tick {k}"
            got = {n: pull(w, n) for n in (ACT, "_done_", REW, "loc_x", "loc_y", "_timestep_", OBS)}
            EQ(got[ACT][..., 0], rec["actions"], err_msg=tag)
            EQ(got["_done_"], rec["done"], err_msg=tag)        # still set
            EQ(got[REW], rec["rewards"], err_msg=tag)
            EQ(got["loc_x"], rec["loc_x"], err_msg=tag)        # finished replicas are back at their start
            EQ(got["loc_y"], rec["loc_y"], err_msg=tag)
            EQ(got["_timestep_"], rec["timestep"], err_msg=tag)
            EQ(got[OBS], rec["obs"], err_msg=tag)
            if k == len(ticks) - 1:
                got["rng"] = _words(sampler.rng_state, E * N)
                assert (got["rng"][4:] == case.start_epochs() + np.uint32(len(ticks))).all()
                out = got
        results.append(out)
        _report(case, "tick", geom, info, cov, fn)
    _same(results, case.name)


# ------------------------------------------------------------------------------------------------------- Rollout
def _batch(T, E, N, F):
    import torch

    return {"obs": torch.full((T, E, N, F), 7.0, device="cuda"),
            "actions": torch.full((T, E, N, 1), -1, dtype=torch.int32, device="cuda"),
            "rewards": torch.full((T, E, N), -1.0, device="cuda"),
            "done": torch.full((T, E), -1, dtype=torch.int32, device="cuda")}


def _refill(batch):
    batch["obs"].fill_(7.0)
    batch["actions"].fill_(-1)
    batch["rewards"].fill_(-1.0)
    batch["done"].fill_(-1)


def _record_paths(E, NF, epb, T):
    """(record copies through 16-byte vectors, through 4-byte stores) over the trips and ticks of one launch, by the
    kernel's rule: the block's slice of row k starts on a 16-byte boundary and is a whole number of vectors"""
    vec = scalar = 0
    for env0 in range(0, E, epb):
        n_out = min(epb, E - env0) * NF
        for k in range(T):
            aligned = ((k * E + env0) * NF) % 4 == 0 and n_out % 4 == 0
            vec, scalar = vec + aligned, scalar + (not aligned)
    return vec, scalar


def _run_rollout(w, case, sampler, launch, geom, T, obs0, ticks, tag):
    """`len(ticks) // T` launches of T ticks; returns what the last launch left (batch rows, per-tick arrays, words)"""
    import torch
    from tests.hip_harness import ACT, OBS, REW, pull

    fn, args, block, grid, shared, batch = launch
    E, N = case.E, case.N
    out = {}
    for l in range(len(ticks) // T):
        _refill(batch)
        fn(*args, block=block, grid=grid, shared=shared)
        torch.cuda.synchronize()
        b = {k: v.cpu().numpy() for k, v in batch.items()}
        for k in range(T):
            rec = ticks[l * T + k]
            where = f"{tag} launch {l} row {k}"
            EQ(b["obs"][k], obs0 if l * T + k == 0 else ticks[l * T + k - 1]["obs"], err_msg="obs " + where)
            EQ(b["actions"][k, :, :, 0], rec["actions"], err_msg="actions " + where)
            EQ(b["rewards"][k], rec["rewards"], err_msg="rewards " + where)
            EQ(b["done"][k], rec["done"], err_msg="done " + where)
        last = ticks[l * T + T - 1]
        got = {n: pull(w, n) for n in ("loc_x", "loc_y", "_timestep_", "_done_", OBS, REW, ACT)}
        EQ(got["loc_x"], last["loc_x"], err_msg=where)
        EQ(got["loc_y"], last["loc_y"], err_msg=where)
        EQ(got["_timestep_"], last["timestep"], err_msg=where)
        EQ(got["_done_"], last["done"], err_msg=where)
        EQ(got[OBS], last["obs"], err_msg=where)
        EQ(got[REW], last["rewards"], err_msg=where)
        EQ(got[ACT][..., 0], last["actions"], err_msg=where)
        got["rng"] = _words(sampler.rng_state, E * N)
        assert (got["rng"][4:] == case.start_epochs() + np.uint32((l + 1) * T)).all(), where
        out = dict(got, **{"batch_" + k: v for k, v in b.items()})
    return out


def _rollout_case(case, T, geoms_of, check=True, kernel="HipTagGridWorldRollout", cov_check=None):
    import torch
    from warp_drive_amd.managers.function_manager import HIPSampler

    obs0, ticks, cov = gc.simulate(case)
    if check:
        cov.check(case.E)
    if cov_check is not None:
        cov_check(cov)
    assert len(ticks) % T == 0
    w = _wrapper(case)
    w.env.ticks_per_launch = T
    sampler = HIPSampler(w.cuda_function_manager)
    probs = torch.from_numpy(case.probabilities()).cuda()
    batch = _batch(T, case.E, case.N, case.F)
    results, infos = [], []
    for geom in geoms_of(w.env):
        if geom == "general":   # (an instance attribute: the class keeps its rule for the other geometries)
            w.env.SPECIALISED_ROLLOUT = False
        elif "SPECIALISED_ROLLOUT" in vars(w.env):
            del w.env.SPECIALISED_ROLLOUT
        _start(w, case, sampler, obs0)
        launch = w.env.tick_launch(sampler, [probs], w.env_resetter, batch=batch)
        if launch[0].name.endswith("_N5"):   # the specialised kernel: its own LDS formula, blocks of one wavefront
            fn, args, block, grid, shared = launch
            groups = -(-case.E // 12)
            blocks = groups if geom == "product" else geom[1]
            assert block == (64, 1, 1) and 1 <= blocks <= groups
            grid, info = (blocks, 1), dict(threads=64, blocks=blocks, epb=12, cache=int(args[-2]),
                                           trips=-(-groups // blocks), image=True)
        else:
            fn, args, block, grid, shared, info = _regeometry(w, case, launch, "product" if geom == "general" else geom,
                                                              rollout=True)
        assert fn.name == (kernel if geom != "general" else "HipTagGridWorldRollout"), (fn.name, geom)
        assert info["image"]
        if geom not in ("product", "general") and geom[1] in (1, 3):
            assert info["trips"] >= 3, (case, geom, info)
        info["paths"] = _record_paths(case.E, case.N * case.F, info["epb"], T)
        results.append(_run_rollout(w, case, sampler, (fn, args, block, grid, shared, batch), geom, T, obs0, ticks,
                                    f"{case.name} {geom}"))
        infos.append(info)
        _report(case, "rollout", geom, info, cov, fn)
        print(f"    record copies of one launch: {info['paths'][0]} through 16-byte vectors, {info['paths'][1]} through 4-byte stores")
    _same(results, case.name)
    return infos, cov


@pytest.mark.parametrize("case", gc.ROLLOUT_CASES, ids=repr)
def test_rollout_shapes_and_geometries(case):
    """HipTagGridWorldRollout off N = 5: every row of the four batch tensors of every launch, the per-tick arrays and
    the RNG words after it; with and without the restore cache; same bytes under every geometry"""
    infos, cov = _rollout_case(case, gc.ROLLOUT_TICKS_PER_LAUNCH[case.name], lambda env: _geometries(case, env, "rollout"))
    if case.name == "rollout_N13_L10_full_nocache":
        # (N F = 689 is odd: both record paths; 256-thread blocks hold the image and have no room for the cache)
        assert any(i["threads"] == 256 and i["cache"] == 0 for i in infos) and any(i["cache"] > 0 for i in infos)
        assert infos[0]["paths"][0] > 0 and infos[0]["paths"][1] > 0 and any(i["paths"][0] == 0 for i in infos)
    if case.starts == "corners":
        assert cov.consecutive > case.E   # replicas that finish on consecutive ticks (the runner starts next to a tagger)
    assert any(i["cache"] == 0 for i in infos) and any(i["trips"] >= 3 for i in infos)


def test_rollout_falls_back_to_a_block_size_with_an_image():
    """15 agents with full observations at 8 800 replicas: `_geometry()` picks 256-thread blocks (17 replicas: no LDS
    image), the rollout launch must come with 64-thread blocks (4 replicas, image and restore cache) -- and compute
    the oracle's rows"""
    case = gc.Case("rollout_N15_L10_full_E8800", 15, 10, 23, True, 8800, 6, reward="thirds", seed=28)
    envs = []
    infos, cov = _rollout_case(case, 3, lambda env: envs.append(env) or ["product"], check=False)
    assert envs[0]._geometry()[1][0] == 256 and not envs[0].image_fits(envs[0]._geometry()[0])
    assert infos[0]["threads"] == 64 and infos[0]["epb"] == 4 and infos[0]["cache"] == 2 * 15 + 15 * 61
    assert cov.tags > 0 and cov.seen.all(), cov.line()


def _stay_case(name, N, T, E, full=True, L=7):
    """one-hot "stay" everywhere from the default start (taggers in the centre, the runner in the corner): nobody is
    ever tagged and EVERY replica finishes on tick T of its episode"""
    case = gc.Case(name, N, L, T, full, E, 2 * T, reward="thirds", starts="default", seed=40)
    stay = np.zeros((E, N, 5), np.float32)
    stay[..., 0] = 1.0
    case.probabilities = lambda: stay
    return case


@pytest.mark.parametrize("N,T,full", [(6, 7, True), (6, 8, True), (9, 5, False), (5, 7, True), (5, 8, True)])
def test_rollout_every_replica_finishes_on_the_last_tick_of_a_launch(N, T, full):
    """ticks per launch == episode_length from a fresh reset, nobody tagged: all replicas time out on the LAST tick of
    the launch (odd and even tick counts: both parities of the block's vote flag), on grids of several trips -- the
    next trip's tick 0 must restore nothing, and the next launch starts from the restored rows.  General kernel with
    and without the restore cache, and the specialised kernel (N = 5)."""
    E = 203
    case = _stay_case(f"stay_N{N}_T{T}", N, T, E, full)

    def exact(cov):
        assert (cov.tags, cov.timeouts, cov.restarts, cov.consecutive) == (0, 2 * E, 2 * E, 0), cov.line()

    n5 = N == 5
    geoms = (lambda env: ["product", (64, 3), (64, 1), "general"]) if n5 else \
        (lambda env: ["product", (64, 3), (64, 1), (128, 1, "nocache"), (128, 3)])
    infos, _ = _rollout_case(case, T, geoms, check=False, cov_check=exact,
                             kernel="HipTagGridWorldRollout_N5" if n5 else "HipTagGridWorldRollout")
    assert sum(i["trips"] >= 3 for i in infos) >= 2


N5_CASE = gc.Case("n5_L10", 5, 10, 23, True, 12 * 30 + 7, 48, reward="small_cost", seed=41)
N5_EDGE = gc.Case("n5_L63_T4095_corners", 5, 63, 4095, True, 12 * 9 + 5, 16, reward="big", starts="corners", push_t=4090,
                  seed=42)
GENERAL_EDGE_L = gc.Case("general_L64_T4095_corners", 5, 64, 4095, True, 12 * 9 + 5, 16, reward="big", starts="corners",
                         push_t=4090, seed=42)
GENERAL_EDGE_T = gc.Case("general_L63_T4096_corners", 5, 63, 4096, True, 12 * 9 + 5, 16, reward="big", starts="corners",
                         push_t=4091, seed=42)


def test_n5_rollout_on_other_grids_equals_the_general_kernel():
    """HipTagGridWorldRollout_N5 on grids of 1, 7, 8, 9 and 13 blocks (remainders of the XCD remap != 0, several trips,
    E no multiple of 12) and the general kernel on the same seed: the oracle's bytes, all of them"""
    infos, _ = _rollout_case(N5_CASE, 12, lambda env: ["product", (64, 1), (64, 7), (64, 8), (64, 9), (64, 13), "general"],
                             kernel="HipTagGridWorldRollout_N5")
    assert [i["blocks"] for i in infos[:6]] == [31, 1, 7, 8, 9, 13] and infos[1]["trips"] == 31


def _crafted_counts(case):
    def check(cov):
        late = int((np.arange(case.E) % 4 >= 2).sum())
        # classes 0 and 1 are tagged on every tick; classes 2 and 3 run from push_t into the time-out once
        assert cov.tags == (case.E - late) * case.ticks and cov.timeouts == late and cov.seen.all(), cov.line()
        assert case.T - case.push_t <= case.ticks
    return check


def test_n5_rollout_at_the_limits_it_is_admitted_for():
    """grid_length 63 (agents on cells 62 / 63: the last entries of the quotient table and the widest packed cell) and
    episode_length 4095 with `_timestep_` pushed to 4090 (the last entry of the time table, and the time-out)"""
    infos, _ = _rollout_case(N5_EDGE, 8, lambda env: ["product", (64, 3)], check=False, cov_check=_crafted_counts(N5_EDGE),
                             kernel="HipTagGridWorldRollout_N5")
    assert infos[1]["trips"] >= 3


@pytest.mark.parametrize("case", [GENERAL_EDGE_L, GENERAL_EDGE_T], ids=repr)
def test_general_rollout_takes_the_shapes_past_the_n5_limits(case):
    """grid_length 64 and episode_length 4096 with the same crafted states: the general kernel (by name)"""
    _rollout_case(case, 8, lambda env: ["product", (64, 3)], check=False, cov_check=_crafted_counts(case))


# ------------------------------------------------------------------------------------------- live-policy entries
@pytest.mark.parametrize("hidden,E,T,blocks", [(32, 257, 23, 7), (64, 100, 23, 3), (64, 60, 4095, None)])
def test_live_policy_rollout_on_other_grids_and_above_64_kib(hidden, E, T, blocks):
    """HipTagGridWorldRollout_N5_H32 / _H64 on grids of several trips, by the method of
    test_gridworld_rollout_with_the_policies_inside_the_kernel (actions: the inverse-CDF draw on the float32
    restatement of the in-kernel forward, except where the uniform sits within 2e-6 of a threshold; at most
    2 + draws // 50000 such draws; the rest exact).  episode_length 4095 at H = 64 asks for 75 904 bytes of dynamic
    LDS: the host rule (ROLLOUT_POLICY_MAX_LDS) is asserted first, and the launch is sent once only if it admits it."""
    import torch
    from oracle.core_np import seed_words, single_head_tick_uniform
    from oracle.tag_gridworld_np import TagGridWorldOracle, policy_probabilities, running_sums
    from tests.hip_harness import OBS, make_wrapper, pull, require_gpu
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorld
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.models import FullyConnected
    from warp_drive_amd.training.policy_kernel import pack_gridworld_policy

    require_gpu()
    ticks, N, F = 20, 5, 21
    cfg = dict(num_taggers=4, grid_length=10, episode_length=T, wall_hit_penalty=0.1, tag_reward_for_tagger=10.0,
               tag_penalty_for_runner=2.0, step_cost_for_tagger=0.01, use_full_observation=True)
    w = make_wrapper(CUDATagGridWorld(seed=27, **cfg), E)
    env = w.env
    env.ticks_per_launch = ticks
    need = env.live_policy_lds_bytes(hidden)
    admitted = env.has_live_policy_rollout(hidden, 5)
    assert admitted == (need <= env.ROLLOUT_POLICY_MAX_LDS)
    print(f"H{hidden} episode_length {T}: {need} bytes of dynamic LDS, limit {env.ROLLOUT_POLICY_MAX_LDS}, admitted {admitted}")
    if T == 4095:
        assert need == 75904 > 65536
    if not admitted:
        return   # (asserted on the host; nothing is sent)
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=gc.SAMPLER_SEED)
    torch.manual_seed(hidden)
    models = [FullyConnected(F, [5], [hidden, hidden]).cuda() for _ in range(2)]
    with torch.no_grad():
        for m, scale in zip(models, (4.0, 7.0)):
            m.policy_head[0].weight.mul_(scale)
            m.fc["0"][0].weight.mul_(2.0)
    packed = [pack_gridworld_policy(m) for m in models]
    packed_host = [p.cpu().numpy() for p in packed]
    probs = torch.full((E, N, 5), 0.2, device="cuda")
    batch = _batch(ticks, E, N, F)
    fn, args, block, grid, shared = env.tick_launch(sampler, [probs], w.env_resetter, batch=batch, policy=(packed, hidden))
    assert fn.name == f"HipTagGridWorldRollout_N5_H{hidden}" and shared == need and block == (64, 1, 1)
    groups = -(-E // 12)
    grid = (groups if blocks is None else blocks, 1)
    assert blocks is None or groups >= 3 * blocks
    orc = TagGridWorldOracle(num_envs=E, **cfg)
    lo, hi = seed_words(gc.SAMPLER_SEED)
    near = draws = finished = 0
    for launch in range(4):
        words = _words(sampler.rng_state, E * N)
        assert (int(words[0]), int(words[1])) == (lo, hi) and (words[4:] == launch * ticks).all()
        _refill(batch)
        fn(*args, block=block, grid=grid, shared=shared)
        torch.cuda.synchronize()
        b = {k: v.cpu().numpy() for k, v in batch.items()}
        for k in range(ticks):
            obs = orc.obs.astype(np.float32)
            EQ(b["obs"][k], obs, err_msg=f"obs row {k} of launch {launch}")
            p = np.empty((E, N, 5), np.float32)
            p[:, :4] = policy_probabilities(packed_host[0], hidden, obs[:, :4].reshape(-1, F)).reshape(E, 4, 5)
            p[:, 4] = policy_probabilities(packed_host[1], hidden, obs[:, 4])
            cum = running_sums(p.reshape(-1, 5)).reshape(E, N, 5)
            u = single_head_tick_uniform(E * N, words[4:] + np.uint32(k), lo, hi, gc.TICK_TAG).reshape(E, N)
            want = np.minimum((cum < u[..., None]).sum(axis=-1), 4).astype(np.int32)
            got = b["actions"][k, :, :, 0]
            bad = got != want
            if bad.any():  # only where the uniform sits on a threshold
                gap = np.abs(cum[bad] - u[bad][:, None]).min(axis=1)
                assert (gap < 2e-6).all(), (launch, k, gap.max(), np.argwhere(bad)[:5])
            near += int(bad.sum())
            draws += E * N
            orc.step(got)
            EQ(b["rewards"][k], orc.rewards.astype(np.float32), err_msg=f"rewards row {k}")
            EQ(b["done"][k], orc.done, err_msg=f"done row {k}")
            finished += int((orc.done > 0).sum())
            orc.reset_done_envs()
        EQ(pull(w, "loc_x"), orc.loc_x)
        EQ(pull(w, "loc_y"), orc.loc_y)
        EQ(pull(w, "_timestep_"), orc.timestep)
        EQ(pull(w, OBS), orc.obs.astype(np.float32))
    hist = np.bincount(b["actions"].ravel(), minlength=5) / b["actions"].size
    print(f"H{hidden} E={E} grid {grid[0]} of {groups} groups: {finished} finished, {near} draws on a threshold of {draws}")
    assert finished >= (E if T < 100 else 1) and near <= 2 + draws // 50000 and hist.max() < 0.95, (finished, near, hist)


# ---------------------------------------------------------------------------------------------------- reset pool
@pytest.mark.parametrize("N", [5, 8])
def test_reset_pool_env_restarts_from_the_row_the_device_drew(N):
    """CUDATagGridWorldWithResetPool through step_all_envs / reset_only_done_envs and through a RolloutEngine (not
    fused): every restart is the pool row `pool_pick` names from the device's own words (the same row for x and y),
    the epoch words advance by exactly the done replicas, the ticks in between are the oracle's"""
    import torch
    from oracle.core_np import pool_pick
    from tests.hip_harness import ACT, OBS, REW, pull, push_actions
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorldWithResetPool
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.rollout import RolloutEngine

    E, T, n_ticks = 300, 6, 30
    case = gc.Case(f"pool_N{N}", N, 7, T, N == 5, E, n_ticks, reward="negative", starts="default", seed=50 + N)
    w = _wrapper(case, CUDATagGridWorldWithResetPool)
    w.init_reset_pool(seed=17)
    pool_x, pool_y = pull(w, "loc_x_reset_pool"), pull(w, "loc_y_reset_pool")
    assert pool_x.shape == (5, N) and (pool_x[:, -1] == 0).all() and len({r.tobytes() for r in pool_x}) > 1
    orc = gc.make_oracle(case)
    rng = np.random.RandomState(7)
    envs = np.arange(E)
    restarts = 0

    def restart(words_before):
        nonlocal restarts
        fin = orc.done > 0
        pick = pool_pick(envs, words_before[4:], words_before[0], words_before[1], pool_x.shape[0])
        orc.reset_done_envs(x=pool_x[pick], y=pool_y[pick])
        EQ(pull(w, "loc_x"), orc.loc_x)
        EQ(pull(w, "loc_y"), orc.loc_y)
        EQ(pull(w, "_timestep_"), orc.timestep)
        EQ(pull(w, "_done_"), 0)
        EQ(pull(w, OBS), orc.obs.astype(np.float32))
        after = _words(w.env_resetter._pool_rng, E)
        EQ(after[4:] - words_before[4:], fin.astype(np.uint32))
        restarts += int(fin.sum())
        return len(set(pick[fin].tolist()))

    rows_used = set()
    for t in range(n_ticks):
        a = rng.randint(0, 5, size=(E, N)).astype(np.int32)
        push_actions(w, a)
        w.step_all_envs()
        orc.step(a)
        EQ(pull(w, "loc_x"), orc.loc_x, err_msg=f"t={t}")
        EQ(pull(w, "_done_"), orc.done, err_msg=f"t={t}")
        EQ(pull(w, OBS), orc.obs.astype(np.float32), err_msg=f"t={t}")
        EQ(pull(w, REW), orc.rewards.astype(np.float32), err_msg=f"t={t}")
        words = _words(w.env_resetter._pool_rng, E)
        w.reset_only_done_envs()
        rows_used.add(restart(words))
    assert restarts >= 3 * E and max(rows_used) == 5, (restarts, rows_used)   # >= 3 episodes, every pool row drawn
    # the same through a launch plan: sample, step, table reset, two pool launches, undo
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=gc.SAMPLER_SEED)
    probs = torch.from_numpy(case.probabilities()).cuda()
    engine = RolloutEngine(w, sampler, probabilities=[probs])
    assert not engine.fused and engine.step_kernel_name == "HipTagGridWorldStep"
    assert sum(name == "reset_when_done_from_pool" for name in engine.entry_names) == 2, engine.entry_names
    before = restarts
    for t in range(n_ticks):
        words = _words(w.env_resetter._pool_rng, E)
        engine.run(1)
        torch.cuda.synchronize()
        a = pull(w, ACT)[..., 0]
        assert a.min() >= 0 and a.max() <= 4
        orc.step(a)
        EQ(pull(w, REW), orc.rewards.astype(np.float32), err_msg=f"engine t={t}")
        restart(words)
    print(f"{case.name}: {before} restarts through the wrapper, {restarts - before} through the launch plan")
    assert restarts - before >= 2 * E
