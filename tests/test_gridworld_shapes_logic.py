"""Host-side restatement of the arithmetic the TagGridWorld kernels (csrc/kernels/tag_gridworld.hip,
tag_gridworld_n5.hip) rely on, over the whole admissible range, and of the host rules that size their launches
(envs/tag_gridworld.py).  The kernels themselves run in tests/test_gpu_gridworld_shapes.py, whose cases
(tests/gridworld_cases.py) are simulated here with the oracle alone and must reach the coverage they are meant to have.
`pytest -s` prints the lists docs/rounds/r10.md quotes."""
import types

import numpy as np
import pytest

from tests import gridworld_cases as gc

F32 = np.float32
IMAGE_MAX_BYTES = 60000   # WD_GW_IMAGE_MAX_BYTES
BLOCK_SIZES = (256, 128, 64)   # what _geometry() tries


def _env(N, full, **kw):
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorld

    return CUDATagGridWorld(num_taggers=N - 1, use_full_observation=full, **kw)


def _packed_geometry(N, E, max_threads):
    from warp_drive_amd.managers.function_manager import HIPFunctionManager

    me = types.SimpleNamespace(_num_agents=N, _num_envs=E)
    return HIPFunctionManager.packed_geometry(me, N, max_threads=max(max_threads, N))


# ------------------------------------------------------------------------------------ the kernels' LDS layout, restated
def kernel_tables_bytes(N, epb):
    """byte offset of `s_obs` in gw_step_impl / gw_rollout_impl: 4 A + 2 epb + 2 ints, padded to 16 bytes"""
    A = epb * N
    ints = 4 * A + 2 * epb + 2
    return 4 * (ints + ((4 - (ints & 3)) & 3))


def kernel_image(N, F, epb):
    """the kernel's `image` expression"""
    A = epb * N
    return ((4 * (4 * A + 2 * epb + 2) + 15) & ~15) + 4 * A * F <= IMAGE_MAX_BYTES


def _F(N, full):
    return 4 * N + 1 if full else 6


def test_host_lds_rule_is_the_kernels():
    """lds_bytes(epb) == the kernel's table offset (16-byte aligned) + the image where the kernel's `image` holds, for
    every N, mode and replicas-per-block a block of up to 1024 threads can have; `s_cache` sits directly behind it"""
    no_image = []
    for full in (True, False):
        for N in range(2, 1025):
            env, F = _env(N, full), _F(N, full)
            for epb in range(1, max(1, 1024 // N) + 1):
                tables, image = kernel_tables_bytes(N, epb), kernel_image(N, F, epb)
                assert tables % 16 == 0
                assert tables == ((4 * (4 * epb * N + 2 * epb + 2) + 15) & ~15)   # the two spellings in the kernel agree
                assert env.lds_bytes(epb) == tables + (4 * epb * N * F if image else 0), (N, full, epb)
                assert env.image_fits(epb) == image, (N, full, epb)
            if not kernel_image(N, F, 1):
                no_image.append((N, full))
    first_full = min(n for n, f in no_image if f)
    first_partial = min((n for n, f in no_image if not f), default=None)
    print(f"no LDS image even at one replica per block: full observations from N = {first_full}, "
          f"partial observations from N = {first_partial}")
    assert first_full == 61 and first_partial is None   # 4 * 61 * 245 + tables > 60000


def _rollout_shapes():
    """(N, full, thread cap, epb, image, cache dwords that fit or 0) for the three block sizes _geometry() tries; the
    registered reset arrays of CUDATagGridWorld are the positions and the observations: 2 N + N F dwords per replica"""
    for full in (True, False):
        for N in range(2, 1025):
            env, F = _env(N, full), _F(N, full)
            for m in BLOCK_SIZES:
                epb, block, _ = _packed_geometry(N, 1000, m)
                image = env.image_fits(epb)
                cd = 2 * N + N * F
                cache = cd if image and env.lds_bytes(epb) + 4 * epb * cd <= IMAGE_MAX_BYTES else 0
                yield N, full, m, epb, image, cache


def test_lds_branches_by_shape():
    """which shapes run without the LDS image and which rollouts run without the restore cache (the GPU cases are
    drawn from these lists)"""
    shapes = list(_rollout_shapes())
    for full in (True, False):
        for threads in BLOCK_SIZES:
            rows = [s for s in shapes if s[1] == full and s[2] == threads]
            no_img = [s[0] for s in rows if not s[4]]
            no_cache = [s[0] for s in rows if s[4] and not s[5]]
            print(f"{'full' if full else 'partial'} observations, blocks of up to {threads} threads: no image N = "
                  f"{_ranges(no_img)}; image but no restore cache N = {_ranges(no_cache)}")
    pick = {(s[0], s[1], s[2]): s for s in shapes}
    assert pick[(13, True, 256)][4] and pick[(13, True, 256)][5] == 0      # rollout_N13_L10_full_nocache at 256 threads
    assert pick[(6, True, 256)][5] > 0 and pick[(6, True, 64)][5] > 0
    assert not pick[(15, True, 256)][4] and pick[(15, True, 64)][4]        # the shape of the geometry fix
    assert not pick[(64, True, 64)][4] and pick[(64, False, 64)][4]


def _ranges(values):
    out, values = [], sorted(values)
    i = 0
    while i < len(values):
        j = i
        while j + 1 < len(values) and values[j + 1] == values[j] + 1:
            j += 1
        out.append(str(values[i]) if i == j else f"{values[i]}..{values[j]}")
        i = j + 1
    return ", ".join(out) or "-"


def test_quotient_without_a_division_is_exact():
    """`(int)(((float)q + 0.5f) * (1.0f / (float)re))` == q / re for every q the cache fill of both rollout kernels can
    see: every N, both modes, the block sizes _geometry() tries, every shape whose image and cache fit, re in
    {N, N F} (the row lengths of the positions and the observations), q < epb * re"""
    pairs = mismatches = q_max = 0
    for N, full, threads, epb, image, cache in _rollout_shapes():
        if not cache:
            continue
        for re in (N, N * _F(N, full)):
            q = np.arange(epb * re, dtype=np.int64)
            got = ((q.astype(F32) + F32(0.5)) * (F32(1.0) / F32(re))).astype(F32).astype(np.int64)
            mismatches += int((got != q // re).sum())
            pairs += 1
            q_max = max(q_max, int(q[-1]))
    print(f"q / re without a division: {pairs} (shape, re) pairs, {mismatches} mismatches, largest q {q_max}")
    assert pairs > 4000 and mismatches == 0
    # the specialised kernel: 12 replicas, re in {5, 105}
    for re in (5, 105):
        q = np.arange(12 * re)
        assert ((((q.astype(F32) + F32(0.5)) * (F32(1.0) / F32(re))).astype(np.int64)) == q // re).all()


# ---------------------------------------------------------------------------------------------- the N5 block remap
def n5_group0(block, grid):
    xcd, nq, nr = block & 7, grid >> 3, grid & 7
    return xcd * nq + min(xcd, nr) + (block >> 3)


def test_n5_block_remap_is_a_bijection_and_the_trips_cover_every_group_once():
    for grid in range(1, 4097):
        groups = sorted(n5_group0(b, grid) for b in range(grid))
        assert groups == list(range(grid)), grid
    for E, grid in ((100, 1), (100, 7), (1000, 8), (1000, 9), (1000, 13), (12 * 2600 + 7, 100), (31207, 257),
                    (5000, 3), (12 * 40, 39)):
        n_groups = -(-E // 12)
        assert grid < n_groups
        visits = np.zeros(n_groups, int)
        for b in range(grid):
            env0 = n5_group0(b, grid) * 12
            while env0 < E:
                visits[env0 // 12] += 1
                env0 += grid * 12
        assert (visits == 1).all(), (E, grid)


# ---------------------------------------------------------------------------------------------- the N5 LDS formulas
def n5_layout_bytes(CD, T, H):
    """gw5_rollout: s_obs [1260], s_cache [12 CD], s_div [64], s_tn [T + 1] (rounded up to four floats in front of the
    policies), s_pol [2][gw5_policy_floats(H)]"""
    floats = 12 * 105 + 12 * CD + 64
    if H == 0:
        return 4 * (floats + T + 1)
    pol = (H * 24 + H + H * H + H + 5 * H + 5 + 3) & ~3
    return 4 * (floats + ((T + 1 + 3) & ~3) + 2 * pol)


def test_n5_lds_formulas_match_the_kernel_layout():
    from warp_drive_amd.envs.tag_gridworld import gridworld_policy_floats

    CD = 5 + 5 + 105
    for T in (1, 2, 3, 4, 23, 100, 1503, 1504, 4095):
        env = _env(5, True, episode_length=T)
        for H in (32, 64):
            assert gridworld_policy_floats(H) == (H * 24 + H + H * H + H + 5 * H + 5 + 3) & ~3
            need = n5_layout_bytes(CD, T, H)
            assert need <= env.live_policy_lds_bytes(H) < need + 16 and env.live_policy_lds_bytes(H) % 16 == 0
            assert env.live_policy_lds_bytes(H) == env.live_policy_lds_bytes(H, CD)
        fixed = _tick_launch(env, 1000, 4)[4]     # the fixed-policy entry's bytes as tick_launch computes them
        assert n5_layout_bytes(CD, T, 0) <= fixed < n5_layout_bytes(CD, T, 0) + 16
        assert (12 * 105) % 4 == 0 and (12 * CD) % 4 == 0 and (12 * 105 + 12 * CD + 64) % 4 == 0   # s_pol stays 16-byte aligned


def test_the_rollout_units_share_one_policy_header_and_its_float_counts():
    """the five units with an in-kernel policy are built around csrc/kernels/rollout_policy.h, and its float counts --
    restated here, next to the header's own expressions -- are what the host sizes the launches' LDS with"""
    import os

    from warp_drive_amd import build as wd_build
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv
    from warp_drive_amd.envs.classic_control import rollout_actor_floats
    from warp_drive_amd.envs.tag_gridworld import gridworld_policy_floats

    header = os.path.join(wd_build.KDIR, "rollout_policy.h")
    for unit in ("wd_kernels.hip", "cartpole_pool.hip", "classic_control.hip", "tag_gridworld_n5.hip",
                 "tag_gridworld_n5_pool.hip"):
        assert header in wd_build.unit_sources(unit), unit
    text = open(header).read()
    for expression in ("rp_pad4(int n) { return (n + 3) & ~3; }",
                       "rp_policy_floats(int I, int H, int A) { return I * H + H + H * H + H + A * H + A; }",
                       "rp_actor_op(int O) { return (O + 1) & ~1; }",
                       "rp_actor_floats(int H, int O) { return rp_actor_op(O) * H + H + H * H + H + H + 1; }"):
        assert expression in text, expression
    common = open(os.path.join(wd_build.KDIR, "tag_gridworld_n5_common.h")).read()
    assert "return rp_pad4(rp_policy_floats(GW5_IN_STRIDE, H, GW5_ACTIONS));" in common
    assert "GW5_IN_STRIDE = 24;" in common and "GW5_ACTIONS = 5;" in common

    def rp_pad4(n):
        return (n + 3) & ~3

    def rp_policy_floats(I, H, A):
        return I * H + H + H * H + H + A * H + A

    def rp_actor_floats(H, O):
        return ((O + 1) & ~1) * H + H + H * H + H + H + 1

    for H in (32, 64):
        assert gridworld_policy_floats(H) == rp_pad4(rp_policy_floats(24, H, 5))
        for O in (2, 3, 4, 6):
            assert rollout_actor_floats(O, H) == rp_actor_floats(H, O)
        for A in (1, 2, 3, 5, 8):
            policy_bytes = CUDAClassicControlCartPoleEnv.pool_rollout_lds_bytes(H, A, 0, False)
            assert policy_bytes == 4 * rp_pad4(rp_policy_floats(4, H, A))
            assert CUDAClassicControlCartPoleEnv.pool_rollout_lds_bytes(H, A, 7, True) == policy_bytes + 16 * 7


def test_live_policy_rollout_has_one_lds_limit():
    """has_live_policy_rollout admits a shape only if its launch fits ROLLOUT_POLICY_MAX_LDS (the time table grows with
    the episode length); H = 64 passes 64 KiB at episode_length 1504 and needs 75 904 bytes at 4095"""
    env = _fake_managed(_env(5, True, episode_length=1503), 1000)
    assert env.live_policy_lds_bytes(64) <= 65536 < _env(5, True, episode_length=1504).live_policy_lds_bytes(64) == 65552
    big = _fake_managed(_env(5, True, episode_length=4095), 1000)
    assert big.live_policy_lds_bytes(64) == 75904 and big.live_policy_lds_bytes(32) <= 65536
    for e in (env, big):
        for H in (32, 64):
            assert e.has_live_policy_rollout(H, 5) == (e.live_policy_lds_bytes(H) <= e.ROLLOUT_POLICY_MAX_LDS)
    big.ROLLOUT_POLICY_MAX_LDS = 65536
    assert big.has_live_policy_rollout(32, 5) and not big.has_live_policy_rollout(64, 5)


# ------------------------------------------------------------------------------------------------- the reward table
def test_reward_table_is_float32_of_the_float64_sum():
    """the eight sums of tag_gridworld_rewards.h against the oracle's float64 `reward_tag + penalty`, narrowed once,
    for a few hundred scalar sets; and the sets the GPU cases use must tell the float32-add form apart"""
    from oracle.tag_gridworld_np import TagGridWorldOracle

    rng = np.random.RandomState(0)
    sets = list(gc.REWARD_SETS.values()) + [(0.0, 0.0, 0.0, 0.0), (0.0, 1.0, 1.0, 0.0), (1e-30, 1e-30, 3e-31, 7e-31),
                                            (-0.1, -10.0, -2.0, -0.01)]
    sets += [tuple(rng.uniform(-20, 20, 4) * 10.0 ** rng.randint(-6, 3, 4)) for _ in range(300)]
    differ = 0
    for s in sets:
        table = gc.reward_table(s)
        # the oracle's own step on a 2-agent replica in each of the eight situations
        for tagged in (0, 1):
            for wall_t in (0, 1):
                for wall_r in (0, 1):
                    orc = TagGridWorldOracle(1, num_taggers=1, grid_length=3, episode_length=9,
                                             starting_location_x=[1 if not wall_t else 0, 0 if tagged and wall_t else (1 if tagged else 3)],
                                             starting_location_y=[0, 0], wall_hit_penalty=s[0], tag_reward_for_tagger=s[1],
                                             tag_penalty_for_runner=s[2], step_cost_for_tagger=s[3])
                    # tagger: left into the wall (from x = 0) or stay; runner: right into the wall (from x = 3), left
                    # into it (from x = 0), or stay
                    a_t = 2 if wall_t else 0
                    a_r = (2 if orc.loc_x[0, 1] == 0 else 1) if wall_r else 0
                    if wall_r and not (orc.loc_x[0, 1] in (0, 3)):
                        continue   # (a runner in the open cannot hit a wall on this tick)
                    orc.step(np.array([[a_t, a_r]]))
                    is_tag = bool(orc.loc_x[0, 0] == orc.loc_x[0, 1])
                    if is_tag != bool(tagged):
                        continue
                    assert F32(orc.rewards[0, 0]) == table[0, tagged, wall_t], (s, tagged, wall_t)
                    assert F32(orc.rewards[0, 1]) == table[1, tagged, wall_r], (s, tagged, wall_r)
        differ += int((table != gc.reward_table_float32_add(s)).any())
    print(f"reward table: {differ} of {len(sets)} scalar sets have a sum where float32(a) + float32(b) != float32(a + b)")
    for name, s in gc.REWARD_SETS.items():
        if name != "shipped":
            assert (gc.reward_table(s) != gc.reward_table_float32_add(s)).any(), name
    used = {c.reward for c in gc.STEP_CASES + gc.TICK_CASES + gc.ROLLOUT_CASES}
    assert "shipped" not in used and used == set(gc.REWARD_SETS) - {"shipped"}


# ---------------------------------------------------------------------------- tick_launch with fakes for the managers
class _FakeFn:
    def __init__(self, name):
        self.name = name


class _FakeFM:
    def __init__(self, N, E):
        self.N, self.E = N, E

    def packed_geometry(self, n_agents=None, max_threads=512, prefer_large=False):
        return _packed_geometry(self.N, self.E, max_threads)

    def initialize_functions(self, names):
        pass

    def has_function(self, name):
        return True

    def get_function(self, name):
        return _FakeFn(name)

    def global_address(self, name):
        return 0


class _FakeDM:
    reset_data_list = ["loc_x", "loc_y", "observations"]

    def __init__(self, N, F, E):
        self.shapes, self.E = {"loc_x": (E, N), "loc_y": (E, N), "observations": (E, N, F)}, E

    def meta_info(self, key):
        return {"n_envs": self.E}[key]

    def get_shape(self, name):
        return self.shapes[name]


class _FakeResetter:
    def fused_launch(self, dm, force, undo):
        return None, [0, 0], None, None


def _fake_managed(env, E):
    N, F = env.num_agents, _F(env.num_agents, env.use_full_observation)
    env.cuda_function_manager, env.cuda_data_manager = _FakeFM(N, E), _FakeDM(N, F, E)
    env.cuda_step = _FakeFn("HipTagGridWorldStep")
    env._step_args = lambda: [0] * 16
    return env


def _tick_launch(env, E, ticks):
    import torch

    _fake_managed(env, E)
    N, F = env.num_agents, _F(env.num_agents, env.use_full_observation)
    env.ticks_per_launch = ticks

    def tensor(shape, dtype):
        return types.SimpleNamespace(is_cuda=True, is_contiguous=lambda: True, dtype=dtype, shape=shape)

    batch = {"obs": tensor((ticks, E, N, F), torch.float32), "actions": tensor((ticks, E, N, 1), torch.int32),
             "rewards": tensor((ticks, E, N), torch.float32), "done": tensor((ticks, E), torch.int32)}
    sampler = types.SimpleNamespace(rng_state=0)
    probs = types.SimpleNamespace(shape=(E, N, 5))
    return env.tick_launch(sampler, [probs], _FakeResetter(), batch=batch)


def test_rollout_launch_has_an_image_or_says_unsupported():
    """for every N in 2 .. 64, both modes, 1 000 / 10 000 / 100 000 replicas: building the rollout launch yields a
    geometry whose blocks have the LDS image (and whose bytes are image + cache by the host rule), or raises
    UnsupportedRolloutShape -- never another error.  15 agents with full observations have an image at 64 threads (4
    replicas) and none at 256 (17): the launch must not depend on the replica count for its existence."""
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    unsupported, fell_back = set(), []
    for full in (True, False):
        for N in range(2, 65):
            outcomes = []
            for E in (1000, 10000, 100000):
                env = _env(N, full)
                try:
                    fn, args, block, grid, shared = _tick_launch(env, E, 4)
                except UnsupportedRolloutShape:
                    unsupported.add((N, full))
                    outcomes.append(None)
                    continue
                epb = max(1, block[0] // N) if not fn.name.endswith("_N5") else 12
                assert fn.name in ("HipTagGridWorldRollout", "HipTagGridWorldRollout_N5")
                assert kernel_image(N, _F(N, full), epb), (N, full, E, block)
                assert grid[0] == -(-E // epb) and block[0] >= min(N, 64) and shared <= 65536
                if fn.name == "HipTagGridWorldRollout":
                    cd = int(args[-1])
                    assert cd in (0, 2 * N + N * _F(N, full)) and shared == env.lds_bytes(epb) + 4 * epb * cd <= IMAGE_MAX_BYTES
                    if block != env._geometry()[1]:
                        fell_back.append((N, full, E, block[0]))
                outcomes.append(fn.name)
            assert all(o is None for o in outcomes) or all(o is not None for o in outcomes), (N, full, outcomes)
    print("rollout unsupported (no image at any block size):", _ranges([n for n, f in unsupported if f]), "with full "
          "observations;", _ranges([n for n, f in unsupported if not f]), "with partial")
    print("rollout geometry fell back to a smaller block:", sorted({(n, e, b) for n, f, e, b in fell_back}))
    assert any(n == 15 for n, f, e, b in fell_back) and all(f for n, f in unsupported)
    assert min(n for n, f in unsupported) == 61


# ---------------------------------------------------------------------------------- the GPU cases, oracle only
@pytest.mark.parametrize("case", gc.TICK_CASES + gc.ROLLOUT_CASES, ids=repr)
def test_gpu_case_reaches_its_coverage(case):
    """every Tick / Rollout case of the shape and geometry matrix: at least one tag, one time-out, one restart per two
    replicas, all eight (tagger / runner) x (tagged / not) x (wall / not) reward cases -- from the oracle alone"""
    _, _, cov = gc.simulate(case)
    print(f"{case.name}: {cov.line()}")
    cov.check(case.E)


def test_stacked_starts_produce_argmin_ties_on_different_cells():
    """the partial observation's closest tagger is the FIRST argmin: the stacked cases must contain ticks where the
    last argmin stands on another cell (else `d <= bd` in the kernel would pass)"""
    for case in [c for c in gc.STEP_CASES + gc.TICK_CASES + gc.ROLLOUT_CASES if c.starts == "stacked"]:
        assert not case.full
        orc, hits = gc.make_oracle(case), 0
        rng = np.random.RandomState(1)
        for _ in range(case.ticks):
            orc.step(rng.randint(0, 5, size=(case.E, case.N)))
            d = np.square(orc.loc_x[:, :-1] - orc.loc_x[:, -1:]) + np.square(orc.loc_y[:, :-1] - orc.loc_y[:, -1:])
            first, last = d.argmin(axis=1), d.shape[1] - 1 - d[:, ::-1].argmin(axis=1)
            ar = np.arange(case.E)
            hits += int(((orc.loc_x[ar, first] != orc.loc_x[ar, last]) | (orc.loc_y[ar, first] != orc.loc_y[ar, last])).sum())
            orc.reset_done_envs()
        assert hits > case.E, (case.name, hits)


def test_oracle_restart_rows_per_replica():
    """TagGridWorldOracle.reset_done_envs(x=, y=): done replicas restart from their own row, the others keep theirs"""
    from oracle.tag_gridworld_np import TagGridWorldOracle

    orc = TagGridWorldOracle(4, num_taggers=2, grid_length=5, episode_length=3)
    orc.done[:] = [1, 0, 1, 0]
    orc.timestep[:] = 2
    keep_x = orc.loc_x.copy()
    x, y = np.arange(12).reshape(4, 3), 20 + np.arange(12).reshape(4, 3)
    orc.reset_done_envs(x=x, y=y)
    np.testing.assert_array_equal(orc.loc_x[[0, 2]], x[[0, 2]])
    np.testing.assert_array_equal(orc.loc_y[[0, 2]], y[[0, 2]])
    np.testing.assert_array_equal(orc.loc_x[[1, 3]], keep_x[[1, 3]])
    np.testing.assert_array_equal(orc.timestep, [0, 2, 0, 2])
    assert orc.done.sum() == 0
