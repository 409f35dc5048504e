"""Host checks of tests/tick_range_cases.py: the range checker must name planted faults, the cohort cuts must be what the
range tests assume, `_range_args` must size the grid for the range, and the seeded sweep of the fused tick must contain
the shapes it is there for.  No GPU."""
import numpy as np
import pytest

from tests import tick_range_cases as trc

E, N, K, BEGIN, END = 11, 3, 2, 4, 8


def _snapshot(rng):
    f32 = np.float32
    out = {k: rng.standard_normal((E, N)).astype(f32) for k in ("rewards", "loc_x", "loc_y", "speed", "direction",
                                                               "acceleration", "edge_hit_reward_penalty")}
    out["observations"] = rng.standard_normal((E, N, 7 * K + 1)).astype(f32)
    out["sampled_actions"] = rng.randint(0, 5, size=(E, N, 2)).astype(np.int32)
    out["nearest_neighbor_ids"] = rng.randint(-1, N, size=(E, N, K)).astype(np.int32)
    out["still_in_the_game"] = rng.randint(0, 2, size=(E, N)).astype(np.int32)
    out["obs_rows_cleared"] = rng.randint(0, 2, size=(E, N)).astype(np.int32)
    out["knn_prev"] = rng.randint(-1, 99, size=(E, 1, 8)).astype(np.int32)
    out["num_runners"] = rng.randint(0, N, size=(E,)).astype(np.int32)
    out["_timestep_"] = rng.randint(0, 5, size=(E,)).astype(np.int32)
    out["_done_"] = rng.randint(0, 2, size=(E,)).astype(np.int32)
    out[trc.RNG] = rng.randint(0, 2 ** 31, size=(trc.RNG_HEADER_WORDS + E * N,)).astype(np.uint32)
    return out


@pytest.fixture
def clean():
    """(before, after, whole) of a launch that kept to [BEGIN, END)"""
    rng = np.random.RandomState(7)
    before, whole = _snapshot(rng), _snapshot(rng)
    whole[trc.RNG][:trc.RNG_HEADER_WORDS] = before[trc.RNG][:trc.RNG_HEADER_WORDS]
    before["_done_"][END + 1] = 1
    whole["_done_"][END + 1] = 0  # (the tick clears the flag of a replica that finished on the tick before)
    after = {}
    for k in before:
        after[k] = before[k].copy()
        if k == trc.RNG:
            body = after[k][trc.RNG_HEADER_WORDS:].reshape(E, N)
            body[BEGIN:END] = whole[k][trc.RNG_HEADER_WORDS:].reshape(E, N)[BEGIN:END]
        else:
            after[k][BEGIN:END] = whole[k][BEGIN:END]
    return before, after, whole


def test_snapshot_holds_every_array_the_tick_may_write():
    assert set(_snapshot(np.random.RandomState(0))) == set(trc.ARRAYS) | set(trc.EXTRA_ARRAYS) | {trc.RNG}


def test_checker_passes_a_launch_that_kept_to_its_range(clean):
    before, after, whole = clean
    assert trc.check_range(before, after, whole, BEGIN, END, N) == []
    # the empty range: nothing may change
    assert trc.check_range(before, before, whole, BEGIN, BEGIN, N) == []
    assert trc.check_range(before, after, whole, BEGIN, BEGIN, N) != []
    # the whole range
    assert trc.check_range(before, whole, whole, 0, E, N) == []


def _one_fault(faults, array, replica, where):
    assert len(faults) == 1, faults
    assert faults[0].startswith(array + ":") and f"[{replica}]" in faults[0] and where in faults[0], faults


def test_checker_names_a_replica_at_end_that_moved(clean):
    before, after, whole = clean
    after["loc_x"][END, 1] = whole["loc_x"][END, 1]
    _one_fault(trc.check_range(before, after, whole, BEGIN, END, N), "loc_x", END, "outside")


def test_checker_names_an_epoch_word_that_advanced_below_begin(clean):
    before, after, whole = clean
    after[trc.RNG][trc.RNG_HEADER_WORDS + (BEGIN - 1) * N + 2] += 1
    _one_fault(trc.check_range(before, after, whole, BEGIN, END, N), trc.RNG, BEGIN - 1, "outside")


def test_checker_names_a_changed_rng_header(clean):
    before, after, whole = clean
    after[trc.RNG][1] ^= 1
    faults = trc.check_range(before, after, whole, BEGIN, END, N)
    assert faults == [f"{trc.RNG}: header words changed"]


def test_checker_names_a_boundary_replica_stepped_twice(clean):
    before, after, whole = clean
    after["_timestep_"][END - 1] += 1
    _one_fault(trc.check_range(before, after, whole, BEGIN, END, N), "_timestep_", END - 1, "inside")
    after["_timestep_"][END - 1] -= 1
    after["_timestep_"][BEGIN - 1] += 1  # ... or the neighbour's replica, stepped by this launch as well
    _one_fault(trc.check_range(before, after, whole, BEGIN, END, N), "_timestep_", BEGIN - 1, "outside")


def test_checker_names_a_done_flag_cleared_outside_the_range(clean):
    before, after, whole = clean
    assert before["_done_"][END + 1] == 1 and after["_done_"][END + 1] == 1
    after["_done_"][END + 1] = 0
    _one_fault(trc.check_range(before, after, whole, BEGIN, END, N), "_done_", END + 1, "outside")


@pytest.mark.parametrize("replica,where", [(BEGIN + 1, "inside"), (0, "outside"), (E - 1, "outside")])
def test_checker_names_an_observation_row_that_differs_in_one_bit(clean, replica, where):
    before, after, whole = clean
    after["observations"].view(np.uint32)[replica, N - 1, 7 * K] ^= 1
    _one_fault(trc.check_range(before, after, whole, BEGIN, END, N), "observations", replica, where)


def test_checker_compares_bit_patterns_not_values(clean):
    before, after, whole = clean
    whole["rewards"][BEGIN, 0] = after["rewards"][BEGIN, 0] = np.float32(0.0)
    assert trc.check_range(before, after, whole, BEGIN, END, N) == []
    after["rewards"][BEGIN, 0] = np.float32(-0.0)  # equal as a number
    _one_fault(trc.check_range(before, after, whole, BEGIN, END, N), "rewards", BEGIN, "inside")
    whole["speed"][BEGIN, 0] = after["speed"][BEGIN, 0] = np.float32(np.nan)  # unequal as a number
    assert len(trc.check_range(before, after, whole, BEGIN, END, N)) == 1


def test_run_dependent_hint_is_still_held_to_its_range(clean):
    """`knn_prev` of the shapes whose kernel writes it differs from launch to launch (run_dependent_arrays): inside the
    range it is not compared with the twin's, outside the range it must not move like any other array"""
    before, after, whole = clean
    after["knn_prev"][BEGIN + 1, 0, 3] ^= 0x10001
    _one_fault(trc.check_range(before, after, whole, BEGIN, END, N), "knn_prev", BEGIN + 1, "inside")
    assert trc.check_range(before, after, whole, BEGIN, END, N, run_dependent=("knn_prev",)) == []
    after["knn_prev"][END, 0, 0] ^= 1
    _one_fault(trc.check_range(before, after, whole, BEGIN, END, N, run_dependent=("knn_prev",)), "knn_prev", END, "outside")
    shapes = trc.range_shapes()
    assert [n for n in shapes if trc.run_dependent_arrays(shapes[n])] == ["n304_heads10_6", "n604"]
    assert all(trc.run_dependent_arrays(shapes[n]) == ("knn_prev",) for n in ("n304_heads10_6", "n604"))


# ---------------------------------------------------------------------------------------------------------------------
def test_range_list():
    for E_, epb in [(155, 51), (23, 7), (11, 3), (59, 19), (7, 1)]:
        r = trc.ranges(E_, epb)
        assert r[:6] == [(0, E_), (1, E_ - 1), (epb + 1, epb + 2), (0, 1), (E_ - 1, E_), (epb + 1, epb + 1)]
        part = r[6:]
        assert part == trc.partition(E_, epb) and len(part) == 3
        assert part[0][0] == 0 and part[-1][1] == E_ and all(a[1] == b[0] for a, b in zip(part, part[1:]))
        assert all(b < e for b, e in part)
        if epb > 1:
            assert all(b % epb for b, _ in part[1:])


def test_range_shapes_cover_the_entry_classes():
    shapes = trc.range_shapes()
    assert list(shapes) == trc.RANGE_SHAPE_NAMES and set(trc.COHORT_SHAPE_NAMES) <= set(shapes)
    entries = [s["entry"] for s in shapes.values()]
    classes = {"folded" if "A21" in e else "n512" if e.endswith("_N512") else "n1024" if e.endswith("_N1024") else
               "generic" if e == "HipTagContinuousStep" else "k" for e in entries}
    assert classes == {"folded", "n512", "n1024", "generic", "k"}
    assert {s["epb"] for s in shapes.values()} >= {51, 19, 7, 3, 1}
    for s in shapes.values():
        cfg = s["cfg"]
        assert 5 <= cfg["episode_length"] <= 7
        assert s["E"] == (3 * s["epb"] + 2 if s["epb"] > 1 else 7)
        assert s["N"] == cfg["num_taggers"] + cfg["num_runners"]
    heads = [(s["cfg"]["num_acceleration_levels"] + 1, s["cfg"]["num_turn_levels"] + 1) for s in shapes.values()]
    assert (24, 25) in heads and any(a > b for a, b in heads)
    assert any(s["cfg"]["num_other_agents_observed"] > s["N"] - 1 for s in shapes.values())


class _StubFunctionManager:
    """the geometry rule of HIPFunctionManager without a device"""

    def __init__(self, n_agents, n_envs):
        self._num_agents, self._num_envs = n_agents, n_envs

    def has_function(self, name):
        return name in ("HipTagContinuousStep_K10_N105A21",)

    def packed_geometry(self, *args, **kwargs):
        from warp_drive_amd.managers.function_manager import HIPFunctionManager

        return HIPFunctionManager.packed_geometry(self, *args, **kwargs)


def _host_env(shape):
    from warp_drive_amd.envs.tag_continuous import TagContinuous

    env = TagContinuous(**shape["cfg"])
    env.cuda_function_manager = _StubFunctionManager(shape["N"], shape["E"])
    env.cuda_step_function_feed = lambda names: list(names)
    return env


@pytest.mark.parametrize("name", trc.RANGE_SHAPE_NAMES)
def test_shape_geometry_entry_and_grid_rule(name):
    """every RANGE_SHAPES row: the geometry and the entry name it states, and `_range_args` on every range of ranges():
    grid = ceil((end - begin) / epb), at least 1; kNumEnvs = end, kEnvBegin = begin"""
    shape = trc.range_shapes()[name]
    env = _host_env(shape)
    E_, epb = shape["E"], shape["epb"]
    assert env._geometry() == (epb, (shape["threads"], 1, 1), (-(-E_ // epb), 1))
    assert env.resolve_step_function_name("HipTagContinuousStep") == shape["entry"]
    assert trc.has_tick_on_given_actions(shape) == env._fast_path()
    n_envs_pos = env._STEP_ARGS.index(("n_envs", "meta"))
    args, _, block, grid = env._range_args(None)
    assert int(args[-1]) == 0 and args[n_envs_pos] == ("n_envs", "meta") and grid == (-(-E_ // epb), 1)
    for begin, end in trc.ranges(E_, epb):
        args, epb_, block, grid = env._range_args((begin, end))
        assert epb_ == epb and block == (shape["threads"], 1, 1)
        assert grid == (max(1, -(-(end - begin) // epb)), 1), (begin, end, grid)
        assert int(args[n_envs_pos]) == end and int(args[-1]) == begin and len(args) == len(env._STEP_ARGS) + 1
        # the blocks of the launch cover [begin, end) and no block starts at or beyond `end` (unless the range is empty)
        assert begin + grid[0] * epb >= end and (begin + (grid[0] - 1) * epb < end or begin == end)


def test_cohort_bounds_partition_the_replicas_at_multiples_of_32():
    from warp_drive_amd.rollout import COHORT_ALIGN, cohort_bounds

    assert COHORT_ALIGN == 32
    for C in (2, 3, 4):
        for E_ in range(1, 5001):
            b = cohort_bounds(E_, C)
            assert len(b) == C and b[0][0] == 0 and b[-1][1] == E_
            assert all(x[1] == y[0] for x, y in zip(b, b[1:])) and all(lo <= hi for lo, hi in b)
            assert all(lo % 32 == 0 for lo, _ in b[1:])
            # near-equal cohorts: a cut is the multiple of 32 nearest to E * c / C wherever that lies inside [0, E]
            for c, (lo, _) in enumerate(b[1:], start=1):
                nearest = int(round(E_ * c / C / 32)) * 32
                assert lo == nearest or (nearest > E_ and lo == E_ // 32 * 32), (E_, C, b)


def test_cohort_cuts_fall_inside_blocks_of_the_packed_shapes():
    """what makes the cohort cases worth running: with E = epb * B * C + 45 (B blocks per cohort at least) an inner cut is
    no multiple of epb for the packed shapes, whatever B the device has"""
    from warp_drive_amd.rollout import cohort_bounds

    shapes = trc.range_shapes()
    for name in trc.COHORT_SHAPE_NAMES:
        epb = shapes[name]["epb"]
        if epb == 1:
            continue
        for half_cus in (52, 64, 120, 128, 152):
            for C in (2, 3):
                cuts = [lo for lo, _ in cohort_bounds(epb * half_cus * C + 45, C)[1:]]
                assert any(c % epb for c in cuts), (name, half_cus, C, cuts)


# ---------------------------------------------------------------------------------------------------------------------
def test_random_configuration_is_the_sweep_it_was():
    """the generator moved here from test_random_configurations: same draws, in the same order (first cases pinned)"""
    cfg, E_ = trc.random_configuration(np.random.RandomState(1000))
    rng = np.random.RandomState(1000)
    assert cfg["num_taggers"] == int(rng.randint(1, 7))
    assert cfg["num_runners"] == int(rng.choice([1, 2, 5, 30, 58, 59, 60, 63, 64, 65, 100, 123, 124, 127, 130]))
    assert len(cfg) == 24 and E_ in (1, 2, 3, 7, 33)
    cfg2, E2 = trc.random_configuration(np.random.RandomState(1000))
    assert cfg2 == cfg and E2 == E_


def test_fused_tick_sweep_coverage():
    cases = [trc.fused_tick_sweep_case(c) for c in range(trc.FUSED_SWEEP_CASES)]
    assert len(cases) == 32
    seen = set()
    for cfg, E_, heads in cases:
        n = cfg["num_taggers"] + cfg["num_runners"]
        full = cfg["use_full_observation"]
        assert E_ in (1, 2, 3, 7, 33) and 1 <= cfg["num_other_agents_observed"] <= max(n - 1, 1)
        assert heads == (cfg["num_acceleration_levels"] + 1, cfg["num_turn_levels"] + 1) and min(heads) >= 2
        assert not full or n <= 70
        epb = _StubFunctionManager(n, E_).packed_geometry(n, max_threads=256, prefer_large=full)[0]
        if epb > 1 and E_ % epb:
            seen.add("ragged last block")
        if epb > 1 and E_ > epb and E_ % epb:
            seen.add("ragged last block after a full one")
        seen.add(f"N={n}" if n in (64, 65, 128) else "N>128" if n > 128 else "other N")
        seen.add("full" if full else "partial")
        seen.add("exits" if cfg["runner_exits_game_after_tagged"] else "stays")
        seen |= {f"head {h}" for h in heads if h in (24, 25)}
        if max(heads) > 64:
            seen.add("head > 64")
        if heads[0] != heads[1]:
            seen.add("larger head first" if heads[0] > heads[1] else "larger head second")
        if not full and cfg["num_other_agents_observed"] > 32:
            seen.add("generic K")
    want = {"ragged last block", "ragged last block after a full one", "N=64", "N=65", "N=128", "N>128", "full", "partial",
            "exits", "stays", "head 24", "head 25", "head > 64", "larger head first", "larger head second", "generic K"}
    assert want <= seen, want - seen
    assert len(trc.TICK_ON_GIVEN_ACTIONS_SWEEP) >= 16
    for c in trc.TICK_ON_GIVEN_ACTIONS_SWEEP:
        cfg = cases[c][0]
        assert not cfg["use_full_observation"] and cfg["num_other_agents_observed"] <= 32


def test_sweep_probabilities_hold_the_end_cases():
    for A in (2, 3, 24, 25, 71):
        p = trc.sweep_probabilities(np.random.RandomState(A), 5, 7, A)
        assert p.dtype == np.float32 and p.shape == (5, 7, A)
        np.testing.assert_allclose(p.sum(axis=-1), 1.0, atol=1e-5)
        for e in range(5):
            one_hot = [(row == 1.0).sum() == 1 and (row == 0.0).sum() == A - 1 for row in p[e]]
            assert any(one_hot)
            if A >= 3:
                assert any(row[0] == 0.0 and row[-1] == 0.0 and (row[1:-1] > 0).all() for row in p[e])
