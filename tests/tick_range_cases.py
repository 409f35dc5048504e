"""Case lists and the checker of the replica-range tests of the TagContinuous tick (tests/test_gpu_tick_ranges.py), and
the seeded shape sweeps of tests/test_gpu_tag_continuous.py.  Nothing here needs a GPU: tests/test_tick_range_cases_host.py
checks the lists and the checker themselves.

A range launch is the tick entry with `kNumEnvs = end` and `kEnvBegin = begin` (TagContinuous._range_args): it must step
replicas [begin, end) exactly as a whole-range launch does and must not touch any other replica.  RolloutEngine's cohorts
cut the replicas at multiples of 32, which is no multiple of `epb` (replicas per block) off the headline shape."""
import numpy as np

# every array a TagContinuous tick (Step / Tick / TickA) may write, plus the sampler's RNG words ("rng_state":
# 4 header words, then one epoch word per (replica, agent))
ARRAYS = ("observations", "rewards", "_done_", "sampled_actions", "nearest_neighbor_ids", "loc_x", "loc_y", "speed",
          "direction", "acceleration", "still_in_the_game", "num_runners", "_timestep_")
EXTRA_ARRAYS = ("edge_hit_reward_penalty", "obs_rows_cleared", "knn_prev")
RNG = "rng_state"
RNG_HEADER_WORDS = 4

_PHYSICS = dict(grid_length=6.0, max_speed=0.6, max_acceleration=0.3, min_acceleration=-0.3, tagging_distance=0.12,
                edge_hit_penalty=-0.2, step_reward_for_runner=0.01, runner_exits_game_after_tagged=True)


def _shape(name, taggers, runners, K, levels, T, entry, epb, threads, full=False, seed=5):
    """one RANGE_SHAPES row: the configuration, the Step entry it must resolve to and the geometry `_geometry()` must
    give (asserted by the tests, so that no shape drifts to another entry class unnoticed)"""
    cfg = dict(_PHYSICS, num_taggers=taggers, num_runners=runners, num_other_agents_observed=K,
               num_acceleration_levels=levels[0], num_turn_levels=levels[1], episode_length=T, seed=seed,
               use_full_observation=full)
    E = 3 * epb + 2 if epb > 1 else 7
    return dict(name=name, cfg=cfg, entry=entry, epb=epb, threads=threads, E=E, N=taggers + runners)


# levels = (acceleration, turn); a head has levels + 1 actions.  Episodes of 5 .. 7 ticks: replicas finish and are
# restored inside ranges.
RANGE_SHAPES = [
    # `_K<k>`, whole replicas packed into 256-thread blocks
    _shape("n5", 1, 4, 2, (3, 3), 5, "HipTagContinuousStep_K2", 51, 256),
    _shape("n34_heads24_25", 3, 31, 7, (23, 24), 6, "HipTagContinuousStep_K8", 7, 256),  # both sides of WD_SLAB_CH = 24
    _shape("n65", 5, 60, 10, (5, 5), 7, "HipTagContinuousStep_K10", 3, 256),
    # ... K clipped by the agent count: neighbour rows padded with -1.  (The constructor asks K <= N, so "K = 10 > N - 1"
    # is a 10-agent shape; at 5 agents the largest K beyond N - 1 is 5.)
    _shape("n5_K4", 2, 3, 4, (4, 2), 5, "HipTagContinuousStep_K4", 51, 256),
    _shape("n5_K5", 2, 3, 5, (2, 6), 6, "HipTagContinuousStep_K6", 51, 256),
    _shape("n10_K10", 2, 8, 10, (6, 6), 5, "HipTagContinuousStep_K10", 19, 192),
    # ... one replica per block: one wavefront and two wavefronts without an idle lane
    _shape("n64", 4, 60, 12, (7, 7), 6, "HipTagContinuousStep_K12", 1, 64),
    _shape("n128", 6, 122, 16, (4, 8), 5, "HipTagContinuousStep_K16", 1, 128),
    # `_K<k>_N512`: three wavefronts; beyond 256 agents both heads are sampled from ONE slab (unequal heads, the larger
    # first: the wavefronts' rows of the two heads overlap)
    _shape("n134", 4, 130, 6, (3, 3), 6, "HipTagContinuousStep_K6_N512", 1, 192),
    _shape("n304_heads10_6", 4, 300, 10, (9, 5), 5, "HipTagContinuousStep_K10_N512", 1, 320),
    # `_K<k>_N1024`: a block of ten wavefronts
    _shape("n604", 4, 600, 10, (6, 8), 5, "HipTagContinuousStep_K10_N1024", 1, 640),
    # generic entry: full observations (`prefer_large` packing), and K beyond the specialisations (K-pass selection)
    _shape("n34_full", 3, 31, 5, (6, 8), 6, "HipTagContinuousStep", 7, 256, full=True),
    _shape("n60_K40", 4, 56, 40, (5, 5), 5, "HipTagContinuousStep", 1, 64),
]
# control: the class the suite already covers (size-folded entry of the headline configuration; its configuration is
# tests.test_gpu_tag_continuous.BENCH_CFG with a short episode, filled in by range_shapes())
HEADLINE = dict(name="n105_headline", entry="HipTagContinuousStep_K10_N105A21", epb=1, threads=128, E=7, N=105)
RANGE_SHAPE_NAMES = [s["name"] for s in RANGE_SHAPES] + [HEADLINE["name"]]
# the shapes a RolloutEngine with cohorts is run at (E is sized on the device: epb * half the CUs * C + 45)
COHORT_SHAPE_NAMES = ["n5", "n34_heads24_25", "n134", "n604", "n34_full"]


def range_shapes():
    """name -> shape row, the headline control included"""
    from tests.test_gpu_tag_continuous import BENCH_CFG

    out = {s["name"]: s for s in RANGE_SHAPES}
    out[HEADLINE["name"]] = dict(HEADLINE, cfg=dict(BENCH_CFG, episode_length=6))
    return out


def has_tick_on_given_actions(shape):
    """the fast entry classes have a TickA form, the generic entry has none"""
    return shape["entry"] != "HipTagContinuousStep"


def partition(E, epb):
    """three ranges that cover [0, E), cut at epb + 1 and 2 * epb + 1 (no multiple of epb for epb > 1)"""
    return [(0, epb + 1), (epb + 1, 2 * epb + 1), (2 * epb + 1, E)]


def ranges(E, epb):
    """the replica ranges every shape is launched on"""
    assert E >= 2 * epb + 2 and E >= 4
    return [(0, E), (1, E - 1), (epb + 1, epb + 2), (0, 1), (E - 1, E), (epb + 1, epb + 1)] + partition(E, epb)


def _bits(a, E):
    """[E, bytes per replica] view of an array's bit patterns"""
    a = np.ascontiguousarray(a)
    return a.reshape(E, -1).view(np.uint8) if a.size else a.reshape(E, 0).view(np.uint8)


def run_dependent_arrays(shape):
    """arrays whose content differs between two launches of the same kernel on the same state: `knn_prev`, the hint of
    the prefiltered neighbour search, wherever the kernel writes it (the fast entries with at least WD_TC_PRE_MIN_LIVE =
    200 agents in the game).  It holds the K + 3 nearest in the order of the cell-sorted packing, which within a cell is
    the order of LDS atomics (tc_knn.h, "CELL-SORTED packing": "varies from run to run and changes nothing that leaves
    the kernel but the look-ahead ids remembered in `knn_prev`").  Seen on the device: the 304-agent shape, Step, tick
    0, the range [0, 7) of 7 replicas against the whole-range launch of the twin -- the same launch twice -- differed in
    `knn_prev` of replicas 2 and 5 and in nothing else.  Such an array cannot equal the twin's inside the range; it must
    still be untouched outside it, and whatever it holds must not move any other array on the ticks that follow."""
    return ("knn_prev",) if has_tick_on_given_actions(shape) and shape["N"] >= 200 else ()


def check_range(before, after, whole, begin, end, N, run_dependent=()):
    """`after` = `before` + ONE launch on replicas [begin, end); `whole` = `before` + one whole-range launch (the twin).
    Replicas in [begin, end) must equal `whole`, every other replica (and the RNG header) `before`, bit for bit.
    run_dependent: arrays left out of the first comparison (run_dependent_arrays), never of the second.
    Returns the list of faults, one line per (array, kind), naming the replicas; empty = the launch kept to its range."""
    faults = []
    E = int(np.asarray(before["_done_"]).shape[0])
    inside = np.zeros(E, dtype=bool)
    inside[begin:end] = True
    assert set(before) == set(after) == set(whole), "the three snapshots hold different arrays"
    for k in before:
        b, a, w = (np.asarray(d[k]) for d in (before, after, whole))
        if not (b.shape == a.shape == w.shape and b.dtype == a.dtype == w.dtype):
            faults.append(f"{k}: shape or dtype changed")
            continue
        if k == RNG:
            assert b.size == RNG_HEADER_WORDS + E * N, "rng_state is 4 header words + one word per (replica, agent)"
            if not np.array_equal(a[:RNG_HEADER_WORDS], b[:RNG_HEADER_WORDS]):
                faults.append(f"{k}: header words changed")
            b, a, w = (v[RNG_HEADER_WORDS:] for v in (b, a, w))
        bb, ab, wb = _bits(b, E), _bits(a, E), _bits(w, E)
        touched = np.flatnonzero(~inside & (ab != bb).any(axis=1))
        if touched.size:
            faults.append(f"{k}: replicas {touched.tolist()} outside [{begin}, {end}) changed")
        wrong = np.flatnonzero(inside & (ab != wb).any(axis=1))
        if wrong.size and k not in run_dependent:
            faults.append(f"{k}: replicas {wrong.tolist()} inside [{begin}, {end}) differ from the whole-range launch")
    return faults


# ---------------------------------------------------------------------------------------------------------------------
# seeded shape sweeps (tests/test_gpu_tag_continuous.py)

def random_configuration(rng):
    """test_random_configurations' generator: agent counts around the wavefront / block boundaries, K from 1 to N - 1,
    both observation modes, both exit rules, all reward scalars, replica counts that do not fill a block.
    Returns (cfg, E); the order of the draws is part of the cases."""
    n_taggers = int(rng.randint(1, 7))
    n_runners = int(rng.choice([1, 2, 5, 30, 58, 59, 60, 63, 64, 65, 100, 123, 124, 127, 130]))
    N = n_taggers + n_runners
    full = bool(rng.randint(0, 2)) and N <= 70
    K = int(rng.randint(1, min(N - 1, 33) + 1)) if N > 2 else 1
    cfg = dict(num_taggers=n_taggers, num_runners=n_runners, grid_length=float(rng.choice([2.0, 7.5, 20.0])),
               episode_length=int(rng.randint(3, 12)), seed=int(rng.randint(1, 10 ** 6)),
               max_speed=float(rng.choice([0.5, 1.0, 2.5])), max_acceleration=0.25, min_acceleration=-0.25,
               max_turn=float(rng.choice([0.8, 2.356])), min_turn=-float(rng.choice([0.8, 2.356])),
               num_acceleration_levels=int(rng.randint(1, 9)), num_turn_levels=int(rng.randint(1, 9)),
               skill_level_runner=float(rng.choice([0.7, 1.0])), skill_level_tagger=float(rng.choice([0.9, 1.0, 1.3])),
               use_full_observation=full, num_other_agents_observed=K,
               tagging_distance=float(rng.choice([0.02, 0.3, 1.0])), tag_reward_for_tagger=float(rng.choice([1.0, 10.0])),
               tag_penalty_for_runner=-float(rng.choice([1.0, 10.0])), step_penalty_for_tagger=-float(rng.choice([0.0, 0.01])),
               step_reward_for_runner=float(rng.choice([0.0, 0.01])), edge_hit_penalty=-float(rng.choice([0.0, 0.5])),
               end_of_game_reward_for_runner=float(rng.choice([0.0, 1.0])),
               runner_exits_game_after_tagged=bool(rng.randint(0, 2)))
    return cfg, int(rng.choice([1, 2, 3, 7, 33]))


FUSED_SWEEP_CASES = 32
HEAD_SIZES = (2, 3, 5, 8, 13, 21, 23, 24, 25, 26, 32, 33, 48, 65, 71)
# coverage forced into fixed case numbers: overrides applied to the drawn case (taggers, runners, K, full, heads, E,
# exit rule); None = as drawn
_FORCED = {
    0: dict(num_taggers=1, num_runners=4, K=3, full=False, E=33),                     # epb 51: E < epb
    1: dict(num_taggers=4, num_runners=30, K=6, full=False, E=33, heads=(24, 25)),    # epb 7, 33 % 7 != 0; WD_SLAB_CH
    2: dict(num_taggers=4, num_runners=60, K=9, full=False, E=3),                     # N = 64
    3: dict(num_taggers=5, num_runners=60, K=10, full=False, E=7, heads=(25, 24)),    # N = 65: epb 3, 7 % 3 != 0
    4: dict(num_taggers=4, num_runners=124, K=12, full=False, E=3),                   # N = 128
    5: dict(num_taggers=6, num_runners=130, K=8, full=False, E=3, heads=(9, 5)),      # N = 136 > 128, larger head first
    6: dict(num_taggers=3, num_runners=31, K=4, full=True, E=7, heads=(5, 9)),        # full observations, epb 7
    7: dict(num_taggers=2, num_runners=30, K=5, full=False, E=2, heads=(71, 3)),      # a head above 64 entries
    8: dict(num_taggers=2, num_runners=58, K=7, full=False, E=3, exits=False),        # runners stay in the game
    9: dict(num_taggers=2, num_runners=58, K=7, full=False, E=3, exits=True),
    10: dict(num_taggers=5, num_runners=64, K=33, full=False, E=2, heads=(3, 65)),    # generic entry, K-pass selection
}


def fused_tick_sweep_case(case):
    """case -> (cfg, E, (n_acc, n_turn)): random_configuration plus the two head sizes, with the coverage conditions
    that tests/test_tick_range_cases_host.py lists forced into the first case numbers"""
    rng = np.random.RandomState(5000 + case)
    cfg, E = random_configuration(rng)
    heads = (int(rng.choice(HEAD_SIZES)), int(rng.choice(HEAD_SIZES)))
    f = _FORCED.get(case, {})
    for k in ("num_taggers", "num_runners"):
        cfg[k] = f.get(k, cfg[k])
    N = cfg["num_taggers"] + cfg["num_runners"]
    cfg["use_full_observation"] = f.get("full", cfg["use_full_observation"] and N <= 70)
    cfg["num_other_agents_observed"] = f.get("K", min(cfg["num_other_agents_observed"], max(N - 1, 1)))
    cfg["runner_exits_game_after_tagged"] = f.get("exits", cfg["runner_exits_game_after_tagged"])
    heads = f.get("heads", heads)
    E = f.get("E", E)
    if cfg["use_full_observation"] or N > 100:  # (rows of 7 * (N - 1) + 1 floats, the numpy oracle's [E, N, N] tables)
        E = min(E, 7)
    cfg["num_acceleration_levels"], cfg["num_turn_levels"] = heads[0] - 1, heads[1] - 1
    return cfg, E, heads


def sweep_case_has_tick_on_given_actions(case):
    """partial observations and K within the register-resident specialisations: the fast entry classes (TagContinuous.
    _fast_path), which have a TickA form"""
    cfg, _, _ = fused_tick_sweep_case(case)
    return not cfg["use_full_observation"] and 1 <= cfg["num_other_agents_observed"] <= 32


TICK_ON_GIVEN_ACTIONS_SWEEP = [c for c in range(FUSED_SWEEP_CASES) if sweep_case_has_tick_on_given_actions(c)]


def sweep_probabilities(rng, E, N, A):
    """[E, N, A] float32 Dirichlet rows; in every replica one agent row is one-hot and one has exact zeros in front of
    and behind its mass (the inverse CDF's end cases: the count of prefix sums below u must stop at the last entry
    with mass and must skip leading zeros).  With two actions the second kind is the one-hot row [0, 1]."""
    p = rng.dirichlet(np.ones(A), size=(E, N)).astype(np.float32)
    for e in range(E):
        i = (3 * e) % N
        p[e, i] = 0.0
        p[e, i, rng.randint(0, A)] = 1.0
        j = (3 * e + 1) % N
        if j != i:
            if A >= 3:
                row = p[e, j].astype(np.float64)
                row[0] = row[-1] = 0.0
                p[e, j] = (row / row.sum()).astype(np.float32)
            else:
                p[e, j] = np.array([0.0, 1.0], dtype=np.float32)
    return p
