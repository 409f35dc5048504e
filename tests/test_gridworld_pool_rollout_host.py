"""TagGridWorld with a reset pool, the one-launch rollout on the host: the code object of the five N5P entries, which env
shapes admit them, the launches `tick_launch` / `evaluate_launch` build (fakes for the managers, as
tests/test_gridworld_evaluate_host.py), the numpy model of the pooled T-tick launch against single oracle ticks, the sizing
of the GPU cases of tests/test_gpu_gridworld_pool_rollout.py from the model alone, the quotient table, the run config."""
import json
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

from oracle.core_np import pool_pick, sample_actions_counting, seed_words, single_head_tick_uniform
from oracle.tag_gridworld_np import TagGridWorldOracle
from tests import gridworld_pool_cases as gp

F32 = np.float32
ROLLOUT_KERNELS = ("HipTagGridWorldRollout_N5P", "HipTagGridWorldRollout_N5P_H32", "HipTagGridWorldRollout_N5P_H64")
EVALUATE_KERNELS = ("HipTagGridWorldEvaluate_N5P_H32", "HipTagGridWorldEvaluate_N5P_H64")
OBJECT = "wd_kernels_gw5_pool.hsaco"


def _manifest():
    from warp_drive_amd import build as wd_build

    wd_build.build_kernels_locked()
    return json.load(open(wd_build.MANIFEST))


def test_pool_kernels_in_their_own_code_object_without_scratch_or_spills():
    """the five entries are in wd_kernels_gw5_pool.hsaco (a key of build.UNITS with no extra flags); each has no private
    segment, no spilled VGPR and `.max_flat_workgroup_size` 64"""
    from warp_drive_amd import build as wd_build

    assert wd_build.UNITS[OBJECT] == ("tag_gridworld_n5_pool.hip", [])
    manifest = _manifest()
    for k in ROLLOUT_KERNELS + EVALUATE_KERNELS:
        assert manifest.get(k) == OBJECT, k
    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "x.elf")
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={os.path.join(wd_build.CSRC, OBJECT)}", f"--output={elf}"],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                               text=True).stdout
    found = {}
    for block in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        field = lambda key: re.search(r"\." + key + r":\s+(\S+)", block).group(1)   # noqa: E731
        found[field("name")] = (int(field("private_segment_fixed_size")), int(field("vgpr_spill_count")),
                                int(field("max_flat_workgroup_size")))
    assert set(found) == set(ROLLOUT_KERNELS + EVALUATE_KERNELS)
    for name in found:
        assert found[name] == (0, 0, 64), (name, found[name])


# ----------------------------------------------------------------------------------- fakes for the managers
class _FakeFn:
    def __init__(self, name):
        self.name = name


class _FakeFM:
    def __init__(self, manifest):
        self.manifest, self.initialized = manifest, []

    def initialize_functions(self, names):
        self.initialized += list(names)

    def has_function(self, name):
        return name in self.manifest

    def get_function(self, name):
        return _FakeFn(name)

    def global_address(self, name):
        return ("address of", name)


class _FakeDM:
    def __init__(self, E, reset_list=("observations",), pools=None, rows=(5, 5)):
        self.E, self.reset_data_list = E, list(reset_list)
        self.reset_target_to_pool = {"loc_x": "loc_x_reset_pool", "loc_y": "loc_y_reset_pool"} if pools is None else pools
        self.shapes = {"loc_x_reset_pool": (rows[0], 5), "loc_y_reset_pool": (rows[1], 5), "state_reset_pool": (rows[0], 5)}

    def meta_info(self, key):
        return {"n_envs": self.E}[key]

    def get_shape(self, name):
        return self.shapes[name]

    def device_data(self, name):
        return ("device", name)


class _FakeResetter:
    def __init__(self, initialised=True):
        self._pool_rng = "pool words" if initialised else None

    def fused_launch(self, dm, force, undo):
        return _FakeFn("reset_when_done_fused"), ("reset table", np.int32(len(dm.reset_data_list))), None, None


def _fake_pool_env(E, manifest, grid_length=100, episode_length=23, num_taggers=4, full=True, initialised=True, **dm_kw):
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorldWithResetPool

    env = CUDATagGridWorldWithResetPool(num_taggers=num_taggers, grid_length=grid_length, episode_length=episode_length,
                                        seed=5, use_full_observation=full)
    env.cuda_function_manager, env.cuda_data_manager = _FakeFM(manifest), _FakeDM(E, **dm_kw)
    env.cuda_env_resetter = _FakeResetter(initialised)
    env.cuda_step = _FakeFn("HipTagGridWorldStep")
    env.cuda_step_function_feed = lambda names: [("arg", n) for n in names]
    return env


def _tensor(shape, dtype, cuda=True, contiguous=True):
    n = int(np.prod(shape))
    return types.SimpleNamespace(is_cuda=cuda, is_contiguous=lambda: contiguous, dtype=dtype, shape=tuple(shape),
                                 numel=lambda: n)


def _up4(n):
    return -(-n // 4) * 4


def _lds_bytes(width, episode_length, n_pool, cache=105, rollout=True):
    """the issue's table restated: image 12 * 105, restore cache 12 * CD, 256 quotients, time table roundup4(T + 1), the
    two pools 2 * roundup4(5 * n_pool), the two packed policies; times 4 bytes, rounded up to 16.  The evaluation has
    neither cache nor pools."""
    policy = 2 * _up4(width * 24 + width + width * width + width + 5 * width + 5) if width else 0
    dwords = 12 * 105 + (12 * cache if rollout else 0) + 256 + _up4(episode_length + 1) + \
        (2 * _up4(5 * n_pool) if rollout else 0) + policy
    return -(-4 * dwords // 16) * 16


def test_which_shapes_admit_the_pool_rollout():
    manifest = _manifest()
    for L in (100, 255):
        env = _fake_pool_env(300, manifest, grid_length=L)
        for width in (16, 32, 48, 64, 128):
            for n_actions in (4, 5, 6):
                want = width in (32, 64) and n_actions == 5
                assert env.has_live_policy_rollout(width, n_actions) is want, (L, width, n_actions)
                assert env.has_live_policy_evaluate(width, n_actions) is want, (L, width, n_actions)
        assert env.has_pool_rollout(5) is True
    assert env.ROLLOUT_POLICY_OPT_IN is True and not getattr(env, "TICK_POOL_RESET", False)
    assert not _fake_pool_env(300, manifest, grid_length=256).has_live_policy_rollout(32, 5)
    assert not _fake_pool_env(300, manifest, grid_length=256).has_pool_rollout(5)
    assert not _fake_pool_env(300, manifest, episode_length=4096).has_live_policy_rollout(32, 5)
    assert _fake_pool_env(300, manifest, episode_length=4095).has_live_policy_rollout(64, 5) is True
    assert not _fake_pool_env(300, manifest, num_taggers=3).has_live_policy_rollout(32, 5)
    assert not _fake_pool_env(300, manifest, full=False).has_live_policy_rollout(32, 5)
    # loc_x also in the reset list; the reset list of CUDATagGridWorld
    assert not _fake_pool_env(300, manifest, reset_list=("observations", "loc_x")).has_live_policy_rollout(32, 5)
    assert not _fake_pool_env(300, manifest, reset_list=("loc_x", "loc_y", "observations")).has_live_policy_rollout(32, 5)
    # unequal pool sizes; another pooled array; one pool only
    assert not _fake_pool_env(300, manifest, rows=(5, 6)).has_live_policy_rollout(32, 5)
    assert not _fake_pool_env(300, manifest, pools={"loc_x": "loc_x_reset_pool", "state": "state_reset_pool"}).has_live_policy_rollout(32, 5)
    assert not _fake_pool_env(300, manifest, pools={"loc_x": "loc_x_reset_pool"}).has_live_policy_rollout(32, 5)
    # the pool generator not initialised
    assert not _fake_pool_env(300, manifest, initialised=False).has_live_policy_rollout(32, 5)
    # an entry missing from the manifest
    for missing, rollout32, eval32 in (("HipTagGridWorldRollout_N5P_H32", False, False), ("HipTagGridWorldEvaluate_N5P_H32", True, False)):
        env = _fake_pool_env(300, manifest)
        env.cuda_function_manager = _FakeFM({k: v for k, v in manifest.items() if k != missing})
        assert bool(env.has_live_policy_rollout(32, 5)) is rollout32 and bool(env.has_live_policy_evaluate(32, 5)) is eval32
        assert env.has_live_policy_rollout(64, 5) is True and env.has_live_policy_evaluate(64, 5) is True
    # LDS over the limit: the only admission limit on n_pool
    limit = _fake_pool_env(300, manifest).ROLLOUT_POLICY_MAX_LDS
    assert limit == 160 * 1024
    big = next(n for n in range(64, 10 ** 6, 64) if _lds_bytes(32, 23, n) > limit)
    assert _lds_bytes(32, 23, big - 64) <= limit
    env = _fake_pool_env(300, manifest, rows=(big, big))
    assert env.pool_rollout_lds_bytes(32) == _lds_bytes(32, 23, big) and not env.has_live_policy_rollout(32, 5)
    assert not env.has_live_policy_evaluate(32, 5)
    env = _fake_pool_env(300, manifest, rows=(big - 64, big - 64))
    assert env.has_live_policy_rollout(32, 5) is True and big > 1000


def test_the_env_without_a_pool_answers_as_before():
    """CUDATagGridWorld: the N5 entries, grid_length 63 admitted and 64 refused, its LDS sums"""
    from tests.test_gridworld_evaluate_host import _fake_managed, _lds_bytes as n5_eval_lds

    manifest = _manifest()
    assert _fake_managed(257, manifest, grid_length=63).has_live_policy_rollout(32, 5)
    assert not _fake_managed(257, manifest, grid_length=64).has_live_policy_rollout(32, 5)
    assert not _fake_managed(257, manifest, grid_length=100).has_live_policy_evaluate(32, 5)
    env = _fake_managed(257, manifest)
    assert not getattr(env, "ROLLOUT_POLICY_OPT_IN", False) and not getattr(env, "ROLLOUT_POOL_RESET", False)
    for width in (32, 64):
        assert env.live_policy_evaluate_lds_bytes(width) == n5_eval_lds(width, 23)
        assert env.live_policy_lds_bytes(width) == n5_eval_lds(width, 23) + 4 * 12 * (2 * 5 + 105)


# dynamic LDS bytes the three separate formulas of the host gave before they became `n5_lds_bytes`, computed with that
# version of envs/tag_gridworld.py.  Plain env, episode length -> width -> (live_policy_lds_bytes(w), (w, 0), (w, 105),
# live_policy_evaluate_lds_bytes(w)); "fixed": the shared bytes of the HipTagGridWorldRollout_N5 launch.  Episode lengths
# 1, 2 and 3 fill the same four-entry time table.
_SHORT_PLAIN = {0: (10896, 5376, 10416, 5376), 32: (27024, 21504, 26544, 21504), 64: (59536, 54016, 59056, 54016),
                "fixed": 10832}
PLAIN_LDS = {
    1: _SHORT_PLAIN, 2: _SHORT_PLAIN, 3: _SHORT_PLAIN,
    100: {0: (11296, 5776, 10816, 5776), 32: (27424, 21904, 26944, 21904), 64: (59936, 54416, 59456, 54416), "fixed": 11232},
    4095: {0: (27264, 21744, 26784, 21744), 32: (43392, 37872, 42912, 37872), 64: (75904, 70384, 75424, 70384),
           "fixed": 27200},
}
# env with a reset pool, (episode length, pool rows) -> width -> (pool_rollout_lds_bytes(w), (w, cache_dwords=0),
# (w, cache_dwords=115, n_pool=rows), (w, n_pool=0), live_policy_evaluate_lds_bytes(w), the inherited live_policy_lds_bytes(w))
_SHORT_POOLED = {
    1: {0: (11184, 6144, 11664, 11120, 6080, 10896), 32: (27376, 22336, 27856, 27312, 22272, 27024),
        64: (59888, 54848, 60368, 59824, 54784, 59536)},
    5: {0: (11344, 6304, 11824, 11120, 6080, 10896), 32: (27536, 22496, 28016, 27312, 22272, 27024),
        64: (60048, 55008, 60528, 59824, 54784, 59536)},
    7: {0: (11408, 6368, 11888, 11120, 6080, 10896), 32: (27600, 22560, 28080, 27312, 22272, 27024),
        64: (60112, 55072, 60592, 59824, 54784, 59536)},
}
POOLED_LDS = {
    **{(T, rows): _SHORT_POOLED[rows] for T in (1, 2, 3) for rows in (1, 5, 7)},
    (100, 1): {0: (11584, 6544, 12064, 11520, 6480, 11296), 32: (27776, 22736, 28256, 27712, 22672, 27424),
               64: (60288, 55248, 60768, 60224, 55184, 59936)},
    (100, 5): {0: (11744, 6704, 12224, 11520, 6480, 11296), 32: (27936, 22896, 28416, 27712, 22672, 27424),
               64: (60448, 55408, 60928, 60224, 55184, 59936)},
    (100, 7): {0: (11808, 6768, 12288, 11520, 6480, 11296), 32: (28000, 22960, 28480, 27712, 22672, 27424),
               64: (60512, 55472, 60992, 60224, 55184, 59936)},
    (4095, 1): {0: (27552, 22512, 28032, 27488, 22448, 27264), 32: (43744, 38704, 44224, 43680, 38640, 43392),
                64: (76256, 71216, 76736, 76192, 71152, 75904)},
    (4095, 5): {0: (27712, 22672, 28192, 27488, 22448, 27264), 32: (43904, 38864, 44384, 43680, 38640, 43392),
                64: (76416, 71376, 76896, 76192, 71152, 75904)},
    (4095, 7): {0: (27776, 22736, 28256, 27488, 22448, 27264), 32: (43968, 38928, 44448, 43680, 38640, 43392),
                64: (76480, 71440, 76960, 76192, 71152, 75904)},
}


def test_one_lds_formula_gives_the_bytes_of_the_three_it_replaces():
    """`n5_lds_bytes` (table entries, cache dwords, pool rows, width, time table rounded up or not) and the four callers
    that were formulas of their own reproduce the recorded numbers; both 5-agent units include the shared header"""
    from tests.test_gridworld_shapes_logic import _env, _tick_launch
    from warp_drive_amd import build as wd_build

    assert sorted(PLAIN_LDS) == [1, 2, 3, 100, 4095]
    assert sorted(POOLED_LDS) == [(T, rows) for T in (1, 2, 3, 100, 4095) for rows in (1, 5, 7)]
    for T, want in PLAIN_LDS.items():
        env = _env(5, True, episode_length=T)
        for w in (0, 32, 64):
            assert (env.live_policy_lds_bytes(w), env.live_policy_lds_bytes(w, 0), env.live_policy_lds_bytes(w, 105),
                    env.live_policy_evaluate_lds_bytes(w)) == want[w], (T, w)
            assert (env.n5_lds_bytes(64, 115, 0, w), env.n5_lds_bytes(64, 0, 0, w), env.n5_lds_bytes(64, 105, 0, w),
                    env.n5_lds_bytes(64, 0, 0, w)) == want[w], (T, w)
        assert _tick_launch(_env(5, True, episode_length=T), 1000, 4)[4] == want["fixed"], T
        assert env.n5_lds_bytes(64, 115, 0, None, round_time_table=False) == want["fixed"], T
    for (T, rows), want in POOLED_LDS.items():
        env = _fake_pool_env(300, {}, episode_length=T, rows=(rows, rows))
        for w in (0, 32, 64):
            assert (env.pool_rollout_lds_bytes(w), env.pool_rollout_lds_bytes(w, cache_dwords=0),
                    env.pool_rollout_lds_bytes(w, cache_dwords=115, n_pool=rows), env.pool_rollout_lds_bytes(w, n_pool=0),
                    env.live_policy_evaluate_lds_bytes(w), env.live_policy_lds_bytes(w)) == want[w], (T, rows, w)
            assert env.pool_rollout_lds_bytes(w, n_pool=rows) == env.pool_rollout_lds_bytes(w, 105, rows) == want[w][0]
            pw = w or None   # the fixed-probability N5P entry has no policies behind its tables
            assert (env.n5_lds_bytes(256, 105, rows, pw), env.n5_lds_bytes(256, 0, rows, pw),
                    env.n5_lds_bytes(256, 115, rows, pw), env.n5_lds_bytes(256, 105, 0, pw),
                    env.n5_lds_bytes(256, 0, 0, pw), env.n5_lds_bytes(64, 115, 0, w)) == want[w], (T, rows, w)
    header = os.path.join(wd_build.KDIR, "tag_gridworld_n5_common.h")
    for unit in ("tag_gridworld_n5.hip", "tag_gridworld_n5_pool.hip"):
        assert header in wd_build.unit_sources(unit) and os.path.exists(header), unit


@pytest.mark.parametrize("width", [0, 32, 64])
def test_tick_launch(width):
    """entry name; the N5 entry's arguments, then (for the live entries) the two policies, then the four pool arguments;
    block (64, 1, 1), grid ceil(E / 12); the LDS of the restated table"""
    import torch
    from warp_drive_amd.envs.tag_gridworld import gridworld_policy_floats
    from warp_drive_amd.managers.function_manager import _stream_tag
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    E, T, ep, rows = 70001, 9, 37, 7
    env = _fake_pool_env(E, _manifest(), episode_length=ep, rows=(rows, rows))
    env.ticks_per_launch = T
    sampler, resetter = types.SimpleNamespace(rng_state="rng"), env.cuda_env_resetter
    probs = _tensor((E, 5, 5), torch.float32)
    batch = {"obs": _tensor((T, E, 5, 21), torch.float32), "actions": _tensor((T + 1, E, 5, 1), torch.int32),
             "rewards": _tensor((T, E, 5), torch.float32), "done": _tensor((T, E), torch.int32)}
    step_args = env._step_args()
    assert len(step_args) == 16
    if width:
        n_w = gridworld_policy_floats(width)
        shared_policy = _tensor((n_w,), torch.float32)
        policy, pol_args = ((shared_policy, shared_policy), width), [shared_policy, shared_policy]
        name = f"HipTagGridWorldRollout_N5P_H{width}"
    else:
        policy, pol_args, name = None, [], "HipTagGridWorldRollout_N5P"
    fn, args, block, grid, shared = env.tick_launch(sampler, [probs], resetter, batch=batch, policy=policy)
    assert fn.name == name and name in env.cuda_function_manager.initialized
    assert (block, grid) == ((64, 1, 1), ((E + 11) // 12, 1))
    assert shared == _lds_bytes(width, ep, rows) == env.pool_rollout_lds_bytes(width) and shared % 16 == 0
    want = list(step_args) + ["rng", probs, np.int32(5), "reset table", np.int32(1), _stream_tag("tick"), np.int32(T),
                              batch["obs"], batch["actions"], batch["rewards"], batch["done"], np.int32(105),
                              ("address of", "kIndexToActionArr")] + pol_args + \
        ["pool words", ("device", "loc_x_reset_pool"), ("device", "loc_y_reset_pool"), np.int32(rows)]
    assert len(args) == len(want) == 16 + 13 + len(pol_args) + 4
    for i, (got, w) in enumerate(zip(args, want)):
        assert type(got) is type(w) and got == w, (i, got, w)
    assert args[-4:] == want[-4:]   # the four pool arguments are the last four
    # no fused single tick; no launch before init_reset_pool(); a malformed policy
    with pytest.raises(UnsupportedRolloutShape):
        env.tick_launch(sampler, [probs], resetter, policy=policy)
    env.ticks_per_launch = 1
    with pytest.raises(UnsupportedRolloutShape):
        env.tick_launch(sampler, [probs], resetter, batch=batch, policy=policy)
    env.ticks_per_launch = T
    cold = _fake_pool_env(E, _manifest(), episode_length=ep, initialised=False)
    cold.ticks_per_launch = T
    with pytest.raises(RuntimeError, match=r"call init_reset_pool\(\)"):
        cold.tick_launch(sampler, [probs], cold.cuda_env_resetter, batch=batch, policy=policy)
    if width:
        for bad in (((_tensor((n_w + 4,), torch.float32), shared_policy), width), ((shared_policy,), width),
                    ((shared_policy, shared_policy), 48), (shared_policy, shared_policy)):
            with pytest.raises(UnsupportedRolloutShape):
                env.tick_launch(sampler, [probs], resetter, batch=batch, policy=bad)
    far = _fake_pool_env(E, _manifest(), grid_length=256, episode_length=ep)
    far.ticks_per_launch = T
    with pytest.raises(UnsupportedRolloutShape):
        far.tick_launch(sampler, [probs], far.cuda_env_resetter, batch=batch, policy=policy)
    with pytest.raises(AssertionError):   # fewer batch rows than ticks
        env.tick_launch(sampler, [probs], resetter, batch=dict(batch, done=_tensor((T - 1, E), torch.int32)), policy=policy)


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("use_argmax", [True, False])
def test_evaluate_launch(width, use_argmax):
    """the Evaluate_N5P_H<width> entry: the N5 evaluation's 16 + 11 arguments, then the four pool arguments; no restore
    cache and no pools in its LDS"""
    import torch
    from warp_drive_amd.envs.tag_gridworld import gridworld_policy_floats
    from warp_drive_amd.managers.function_manager import _stream_tag
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    E, T = 70001, 37
    env = _fake_pool_env(E, _manifest(), episode_length=T, rows=(9, 9))
    sampler = types.SimpleNamespace(rng_state="rng")
    n_w = gridworld_policy_floats(width)
    tagger, runner = _tensor((n_w,), torch.float32), _tensor((n_w,), torch.float32)
    out = {"reward_sum": _tensor((E, 5), torch.float32), "steps": _tensor((E,), torch.int32), "done": _tensor((E,), torch.int32)}
    trace = _tensor((T, E, 5), torch.int32)
    for given_trace, ticks in ((None, None), (trace, T - 5)):
        fn, args, b, g, shared = env.evaluate_launch(sampler, policy=((tagger, runner), width), use_argmax=use_argmax,
                                                     outputs=out, action_trace=given_trace, ticks=ticks)
        assert fn.name == f"HipTagGridWorldEvaluate_N5P_H{width}" and fn.name in env.cuda_function_manager.initialized
        assert (b, g) == ((64, 1, 1), ((E + 11) // 12, 1))
        assert shared == _lds_bytes(width, T, 0, rollout=False) == env.live_policy_evaluate_lds_bytes(width)
        want = list(env._step_args()) + ["rng", _stream_tag("tick"), np.int32(T if ticks is None else ticks),
                                         ("address of", "kIndexToActionArr"), tagger, runner, np.int32(1 if use_argmax else 0),
                                         out["reward_sum"], out["steps"], out["done"],
                                         np.uint64(0) if given_trace is None else given_trace,
                                         "pool words", ("device", "loc_x_reset_pool"), ("device", "loc_y_reset_pool"), np.int32(9)]
        assert len(args) == len(want) == 16 + 11 + 4
        for i, (got, w) in enumerate(zip(args, want)):
            assert type(got) is type(w) and got == w, (i, got, w)
    with pytest.raises(UnsupportedRolloutShape):
        env.evaluate_launch(sampler, policy=((tagger, runner), 48), use_argmax=use_argmax, outputs=out)
    with pytest.raises(UnsupportedRolloutShape):
        _fake_pool_env(E, _manifest(), grid_length=256).evaluate_launch(sampler, policy=((tagger, runner), width),
                                                                        use_argmax=use_argmax, outputs=out)


# ------------------------------------------------------------------------------------------- the model and the cases
_MODELS = {}


def _modelled(case):
    """the fixed-probability launches of a case on the model alone -> (model, [rows of every launch])"""
    if case.name not in _MODELS:
        model = gp.PoolModel(case)
        rows = [model.launch(case.ticks, probs=case.probabilities()) for _ in range(case.launches)]
        _MODELS[case.name] = (model, rows)
    return _MODELS[case.name]


@pytest.mark.parametrize("case", [gp.SMALL_CASES[-1], gp.BOUNDARY_CASES[0], gp.POOL_SIZE_CASES[2], gp.TAG_CASE], ids=repr)
def test_the_model_of_a_launch_is_single_oracle_ticks_with_explicit_restarts(case):
    """T single ticks written out by hand -- the draw, TagGridWorldOracle.step, `pool_pick` on the words before the
    reset, reset_done_envs(x=, y=), words += done -- give the rows and the final arrays of the model's launches"""
    model, rows = _modelled(case)
    E = case.E
    orc = TagGridWorldOracle(num_envs=E, **case.config())
    pool_x, pool_y = case.pools()
    assert pool_x.shape == pool_y.shape == (case.n_pool, 5) and (pool_x[:, -1] == 0).all() and (pool_y[:, -1] == 0).all()
    assert pool_x.min() >= 0 and pool_x.max() <= max(case.L - 1, 1)
    words, pool_words = case.start_epochs().copy(), case.start_pool_epochs().copy()
    (lo, hi), (plo, phi) = seed_words(gp.SAMPLER_SEED), seed_words(gp.POOL_SEED)
    probs = case.probabilities()
    placeholder = orc.obs.astype(F32).copy()
    tick = 0
    for launch in range(case.launches):
        for k in range(case.ticks):
            np.testing.assert_array_equal(rows[launch]["obs"][k], orc.obs.astype(F32))
            u = single_head_tick_uniform(E * 5, words, lo, hi, gp.TICK_TAG).reshape(E, 5)
            a = sample_actions_counting(probs, u)
            words = (words + np.uint32(1)).astype(np.uint32)
            orc.step(a)
            np.testing.assert_array_equal(rows[launch]["actions"][k], a)
            np.testing.assert_array_equal(rows[launch]["rewards"][k], orc.rewards.astype(F32))
            np.testing.assert_array_equal(rows[launch]["done"][k], orc.done)
            fin = orc.done > 0
            last_done = orc.done.copy()
            pick = pool_pick(np.arange(E), pool_words, plo, phi, case.n_pool)
            orc.reset_done_envs(x=pool_x[pick], y=pool_y[pick])
            pool_words = (pool_words + fin.astype(np.uint32)).astype(np.uint32)
            # a restarted replica: the pool row's cells, the START positions' observation rows, time step 0
            np.testing.assert_array_equal(orc.loc_x[fin], pool_x[pick][fin])
            np.testing.assert_array_equal(orc.obs.astype(F32)[fin], placeholder[fin])
            assert (orc.timestep[fin] == 0).all()
            tick += 1
    st = model.state()
    np.testing.assert_array_equal(st["loc_x"], orc.loc_x)
    np.testing.assert_array_equal(st["loc_y"], orc.loc_y)
    np.testing.assert_array_equal(st["obs"], orc.obs.astype(F32))
    np.testing.assert_array_equal(st["timestep"], orc.timestep)
    np.testing.assert_array_equal(st["done"], last_done)
    np.testing.assert_array_equal(st["epochs"], words)
    np.testing.assert_array_equal(st["pool_epochs"], pool_words)
    assert tick == case.ticks * case.launches


@pytest.mark.parametrize("case", gp.FIXED_CASES, ids=repr)
def test_gpu_case_is_not_vacuous_on_the_model(case):
    """what the GPU test demands, from the model alone: at least 2 * E restarts, every replica restarted, every pool row
    drawn (2 / 5 / 7 rows), pool words advanced by the restarts; boundary starts stand on coordinate L; the tag case
    restarts from tags, mid-episode"""
    model, rows = _modelled(case)
    print(f"{case.name}: {int(model.restarts.sum())} restarts of {case.E} replicas ({model.tags} tags, {model.timeouts} "
          f"time-outs), pool rows {sorted(model.rows_drawn)} of {case.n_pool}, largest coordinate {model.max_coord}")
    assert gp.coverage_ok(case, model)
    assert sum(int(r["done"].sum()) for r in rows) == int(model.restarts.sum())
    if case is gp.TAG_CASE:
        assert model.tags >= 2 * case.E and model.tags > 4 * model.timeouts
    if case.E in (1, 11, 12, 13, 25):   # one partial group, one lane group, a full group, 2 / 3 trips of a grid of one block
        assert -(-case.E // gp.EPB) == {1: 1, 11: 1, 12: 1, 13: 2, 25: 3}[case.E]
    probs = case.probabilities()
    assert np.abs(probs - 0.2).max() > 0.3 and len({p.tobytes() for p in probs.reshape(-1, 5)}) == probs.shape[0] * 5


@pytest.mark.parametrize("case", gp.EVAL_CASES, ids=repr)
def test_evaluation_case_is_not_vacuous_on_the_host(case):
    """the evaluation cases replayed on the host alone: every replica finishes; from E = 13 on there are tags, time-outs,
    wall hits and an agent on coordinate 100; no decision sits inside the 2e-6 window, so the cap is all headroom for
    the device; greedy cases use at least three actions"""
    from tests import gridworld_evaluate as gev

    r = gev.replay(case)
    assert (r["done"] == 1).all() and r["near"] == 0 and r["followed"] == 0
    assert case.L == 100 and -(-case.E // gp.EPB) == {1: 1, 13: 2, 25: 3}[case.E]
    if case.E >= 13:
        assert gp.eval_coverage_ok(case, r), (int(r["tagged"].sum()), int(r["timed_out"].sum()), r["wall_hits"], r["max_coord"])
        share = r["counts"] / r["counts"].sum()
        assert (np.sort(share)[-3] >= 0.05) if case.greedy else (share.min() >= 0.02), share


@pytest.mark.parametrize("L", [100, 255])
def test_quotient_table(L):
    """table[c] == float32(c) / float32(L) for every c: the kernel's `(float)c / (float)L` with the correctly rounded
    division is the float32 of the oracle's float64 quotient of the two integers"""
    c = np.arange(L + 1)
    table = (c.astype(F32) / F32(L)).astype(F32)
    np.testing.assert_array_equal(table, (c / L).astype(F32))   # (exact integers: one rounding either way)
    orc = TagGridWorldOracle(num_envs=1, num_taggers=4, grid_length=L, episode_length=5,
                             starting_location_x=np.array([L, L - 1, 1, 0, L // 2]), starting_location_y=np.zeros(5))
    np.testing.assert_array_equal(orc.obs.astype(F32)[0, 0, :5], table[[L, L - 1, 1, 0, L // 2]])
    assert table[L] == 1.0 and L <= 255


def test_the_run_config():
    import yaml
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorldWithResetPool
    from warp_drive_amd.training.scripts import train

    assert train._ENVS["tag_gridworld_with_reset_pool"] is CUDATagGridWorldWithResetPool
    config = yaml.safe_load(open(os.path.join(train._CONFIGS, "tag_gridworld_with_reset_pool.yaml")))
    assert config["name"] == "tag_gridworld_with_reset_pool"
    env = train._ENVS["tag_gridworld_with_reset_pool"](**dict(config["env"]))   # (setup_trainer's construction)
    assert (env.num_agents, env.grid_length, env.episode_length) == (5, 100, 100)
    assert (env.wall_hit_penalty, env.tag_reward_for_tagger, env.tag_penalty_for_runner, env.step_cost_for_tagger) == \
        (0.1, 10.0, 5.0, 0.01)
    assert config["env"]["seed"] == 20
    assert train.policy_map_for("tag_gridworld_with_reset_pool", env) == {"shared": [0, 1, 2, 3, 4]}
    assert (config["trainer"]["num_envs"], config["trainer"]["train_batch_size"]) == (2000, 200000)
    assert list(config["policy"]) == ["shared"]
    p = config["policy"]["shared"]
    assert (p["algorithm"], p["model"]["fc_dims"], p["gamma"], p["lr"], p["entropy_coeff"], p["vf_loss_coeff"]) == \
        ("A2C", [32, 32], 0.98, 0.001, 0.05, 1)
    assert p["clip_grad_norm"] is True and p["max_grad_norm"] == 3
    assert not [k for k in config["trainer"] if k.startswith("fused")]   # shipped configs keep the per-tick path
