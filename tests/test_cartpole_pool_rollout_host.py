"""Cartpole with a reset pool, the one-launch rollout on the host: the code object of the three ..._P entries, the LDS
formula, which env shapes admit them and why the others do not, the launches `tick_launch` builds (fakes for the managers,
as tests/test_gridworld_pool_rollout_host.py) -- with a pool the new entries and the pool arguments, without one today's
argument list --, the run config, and every GPU case of tests/test_gpu_cartpole_pool_rollout.py sized from the numpy model
alone."""
import json
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import cartpole_pool_cases as cp
from tests import classic_control_cases as cc

F32 = np.float32
KERNELS = tuple(cp.ENTRY.values())


def _manifest():
    from warp_drive_amd import build as wd_build

    wd_build.build_kernels_locked()
    return json.load(open(wd_build.MANIFEST))


def test_pool_kernels_in_their_own_code_object_without_scratch_or_spills():
    """the three entries are in wd_kernels_cp_pool.hsaco (a key of build.UNITS with no extra flags); none has a private
    segment or a spilled VGPR; the live-policy entries keep the unpooled ones' block of 256; both Cartpole units include
    the shared header"""
    from warp_drive_amd import build as wd_build

    assert wd_build.UNITS[cp.OBJECT] == ("cartpole_pool.hip", [])
    manifest = _manifest()
    for k in KERNELS:
        assert manifest.get(k) == cp.OBJECT, k
    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "x.elf")
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={os.path.join(wd_build.CSRC, cp.OBJECT)}", f"--output={elf}"],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                               text=True).stdout
    found = {}
    for block in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
        field = lambda key: re.search(r"\." + key + r":\s+(\S+)", block).group(1)   # noqa: E731
        found[field("name")] = (int(field("private_segment_fixed_size")), int(field("vgpr_spill_count")),
                                int(field("max_flat_workgroup_size")), int(field("group_segment_fixed_size")))
    assert set(found) == set(KERNELS)
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv as Env

    for name, (private, spills, block, static_lds) in found.items():
        assert private == 0 and spills == 0, (name, private, spills)
        assert static_lds == Env.POOL_ROLLOUT_STATIC_LDS, (name, static_lds)
        assert block == (1024 if name.endswith("_P") else 256), (name, block)
    header = os.path.join(wd_build.KDIR, "cartpole_common.h")
    for unit in ("wd_kernels.hip", "cartpole_pool.hip"):
        assert header in wd_build.unit_sources(unit) and os.path.exists(header), unit


def test_lds_formula():
    """the packed policy rounded up to whole float4, then 16 bytes per staged pool row"""
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv as Env

    f = Env.pool_rollout_lds_bytes
    assert f(0, 2, 1000, True) == 16000 and f(0, 2, 1000, False) == 0 and f(0, 8, 7, True) == 112
    # [32, 32] with 2 actions: 128 + 32 + 1024 + 32 + 64 + 2 = 1282 floats -> 1284; [64, 64]: 4610 -> 4612
    assert f(32, 2, 0, False) == 5136 and f(64, 2, 0, False) == 18448
    assert f(32, 2, 1000, True) == 5136 + 16000 and f(64, 2, 1000, True) == 18448 + 16000
    assert f(64, 8, 1000, True) == 4 * 5000 + 16000 and f(64, 8, 1000, False) == 20000   # 5000 floats: whole float4
    assert f(32, 3, 7, True) == 4 * 1316 + 112 and f(32, 1, 16, True) == 4 * 1252 + 256    # 1315 -> 1316, 1249 -> 1252
    assert f(64, 2, 10000, True) == 18448 + 160000 > Env.POOL_ROLLOUT_MAX_LDS == 64 * 1024


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


class _FakeDM:
    def __init__(self, E, reset_list=("observations",), pools=None, rows=1000, pool_shape=None, pool_dtype="float32"):
        self.E, self.reset_data_list = E, list(reset_list)
        self.reset_target_to_pool = {"state": "state_reset_pool"} if pools is None else pools
        self.shapes = {"state_reset_pool": (rows, 1, 4) if pool_shape is None else pool_shape, "other_reset_pool": (rows, 1)}
        self.pool_dtype = pool_dtype

    def meta_info(self, key):
        return {"n_envs": self.E}[key]

    def get_shape(self, name):
        return self.shapes[name]

    def get_dtype(self, name):
        return self.pool_dtype

    def device_data(self, name):
        return ("device", name)


class _FakeResetter:
    def __init__(self, initialised=True):
        self._pool_rng = "pool words" if initialised else None

    def fused_launch(self, dm, force, undo):
        return _FakeFn("reset_when_done_fused"), ("reset table", np.int32(len(dm.reset_data_list))), None, None


def _fake_env(E, manifest, pool=1000, initialised=True, **dm_kw):
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv

    env = CUDAClassicControlCartPoleEnv(episode_length=37, seed=5, reset_pool_size=pool)
    if pool:
        dm = _FakeDM(E, rows=pool, **dm_kw)
    else:
        dm = _FakeDM(E, reset_list=("state", "observations"), pools={}, **dm_kw)
    env.cuda_function_manager, env.cuda_data_manager = _FakeFM(manifest), dm
    env.cuda_env_resetter = _FakeResetter(initialised)
    env.cuda_step = _FakeFn("HipClassicControlCartPoleEnvStep")
    env.cuda_step_function_feed = lambda names: [("arg", n) for n in names]
    env._inv_div_ok = 1   # (the division proof is one launch per env object: not on the host)
    return env


def _tensor(shape, dtype, cuda=True, contiguous=True):
    n = int(np.prod(shape))
    return types.SimpleNamespace(is_cuda=cuda, is_contiguous=lambda: contiguous, dtype=dtype, shape=tuple(shape),
                                 numel=lambda: n)


def _n_w(width, A):
    return 4 * width + width + width * width + width + A * width + A if width else 0


def _launch_inputs(E, T, A, width):
    import torch

    probs = _tensor((E, 1, A), torch.float32)
    batch = {"obs": _tensor((T, E, 1, 4), torch.float32), "actions": _tensor((T + 1, E, 1, 1), torch.int32),
             "rewards": _tensor((T, E, 1), torch.float32), "done": _tensor((T, E), torch.int32)}
    packed = _tensor((_n_w(width, A),), torch.float32) if width else None
    return probs, batch, packed


@pytest.mark.parametrize("width", [0, 32, 64])
@pytest.mark.parametrize("A", [2, 8])
def test_tick_launch_with_a_pool(width, A):
    """entry name; the unpooled entry's arguments, then the pool generator's words, the pool, its row count and the
    placement flag; the host's block and grid; the LDS of the formula"""
    from warp_drive_amd.managers.function_manager import _stream_tag
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    E, T, rows = 70001, 9, 1000
    env = _fake_env(E, _manifest(), pool=rows)
    env.ticks_per_launch = T
    sampler, resetter = types.SimpleNamespace(rng_state="rng"), env.cuda_env_resetter
    probs, batch, packed = _launch_inputs(E, T, A, width)
    policy = (packed, width) if width else None
    pol_args = [packed, np.int32(width)] if width else [np.uint64(0), np.int32(0)]
    assert env.ROLLOUT_POOL_RESET is True and env.ROLLOUT_POLICY_OPT_IN is True
    assert not getattr(env, "TICK_POOL_RESET", False)   # the single tick of a pooled Cartpole stays the unfused plan
    assert env.has_pool_rollout(A) and (not width or env.has_live_policy_rollout(width, A))
    for placement, staged in (("auto", True), ("lds", True), ("global", False)):
        env.pool_placement = placement
        fn, args, block, grid, shared = env.tick_launch(sampler, [probs], resetter, batch=batch, policy=policy)
        assert fn.name == cp.ENTRY[width] and fn.name in env.cuda_function_manager.initialized
        assert (block, grid) == ((256, 1, 1), ((E + 255) // 256, 1))
        assert shared == env.pool_rollout_lds_bytes(width, A, rows, staged) == \
            4 * (-(-_n_w(width, A) // 4) * 4) + (16 * rows if staged else 0)
        want = [("arg", n) for n in env._STEP_ARGS] + \
            ["rng", probs, np.int32(A), "reset table", np.int32(1), _stream_tag("tick"), np.int32(T),
             batch["obs"], batch["actions"], batch["rewards"], batch["done"]] + pol_args + \
            [np.int32(1), "pool words", ("device", "state_reset_pool"), np.int32(rows), np.int32(1 if staged else 0)]
        assert len(args) == len(want) == 17 + 14 + 4
        for i, (got, w) in enumerate(zip(args, want)):
            assert type(got) is type(w) and got == w, (i, got, w)
    # a pool that does not fit the LDS: "auto" reads it from global memory, a forced "lds" is refused with the reason
    big = _fake_env(E, _manifest(), pool=10000)
    big.ticks_per_launch = T
    fn, args, _, _, shared = big.tick_launch(sampler, [probs], big.cuda_env_resetter, batch=batch, policy=policy)
    assert int(args[-1]) == 0 and int(args[-2]) == 10000 and shared == big.pool_rollout_lds_bytes(width, A, 10000, False)
    big.pool_placement = "lds"
    with pytest.raises(UnsupportedRolloutShape, match="bytes of LDS"):
        big.tick_launch(sampler, [probs], big.cuda_env_resetter, batch=batch, policy=policy)
    assert not big.has_pool_rollout(A) and not big.has_live_policy_rollout(32, A)
    # no fused single tick
    env.pool_placement = "auto"
    with pytest.raises(UnsupportedRolloutShape, match="no fused single tick"):
        env.tick_launch(sampler, [probs], resetter, policy=policy)
    env.ticks_per_launch = 1
    with pytest.raises(UnsupportedRolloutShape, match="no fused single tick"):
        env.tick_launch(sampler, [probs], resetter, batch=batch, policy=policy)
    env.ticks_per_launch = T
    with pytest.raises(AssertionError):   # fewer batch rows than ticks
        env.tick_launch(sampler, [probs], resetter, batch=dict(batch, done=_tensor((T - 1, E), "x")), policy=policy)


@pytest.mark.parametrize("width", [0, 32, 64])
def test_tick_launch_without_a_pool_builds_what_it_built_before(width):
    """the unpooled env: HipClassicControlCartPoleEnvTick / ...Rollout_H<width>, the 17 + 14 arguments restated here as
    literals, no pool argument, the shared bytes of the packed policy alone"""
    from warp_drive_amd.managers.function_manager import _stream_tag

    E, T, A = 70001, 9, 2
    env = _fake_env(E, _manifest(), pool=0)
    assert env.ROLLOUT_POOL_RESET is False and env.ROLLOUT_POLICY_OPT_IN is False and not env.has_pool_rollout()
    assert env.has_live_policy_rollout(32, 2) and env.has_live_policy_rollout(64, 8) and not env.has_live_policy_rollout(48, 2)
    env.ticks_per_launch = T
    sampler, resetter = types.SimpleNamespace(rng_state="rng"), env.cuda_env_resetter
    probs, batch, packed = _launch_inputs(E, T, A, width)
    for given in (batch, None):
        fn, args, block, grid, shared = env.tick_launch(sampler, [probs], resetter, batch=given,
                                                        policy=(packed, width) if width else None)
        assert fn.name == (f"HipClassicControlCartPoleEnvRollout_H{width}" if width else "HipClassicControlCartPoleEnvTick")
        assert (block, grid, shared) == ((256, 1, 1), ((E + 255) // 256, 1), 4 * _n_w(width, A))
        null = np.uint64(0)
        want = [("arg", n) for n in ["state", "sampled_actions", "_done_", "rewards", "observations", "gravity", "masspole",
                                     "total_mass", "length", "polemass_length", "force_mag", "tau",
                                     "theta_threshold_radians", "x_threshold", "_timestep_", ("episode_length", "meta"),
                                     ("n_envs", "meta")]] + \
            ["rng", probs, np.int32(A), "reset table", np.int32(2), _stream_tag("tick"), np.int32(T)] + \
            ([batch["obs"], batch["actions"], batch["rewards"], batch["done"]] if given else [null] * 4) + \
            ([packed, np.int32(width)] if width else [null, np.int32(0)]) + [np.int32(1)]
        assert len(args) == len(want) == 31
        for i, (got, w) in enumerate(zip(args, want)):
            assert type(got) is type(w) and got == w, (i, got, w)
    if width:   # a packed policy of another size, or of the right size and not float32: the caller's bug
        import torch

        for bad in (_tensor((_n_w(width, A) + 1,), torch.float32), _tensor((_n_w(width, A),), torch.float64)):
            with pytest.raises(AssertionError):
                env.tick_launch(sampler, [probs], resetter, batch=batch, policy=(bad, width))


def test_refusals_name_their_reason():
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    E, T = 300, 9
    manifest = _manifest()
    sampler = types.SimpleNamespace(rng_state="rng")

    def refused(env, width, A, reason):
        env.ticks_per_launch = T
        probs, batch, packed = _launch_inputs(E, T, A, width)
        assert not env.has_live_policy_rollout(width, A) and (width or not env.has_pool_rollout(A))
        with pytest.raises(UnsupportedRolloutShape, match=reason):
            env.tick_launch(sampler, [probs], env.cuda_env_resetter, batch=batch, policy=(packed, width) if width else None)

    for width in (0, 32):
        refused(_fake_env(E, manifest, initialised=False), width, 2, "pool generator is not initialised")
        refused(_fake_env(E, manifest, pools={"state": "state_reset_pool", "other": "other_reset_pool"}), width, 2,
                "restarts `state` from its pool and nothing else")
        refused(_fake_env(E, manifest, pools={"other": "other_reset_pool"}), width, 2, "restarts `state` from its pool")
        refused(_fake_env(E, manifest, reset_list=("observations", "restored_flag")), width, 2,
                "restores the observations and nothing else")
        refused(_fake_env(E, manifest, reset_list=("state", "observations")), width, 2,
                "restores the observations and nothing else")
        refused(_fake_env(E, manifest, pool_shape=(1000, 4)), width, 2, r"must be \[n, 1, 4\]")
        refused(_fake_env(E, manifest, pool_shape=(1000, 1, 2)), width, 2, r"must be \[n, 1, 4\]")
        refused(_fake_env(E, manifest, pool_dtype="float64"), width, 2, "must be float32")
        refused(_fake_env(E, manifest), width, 9, "1 .. 8 actions, not 9")
        refused(_fake_env(E, manifest), width, 0, "1 .. 8 actions, not 0")
    refused(_fake_env(E, manifest), 48, 2, "no in-kernel policy of width 48")
    # an entry missing from the manifest
    for width in (0, 32, 64):
        env = _fake_env(E, manifest)
        env.cuda_function_manager = _FakeFM({k: v for k, v in manifest.items() if k != cp.ENTRY[width]})
        refused(env, width, 2, "is not in the kernel manifest")
        for other in (0, 32, 64):
            if other != width:
                assert env.has_live_policy_rollout(other, 2) if other else env.has_pool_rollout(2)
    # a packed policy of another size
    env = _fake_env(E, manifest)
    env.ticks_per_launch = T
    probs, batch, packed = _launch_inputs(E, T, 2, 32)
    _, _, wrong = _launch_inputs(E, T, 3, 32)
    import torch

    for bad in (wrong, _tensor((_n_w(32, 2),), torch.float64)):   # ... or of the right size and not float32
        with pytest.raises(UnsupportedRolloutShape, match="packed policy"):
            env.tick_launch(sampler, [probs], env.cuda_env_resetter, batch=batch, policy=(bad, 32))
    # the evaluation never restarts: its answer does not depend on the pool
    assert env.has_live_policy_evaluate(32, 2) and env.has_live_policy_evaluate(64, 8)


def test_the_run_configs():
    import yaml
    from warp_drive_amd.envs.cartpole import CUDAClassicControlCartPoleEnv
    from warp_drive_amd.training.scripts import train

    assert train._ENVS["single_cartpole_with_reset_pool"] is CUDAClassicControlCartPoleEnv
    pooled = yaml.safe_load(open(os.path.join(train._CONFIGS, "single_cartpole_with_reset_pool.yaml")))
    plain = yaml.safe_load(open(os.path.join(train._CONFIGS, "single_cartpole.yaml")))
    assert pooled["name"] == "single_cartpole_with_reset_pool" and pooled["env"]["reset_pool_size"] == 1000
    assert plain["name"] == "single_cartpole" and plain["env"]["reset_pool_size"] == 0
    # the shipped config with the pool and its own name, nothing else
    for cfg in (pooled, plain):
        cfg.pop("name"), cfg["env"].pop("reset_pool_size"), cfg["saving"].pop("name")
    assert pooled == plain
    env = train._ENVS["single_cartpole_with_reset_pool"](**dict(yaml.safe_load(open(os.path.join(
        train._CONFIGS, "single_cartpole_with_reset_pool.yaml")))["env"]))
    assert env.reset_pool_size == 1000 and env.ROLLOUT_POLICY_OPT_IN is True and env.ROLLOUT_POOL_RESET is True
    assert train.policy_map_for("single_cartpole_with_reset_pool", env) == {"shared": [0]}
    assert not [k for k in pooled["trainer"] if k.startswith("fused")]   # shipped configs keep the per-tick path
    feed = env.get_reset_pool_dictionary()
    assert np.asarray(feed["state_reset_pool"]["data"]).shape == (1000, 1, 4)


# ------------------------------------------------------------------------------------------- the model and the cases
_MODELS = {}


def _modelled(case):
    if case.name not in _MODELS:
        model, choice = cp.PoolModel(case), cp.HostChoice(case)
        rows = [model.launch(choice) for _ in range(case.launches)]
        _MODELS[case.name] = (model, choice, rows)
    return _MODELS[case.name]


def test_the_case_list():
    """E = 1501 with 11-tick launches over 4-tick episodes, 11 or 14 batch rows; pools of 2, 7 and 16 rows; 1, 2, 3 and 8
    actions; E = 1, 63, 65; 30-tick episodes; the crafted pool and its ordinary twin -- for every entry"""
    for H in cp.HIDDEN:
        cases = [c for c in cp.CASES if c.hidden == H]
        assert len(cases) == 12 and all(c.env == "cartpole" and c.pool >= 2 and c.launches == 3 and c.ticks == 11 for c in cases)
        assert {c.A for c in cases} == {1, 2, 3, 8} and {c.pool for c in cases} == {2, 7, 9, 16}
        assert {c.E for c in cases} == {1, 63, 65, 1501} and {c.rows for c in cases} == {11, 14}
        assert {c.T for c in cases} == {4, 30} and all(c.epochs == "residue" for c in cases)
        assert sum(c.crafted for c in cases) == 1
    assert len({c.name for c in cp.CASES}) == len(cp.CASES)
    # (the grid of 3 blocks of 128 threads takes its three trips at E = 1501)
    assert cc.geometry(1501, (128, 3))[2] >= 3 and cc.geometry(65, (128, 3)) is None


@pytest.mark.parametrize("case", cp.CASES, ids=repr)
def test_gpu_case_is_not_vacuous_on_the_model(case):
    """the host replay alone (oracle/cartpole_np.py, oracle.core_np.pool_pick, single_head_tick_uniform and
    tests/classic_control_policy.py): restarts on several ticks of every launch, every pool row drawn, every action's
    share, both generators across 2^32, the draws near a threshold within the cap"""
    model, choice, rows = _modelled(case)
    E = case.E
    shares = model.actions / model.actions.sum()
    print(f"{case.name}: {int(model.restarts.sum())} restarts ({model.terminal} terminal) on ticks {model.restart_ticks}, "
          f"pool rows {sorted(model.rows_drawn)} of {case.pool}, action shares {np.round(shares, 3).tolist()}, "
          f"{model.wrapped} / {model.pool_wrapped} replicas cross 2^32 (sampler / pool), {choice.near} near draws "
          f"(cap {case.near_cap()}), {model.crafted_survivors} restarts from a crafted row survive a tick")
    assert int(model.restarts.sum()) >= E
    assert sum(int(r["done"].sum()) for r in rows) == int(model.restarts.sum())
    np.testing.assert_array_equal(model.pool_epochs - case.start_pool_epochs(), model.restarts.astype(np.uint32))
    np.testing.assert_array_equal(model.epochs - case.start_epochs(), np.uint32(case.ticks * case.launches))
    assert choice.near <= case.near_cap()
    assert case.A == 1 or case.hidden == 0 or case.near_cap() == 2 * (case.A - 1)
    if E >= 63:
        assert all(len(t) >= 3 for t in model.restart_ticks), model.restart_ticks
        assert model.rows_drawn == set(range(case.pool))
        assert (shares >= case.share).all(), shares
        assert model.wrapped >= 16                    # WRAP_ROWS, in the one launch that starts at 0xfffffffd
        if case.T == 4:
            assert model.pool_wrapped >= 16           # ... and their pool words after three restarts
    if case.T == 30:   # in every launch some replicas finish and some do not
        assert all(0 < int(f.sum()) < E for f in model.finished_in_launch)
    if case.has_one_draw():   # the draw of exactly 1.0 on a row whose sums stay below it: the clamp
        assert rows[0]["actions"][case.one_draw_tick(), cc.ONE_DRAW[0]] == case.A - 1
    if case.crafted:
        assert model.crafted_survivors >= 10
        # no launch of this case may run the fast ticks, and every pool row of the others allows them
        assert (np.abs(case.pool_rows()[:, 2]) > 0.75).sum() == 4
    else:
        assert (np.abs(case.pool_rows()[:, 2]) <= 0.05).all()


def test_crafted_rows_tell_the_fast_tick_from_the_general_one():
    """CRAFTED_ROWS[3:] survive one step (theta back inside the threshold), and the velocities after that step depend on
    sin / cos of 1.0: the small-angle polynomials of the fast tick give other bits than numpy's float32 kernels there, so
    a launch that ran fast ticks on this pool would record other observation rows"""
    from oracle.cartpole_np import CartPoleOracle

    rows = cp.CRAFTED_ROWS
    for a in (0, 1):
        orc = CartPoleOracle(len(rows), 500)
        orc.state = rows.copy()
        orc.step(np.full(len(rows), a))
        assert orc.done.tolist() == [1, 1, 1, 0, 0]
        assert (np.abs(orc.state[3:, 2]) < 0.2).all()
    s, c = cp.sincos_small(rows[3:, 2])
    assert (s.view(np.int32) != np.sin(rows[3:, 2]).view(np.int32)).any() or \
        (c.view(np.int32) != np.cos(rows[3:, 2]).view(np.int32)).any()
    # ... while inside +-0.75 they are numpy's, bit for bit
    x = np.linspace(-0.75, 0.75, 20001).astype(F32)
    s, c = cp.sincos_small(x)
    np.testing.assert_array_equal(s.view(np.int32), np.sin(x).view(np.int32))
    np.testing.assert_array_equal(c.view(np.int32), np.cos(x).view(np.int32))
