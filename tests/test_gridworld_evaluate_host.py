"""TagGridWorld's one-launch evaluation on the host: the code object of HipTagGridWorldEvaluate_N5_H<32|64>, which env
shapes admit them, the launch `evaluate_launch` builds (fakes for the managers, as
tests/test_classic_control_evaluate_host.py), and the sizing of the GPU cases of tests/test_gpu_gridworld_evaluate.py from
the host replay alone."""
import json
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import gridworld_evaluate as gev

EVALUATE_KERNELS = ("HipTagGridWorldEvaluate_N5_H32", "HipTagGridWorldEvaluate_N5_H64")
ROLLOUT_KERNELS = ("HipTagGridWorldRollout_N5", "HipTagGridWorldRollout_N5_H32", "HipTagGridWorldRollout_N5_H64")
OBJECT = "wd_kernels_gw5.hsaco"


def _manifest():
    from warp_drive_amd import build as wd_build

    wd_build.build_kernels_locked()
    return json.load(open(wd_build.MANIFEST))


def test_evaluate_kernels_in_the_code_object_without_scratch_or_spills():
    """the two entries are in wd_kernels_gw5.hsaco next to the three rollout entries; they have no private segment, no
    spilled VGPR and `.max_flat_workgroup_size` 64"""
    from warp_drive_amd import build as wd_build

    manifest = _manifest()
    for k in EVALUATE_KERNELS + ROLLOUT_KERNELS:
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
    assert set(found) == set(EVALUATE_KERNELS + ROLLOUT_KERNELS)
    for name in EVALUATE_KERNELS:
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
    def __init__(self, E, reset_list=("loc_x", "loc_y", "observations")):
        self.E, self.reset_data_list = E, list(reset_list)

    def meta_info(self, key):
        return {"n_envs": self.E}[key]


def _fake_managed(E, manifest, num_taggers=4, grid_length=10, episode_length=23, full=True):
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorld

    env = CUDATagGridWorld(num_taggers=num_taggers, grid_length=grid_length, episode_length=episode_length, seed=5,
                           use_full_observation=full)
    env.cuda_function_manager, env.cuda_data_manager = _FakeFM(manifest), _FakeDM(E)
    env.cuda_step = _FakeFn("HipTagGridWorldStep")
    env.cuda_step_function_feed = lambda names: [("arg", n) for n in names]
    return env


def _tensor(shape, dtype, cuda=True, contiguous=True):
    n = int(np.prod(shape))
    return types.SimpleNamespace(is_cuda=cuda, is_contiguous=lambda: contiguous, dtype=dtype, shape=tuple(shape),
                                 numel=lambda: n)


def _lds_bytes(width, episode_length):
    """the layout of gw5_evaluate restated: the image [12][5][21], s_div [64], s_tn [episode_length + 1] rounded up to
    four floats, two packed policies of W0 [H][24], b0 [H], W1 [H][H], b1 [H], Wp [5][H], bp [5] rounded up to four floats"""
    H = width
    policy = -(-(H * 24 + H + H * H + H + 5 * H + 5) // 4) * 4
    return 4 * (12 * 5 * 21 + 64 + -(-(episode_length + 1) // 4) * 4 + 2 * policy)


def test_which_shapes_admit_the_in_kernel_evaluation():
    """true exactly for 5 agents x full observations x 5 actions x width in {32, 64} with grid_length <= 63, the LDS within
    the limit and the entry in the manifest"""
    manifest = _manifest()
    env = _fake_managed(257, manifest)
    assert env.EVALUATE_POLICY_OPT_IN is True
    for width in (8, 16, 31, 32, 33, 48, 64, 128, 256):
        for n_actions in (0, 4, 5, 6, 8):
            want = width in (32, 64) and n_actions == 5
            assert env.has_live_policy_evaluate(width, n_actions) is want, (width, n_actions)
            assert env.has_live_policy_evaluate(width, n_actions) is bool(env.has_live_policy_rollout(width, n_actions))
    for taggers in (3, 5):   # 4 and 6 agents
        assert not _fake_managed(257, manifest, num_taggers=taggers).has_live_policy_evaluate(32, 5)
    assert not _fake_managed(257, manifest, full=False).has_live_policy_evaluate(32, 5)
    assert _fake_managed(257, manifest, grid_length=63).has_live_policy_evaluate(64, 5) is True
    assert not _fake_managed(257, manifest, grid_length=64).has_live_policy_evaluate(32, 5)
    # the time table grows with the episode length: 4095 ticks fit, an episode that pushes H = 64 over the limit does not
    assert _fake_managed(257, manifest, episode_length=4095).has_live_policy_evaluate(64, 5) is True
    limit = env.ROLLOUT_POLICY_MAX_LDS
    too_long = next(T for T in range(4096, 10 ** 6, 512) if _lds_bytes(64, T) > limit)
    long_env = _fake_managed(257, manifest, episode_length=too_long)
    assert long_env.live_policy_evaluate_lds_bytes(64) == _lds_bytes(64, too_long) > limit >= _lds_bytes(64, too_long - 512)
    assert not long_env.has_live_policy_evaluate(64, 5)
    # ... and only while the code object has the entry
    env.cuda_function_manager = _FakeFM({k: v for k, v in manifest.items() if k != "HipTagGridWorldEvaluate_N5_H32"})
    assert not env.has_live_policy_evaluate(32, 5) and env.has_live_policy_evaluate(64, 5) is True
    assert env.has_live_policy_rollout(32, 5)
    # a reset pool (other reset arrays than the rollout kernel restores): no live-policy rollout, so no evaluation either
    env = _fake_managed(257, manifest)
    env.cuda_data_manager = _FakeDM(257, reset_list=("observations",))
    assert not env.has_live_policy_evaluate(32, 5)


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("use_argmax", [True, False])
def test_evaluate_launch(width, use_argmax):
    """the Evaluate_N5_H<width> entry; the step's arguments (the four reward scalars as float64) followed by (rng, tag,
    ticks, the action table's address, tagger, runner, use_argmax, the three outputs, the trace or null); blocks of one
    wavefront on a grid of ceil(E / 12); the LDS of the restated layout.  The malformed policies `tick_launch` refuses
    are UnsupportedRolloutShape here too."""
    import torch
    from warp_drive_amd.envs.tag_gridworld import gridworld_policy_floats
    from warp_drive_amd.managers.function_manager import _stream_tag
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    E, T = 70001, 37
    env = _fake_managed(E, _manifest(), episode_length=T)
    sampler = types.SimpleNamespace(rng_state="rng")
    n_w = gridworld_policy_floats(width)
    assert n_w == -(-(width * 24 + width + width * width + width + 5 * width + 5) // 4) * 4
    tagger, runner = _tensor((n_w,), torch.float32), _tensor((n_w,), torch.float32)
    out = {"reward_sum": _tensor((E + 3, 5), torch.float32), "steps": _tensor((E + 3,), torch.int32),
           "done": _tensor((E + 3,), torch.int32)}
    flat_out = dict(out, reward_sum=_tensor((E * 5,), torch.float32))
    trace = _tensor((T + 2, E, 5), torch.int32)
    step_args = env._step_args()
    assert len(step_args) == 16 and [type(a) for a in step_args[6:10]] == [np.float64] * 4
    for given_trace, ticks, outputs in ((None, None, out), (trace, T - 5, flat_out), (trace, T + 2, out)):
        fn, args, b, g, shared = env.evaluate_launch(sampler, policy=((tagger, runner), width), use_argmax=use_argmax,
                                                     outputs=outputs, action_trace=given_trace, ticks=ticks)
        assert fn.name == f"HipTagGridWorldEvaluate_N5_H{width}" and fn.name in env.cuda_function_manager.initialized
        assert (b, g) == ((64, 1, 1), ((E + 11) // 12, 1))
        assert shared == _lds_bytes(width, T) == env.live_policy_evaluate_lds_bytes(width) and shared % 16 == 0
        assert shared <= 64 * 1024 and shared == env.live_policy_lds_bytes(width) - 4 * 12 * (2 * 5 + 5 * 21)
        want = list(step_args) + ["rng", _stream_tag("tick"), np.int32(T if ticks is None else ticks),
                                  ("address of", "kIndexToActionArr"), tagger, runner, np.int32(1 if use_argmax else 0),
                                  outputs["reward_sum"], outputs["steps"], outputs["done"],
                                  np.uint64(0) if given_trace is None else given_trace]
        assert len(args) == len(want) == 16 + 11
        for i, (got, w) in enumerate(zip(args, want)):
            assert type(got) is type(w) and got == w, (i, got, w)
    pair = (tagger, runner)
    bad = [((_tensor((n_w + 4,), torch.float32), runner), width), ((tagger, _tensor((n_w,), torch.float64)), width),
           ((_tensor((n_w,), torch.float32, cuda=False), runner), width),
           ((tagger, _tensor((n_w,), torch.float32, contiguous=False)), width),
           (pair, 48), (pair, 96 - width), (pair, 16), (pair, 128), pair, (tagger, width), ((tagger,), width)]
    for policy in bad:
        with pytest.raises(UnsupportedRolloutShape):
            env.evaluate_launch(sampler, policy=policy, use_argmax=use_argmax, outputs=out)
    for other in (_fake_managed(E, _manifest(), num_taggers=3), _fake_managed(E, _manifest(), full=False),
                  _fake_managed(E, _manifest(), grid_length=64)):
        with pytest.raises(UnsupportedRolloutShape):
            other.evaluate_launch(sampler, policy=(pair, width), use_argmax=use_argmax, outputs=out)
    with pytest.raises(AssertionError):  # a trace with fewer rows than ticks
        env.evaluate_launch(sampler, policy=(pair, width), use_argmax=use_argmax, outputs=out,
                            action_trace=_tensor((T - 1, E, 5), torch.int32))
    with pytest.raises(AssertionError):  # one reward sum per replica instead of one per agent
        env.evaluate_launch(sampler, policy=(pair, width), use_argmax=use_argmax,
                            outputs=dict(out, reward_sum=_tensor((E,), torch.float32)))


# ------------------------------------------------------------------------------------------- sizing of the GPU cases
def test_an_evaluation_from_the_reset_state_is_one_trajectory():
    """why the cases write per-replica start states: from the state `reset_all_envs()` leaves, a greedy evaluation is one
    trajectory repeated E times"""
    case = gev.GwCase(32, "greedy", E=25)
    orc = gev.TagGridWorldOracle(num_envs=case.E, **case.env_config())
    packed = case.policies()[1]
    for _ in range(case.T):
        orc.step(gev.first_maximum(gev.probabilities(packed, case.hidden, orc.obs.astype(np.float32))))
        assert (orc.loc_x == orc.loc_x[0]).all() and (orc.loc_y == orc.loc_y[0]).all() and len(np.unique(orc.done)) == 1


_REPLAYS = {}


def _replay(case, ticks=None):
    key = (case.name, ticks)
    if key not in _REPLAYS:
        _REPLAYS[key] = gev.replay(case, ticks=ticks)
    return _REPLAYS[key]


@pytest.mark.parametrize("case", gev.PARITY_CASES, ids=repr)
def test_gpu_case_is_not_vacuous_on_the_host(case):
    """the GPU case replayed on the host alone (oracle step, restated networks, Philox replay): finished replicas end on
    at least 8 distinct ticks; at least one group of 12 holds replicas tagged on different ticks and one that times out;
    tags, time-outs and wall hits occur; sampled: every action's share is at least 0.02; greedy: at least three actions
    have a share of at least 0.05; the decisions within 2e-6 of a threshold or tie stay at or under 2 + decisions //
    50000"""
    assert case.E == 257 and case.T <= 30 and -(-case.E // (3 * gev.EPB)) == 8   # the 3-block grid takes 8 trips
    r = _replay(case)
    ok, fig = gev.vacuity(case, r)
    print(f"{case.name} (policy seed {gev.POLICY_SEED[case.hidden, case.L, case.mode]}): {fig}")
    share = r["counts"] / r["counts"].sum()
    fin = r["end_tick"] >= 0
    assert fin.all() and (r["done"] == 1).all() and (r["steps"] >= 1).all() and (r["steps"] <= case.T).all()
    assert len(np.unique(r["end_tick"][fin])) >= 8
    assert fig["mixed groups"] >= 1
    assert r["tagged"].sum() > 0 and r["timed_out"].sum() > 0 and (r["tagged"] ^ r["timed_out"]).all()
    assert r["wall_hits"] > 0
    if case.greedy:
        assert (share >= 0.05).sum() >= 3, share
    else:
        assert (share >= 0.02).all(), share
    assert r["near"] <= case.near_cap(r["decisions"]) and r["followed"] == 0
    assert r["near"] == int((r["margins"] < gev.NEAR_WINDOW).sum()) and len(r["margins"]) == r["decisions"]
    assert ok
    # a time-out arrives row % 4 ticks sooner; steps count the ticks a replica ran
    rows = np.arange(case.E) % 4
    np.testing.assert_array_equal(r["steps"][r["timed_out"]], case.T - rows[r["timed_out"]])
    np.testing.assert_array_equal(r["steps"], r["end_tick"] + 1)
    np.testing.assert_array_equal((r["actions"] >= 0).all(axis=2).sum(axis=0), r["steps"])
    if case.greedy:
        np.testing.assert_array_equal(r["epochs"], case.start_epochs())
    else:
        np.testing.assert_array_equal(r["epochs"], case.start_epochs() + r["steps"].astype(np.uint32)[:, None])
        wrapped = case.start_epochs()[gev.WRAP_ROWS].astype(np.uint64) + r["steps"][gev.WRAP_ROWS, None]
        assert (wrapped >= 1 << 32).any() and (case.start_epochs()[gev.WRAP_ROWS] == 0xFFFFFFFD).all()
        assert case.start_epochs()[gev.WRAP_ROWS].shape == (16, 5)


@pytest.mark.parametrize("case", gev.SMALL_CASES + gev.BOUND_CASES, ids=repr)
def test_small_and_bound_cases_on_the_host(case):
    """E = 1 and E = 13 finish; grid_length = 63: live agents stand on coordinate 63 after a move, walk into walls, and
    time out"""
    r = _replay(case)
    assert (r["done"] == 1).all() and r["followed"] == 0 and r["near"] <= case.near_cap(r["decisions"])
    if case.L == 63:
        assert gev.reaches_bound(case, r) and case.E == 257
    else:
        assert case.E in (1, 13) and -(-case.E // gev.EPB) == (1 if case.E == 1 else 2)


@pytest.mark.parametrize("case", [c for c in gev.PARITY_CASES if c.hidden == 32 and c.L == 10], ids=repr)
def test_fewer_ticks_than_an_episode_leave_replicas_unfinished(case):
    """`ticks = episode_length - 5`: some replicas are unfinished (done 0, steps == ticks), the finished ones are the
    full run's; `ticks = episode_length + 7` is the full run"""
    full, short, long = _replay(case), gev.replay(case, ticks=case.T - 5), gev.replay(case, ticks=case.T + 7)
    unfinished = short["done"] == 0
    assert 20 <= unfinished.sum() < case.E and (short["steps"][unfinished] == case.T - 5).all()
    assert (full["steps"][unfinished] > case.T - 5).all()
    for key in ("reward_sum", "steps", "done"):
        np.testing.assert_array_equal(short[key][~unfinished], full[key][~unfinished])
        np.testing.assert_array_equal(long[key], full[key])
    np.testing.assert_array_equal(long["actions"][: case.T], full["actions"])
    assert (long["actions"][case.T:] == -1).all()


def test_replay_refuses_a_changed_trace_and_sums_in_float32():
    """the replay that follows a trace accepts the host's own and refuses one with a changed action; the reward sum is
    the float32 running sum in tick order"""
    case = gev.GwCase(32, "sampled", E=13)
    r = _replay(case)
    again = gev.replay(case, trace=r["actions"])
    for key in ("reward_sum", "steps", "done", "actions", "epochs"):
        np.testing.assert_array_equal(again[key], r[key])
    wrong = r["actions"].copy()
    wrong[0, 3, 2] = (wrong[0, 3, 2] + 1) % 5
    with pytest.raises(AssertionError):
        gev.replay(case, trace=wrong)
    # by hand for one replica
    orc, e = case.oracle(), 5
    acc = np.zeros(5, np.float32)
    for k in range(int(r["steps"][e])):
        _, rew, _ = orc.step(np.where(r["actions"][k] >= 0, r["actions"][k], 0))
        acc = (acc + rew[e].astype(np.float32)).astype(np.float32)
    np.testing.assert_array_equal(acc, r["reward_sum"][e])


def test_first_maximum_is_argmax_with_the_first_of_equals():
    p = np.array([[0.2, 0.5, 0.1, 0.1, 0.1], [0.3, 0.3, 0.2, 0.1, 0.1], [0.1, 0.1, 0.1, 0.35, 0.35]], np.float32)
    np.testing.assert_array_equal(gev.first_maximum(p), [1, 0, 3])
    np.testing.assert_array_equal(gev.first_maximum(p), np.argmax(p, axis=1))

