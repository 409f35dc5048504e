"""Trainer.evaluate_episodes on the host: the code object of the six HipClassicControl<X>EnvEvaluate_H<width> entries, which
env classes admit them, the launch `evaluate_launch` builds (fakes for the managers, as
tests/test_classic_control_policy_host.py), the sizing of the GPU cases of tests/test_gpu_evaluate.py from the host replay
alone, and the numpy model of HipEvaluateAccumulate on its crafted done patterns."""
import json
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import classic_control_cases as cc
from tests import classic_control_evaluate as ev

EVALUATE_KERNELS = {f"HipClassicControl{x}EnvEvaluate_H{h}": obj
                    for x, obj in (("CartPole", "wd_kernels.hsaco"), ("Acrobot", "wd_kernels_cc.hsaco"),
                                   ("MountainCar", "wd_kernels_cc.hsaco")) for h in (32, 64)}


def _manifest():
    from warp_drive_amd import build as wd_build

    wd_build.build_kernels_locked()
    return json.load(open(wd_build.MANIFEST))


def test_evaluate_kernels_in_the_code_objects_without_scratch_or_spills():
    """the six entries and HipEvaluateAccumulate are in the manifest; the six have no private segment, no spilled VGPR
    and `.max_flat_workgroup_size` 256"""
    from warp_drive_amd import build as wd_build

    manifest = _manifest()
    for k, obj in EVALUATE_KERNELS.items():
        assert manifest.get(k) == obj, k
    assert manifest.get("HipEvaluateAccumulate") == "wd_kernels.hsaco"
    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    found = {}
    for obj in sorted(set(EVALUATE_KERNELS.values())):
        with tempfile.TemporaryDirectory() as tmp:
            elf = os.path.join(tmp, "x.elf")
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--input={os.path.join(wd_build.CSRC, obj)}", f"--output={elf}"],
                           check=True, capture_output=True)
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                                   text=True).stdout
        for block in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
            field = lambda key: re.search(r"\." + key + r":\s+(\S+)", block).group(1)   # noqa: E731
            if field("name") in EVALUATE_KERNELS:
                found[field("name")] = (int(field("private_segment_fixed_size")), int(field("vgpr_spill_count")),
                                        int(field("max_flat_workgroup_size")))
    assert set(found) == set(EVALUATE_KERNELS)
    for name, (private, spills, size) in found.items():
        assert private == 0 and spills == 0 and size == 256, (name, private, spills, size)


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
    reset_target_to_pool = {}

    def __init__(self, E, O):
        self.E, self.O = E, O

    def meta_info(self, key):
        return {"n_envs": self.E}[key]

    def get_shape(self, name):
        return {"observations": (self.E, 1, self.O)}[name]


def _classes():
    from warp_drive_amd.envs import cartpole as cp
    from warp_drive_amd.envs import classic_control as ccl

    return {"cartpole": (cp.CUDAClassicControlCartPoleEnv, 4, "CartPole"),
            "acrobot": (ccl.CUDAClassicControlAcrobotEnv, 6, "Acrobot"),
            "mountain_car": (ccl.CUDAClassicControlMountainCarEnv, 2, "MountainCar"),
            "continuous_mountain_car": (ccl.CUDAClassicControlContinuousMountainCarEnv, 2, "ContinuousMountainCar"),
            "pendulum": (ccl.CUDAClassicControlPendulumEnv, 3, "Pendulum")}


def _fake_managed(env_name, E, manifest, episode_length=20):
    cls, O, x = _classes()[env_name]
    env = cls(episode_length=episode_length, seed=5)
    env.cuda_function_manager, env.cuda_data_manager = _FakeFM(manifest), _FakeDM(E, O)
    env.cuda_step = _FakeFn(f"HipClassicControl{x}EnvStep")
    env.cuda_step_function_feed = lambda names: [("arg", n) for n in names]
    return env


def _tensor(shape, dtype, cuda=True, contiguous=True):
    n = int(np.prod(shape))
    return types.SimpleNamespace(is_cuda=cuda, is_contiguous=lambda: contiguous, dtype=dtype, shape=tuple(shape),
                                 numel=lambda: n)


def test_which_envs_admit_an_in_kernel_evaluation():
    """true exactly for (Cartpole | Acrobot | MountainCar) x {32, 64} x 1 .. 8 actions with the entry in the manifest"""
    manifest = _manifest()
    for name in _classes():
        discrete = name in ev.ENVS
        env = _fake_managed(name, 1000, manifest)
        for width in (8, 16, 31, 32, 33, 48, 64, 128, 256):
            for n_actions in (0, 1, 2, 3, 8, 9, 21):
                want = discrete and width in (32, 64) and 1 <= n_actions <= 8
                assert env.has_live_policy_evaluate(width, n_actions) is want, (name, width, n_actions)
        # ... and only while the code object has the entry
        env.cuda_function_manager = _FakeFM({k: v for k, v in manifest.items() if "Evaluate_H32" not in k})
        assert not env.has_live_policy_evaluate(32, 2) and env.has_live_policy_evaluate(64, 2) is discrete


@pytest.mark.parametrize("env_name", ev.ENVS)
@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("use_argmax", [True, False])
def test_evaluate_launch(env_name, width, use_argmax):
    """the Evaluate_H<width> entry; the step's arguments followed by (rng, n_actions, tag, ticks, packed, width,
    use_argmax, the three outputs, the trace or null); the step's block and grid; 4 n_w bytes of LDS.  The malformed
    policies `tick_launch` refuses are UnsupportedRolloutShape here too."""
    import torch
    from tests.classic_control_policy import policy_weight_count
    from warp_drive_amd.managers.function_manager import _stream_tag
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    E, T = 70001, 37
    _, O, x = _classes()[env_name]
    A = ev.N_ACTIONS[env_name]
    env = _fake_managed(env_name, E, _manifest(), episode_length=T)
    sampler = types.SimpleNamespace(rng_state="rng")
    n_w = policy_weight_count(O, width, A)
    packed = _tensor((n_w,), torch.float32)
    out = {"reward_sum": _tensor((E + 3,), torch.float32), "steps": _tensor((E + 3,), torch.int32),
           "done": _tensor((E + 3,), torch.int32)}
    trace = _tensor((T + 2, E), torch.int32)
    step_fn, step_args, block, grid, _ = env.step_launch()
    for given_trace, ticks in ((None, None), (trace, T - 5), (trace, T + 2)):
        fn, args, b, g, shared = env.evaluate_launch(sampler, policy=(packed, width), use_argmax=use_argmax, outputs=out,
                                                     action_trace=given_trace, ticks=ticks)
        assert fn.name == f"HipClassicControl{x}EnvEvaluate_H{width}" and fn.name in env.cuda_function_manager.initialized
        assert (b, g) == (block, grid) == ((256, 1, 1), (min(4096, (E + 255) // 256), 1)) and shared == 4 * n_w <= 65536
        want = list(step_args) + ["rng", np.int32(A), _stream_tag("tick"), np.int32(T if ticks is None else ticks), packed,
                                  np.int32(width), np.int32(1 if use_argmax else 0), out["reward_sum"], out["steps"],
                                  out["done"], np.uint64(0) if given_trace is None else given_trace]
        assert len(args) == len(want)
        for i, (got, w) in enumerate(zip(args, want)):
            assert type(got) is type(w) and got == w, (i, got, w)
    bad = [(_tensor((n_w + 1,), torch.float32), width), (_tensor((n_w,), torch.float64), width),
           (_tensor((n_w,), torch.float32, cuda=False), width), (_tensor((n_w,), torch.float32, contiguous=False), width),
           (packed, 48), (packed, 96 - width), packed]
    for policy in bad:
        with pytest.raises(UnsupportedRolloutShape):
            env.evaluate_launch(sampler, policy=policy, use_argmax=use_argmax, outputs=out)
    with pytest.raises(UnsupportedRolloutShape):  # nine actions do not fit the kernel's registers
        env.evaluate_launch(sampler, policy=(_tensor((policy_weight_count(O, width, 9),), torch.float32), width),
                            use_argmax=use_argmax, outputs=out, n_actions=9)
    with pytest.raises(AssertionError):  # a trace with fewer rows than ticks
        env.evaluate_launch(sampler, policy=(packed, width), use_argmax=use_argmax, outputs=out,
                            action_trace=_tensor((T - 1, E), torch.int32))


@pytest.mark.parametrize("env_name", ["continuous_mountain_car", "pendulum"])
def test_box_envs_refuse_an_evaluation_launch(env_name):
    import torch
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    env = _fake_managed(env_name, 1000, _manifest())
    with pytest.raises(UnsupportedRolloutShape):
        env.evaluate_launch(types.SimpleNamespace(rng_state="rng"), policy=(_tensor((100,), torch.float32), 32),
                            use_argmax=True, outputs={})


# ------------------------------------------------------------------------------------------- sizing of the GPU cases
@pytest.mark.parametrize("case", ev.PARITY_CASES + ev.RESIDUE_CASES, ids=repr)
def test_gpu_case_is_not_vacuous_on_the_host(case):
    """the GPU case replayed on the host alone (numpy step, restated network, Philox replay): replicas end by termination
    on at least three different ticks, some by time-out, MountainCar's crafted goal rows with done 2, every action has a
    share of at least 0.02, and the near-tie decisions stay under the cap (2 + decisions // 50000) * (A - 1)"""
    assert case.T <= 60 and case.E == 1501 and cc.geometry(case.E, (128, 3))[2] >= 3
    r = ev.replay(case)
    share = r["counts"] / r["counts"].sum()
    print(f"{case.name}: terminations on {len(r['end_ticks'])} ticks, {r['timeouts']} time-outs, done values "
          f"{np.unique(r['done']).tolist()}, action shares {np.round(share, 3).tolist()}, {r['near']} of {r['decisions']} "
          f"decisions near a tie (cap {case.near_cap(r['decisions'])})")
    assert len(r["end_ticks"]) >= 3 and r["timeouts"] > 0
    assert (r["done"] > 0).all() and (r["steps"] >= 1).all() and (r["steps"] <= case.T).all()
    assert len(np.unique(r["steps"])) >= 4
    assert (share >= 0.02).all(), share
    assert r["near"] <= case.near_cap(r["decisions"]) and r["followed"] == 0
    if case.env == "mountain_car":
        labels = [row[3] for row in cc.crafted_step_rows("mountain_car", case.T)]
        assert r["done"][labels.index("goal")] == 2 and r["steps"][labels.index("goal")] == 1
        assert r["done"][labels.index("goal_on_last_tick")] == 1   # the time-out wins
        assert (r["done"] == 2).sum() >= 50
    if case.env == "cartpole":
        np.testing.assert_array_equal(r["reward_sum"], r["steps"].astype(np.float32))
    if case.timesteps == "residue":
        zero = ev.replay(ev.EvalCase(case.env, case.hidden, case.mode))
        rows = np.arange(case.E) % 4
        timed_out = (r["steps"] + rows == case.T) & (r["done"] == 1)
        assert timed_out[rows > 0].sum() >= 20 and (r["steps"] <= zero["steps"]).all()
    if not case.greedy:
        np.testing.assert_array_equal(r["epochs"], case.start_epochs() + r["steps"].astype(np.uint32))
        assert (case.start_epochs()[cc.WRAP_ROWS].astype(np.uint64) + r["steps"][cc.WRAP_ROWS] > 1 << 32).any()


@pytest.mark.parametrize("case", [c for c in ev.PARITY_CASES if c.hidden == 32], ids=repr)
def test_fewer_ticks_than_an_episode_leave_replicas_unfinished(case):
    """`ticks = episode_length - 5`: some replicas are unfinished (done 0, steps == ticks), the finished ones are the
    full run's; `ticks = episode_length + 7` is the full run"""
    full, short, long = ev.replay(case), ev.replay(case, ticks=case.T - 5), ev.replay(case, ticks=case.T + 7)
    unfinished = short["done"] == 0
    assert 20 <= unfinished.sum() < case.E and (short["steps"][unfinished] == case.T - 5).all()
    for key in ("reward_sum", "steps", "done"):
        np.testing.assert_array_equal(short[key][~unfinished], full[key][~unfinished])
        np.testing.assert_array_equal(long[key], full[key])


def test_first_maximum_and_near_tie_helpers():
    p = np.array([[0.2, 0.5, 0.3], [0.4, 0.4, 0.2], [0.1, 0.45, 0.45], [0.5, 0.5 - 1e-6, 1e-6]], np.float32)
    np.testing.assert_array_equal(ev.first_maximum(p), [1, 0, 1, 0])
    np.testing.assert_array_equal(ev.near_top_two(p), [False, True, True, True])
    np.testing.assert_array_equal(ev.first_maximum(p), np.argmax(p, axis=1))


# -------------------------------------------------------------------------------------------- HipEvaluateAccumulate
@pytest.mark.parametrize("N", ev.ACC_AGENTS)
def test_accumulate_model_on_the_crafted_done_patterns(N):
    """the numpy model of HipEvaluateAccumulate: done on tick 0, never done, done twice (the second episode does not
    count), done value 2, done on the last tick -- against sums written out by hand"""
    rewards, done = ev.accumulate_inputs(N)
    total, end = ev.accumulate_model(rewards, done)
    ticks = ev.ACC_TICKS
    np.testing.assert_array_equal(end[:5], [0, -1, 3, 5, ticks - 1])

    def by_hand(env, last):
        acc = np.zeros(N, np.float32)
        for k in range(last + 1):
            acc = (acc + rewards[k, env]).astype(np.float32)
        return acc

    for env, last in ((0, 0), (1, ticks - 1), (2, 3), (3, 5), (4, ticks - 1)):
        np.testing.assert_array_equal(total[env], by_hand(env, last))
    first = np.array([np.flatnonzero(done[:, e])[0] if done[:, e].any() else -1 for e in range(ev.ACC_E)])
    np.testing.assert_array_equal(end, first)
    assert (end >= 0).sum() > ev.ACC_E // 2 and (end < 0).sum() >= 1 and len(np.unique(end)) >= 6
    # a replica that is done twice: the ticks after its first end add nothing
    assert done[:, 2].sum() == 2 and not np.array_equal(total[2], by_hand(2, 7))


def test_train_script_offers_evaluate():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "warp_drive_amd", "training", "scripts", "train.py")).read()
    assert '"--evaluate"' in text and "evaluate_episodes(use_argmax=" in text
