"""One-launch evaluation of the Box envs (DDPG), on the host: the code object of the four
HipClassicControl<Pendulum|ContinuousMountainCar>EnvEvaluate_A<32|64> entries, which env classes admit them, the launch
`evaluate_actor_launch` builds (the fake managers of tests/test_classic_control_policy_host.py), what it refuses, the
sizing of the GPU test's cases on the host replay of tests/classic_control_actor_evaluate.py, and TrainerDDPG's choice
of the evaluation path and its evaluator metrics on an object assembled by hand."""
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

from tests import classic_control_actor as ca
from tests import classic_control_actor_evaluate as ae
from tests import classic_control_cases as cc
from tests.test_classic_control_policy_host import _FakeFM, _classes, _fake_managed, _manifest, _tensor

KERNELS = {f"{ca.ENTRY[env]}Evaluate_A{h}": env for env in ae.ENVS for h in ae.WIDTHS}
# rng_state, stream_tag, ticks, actor, hidden, action_scale, action_bias, ou_state, damping, stddev, scale,
# eval_reward_sum, eval_steps, eval_done, mean_trace, action_trace
N_TAIL = 16
# state, action, done, reward, observation, (the env's constants,) timestep, episode_length, n_envs
N_STEP_ARGS = {"pendulum": 8, "continuous_mountain_car": 16}


def _code_object_metadata():
    """{kernel: (workgroup, private segment, VGPR spills, VGPRs, SGPRs, SGPR spills, static LDS, explicit arguments)} of
    wd_kernels_cc.hsaco"""
    from warp_drive_amd import build as wd_build

    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "cc.elf")
        subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--input={os.path.join(wd_build.CSRC, 'wd_kernels_cc.hsaco')}", f"--output={elf}"],
                       check=True, capture_output=True)
        notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                               text=True).stdout
    out = {}
    for block in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        name = re.search(r"^\s{4}\.name:\s+(\S+)$", block, re.M)
        if name is None:
            continue
        field = lambda key: int(re.search(r"^\s{4}\." + key + r":\s+(\d+)$", block, re.M).group(1))
        out[name.group(1)] = (field("max_flat_workgroup_size"), field("private_segment_fixed_size"),
                              field("vgpr_spill_count"), field("vgpr_count"), field("sgpr_count"),
                              field("sgpr_spill_count"), field("group_segment_fixed_size"),
                              len(re.findall(r"\.value_kind:\s+(?:by_value|global_buffer)\s", block)))
    return out


def test_evaluate_actor_kernels_in_the_code_object_without_scratch_or_spills():
    """all four entries are in wd_kernels_cc.hsaco with a workgroup of 256, no private segment, no spilled VGPR, no static
    LDS (the packed actor lives in dynamic LDS) and as many kernel arguments as the env's step takes plus the sixteen of
    the evaluation"""
    manifest = _manifest()
    for k in KERNELS:
        assert manifest.get(k) == "wd_kernels_cc.hsaco", k
    meta = _code_object_metadata()
    assert set(KERNELS) <= set(meta)
    for name, env in KERNELS.items():
        workgroup, private, spills, vgprs, sgprs, sgpr_spills, lds, n_args = meta[name]
        print(f"{name}: {vgprs} VGPRs, {sgprs} SGPRs ({sgpr_spills} spilled to VGPR lanes), private {private}, VGPR "
              f"spills {spills}, static LDS {lds}, {n_args} arguments")
        assert (workgroup, private, spills, lds) == (256, 0, 0, 0), (name, workgroup, private, spills, lds)
        assert vgprs <= 256   # two blocks of 256 threads per CU (__launch_bounds__(256, 2))
        assert n_args == N_STEP_ARGS[env] + N_TAIL, (name, n_args)


def test_which_envs_admit_a_live_actor_evaluation():
    """true exactly for (ContinuousMountainCar | Pendulum) x {32, 64} with the entry in the manifest; the discrete
    envs' `has_live_policy_evaluate` is what it was"""
    manifest = _manifest()
    for name, (cls, _, x) in _classes().items():
        box = name in ae.ENVS
        env = _fake_managed(name, 1000, manifest)
        for width in (8, 16, 31, 32, 33, 48, 64, 128, 256):
            assert env.has_live_actor_evaluate(width) is (box and width in (32, 64)), (name, width)
            assert env.has_live_policy_evaluate(width, 3) is (not box and width in (32, 64)), (name, width)
        # ... and only while the code object has the entry
        env.cuda_function_manager = _FakeFM({k: v for k, v in manifest.items() if "Evaluate_A32" not in k})
        assert not env.has_live_actor_evaluate(32) and env.has_live_actor_evaluate(64) is box
        assert env.has_live_actor_rollout(32) is box   # (the rollout entry is another kernel)


def _launch_inputs(env_name, width, E=1000, T=20):
    import torch

    O = cc.OBS_DIM[env_name]
    env = _fake_managed(env_name, E, _manifest())
    env.cuda_data_manager.device_data = lambda name: ("device", name)
    OP = O + O % 2
    n_w = OP * width + width + width * width + width + width + 1   # W0 [H][OP], b0, W1 [H][H], b1, Wa [H], ba
    packed = _tensor((n_w,), torch.float32)
    outputs = {"reward_sum": _tensor((E, 1), torch.float32), "steps": _tensor((E + 3,), torch.int32),
               "done": _tensor((E,), torch.int32)}
    sampler = types.SimpleNamespace(rng_state="rng")
    return env, sampler, packed, outputs, n_w


@pytest.mark.parametrize("env_name", ae.ENVS)
@pytest.mark.parametrize("width", [32, 64])
def test_evaluate_actor_launch_argument_by_argument(env_name, width):
    """the Evaluate_A<width> entry at the step's block and grid; the step's arguments, then (rng words, the tick's stream
    tag, ticks, packed, width, action_scale, action_bias, ou_state, damping, stddev, scale, reward_sum, steps, done,
    mean_trace or null, action_trace or null); 4 n_w bytes of LDS"""
    import torch
    from warp_drive_amd.managers.function_manager import _stream_tag

    E, T = 1000, 20
    x = _classes()[env_name][2]
    env, sampler, packed, outputs, n_w = _launch_inputs(env_name, width, E, T)
    assert n_w == ca.actor_weight_count(cc.OBS_DIM[env_name], width)
    if (env_name, width) == ("pendulum", 64):
        assert 4 * n_w == 18180   # 4 * (4 * 64 + 64 + 64 * 64 + 64 + 64 + 1)
    step = env.step_launch()
    assert len(step[1]) == N_STEP_ARGS[env_name]
    means, acts = _tensor((T + 2, E), torch.float32), _tensor((T, E, 1), torch.float32)
    for ticks, want_ticks in ((None, 20), (T, T), (7, 7)):   # (default: the env's episode_length, 20 in the fake)
        for mean_trace, action_trace in ((None, None), (means, None), (None, acts), (means, acts)):
            fn, args, block, grid, shared = env.evaluate_actor_launch(
                sampler, actor=(packed, width, 1.25, 0.75), ou=(0.1, 0.3, 0.5), outputs=outputs, mean_trace=mean_trace,
                action_trace=action_trace, ticks=ticks)
            assert fn.name == f"HipClassicControl{x}EnvEvaluate_A{width}" and shared == 4 * n_w <= 65536
            assert fn.name in env.cuda_function_manager.initialized
            assert (block, grid) == (step[2], step[3]) and block[0] <= cc.LAUNCH_BOUND
            assert len(args) == len(step[1]) + N_TAIL
            for g, w in zip(args[:-N_TAIL], step[1]):
                assert type(g) is type(w) and g == w
            tail = args[-N_TAIL:]
            assert tail[0] == "rng"
            assert type(tail[1]) is type(_stream_tag("tick")) and tail[1] == _stream_tag("tick") == cc.TICK_TAG
            assert type(tail[2]) is np.int32 and tail[2] == want_ticks
            assert tail[3] is packed
            assert type(tail[4]) is np.int32 and tail[4] == width
            for got, want in zip(tail[5:7] + tail[8:11], (1.25, 0.75, 0.1, 0.3, 0.5)):
                assert type(got) is np.float32 and got == np.float32(want)
            assert tail[7] == ("device", "sampled_actions_ou_state")
            assert tail[11] is outputs["reward_sum"] and tail[12] is outputs["steps"] and tail[13] is outputs["done"]
            for got, want in ((tail[14], mean_trace), (tail[15], action_trace)):
                if want is None:
                    assert type(got) is np.uint64 and got == 0
                else:
                    assert got is want


@pytest.mark.parametrize("env_name", ae.ENVS)
def test_evaluate_actor_launch_refusals(env_name):
    """a packed actor of the wrong size, dtype, device or layout, a width of 48 or of the other entry's size, a malformed
    `actor` or `ou`, trace tensors too short / too narrow / of another dtype, outputs too short or of another dtype: all
    UnsupportedRolloutShape, nothing initialised"""
    import torch
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    E, T, width = 1000, 20, 32
    env, sampler, packed, outputs, n_w = _launch_inputs(env_name, width, E, T)
    ou = (0.15, 0.2, 1.0)
    bad_actors = [(_tensor((n_w + 1,), torch.float32), width, 1.0, 0.0), (_tensor((n_w - 1,), torch.float32), width, 1.0, 0.0),
                  (_tensor((n_w,), torch.float64), width, 1.0, 0.0), (_tensor((n_w,), torch.float32, cuda=False), width, 1.0, 0.0),
                  (_tensor((n_w,), torch.float32, contiguous=False), width, 1.0, 0.0), (packed, 48, 1.0, 0.0),
                  (packed, 64, 1.0, 0.0), (packed, width), packed, None, (packed, width, "x", 0.0)]
    for actor in bad_actors:
        with pytest.raises(UnsupportedRolloutShape):
            env.evaluate_actor_launch(sampler, actor=actor, ou=ou, outputs=outputs)
    good = (packed, width, 1.0, 0.0)
    for bad_ou in ((0.15, 0.2), None, (0.15, "x", 1.0)):
        with pytest.raises(UnsupportedRolloutShape):
            env.evaluate_actor_launch(sampler, actor=good, ou=bad_ou, outputs=outputs)
    for trace in (_tensor((T - 1, E), torch.float32), _tensor((T, E + 1), torch.float32), _tensor((T, E - 1), torch.float32),
                  _tensor((T, E), torch.float64), _tensor((T, E), torch.int32), _tensor((T, E), torch.float32, cuda=False),
                  _tensor((T, E), torch.float32, contiguous=False), _tensor((T * E,), torch.float32)):
        for key in ("mean_trace", "action_trace"):
            with pytest.raises(UnsupportedRolloutShape):
                env.evaluate_actor_launch(sampler, actor=good, ou=ou, outputs=outputs, **{key: trace})
    ok = _tensor((T - 1, E), torch.float32)   # ... long enough for a shorter launch
    env.evaluate_actor_launch(sampler, actor=good, ou=ou, outputs=outputs, mean_trace=ok, action_trace=ok, ticks=T - 1)
    for key, bad in (("reward_sum", _tensor((E - 1,), torch.float32)), ("reward_sum", _tensor((E,), torch.float64)),
                     ("steps", _tensor((E - 1,), torch.int32)), ("steps", _tensor((E,), torch.float32)),
                     ("done", _tensor((E - 1,), torch.int32)), ("done", _tensor((E,), torch.int32, cuda=False))):
        with pytest.raises(UnsupportedRolloutShape):
            env.evaluate_actor_launch(sampler, actor=good, ou=ou, outputs={**outputs, key: bad})


@pytest.mark.parametrize("env_name", ["acrobot", "mountain_car"])
def test_discrete_envs_refuse_an_actor_evaluation(env_name):
    import torch
    from warp_drive_amd.rollout import UnsupportedRolloutShape

    env = _fake_managed(env_name, 1000, _manifest())
    out = {"reward_sum": _tensor((1000,), torch.float32), "steps": _tensor((1000,), torch.int32),
           "done": _tensor((1000,), torch.int32)}
    with pytest.raises(UnsupportedRolloutShape):
        env.evaluate_actor_launch(types.SimpleNamespace(rng_state="rng"), actor=(_tensor((100,), torch.float32), 32, 1.0, 0.0),
                                  ou=(0.15, 0.2, 1.0), outputs=out)


# ----------------------------------------------------------------------------------- the cases are not vacuous
def test_recorded_seeds_and_scales_are_what_the_search_finds():
    assert ae.search() == {key: (ae.SEED[key], ae.HEAD_SCALE[key]) for key in ae.SEED}


def test_episode_lengths_and_geometries():
    """episodes of 16 to 24 ticks (the range of the discrete evaluation cases); block 256 x grid 1: three trips, the last
    partial; block 64 x grid 3: more than three; a grid with idle blocks; E = 1 and 65 run the host's geometry only"""
    assert all(16 <= T <= 24 for T in ae.EPISODE_LENGTH.values())
    assert cc.geometry(ae.E_PARITY, (256, 1)) == (256, 1, 3) and ae.E_PARITY % 256 != 0
    assert cc.geometry(ae.E_PARITY, (64, 3)) == (64, 3, 4)
    assert cc.geometry(ae.E_PARITY, (64, "idle"))[1] == 11 + 2
    assert {c.E for c in ae.SMALL_CASES} == {1, 65}
    assert {(c.env, c.hidden, c.mode) for c in ae.PARITY_CASES} == {(e, h, m) for e in ae.ENVS for h in (32, 64)
                                                                    for m in ae.MODES}


@pytest.mark.parametrize("case", ae.CASES, ids=repr)
def test_case_is_not_vacuous_on_the_host(case):
    """the GPU test's actor, seeds and sizes replayed on the host alone.  With more than one replica: a tenth of the
    means in tanh's linear range and a tenth in its saturated one.  ContinuousMountainCar at full length: terminations
    on at least 3 different ticks, and time-outs.  Residue timesteps: the time-out arrives on 4 different ticks.  Sampled
    with the wrap rows: 16 replicas (15 where one terminates first) cross 2^32.  A launch shorter than the episode leaves
    replicas unfinished (done 0, steps == ticks)."""
    r = ae.replay(case)
    t = r["tanh"]
    print(f"{case.name}: |tanh z| < 0.5 {float((t < 0.5).mean()):.3f}, > 0.99 {float((t > 0.99).mean()):.3f}; terminations "
          f"{r['end_ticks']}, time-outs {r['timeout_ticks']}, {r['wrapped']} replicas cross 2^32")
    assert len(t) == int(r["steps"].sum())
    if case.E > 1:
        assert ae.spans_tanh(t)
    full = case.ticks == case.T
    if full:
        assert (r["done"] > 0).all() and (r["steps"] >= 1).all() and (r["steps"] <= case.T).all()
    else:
        unfinished = r["done"] == 0
        assert unfinished.sum() >= case.E // 2 and (r["steps"][unfinished] == case.ticks).all()
    if case.env == "continuous_mountain_car" and full and case.E > 1:
        assert len(r["end_ticks"]) >= 3 and sum(r["timeout_ticks"].values()) > 0
    if case.env == "pendulum":
        assert not r["end_ticks"]   # (Pendulum has no terminal state: only the time-out ends an episode)
    if case.timesteps == "residue":
        late = {k: n for k, n in r["timeout_ticks"].items() if k >= case.T - 4}
        assert sorted(late) == list(range(case.T - 4, case.T)) and min(late.values()) >= 20
    if not case.greedy and case.E >= 63:
        assert r["wrapped"] >= 15
        assert (r["epochs"] != case.start_epochs()).all()
    if case.greedy:
        assert r["wrapped"] == 0 and (r["epochs"] == case.start_epochs()).all() and (r["ou"] == case.start_ou()).all()
    assert np.abs(case.start_ou()).max() > 0


# ------------------------------------------------------------------------------------------------------ trainer
class _Env:
    def __init__(self, widths):
        self.widths, self.asked = widths, []

    def has_live_actor_evaluate(self, width):
        self.asked.append(width)
        return width in self.widths


def _bare_trainer(key, rollout_path, width, env_widths=(32, 64), evaluator=None):
    from warp_drive_amd.training.trainer_ddpg import TrainerDDPG

    tr = TrainerDDPG.__new__(TrainerDDPG)
    tr.policies = ["shared"]
    tr.config = {"trainer": {}}
    if key is not None:
        tr.config["trainer"]["fused_evaluation"] = key
    if evaluator is not None:
        tr.config["trainer"]["evaluator"] = evaluator
    tr.rollout_path = rollout_path
    tr._batch_rollout = {"width": width, "packed": {}, "range": (2.0, 0.0)} if rollout_path == "one launch" else None
    tr.w = types.SimpleNamespace(env=_Env(env_widths))
    return tr


def test_trainer_chooses_the_evaluation_path():
    """one launch exactly when `trainer.fused_evaluation` is true AND the rollout is one launch AND the env has the entry
    of the actor's width; the key's absence means false"""
    for key in (None, False, True):
        for path in ("per tick", "one launch"):
            for width, env_widths in ((32, (32, 64)), (64, (32, 64)), (32, (64,)), (64, ())):
                tr = _bare_trainer(key, path, width, env_widths)
                got = tr._one_launch_evaluation()
                want = key is True and path == "one launch" and width in env_widths
                assert (got is not None) is want, (key, path, width, env_widths)
                if want:
                    assert got == (tr.w.env, width)
                if key is not True or path != "one launch":
                    assert tr.w.env.asked == []   # (the env is not even asked)
    tr = _bare_trainer(True, "one launch", 32)
    tr.w = types.SimpleNamespace(env=object())   # an env without Evaluate entries
    assert tr._one_launch_evaluation() is None


def test_evaluator_adds_the_two_test_metrics(tmp_path):
    """`trainer.evaluator: true`: `_log_metrics` runs ONE greedy evaluate_episodes and adds the reference's two names, the
    means over the replicas, to the policy's metrics and to results.json; without the key (or false) no evaluation runs
    and the names are absent"""
    import json

    from warp_drive_amd.training.trainer import PerfStats

    rewards = np.array([[-3.0], [-1.0], [-8.0], [0.0]], np.float32)
    steps = np.array([16, 16, 7, 1], np.int32)
    names = {"Mean episodic reward (test)", "Mean episodic steps (test)"}
    for evaluator in (None, False, True):
        tr = _bare_trainer(True, "one launch", 32, evaluator=evaluator)
        tr.perf_stats, tr.world, tr.rank, tr.verbose = PerfStats(), 1, 0, False
        tr.save_dir = str(tmp_path / f"evaluator-{evaluator}")
        calls = []

        def evaluate_episodes(**kw):
            calls.append(kw)
            return {"shared": rewards}, {"shared": steps}

        tr.evaluate_episodes = evaluate_episodes
        metrics = {"shared": {"Total loss": 0.5, "Mean episodic reward": -2.0}}
        tr._log_metrics(4, metrics)
        record = json.loads(open(os.path.join(tr.save_dir, "results.json")).read().splitlines()[-1])
        assert record["Iterations Completed"] == 5 and record["shared"] == metrics["shared"]
        if evaluator:
            assert calls == [{"use_argmax": True}]
            assert names < set(metrics["shared"])
            assert metrics["shared"]["Mean episodic reward (test)"] == -3.0
            assert metrics["shared"]["Mean episodic steps (test)"] == 10.0
        else:
            assert calls == [] and not names & set(metrics["shared"])
        assert metrics["shared"]["Mean episodic reward"] == -2.0   # the training value stays
