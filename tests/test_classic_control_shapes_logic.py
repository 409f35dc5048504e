"""Host half of tests/test_gpu_classic_control_shapes.py: every case of tests/classic_control_cases.py is replayed with the
numpy steps and the host's Philox replay alone and must reach what it is there for -- restarts (on several ticks of a
launch), every action, every pool row, launches that start at every epoch residue, a replica that crosses the 2^32 wrap,
the crafted step rows' outcomes, three trips under every fixed grid -- so that the device file cannot pass vacuously.
No GPU."""
import copy
import json
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from tests import classic_control_cases as cc

F32 = np.float32


def test_case_names_are_unique_and_sizes_are_the_stated_ones():
    names = [c.name for c in cc.TICK_CASES + cc.ROLLOUT_CASES + cc.STEP_CASES]
    assert len(names) == len(set(names))
    for env in cc.ENVS:
        mine = [c for c in cc.TICK_CASES if c.env == env]
        assert {c.E for c in mine} >= {1, 63, 65, 700, 1501}
        assert all(c.launches >= 3 and c.ticks <= 50 for c in mine)
        assert any(c.rows is None for c in mine) and any(c.rows and c.rows > c.ticks for c in mine)
        assert any(c.ticks > c.T for c in mine) and any(c.ticks == c.T for c in mine)
        if env != "cartpole":
            assert {c.pool for c in mine} >= {0, 2, 7, 16}
            assert any(c.pool == 0 and c.rows for c in mine), "a recorded launch without a pool"


def test_the_draw_of_exactly_one_is_where_the_cases_say():
    from oracle.core_np import seed_words, single_head_tick_uniform

    row, epoch = cc.ONE_DRAW
    lo, hi = seed_words(cc.SAMPLER_SEED)
    u = single_head_tick_uniform(row + 1, np.full(row + 1, epoch, np.uint32), lo, hi, cc.TICK_TAG)
    assert u[row] == F32(1.0) and row * 16644 < (1 << 20) + 16644
    for case in cc.TICK_CASES:
        if case.has_one_draw():
            p = case.probabilities()[row]
            assert np.cumsum(p, dtype=F32)[-1] < 1   # every running sum is below the draw: the clamp decides
            assert case.actions()[case.one_draw_tick(), row] == case.A - 1


# ------------------------------------------------------------------------------------------------------ geometries
def test_every_fixed_grid_takes_three_trips_and_runs_somewhere():
    fixed = [g for g in cc.GEOMETRIES if g != "product" and isinstance(g[1], int)]
    assert fixed == [(128, 3), (192, 1), (256, 3)]
    for case in cc.TICK_CASES + cc.STEP_CASES:
        for g in cc.geometries(case.E):
            threads, blocks, trips = cc.geometry(case.E, g)
            assert threads <= cc.LAUNCH_BOUND and blocks >= 1 and threads * blocks * trips >= case.E
            if g in fixed:
                assert trips >= 3, (case, g)
            if g != "product" and g[1] == "idle":
                assert (blocks - 2) * threads >= case.E and trips == 1   # two blocks without a replica
            if g == (64, None) and case.E % 64:
                assert blocks * 64 > case.E   # a partial last wavefront
    for env in cc.ENVS:
        for kind in (cc.TICK_CASES, cc.STEP_CASES):
            ran = {g for c in kind if c.env == env for g in cc.geometries(c.E)}
            assert ran == set(cc.GEOMETRIES), (env, ran)
    for case in cc.ROLLOUT_CASES:
        for g in cc.ROLLOUT_GEOMETRIES:
            got = cc.geometry(case.E, g)
            assert got is not None and (not isinstance(g[1], int) or got[2] >= 3)
    # E = 1601 is the one size beyond the issue's list: (256, 3) needs E > 1536 for its third trip
    assert cc.geometry(1501, (256, 3)) is None and cc.geometry(1601, (256, 3)) == (256, 3, 3)


def test_a_block_over_the_launch_bound_is_refused():
    for threads in (257, 320, 512, 1024):
        with pytest.raises(ValueError):
            cc.geometry(700, (threads, 1))


def test_launch_bound_is_the_code_objects():
    """.max_flat_workgroup_size of every classic_control.hip entry is cc.LAUNCH_BOUND (Cartpole's entries are built
    without a bound or with 256: never below)"""
    from warp_drive_amd import build as wd_build

    wd_build.build_kernels_locked()
    manifest = json.load(open(wd_build.MANIFEST))
    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    found = {}
    for obj in sorted({manifest[cc.ENTRY[e] + "Step"] for e in cc.ENVS}):
        path = os.path.join(wd_build.CSRC, obj)
        with tempfile.TemporaryDirectory() as tmp:
            elf = os.path.join(tmp, "o.elf")
            subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={path}", f"--output={elf}"],
                           check=True, capture_output=True)
            notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True,
                                   capture_output=True, text=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            size = re.search(r"\.max_flat_workgroup_size:\s+(\d+)", block)
            if name and size and name.group(1).startswith("HipClassicControl"):
                found[name.group(1)] = int(size.group(1))
    want = [cc.ENTRY[e] + k for e in cc.ENVS for k in ("Step", "Tick")] + \
           [cc.ENTRY[e] + f"Rollout_H{h}" for e in cc.DISCRETE for h in (32, 64)]
    assert len(want) == 16 and set(want) <= set(found), sorted(set(want) - set(found))
    for name in want:
        if "CartPole" in name and "Rollout" not in name:
            assert found[name] >= cc.LAUNCH_BOUND, (name, found[name])
        else:
            assert found[name] == cc.LAUNCH_BOUND, (name, found[name])


# ------------------------------------------------------------------------------------------------------ tick cases
@pytest.fixture(scope="module")
def coverage():
    return {c.name: cc.simulate(c) for c in cc.TICK_CASES}


@pytest.mark.parametrize("case", cc.TICK_CASES, ids=repr)
def test_tick_case_reaches_its_coverage(case, coverage):
    cov = coverage[case.name]
    print(f"{case.name}: {cov.line()}")
    assert cov.restarts >= case.E, cov.line()
    if case.ticks >= 3:   # (a launch of one tick has one tick to restart on)
        assert len(cov.restart_ticks) >= 3, cov.line()
    if not case.cont:
        share = cov.actions / cov.actions.sum()
        assert len(share) == case.A and share.min() >= case.share, (case, share)
    if case.pool:
        assert len(cov.pool_rows) == case.pool if case.pool <= 7 else len(cov.pool_rows) >= 8, cov.line()
    if case.epochs == "residue" and case.E >= 63:
        assert cov.residues == {0, 1, 2, 3}, cov.line()
        if case.ticks >= 3:
            assert cov.wrapped >= 1, cov.line()
    if case.extra == "third":
        for fin in cov.finished_in_launch:   # the dirtied array comes back for some replicas and stays dirty for others
            assert 0 < fin.sum() < case.E, (case, int(fin.sum()))


def test_launch_lengths_do_what_they_are_there_for(coverage):
    for env in cc.ENVS:
        long_ = coverage[f"{env}-long-launch"]
        assert long_.case.ticks == 11 and long_.case.T == 4    # two or three restarts inside a launch
        assert long_.restarts >= 2 * long_.case.E * long_.case.launches
        ends = coverage[f"{env}-ends-on-restart"]
        assert ends.case.ticks == ends.case.T and (ends.case.start_timesteps() == 0).mean() > 0.6
        assert (ends.case.ticks - 1) in ends.restart_ticks     # every launch ends on the time-out
        one = coverage[f"{env}-one-tick"]
        assert one.case.ticks == 1 and (one.case.start_epochs() % 2 == 1).all()
        # every residue mod 4 starts a launch, in the 5-tick and in the 7-tick case alike
        for name in ("epochs-5", "epochs-7"):
            c = coverage[f"{env}-{name}"].case
            starts = {(int(c.start_epochs()[0]) + l * c.ticks) % 4 for l in range(c.launches)}
            assert starts == {0, 1, 2, 3}, (c, starts)


def test_action_counts_take_every_sampler_path():
    counts = {env: sorted({c.A for c in cc.TICK_CASES if c.env == env}) for env in cc.DISCRETE}
    assert counts["mountain_car"] == [1, 2, 3, 5, 8] and counts["acrobot"] == [1, 2, 3]
    assert counts["cartpole"] == [1, 2, 3, 8, 9, 12]   # the A2 copy / n_actions == 2, the masked path, the loop path
    for A in counts["cartpole"]:
        mine = [c for c in cc.TICK_CASES if c.env == "cartpole" and c.A == A]
        assert any(c.rows for c in mine) and any(c.rows is None for c in mine)
    for case in cc.TICK_CASES:
        if not case.cont and case.E >= 63:
            p = case.probabilities()
            A = case.A
            assert p[0, 0] == 1 and p[0].sum() == 1 and p[1, A - 1] == 1 and p[1].sum() == 1
            assert np.cumsum(p[2], dtype=F32)[-1] < 1
            assert A < 3 or (p[3, 1:A - 1] == 0).all()
            assert A < 2 or p[4, A // 2] == 0


# ------------------------------------------------------------------------------------------------ crafted step rows
def _crafted_outcomes(case):
    from warp_drive_amd.envs.classic_control import apply_done

    state, ts = case.start()
    a = case.actions()[0]
    n = len(case.crafted())
    out, obs, rew, term = cc.numpy_step(case.env, case.physics)(state[:n], a[:n])
    done = apply_done(term, ts[:n] + 1, case.T)
    return {label: (out[i], rew[i], int(done[i])) for i, (_, _, _, label) in enumerate(case.crafted())}


@pytest.mark.parametrize("case", [c for c in cc.STEP_CASES if c.E == 700 and c.env != "cartpole"], ids=repr)
def test_crafted_step_rows_give_the_listed_outcomes(case):
    from warp_drive_amd.envs import classic_control as ccenv

    got = _crafted_outcomes(case)
    env = case.env
    if env in ("mountain_car", "continuous_mountain_car"):
        base = ccenv.MountainCarPhysics if env == "mountain_car" else ccenv.ContinuousMountainCarPhysics
        p = type("P", (base,), dict(case.physics or {}))
        goal_done = 2 if env == "mountain_car" else 1
        s, _, d = got["wall"]
        assert s[0] == F32(p.min_position) and s[1] == 0 and d == 0
        s, r, d = got["goal"]
        assert s[0] == F32(p.max_position) and d == goal_done
        assert r == (F32(-1.0) if env == "mountain_car" else F32(100.0 - float(F32(3.0) * F32(3.0)) * 0.1))
        assert got["goal_on_last_tick"][2] == 1 and got["last_tick"][2] == 1   # the time-out wins (apply_done)
        if p.goal_velocity == p.max_speed:
            s, _, d = got["goal_at_clipped_speed"]
            assert s[1] == F32(p.max_speed) and d == goal_done
            s, _, d = got["slow_past_goal"]
            assert s[0] >= F32(p.goal_position) and s[1] < F32(p.max_speed) and d == 0
        if env == "continuous_mountain_car":
            np.testing.assert_array_equal(got["action_above"][0], got["action_max"][0])   # the clip decides
            np.testing.assert_array_equal(got["action_below"][0], got["action_min"][0])
            assert got["action_above"][1] != got["action_max"][1] or p.max_action == 3.0   # the reward takes the raw action
    elif env == "acrobot":
        # (moving outward from within 1e-3 of +-pi: the angle comes back on the other side)
        assert -np.pi <= got["wrap_theta1_up"][0][0] < 0 < got["wrap_theta1_down"][0][0] <= np.pi
        assert -np.pi <= got["wrap_theta2_up"][0][1] < 0 < got["wrap_theta2_down"][0][1] <= np.pi
        v1, v2 = F32(4 * np.pi), F32(9 * np.pi)
        hit = {(i, sg) for lab in ("bound_up", "bound_down", "bound_mixed", "bound_mixed2")
               for i, v in ((2, v1), (3, v2)) for sg in (1, -1) if got[lab][0][i] == F32(sg) * v}
        assert hit == {(2, 1), (2, -1), (3, 1), (3, -1)}, hit
        assert got["upright_last_tick"][2] == 1
    else:
        for label, (s, r, d) in got.items():
            assert d == 0 and abs(s[1]) <= 8.0 and np.isfinite(r)
        assert any(abs(s[1]) == 8.0 for s, _, _ in got.values())   # the speed clip binds
        assert max(abs(s[0]) for s, _, _ in got.values()) > 89.0


def test_other_physics_is_what_the_issue_lists():
    assert cc.OTHER_PHYSICS["mountain_car"] == dict(goal_velocity=0.05, max_speed=0.05, min_position=-0.9, force=0.002)
    assert cc.OTHER_PHYSICS["continuous_mountain_car"] == dict(min_action=-0.5, max_action=2.0, power=0.003,
                                                               goal_position=0.3)
    for env in cc.OTHER_PHYSICS:
        assert any(c.physics for c in cc.TICK_CASES if c.env == env)
        assert any(c.physics for c in cc.STEP_CASES if c.env == env)


# --------------------------------------------------------------------------------------------------------- rollout
@pytest.fixture(scope="module")
def rollouts():
    return {c.name: cc.simulate_rollout(c) for c in cc.ROLLOUT_CASES}


@pytest.mark.parametrize("case", cc.ROLLOUT_CASES, ids=repr)
def test_rollout_case_reaches_its_coverage_and_stays_under_the_cap(case, rollouts):
    cov, near = rollouts[case.name]
    print(f"{case.name}: {cov.line()}; {near} draws within {cc.NEAR_WINDOW} of a threshold (cap {case.near_cap()})")
    assert near <= case.near_cap()
    assert cov.restarts >= case.E and len(cov.restart_ticks) >= 3
    share = cov.actions / cov.actions.sum()
    assert share.min() >= case.share, share
    assert not case.pool or len(cov.pool_rows) == case.pool
    assert cov.residues == {0, 1, 2, 3} and cov.wrapped >= 1


# the largest |policy_probabilities - float64 PyTorch forward| over 20 000 observations must stay at or below 1e-6, half
# the 2e-6 window, for the window to stay (round 11: at most 6.7e-7 at A = 3)
RESTATEMENT_BAR = 1e-6


@pytest.mark.parametrize("case", cc.ROLLOUT_CASES, ids=repr)
def test_restatement_error_at_the_new_action_counts(case):
    import torch

    model, packed = case.policy()
    O = cc.OBS_DIM[case.env]
    rng = np.random.RandomState(7)
    states = cc.spread_states(case.env, rng, 20000)
    obs = cc.host_obs(case.env, states)
    assert obs.shape == (20000, O)
    got = cc.rollout_probabilities(case, packed, obs)
    with torch.no_grad():
        want = copy.deepcopy(model).double()(torch.from_numpy(obs).double())[0][0].numpy()
    assert want.shape == (20000, case.A)
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"{case.name}: O={O} H={case.hidden} A={case.A}: largest restatement difference {err:.3g}")
    assert err <= RESTATEMENT_BAR, err
