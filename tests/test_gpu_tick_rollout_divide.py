"""The multi-tick TagContinuous entry divides by its launch constants (max_speed + eps, 2 pi, the grid diagonal, the episode
length) through reciprocals formed once per launch (csrc/kernels/tc_divide.h).  That the form returns the bits of the true
division is proved on the device, per divisor, by HipTagContinuousVerifyInvariantDivide (every float32 dividend); the env
offers the multi-tick entry only with that proof, and the rollout engine keeps the cohort path without it.

Everything else here is the usual comparison: two engines from the same state, run(1) repeated (the one-tick entry, which
keeps the true divisions) against run(n), the thirteen arrays and the RNG words at tolerance 0, with divisors other than the
headline's (whose max_speed + eps is exactly 1.0)."""
import itertools

import numpy as np
import pytest
import torch

from tests.test_gpu_tick_cohorts import ARRAYS, CFG, _assert_same, _state
from tests.test_gpu_tick_rollout import ROLLOUT
from tests.test_gpu_tick_rollout_rows import _host_write, _run_chunks
from tests.test_gpu_tick_rollout_straight import _engine

pytestmark = pytest.mark.gpu

# (max_speed, grid_length, episode_length): the headline's, then every combination of the other values
HEADLINE = (1.0, 20.0, 500)
COMBOS = [HEADLINE] + list(itertools.product((0.7, 3.0), (13.0, 20.0), (3, 7, 500)))
CFG_A = dict(CFG, max_speed=0.7, grid_length=13.0, episode_length=7)
CFG_B = dict(CFG, max_speed=3.0, grid_length=20.0, episode_length=500)
CFG_C = dict(CFG, max_speed=0.7, grid_length=13.0, episode_length=3)


def _env(max_speed, grid_length, episode_length):
    from tests.hip_harness import require_gpu
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.envs.tag_continuous import TagContinuous

    require_gpu()
    env = TagContinuous(**dict(CFG, max_speed=max_speed, grid_length=grid_length, episode_length=episode_length))
    EnvWrapper(env_obj=env, num_envs=1, env_backend="hip")
    return env


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "ms%g_L%g_T%d" % c)
def test_verifier_proves_the_form_for_these_divisors(combo):
    """res = [ok, mismatches for max_speed + eps, 2 pi, the diagonal, t / T, excluded patterns (+-inf, diagonal only),
    float32 patterns inside the class the form is used for (64 bits)]"""
    from warp_drive_amd.envs.tag_continuous import TagContinuous

    TagContinuous._INVARIANT_DIVIDE_VERDICTS.pop((float(np.float32(combo[0])), float(np.float32(combo[1])), combo[2]), None)
    env = _env(*combo)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    res = env.invariant_divide_verdict()
    stop.record()
    torch.cuda.synchronize()
    in_class = (res[6] & 0xFFFFFFFF) | (res[7] << 32)
    print(f"verifier {combo}: {res[:6]}, {in_class} float32 patterns inside the class, {start.elapsed_time(stop):.1f} ms "
          "(launch + read-back)")
    assert res[:6] == [1, 0, 0, 0, 0, 2]
    # zero and 2^-65 <= |x| < 2^64, both signs: 2 + 2 * 129 binades of 2^23 patterns -- -0.0 is inside, not excluded
    assert in_class == 2 + 2 * 129 * (1 << 23)
    assert env.invariant_divide_ok()
    assert env.invariant_divide_verdict() is res  # cached: one launch per distinct triple


def test_verifier_notices_a_divisor_it_cannot_prove():
    """an infinite grid length has no finite diagonal: the verdict fails and the env offers no multi-tick entry"""
    from warp_drive_amd.envs.tag_continuous import TagContinuous

    env = _env(1.0, 20.0, 15)
    env.grid_length = np.float32(np.inf)
    try:
        res = env.invariant_divide_verdict()
        assert res[0] == 0 and not env.invariant_divide_ok()
    finally:
        TagContinuous._INVARIANT_DIVIDE_VERDICTS.pop((1.0, float("inf"), 15), None)


def test_failed_verdict_keeps_the_cohort_path(monkeypatch):
    from warp_drive_amd.envs.tag_continuous import TagContinuous

    E = 600  # two cohorts of 300 blocks: each covers more than half of the CUs
    w1, s1, ref, _ = _engine(monkeypatch, E, False, CFG)
    monkeypatch.setattr(TagContinuous, "invariant_divide_ok", lambda self: False)
    from warp_drive_amd import rollout
    from warp_drive_amd.env_wrapper import EnvWrapper
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.training.data_loader import create_and_push_data_placeholders
    from tests.test_gpu_tick_rollout_straight import _random_rows

    monkeypatch.setattr(rollout, "TICK_COHORTS", 2)
    monkeypatch.setattr(rollout, "TICK_ROLLOUT", 1)
    w = EnvWrapper(env_obj=TagContinuous(**CFG), num_envs=E, env_backend="hip")
    w.reset_all_envs()
    sampler = HIPSampler(w.cuda_function_manager)
    sampler.init_random(seed=4242)
    create_and_push_data_placeholders(env_wrapper=w, action_sampler=sampler, training_batch_size_per_env=None,
                                      push_data_batch_placeholders=False)
    engine = rollout.RolloutEngine(w, sampler, probabilities=_random_rows(E, w.n_agents, [21, 21], 77))
    assert not engine.rollout_kernel_name
    assert engine.cohorts == 2 and engine.plan.cohorts == 2
    for _ in range(6):
        ref.run(1)
    engine.run(6)
    _assert_same(_state(w, sampler), _state(w1, s1), "run(6) on the cohort path")
    monkeypatch.undo()
    w2, _, eng2, _ = _engine(monkeypatch, 1, True, CFG)  # the verdict itself is intact: the entry is offered again
    assert eng2.rollout_kernel_name == ROLLOUT


@pytest.mark.parametrize("E,cfg", [(1, CFG_A), (2, CFG_B), (9, CFG_A)], ids=["E1_A", "E2_B", "E9_A"])
@pytest.mark.parametrize("tagging_distance", [1.0, 0.0])
def test_run_40_with_other_divisors(monkeypatch, E, cfg, tagging_distance):
    cfg = dict(cfg, tagging_distance=tagging_distance)
    one, multi = _engine(monkeypatch, E, False, cfg), _engine(monkeypatch, E, True, cfg)
    _run_chunks(one, multi, (40,))


@pytest.mark.parametrize("E", [1, 2, 9])
def test_three_tick_episodes_reload_and_steady_trips(monkeypatch, E):
    one, multi = _engine(monkeypatch, E, False, CFG_C), _engine(monkeypatch, E, True, CFG_C)
    _run_chunks(one, multi, (1, 2, 3, 5, 1, 8))


@pytest.mark.parametrize("E,cfg", [(1, CFG_A), (2, CFG_B), (9, CFG_B)], ids=["E1_A", "E2_B", "E9_B"])
def test_host_written_state_between_launches(monkeypatch, E, cfg):
    """-0.0 in `acceleration` (the plain residual form returns +0.0 for it), 0 and grid_length in the positions, the largest
    heading below 2 pi: written into both engines between run(7) and run(6); trip 0 of the next launch reads them"""
    cfg = dict(cfg, episode_length=500, tagging_distance=0.0)
    one, multi = _engine(monkeypatch, E, False, cfg), _engine(monkeypatch, E, True, cfg)
    _run_chunks(one, multi, (7,))
    L = np.float32(cfg["grid_length"])
    two_pi = np.float32(6.2831854820251465)
    below_two_pi = np.nextafter(two_pi, np.float32(0))

    def acc(a):
        a[:, 0::3] = np.float32(-0.0)
        a[:, 1::7] = np.float32(0.0)

    def speed(s):
        s[:, 0::3] = np.float32(0.0)  # v = 0 + (-0.0 + table entry): the no-op entry keeps acc at -0.0 * 0 = -0.0

    def loc_x(x):
        x[:, 0::5] = np.float32(0.0)
        x[:, 1::5] = L

    def loc_y(y):
        y[:, 0::4] = L
        y[:, 2::4] = np.float32(0.0)

    def direction(d):
        d[:, 0::2] = below_two_pi
        d[:, 1::6] = np.float32(0.0)

    for w in (one[0], multi[0]):
        for name, fn in (("acceleration", acc), ("speed", speed), ("loc_x", loc_x), ("loc_y", loc_y), ("direction", direction)):
            _host_write(w, name, fn)
    torch.cuda.synchronize()
    want = _run_chunks(one, multi, (6,))
    # the reference itself met the pattern: a negative acceleration times the "is moving" zero is stored as -0.0
    assert (np.ascontiguousarray(want["acceleration"]).view(np.uint32) == 0x80000000).any()
