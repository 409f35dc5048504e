"""The multi-tick TagContinuous entry leaves the tag scan after the squared distances when no runner of the wavefront can be
tagged (tc_find_tag<SKIP>, tc_tags.h): the vote is `!(m2 > Bc)` with Bc = RN(margin^2) * (1 + 2^-20) rounded up.  It must
tag exactly whom the one-tick entry tags: two engines from the same state, run(1) repeated against run(n), the thirteen arrays
and the RNG words at tolerance 0.

Positions are written by the host and every agent draws the no-op action (both heads put all their mass on entry 0, speeds
start at 0), so nobody moves and the squared distance of the crafted pair is the float32 the test chose, to the bit: the
tagger sits at the origin, the runner at (dx, dy) with RN(RN(dx * dx) + RN(dy * dy)) equal to the target."""
import numpy as np
import pytest
import torch

from tests.test_gpu_tick_cohorts import CFG
from tests.test_gpu_tick_rollout_rows import _host_write, _run_chunks
from tests.test_gpu_tick_rollout_straight import _compare, _engine

pytestmark = pytest.mark.gpu

N = 105
f32 = np.float32
L = f32(CFG["grid_length"])


def _margin(cfg):
    return f32(cfg["tagging_distance"] * f32(cfg["grid_length"]))


def _bound(margin):
    """Bc as the kernel's prologue forms it (tc_loop_consts)"""
    b = f32(f32(margin * margin) * f32(1.0 + 2.0 ** -20))
    return np.nextafter(b, f32(np.inf)) if b > 0 else b


def _step(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf) if k > 0 else f32(-np.inf))
    return x


def _offset_for(target):
    """float32 (dx, dy) whose squared length, rounded as the kernel rounds it, is exactly `target`"""
    target = f32(target)
    base = f32(np.sqrt(np.float64(target) * 0.75))
    for k in range(0, 400):
        dx = _step(base, k)
        rem = np.float64(target) - np.float64(f32(dx * dx))
        if rem <= 0:
            break
        dy0 = f32(np.sqrt(rem))
        for m in range(-6, 7):
            dy = _step(dy0, m)
            if f32(f32(dx * dx) + f32(dy * dy)) == target:
                return dx, dy
    raise AssertionError(f"no float32 offset with squared length {target!r}")


def _pair(monkeypatch, E, cfg):
    """both engines with one-hot no-op probabilities; returns (one, multi, tagger ids, runner ids)"""
    one, multi = _engine(monkeypatch, E, False, cfg), _engine(monkeypatch, E, True, cfg)
    for _, _, _, probs in (one, multi):
        for p in probs:
            p.zero_()
            p[..., 0] = 1.0
    torch.cuda.synchronize()
    types = np.asarray(one[0].cuda_data_manager.pull_data_from_device("agent_types")).reshape(-1)[:N]
    taggers, runners = np.nonzero(types == 1)[0], np.nonzero(types == 0)[0]
    assert len(taggers) == 5 and len(runners) == 100
    return one, multi, taggers, runners


def _far_layout(E, taggers, runners):
    """nobody within 6 units of a tagger: taggers in the corners region x = 0 / x = L, runners in a band in the middle"""
    x, y = np.zeros((E, N), dtype=f32), np.zeros((E, N), dtype=f32)
    for k, t in enumerate(taggers):
        x[:, t], y[:, t] = (f32(0), f32(0)) if k == 0 else (L, f32(4 * k))
    for i, r in enumerate(runners):
        x[:, r], y[:, r] = f32(8 + 0.04 * i), f32(10 + 0.3 * (i % 3))
    return x, y


def _write_positions(one, multi, x, y):
    for w in (one[0], multi[0]):
        _host_write(w, "loc_x", lambda a: a.__setitem__(slice(None), x))
        _host_write(w, "loc_y", lambda a: a.__setitem__(slice(None), y))
    torch.cuda.synchronize()


def _run(one, multi, ticks=3):
    want = _run_chunks(one, multi, (ticks,))
    assert (want["sampled_actions"] == 0).all() and not want["speed"].any()  # nobody moved
    return want


D2_CASES = ["just_below_margin2", "margin2", "just_above_margin2", "at_Bc", "just_above_Bc"]


@pytest.mark.parametrize("case", D2_CASES)
def test_squared_distance_around_the_bound(monkeypatch, case):
    cfg = dict(CFG)
    margin = _margin(cfg)
    m2, Bc = f32(margin * margin), _bound(margin)
    assert m2 < Bc
    target = {"just_below_margin2": _step(m2, -1), "margin2": m2, "just_above_margin2": _step(m2, 1), "at_Bc": Bc,
              "just_above_Bc": _step(Bc, 1)}[case]
    assert (target > Bc) == (case == "just_above_Bc")  # every other case takes the roots
    E = 1 + D2_CASES.index(case) % 3
    one, multi, taggers, runners = _pair(monkeypatch, E, cfg)
    x, y = _far_layout(E, taggers, runners)
    dx, dy = _offset_for(target)
    # one crafted runner in the last replica, in wavefront 0 or 1 by turns; tagger 0 is at the origin, so the differences the
    # kernel forms are dx - 0 and dy - 0
    r0 = (runners[runners < 64] if D2_CASES.index(case) % 2 == 0 else runners[runners >= 64])[0]
    x[E - 1, r0], y[E - 1, r0] = dx, dy
    _write_positions(one, multi, x, y)
    want = _run(one, multi)
    tagged = bool(f32(np.sqrt(target)) < margin)  # numpy's float32 root is correctly rounded, as the kernel's is
    sig = want["still_in_the_game"].copy()
    assert sig[E - 1, r0] == (0 if tagged else 1), (case, target, margin)
    sig[E - 1, r0] = 1
    assert (sig == 1).all()
    if target >= Bc:  # what the bound promises: such a distance is never below the margin
        assert not tagged


def test_two_taggers_at_equal_distance_first_one_tags(monkeypatch):
    cfg = dict(CFG, runner_exits_game_after_tagged=False)
    one, multi, taggers, runners = _pair(monkeypatch, 2, cfg)
    x, y = _far_layout(2, taggers, runners)
    r = runners[runners >= 64][3]
    x[1, taggers[0]], y[1, taggers[0]] = f32(5.0), f32(5.0)
    x[1, taggers[1]], y[1, taggers[1]] = f32(5.5), f32(5.0)
    x[1, r], y[1, r] = f32(5.25), f32(5.1)
    _write_positions(one, multi, x, y)
    want = _run(one, multi)
    rew = want["rewards"]
    assert rew[1, taggers[0]] == 10.0 and rew[1, taggers[1]] == 0.0 and rew[1, r] == -10.0
    assert not rew[0].any()


@pytest.mark.parametrize("tagging_distance,tagged", [(0.0, False), (1e-30, True)])
def test_runner_coincident_with_a_tagger(monkeypatch, tagging_distance, tagged):
    """the bound is 0 in both cases (the square of 2e-29 underflows): only coincident points take the roots; sqrt(0) = 0 is
    below a margin of 2e-29 and not below a margin of 0"""
    cfg = dict(CFG, tagging_distance=tagging_distance)
    assert _bound(_margin(cfg)) == 0 and (_margin(cfg) > 0) == tagged
    one, multi, taggers, runners = _pair(monkeypatch, 3, cfg)
    x, y = _far_layout(3, taggers, runners)
    r = runners[runners < 64][5]
    x[2, taggers[2]], y[2, taggers[2]] = f32(3.0), f32(3.0)
    x[2, r], y[2, r] = f32(3.0), f32(3.0)
    _write_positions(one, multi, x, y)
    sig = _run(one, multi)["still_in_the_game"]
    assert sig[2, r] == (0 if tagged else 1)
    assert sig.sum() == sig.size - (1 if tagged else 0)


@pytest.mark.parametrize("where", ["wave1_only", "wave0_only", "both"])
@pytest.mark.parametrize("runner_exits", [True, False])
def test_runner_within_the_margin_in_one_wavefront_or_both(monkeypatch, where, runner_exits):
    cfg = dict(CFG, runner_exits_game_after_tagged=runner_exits)
    E = {"wave1_only": 1, "wave0_only": 2, "both": 3}[where]
    one, multi, taggers, runners = _pair(monkeypatch, E, cfg)
    x, y = _far_layout(E, taggers, runners)
    r0, r1 = runners[runners < 64][-1], runners[runners >= 64][-1]
    near = []
    if where != "wave1_only":
        x[E - 1, r0], y[E - 1, r0] = f32(0.1), f32(0.1)            # tagger 0 is at the origin
        near.append(r0)
    if where != "wave0_only":
        x[E - 1, r1], y[E - 1, r1] = f32(L - f32(0.1)), f32(4.1)   # tagger 1 is at (L, 4)
        near.append(r1)
    _write_positions(one, multi, x, y)
    want = _run(one, multi)
    sig, rew = want["still_in_the_game"], want["rewards"]
    out = np.zeros((E, N), dtype=bool)
    out[E - 1, near] = runner_exits
    assert np.array_equal(sig == 0, out)
    if not runner_exits:  # tagged again on the last tick
        assert all(rew[E - 1, r] == -10.0 for r in near)
        assert rew[E - 1, taggers[0]] == (10.0 if r0 in near else 0.0) and rew[E - 1, taggers[1]] == (10.0 if r1 in near else 0.0)


@pytest.mark.parametrize("tagging_distance", [1.0, 0.0])
def test_every_wavefront_takes_the_roots_or_none_does(monkeypatch, tagging_distance):
    """E = 9, run(40), random policies: with a margin of the grid length every runner is near a tagger, with 0 none is"""
    _compare(monkeypatch, 9, dict(CFG, tagging_distance=tagging_distance), (40,))
