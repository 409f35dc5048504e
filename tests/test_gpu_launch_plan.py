"""The launch plans of libwdhip.so on the real runtime: what tests/test_launch_plan_host.py pins against a recording
fake, tied to the device at two points the fake cannot vouch for.
  * The graph route (RolloutEngine.run_graph: capture, instantiate, replay) must BE the plan route: every array and the
    RNG words bit-identical to an engine stepped with run(1), restarts inside a graph included (15-tick episodes).
  * The event-bracket sampler bench.py reads must cover exactly the launches the host test's model of its counters
    says, and its total lies inside the host's wall-clock interval around the runs (every bracket does: a bound, not a
    measurement).
No error path is exercised here."""
import time

import numpy as np
import pytest
import torch

from tests.test_gpu_tick_cohorts import ARRAYS, CFG, _assert_same, _state
from tests.test_gpu_tick_rollout import _engine
from tests.test_launch_plan_host import MIXED_SEQUENCES, mixed_runs, model_for

pytestmark = pytest.mark.gpu

GW_ARRAYS = ("observations", "rewards", "_done_", "sampled_actions", "loc_x", "loc_y", "_timestep_")


def _graph_against_single_ticks(ref, eng, state_of):
    side = torch.cuda.Stream()  # (a capture cannot begin on the legacy default stream)
    torch.cuda.synchronize()
    done = 0
    for ticks, per_graph in ((40, 10), (20, 5)):  # the second one re-instantiates
        eng.run_graph(ticks, per_graph, side.cuda_stream)
        for _ in range(ticks):
            ref.run(1)
        done += ticks
        a, b = state_of(eng), state_of(ref)
        assert set(a) == set(b) and "rng_state" in a
        _assert_same(a, b, f"after {done} ticks (graphs of {per_graph})")
    assert eng._graph_ticks == 5


def test_graph_of_the_fused_tick_is_the_plan(monkeypatch):
    """the one-entry TagContinuous tick at E = 200: 4 replays of a 10-tick graph, then 4 of a 5-tick one"""
    w1, s1, ref = _engine(monkeypatch, 200, False, cohorts=1)
    wg, sg, eng = _engine(monkeypatch, 200, False, cohorts=1)
    assert len(eng.plan) == 1 and CFG["episode_length"] == 15
    states = {id(ref): (w1, s1), id(eng): (wg, sg)}
    _graph_against_single_ticks(ref, eng, lambda e: _state(*states[id(e)]))
    assert set(ARRAYS) < set(_state(wg, sg))
    assert int(_state(w1, s1)["_timestep_"].max()) <= 15  # 60 ticks of 15-tick episodes: restarts fell inside the graphs


def test_graph_of_a_multi_entry_plan_is_the_plan():
    """TagGridWorld, 5 agents, E = 257, unfused: sample -> step -> reset, three launches per tick inside the graph"""
    from tests.hip_harness import make_wrapper, pull, require_gpu
    from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorld
    from warp_drive_amd.managers import hip_driver as drv
    from warp_drive_amd.managers.function_manager import HIPSampler
    from warp_drive_amd.rollout import RolloutEngine

    require_gpu()
    E = 257
    cfg = dict(num_taggers=4, grid_length=10, episode_length=15, seed=27, wall_hit_penalty=0.1, tag_reward_for_tagger=10.0,
               tag_penalty_for_runner=2.0, step_cost_for_tagger=0.01, use_full_observation=True)
    probs_host = np.random.RandomState(3).dirichlet(np.ones(5), size=(E, 5)).astype(np.float32)

    def make():
        w = make_wrapper(CUDATagGridWorld(**cfg), E)
        sampler = HIPSampler(w.cuda_function_manager)
        sampler.init_random(seed=5)
        engine = RolloutEngine(w, sampler, probabilities=[torch.from_numpy(probs_host).cuda()], fused=False)
        assert not engine.fused and len(engine.plan) == 3 and engine.step_kernel_name == "HipTagGridWorldStep"
        return w, sampler, engine

    def state_of(made):
        w, sampler, _ = made
        torch.cuda.synchronize()
        out = {k: pull(w, k) for k in GW_ARRAYS}
        out["rng_state"] = np.zeros(4 + E * 5, dtype=np.uint32)
        drv.memcpy_dtoh(out["rng_state"], sampler.rng_state)
        return out

    a, b = make(), make()
    by_engine = {id(a[2]): a, id(b[2]): b}
    _graph_against_single_ticks(a[2], b[2], lambda e: state_of(by_engine[id(e)]))
    assert int(state_of(a)["_timestep_"].max()) <= 15  # restarts fell inside the graphs


@pytest.mark.parametrize("kind,E", [("cohorts", 2000), ("multi", 2000), ("single", 200)])
def test_sampler_counts_on_the_real_runtime(monkeypatch, kind, E):
    """the host test's mixed run(k) sequences at stride 8 on an engine that takes the cohort route, the multi-tick
    route, or neither: read_timing() covers exactly the launches the model of the counters says"""
    from warp_drive_amd import rollout

    _, _, eng = _engine(monkeypatch, E, kind == "multi", cohorts=2 if kind == "cohorts" else 1)
    assert eng.cohorts == (2 if kind == "cohorts" else 1) and len(eng.plan) == 1
    eng.run(3)  # (first launches: code object load)
    torch.cuda.synchronize()
    for name in MIXED_SEQUENCES:
        model = model_for(kind, max_ticks=rollout.ROLLOUT_MAX_TICKS)
        eng.plan.enable_timing(0, 8, 64)
        model.enable(0, 8, 64)
        t0 = time.perf_counter()
        for k in mixed_runs(name):
            eng.run(k)
            model.run(k)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        ms, n = eng.plan.read_timing()
        print(f"{kind} E={E} {name}: {n} launches in {ms:.4f} ms of brackets, {wall_ms:.3f} ms on the host's clock")
        assert n == model.read()[0] and n > 0
        assert 0.0 < ms <= wall_ms
        assert eng.plan.read_timing() == (0.0, 0)  # a read starts over
    eng.plan.enable_timing(-1, 1, 1)
    eng.run(1)
    eng.run(9)
    torch.cuda.synchronize()
    assert eng.plan.read_timing() == (0.0, 0)
