"""Replica ranges of the TagContinuous tick off the headline shape: `step_launch(env_range=)` / `tick_launch(env_range=)`
(kEnvBegin = begin, kNumEnvs = end; what RolloutEngine's cohorts launch on parallel streams) for every entry class and
block packing of tests/tick_range_cases.py.  Device against device, tolerance 0, bit patterns: a range launch must do to
its replicas what the whole-range launch does and must leave every other replica alone -- the cohort next door runs at
the same time.  The cuts used here fall INSIDE the span of a packed block (no multiple of epb), as the cohorts' cuts at
multiples of 32 do."""
import numpy as np
import pytest
import torch

from tests import tick_range_cases as trc

pytestmark = pytest.mark.gpu

ALL_ARRAYS = trc.ARRAYS + trc.EXTRA_ARRAYS
ENTRIES = ("Step", "Tick", "TickA")
SHAPES = trc.range_shapes()


class _Twin:
    """a wrapper + sampler of a RANGE_SHAPES row with seeded Dirichlet policies, launched entry by entry"""

    def __init__(self, shape, E=None, seed=4242):
        from tests.hip_harness import require_gpu
        from warp_drive_amd.env_wrapper import EnvWrapper
        from warp_drive_amd.envs.tag_continuous import TagContinuous
        from warp_drive_amd.managers.function_manager import HIPSampler
        from warp_drive_amd.training.data_loader import create_and_push_data_placeholders

        require_gpu()
        self.shape = shape
        self.E = E = shape["E"] if E is None else E
        self.w = w = EnvWrapper(env_obj=TagContinuous(**shape["cfg"]), num_envs=E, env_backend="hip")
        w.reset_all_envs()
        self.sampler = HIPSampler(w.cuda_function_manager)
        self.sampler.init_random(seed=seed)
        create_and_push_data_placeholders(env_wrapper=w, action_sampler=self.sampler, training_batch_size_per_env=None,
                                          push_data_batch_placeholders=False)
        self.N = w.n_agents
        env = w.env
        # the row's claims: entry class and packing
        assert env.cuda_step.name == shape["entry"], (env.cuda_step.name, shape["entry"])
        epb, block, grid = env._geometry()
        assert (epb, block[0]) == (shape["epb"], shape["threads"]) and grid[0] == -(-E // epb), (epb, block, grid)
        assert env.can_fuse_tick() and env.has_presampled_tick() == trc.has_tick_on_given_actions(shape)
        rng = np.random.RandomState(seed)
        heads = (len(env.acceleration_actions), len(env.turn_actions))
        self.probs = [torch.from_numpy(rng.dirichlet(np.ones(a), size=(E, self.N)).astype(np.float32)).cuda()
                      for a in heads]

    def launch(self, entry, env_range=None):
        env = self.w.env
        if entry == "Step":
            fn, args, block, grid, shared = env.step_launch(env_range=env_range)
        else:
            fn, args, block, grid, shared = env.tick_launch(self.sampler, None if entry == "TickA" else self.probs,
                                                            self.w.env_resetter, env_range=env_range)
        assert fn.name == self.shape["entry"].replace("Step", entry)
        fn(*args, block=block, grid=grid, shared=shared)
        return grid[0]

    def snapshot(self):
        from tests.hip_harness import pull
        from warp_drive_amd.managers import hip_driver as drv

        torch.cuda.synchronize()
        out = {k: pull(self.w, k).copy() for k in ALL_ARRAYS}
        rng = np.zeros(trc.RNG_HEADER_WORDS + self.E * self.N, dtype=np.uint32)
        drv.memcpy_dtoh(rng, self.sampler.rng_state)
        torch.cuda.synchronize()
        out[trc.RNG] = rng
        return out

    def restore(self, snap):
        """every array back to a snapshot, bit for bit (the bookkeeping derived from them included: nothing to void)"""
        from warp_drive_amd.managers import hip_driver as drv

        dm = self.w.cuda_data_manager
        for k in ALL_ARRAYS:
            v = np.ascontiguousarray(snap[k])
            if dm.is_data_on_device_via_torch(k):
                dm.data_on_device_via_torch(k).copy_(torch.from_numpy(v))
            else:
                drv.memcpy_htod(dm.device_data(k), v)
        drv.memcpy_htod(self.sampler.rng_state, snap[trc.RNG])
        torch.cuda.synchronize()


def _same(a, b, tag, run_dependent=()):
    assert set(a) == set(b)
    for k in a:
        if k in run_dependent:  # (tick_range_cases.run_dependent_arrays: a hint that no result depends on)
            continue
        np.testing.assert_array_equal(a[k].view(np.uint8), b[k].view(np.uint8), err_msg=f"{k} {tag}")


def _entry_cases():
    return [(n, e) for n in trc.RANGE_SHAPE_NAMES for e in ENTRIES
            if e != "TickA" or trc.has_tick_on_given_actions(SHAPES[n])]


@pytest.mark.parametrize("name,entry", _entry_cases())
def test_range_launch_touches_its_replicas_only(name, entry):
    """ONE launch on each range of ranges(E, epb) -- whole, (1, E-1), one replica in the middle of a block's span, the
    first, the last, an empty one and a three-way partition cut inside blocks -- at tick 0, at the tick on which the
    replicas finish (restored inside the launch) and at the tick after it (`_done_` still set from the restore): the
    replicas of the range equal the twin's whole-range launch of the same entry from the same state, every other
    replica and the RNG header are untouched.  Step and TickA run on the actions the twin's sampling tick drew."""
    shape = SHAPES[name]
    T = shape["cfg"]["episode_length"]
    twin, other = _Twin(shape), _Twin(shape)
    E, N, epb = twin.E, twin.N, shape["epb"]
    hint = trc.run_dependent_arrays(shape)
    finished_seen = False
    for t in range(T + 1):
        if t in (0, T - 1, T):
            start = twin.snapshot()
            _same(other.snapshot(), start, f"the two wrappers at tick {t}", hint)
            twin.launch("Tick")
            after_tick = twin.snapshot()
            before = dict(start, sampled_actions=after_tick["sampled_actions"]) if entry != "Tick" else start
            if entry == "Tick":
                whole = after_tick
            else:
                twin.restore(before)
                twin.launch(entry)
                whole = twin.snapshot()
            # (a tick does change its replicas: "equal to `before`" outside the range is a statement)
            assert (whole["_timestep_"] != before["_timestep_"]).mean() > 0.5
            fin = whole["_done_"] > 0
            if t == T - 1:  # (a replica whose runners were all tagged finished earlier and is in mid-episode here)
                assert fin.mean() > 0.5
                if entry != "Step":  # restored inside the launch
                    assert (whole["_timestep_"][fin] == 0).all()
                finished_seen = True
            if t == T and entry != "Step":
                was = before["_done_"] > 0
                assert was.mean() > 0.5 and (whole["_done_"][was] == 0).all()
            for begin, end in trc.ranges(E, epb):
                other.restore(before)
                blocks = other.launch(entry, (begin, end))
                assert blocks == max(1, -(-(end - begin) // epb))
                faults = trc.check_range(before, other.snapshot(), whole, begin, end, N, hint)
                assert not faults, f"tick {t}, range [{begin}, {end}) of {E} replicas, epb {epb}: {faults}"
            twin.restore(start)
            other.restore(start)
        twin.launch("Tick")
        other.launch("Tick")
    assert finished_seen
    _same(other.snapshot(), twin.snapshot(), "after the last tick", hint)


@pytest.mark.parametrize("name", trc.RANGE_SHAPE_NAMES)
def test_partition_in_any_order_is_the_whole_tick(name):
    """the three ranges of the partition (cuts at epb + 1 and 2 * epb + 1), one after the other on one stream in a
    seeded shuffled order, on every tick until each replica has restarted twice: every array and the RNG words equal the
    twin's whole-range tick after every tick"""
    shape = SHAPES[name]
    T = shape["cfg"]["episode_length"]
    twin, other = _Twin(shape), _Twin(shape)
    parts = trc.partition(twin.E, shape["epb"])
    order = np.random.RandomState(len(name))
    restarts = np.zeros(twin.E, dtype=np.int64)
    for t in range(2 * T + 2):
        twin.launch("Tick")
        for i in order.permutation(3):
            other.launch("Tick", parts[i])
        a, b = other.snapshot(), twin.snapshot()
        _same(a, b, f"after tick {t}", trc.run_dependent_arrays(shape))
        restarts += b["_done_"] > 0
    assert restarts.min() >= 2, restarts


def _engine(monkeypatch, shape, E, cohorts, seed=4242):
    from warp_drive_amd import rollout

    monkeypatch.setattr(rollout, "TICK_COHORTS", cohorts)
    tw = _Twin(shape, E=E, seed=seed)
    engine = rollout.RolloutEngine(tw.w, tw.sampler, probabilities=tw.probs)
    assert engine.fused and engine.step_kernel_name == shape["entry"].replace("Step", "Tick")
    assert engine.rollout_kernel_name is None and len(engine.entry_names) == 1
    return tw, engine


def _half_cus():
    from tests.hip_harness import require_gpu

    require_gpu()
    return torch.cuda.get_device_properties(torch.device("cuda", torch.cuda.current_device())).multi_processor_count // 2


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("name", trc.COHORT_SHAPE_NAMES)
def test_cohort_engine_off_the_headline_shape(monkeypatch, name, C):
    """RolloutEngine with C cohorts on parallel streams at packed and big-replica shapes, E = epb * (half the CUs) * C
    + 45 so that every cohort still covers half of the CUs and the engine does split: run(n) sequences against an engine
    without cohorts stepped with run(1), every array (the three extra ones included) and the RNG words bit-identical"""
    from warp_drive_amd.rollout import cohort_bounds

    shape = SHAPES[name]
    epb = shape["epb"]
    half_cus = _half_cus()
    E = epb * half_cus * C + 45
    tw1, ref = _engine(monkeypatch, shape, E, 1)
    assert ref.cohorts == 1
    twc, eng = _engine(monkeypatch, shape, E, C)
    assert eng.cohorts == C and eng.plan.cohorts == C
    bounds = cohort_bounds(E, C)
    cuts = [b for b, _ in bounds[1:]]
    if epb > 1:
        assert any(c % epb for c in cuts), (cuts, epb)
    print(f"COHORT_CASE shape={name} N={shape['N']} E={E} C={C} epb={epb} half_cus={half_cus} cuts={cuts} "
          f"blocks_per_cohort={[-(-(e - b) // epb) for b, e in bounds]} off_epb={[c % epb for c in cuts]}")
    done = 0
    for chunk in (1, 7, 2, 5):
        for _ in range(chunk):
            ref.run(1)
        eng.run(chunk)
        done += chunk
        _same(twc.snapshot(), tw1.snapshot(), f"after {done} ticks (last run({chunk}))",
              trc.run_dependent_arrays(shape))
    assert done >= 2 * shape["cfg"]["episode_length"]  # every replica restarted twice along the way


def test_caller_stream_sees_every_cohort_at_a_packed_shape(monkeypatch):
    """a torch read on the caller's stream right after run(n), with no synchronisation, sees the final state of every
    cohort (the join events) -- at the 5-agent shape, 51 replicas per block"""
    shape = SHAPES["n5"]
    E = shape["epb"] * _half_cus() * 3 + 45
    tw1, ref = _engine(monkeypatch, shape, E, 1)
    twc, eng = _engine(monkeypatch, shape, E, 3)
    assert eng.cohorts == 3
    ref.run(24)
    dm = twc.w.cuda_data_manager
    eng.run(24)
    snap = {k: dm.data_on_device_via_torch(k).clone() for k in ("observations", "rewards", "sampled_actions")}
    torch.cuda.synchronize()
    for k, v in snap.items():
        np.testing.assert_array_equal(v.cpu().numpy(), tw1.w.cuda_data_manager.pull_data_from_device(k), err_msg=k)
