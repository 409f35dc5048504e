"""The multi-tick TagContinuous entry carries a thread's state in registers from trip to trip (TcCarry, tc_fast.h): it reads
memory on trip 0 of a launch and on the trip after a restore only.  Every array of tests/test_gpu_tick_rollout.py plus the
RNG words, tolerance 0, against a second engine stepped with run(1), at the smallest shapes at which a carry can go wrong:
restores on almost every trip (back to back included), an episode that ends on the last tick of a launch and on the first
of the next, replicas that empty and finish at their own ticks inside a launch, a lone block, slab addresses of every
16-byte alignment class, and host writes between two launches."""
import numpy as np
import pytest
import torch

from tests.test_gpu_tick_cohorts import CFG, _assert_same, _state
from tests.test_gpu_tick_rollout import ARRAYS, _engine

pytestmark = pytest.mark.gpu


def _pair(monkeypatch, E, cfg):
    w1, s1, ref = _engine(monkeypatch, E, False, cohorts=1, cfg=cfg)
    wr, sr, eng = _engine(monkeypatch, E, True, cfg=cfg)
    return (w1, s1, ref), (wr, sr, eng)


def _run_chunks(one, multi, chunks, done=0):
    (w1, s1, ref), (wr, sr, eng) = one, multi
    for chunk in chunks:
        for _ in range(chunk):
            ref.run(1)
        eng.run(chunk)
        done += chunk
        got, want = _state(wr, sr), _state(w1, s1)
        assert set(ARRAYS) < set(got) and "rng_state" in got
        _assert_same(got, want, f"after {done} ticks (last run({chunk}))")
    return done


@pytest.mark.parametrize("episode_length", [2, 3])
def test_restore_on_almost_every_trip(monkeypatch, episode_length):
    """episodes of 2 and 3 ticks: every second / third trip restores, launches of one tick among them, restores on the last
    trip of a launch and on trip 0 of the next"""
    one, multi = _pair(monkeypatch, 9, dict(CFG, episode_length=episode_length))
    _run_chunks(one, multi, (1, 2, 3, 5, 1, 8))


def test_episode_ends_on_the_last_and_on_the_first_tick_of_a_launch(monkeypatch):
    """5-tick episodes: they end on the last tick of run(5), run(5) and, after run(4), on the first tick of run(1) and inside run(6)"""
    one, multi = _pair(monkeypatch, 9, dict(CFG, episode_length=5))
    _run_chunks(one, multi, (5, 5, 4, 1, 6))


@pytest.mark.parametrize("override", [dict(tagging_distance=1.0), dict(tagging_distance=0.0),
                                      dict(runner_exits_game_after_tagged=False)],
                         ids=["arena_empties", "nobody_leaves", "tagged_runners_stay"])
def test_one_launch_of_forty_ticks(monkeypatch, override):
    """E = 33, 15-tick episodes, one run(40).  Tagging distance 1.0: replicas empty and finish (`no runners left`) at ticks of
    their own inside the launch, so blocks reload on different trips; 0.0: nobody leaves; tagged runners that stay in the game:
    the carried `still_in_the_game` must not follow the tag"""
    one, multi = _pair(monkeypatch, 33, dict(CFG, **override))
    _run_chunks(one, multi, (40,))
    sig = one[0].cuda_data_manager.pull_data_from_device("still_in_the_game")
    if override.get("tagging_distance") != 1.0:
        assert (sig == 1).all()


@pytest.mark.parametrize("E", [1, 257])
def test_lone_block_and_every_slab_alignment(monkeypatch, E):
    """a replica's slab is 105 * 21 * 4 = 8820 bytes = 4 mod 16: replicas 0 .. 3 start in the four 16-byte alignment classes, 257
    replicas (one more than a block per CU) cover each of them on every XCD; E = 1 is a launch of one block"""
    one, multi = _pair(monkeypatch, E, CFG)
    _run_chunks(one, multi, (3, 17))


def _host_write(w, name, fn):
    from warp_drive_amd.managers import hip_driver as drv

    dm = w.cuda_data_manager
    host = np.ascontiguousarray(dm.pull_data_from_device(name))
    fn(host)
    drv.memcpy_htod(dm.device_data(name), host)


@pytest.mark.parametrize("how", ["arrays", "reset_all_envs"])
def test_trip_zero_reads_what_the_host_wrote(monkeypatch, how):
    """run(7), a host write to the state of both engines, run(6): equal results prove that trip 0 of a launch takes its state
    from memory, not from anything the previous launch left"""
    one, multi = _pair(monkeypatch, 9, CFG)
    done = _run_chunks(one, multi, (7,))
    torch.cuda.synchronize()
    for w in (one[0], multi[0]):
        if how == "arrays":
            def move(x):
                x[:] = np.float32(20.0) - x  # mirrored: still inside the arena

            def retire(sig):
                sig[:, 7::9] = 0  # some runners (agents 7, 16, ... ; the taggers are agents of their own type) leave the game

            _host_write(w, "loc_x", move)
            _host_write(w, "still_in_the_game", retire)
            # the rows of the retired agents still hold their last observation: nothing is known to be cleared
            _host_write(w, "obs_rows_cleared", lambda c: c.fill(0))
        else:
            w.reset_all_envs()
    torch.cuda.synchronize()
    _run_chunks(one, multi, (6,), done)
    if how == "arrays":
        sig = multi[0].cuda_data_manager.pull_data_from_device("still_in_the_game")
        assert (sig[:, 7::9] == 0).all()
