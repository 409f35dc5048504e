"""Host side of `trainer.fused_update_normalize` (csrc/kernels/pg_normalize.hip, wd_kernels_pg_norm.hsaco), no GPU: the three
entries and their cost, the launches of `_PgUpdateLaunches.normalize`, what the gradient launch is handed, the key's validation."""
import os

import numpy as np
import pytest
import torch

from tests.test_pg_update_host import _kernel_metadata, _NoDevice, _Recorder, built  # noqa: F401  (`built` is a fixture)
from warp_drive_amd.training import pg_update_kernels as pguk

OBJECT = "wd_kernels_pg_norm.hsaco"
MOMENTS, RETURNS, ADVANTAGES = pguk.NORMALIZE_ENTRIES


def test_the_three_entries_are_the_new_unit_without_scratch_or_spills(built):  # noqa: F811
    from warp_drive_amd import build as wd_build

    assert wd_build.UNITS[OBJECT] == ("pg_normalize.hip", wd_build.UNITS["wd_kernels_pg.hsaco"][1])
    assert pguk.NORMALIZE_CODE_OBJECT == OBJECT
    names = sorted(pguk.NORMALIZE_ENTRIES)
    assert names == ["HipPgNormalizeAdvantages", "HipPgNormalizeReturns", "HipPgTickMoments"] and pguk.NORMALIZE_CHUNK == 4096
    meta = _kernel_metadata(os.path.join(wd_build.CSRC, OBJECT))
    assert sorted(k for k, v in built.manifest().items() if v == OBJECT) == names == sorted(meta)
    for name, fields in meta.items():
        assert fields[".private_segment_fixed_size"] == 0 and fields[".vgpr_spill_count"] == 0, (name, fields)
        assert fields[".max_flat_workgroup_size"] == pguk.NORMALIZE_THREADS == 256, (name, fields)


@pytest.mark.parametrize("normalize_return,normalize_advantage", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("E,n,chunks", [(2, 1, 1), (1024, 4, 1), (4097, 1, 2)])
def test_the_launch_sequence_its_grids_and_what_the_gradient_launch_reads(E, n, chunks, normalize_return, normalize_advantage):
    from warp_drive_amd.training.pg_update_gridworld_kernels import PgGridworldUpdateKernels

    T, rec = 3, _Recorder()
    k = (pguk.PgUpdateKernels(rec, E, T, 32, 4, 2, "cpu", compute_units=4) if n == 1
         else PgGridworldUpdateKernels(rec, E, T, n, 32, "cpu", compute_units=4))
    five = list(rec.initialised)
    assert not set(five) & set(pguk.NORMALIZE_ENTRIES)                  # (entries and buffers come with the first use)
    assert k.normalize(False, False) == (k.advantages, k.returns) and not rec.launches
    advantages, returns = k.normalize(normalize_return, normalize_advantage)
    assert rec.initialised == five + list(pguk.NORMALIZE_ENTRIES)
    assert advantages is (k.norm_advantages if normalize_advantage else k.advantages)
    assert returns is (k.norm_returns if normalize_return else k.returns)
    want = ([MOMENTS, RETURNS] if normalize_return else [MOMENTS]) + ([ADVANTAGES] if normalize_advantage else [])
    assert [name for name, *_ in rec.launches] == want
    for name, args, block, grid, shared in rec.launches:
        assert block == (256, 1, 1) and grid == (T * chunks, 1) and shared == 0, (name, block, grid)
        at = {MOMENTS: 1, RETURNS: 3, ADVANTAGES: 2}[name]
        assert [int(a) for a in args[at:at + 3]] == [T, E * n, chunks], name
    assert k.partials_returns.shape == k.partials_advantages.shape == (T, chunks, 2)
    first = rec.launches[0][1]
    assert first[0] is (k.returns if normalize_return else k.advantages)
    assert first[4] is (k.partials_returns if normalize_return else k.partials_advantages)
    if normalize_return:
        a = rec.launches[1][1]
        assert (a[0], a[1], a[2], a[7], a[8]) == (k.returns, k.values, k.partials_returns, k.norm_returns, k.advantages)
        assert float(a[6]) == float(np.float32(1e-10))
        assert a[9] is k.partials_advantages if normalize_advantage else int(a[9]) == 0
    if normalize_advantage:
        a = rec.launches[-1][1]
        assert (a[0], a[1], a[6]) == (k.advantages, k.partials_advantages, k.norm_advantages)
    rec.launches.clear()
    z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)  # noqa: E731
    k.gradients(z(T, E, n, k.O), z(T, E, n, 1, dtype=torch.int32), z(k.P), 0.0, 0.1, advantages=advantages, returns=returns)
    (_, a, _, _, _), = rec.launches
    assert a[2] is advantages and a[3] is returns


def test_one_column_per_tick_is_refused():
    ok, why = pguk.normalize_refusal(1, 1)
    assert not ok and "standard deviation" in why and pguk.normalize_refusal(2, 1) == pguk.normalize_refusal(1, 2) == (True, "")
    rec = _Recorder()
    with pytest.raises(AssertionError, match="standard deviation"):
        pguk.PgUpdateKernels(rec, 1, 4, 32, 4, 2, "cpu", compute_units=4).normalize(True, True)
    assert not rec.launches


@pytest.mark.parametrize("value", ["true", 1, None])
def test_anything_but_a_bool_is_refused_before_anything_touches_the_device(value):
    from warp_drive_amd.training.trainer import Trainer

    config = lambda v: {"trainer": {"fused_update": "all", "fused_update_normalize": v, "num_envs": 4,  # noqa: E731
                                    "train_batch_size": 8, "num_episodes": 1}, "policy": {"shared": {"algorithm": "A2C"}}}
    with pytest.raises(ValueError, match="trainer.fused_update_normalize: True or False"):
        Trainer(env_wrapper=_NoDevice(), config=config(value))
    with pytest.raises(AttributeError):   # accepted: the constructor goes on to the wrapper, which this one does not have
        Trainer(env_wrapper=_NoDevice(), config=config(True))
