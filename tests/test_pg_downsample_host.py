"""Host side of `trainer.fused_update_downsample` (csrc/kernels/pg_downsample.hip, wd_kernels_pg_select.hsaco), no GPU: the
three entries and their cost, the key's validation, today's refusal without the key, and the numpy restatement of the
selection rule (`restated`, which tests/test_gpu_pg_downsample.py holds the launches to) against the framework's."""
import os

import numpy as np
import pytest
import torch

from tests.test_pg_update_host import _kernel_metadata, _NoDevice, built  # noqa: F401  (`built` is a fixture)
from warp_drive_amd.training import pg_update_kernels as pguk

OBJECT = "wd_kernels_pg_select.hsaco"


def restated(positive, keys, ratio):
    """(keep_ids ascending, (K, positives, negatives kept)): the framework's rule, the negatives ranked by (key, replica)"""
    E, pos = positive.size, int(positive.sum())
    neg = int(pos * ratio)
    if pos == 0 or pos + neg >= E:
        return np.arange(E), (E, pos, E - pos)
    negatives = np.flatnonzero(~positive)
    chosen = negatives[np.lexsort((negatives, keys[negatives]))[:neg]]
    return np.sort(np.concatenate([np.flatnonzero(positive), chosen])), (pos + neg, pos, neg)


def test_the_three_entries_are_the_new_unit_without_scratch_or_spills(built):  # noqa: F811
    from warp_drive_amd import build as wd_build

    assert wd_build.UNITS[OBJECT] == ("pg_downsample.hip", wd_build.UNITS["wd_kernels_pg.hsaco"][1])
    names = sorted(pguk.DOWNSAMPLE_ENTRIES)
    assert pguk.DOWNSAMPLE_CODE_OBJECT == OBJECT and names == ["HipPgGatherColumns", "HipPgSelectKeep", "HipPgSelectScan"]
    meta = _kernel_metadata(os.path.join(wd_build.CSRC, OBJECT))
    assert sorted(k for k, v in built.manifest().items() if v == OBJECT) == names == sorted(meta)
    threads = dict(zip(pguk.DOWNSAMPLE_ENTRIES, (pguk.SELECT_SCAN_THREADS, pguk.SELECT_KEEP_THREADS, pguk.GATHER_THREADS)))
    for name, fields in meta.items():
        assert fields[".private_segment_fixed_size"] == 0 and fields[".vgpr_spill_count"] == 0, (name, fields)
        assert fields[".max_flat_workgroup_size"] == threads[name], (name, fields)


@pytest.mark.parametrize("value", ["true", 1, None])
def test_anything_but_a_bool_is_refused_before_anything_touches_the_device(value):
    from warp_drive_amd.training.trainer import Trainer

    config = lambda v: {"trainer": {"fused_update": "all", "fused_update_downsample": v, "num_envs": 4,  # noqa: E731
                                    "train_batch_size": 8, "num_episodes": 1}, "policy": {"shared": {"algorithm": "A2C"}}}
    with pytest.raises(ValueError, match="trainer.fused_update_downsample: True or False"):
        Trainer(env_wrapper=_NoDevice(), config=config(value))
    with pytest.raises(AttributeError):   # accepted: the constructor goes on to the wrapper, which this one does not have
        Trainer(env_wrapper=_NoDevice(), config=config(True))


def test_without_the_key_the_ratio_is_refused_with_todays_sentence():
    shape = (True, 1, 1, [3], [32, 32], 2, torch.float32, False, False)
    assert pguk.admitted_shape(*shape, 10, 1, "A2C")[1] == "neg_pos_env_ratio: the replicas are down-sampled by the framework path only"
    assert pguk.admitted_shape(*shape, -1, 1, "A2C") == (True, "")


@pytest.mark.parametrize("ratio", [0.05, 1, 10, 1e6])
@pytest.mark.parametrize("positives", [(), (0, 31, 62), tuple(range(63))])
def test_the_restated_rule_is_the_frameworks(positives, ratio):
    from warp_drive_amd.training.losses import A2C

    E, rng = 63, np.random.default_rng(53)
    done = np.zeros((4, E), np.int32)
    done[2, 1::5] = 1                      # (an ordinary end of episode is no positive)
    done[3, list(positives)] = 2
    positive = (done == 2).any(axis=0)
    keep, (K, pos, neg) = restated(positive, rng.integers(0, 2 ** 32, E, dtype=np.uint32), ratio)
    np.random.seed(0)
    pos_ids, neg_ids, need = A2C._sample_positive_negative_env_ids(torch.from_numpy(done), ratio)
    assert (pos, neg, K < E) == (len(pos_ids), len(neg_ids), need) and K == len(keep) == len(set(keep.tolist()))
    assert sorted(pos_ids) == np.flatnonzero(positive).tolist() and set(pos_ids) <= set(keep.tolist())
    assert not positive[np.setdiff1d(keep, pos_ids)].any()
