"""`trainer.fused_update_downsample` (csrc/kernels/pg_downsample.hip): its three launches against numpy, exactly -- the Philox
draw of oracle/core_np.py, tests/test_pg_downsample_host.py::restated (np.lexsort on (e, key)), fancy indexing for the
gather -- then one iteration inside Trainer under tests/test_gpu_pg_update.py's bound."""
import numpy as np
import pytest
import torch

from oracle.core_np import philox4x32_10
from tests import pg_update_cases as pc
from tests.test_gpu_pg_update import DEV, STAGES, _counts, _judge, _launched_since, _trainer, fm  # noqa: F401
from tests.test_pg_downsample_host import restated
from warp_drive_amd.training import pg_update_kernels as pguk

pytestmark = pytest.mark.gpu
SEED_WORDS, EPOCH, FENCE = (12345, 0x5BD1E995), 7, -7


def _kernels(fm, E, T):  # noqa: F811
    return pguk.PgUpdateKernels(fm, E, T, 32, 2, 3, DEV)


def _keys(E, epoch=EPOCH, seed_words=SEED_WORDS):
    return philox4x32_10(np.arange(E, dtype=np.uint32), np.uint32(epoch), np.uint32(pguk.DOWNSAMPLE_STREAM_TAG), np.uint32(6),
                         *seed_words)[0]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _keep(k, ratio, E, **given):   # one HipPgSelectKeep into a fenced keep_ids -> (the K ids, the three counts)
    keep_ids = torch.full((E + 3,), FENCE, dtype=torch.int32, device=DEV)
    k.select_keep(ratio, keep_ids=keep_ids, **given)
    counts, ids = k.counts.tolist(), keep_ids.cpu().numpy()
    assert (ids[counts[0]:] == FENCE).all()                  # nothing past the K ids
    return ids[:counts[0]], tuple(counts)


@pytest.mark.parametrize("ratio", [0.05, 1, 10, 1e6])
@pytest.mark.parametrize("placed", ["first tick", "last tick", "none", "all"])
@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("E", [1, 63, 65, 1024, 1025, 4097])
def test_select_is_the_restated_rule(fm, E, T, placed, ratio):  # noqa: F811
    done = np.zeros((T, E), np.int32)
    done[T // 2, 1::5] = 1                                   # (an ordinary end of episode is no positive)
    where = {"none": [], "all": np.arange(E)}.get(placed, sorted({0, E // 2, E - 1}))
    done[-1 if placed == "last tick" else 0, where] = 2
    positive, keys = (done == 2).any(axis=0), _keys(E)
    want_ids, want_counts = restated(positive, keys, ratio)
    k = _kernels(fm, E, T)
    before = _counts()
    k.select_scan(_dev(done), EPOCH, SEED_WORDS)
    got_ids, got_counts = _keep(k, ratio, E)
    assert _launched_since(before) == {"HipPgSelectScan": 1, "HipPgSelectKeep": 1}
    assert np.array_equal(k.positive.cpu().numpy(), positive.astype(np.int32))
    assert np.array_equal(k.keys.cpu().numpy().view(np.uint32), keys)
    assert int(k.block_counts.sum()) == int(positive.sum()) and k.block_counts.numel() == -(-E // 256)
    assert got_counts == want_counts and np.array_equal(got_ids, want_ids)


TIES = {"all equal": lambda E: np.full(E, 0x1234ABCD, np.uint32),
        "two values, the threshold inside the run of equals": lambda E: np.where(np.arange(E) % 3 == 0, 5, 0x80000000).astype(np.uint32),
        "0xFFFFFFFF throughout": lambda E: np.full(E, 0xFFFFFFFF, np.uint32)}


@pytest.mark.parametrize("ratio", [1, 100, 200])            # 4, 400, 800 of 1021 negatives: a third of them hold the lower key
@pytest.mark.parametrize("tie", TIES.values(), ids=list(TIES))
def test_a_tie_on_the_key_goes_to_the_lower_replica(fm, tie, ratio):  # noqa: F811
    E = 1025
    keys, positive = tie(E), np.zeros(E, bool)
    positive[[0, 511, 1023, 1024]] = True
    want_ids, want_counts = restated(positive, keys, ratio)
    k = _kernels(fm, E, 1)
    counts = np.add.reduceat(positive.astype(np.int32), np.arange(0, E, 256))
    got_ids, got_counts = _keep(k, ratio, E, positive=_dev(positive.astype(np.int32)), keys=_dev(keys.view(np.int32)),
                                block_counts=_dev(counts.astype(np.int32)))
    assert got_counts == want_counts == (4 + 4 * ratio, 4, 4 * ratio) and np.array_equal(got_ids, want_ids)


@pytest.mark.parametrize("T", [1, 7])
@pytest.mark.parametrize("K", [1, 65, 257])               # (257: a second chunk of kept columns)
@pytest.mark.parametrize("w", [1, 2, 4, 6, 105])
def test_gather_is_fancy_indexing(fm, w, K, T):  # noqa: F811
    """one launch: widths w, 1 (int32), 4 (the 16-byte path) and w again from a base that is NOT 16-byte aligned; fenced"""
    E, rng = 300, np.random.default_rng(w + 10 * K + T)
    keep = np.sort(rng.choice(E, K, replace=False)).astype(np.int32)
    k = _kernels(fm, E, T)
    srcs = [rng.standard_normal((T, E, w)).astype(np.float32), rng.integers(-9, 9, (T, E, 1)).astype(np.int32),
            rng.standard_normal((T, E, 4)).astype(np.float32), rng.standard_normal((T, E, w)).astype(np.float32)]
    pairs, wholes = [], []
    for i, a in enumerate(srcs):
        off = 1 if i == 3 else 0
        src = torch.zeros(a.size + off, dtype=_dev(a).dtype, device=DEV)[off:].view(a.shape)
        src.copy_(_dev(a))
        whole = torch.full((off + T * K * a.shape[2] + 5,), FENCE, dtype=src.dtype, device=DEV)
        pairs.append((src, whole[off:off + T * K * a.shape[2]].view(T, K, a.shape[2])))
        wholes.append(whole)
    before = _counts()
    k.gather_columns(K, pairs, keep_ids=_dev(keep))
    assert _launched_since(before) == {"HipPgGatherColumns": 1}
    for a, (_, dst), whole in zip(srcs, pairs, wholes):
        assert np.array_equal(dst.cpu().numpy().view(np.int32), a[:, keep].view(np.int32))
        outside = torch.cat([whole[:dst.storage_offset()], whole[dst.storage_offset() + dst.numel():]])
        assert bool((outside == FENCE).all())


@pytest.mark.parametrize("entry", pguk.GRADIENTS_ENTRIES)
def test_one_iteration_in_the_trainer(entry, tmp_path):
    """MountainCar, ratio 2, three replicas given done == 2: the update is the kernels', on the restated rule's columns, its
    gradient after Reduce the float64 A2C gradient of exactly those; without the key the same config is the framework's"""
    pol, E, T, extra = "shared", 256, 8, {"neg_pos_env_ratio": 2, "fused_update_gradients": entry}
    tr = _trainer(tmp_path / "k", "mountain_car", E=E, T=T, trainer_extra={**extra, "fused_update_downsample": True})
    ref = _trainer(tmp_path / "f", "mountain_car", E=E, T=T, trainer_extra=extra)
    assert tr.update_path == {pol: "kernels"} and ref.update_path == {pol: "framework"}
    ref.graceful_close()
    tr._generate_rollout_batch()
    tr.done_batch[3, [5, 100, 255]] = 2
    k, pcfg, b = tr._pg_kernels[pol], tr.config["policy"][pol], tr.batch[pol]
    theta = tr._pg_flat[pol].flat.cpu().numpy().copy()
    done = tr.done_batch[:T].cpu().numpy()
    want_ids, want_counts = restated((done == 2).any(axis=0), _keys(E, tr._pg_adam[pol]["step"], tr._seed_words), 2)
    before = _counts()
    metrics = tr._update_model_params(0, True)[pol]
    torch.cuda.synchronize()
    launched = set(STAGES) - {"HipPgGradients"} | {"HipPgGradients" + "Mx" * (entry == "matrix"), *pguk.DOWNSAMPLE_ENTRIES}
    assert _launched_since(before) == {s: 1 for s in launched}
    assert np.array_equal(k.keep_ids[:k.E].cpu().numpy(), want_ids) and (k.E, k.rows) == (9, 72)
    assert (metrics["Num of Positive Sampled Envs"], metrics["Num of Negative Sampled Envs"]) == (3, 6)
    case = pc._case(9, T, pcfg["gamma"], 32, 2, 3, pcfg["entropy_coeff"], pcfg["vf_loss_coeff"], "none")
    inp = {"obs": b["obs"][:T].cpu().numpy()[:, want_ids, 0], "actions": b["actions"][:T].cpu().numpy()[:, want_ids, 0, 0],
           "rewards": b["rewards"][:T].cpu().numpy()[:, want_ids, 0], "done": done[:, want_ids], "theta": theta}
    values = k.values.cpu().numpy()
    want, yard = pc.yardstick(case, inp, values=values), pc.framework(case, inp, torch.float32, DEV, values=values)
    grads = k.grads.cpu().numpy()
    got = {name: grads[lo:hi] for name, (lo, hi) in zip(pc.TENSOR_NAMES, pc.tensor_bounds(32, 2, 3))}
    got.update({name: k.sums[i].item() for i, name in enumerate(pc.SUM_NAMES)})
    _judge(f"downsampled {entry}", got, want, yard, pc.TENSOR_NAMES + pc.SUM_NAMES)
    tr.done_batch[3, [5, 100, 255]] = 0                      # no positive: every replica again, on the same buffers
    tr._update_model_params(1, False)
    assert (k.E, k.rows, k.sampled) == (E, E * T, (0, E)) and bool(torch.isfinite(tr._pg_flat[pol].flat).all())
    tr.graceful_close()
