"""bench.py's --dump-outputs writer and its --steps contract, on CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_dtypes_cap_and_sample(tmp_path, monkeypatch):
    """float32 stays float32, integers become float64 (exact); over the cap, every array keeps the SAME seeded sample of
    replicas (axis 0, or axis 1 of [T, E, ...] batch tensors), and the same arrays give the same files."""
    sys.path.insert(0, ROOT)
    import bench

    E = 50
    obs = np.arange(E * 3 * 4, dtype=np.float32).reshape(E, 3, 4)
    acts = np.arange(E * 3, dtype=np.int32).reshape(E, 3) + (1 << 24) + 1  # not exact in float32
    batch = np.arange(2 * E, dtype=np.float32).reshape(2, E)
    arrays = {"observations": (obs, 0), "sampled_actions": (acts, 0), "batch_obs": (batch, 1)}
    bench.dump_outputs(str(tmp_path / "all"), arrays, E)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert got["observations"].dtype == np.float32 and np.array_equal(got["observations"], obs)
    assert got["sampled_actions"].dtype == np.float64 and np.array_equal(got["sampled_actions"], acts)

    total = obs.nbytes + acts.size * 8 + batch.nbytes
    monkeypatch.setattr(bench, "DUMP_BYTES", total // 4)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays, E, "_rank1")
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert set(a) == {"observations_rank1.npy", "sampled_actions_rank1.npy", "batch_obs_rank1.npy"}
    assert sum(v.nbytes for v in a.values()) <= total // 4
    rows = a["observations_rank1.npy"][:, 0, 0] / 12                     # replica index of every kept row
    assert len(rows) == E // 4 and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["sampled_actions_rank1.npy"][:, 0], acts[rows.astype(int), 0])
    assert np.array_equal(a["batch_obs_rank1.npy"], batch[:, rows.astype(int)])
    assert all(np.array_equal(v, np.load(tmp_path / "b" / f)) for f, v in a.items())


@pytest.mark.parametrize("extra", [["--steps", "0"], ["--mode", "graph", "--steps", "25"]])
def test_steps_is_the_number_of_timed_steps(extra):
    """--steps is never rounded or ignored: a value the benchmark could not time exactly is refused before any work."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 2 and "--steps is the number of timed steps" in out.stderr
