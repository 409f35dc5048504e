"""Host-side replay of the index arithmetic of the fused policy forward's epilogue (csrc/kernels/mlp_forward.h::
mlp_epilogue), in float32 exactly as the kernel computes it (the code object is built with correctly rounded division and
-ffp-contract=off).  Two pieces replace integer division there:

  the stored-outputs copy   32 agent rows of W floats leave the LDS tile as one contiguous run: lane + 64 i -> flat
                            element q, agent a = (int)((q + 0.5f) * (1.0f / W)), column q - a W
  the probability stores    a head of A columns: per_pass = 64 / A agents per store instruction, lane -> (agent of the
                            pass sub = (int)((lane + 0.5f) / A), column lane - sub A), passes a0 = 0, per_pass, ...

For every width the kernel accepts, each (agent, column) pair must be written exactly once and nothing else.  (The
device run is tests/test_gpu_policy_forward_shapes.py.)"""
import numpy as np
import pytest

f32 = np.float32


@pytest.mark.parametrize("W", range(2, 65))
def test_stored_outputs_row_split(W):
    """W = A0 + A1 + 1 in 2 .. 64; every count of valid rows in a tile (a ragged last tile)"""
    inv_w = f32(1.0) / f32(W)
    for rows in (1, 2, 7, 31, 32):
        n = rows * W
        seen = np.zeros((32, 64), np.int64)
        for lane in range(64):
            for q in range(lane, n, 64):
                a = int(f32(f32(q) + f32(0.5)) * inv_w)
                assert a == q // W, (W, q, a)
                col = q - a * W
                assert 0 <= col < W
                seen[a, col] += 1
        assert (seen[:rows, :W] == 1).all() and seen.sum() == n, (W, rows)


@pytest.mark.parametrize("A", range(1, 64))
def test_probability_store_lane_mapping(A):
    """a head of A in 1 .. 63 columns: every agent of the tile (32) and column written once, no lane out of range"""
    per_pass = 64 // A
    seen = np.zeros((32, A), np.int64)
    for lane in range(64):
        sub = int(f32(f32(lane) + f32(0.5)) / f32(A))
        assert sub == lane // A, (A, lane, sub)
        col = lane - sub * A
        assert 0 <= col < A
        for a0 in range(0, 32, per_pass):
            ag = a0 + sub
            if sub < per_pass and ag < 32:
                seen[ag, col] += 1
    assert (seen == 1).all(), (A, np.argwhere(seen != 1)[:5])

