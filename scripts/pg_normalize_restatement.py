"""csrc/kernels/pg_normalize.hip restated in numpy float32, in the kernel's own order (no GPU), on the inputs of
tests/test_gpu_pg_normalize.py: per shape and switch pair, err / err_f32 against the float64 yardstick under that file's
bound -- for the kernel's two-pass chunk moments, and for a ONE-PASS variant (M2 = sum x^2 - (sum x)^2 / n in the same
summation order), which must fall outside the bound.

    python scripts/pg_normalize_restatement.py [seed ...]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import pg_update_cases as pc  # noqa: E402
from tests import test_gpu_pg_normalize as tn  # noqa: E402

f32 = np.float32
THREADS, PER_LANE = 256, 16
CHUNK = THREADS * PER_LANE


def block_sum(values):
    """values [count <= 4096] of one chunk -> the block's float32 sum: lanes in k order from +0, the xor butterfly over
    each wavefront, the four wavefronts in order from +0"""
    padded = np.zeros(CHUNK, f32)
    padded[:values.size] = values
    lane = np.zeros(THREADS, f32)
    for k in range(PER_LANE):
        lane = lane + padded[k * THREADS:(k + 1) * THREADS]
    waves = lane.reshape(THREADS // 64, 64)
    for step in (1, 2, 4, 8, 16, 32):
        waves = waves + waves[:, np.arange(64) ^ step]
    s = f32(0)
    for w in range(THREADS // 64):
        s = s + waves[w, 0]
    return s


def chunk_moments(x, one_pass):
    n = f32(x.size)
    mean = block_sum(x) / n
    if one_pass:
        s = block_sum(x)
        return mean, block_sum(x * x) - s * s / n
    d = x - mean
    return mean, block_sum(d * d)


def tick_mean_std(x, one_pass):
    """x [C] float32 -> (mean, std) by the merge of the chunks' partials in ascending chunk order"""
    C = x.size
    mean, m2 = chunk_moments(x[:CHUNK], one_pass)
    n_a = f32(min(CHUNK, C))
    for first in range(CHUNK, C, CHUNK):
        mean_b, m2_b = chunk_moments(x[first:first + CHUNK], one_pass)
        n_b = f32(min(CHUNK, C - first))
        n = n_a + n_b
        delta = mean_b - mean
        mean = mean + delta * (n_b / n)
        m2 = m2 + m2_b + delta * delta * (n_a * n_b / n)
        n_a = n
    return mean, np.sqrt(m2 / f32(C - 1), dtype=f32)


def normalise(x, one_pass=False):
    out = np.empty_like(x)
    with np.errstate(invalid="ignore"):
        for t in range(x.shape[0]):
            mean, std = tick_mean_std(x[t].reshape(-1), one_pass)
            out[t] = (x[t] - mean) / (std + f32(1e-10))
    return out


def main(seeds):
    for seed in seeds:
        worst = {False: 0.0, True: 0.0}
        outside = {False: [], True: []}
        for shape in tn.SHAPES:
            inp = tn.inputs(shape, seed)
            for switches in tn.SWITCHES:
                want, yard = tn.yardstick(inp, *switches), tn.framework32(inp, *switches)
                for one_pass in (False, True):
                    got = tn.yardstick(inp, *switches, normalise=lambda x: normalise(x, one_pass), cast=lambda a: a)
                    for key in want:
                        g = np.nan_to_num(np.asarray(got[key], np.float64), nan=1e30).reshape(-1)
                        ok, err, err_f32, scale, ratio = pc.compare(g, want[key].reshape(-1), np.asarray(yard[key]).reshape(-1))
                        worst[one_pass] = max(worst[one_pass], ratio)
                        if not ok:
                            outside[one_pass].append((shape, switches, key, f"{err:.2e}", f"{max(4 * err_f32, 2e-6 * scale):.2e}"))
        print(f"seed {seed}: two-pass worst err / err_f32 {worst[False]:.2f}, outside the bound: {outside[False] or 'none'}")
        print(f"seed {seed}: ONE-PASS worst err / err_f32 {worst[True]:.1f}, outside the bound in {len(outside[True])} of "
              f"{sum(len(tn.yardstick(tn.inputs(s, seed), *sw)) for s in tn.SHAPES for sw in tn.SWITCHES)} results")


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [tn.SEED])
