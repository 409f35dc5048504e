"""Cases, input generators and numpy models for the update object's kernels (wd_kernels_update.hsaco) and the trainer's
bookkeeping kernel HipRolloutRecord, launched OFF the geometry `UpdateKernels` / `FusedRolloutTick` fix (256 threads, 4096
rows per block or one block per CU, v_col = W - 1, fresh outputs).  Shared by tests/test_update_kernel_models_host.py (the
models against independent forms, the cases' teeth, their legality) and tests/test_gpu_update_kernel_entries.py (the
launches).  Nothing here touches a GPU.

Section A: kernels with a fixed float32 operation order (the objects are built with -ffp-contract=off): numpy restatements
operation for operation, compared at tolerance 0.
Section B: kernels judged against float64 with a float32 evaluation of the same operation as yardstick,
    err <= max(4 * err_f32, 2e-6 * scale)                                            (`within_bound`)
per launch and result tensor; `bf16x3_product` emulates the matrix-core kernels' arithmetic (the exact three-term bf16 split,
six partial products, float32 accumulation) so that the host test can show that the bound, on THESE inputs, passes the
shipped arithmetic and fails one that drops a term."""
import numpy as np

f32, f64 = np.float32, np.float64
SENTINEL_BITS = 0x7FC0BEEF   # a quiet NaN with a payload: what unwritten output holds, compared byte for byte
HEAD_WIDTHS = (43, 6, 3)     # UpdateKernels.HEAD_WIDTHS (asserted by the host test)


def sentinel(shape):
    return np.full(shape, SENTINEL_BITS, dtype=np.uint32).view(f32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def seq_sum_f32(x, axis=0):
    """float32 sum along `axis` in ascending index order starting from +0.0f (what `float s = 0; for (...) s += x[i]` does)"""
    x = np.asarray(x, f32)
    shape = list(x.shape)
    shape[axis] = 1
    zero = np.zeros(shape, f32)
    return np.take(np.cumsum(np.concatenate([zero, x], axis=axis), axis=axis, dtype=f32), -1, axis=axis)


def within_bound(err, err_f32, scale):
    return err <= max(4.0 * err_f32, 2e-6 * scale)


def judge(got, want64, yard32):
    """(err, err_f32, scale) of one result tensor: largest distance to float64 of the result and of the yardstick"""
    want64 = np.asarray(want64, f64)
    err = float(np.abs(np.asarray(got, f64) - want64).max()) if want64.size else 0.0
    err_f32 = float(np.abs(np.asarray(yard32, f64) - want64).max()) if want64.size else 0.0
    return err, err_f32, float(np.abs(want64).max()) if want64.size else 0.0


# =========================================================================================== A. HipRolloutRecord
RECORD_TICKS, RECORD_ROWS, RECORD_FIRST_ROW, RECORD_SURPLUS = 6, 9, 2, 3
DONE_PATTERNS = {            # `done` of a replica over the 6 ticks
    "two in a row": (0, 0, 1, 1, 0, 0),
    "every tick": (1, 1, 1, 1, 1, 1),
    "value 2": (0, 2, 0, 0, 2, 0),
    "never": (0, 0, 0, 0, 0, 0),
    "tick 0 only": (1, 0, 0, 0, 0, 0),
    "last tick only": (0, 0, 0, 0, 0, 1),
}
_PATTERN_ORDER = tuple(DONE_PATTERNS)   # replica e takes pattern e % 6 of this order: E = 1 and E = 3 still finish twice


class RecordCase:
    def __init__(self, name, N, layout, E, blocks):
        self.name, self.N, self.layout, self.E, self.blocks = name, N, layout, E, tuple(blocks)
        self.seed = 1000 + 7 * N + E

    def slot(self):
        """(slot int32 [N], n_pol_a, n_pol_b): slot[a] = policy * 65536 + index inside the policy"""
        N, a = self.N, np.arange(self.N)
        if self.layout == "one":
            return a.astype(np.int32), N, 0
        if self.layout == "interleaved":       # policy b = every third agent
            is_b = a % 3 == 2
        else:                                  # ("contiguous", n_a): policy a = the first n_a agents
            is_b = a >= self.layout[1]
        slot = np.where(is_b, 65536 + np.cumsum(is_b) - 1, np.cumsum(~is_b) - 1).astype(np.int32)
        return slot, int((~is_b).sum()), int(is_b.sum())

    def pattern_of(self, e):
        return _PATTERN_ORDER[e % len(_PATTERN_ORDER)]

    def inputs(self):
        """per tick: rewards [E + 3, N] float32 of magnitudes 1e-3 .. 1e3 and both signs, done [E + 3] int32"""
        rng = np.random.RandomState(self.seed)
        E3 = self.E + RECORD_SURPLUS
        rewards = (rng.choice([-1.0, 1.0], (RECORD_TICKS, E3, self.N)) * 10.0 ** rng.uniform(-3, 3, (RECORD_TICKS, E3, self.N))).astype(f32)
        done = np.zeros((RECORD_TICKS, E3), np.int32)
        for e in range(self.E):
            done[:, e] = DONE_PATTERNS[self.pattern_of(e)]
        done[:, self.E:] = 1                   # (replicas no block serves)
        return rewards, done

    def initial_state(self):
        """every array the kernel writes: the batches full of the sentinel, the running sums with history in them"""
        rng = np.random.RandomState(self.seed + 1)
        _, na, nb = self.slot()
        E, E3 = self.E, self.E + RECORD_SURPLUS
        return {
            "reward_batch_a": sentinel((RECORD_ROWS, E, na)), "reward_batch_b": sentinel((RECORD_ROWS, E, nb)),
            "done_batch": np.full((RECORD_ROWS, E), -77, np.int32),
            "ep_reward_a": rng.uniform(-5, 5, (E3, na)).astype(f32), "ep_reward_b": rng.uniform(-5, 5, (E3, nb)).astype(f32),
            "ep_sum_a": rng.uniform(-50, 50, E3).astype(f32), "ep_sum_b": rng.uniform(-50, 50, E3).astype(f32),
            "ep_count": rng.randint(0, 4, E3).astype(f32),
            "batch_row": np.full(E3, RECORD_FIRST_ROW, np.int64),
        }


RECORD_CASES = [
    RecordCase("N1-one-E1", 1, "one", 1, [64]),
    RecordCase("N5-one-E37", 5, "one", 37, [64]),
    RecordCase("N60-contiguous-E37", 60, ("contiguous", 5), 37, [64]),
    RecordCase("N105-interleaved-E130", 105, "interleaved", 130, [64, 128, 256]),
    RecordCase("N1100-contiguous-E3", 1100, ("contiguous", 100), 3, [1024]),
]
RECORD_STATE_NAMES = ("reward_batch_a", "reward_batch_b", "done_batch", "ep_reward_a", "ep_reward_b", "ep_sum_a", "ep_sum_b",
                      "ep_count", "batch_row")


def record_model(state, rewards, done, slot, E, summation="f32", sum_policy_of=None):
    """one HipRolloutRecord launch of E blocks on `state` (in place).  summation: "f32" = the kernel's (ascending agent id,
    float32, from 0.0f), "f64" = float64 rounded once (the vacuity check: does the order show?).  sum_policy_of (tests of
    the cases' teeth): the policy whose agents thread p sums instead of p's own."""
    pol, la = slot >> 16, slot & 0xffff
    n_pol = [int((pol == 0).sum()), int((pol == 1).sum())]
    names = [("reward_batch_a", "ep_reward_a", "ep_sum_a"), ("reward_batch_b", "ep_reward_b", "ep_sum_b")]
    for e in range(E):
        t = int(state["batch_row"][e])
        finished = done[e] > 0
        total = np.zeros(len(slot), f32)
        for p in (0, 1):
            if not n_pol[p]:
                continue
            batch, acc, _ = (state[n] for n in names[p])
            mine = pol == p
            r = rewards[e, mine]
            batch[t, e, la[mine]] = r
            total[mine] = acc[e, la[mine]] + r
            acc[e, la[mine]] = f32(0.0) if finished else total[mine]
        state["done_batch"][t, e] = done[e]
        if finished:
            for p in (0, 1):
                if not n_pol[p]:
                    continue
                src = total[pol == (p if sum_policy_of is None else sum_policy_of[p])]
                s = seq_sum_f32(src) if summation == "f32" else f32(src.astype(f64).sum())
                state[names[p][2]][e] = state[names[p][2]][e] + f32(s) / f32(n_pol[p])
            state["ep_count"][e] += f32(1.0)
        state["batch_row"][e] = t + 1
    return state


def record_run_model(case, **kw):
    """the case's 6 launches on the model: final state"""
    slot, _, _ = case.slot()
    rewards, done = case.inputs()
    state = case.initial_state()
    for tick in range(RECORD_TICKS):
        record_model(state, rewards[tick], done[tick], slot, case.E, **kw)
    return state


# =========================================================================================== A. HipDiscountedReturns
class ReturnsCase:
    def __init__(self, T, E, n, W, v_col, block, surplus_blocks=0):
        self.T, self.E, self.n, self.W, self.v_col, self.block = T, E, n, W, v_col, block
        self.grid = -(-E * n // block) + surplus_blocks
        self.name = f"T{T}-E{E}-n{n}-W{W}-v{v_col}-b{block}-g{self.grid}"
        self.seed = 2000 + 31 * T + 7 * E + n + v_col

    def inputs(self):
        """rewards [T, E, n], done [T, E] int32 in {0, 1, 2}, out [T, E, n, W]"""
        rng = np.random.RandomState(self.seed)
        rewards = (rng.standard_normal((self.T, self.E, self.n)) * 3.0).astype(f32)
        done = (rng.randint(0, 3, (self.T, self.E)) * (rng.uniform(size=(self.T, self.E)) < 0.4)).astype(np.int32)
        if self.T * self.E >= 12:   # all three flag values, on the last step too
            done.reshape(-1)[:3] = (0, 1, 2)
            done[-1, :3] = (2, 0, 1)
        out = rng.standard_normal((self.T, self.E, self.n, self.W)).astype(f32)
        return rewards, done, out


RETURNS_CASES = [
    ReturnsCase(1, 1, 1, 3, 2, 64),
    ReturnsCase(5, 3, 86, 6, 5, 256),                       # E * n = 258: one block boundary
    ReturnsCase(7, 61, 9, 43, 42, 128),
    ReturnsCase(7, 61, 9, 43, 0, 64, surplus_blocks=2),
    ReturnsCase(4, 2, 5, 7, 3, 256),                        # a width and a column the trainer never uses
]
RETURNS_GAMMAS = (1.0, 0.97)


def returns_model(rewards, done, out, v_col, gamma):
    """(returns, advantages) [T, E, n]: the recursion of the kernel's comment in float32, ((1 - d) * gamma) * R formed
    before it is added to r; done > 0 counts as done"""
    T = rewards.shape[0]
    gamma = f32(gamma)
    d = (done > 0).astype(f32)[..., None]
    v = np.ascontiguousarray(out[..., v_col])
    one = f32(1.0)
    returns = np.empty_like(rewards)
    R = None
    for t in range(T - 1, -1, -1):
        if t == T - 1:
            R = (d[t] * rewards[t] + (one - d[t]) * v[t]).astype(f32)
        else:
            R = (rewards[t] + ((one - d[t]) * gamma).astype(f32) * R).astype(f32)
        returns[t] = R
    return returns, (returns - v).astype(f32)


# =========================================================================================== A. HipReluBackwardColumnSums
COLSUM_WIDTHS = (16, 32, 64, 128, 256)
COLSUM_GEOMETRIES = [(1, 4096, 1), (3, 1, 3), (70, 64, 2), (333, 100, 4), (64, 64, 3)]   # (R, rows_per_block, grid)


def colsum_inputs(R, C):
    """gx [R, C] of mixed magnitudes, y [R, C] with positives, negatives, exact zeros and negative zeros"""
    rng = np.random.RandomState(3000 + 17 * R + C)
    gx = (rng.standard_normal((R, C)) * 10.0 ** rng.uniform(-2, 2, (R, C))).astype(f32)
    y = rng.standard_normal((R, C)).astype(f32)
    kind = rng.randint(0, 4, (R, C))
    y[kind == 0] = 0.0
    y[kind == 1] = -0.0
    if R * C >= 4:
        y.reshape(-1)[:2] = (0.0, -0.0)
    return gx, y


def colsum_model(gx, y, rows_per_block, grid):
    """(g [R, C], partial [grid, C]) in the kernel's order: thread (row phase rp, column quad) adds its rows r_begin + rp,
    + rows_per_pass, ... sequentially, then the phases are added in ascending rp from 0.0f; rows_per_pass = 1024 / C"""
    R, C = gx.shape
    g = np.where(y > 0, gx, f32(0.0)).astype(f32)
    rpp = 1024 // C
    partial = np.zeros((grid, C), f32)
    for b in range(grid):
        r0, r1 = min(R, b * rows_per_block), min(R, (b + 1) * rows_per_block)
        phases = np.stack([seq_sum_f32(g[r0 + rp:r1:rpp], axis=0) if r0 + rp < r1 else np.zeros(C, f32) for rp in range(rpp)])
        partial[b] = seq_sum_f32(phases, axis=0)
    return g, partial


# ================================================================================ B. the bf16x3 arithmetic, emulated
def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even) as float32; finite inputs"""
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(f32)


def split3(x):
    """the kernels' split (wg_split3 / split_bf16x3): hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid); the
    subtractions are exact in float32"""
    x = np.asarray(x, f32)
    hi = bf16_round(x)
    r1 = (x - hi).astype(f32)
    mid = bf16_round(r1)
    lo = bf16_round((r1 - mid).astype(f32))
    return [hi, mid, lo]


_TERMS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))   # (first, second operand's term), ascending product size


def bf16x3_product(a, b, drop=None):
    """a [m, k] . b [k, n] as the matrix-core kernels form it: six partial products of bf16 terms (each product exact,
    float32 accumulation -- numpy's float32 matmul per partial product, summed in the kernels' ascending order).
    drop = "a" / "b": that operand's third term is missing (bf16x2), the defect the bound must catch."""
    ta, tb = split3(a), split3(b)
    acc = np.zeros((a.shape[0], b.shape[1]), f32)
    for i, j in _TERMS:
        if (drop == "a" and i == 2) or (drop == "b" and j == 2):
            continue
        acc = (acc + ta[i] @ tb[j]).astype(f32)
    return acc


def full_mantissa(rng, shape, exponents=(-1, 0)):
    """positive float32 2^k * m, k drawn from `exponents`, m in [1, 1.25), with a third bf16 term of one sign and nearly the
    largest size it can have: significand bit 2^-8 clear and 2^-9 set (the first term rounds down, the second starts at
    2^-9 and ends at 2^-16), bit 2^-17 clear and 2^-18 .. 2^-23 set (the second term rounds down and leaves 2^-17 -
    2^-23: 6e-6 .. 7.5e-6 of the value).  With operands of one sign nothing cancels, neither in the product nor in what a
    dropped term leaves out, so an arithmetic that drops one is off by ~7e-6 of EVERY result -- over the 2e-6 floor of the
    bound.  Random operands do not reach it: their third terms have both signs and average out over the contraction
    (measured: 1e-7 of the result).  Found necessary by the host test's teeth check."""
    n = int(np.prod(shape))
    mant = (rng.randint(0, 32, n).astype(np.uint32) << 16) | np.uint32(1 << 14) | (rng.randint(0, 128, n).astype(np.uint32) << 7) | np.uint32(0x3F)
    expo = (127 + rng.choice(np.asarray(exponents), n)).astype(np.uint32) << 23
    return (expo | mant).view(f32).reshape(shape).copy()


def relu_like(rng, shape, zero_fraction=0.3):
    """post-ReLU activations: `full_mantissa` values with exact zeros and negative zeros"""
    x = full_mantissa(rng, shape)
    kind = rng.uniform(size=shape)
    x[kind < zero_fraction] = 0.0
    x[kind < zero_fraction / 3] = -0.0
    return x


def slab_rows(R, rows_per_block, grid):
    """[(first, last + 1) row of block b]: empty for blocks past R"""
    return [(min(R, b * rows_per_block), min(R, (b + 1) * rows_per_block)) for b in range(grid)]


# ---------------------------------------------------------------------------------- B. HipHeadBackward_W* / Bx3_W*
HEAD_VECTOR_GEOMETRIES = [(1, 4096, 1), (33, 32, 2), (100, 40, 3), (70, 5, 14), (64, 32, 4)]
HEAD_VECTOR_CASES = [(W, C, g) for W in HEAD_WIDTHS for C in (64, 128, 256) for g in HEAD_VECTOR_GEOMETRIES[:3]] + \
                    [(W, C, g) for W, C in ((43, 64), (3, 256)) for g in HEAD_VECTOR_GEOMETRIES[3:]]
HEAD_BX3_GEOMETRIES = [(32, 32, 1), (64, 64, 1), (96, 96, 1), (160, 64, 3), (160, 160, 1), (128, 32, 6)]
HEAD_BX3_CASES = [(W, g) for W in HEAD_WIDTHS for g in HEAD_BX3_GEOMETRIES]
HEAD_BX3_STAGES, HEAD_BX3_STEP_ROWS = 3, 32


def head_inputs(R, W, C, one_sign=False):
    """g3 [R, W], w3 [W, C], h2 [R, C] (post-ReLU).  one_sign: the bf16x3 cases' operands (`full_mantissa`)"""
    rng = np.random.RandomState(4000 + 13 * R + 5 * W + C)
    if one_sign:
        return full_mantissa(rng, (R, W)), full_mantissa(rng, (W, C), (-3, -2)), relu_like(rng, (R, C))
    g3 = rng.standard_normal((R, W)).astype(f32)
    w3 = (rng.standard_normal((W, C)) * 0.2).astype(f32)
    h2 = np.maximum(rng.standard_normal((R, C)), 0.0).astype(f32)
    h2[rng.uniform(size=(R, C)) < 0.1] = -0.0
    return g3, w3, h2


def head_reference(g3, w3, h2, rows_per_block, grid, dtype=f64, product=None, db3_waves=False):
    """{g2 [R, C], db2_part [grid, C], dw3_part [grid, W, C] (, db3_part [4 grid, W])} per block of rows, evaluated in
    `dtype`; `product(a, b)` replaces the matrix product (the bf16x3 emulation).  db3_part: wavefront w of a block sums
    rows 8 w .. 8 w + 7 of each of its 32-row steps."""
    mm = product or (lambda a, b: a @ b)
    R, W = g3.shape
    C = h2.shape[1]
    a, w, h = g3.astype(dtype), w3.astype(dtype), h2.astype(dtype)
    g2 = np.where(h2 > 0, mm(a, w), 0).astype(dtype) if R else np.zeros((0, C), dtype)
    res = {"g2": g2, "db2_part": np.zeros((grid, C), dtype), "dw3_part": np.zeros((grid, W, C), dtype)}
    if db3_waves:
        res["db3_part"] = np.zeros((grid * 4, W), dtype)
    for b, (r0, r1) in enumerate(slab_rows(R, rows_per_block, grid)):
        if r0 == r1:
            continue
        res["db2_part"][b] = g2[r0:r1].sum(0, dtype=dtype)
        res["dw3_part"][b] = mm(np.ascontiguousarray(a[r0:r1].T), h[r0:r1])
        if db3_waves:
            local = np.arange(r1 - r0)
            for wv in range(4):
                res["db3_part"][4 * b + wv] = a[r0:r1][(local % 32) // 8 == wv].sum(0, dtype=dtype)
    return res


def head_bx3_lds_bytes(W):
    """dynamic LDS of HipHeadBackwardBx3_W<W>, from the kernel's constants: stages of (the step's g3 in whole KB pieces per
    wavefront + 32 rows of 260 floats of h2)"""
    ks, ot = (W + 15) // 16, (W + 31) // 32
    g3_max = 31 * W + max(32 * ot, 16 * ks) - 1
    pieces_per_wave = (g3_max // 256 + 1 + 3) // 4
    return HEAD_BX3_STAGES * 4 * (1024 * pieces_per_wave + 32 * 260)


# ---------------------------------------------------------------------------------- B. HipWeightGradBx3_256x{256,96}
WEIGHT_GRAD_GEOMETRIES = [(32, 32, 1), (64, 64, 1), (96, 96, 1), (288, 128, 3), (64, 32, 4)]
WEIGHT_GRAD_CASES = [(256, -1, g) for g in WEIGHT_GRAD_GEOMETRIES] + \
                    [(ci, ones, g) for ci in (1, 3, 4, 71, 95) for ones in (-1, ci) for g in WEIGHT_GRAD_GEOMETRIES]
WEIGHT_GRAD_STAGES, WEIGHT_GRAD_STEP_ROWS = 4, 16


def weight_grad_inputs(R, ci):
    """G [R, 256] with whole zero rows (as masked gradients have), X [R, ci]"""
    rng = np.random.RandomState(5000 + 3 * R + ci)
    G = full_mantissa(rng, (R, 256))
    zero = rng.uniform(size=R) < 0.15
    zero[[1, 17]], zero[[0, R - 1]] = True, False     # a zero row in both steps of a slab's first pair; its ends are not
    G[zero] = 0.0
    return G, full_mantissa(rng, (R, ci))


def weight_grad_reference(G, X, ones_col, rows_per_block, grid, dtype=f64, product=None):
    """partial [grid, 256, ci (+ 1: the ones column's result, the column sums of G)] per block of rows"""
    mm = product or (lambda a, b: a @ b)
    R, ci = X.shape
    Xa = np.concatenate([X, np.ones((R, 1), f32)], axis=1) if ones_col >= 0 else X
    g, x = G.astype(dtype), Xa.astype(dtype)
    out = np.zeros((grid, 256, Xa.shape[1]), dtype)
    for b, (r0, r1) in enumerate(slab_rows(R, rows_per_block, grid)):
        if r0 < r1:
            out[b] = mm(np.ascontiguousarray(g[r0:r1].T), x[r0:r1])
    return out


def weight_grad_lds_bytes(cip):
    """dynamic LDS of HipWeightGradBx3_256x<cip>: stages of 16 staged rows of G (260 floats each) and of X (the same, or
    a flat run of 2048 floats for the narrow one)"""
    return WEIGHT_GRAD_STAGES * 4 * (16 * 260 + (16 * 260 if cip == 256 else 2048))


# ---------------------------------------------------------------------------------- B. HipLinearMaskBackwardBx3_<C>
MASK_ROWS = (1, 31, 32, 33, 257)
# threads per block: a weight chunk of 6 * C / 32 KB pieces is fetched by all wavefronts, `pieces / wavefronts` each
# (mlp_fetch_kb): 48 and 24 pieces divide over 8 and over 4 wavefronts, so C = 128 / 256 also run at 256 threads (the product
# uses 512); C = 64 has 12 pieces, which 8 wavefronts do not divide: 256 threads only
MASK_BLOCKS = {64: (256,), 128: (512, 256), 256: (512, 256)}
MASK_CASES = [(C, R) for C in (64, 128, 256) for R in MASK_ROWS]


def mask_inputs(R, C):
    """g_in [R, C], w [C out, C in], h [R, C] (post-ReLU)"""
    rng = np.random.RandomState(6000 + 11 * R + C)
    return full_mantissa(rng, (R, C)), full_mantissa(rng, (C, C), (-5, -4)), relu_like(rng, (R, C))


def mask_reference(g_in, w, h, dtype=f64, product=None):
    mm = product or (lambda a, b: a @ b)
    return np.where(h > 0, mm(g_in.astype(dtype), w.astype(dtype)), 0).astype(dtype)


def mask_lds_bytes(C):
    return 3 * (C // 32) * 6144


# ---------------------------------------------------------------------------------- B. HipPolicyGradientHead
PG_HEADS = ([2], [5], [21, 21], [63])
PG_ROWS = (1, 255, 256, 257, 600)
PG_ENT_COEFF, PG_VF_COEFF = 0.03, 0.7


def pg_inputs(heads, R):
    """out [R, W] with logits of magnitude 1 .. 300 per row and a value column, actions [R, heads] int32 drawn from the
    float64 probabilities, adv [R] (mean 0.75, both signs), ret [R]"""
    rng = np.random.RandomState(7000 + 5 * sum(heads) + R)
    W = sum(heads) + 1
    spread = 10.0 ** (rng.uniform(size=(R, 1)) * np.log10(300.0))
    out = ((rng.uniform(size=(R, W)) * 2.0 - 1.0) * spread).astype(f32)
    out[:, -1] = rng.standard_normal(R).astype(f32)
    actions = np.zeros((R, len(heads)), np.int32)
    start = 0
    for k, A in enumerate(heads):
        z = out[:, start:start + A].astype(f64)
        p = np.exp(z - z.max(1, keepdims=True))
        cdf = np.cumsum(p / p.sum(1, keepdims=True), axis=1)
        actions[:, k] = np.minimum((cdf < rng.uniform(size=(R, 1))).sum(1), A - 1)
        start += A
    # advantages with a mean, as unnormalised ones have: a block's sum of them (and of logp * adv) is then a sum, not the
    # small difference of large numbers, which a bound relative to the sum itself could not judge
    adv = (rng.standard_normal(R) + 0.75).astype(f32)
    return out, actions, adv, rng.standard_normal(R).astype(f32)


def pg_reference(out, actions, adv, ret, heads, ent_coeff=PG_ENT_COEFF, vf_coeff=PG_VF_COEFF):
    """float64 closed forms of the kernel's comment: (grad [R, W], sums [blocks of 256 rows, 4] = sum logp(a) * adv, sum of
    the heads' entropies, sum (v - ret)^2, sum adv)"""
    R, W = out.shape
    z, a, rt = out.astype(f64), adv.astype(f64), ret.astype(f64)
    grad = np.zeros((R, W), f64)
    logp_taken, ent = np.zeros(R), np.zeros(R)
    start = 0
    for k, A in enumerate(heads):
        zh = z[:, start:start + A]
        sh = zh - zh.max(1, keepdims=True)
        lp = sh - np.log(np.exp(sh).sum(1, keepdims=True))
        p = np.exp(lp)
        H = -(p * lp).sum(1)
        onehot = np.arange(A)[None, :] == actions[:, k:k + 1]
        grad[:, start:start + A] = (a[:, None] * (p - onehot) + ent_coeff * p * (lp + H[:, None])) / R
        logp_taken += lp[np.arange(R), actions[:, k]]
        ent += H
        start += A
    d = z[:, -1] - rt
    grad[:, -1] = 2.0 * vf_coeff * d / R
    per_row = np.stack([logp_taken * a, ent, d * d, a], axis=1)
    blocks = -(-R // 256)
    sums = np.stack([per_row[256 * b:256 * (b + 1)].sum(0) for b in range(blocks)])
    return grad, sums
