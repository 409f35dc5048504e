"""Cases, band layouts, models and checks for the update and record kernels at element offsets past 2^30 (= byte offset
2^32), 2^31 and 2^32: shared by tests/test_big_offset_cases_host.py (the layouts at the real boundaries, the checks' teeth
against planted wraps at scaled-down boundaries) and tests/test_gpu_big_offsets.py (the launches).  Nothing here touches a GPU.

The scheme.  A float64 reference over 1e7 .. 1e8 rows is neither affordable nor needed: every big tensor is ZERO except
for BANDS of consecutive rows -- at row 0, around each boundary row floor(boundary / row width) the tensor reaches (a
boundary inside a row counts), and at the ragged end -- which hold seeded data of `tests/update_kernel_cases.py`'s
generators, different in every band.  Outputs start as `uk.SENTINEL_BITS`.  Then
  * row-local outputs: band rows against the model of those rows alone (section A kernels bit for bit, section B under
    `uk.within_bound` against float64 with a numpy float32 evaluation as yardstick); every other row equal, bit for bit, to
    what the kernel makes of an all-zero row; no sentinel left.  A write that wrapped shows twice (a sentinel behind the
    boundary, band data in front of it), a read that wrapped meets zeros or another band's data;
  * reductions: zero rows add exactly 0, so totals (and the partials of blocks that hold a band) are judged by float64
    over the band rows alone.
A `Scale` carries the three boundaries, so the SAME case builders and checks run at 2^10 / 2^11 / 2^12 elements on the host
against numpy stand-ins whose flat offsets go through a pluggable map (`mutation`).

A check reads results through a store (`HostStore` here, a device store in the GPU file):
    rows(name, r0, r1) -> numpy rows;  sentinels(name) -> count of sentinel words;
    mismatch_outside(name, bands, pattern) -> count of words in rows outside `bands` that differ from `pattern` (None: zero bits)
"""
import numpy as np

from tests import update_kernel_cases as uk

f32, f64 = np.float32, np.float64
CAP_BYTES = 64 * 10 ** 9          # device memory a case may fill
BOUNDARIES = ("b30", "b31", "b32")


class Scale:
    """the boundaries in elements; `real`: the kernels' geometry (units of rows) as launched, else 1-row units"""

    def __init__(self, name, e30, e31, e32, real):
        self.name, self.e, self.real = name, {"b30": e30, "b31": e31, "b32": e32}, real
        self.extra = 4096 + 7 if real else 7      # rows behind the last boundary row (4096: a wrapper's rows per block)

    def unit(self, rows):
        return rows if self.real else 1

    def halo(self, unit):
        """rows of a band on each side of its boundary row: two units hold a whole ALIGNED unit wherever they start"""
        return 2 * unit if self.real else 1

    def tail(self, unit):
        return 2 * unit + 32 if self.real else 2  # (+ 32: the R % 32 rows a wrapper finishes on the host)


REAL = Scale("real", 2 ** 30, 2 ** 31, 2 ** 32, True)
SMALL = Scale("small", 2 ** 10, 2 ** 11, 2 ** 12, False)


def mutation(kind, scale):
    """flat element offsets -> (offsets the access goes to, access happens at all).  "u32": the offset mod 2^32 (an unsigned
    32-bit element index); "s32": a signed one -- [2^31, 2^32) is negative: a read of zeros / a dropped write, never an
    out-of-range access; "byte": a 32-bit BYTE offset = the element offset mod 2^30"""
    e = scale.e
    if kind == "identity":
        return lambda o: (o, np.ones(o.shape, bool))
    if kind == "u32":
        return lambda o: (o % e["b32"], np.ones(o.shape, bool))
    if kind == "s32":
        return lambda o: (o % e["b32"], o % e["b32"] < e["b31"])
    assert kind == "byte", kind
    return lambda o: (o % e["b30"], np.ones(o.shape, bool))


MUTATIONS = {"u32": "b32", "s32": "b31", "byte": "b30"}   # the boundary a tensor must cross for the mutation to bite


class Layout:
    """R rows; raw bands [(first, last + 1, label)] as claimed, `bands` = the same merged where they touch (scaled-down
    boundaries are a few rows apart); band data = one array of `nb` rows, band k holding rows starts[k] .. of it"""

    def __init__(self, R, raw):
        self.R, self.raw = R, [(max(0, a), min(R, b), label) for a, b, label in raw if max(0, a) < min(R, b)]
        merged = []
        for a, b, _ in sorted(self.raw):
            if merged and a <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], b)
            else:
                merged.append([a, b])
        self.bands = [tuple(m) for m in merged]
        self.starts = np.concatenate([[0], np.cumsum([b - a for a, b in self.bands])]).astype(np.int64)
        self.nb = int(self.starts[-1])

    def gaps(self):
        edges = [0] + [x for band in self.bands for x in band] + [self.R]
        return [(edges[i], edges[i + 1]) for i in range(0, len(edges), 2) if edges[i] < edges[i + 1]]

    def host_rows(self, data, r0, r1):
        """rows r0 .. r1 - 1 of the tensor whose band data is `data` [nb, ...]: zeros outside the bands"""
        out = np.zeros((r1 - r0,) + data.shape[1:], data.dtype)
        for (a, b), k in zip(self.bands, self.starts):
            lo, hi = max(a, r0), min(b, r1)
            if lo < hi:
                out[lo - r0:hi - r0] = data[k + lo - a:k + hi - a]
        return out

    def blocks(self, rows_per_block):
        """sorted block indices that hold band rows"""
        return sorted({b for a, z in self.bands for b in range(a // rows_per_block, (z - 1) // rows_per_block + 1)})


def _ragged(R):
    return R + 1 if R % 32 == 0 else R


# =========================================================================================================== host store
class Flat:
    """a flat host tensor whose accesses by the stand-ins go through `mapper`; the test's own reads and writes do not"""

    def __init__(self, n, dtype, mapper, sentinel=False):
        self.a = np.zeros(n, dtype)
        if sentinel:
            self.a.view(np.uint32)[:] = uk.SENTINEL_BITS
        self.mapper = mapper

    def load(self):
        m, ok = self.mapper(np.arange(self.a.size, dtype=np.int64))
        v = self.a[m]
        v[~ok] = 0
        return v

    def save(self, values, offsets=None):
        o = np.arange(self.a.size, dtype=np.int64) if offsets is None else np.asarray(offsets, np.int64)
        m, ok = self.mapper(o)
        self.a[m[ok]] = np.asarray(values, self.a.dtype).reshape(-1)[ok]


class HostStore:
    def __init__(self, layout, maps=None):
        self.layout, self.maps, self.t, self.w = layout, maps or {}, {}, {}
        self.identity = lambda o: (o, np.ones(o.shape, bool))

    def add(self, name, width, data=None, dtype=f32, rows=None):
        """an input (`data`: its band rows) or, without data, an output full of the sentinel"""
        R = self.layout.R if rows is None else rows
        t = Flat(R * width, dtype, self.maps.get(name, self.identity), sentinel=data is None)
        if data is not None:
            t.a[:] = self.layout.host_rows(np.asarray(data, dtype).reshape(self.layout.nb, width), 0, R).reshape(-1)
        self.t[name], self.w[name] = t, width
        return t

    def load(self, name):
        return self.t[name].load().reshape(-1, self.w[name])

    def save(self, name, values):
        self.t[name].save(values)

    def rows(self, name, r0, r1):
        w = self.w[name]
        return self.t[name].a[r0 * w:r1 * w].reshape(r1 - r0, w).copy()

    def sentinels(self, name):
        return int((self.t[name].a.view(np.uint32) == uk.SENTINEL_BITS).sum())

    def mismatch_outside(self, name, bands, pattern=None):
        w = self.w[name]
        a = self.t[name].a.view(np.uint32).reshape(-1, w)
        keep = np.ones(a.shape[0], bool)
        for r0, r1 in bands:
            keep[r0:r1] = False
        want = np.zeros(w, np.uint32) if pattern is None else uk.bits(np.asarray(pattern)).reshape(w)
        return int((a[keep] != want).sum())


# =============================================================================================================== checks
class Verdict:
    """collects the err / err_f32 of a case's result tensors and every failed condition; `close` raises on any"""

    def __init__(self, case):
        self.case, self.ratios, self.failures = case, {}, []

    def require(self, ok, *what):
        if not ok:
            self.failures.append(what)

    def judge(self, key, got, want64, yard32):
        got = np.asarray(got)
        err, err_f32, scale = uk.judge(got, want64, yard32)
        ratio = err / err_f32 if err_f32 else (0.0 if err == 0.0 else float("inf"))
        self.ratios[key] = max(self.ratios.get(key, 0.0), ratio)
        self.require(bool(np.isfinite(got).all()) and uk.within_bound(err, err_f32, scale), key, err, err_f32, scale)

    def exact(self, key, got, want):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        self.require(got.shape == want.shape and np.array_equal(uk.bits(got), uk.bits(want)), key, "not bit for bit")

    def close(self):
        assert not self.failures, (self.case, self.failures[:6], len(self.failures))
        return self.ratios

    def report(self):
        return f"{self.case}: worst err / err_f32 " + ", ".join(f"{k} {v:.2f}" for k, v in self.ratios.items())


def _row_local(v, store, layout, name, want=None, yard=None, exact=None, pattern=None, bands=None):
    """output `name`: no sentinel, rows outside the bands = `pattern` (None: zero bits), band rows against the model"""
    bands = layout.bands if bands is None else bands
    v.require(store.sentinels(name) == 0, name, "sentinel words left", store.sentinels(name))
    bad = store.mismatch_outside(name, bands, pattern)
    v.require(bad == 0, name, "words outside the bands differ from an all-zero row's result", bad)
    got = np.concatenate([store.rows(name, a, b) for a, b in bands])
    if exact is not None:
        v.exact(name, got, exact)
    else:
        v.judge(name, got, want, yard)
    return got


class RowsCase:
    """a kernel whose big tensors share one row index.  widths {tensor: row width}; outputs; claims [(tensor, boundary)]:
    the boundaries the case puts under test; unit: rows of the kernel's block / tile / step (real geometry)"""
    name, unit, widths, outputs, claims, small_bytes = None, 32, {}, (), (), 0

    def __init__(self, scale):
        self.scale = scale
        self.boundary_rows = {(t, b): scale.e[b] // self.widths[t] for t, b in self.claims}
        self.R = _ragged(max(self.boundary_rows.values()) + scale.extra)
        halo = scale.halo(self.unit)
        rows = sorted(set(self.boundary_rows.values()))      # (tensors of one width share their boundary rows: one band)
        self.layout = Layout(self.R, self.first_bands(halo) + [(r - halo, r + halo + 1, "boundary") for r in rows]
                             + [(self.R - scale.tail(self.unit), self.R, "end")])

    def first_bands(self, halo):
        return [(0, halo, "row 0")]

    def bytes(self):
        return 4 * self.R * sum(self.widths.values()) + self.small_bytes

    def reach(self, tensor, boundary):
        """does the tensor hold an element at or past the boundary at all?"""
        return self.R * self.widths[tensor] > self.scale.e[boundary]

    def not_crossed(self):
        return sorted((t, b) for t in self.widths for b in BOUNDARIES if (t, b) not in self.claims)

    def gen_rows(self):
        return max(self.layout.nb, 32)   # (a generator of update_kernel_cases.py needs 18 rows)


# ------------------------------------------------------------------------------------------ B. HipPolicyGradientHead
def pg_eval(out, actions, adv, ret, heads, inv_R, dtype, ent_coeff=uk.PG_ENT_COEFF, vf_coeff=uk.PG_VF_COEFF):
    """the closed forms of `uk.pg_reference` for SOME rows of a batch whose size enters as inv_R, in `dtype`:
    (grad [n, W], per row [n, 4] = logp(a) * adv, sum of entropies, (v - ret)^2, adv)"""
    n = out.shape[0]
    z, a, rt = out.astype(dtype), adv.astype(dtype), ret.astype(dtype)
    inv, ent_coeff, vf_coeff = dtype(inv_R), dtype(ent_coeff), dtype(vf_coeff)
    grad = np.zeros(z.shape, dtype)
    logp_taken, ent = np.zeros(n, dtype), np.zeros(n, dtype)
    start = 0
    for k, A in enumerate(heads):
        zh = z[:, start:start + A]
        sh = zh - zh.max(1, keepdims=True)
        lp = sh - np.log(np.exp(sh).sum(1, keepdims=True, dtype=dtype))
        p = np.exp(lp)
        H = -(p * lp).sum(1, dtype=dtype)
        onehot = (np.arange(A)[None, :] == actions[:, k:k + 1]).astype(dtype)
        grad[:, start:start + A] = (a[:, None] * (p - onehot) + ent_coeff * p * (lp + H[:, None])) * inv
        logp_taken += lp[np.arange(n), actions[:, k]]
        ent += H
        start += A
    d = z[:, -1] - rt
    grad[:, -1] = dtype(2.0) * vf_coeff * d * inv
    return grad, np.stack([logp_taken * a, ent, d * d, a], axis=1)


def block_sums(per_row, r0, rows_per_block, dtype):
    """[blocks, k]: per_row = rows r0 .. (r0 a multiple of rows_per_block) summed per block"""
    assert r0 % rows_per_block == 0
    return np.stack([per_row[i:i + rows_per_block].sum(0, dtype=dtype) for i in range(0, per_row.shape[0], rows_per_block)])


PG_SUM_NAMES = ("logp_adv", "entropy", "vf", "adv")


class PolicyGradientHeadCase(RowsCase):
    """out / grad [R, 43], heads [21, 21], blocks of 256 rows.  Row 1 is left zero: its gradient is what every row outside
    the bands must equal bit for bit, so the first band is row 0 and rows 2 .. ; R < 2^31 as the kernel's `int R` requires"""
    name, unit, heads = "HipPolicyGradientHead", 256, [21, 21]
    widths = {"out": 43, "grad": 43}
    outputs = ("grad",)
    claims = tuple((t, b) for t in ("out", "grad") for b in BOUNDARIES)

    def __init__(self, scale):
        super().__init__(scale)
        self.block = scale.unit(256)
        self.blocks = -(-self.R // self.block)
        self.small_bytes = 4 * (4 * self.R + 4 * self.blocks)    # actions [R, 2], adv, ret, sums
        assert self.R < 2 ** 31

    def first_bands(self, halo):
        return [(0, 1, "row 0"), (2, halo, "row 0")]

    def inputs(self):
        out, actions, adv, ret = uk.pg_inputs(self.heads, self.gen_rows())
        nb = self.layout.nb
        return {"out": out[:nb], "actions": actions[:nb], "adv": adv[:nb, None], "ret": ret[:nb, None]}

    def standin(self, maps):
        """the kernel as numpy float32, whole (scaled-down) tensors through the maps: (store, per-block sums)"""
        x, lay = self.inputs(), self.layout
        s = HostStore(lay, maps)
        s.add("out", 43, x["out"])
        s.add("grad", 43)
        full = {k: lay.host_rows(x[k], 0, self.R) for k in ("actions", "adv", "ret")}
        grad, per_row = pg_eval(s.load("out"), full["actions"], full["adv"][:, 0], full["ret"][:, 0], self.heads,
                                f32(1.0 / self.R), f32)
        s.save("grad", grad)
        return s, block_sums(per_row, 0, self.block, f32)

    def check(self, store, sums):
        """sums: the launch's per-block [blocks, 4]"""
        v, lay, x, blk = Verdict(self.name), self.layout, self.inputs(), self.block
        v.require(store.sentinels("grad") == 0, "grad", "sentinel words left")
        bad = store.mismatch_outside("grad", lay.bands, store.rows("grad", 1, 2))
        v.require(bad == 0, "grad", "words outside the bands differ from row 1's (an all-zero row's) gradient", bad)
        band_blocks = lay.blocks(blk)
        for b in band_blocks:         # whole blocks that hold band rows: their zero rows (row 1 among them) are judged too
            r0, r1 = b * blk, min(self.R, (b + 1) * blk)
            args = [lay.host_rows(x[k], r0, r1) for k in ("out", "actions", "adv", "ret")]
            args[2], args[3] = args[2][:, 0], args[3][:, 0]
            g64, p64 = pg_eval(*args, self.heads, 1.0 / self.R, f64)
            g32, p32 = pg_eval(*args, self.heads, f32(1.0 / self.R), f32)
            v.judge("grad", store.rows("grad", r0, r1), g64, g32)
            for i, n in enumerate(PG_SUM_NAMES):
                v.judge(n, sums[b, i], p64[:, i].sum(), p32[:, i].sum(dtype=f32))
        others = np.setdiff1d(np.arange(self.blocks), band_blocks)
        zero = [np.zeros((blk, w), d) for w, d in ((43, f32), (2, np.int32))] + [np.zeros(blk, f32)] * 2
        p64 = pg_eval(*zero, self.heads, 1.0 / self.R, f64)[1]
        p32 = pg_eval(*zero, self.heads, f32(1.0 / self.R), f32)[1]
        for i, n in enumerate(PG_SUM_NAMES):
            v.judge(n + " of a zero block", sums[others[0], i], p64[:, i].sum(), p32[:, i].sum(dtype=f32))
        v.require(bool((uk.bits(sums[others]) == uk.bits(sums[others[:1]])).all()), "sums", "a block of zero rows differs from another")
        return v


# ------------------------------------------------------------------------------------------ A. HipDiscountedReturns
class DiscountedReturnsCase:
    """rewards / returns / advantages [T, E, n] and out [T, E, n, 43] share the row index at = t * E * n + i; a band is a run
    of chains i at EVERY t.  Only `out` is big: chain i meets the boundary row r at t = r // (E n) where i = r % (E n)"""
    name, unit, T, W, gamma = "HipDiscountedReturns", 256, 5, 43, 0.99
    widths = {"out": 43}
    claims = tuple(("out", b) for b in BOUNDARIES)
    outputs = ("returns", "advantages")

    def __init__(self, scale):
        self.scale = scale
        self.E, self.n = (200001, 100) if scale.real else (7, 3)
        S = self.S = self.E * self.n
        self.R = self.T * S
        self.boundary_rows = {(t, b): scale.e[b] // self.W for t, b in self.claims}
        halo = scale.halo(self.unit)
        chains = Layout(S, [(0, halo, "chain 0")]
                        + [(r % S - halo, r % S + halo + 1, f"{t} {b}") for (t, b), r in sorted(self.boundary_rows.items())]
                        + [(S - scale.tail(self.unit), S, "end")])
        self.chains = chains
        self.layout = Layout(self.R, [(t * S + a, t * S + b, f"t {t}") for t in range(self.T) for a, b in chains.bands])

    def bytes(self):
        return 4 * self.R * (43 + 3) + 4 * self.T * self.E

    def reach(self, tensor, boundary):
        return self.R * 43 > self.scale.e[boundary]

    def not_crossed(self):
        return []

    def inputs(self):
        """band data in the row order of `layout` (t outermost): rewards [nb, 1], out [nb, 43]; done [T, E] whole"""
        nc = self.chains.nb
        rewards, _, out = uk.ReturnsCase(self.T, nc, 1, self.W, self.W - 1, 256).inputs()
        done = np.zeros((self.T, self.E), np.int32)
        order = [uk.DONE_PATTERNS[k][:self.T] if k == "tick 0 only" else uk.DONE_PATTERNS[k][-self.T:] for k in uk.DONE_PATTERNS]
        for a, b in self.chains.bands:    # the replicas of the band chains: flags at t = 0, mid-batch, T - 1, and value 2
            for e in range(a // self.n, (b - 1) // self.n + 1):
                done[:, e] = order[e % len(order)]
        return {"rewards": rewards.reshape(self.T * nc, 1), "out": out.reshape(self.T * nc, self.W), "done": done}

    def standin(self, maps):
        x, lay = self.inputs(), self.layout
        s = HostStore(lay, maps)
        s.add("out", 43, x["out"])
        s.add("rewards", 1, x["rewards"])
        s.add("returns", 1)
        s.add("advantages", 1)
        shape = (self.T, self.E, self.n)
        ret, adv = uk.returns_model(s.load("rewards").reshape(shape), x["done"], s.load("out").reshape(shape + (43,)), 42, self.gamma)
        s.save("returns", ret)
        s.save("advantages", adv)
        return s, None

    def check(self, store, _=None):
        v, x, nc, T = Verdict(self.name), self.inputs(), self.chains.nb, self.T
        chain_ids = np.concatenate([np.arange(a, b) for a, b in self.chains.bands])
        want = uk.returns_model(x["rewards"].reshape(T, nc, 1), x["done"][:, chain_ids // self.n],
                                x["out"].reshape(T, nc, 1, self.W), self.W - 1, self.gamma)
        for name, w in zip(self.outputs, want):
            _row_local(v, store, self.layout, name, exact=w.reshape(T * nc, 1))
        return v


# ------------------------------------------------------------------------------------------ A. HipReluBackwardColumnSums
class ColumnSumsCase(RowsCase):
    unit = 64

    def __init__(self, scale, C):
        self.C, self.name = C, f"HipReluBackwardColumnSums C={C}"
        self.widths = {"gx": C, "y": C, "g": C}
        self.outputs = ("g",)
        self.claims = tuple((t, b) for t in self.widths for b in BOUNDARIES)
        super().__init__(scale)
        self.small_bytes = 4 * C * (self.R // 4096 + 2)

    def inputs(self):
        gx, y = uk.colsum_inputs(self.gen_rows(), self.C)
        return {"gx": gx[:self.layout.nb], "y": y[:self.layout.nb]}

    def standin(self, maps):
        x = self.inputs()
        s = HostStore(self.layout, maps)
        s.add("gx", self.C, x["gx"])
        s.add("y", self.C, x["y"])
        s.add("g", self.C)
        g, partial = uk.colsum_model(s.load("gx"), s.load("y"), self.R, 1)
        s.save("g", g)
        return s, {"column sums": partial[0]}

    def check(self, store, results):
        v, x = Verdict(self.name), self.inputs()
        g, _ = uk.colsum_model(x["gx"], x["y"], self.layout.nb, 1)
        _row_local(v, store, self.layout, "g", exact=g)
        v.judge("column sums", results["column sums"], g.astype(f64).sum(0), uk.seq_sum_f32(g, axis=0))
        return v


# ------------------------------------------------------------------------------------------ B. HipLinearMaskBackwardBx3_256
class MaskBackwardCase(RowsCase):
    name, unit, C = "HipLinearMaskBackwardBx3_256", 256, 256
    widths = {"g_in": 256, "h": 256, "g_out": 256}
    outputs = ("g_out",)
    claims = tuple((t, b) for t in widths for b in BOUNDARIES)
    small_bytes = 4 * 4 * 256 * 256

    def inputs(self):
        g, w, h = uk.mask_inputs(self.gen_rows(), self.C)
        return {"g_in": g[:self.layout.nb], "w": w, "h": h[:self.layout.nb]}

    def standin(self, maps):
        x = self.inputs()
        s = HostStore(self.layout, maps)
        for k in ("g_in", "h"):
            s.add(k, self.C, x[k])
        s.add("g_out", self.C)
        s.save("g_out", uk.mask_reference(s.load("g_in"), x["w"], s.load("h"), dtype=f32))
        return s, None

    def check(self, store, _=None):
        v, x = Verdict(self.name), self.inputs()
        got = _row_local(v, store, self.layout, "g_out", uk.mask_reference(x["g_in"], x["w"], x["h"]),
                         uk.mask_reference(x["g_in"], x["w"], x["h"], dtype=f32))
        v.require(bool((uk.bits(got[x["h"] <= 0]) == 0).all()), "g_out", "the mask is not exact")
        return v


# ------------------------------------------------------------------------------------------ B. HipWeightGradBx3_256x{256,96}
class WeightGradCase(RowsCase):
    """ci = 256: g and x cross all three.  ci = 71 with the bias column: x [R, 71] holds 1.19e9 elements at the R that takes
    g past 2^32 -- b30 only; b31 and b32 of x would need R = 3.0e7 / 6.0e7 rows, whose g alone is 31 / 62 GB beside
    x and the cap"""
    unit = 32

    def __init__(self, scale, ci):
        self.ci, self.with_bias = ci, ci != 256
        self.name = f"HipWeightGradBx3_256x{256 if ci == 256 else 96}"
        self.widths = {"g": 256, "x": ci}
        self.claims = tuple(("g", b) for b in BOUNDARIES) + (tuple(("x", b) for b in BOUNDARIES) if ci == 256 else (("x", "b30"),))
        super().__init__(scale)
        self.small_bytes = 4 * 257 * 256 * 256

    def inputs(self):
        G, X = uk.weight_grad_inputs(self.gen_rows(), self.ci)
        return {"g": G[:self.layout.nb], "x": X[:self.layout.nb]}

    def standin(self, maps):
        x = self.inputs()
        s = HostStore(self.layout, maps)
        s.add("g", 256, x["g"])
        s.add("x", self.ci, x["x"])
        total = uk.weight_grad_reference(s.load("g"), s.load("x"), self.ci if self.with_bias else -1, self.R, 1, dtype=f32)[0]
        return s, {"weights": total[:, :self.ci], **({"bias": total[:, self.ci]} if self.with_bias else {})}

    def check(self, store, results):
        v, x = Verdict(self.name), self.inputs()
        ones = self.ci if self.with_bias else -1
        want = uk.weight_grad_reference(x["g"], x["x"], ones, self.layout.nb, 1)[0]
        yard = uk.weight_grad_reference(x["g"], x["x"], ones, self.layout.nb, 1, dtype=f32)[0]
        v.judge("weights", results["weights"], want[:, :self.ci], yard[:, :self.ci])
        if self.with_bias:
            v.judge("bias", results["bias"], want[:, self.ci], yard[:, self.ci])
        return v


# ------------------------------------------------------------------------------------------ B. HipHeadBackward{Bx3,}_W43
class HeadBackwardCase(RowsCase):
    """C = 256 (HipHeadBackwardBx3_W43 through the wrapper): h2 / g2 cross all three; g3 [R, 43] reaches b30 at R = 2.5e7 --
    its b31 would need R = 5.0e7, where h2 and g2 are 51 GB each.
    C = 64 (HipHeadBackward_W43 launched directly, 4096 rows per block): h2 / g2 cross all three at R = 6.7e7, g3 b30 and
    b31; its b32 would need R = 1.0e8: 17 GB of g3 beside 2 x 25.6 GB."""
    unit, W = 32, 43

    def __init__(self, scale, C):
        self.C, self.direct = C, C != 256
        self.name = "HipHeadBackward_W43 C=64" if self.direct else "HipHeadBackwardBx3_W43"
        self.widths = {"g3": 43, "h2": C, "g2": C}
        self.outputs = ("g2",)
        self.claims = tuple((t, b) for t in ("h2", "g2") for b in BOUNDARIES) + (("g3", "b30"),) + ((("g3", "b31"),) if self.direct else ())
        super().__init__(scale)
        self.rows_per_block = scale.unit(4096)
        self.grid = -(-self.R // self.rows_per_block)
        self.small_bytes = 4 * (self.grid if self.direct else 257) * 44 * C

    def inputs(self):
        g3, w3, h2 = uk.head_inputs(self.gen_rows(), self.W, self.C, one_sign=not self.direct)
        return {"g3": g3[:self.layout.nb], "w3": w3, "h2": h2[:self.layout.nb]}

    def standin(self, maps):
        x = self.inputs()
        s = HostStore(self.layout, maps)
        s.add("g3", 43, x["g3"])
        s.add("h2", self.C, x["h2"])
        s.add("g2", self.C)
        rpb, grid = (self.rows_per_block, self.grid) if self.direct else (self.R, 1)
        res = uk.head_reference(s.load("g3"), x["w3"], s.load("h2"), rpb, grid, dtype=f32)
        s.save("g2", res.pop("g2"))
        if not self.direct:
            res = {"db2": res["db2_part"][0], "dw3": res["dw3_part"][0], "db3": s.load("g3").sum(0, dtype=f32)}
        return s, res

    def check(self, store, results):
        """results: direct {db2_part [grid, C], dw3_part [grid, W, C]}; wrapper {db2 [C], dw3 [W, C], db3 [W]}"""
        v, x, lay = Verdict(self.name), self.inputs(), self.layout
        ref = uk.head_reference(x["g3"], x["w3"], x["h2"], lay.nb, 1)
        yard = uk.head_reference(x["g3"], x["w3"], x["h2"], lay.nb, 1, dtype=f32)
        got = _row_local(v, store, lay, "g2", ref["g2"], yard["g2"])
        v.require(bool((uk.bits(got[x["h2"] <= 0]) == 0).all()), "g2", "the mask is not exact")
        if not self.direct:
            v.judge("db2", results["db2"], ref["db2_part"][0], yard["db2_part"][0])
            v.judge("dw3", results["dw3"], ref["dw3_part"][0], yard["dw3_part"][0])
            v.judge("db3", results["db3"], x["g3"].astype(f64).sum(0), x["g3"].sum(0, dtype=f32))
            return v
        rpb, band_blocks = self.rows_per_block, lay.blocks(self.rows_per_block)
        for b in band_blocks:            # a block's zero rows add nothing: float64 over its band rows
            rows = [lay.host_rows(x[k], b * rpb, min(self.R, (b + 1) * rpb)) for k in ("g3", "h2")]
            r64 = uk.head_reference(rows[0], x["w3"], rows[1], rpb, 1)
            r32 = uk.head_reference(rows[0], x["w3"], rows[1], rpb, 1, dtype=f32)
            for k in ("db2_part", "dw3_part"):
                v.judge(k, results[k][b], r64[k][0], r32[k][0])
        others = np.setdiff1d(np.arange(self.grid), band_blocks)
        for k in ("db2_part", "dw3_part"):
            v.require(not uk.bits(np.ascontiguousarray(results[k][others])).any(), k, "a block of zero rows left a partial that is not +0")
        return v


# ------------------------------------------------------------------------------------------ A. HipRolloutRecord
class RecordCase:
    """launches at t - 1, t, t + 1 around every boundary row t = floor(boundary / (E n)) of the batch tensors [rows, E, n]
    (`batch_row` preset by the test), and at t = 0; every other row of the batches keeps the sentinel, one surplus row
    included.  "a": N = 100 agents of one policy, the reward batch past all three; "b": N = 1, the done batch and the reward
    batch (8.6 GB each) past b30 and b31 -- b32 of both is not under test in this case."""
    unit = 1

    def __init__(self, scale, variant):
        self.scale, self.variant = scale, variant
        self.name = f"HipRolloutRecord ({variant})"
        self.E = 2000 if scale.real else 2
        self.N = (100 if scale.real else 5) if variant == "a" else 1
        w = self.E * self.N
        self.widths = {"reward_batch": w} if variant == "a" else {"reward_batch": w, "done_batch": w}
        self.claims = tuple((t, b) for t in self.widths for b in (BOUNDARIES if variant == "a" else BOUNDARIES[:2]))
        self.boundary_rows = {(t, b): scale.e[b] // w for t, b in self.claims}
        rows = sorted(set(self.boundary_rows.values()))
        self.ts = [0] + [t + d for t in rows for d in (-1, 0, 1)]
        self.groups = [(0, 1)] + [(t - 1, 3) for t in rows]          # (batch_row to preset, launches that follow)
        self.R = max(self.ts) + 2
        self.layout = Layout(self.R, [(t, t + 1, "launch") for t in self.ts])
        self.case = uk.RecordCase(self.name, self.N, "one", self.E, [128])

    def bytes(self):
        return 4 * self.R * self.E * (self.N + 1)

    def reach(self, tensor, boundary):
        return self.R * self.widths[tensor] > self.scale.e[boundary]

    def not_crossed(self):
        return sorted((t, b) for t in self.widths for b in BOUNDARIES if (t, b) not in self.claims)

    def inputs(self):
        """rewards [launches, E, N] (both signs, 1e-3 .. 1e3), done [launches, E]: the patterns of update_kernel_cases.py,
        replica e on pattern e % 6, repeated over the launches"""
        L = len(self.ts)
        rng = np.random.RandomState(self.case.seed)
        rewards = (rng.choice([-1.0, 1.0], (L, self.E, self.N)) * 10.0 ** rng.uniform(-3, 3, (L, self.E, self.N))).astype(f32)
        done = np.stack([[uk.DONE_PATTERNS[self.case.pattern_of(e)][k % uk.RECORD_TICKS] for e in range(self.E)]
                         for k in range(L)]).astype(np.int32)
        return rewards, done

    def initial_state(self):
        s = self.case.initial_state()
        return {k: v[:self.E].copy() for k, v in s.items() if k.startswith("ep_") and not k.endswith("_b")}

    def model(self):
        """the final small state and the compact batches [launches, E, N] / [launches, E] of the numpy model"""
        rewards, done = self.inputs()
        slot, _, _ = self.case.slot()
        L = len(self.ts)
        st = dict(self.initial_state(), reward_batch_a=np.zeros((L, self.E, self.N), f32), reward_batch_b=np.zeros((L, self.E, 0), f32),
                  done_batch=np.zeros((L, self.E), np.int32), ep_reward_b=np.zeros((self.E, 0), f32), ep_sum_b=np.zeros(self.E, f32))
        for k in range(L):
            st["batch_row"] = np.full(self.E, k, np.int64)
            uk.record_model(st, rewards[k], done[k], slot, self.E)
        return st

    def standin(self, maps):
        st, w = self.model(), self.E * self.N
        s = HostStore(self.layout, maps)
        s.add("reward_batch", w)
        s.add("done_batch", self.E, dtype=np.int32)
        for k, t in enumerate(self.ts):
            s.t["reward_batch"].save(st["reward_batch_a"][k], t * w + np.arange(w))
            s.t["done_batch"].save(st["done_batch"][k], t * self.E + np.arange(self.E))
        return s, {k: st[k] for k in ("ep_reward_a", "ep_sum_a", "ep_count")}

    def check(self, store, results):
        v, st, L = Verdict(self.name), self.model(), len(self.ts)
        for name, key, w in (("reward_batch", "reward_batch_a", self.E * self.N), ("done_batch", "done_batch", self.E)):
            got = np.concatenate([store.rows(name, t, t + 1) for t in self.ts])
            v.exact(name, got, st[key].reshape(L, w))
            left = store.sentinels(name)
            v.require(left == (self.R - L) * w, name, "rows no launch wrote do not all hold the sentinel", left, (self.R - L) * w)
        for k in ("ep_reward_a", "ep_sum_a", "ep_count"):
            v.exact(k, results[k], st[k])
        return v


def all_cases(scale):
    return [PolicyGradientHeadCase(scale), DiscountedReturnsCase(scale), ColumnSumsCase(scale, 256), ColumnSumsCase(scale, 64),
            MaskBackwardCase(scale), WeightGradCase(scale, 256), WeightGradCase(scale, 71), HeadBackwardCase(scale, 256),
            HeadBackwardCase(scale, 64), RecordCase(scale, "a"), RecordCase(scale, "b")]
