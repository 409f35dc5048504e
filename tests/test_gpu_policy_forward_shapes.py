"""Every compiled instantiation of the fused policy forward (csrc/kernels/policy_mlp.hip) against the SAME network in
float64: HipPolicyMlp{,Bx3}_<H>x<H>_k<KT1> (the plain entries) and HipPolicyMlpAct{,Bx3}_<H>x<H>_k<KT1> (the rollout
tick's entries: actions drawn in the epilogue, activations stored for the update), H in {64, 128, 256}, KT1 =
ceil(F / 32) in {1, 2, 3}, both arithmetics.

The yardstick is the framework's own float32 error on the same inputs: a kernel result is accepted when its distance to
float64 is at most 4 x that of the plain float32 network (floor: 8 float32 ulps of the compared tensor's largest entry,
only against a yardstick that happens to be zero), checked for every variant (launch) on its own.  A variant of fewer
than 4096 rows (a 1-row launch has ONE value, whose float32 error is a single draw of a wide distribution) has its
yardstick measured on its own rows plus 4096 further rows of the same distribution through the same network.  A bf16x3 forward
that dropped one of its three bf16 terms (2^-17-accurate products) is well outside that bound; fixed absolute tolerances
of 2e-6 are not.  The worst err / err_f32 of every case is printed (pytest -s)."""
import copy
import functools
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ULP32 = 2.0 ** -24
HIDDEN = (64, 128, 256)
KTILES = (1, 2, 3)
ARITHMETICS = ("float32", "bf16x3")


@functools.lru_cache(maxsize=None)
def _fm():
    from tests.hip_harness import require_gpu
    from warp_drive_amd.managers.function_manager import HIPFunctionManager

    require_gpu()
    fm = HIPFunctionManager(num_agents=1, num_envs=1)
    fm.load_hip_from_binary_file()
    return fm


def _launches(name):
    from warp_drive_amd.managers import hip_driver as drv

    return drv.LAUNCH_COUNTS[name]


def _model(F, heads, H, seed, saturate=False):
    """a FullyConnected policy with logits of a useful spread and biases that matter (saturate: logits over +-300)"""
    from warp_drive_amd.training.models import FullyConnected

    torch.manual_seed(seed)
    model = FullyConnected(F, heads, fc_dims=(H, H)).to("cuda")
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(3.0) if p.dim() == 2 else p.normal_(0.0, 0.5)
        if saturate:
            x = torch.randn(4096, F, device="cuda")
            logits = _layers(model, x)[-1][:, :sum(heads)]
            s = 300.0 / float(logits.abs().max())
            for hd in model.policy_head:
                hd.weight.mul_(s)
                hd.bias.mul_(s)
    return model


def _layers(model, x):
    """(pre1, h1, pre2, h2, out) of the network on rows x [..., F], in the dtype of `model` and x: out = the logits of
    every head, then the value"""
    l1, l2 = model.fc["0"][0], model.fc["1"][0]
    w3 = torch.cat([h.weight for h in model.policy_head] + [model.vf_head.weight], dim=0)
    b3 = torch.cat([h.bias for h in model.policy_head] + [model.vf_head.bias], dim=0)
    pre1 = torch.nn.functional.linear(x, l1.weight, l1.bias)
    h1 = torch.relu(pre1)
    pre2 = torch.nn.functional.linear(h1, l2.weight, l2.bias)
    h2 = torch.relu(pre2)
    return pre1, h1, pre2, h2, torch.nn.functional.linear(h2, w3, b3)


def _heads_of(out, heads):
    start = 0
    for a in heads:
        yield start, out[..., start:start + a]
        start += a


def _errors(got, want64, f32):
    """(kernel error, framework float32 error, scale): largest distances to float64, its largest magnitude"""
    want64 = want64.double()
    return (float((got.double() - want64).abs().max()), float((f32.double() - want64).abs().max()),
            float(want64.abs().max()))


def _within_bound(err, err_f32, scale):
    return err <= max(4.0 * err_f32, 8.0 * ULP32 * scale)


class _Yardstick:
    """`add` collects the errors of one variant (one launch) per tensor kind; `close` checks the bound against THAT
    variant's float32 error and scale and keeps the worst ratio per kind for the case's printout (`report`)"""

    def __init__(self, case):
        self.case, self.worst, self.cur = case, {}, {}

    def add(self, kind, got, want64, f32, noise=0.0):
        """noise: the framework's float32 error of the same network on further rows (small variants)"""
        err, err_f32, scale = _errors(got, want64, f32)
        e = (err, max(err_f32, noise), scale)
        self.cur[kind] = tuple(max(a, b) for a, b in zip(self.cur.get(kind, (0.0, 0.0, 0.0)), e))

    def close(self, variant):
        cur, self.cur = self.cur, {}
        for k, (err, err_f32, scale) in cur.items():
            ratio = err / err_f32 if err_f32 > 0 else (float("inf") if err else 0.0)
            self.worst[k] = max(self.worst.get(k, 0.0), ratio)
            assert _within_bound(err, err_f32, scale), (self.case, variant, k, err, err_f32, scale)

    def report(self):
        print(f"{self.case}: worst err / err_f32 over its variants", {k: f"{v:.2f}" for k, v in self.worst.items()})


def _evaluate(model, x, heads):
    pre1, h1, pre2, h2, out = _layers(model, x)
    heads_out = [z for _, z in _heads_of(out, heads)]
    return dict(probs=[torch.softmax(z, dim=-1) for z in heads_out], values=out[..., sum(heads)], out=out, pre1=pre1,
                h1=h1, pre2=pre2, h2=h2, shifted=[z - z.max(-1, keepdim=True).values for z in heads_out])


def _reference(model, x, heads, pad_rows=4096):
    """float64 and float32 (probabilities per head, values, out, its heads shifted by their maximum, pre1, h1, pre2, h2)
    of the network on rows x; f32["noise"]: {kind: the float32 error of the same network on `pad_rows` further rows of
    the same distribution} when x has fewer rows than that (else empty)"""
    m64 = copy.deepcopy(model).double()
    noise = {}
    with torch.no_grad():
        f64, f32 = _evaluate(m64, x.double(), heads), _evaluate(model, x, heads)
        if x.numel() // x.shape[-1] < pad_rows:
            g = torch.Generator(device=x.device)
            g.manual_seed(12345)
            xe = torch.randn(pad_rows, x.shape[-1], device=x.device, generator=g)
            e64, e32 = _evaluate(m64, xe.double(), heads), _evaluate(model, xe, heads)
            err = lambda a, b: float((a.double() - b).abs().max())  # noqa: E731
            for k in ("probs", "shifted"):
                noise[k] = max(err(a, b) for a, b in zip(e32[k], e64[k]))
            for k in ("values", "h1", "h2"):
                noise[k] = err(e32[k], e64[k])
    f32["noise"] = noise
    return f64, f32


# --------------------------------------------------------------------------------------------------------------------
#   A. the plain entries: probabilities, values, the batch copy of the rows
# --------------------------------------------------------------------------------------------------------------------
def _plain_variants(kt1):
    """(F, heads, (E, N, ids)) per variant: across the variants of a case, F at both ends of the entry's k-tile range and
    one odd F between; heads of 42, 2, 63 (W = 64), 63 (spanning both output tiles) and 2 x 1 rows; 1, 31, 129 and
    102 623 (ragged) rows; ids out of order (the kernel's id table) and contiguous ranges (its `id0` path)"""
    lo, hi, mid = 32 * kt1 - 31, 32 * kt1, 32 * kt1 - 15
    rng = np.random.default_rng(kt1)
    return [
        (lo, [21, 21], (1, 4, [2])),
        (hi, [2], (1, 40, [int(i) for i in rng.permutation(40)[:31]])),
        (mid, [63], (43, 5, [1, 2, 3])),
        (lo, [30, 33], (2503, 47, [int(i) for i in rng.permutation(47)[:41]])),
        (hi, [1, 1], (31, 6, [4])),
    ]


def _run_plain(fused, heads, E, N, ids, seed):
    dev = torch.device("cuda:0")
    F = fused.F
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    obs = torch.randn(E, N, F, device=dev, generator=g)
    ids_t = torch.tensor(ids, dtype=torch.int32, device=dev)
    n_pol, T = len(ids), 3
    probs = [torch.full((E, N, a), -7.0, device=dev) for a in heads]
    values = torch.full((E, n_pol), -7.0, device=dev)
    obs_out = torch.full((T, E, n_pol, F), -7.0, device=dev)
    row = torch.tensor(1, dtype=torch.int64, device=dev)
    name = fused.fn.name
    before = _launches(name)
    fused(obs, ids_t, probs, values=values, obs_out=obs_out, batch_row=row)
    torch.cuda.synchronize()
    assert _launches(name) == before + 1, name
    sel = ids_t.long()
    x = obs.index_select(1, sel)
    others = [a for a in range(N) if a not in ids]
    for p in probs:
        if others:  # rows of other agents are left alone
            assert (p[:, others] == -7.0).all()
    got = [p.index_select(1, sel) for p in probs]
    for p in got:
        assert torch.isfinite(p).all() and (p >= 0).all()
        assert float((p.double().sum(-1) - 1.0).abs().max()) <= 1e-5
    assert torch.equal(obs_out[1], x), "the batch copy of the rows is not bit-exact"
    assert (obs_out[0] == -7.0).all() and (obs_out[2] == -7.0).all()
    return x, got, values


@pytest.mark.parametrize("arithmetic", ARITHMETICS)
@pytest.mark.parametrize("kt1", KTILES)
@pytest.mark.parametrize("H", HIDDEN)
def test_plain_forward_entry_vs_float64(H, kt1, arithmetic):
    from warp_drive_amd.training.policy_kernel import FusedPolicyForward

    case = f"HipPolicyMlp{'Bx3' if arithmetic == 'bf16x3' else ''}_{H}x{H}_k{kt1}"
    yard = _Yardstick(case)
    for v, (F, heads, (E, N, ids)) in enumerate(_plain_variants(kt1)):
        model = _model(F, heads, H, seed=1000 * H + 10 * kt1 + v)
        fused = FusedPolicyForward(_fm(), model, F, arithmetic=arithmetic)
        assert fused.fn.name == case and fused.kt1 == kt1
        x, got, values = _run_plain(fused, heads, E, N, ids, seed=v)
        want, f32 = _reference(model, x, heads)
        for h, p in enumerate(got):
            yard.add("probs", p, want["probs"][h], f32["probs"][h], f32["noise"].get("probs", 0.0))
        yard.add("values", values, want["values"], f32["values"], f32["noise"].get("values", 0.0))
        yard.close((F, heads, E * len(ids)))
    yard.report()

    # saturated logits (spread over +-300): probabilities underflow to exactly 0, nothing is NaN / Inf, and the bound
    # still holds
    F, heads = 32 * kt1 - 15, [21, 21]
    model = _model(F, heads, H, seed=7 + H + kt1, saturate=True)
    fused = FusedPolicyForward(_fm(), model, F, arithmetic=arithmetic)
    x, got, values = _run_plain(fused, heads, 200, 9, [2, 3, 4, 5, 6], seed=99)
    want, f32 = _reference(model, x, heads)
    assert float(want["out"][..., :sum(heads)].abs().max()) >= 100.0
    sat = _Yardstick(case + " saturated")
    for h, p in enumerate(got):
        assert (p == 0.0).any(), "the saturated variant did not saturate"
        sat.add("probs", p, want["probs"][h], f32["probs"][h], f32["noise"].get("probs", 0.0))
    assert torch.isfinite(values).all()
    sat.add("values", values, want["values"], f32["values"], f32["noise"].get("values", 0.0))
    sat.close("saturated")
    sat.report()


# --------------------------------------------------------------------------------------------------------------------
#   B. the Act entries: actions drawn in the epilogue, batch rows, stored activations
# --------------------------------------------------------------------------------------------------------------------
def _act_launch(H, F, heads, arithmetic, E, N, id_sets, seed, T=3, stored=True, check_untouched=True, only=None):
    """one HipPolicyMlpAct* launch of FusedRolloutTick on synthetic tensors: one policy per id set (all of one network
    shape, different weights); every replica's batch row = T - 1.  Returns what the launch wrote and its inputs.
    only = "obs" / "act" / "out": that batch tensor alone has T rows (all of them the sentinel) and is written; every
    other batch tensor has ONE row and reaches the launch as a null pointer, which the kernel skips -- so T can be what
    takes a narrow tensor past 2^32 elements without 256-wide activations of the same T."""
    from warp_drive_amd.training.policy_kernel import FusedPolicyForward, FusedRolloutTick

    dev = torch.device("cuda:0")
    bx3 = arithmetic == "bf16x3"
    rng = np.random.default_rng(seed)
    models = [_model(F, heads, H, seed=seed + 17 * k) for k in range(len(id_sets))]
    forwards = [FusedPolicyForward(_fm(), m, F, arithmetic=arithmetic) for m in models]
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    obs = torch.randn(E, N, F, device=dev, generator=g)
    actions = torch.full((E, N, 2), -1, dtype=torch.int32, device=dev)
    rewards, done = torch.zeros((E, N), device=dev), torch.zeros((E,), dtype=torch.int32, device=dev)
    # rng words: random key, random per-row epochs with the wrap (0xFFFFFFFF) and 0 among them
    epochs = rng.integers(0, 2 ** 32, size=E * N, dtype=np.uint64).astype(np.uint32)
    epochs[:: 7] = 0xFFFFFFFF
    epochs[3:: 11] = 0
    key = rng.integers(0, 2 ** 32, size=2, dtype=np.uint64).astype(np.uint32)
    words = np.concatenate([key, np.array([E * N, 0], np.uint32), epochs]).view(np.int32)
    rng_state = torch.from_numpy(words.copy()).to(dev)
    stream_tag = 0x3A5 + seed % 97
    batch_row = torch.full((E,), T - 1, dtype=torch.int64, device=dev)
    ns = [len(ids) for ids in id_sets]
    W = sum(heads) + 1
    rows = lambda kind: T if only in (None, kind) else 1  # noqa: E731

    def alloc(shape, fill, **kw):
        if check_untouched or only is not None:
            return torch.full(shape, fill, **kw)
        t = torch.empty(shape, **kw)  # (huge: only rows 0 and T - 2 get the sentinel)
        t[0].fill_(fill)
        t[T - 2].fill_(fill)
        return t

    obs_b = [alloc((rows("obs"), E, n, F), -7.0, device=dev) for n in ns]
    act_b = [alloc((rows("act"), E, n, 2), -9, dtype=torch.int32, device=dev) for n in ns]
    rew_b = [torch.zeros((rows(None), E, n), device=dev) for n in ns]
    done_b = torch.zeros((rows(None), E), dtype=torch.int32, device=dev)
    ep_r, ep_s, ep_c = [torch.zeros((E, n), device=dev) for n in ns], [torch.zeros(E, device=dev) for _ in ns], torch.zeros(E, device=dev)
    st = None
    if bx3 and stored:
        st = [tuple(alloc((rows(kind), E, n, c), -7.0, device=dev) for kind, c in (("h1", H), ("h2", H), ("out", W))) for n in ns]
    probs = [torch.full((E, N, a), -7.0, device=dev) for a in heads]
    ids_t = [torch.tensor(ids, dtype=torch.int32, device=dev) for ids in id_sets]
    tick = FusedRolloutTick(_fm(), forwards, ids_t, obs, actions, rewards, done, rng_state, stream_tag, batch_row,
                            obs_b, act_b, rew_b, done_b, ep_r, ep_s, ep_c, stored=st, probs=probs)
    name = f"HipPolicyMlpAct{'Bx3' if bx3 else ''}_{H}x{H}_k{(F + 31) // 32}"
    assert tick.fwd_name == name
    if only is not None:
        short = [t for t in obs_b + act_b + [x for s in st or [] for x in s] if t.shape[0] != T]
        assert len(short) == len(ns) * (4 if st else 1)
        tick.fwd_args = [np.uint64(0) if any(a is t for t in short) else a for a in tick.fwd_args]
    before = _launches(name)
    tick.forward()
    torch.cuda.synchronize()
    assert _launches(name) == before + 1, name
    return dict(models=models, obs=obs, actions=actions, rng_state=rng_state, epochs=epochs, key=key,
                stream_tag=stream_tag, obs_b=obs_b, act_b=act_b, stored=st, probs=probs, ids=id_sets, T=T)


def _check_act(r, heads, yard, bx3):
    from oracle.core_np import fused_tick_uniforms, sample_actions_counting

    E, N = r["obs"].shape[:2]
    T = r["T"]
    # every row's epoch advanced by exactly one (with the wrap)
    after = r["rng_state"].cpu().numpy().view(np.uint32)
    assert np.array_equal(after[:2], r["key"])
    assert np.array_equal(after[4:], (r["epochs"] + np.uint32(1)).astype(np.uint32)), "epochs not advanced by one"
    # the actions replayed on the host: Philox counter (row, epoch, stream_tag, 3), the counting search on the float32
    # probabilities the kernel drew from
    u = fused_tick_uniforms(E * N, r["epochs"], int(r["key"][0]), int(r["key"][1]), r["stream_tag"])
    got_a = r["actions"].cpu().numpy().reshape(E * N, 2)
    for h, a in enumerate(heads):
        p = r["probs"][h].cpu().numpy().reshape(E * N, a)
        assert (p >= 0).all() and np.isfinite(p).all(), "a row's probabilities were not written"
        want_a = sample_actions_counting(p, u[h])
        bad = np.flatnonzero(got_a[:, h] != want_a)
        assert bad.size == 0, f"head {h} (A = {a}): {bad.size} actions differ from the replay, first rows {bad[:5]}"
    for k, ids in enumerate(r["ids"]):
        sel = torch.tensor(ids, dtype=torch.long, device="cuda")
        x = r["obs"].index_select(1, sel)
        assert torch.equal(r["obs_b"][k][T - 1], x), "batch copy of the rows"
        assert torch.equal(r["act_b"][k][T - 1], r["actions"].index_select(1, sel)), "batch copy of the actions"
        assert (r["obs_b"][k][: T - 1] == -7.0).all() and (r["act_b"][k][: T - 1] == -9).all()
        want, f32 = _reference(r["models"][k], x, heads)
        for h in range(len(heads)):
            yard.add("probs", r["probs"][h].index_select(1, sel), want["probs"][h], f32["probs"][h],
                     f32["noise"].get("probs", 0.0))
        if bx3:
            _check_stored(r["stored"][k], T, want, f32, heads, yard)


def _check_stored(stored, t, want, f32, heads, yard):
    """row t - 1 of the stored h1, h2 and outputs against float64; every other row untouched"""
    h1, h2, out = stored
    for name, got in (("h1", h1[t - 1]), ("h2", h2[t - 1])):
        pre64 = want["pre" + name[1]]
        yard.add(name, got, want[name], f32[name], f32["noise"].get(name, 0.0))
        # a unit ReLU'd on one side only: where float32 rounding can decide the sign
        disagree = (got > 0) != (pre64 > 0)
        if bool(disagree.any()):
            lim = 1e-5 * float(pre64.abs().max())
            assert float(pre64[disagree].abs().max()) <= lim, (name, float(pre64[disagree].abs().max()), lim)
    o, A = out[t - 1], sum(heads)
    for (s, _), z64, z32 in zip(_heads_of(want["out"], heads), want["shifted"], f32["shifted"]):
        yard.add("out", o[..., s:s + z64.shape[-1]], z64, z32, f32["noise"].get("shifted", 0.0))
    yard.add("value", o[..., A], want["values"], f32["values"], f32["noise"].get("values", 0.0))
    for x in (h1, h2, out):
        assert (x[: t - 1] == -7.0).all()


def _act_variants(kt1):
    """(F, heads, E, N, id sets): two policies with interleaved, non-contiguous ids (policy A -- the launch's blocks
    [0, first_block_b) -- with 11 ids x 9 replicas = 99 rows, fewer than a block of 128; then with 9 ids x 37 replicas =
    333 = 2 x 128 + 77 rows, policy B 407) and one policy (the launch's dummy second policy: ids out of order, then a
    contiguous range); heads [21, 21] and [25, 24] (wider than the epilogue's unrolled 24-entry search)"""
    rng = np.random.default_rng(100 + kt1)
    N = 20
    a_ids = sorted(int(i) for i in rng.permutation(N)[:11])
    b_ids = [i for i in range(N) if i not in a_ids][::-1]
    perm = [int(i) for i in rng.permutation(N)]
    out = []
    for heads, F in (([21, 21], 32 * kt1), ([25, 24], 32 * kt1 - 31)):
        out += [(F, heads, 9, N, [a_ids, b_ids]), (F, heads, 37, N, [b_ids[::-1], a_ids[::-1]]),
                (F, heads, 13, N, [perm]), (F, heads, 29, N, [list(range(N))])]
    return out


@pytest.mark.parametrize("arithmetic", ARITHMETICS)
@pytest.mark.parametrize("kt1", KTILES)
@pytest.mark.parametrize("H", HIDDEN)
def test_act_entry_draws_stores_and_records(H, kt1, arithmetic):
    bx3 = arithmetic == "bf16x3"
    case = f"HipPolicyMlpAct{'Bx3' if bx3 else ''}_{H}x{H}_k{kt1}"
    yard = _Yardstick(case)
    for v, (F, heads, E, N, id_sets) in enumerate(_act_variants(kt1)):
        if len(id_sets) == 2:
            assert all(np.any(np.diff(ids) != 1) for ids in id_sets)
        r = _act_launch(H, F, heads, arithmetic, E, N, id_sets, seed=31 * H + 7 * kt1 + v)
        _check_act(r, heads, yard, bx3)
        yard.close((F, heads, E, [len(ids) for ids in id_sets]))
    yard.report()


def _stores_past_2_32(H, F, heads, E, N, T):
    """one HipPolicyMlpActBx3 launch whose stored row T - 1 starts past 2^32 elements: ONLY scalars and booleans leave
    this function, so that nothing of the ~42 GB it allocates outlives it"""
    r = _act_launch(H, F, heads, "bf16x3", E, N, [list(range(N))], seed=5, T=T, check_untouched=False)
    h1, h2, out = r["stored"][0]
    res = {"untouched": all(bool((a[t] == -7.0).all()) for a in (h1, h2, out, r["obs_b"][0]) for t in (0, T - 2))
           and all(bool((r["act_b"][0][t] == -9).all()) for t in (0, T - 2)),
           "rows": torch.equal(r["obs_b"][0][T - 1], r["obs"]) and torch.equal(r["act_b"][0][T - 1], r["actions"])}
    want, f32 = _reference(r["models"][0], r["obs"], heads)
    res["h1"] = _errors(h1[T - 1], want["h1"], f32["h1"])
    res["h2"] = _errors(h2[T - 1], want["h2"], f32["h2"])
    for (s, _), z64, z32 in zip(_heads_of(want["out"], heads), want["shifted"], f32["shifted"]):
        a = z64.shape[-1]
        res[f"out[{s}:{s + a}]"] = _errors(out[T - 1][..., s:s + a], z64, z32)
    A = sum(heads)
    res["value"] = _errors(out[T - 1][..., A], want["values"], f32["values"])
    return res


def test_act_stores_activations_beyond_two_to_the_32_elements():
    """The trainer stores h1 / h2 of every batch row (configs[2]: [250, 2000, 100, 256], 1.3e10 elements): a row whose
    element offset is past 2^32 (so 32-bit offsets, signed or not, would wrap) must land where it belongs.  The ~42 GB
    are released before the test ends: the device is shared with the rest of the suite"""
    _fm()  # (no GPU: fails like every other test here; only a lack of memory skips)
    free, _ = torch.cuda.mem_get_info()
    if free < 48 * 2 ** 30:
        pytest.skip(f"needs 48 GB of free device memory, {free / 2 ** 30:.1f} GB free")
    H, F, heads, E, N = 256, 71, [21, 21], 64, 100
    T = 2623
    assert (T - 1) * E * N * H > 2 ** 32
    torch.cuda.synchronize()
    reserved = torch.cuda.memory_reserved()
    res, failure = None, None
    try:
        res = _stores_past_2_32(H, F, heads, E, N, T)
    except Exception as err:  # noqa: BLE001 -- only its text is kept: its traceback would hold the frames and their tensors
        failure = f"{type(err).__name__}: {err}"
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert torch.cuda.memory_reserved() <= reserved + 2 ** 28, (torch.cuda.memory_reserved(), reserved)
    assert failure is None, failure
    assert res.pop("untouched"), "a row other than T - 1 was written"
    assert res.pop("rows"), "batch copy of the rows / actions"
    print("HipPolicyMlpActBx3_256x256_k3 at element offset > 2^32: err / err_f32",
          {k: f"{e / e32:.2f}" if e32 else f"{e:.1e} / 0" for k, (e, e32, _) in res.items()})
    for k, (e, e32, scale) in res.items():
        assert _within_bound(e, e32, scale), (k, e, e32, scale)


def _equals_everywhere(t, fill):
    """every element of t == fill, in pieces: no temporary the size of t"""
    flat, bad = t.reshape(-1), torch.zeros((), dtype=torch.int64, device=t.device)
    for a in range(0, flat.numel(), 1 << 27):
        bad += (flat[a:a + (1 << 27)] != fill).sum()
    return int(bad) == 0


def _one_store_past(kind, boundary, H, F, heads, E, N):
    """one HipPolicyMlpActBx3 launch that writes ONLY the batch tensor `kind`, at the row that holds element `boundary`;
    scalars and booleans leave this function, nothing of what it allocates"""
    width = {"obs": F, "out": sum(heads) + 1, "act": 2}[kind]
    T = boundary // (E * N * width) + 1
    assert (T - 1) * E * N * width <= boundary < T * E * N * width
    r = _act_launch(H, F, heads, "bf16x3", E, N, [list(range(N))], seed=5, T=T, check_untouched=False, only=kind)
    t = {"obs": r["obs_b"][0], "act": r["act_b"][0], "out": r["stored"][0][2]}[kind]
    assert t.shape[0] == T and t.numel() > boundary
    res = {"bytes": t.numel() * 4, "untouched": _equals_everywhere(t[:T - 1], -9 if kind == "act" else -7.0)}
    if kind == "obs":
        res["row"] = torch.equal(t[T - 1], r["obs"])
    elif kind == "act":
        a = r["actions"]
        res["row"] = torch.equal(t[T - 1], a) and bool((a >= 0).all()) and bool((a < torch.tensor(heads, device=a.device)).all())
    else:
        want, f32 = _reference(r["models"][0], r["obs"], heads)
        for (s, _), z64, z32 in zip(_heads_of(want["out"], heads), want["shifted"], f32["shifted"]):
            res[f"out[{s}:{s + z64.shape[-1]}]"] = _errors(t[T - 1][..., s:s + z64.shape[-1]], z64, z32)
        res["value"] = _errors(t[T - 1][..., sum(heads)], want["values"], f32["values"])
    return res


@pytest.mark.parametrize("boundary", (31, 32))
@pytest.mark.parametrize("kind", ("obs", "out", "act"))
def test_act_stores_batch_rows_beyond_two_to_the_31_and_32_elements(kind, boundary):
    """The trainer's observation batch [T, E, n, 71], stored outputs [T, E, n, 43] and action batch [T, E, n, 2] pass 2^31
    elements at configs[2] (3.6e9, 2.2e9; the action batch stays below there, and is taken past both boundaries here because
    17.2 GB fit): E x N = 8 x 100 rows, T such that row T - 1 HOLDS element 2^31 / 2^32 of the one tensor the launch
    writes (8.6 / 17.2 GB); a store whose offset wrapped lands in the rows before it, which must all keep the sentinel"""
    _fm()
    H, F, heads, E, N = 256, 71, [21, 21], 8, 100
    need = 4 * (2 ** boundary) + 3 * 2 ** 30
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"needs {need / 2 ** 30:.0f} GB of free device memory, {free / 2 ** 30:.1f} GB free")
    torch.cuda.synchronize()
    reserved = torch.cuda.memory_reserved()
    res, failure = None, None
    try:
        res = _one_store_past(kind, 2 ** boundary, H, F, heads, E, N)
    except Exception as err:  # noqa: BLE001 -- only its text is kept: its traceback would hold the frames and their tensors
        failure = f"{type(err).__name__}: {err}"
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert torch.cuda.memory_reserved() <= reserved + 2 ** 28, (torch.cuda.memory_reserved(), reserved)
    assert failure is None, failure
    assert res.pop("bytes") > 4 * 2 ** boundary
    assert res.pop("untouched"), "a row other than T - 1 was written"
    if kind != "out":
        assert res.pop("row"), "batch copy of the rows / actions"
    print(f"HipPolicyMlpActBx3_256x256_k3 {kind} batch at element offset 2^{boundary}: err / err_f32",
          {k: f"{e / e32:.2f}" if e32 else f"{e:.1e} / 0" for k, (e, e32, _) in res.items()})
    for k, (e, e32, scale) in res.items():
        assert _within_bound(e, e32, scale), (k, e, e32, scale)
