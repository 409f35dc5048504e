"""Policies with EXACT probabilities for the in-kernel policy of the custom-environment kits (include/wd_env_rollout.h,
include/wd_env_evaluate.h), in the style of tests/crafted_policies.py: every weight is 0 or a power of two, so every
product of the fmaf chains is exact, and every softmax term is expf(0) = 1 or expf of a gap of 128 or more, which is 0 in
float32 on every correct implementation.  The probabilities are exactly 0, 1 / m (m tied winners) or 1 / A: the action is
a pure function of the observation and the Philox uniform, and a test that uses them needs no window and no cap.  Built
for any (F, H, A) straight into the packed layout W0 [H][F], b0 [H], W1 [H][H], b1 [H], Wp [A][H], bp [A].  Nothing here
touches a GPU.

Kinds:
  uniform    every weight and bias 0: each probability is 1 / A; greedy picks action 0, always;
  constant   a dead first layer (W0 = 0, b0 = -1), the winners' logit 128 through the LAST hidden unit of layer 2 (its bias
             1), every other logit 0; two winners tie at exactly 0.5;
  switched   the winner is decided by the sign of (observation column c - threshold): two first-layer units with gain 2^40
             and opposite signs -- the LAST unit and one in the upper half at H = 64 --, each passed through a second-layer
             unit OTHER than its own index, to one action each; every other action's bias is -128.  A column exactly AT the
             threshold leaves both units at 0: an exact tie, 0.5 / 0.5, between the two switched actions.

PRESET EPOCHS.  END_DRAWS lists (row, epoch) pairs of sampler seed END_SEED at which the kit's draw -- counter
(row, epoch, tick tag, 5), word x -- gives u == 1.0 ("hi": the clamp) and u == 2^-24 ("lo": below every positive running
sum), found with oracle/core_np.py::find_end_draws over 350 rows x 2^17 epochs; tests/test_custom_env_evaluate_build.py
replays them."""
import numpy as np

f32 = np.float32
GAIN, WIN = 2.0 ** 40, 128.0
END_SEED = 17
END_DRAWS = {"hi": [(64, 58264), (175, 70545), (29, 72420)], "lo": [(23, 64599), (234, 67247), (50, 83044), (20, 125522)]}


def units(H):
    """the hidden units a crafted policy uses (tests/crafted_policies.py::units)"""
    return {"pos": H - 1, "neg": H - 6, "pos2": 2, "neg2": H - 1}


def blank(F, H, A):
    return {"W0": np.zeros((H, F), f32), "b0": np.zeros(H, f32), "W1": np.zeros((H, H), f32), "b1": np.zeros(H, f32),
            "Wp": np.zeros((A, H), f32), "bp": np.zeros(A, f32)}


def pack(parts):
    return np.ascontiguousarray(np.concatenate([np.asarray(parts[k], f32).reshape(-1)
                                                for k in ("W0", "b0", "W1", "b1", "Wp", "bp")]), dtype=f32)


def uniform(F, H, A):
    return pack(blank(F, H, A))


def load_into(model, packed, F, H, A):
    """copy the packed weights into a training.models.FullyConnected(F, [A], [H, H]) (its value head is left alone)"""
    import torch

    cuts = np.cumsum([0, F * H, H, H * H, H, A * H, A])
    W0, b0, W1, b1, Wp, bp = (np.asarray(packed, f32)[a:b] for a, b in zip(cuts[:-1], cuts[1:]))
    with torch.no_grad():
        for layer, w, b, shape in ((model.fc["0"][0], W0, b0, (H, F)), (model.fc["1"][0], W1, b1, (H, H)),
                                   (model.policy_head[0], Wp, bp, (A, H))):
            layer.weight.copy_(torch.from_numpy(w.reshape(shape).copy()))
            layer.bias.copy_(torch.from_numpy(b.copy()))


def constant(F, H, A, winners):
    """the same logits on every row: 128 for `winners`, 0 for the rest"""
    winners = sorted(set(int(w) for w in winners))
    assert winners and 0 <= winners[0] and winners[-1] < A and len(winners) < A
    p, u = blank(F, H, A), units(H)
    p["b0"][:] = -1.0                     # the dead first layer: h1 = fmaxf(-1, 0) = 0 on every row
    p["b1"][u["neg2"]] = 1.0              # h2[H - 1] = 1
    for w in winners:
        p["Wp"][w, u["neg2"]] = WIN
    return pack(p)


def switched(F, H, A, column, threshold, above, below):
    """action `above` where obs[column] > threshold, `below` where it is smaller, an exact tie of the two AT the threshold
    (threshold: 0 or a power of two, so gain * threshold is exact)"""
    assert 0 <= column < F and above != below and 0 <= min(above, below) and max(above, below) < A
    p, u = blank(F, H, A), units(H)
    g = f32(GAIN)
    p["W0"][u["pos"], column], p["b0"][u["pos"]] = g, -g * f32(threshold)
    p["W0"][u["neg"], column], p["b0"][u["neg"]] = -g, g * f32(threshold)
    p["W1"][u["pos2"], u["pos"]] = 1.0
    p["W1"][u["neg2"], u["neg"]] = 1.0
    p["Wp"][above, u["pos2"]] = 1.0
    p["Wp"][below, u["neg2"]] = 1.0
    p["bp"][[a for a in range(A) if a not in (above, below)]] = -WIN
    return pack(p)


def switched_winner(obs_column, threshold, above, below):
    """the greedy action of `switched` on a column of float32 observations: the tie goes to the lower index"""
    x = np.asarray(obs_column, f32)
    return np.where(x > f32(threshold), above, np.where(x < f32(threshold), below, min(above, below))).astype(np.int32)


def preset_epochs(n_rows, ticks, seed=END_SEED):
    """(epochs uint32 [n_rows], roles {row: ("hi" | "lo", tick)}): every END_DRAWS row below n_rows reaches its end draw at
    a tick of its own below `ticks` (0, 1, 2, ... in turn); the other rows start at arbitrary epochs"""
    assert seed == END_SEED
    epochs = np.random.RandomState(11).randint(0, 2 ** 31, size=n_rows, dtype=np.int64).astype(np.uint32)
    roles = {}
    picks = [(r, e, kind) for kind in ("hi", "lo") for r, e in END_DRAWS[kind] if r < n_rows]
    for i, (r, e, kind) in enumerate(picks):
        tick = i % ticks
        roles[r] = (kind, tick)
        epochs[r] = e - tick
    return epochs, roles
