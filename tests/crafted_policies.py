"""Policies with EXACT probabilities for the in-kernel policy forward of the in-tree rollout and evaluation entries
(csrc/kernels/rollout_policy.h behind cp_policy_cum / cp_policy_probs, cc_policy_cum / cc_policy_probs and
gw5_policy_cum / gw5_policy_probs), built straight into the packed float32 buffers the kernels read
(training/policy_kernel.py::pack_rollout_policy with I = 4, 2 and 6; pack_gridworld_policy: 21 inputs at stride 24, the pad
columns zero).  Shared by tests/inkernel_policy_exact_cases.py, tests/test_inkernel_policy_exact_host.py and
tests/test_gpu_inkernel_policy_exact.py.  Nothing here touches a GPU.

Every weight is 0 or a power of two, so every product of the fmaf chains is exact, and every softmax term is expf(0) = 1 or
expf of a gap above 110, which is 0 in float32 (the smallest subnormal is e^-103.3) on every correct implementation: the
probabilities are exactly 0, 1 / m (m tied winners) or 1 / A, and a test that uses them needs no window around a threshold.

Kinds:
  uniform    every weight and bias 0: each probability is 1 / A;
  constant   a dead first layer (W0 = 0, b0 = -1), the winners' logit 128 through the LAST hidden unit of layer 2 (its bias
             1), every other logit 0; a decoy unit that only a bias added behind the ReLU would switch on;
  switched   the winner is decided by the sign of a linear form of the observation: two first-layer units with gain 2^40
             (TagGridWorld: 2^20) and opposite signs -- the LAST unit and one in the upper half at H = 64 --, each passed
             through a second-layer unit OTHER than its own index, to one action each; every other action's bias is -128.
             An exact 0 of the form leaves both units at 0: an exact tie, 0.5 / 0.5, between the two switched actions."""
import numpy as np

f32 = np.float32
WIDTHS = (32, 64)
GAIN, GRID_GAIN, WIN = 2.0 ** 40, 2.0 ** 20, 128.0
# env -> (inputs of a W0 row, floats per W0 row, actions)
LAYOUT = {"cartpole": (4, 4, 2), "mountain_car": (2, 2, 3), "acrobot": (6, 6, 3), "gridworld": (21, 24, 5)}
# the linear form of a switched policy: {input column: coefficient}, (action if the form is positive, action if negative)
FORMS = {
    "cartpole": ({2: 1.0, 3: 0.25}, (1, 0)),        # theta + theta_dot / 4 (column 3: the last of the float4 row)
    "mountain_car": ({1: 1.0}, (2, 0)),             # the velocity (the odd column of the float2 row)
    "acrobot": ({4: 1.0}, (2, 0)),                  # theta_dot_1
    "tagger": ({4: 1.0, 0: -1.0}, (1, 2)),          # the runner's x minus tagger 0's: right or left
    "runner": ({9: 1.0, 20: -1.0}, (4, 3)),         # the runner's y / L minus t / T (column 20, behind five whole float4s)
}


def units(H):
    """the hidden units a crafted policy uses: first-layer units `pos` (the LAST one) and `neg` (upper half at H = 64),
    second-layer units `pos2` / `neg2` (neither equals the first-layer unit that feeds it; `neg2` is the last one),
    `decoy`: a second-layer unit only a wrong network switches on"""
    return {"pos": H - 1, "neg": H - 6, "pos2": 2, "neg2": H - 1, "decoy": H - 2}


def blank(env, H, A=None):
    """zero weights in the layout of `env`; A: another action count than the env's own (the logits entries)"""
    I, _, own = LAYOUT[env]
    A = own if A is None else int(A)
    return {"W0": np.zeros((H, I), f32), "b0": np.zeros(H, f32), "W1": np.zeros((H, H), f32), "b1": np.zeros(H, f32),
            "Wp": np.zeros((A, H), f32), "bp": np.zeros(A, f32)}


def pack(env, parts):
    """the packed float32 buffer of `parts`: W0 [H][stride] (pad columns zero), b0, W1, b1, Wp, bp; TagGridWorld's block
    padded with zeros to a multiple of four floats"""
    I, stride, _ = LAYOUT[env]
    H, A = parts["W0"].shape[0], parts["Wp"].shape[0]
    assert parts["W0"].shape == (H, I) and parts["Wp"].shape == (A, H) and parts["bp"].shape == (A,)
    w0 = np.zeros((H, stride), f32)
    w0[:, :I] = parts["W0"]
    flat = np.concatenate([np.asarray(x, f32).reshape(-1) for x in
                           (w0, parts["b0"], parts["W1"], parts["b1"], parts["Wp"], parts["bp"])])
    if env == "gridworld":
        flat = np.concatenate([flat, np.zeros(-len(flat) % 4, f32)])
    return np.ascontiguousarray(flat, dtype=f32)


def unpack(env, packed, H, A=None):
    """the inverse of `pack` (W0 without its pad columns)"""
    I, stride, own = LAYOUT[env]
    A = own if A is None else int(A)
    w = np.asarray(packed, f32).reshape(-1)
    out, at = {}, 0
    for name, shape in (("W0", (H, stride)), ("b0", (H,)), ("W1", (H, H)), ("b1", (H,)), ("Wp", (A, H)), ("bp", (A,))):
        n = int(np.prod(shape))
        out[name] = w[at:at + n].reshape(shape).copy()
        at += n
    assert len(w) - at == (-at % 4 if env == "gridworld" else 0), (len(w), at)
    assert not out["W0"][:, I:].any(), "a pad column of W0 is not zero"
    out["W0"] = out["W0"][:, :I].copy()
    return out


def as_model(env, parts):
    """the same weights as a training.models.FullyConnected, for the packers of training/policy_kernel.py"""
    import torch
    from warp_drive_amd.training.models import FullyConnected

    I = LAYOUT[env][0]
    H, A = parts["W0"].shape[0], parts["Wp"].shape[0]
    model = FullyConnected(I, [A], [H, H])
    with torch.no_grad():
        for layer, w, b in ((model.fc["0"][0], "W0", "b0"), (model.fc["1"][0], "W1", "b1"), (model.policy_head[0], "Wp", "bp")):
            layer.weight.copy_(torch.from_numpy(parts[w]))
            layer.bias.copy_(torch.from_numpy(parts[b]))
    return model


def packed_by_the_project(env, parts):
    """`parts` through FullyConnected and the project's own packer -> float32 numpy"""
    from warp_drive_amd.training.policy_kernel import pack_gridworld_policy, pack_rollout_policy

    packer = pack_gridworld_policy if env == "gridworld" else pack_rollout_policy
    return packer(as_model(env, parts)).numpy().copy()


# ------------------------------------------------------------------------------------------------------------ kinds
def uniform(env, H, A=None):
    return blank(env, H, A)


def constant(env, H, winners, A=None):
    """the same logits on every row: 128 for `winners`, 0 for the rest"""
    A = LAYOUT[env][2] if A is None else int(A)
    winners = sorted(set(int(w) for w in winners))
    assert winners and 0 <= winners[0] and winners[-1] < A and len(winners) < A
    p, u = blank(env, H, A), units(H)
    p["b0"][:] = -1.0                                   # the dead first layer: h1 = fmaxf(-1, 0) = 0 on every row
    p["b1"][u["neg2"]] = 1.0                            # h2[H - 1] = 1
    for w in winners:
        p["Wp"][w, u["neg2"]] = WIN
    # the decoy: h2[decoy] = fmaxf(-1 * h1[3], 0) = 0.  A bias added BEHIND the ReLU makes h1[3] = -1, switches the decoy
    # on and hands a loser a logit of 256
    loser = next(a for a in range(A) if a not in winners)
    p["W1"][u["decoy"], 3] = -1.0
    p["Wp"][loser, u["decoy"]] = 2 * WIN
    return p


def constant_kinds(env, A=None):
    """{name: winners} of an env's constant policies: a single winner at action 0, at A - 1 and in the middle; two tied
    winners without action 0 (a leading exact zero; at five actions a plateau at 0.5 and one at 1.0 before the last action;
    at three actions the tie can only be the last two; at two actions a tie without action 0 does not exist)"""
    A = LAYOUT[env][2] if A is None else int(A)
    if A < 2:
        return {}
    out = {"winner0": (0,), f"winner{A - 1}": (A - 1,)}
    if A >= 3:
        out[f"winner{A // 2}"] = (A // 2,)
        out["tied"] = (1, 3) if A >= 5 else (A - 2, A - 1)
    return out


def switched(form, env, H, sign=1, gain=None):
    """FORMS[form] on the layout of `env`; sign = -1 swaps the two actions"""
    A = LAYOUT[env][2]
    coeff, (hi, lo) = FORMS[form]
    if sign < 0:
        hi, lo = lo, hi
    g = f32(GRID_GAIN if env == "gridworld" else GAIN) if gain is None else f32(gain)
    p, u = blank(env, H), units(H)
    for col, c in coeff.items():
        p["W0"][u["pos"], col] = g * f32(c)
        p["W0"][u["neg"], col] = -g * f32(c)
    p["W1"][u["pos2"], u["pos"]] = 1.0
    p["W1"][u["neg2"], u["neg"]] = 1.0
    p["Wp"][hi, u["pos2"]] = 1.0
    p["Wp"][lo, u["neg2"]] = 1.0
    p["bp"][[a for a in range(A) if a not in (hi, lo)]] = -WIN
    return p


def kinds(env, H):
    """{name: packed} of a single-agent env, or {name: [tagger packed, runner packed]} of TagGridWorld"""
    out = {}
    if env == "gridworld":
        out["uniform"] = [pack(env, uniform(env, H))] * 2
        for name, winners in constant_kinds(env).items():
            # (the runner's winners mirrored: a swap of the two policies changes the actions)
            mirrored = tuple(sorted(4 - w for w in winners)) if name != "tied" else (2, 4)
            out[name] = [pack(env, constant(env, H, winners)), pack(env, constant(env, H, mirrored))]
        out["switched"] = [pack(env, switched("tagger", env, H)), pack(env, switched("runner", env, H))]
        return out
    out["uniform"] = pack(env, uniform(env, H))
    for name, winners in constant_kinds(env).items():
        out[name] = pack(env, constant(env, H, winners))
    if env == "cartpole":
        out["towards"] = pack(env, switched(env, env, H, 1))
        out["away"] = pack(env, switched(env, env, H, -1))
    else:
        out["switched"] = pack(env, switched(env, env, H, 1))
    return out


def allowed_probabilities(env, kind):
    """the exact float32 values a kind's probabilities may take"""
    A = LAYOUT[env][2]
    if kind == "uniform":
        return {float(f32(1.0) / f32(A))}
    if kind == "tied":
        return {0.0, 0.5}
    if kind.startswith("winner"):
        return {0.0, 1.0}
    return {0.0, 0.5, 1.0}
