"""Cases and yardsticks of the A2C / PPO update kernels (csrc/kernels/pg_update.hip; training/pg_update_kernels.py).  No GPU.

  * `CASES`: the smallest shapes at which the five launches can still go wrong -- E in {1, 63, 64, 65, 257} with T in
    {2, 5, 10} (a tile is 128 rows: 2 rows, one partial tile, tile boundaries inside a row of the batch, 2570 rows = 21
    tiles on 3 blocks), grids with 1 to 3 surplus blocks, both widths, O in {2, 4, 6}, A in {1, 2, 3, 8}, gamma 1 and 0.99,
    entropy coefficients 0 and 0.1, value coefficients 0.01 and 0.1, A2C and PPO, four done patterns, and one case whose
    head weights are scaled until the logit gaps exceed 110 (`gap`).
  * the inputs of a case (`inputs`): the network has hidden units whose pre-activation is exactly 0 on every row (a zero
    row of weights and a zero bias, with non-zero weights leaving the unit: relu'(0) = 1 would show) and the usual negative
    pre-activations.
  * `yardstick`: the float64 restatement, a WRITTEN-OUT backward pass in numpy (no autograd), with the mutations the host
    test plants in it; `framework`: training/models.py::FullyConnected + training/losses.py + autograd in a given dtype on
    a given device (float64 on the CPU: what the yardstick must agree with; float32: the error a float32 computation makes).
  * `apply_model` / `framework_apply`: clip + Adam in float64 numpy / with torch's own functions.
  * the bound is tests/update_kernel_cases.py's: err <= max(4 * err_f32, 2e-6 * scale) per result tensor."""
import collections

import numpy as np

from tests.update_kernel_cases import SENTINEL_BITS, bits, judge, within_bound  # noqa: F401  (shared with the GPU file)

f32, f64 = np.float32, np.float64
TILE = 128
TENSOR_NAMES = ("W0", "b0", "W1", "b1", "Wp", "bp", "Wv", "bv")
SUM_NAMES = ("sum logp*adv", "sum entropy", "sum (v-ret)^2", "sum adv")
DONE_PATTERNS = ("none", "last row", "value 2", "one mid-batch")

Case = collections.namedtuple("Case", "name E T gamma H O A ent vf algo done grid gap seed")


def _case(E, T, gamma, H, O, A, ent, vf, done, algo="A2C", grid=None, gap=False, seed=0):
    name = (f"E{E}-T{T}-g{gamma}-H{H}O{O}A{A}-ent{ent}-vf{vf}-{algo}-{done.replace(' ', '_')}" + (f"-grid{grid}" if grid else "")
            + ("-gap" if gap else ""))
    return Case(name, E, T, gamma, H, O, A, ent, vf, algo, done, grid, gap, seed)


# grid: blocks of the gradient launch (None: one per tile)
CASES = (
    _case(1, 2, 1.0, 32, 2, 1, 0.0, 0.01, "none", seed=1),                              # 2 rows, one action
    _case(63, 2, 0.99, 64, 4, 2, 0.1, 0.1, "last row", "PPO", seed=2),                  # 126 rows: one partial tile
    _case(64, 5, 0.99, 64, 6, 3, 0.1, 0.01, "value 2", seed=3),                         # 320 rows: 2.5 tiles
    _case(65, 5, 1.0, 32, 6, 8, 0.0, 0.1, "one mid-batch", "PPO", seed=4),              # 325 rows: boundaries inside a batch row
    _case(257, 10, 0.99, 64, 4, 2, 0.1, 0.01, "value 2", grid=3, seed=5),               # 2570 rows: 21 tiles on 3 blocks
    _case(257, 5, 0.99, 32, 2, 3, 0.1, 0.1, "none", grid=14, seed=6),                   # 1285 rows: 11 tiles, 3 surplus blocks
    _case(64, 10, 1.0, 64, 2, 3, 0.0, 0.01, "last row", grid=2, seed=7),                # 640 rows = 5 whole tiles on 2 blocks
    _case(65, 2, 0.99, 64, 6, 8, 0.1, 0.1, "one mid-batch", grid=4, seed=8),            # 130 rows: 2 tiles, 2 surplus blocks
    _case(63, 10, 0.99, 32, 4, 2, 0.1, 0.01, "value 2", "PPO", seed=9),
    _case(1, 10, 0.99, 32, 4, 8, 0.1, 0.1, "one mid-batch", grid=2, seed=10),           # 10 rows, one surplus block
    _case(64, 5, 0.99, 64, 4, 3, 0.1, 0.1, "value 2", gap=True, seed=11),               # logit gaps above 110
    _case(65, 10, 1.0, 32, 6, 1, 0.1, 0.01, "last row", seed=12),                       # one action: no policy gradient at all
)


def case_tiles(case):
    return -(-case.T * case.E // TILE)


def case_grid(case):
    return case.grid or case_tiles(case)


def net_shapes(H, O, A):
    return (("W0", (H, O)), ("b0", (H,)), ("W1", (H, H)), ("b1", (H,)), ("Wp", (A, H)), ("bp", (A,)), ("Wv", (1, H)), ("bv", (1,)))


def net_floats(H, O, A):
    return sum(int(np.prod(s)) for _, s in net_shapes(H, O, A))


def tensor_bounds(H, O, A):
    out, at = [], 0
    for _, shape in net_shapes(H, O, A):
        out.append((at, at + int(np.prod(shape))))
        at += int(np.prod(shape))
    return out


def _make_net(rng, H, O, A, head_gain=1.0):
    """torch's default Linear init (uniform +- 1 / sqrt(fan_in)); units 1 and H - 2 of the first layer and units 2 and
    H - 1 of the second have a zero row and a zero bias: their pre-activation is exactly 0 on every row, and the weights
    that LEAVE them are not zero"""
    net = {}
    for name, shape in net_shapes(H, O, A):
        fan_in = {"W0": O, "b0": O}.get(name, H)
        net[name] = rng.uniform(-1.0, 1.0, shape).astype(f32) / f32(np.sqrt(fan_in))
    for u in (1, H - 2):
        net["W0"][u], net["b0"][u] = 0.0, 0.0
    for u in (2, H - 1):
        net["W1"][u], net["b1"][u] = 0.0, 0.0
    net["Wp"] = (net["Wp"] * f32(head_gain)).astype(f32)
    net["bp"] = (net["bp"] * f32(head_gain)).astype(f32)
    return net


def flatten(net):
    return np.concatenate([np.asarray(net[p]).reshape(-1) for p in TENSOR_NAMES]).astype(f32)


def unflatten(flat, H, O, A):
    net, at = {}, 0
    for name, shape in net_shapes(H, O, A):
        n = int(np.prod(shape))
        net[name] = flat[at:at + n].reshape(shape)
        at += n
    assert at == flat.size
    return net


def done_flags(case, rng):
    T, E = case.T, case.E
    done = np.zeros((T, E), np.int32)
    if case.done == "last row":
        done[-1] = 1
    elif case.done == "value 2":          # MountainCar's goal flag: finished is `done > 0`
        done[:] = 2 * (rng.random((T, E)) < 0.3)
        done[0, 0] = 2
        done[-1, ::2] = 0
    elif case.done == "one mid-batch":
        done[(T - 1) // 2, E // 2] = 1
    return done


def inputs(case):
    """{obs [T, E, O], actions [T, E] int32, rewards [T, E], done [T, E] int32, theta (flat float32)}"""
    rng = np.random.default_rng(2000 + case.seed)
    T, E, H, O, A = case.T, case.E, case.H, case.O, case.A
    return {
        "obs": rng.standard_normal((T, E, O)).astype(f32),
        "actions": rng.integers(0, A, (T, E)).astype(np.int32),
        "rewards": (rng.standard_normal((T, E)) - 1.0).astype(f32),
        "done": done_flags(case, rng),
        "theta": flatten(_make_net(rng, H, O, A, 20000.0 if case.gap else 1.0)),
    }


# ------------------------------------------------------------------------------------------------------- returns
def returns_model(rewards, done, values, gamma, dtype=f32, ignore_done=False):
    """losses.discounted_returns on [T, E] arrays, operation for operation in `dtype`"""
    r, v = rewards.astype(dtype), values.astype(dtype)
    d = np.zeros_like(r) if ignore_done else (done > 0).astype(dtype)
    one, g = dtype(1), dtype(gamma)
    out = np.zeros_like(r)
    out[-1] = d[-1] * r[-1] + (one - d[-1]) * v[-1]
    for t in range(r.shape[0] - 2, -1, -1):
        out[t] = r[t] + ((one - d[t]) * g) * out[t + 1]
    return out


# ---------------------------------------------------------------------------------- the written-out float64 passes
def forward64(net, x):
    z1 = x @ net["W0"].T + net["b0"]
    h1 = np.maximum(z1, 0)
    z2 = h1 @ net["W1"].T + net["b1"]
    h2 = np.maximum(z2, 0)
    return h2 @ net["Wp"].T + net["bp"], h2 @ net["Wv"][0] + net["bv"][0], (x, z1, h1, z2, h2)


def log_softmax64(z):
    s = z - z.max(axis=1, keepdims=True)
    return s - np.log(np.exp(s).sum(axis=1, keepdims=True))


MUTATIONS = ("relu'(0) = 1", "last tile left out", "entropy term dropped", "inv_R = 1 / E", "returns ignore done",
             "value gradient without the factor 2")


def mutation_applies(case, mutation):
    if mutation == "entropy term dropped":
        return case.ent > 0 and case.A > 1 and not case.gap   # (a saturated policy has no entropy to speak of)
    if mutation == "returns ignore done":
        return case.done != "none"
    if mutation == "inv_R = 1 / E":
        return case.T > 1
    return True


def yardstick(case, inp, mutate=None, values=None):
    """float64: values, returns, advantages [T, E], the eight gradients, the four sums.  values: form the returns and
    advantages from these [T, E] instead of the network's own (a later stage judged from the inputs it was given)."""
    T, E, O, A = case.T, case.E, case.O, case.A
    net = {k: v.astype(f64) for k, v in unflatten(inp["theta"], case.H, O, A).items()}
    rows = T * E
    x = inp["obs"].astype(f64).reshape(rows, O)
    z, v, (_, z1, h1, z2, h2) = forward64(net, x)
    own = v.reshape(T, E)
    base = own if values is None else np.asarray(values, f64).reshape(T, E)
    returns = returns_model(inp["rewards"], inp["done"], base, case.gamma, f64, ignore_done=mutate == "returns ignore done")
    advantages = returns - base
    used = rows if mutate != "last tile left out" else (-(-rows // TILE) - 1) * TILE
    inv_R = 1.0 / (E if mutate == "inv_R = 1 / E" else rows)
    ent = 0.0 if mutate == "entropy term dropped" else case.ent
    adv, ret, taken = advantages.reshape(-1), returns.reshape(-1), inp["actions"].reshape(-1)
    lp = log_softmax64(z)
    p = np.exp(lp)
    entropy = -(p * lp).sum(axis=1)
    onehot = np.arange(A)[None, :] == taken[:, None]
    dz = (adv[:, None] * (p - onehot) + ent * p * (lp + entropy[:, None])) * inv_R
    dv = (1.0 if mutate == "value gradient without the factor 2" else 2.0) * case.vf * (v - ret) * inv_R
    dz[used:], dv[used:] = 0.0, 0.0
    at0 = 1.0 if mutate == "relu'(0) = 1" else 0.0
    step = lambda pre: np.where(pre > 0, 1.0, np.where(pre == 0, at0, 0.0))
    d2 = (dz @ net["Wp"] + dv[:, None] * net["Wv"][0][None]) * step(z2)
    d1 = (d2 @ net["W1"]) * step(z1)
    logp_taken = lp[np.arange(rows), np.clip(taken, 0, A - 1)]
    out = {"values": own, "returns": returns, "advantages": advantages,
           "W0": d1.T @ x, "b0": d1.sum(0), "W1": d2.T @ h1, "b1": d2.sum(0), "Wp": dz.T @ h2, "bp": dz.sum(0),
           "Wv": (dv @ h2)[None], "bv": dv.sum(keepdims=True),
           "sum logp*adv": np.sum(logp_taken * adv), "sum entropy": np.sum(entropy), "sum (v-ret)^2": np.sum((v - ret) ** 2),
           "sum adv": np.sum(adv), "probabilities": p}
    return out


def flat_gradient(result):
    return np.concatenate([np.asarray(result[name]).reshape(-1) for name in TENSOR_NAMES])


def loss_terms(case, sums):
    """(total, policy, value, entropy) losses from the four sums, as the trainer's metrics form them"""
    R = case.T * case.E
    policy = -(sums["sum adv"] if case.algo == "PPO" else sums["sum logp*adv"]) / R
    value, entropy = sums["sum (v-ret)^2"] / R, sums["sum entropy"] / R
    return policy + case.vf * value - case.ent * entropy, policy, value, entropy


# ------------------------------------------------------------------------------------- the framework's computation
def build_module(H, O, A, flat, dtype, device):
    """a training/models.py::FullyConnected holding the flat float32 parameters, in `dtype` on `device`"""
    import torch
    from warp_drive_amd.training.models import FullyConnected

    model = FullyConnected(O, [A], (H, H))
    net = unflatten(np.asarray(flat), H, O, A)
    with torch.no_grad():
        for p, name in zip(module_parameters(model), TENSOR_NAMES):
            p.copy_(torch.from_numpy(net[name].copy()))
    return model.to(device=device, dtype=dtype)


def module_parameters(model):
    """the eight parameters in TENSOR_NAMES order"""
    layers = [model.fc["0"][0], model.fc["1"][0], model.policy_head[0], model.vf_head]
    return [p for layer in layers for p in (layer.weight, layer.bias)]


def framework(case, inp, dtype, device="cpu", values=None):
    """Trainer's framework update up to the gradients, in torch `dtype` on `device`: the keys of `yardstick`, numpy float64
    arrays.  values None: training/losses.py's A2C / PPO object end to end (the gap case: the same objective on the logits).  values [T, E]: the returns and advantages are
    losses.discounted_returns of THESE values (what the gradient launch is handed), the objective is the same expression."""
    import torch
    from torch.distributions import Categorical
    from warp_drive_amd.training import losses

    T, E, O, A = case.T, case.E, case.O, case.A
    model = build_module(case.H, O, A, inp["theta"], dtype, device)
    dev = lambda a, dt=dtype: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)
    obs, actions = dev(inp["obs"]).reshape(T, E, 1, O), dev(inp["actions"], torch.int64).reshape(T, E, 1, 1)
    rewards, done = dev(inp["rewards"]).reshape(T, E, 1), dev(inp["done"], torch.int32)
    if dtype == torch.float64:
        # (FullyConnected's own autograd nodes hand back float32 parameter gradients whatever the input's type: the
        # float64 reference runs the same network through the framework's plain operations)
        F = torch.nn.functional
        l0, l1, lp, lv = model.fc["0"][0], model.fc["1"][0], model.policy_head[0], model.vf_head
        h2 = F.relu(F.linear(F.relu(F.linear(obs, l0.weight, l0.bias)), l1.weight, l1.bias))
        z, v = F.linear(h2, lp.weight, lp.bias), F.linear(h2, lv.weight, lv.bias)[..., 0]
    else:
        out = model.forward_logits(obs)
        z, v = out[..., :A], out[..., A]
    probs = [torch.softmax(z, dim=-1)]
    # (the gap case: Categorical(probs) clamps the probabilities at the type's eps and so departs from the closed form by
    # more than any rounding; there the framework's computation is the one on the logits)
    make_dist = (lambda: Categorical(logits=z)) if case.gap else (lambda: Categorical(probs[0]))
    common = dict(discount_factor_gamma=case.gamma, vf_loss_coeff=case.vf, entropy_coeff=case.ent)
    objective = losses.PPO(clip_param=0.1, **common) if case.algo == "PPO" else losses.A2C(**common)
    base = v.detach() if values is None else dev(values).reshape(T, E, 1)
    returns = losses.discounted_returns(rewards, done, base, case.gamma)
    if values is None and not case.gap:
        loss, _ = objective.compute_loss_and_metrics(timestep=0, actions_batch=actions, rewards_batch=rewards,
                                                     done_flags_batch=done, action_probabilities_batch=probs,
                                                     value_functions_batch=v)
    else:
        dist = make_dist()
        loss = (objective._policy_loss(dist.log_prob(actions[..., 0]), returns - base)
                + case.vf * torch.nn.functional.mse_loss(v, returns) - case.ent * dist.entropy().mean())
    advantages = returns - base
    params = module_parameters(model)
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    num = lambda t: t.detach().double().cpu().numpy()
    with torch.no_grad():
        dist = make_dist()
    out = {"values": num(v).reshape(T, E), "returns": num(returns).reshape(T, E), "advantages": num(advantages).reshape(T, E),
           "sum logp*adv": float((dist.log_prob(actions[..., 0]) * advantages).sum()), "sum entropy": float(dist.entropy().sum()),
           "sum (v-ret)^2": float(((v.detach() - returns) ** 2).sum()), "sum adv": float(advantages.sum()),
           "loss": float(loss.detach())}
    for name, p, g in zip(TENSOR_NAMES, params, grads):
        out[name] = num(torch.zeros_like(p) if g is None else g)
    return out


# ------------------------------------------------------------------------------------------------- the apply stage
ApplyCase = collections.namedtuple("ApplyCase", "name H O A step clip max_norm lr seed")
APPLY_CASES = tuple(
    ApplyCase(f"H{H}O{O}A{A}-step{step}-clip_{clip}", H, O, A, step, clip, 3.0, 1e-3, 40 + i)
    for i, (H, O, A, step, clip) in enumerate([(32, 2, 3, 1, "active"), (64, 4, 2, 1, "inactive"), (64, 6, 3, 1, "off"),
                                               (64, 4, 8, 2, "active"), (32, 6, 1, 2, "inactive"), (32, 2, 3, 2, "off"),
                                               (64, 2, 3, 1000, "active"), (32, 4, 2, 1000, "inactive"),
                                               (64, 6, 8, 1000, "off")]))
ZERO_EVERY = 7   # every 7th gradient entry is exactly 0 and so are its moments: Adam must leave that parameter alone


def apply_inputs(ac):
    """theta, exp_avg, exp_avg_sq, grads (flat float32).  clip "active": the gradient norm is above max_norm; "inactive":
    far below it; "off": large, and no clipping asked for.  At step 1 the moments are zero."""
    rng = np.random.default_rng(ac.seed)
    n = net_floats(ac.H, ac.O, ac.A)
    size = {"active": 0.5, "inactive": 1e-3, "off": 0.5}[ac.clip]
    grads = (size * rng.standard_normal(n)).astype(f32)
    first = ac.step == 1
    exp_avg = np.zeros(n, f32) if first else (0.1 * size * rng.standard_normal(n)).astype(f32)
    exp_avg_sq = np.zeros(n, f32) if first else (size * size * rng.uniform(0.01, 1.0, n)).astype(f32)
    for a in (grads, exp_avg, exp_avg_sq):
        a[::ZERO_EVERY] = 0.0
    return {"theta": rng.uniform(-0.5, 0.5, n).astype(f32), "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq, "grads": grads}


def apply_max_norm(ac):
    return None if ac.clip == "off" else ac.max_norm


def apply_model(ac, inp, betas=(0.9, 0.999), eps=1e-8):
    """float64: clip_grad_norm_ over the eight tensors, Adam's default expression -> theta, exp_avg, exp_avg_sq"""
    g, p = inp["grads"].astype(f64), inp["theta"].astype(f64)
    m, v = inp["exp_avg"].astype(f64), inp["exp_avg_sq"].astype(f64)
    if apply_max_norm(ac) is not None:
        g = g * min(1.0, ac.max_norm / (np.sqrt(np.sum(g ** 2)) + 1e-6))
    m = m + (1 - betas[0]) * (g - m)
    v = v * betas[1] + (1 - betas[1]) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - betas[1] ** ac.step) + eps
    p = p - (ac.lr / (1 - betas[0] ** ac.step)) * (m / denom)
    return {"theta": p, "exp_avg": m, "exp_avg_sq": v}


def framework_apply(ac, inp, dtype, device="cpu"):
    """the same with torch's own functions: clip_grad_norm_, torch.optim.Adam (its state set to the case's moments and
    step - 1) -- float64 numpy results"""
    import torch

    dev = lambda a: torch.from_numpy(a.copy()).to(device=device, dtype=dtype)
    bounds = tensor_bounds(ac.H, ac.O, ac.A)
    tensors = {k: [dev(inp[k][lo:hi]) for lo, hi in bounds] for k in ("theta", "exp_avg", "exp_avg_sq", "grads")}
    params = [torch.nn.Parameter(t) for t in tensors["theta"]]
    opt = torch.optim.Adam(params, lr=ac.lr)
    for p, g, m, v in zip(params, tensors["grads"], tensors["exp_avg"], tensors["exp_avg_sq"]):
        p.grad = g
        if ac.step > 1:
            opt.state[p] = {"step": torch.tensor(float(ac.step - 1)), "exp_avg": m, "exp_avg_sq": v}
    if apply_max_norm(ac) is not None:
        torch.nn.utils.clip_grad_norm_(params, ac.max_norm)
    opt.step()
    cat = lambda ts: np.concatenate([t.detach().double().cpu().numpy().reshape(-1) for t in ts])
    return {"theta": cat(params), "exp_avg": cat([opt.state[p]["exp_avg"] for p in params]),
            "exp_avg_sq": cat([opt.state[p]["exp_avg_sq"] for p in params])}


def compare(got, want64, yard32):
    """(ok, err, err_f32, scale, ratio) of one result tensor under the bound"""
    err, err_f32, scale = judge(got, want64, yard32)
    ratio = err / err_f32 if err_f32 else (0.0 if err == 0.0 else float("inf"))
    return within_bound(err, err_f32, scale), err, err_f32, scale, ratio
