"""Cases and yardsticks of the DDPG update kernels (csrc/kernels/ddpg_update.hip; training/ddpg_update_kernels.py).  No GPU.

  * `CASES`: the smallest shapes at which the four launches can still go wrong -- E in {1, 63, 64, 65, 257} (a tile is 128
    rows: one partial tile, tile boundaries inside a row of the batch, several tiles), the five (T, n_step) pairs (two with
    V = 1: the final-row branch only), gamma 1 and 0.99, both widths, both observation sizes (2 with scale 1 / bias 0, 3
    with scale 2 and a bias), the four done patterns, grids smaller than the number of tiles and grids with surplus blocks.
  * the inputs of a case (`inputs`): every network has hidden units whose pre-activation is exactly 0 on every row (a zero
    row of weights and a zero bias, with non-zero weights leaving the unit: relu'(0) = 1 would show), the usual negative
    pre-activations, and -- `saturate` -- an actor whose output sits in tanh's saturation on most rows.
  * `yardstick`: the float64 restatement, a WRITTEN-OUT backward pass in numpy (no autograd), with the mutations the host
    test plants in it; `framework`: torch modules + training/losses.py::DDPG + autograd in a given dtype on a given device
    (float64 on the CPU: what the yardstick must agree with; float32: the error a float32 computation makes).
  * `returns_model`: n_step_returns in numpy, operation for operation, in float32 (bit for bit) or float64.
  * `apply_model` / `framework_apply`: clip + Adam + soft update in float64 numpy / with torch's own functions.
  * the bound is tests/update_kernel_cases.py's: err <= max(4 * err_f32, 2e-6 * scale) per result tensor."""
import collections

import numpy as np

from tests.update_kernel_cases import SENTINEL_BITS, bits, judge, within_bound  # noqa: F401  (shared with the GPU file)

f32, f64 = np.float32, np.float64
TILE = 128
NETS = ("actor", "critic")
PARTS = ("W0", "b0", "W1", "b1", "Wo", "bo")
TENSOR_NAMES = tuple(f"{net}.{part}" for net in NETS for part in PARTS)
DONE_PATTERNS = ("none", "last row", "inside window", "every row")

Case = collections.namedtuple("Case", "name E T n_step gamma H O scale bias done grid saturate seed")


def _case(E, T, n, gamma, H, O, done, grid=None, saturate=False, seed=0):
    scale, bias = (1.0, 0.0) if O == 2 else (2.0, 0.25)
    name = f"E{E}-T{T}n{n}-g{gamma}-H{H}O{O}-{done.replace(' ', '_')}" + (f"-grid{grid}" if grid else "") + ("-sat" if saturate else "")
    return Case(name, E, T, n, gamma, H, O, scale, bias, done, grid, saturate, seed)


# grid: blocks of the gradient launch (None: one per tile)
CASES = (
    _case(1, 2, 1, 1.0, 32, 2, "none", seed=1),
    _case(63, 2, 2, 0.99, 64, 3, "last row", seed=2),                    # V = 1
    _case(64, 5, 5, 0.99, 64, 3, "inside window", seed=3),               # V = 1
    _case(65, 6, 3, 1.0, 32, 3, "inside window", seed=4),                # 260 rows: 3 tiles, boundaries inside a batch row
    _case(257, 10, 5, 0.99, 64, 2, "every row", grid=3, seed=5),         # 1542 rows: 13 tiles on 3 blocks (5 / 4 / 4 trips)
    _case(257, 6, 3, 0.99, 32, 2, "none", grid=12, seed=6),              # 1028 rows: 9 tiles, 3 surplus blocks
    _case(64, 10, 5, 1.0, 64, 2, "last row", grid=2, saturate=True, seed=7),   # 384 rows = 3 whole tiles on 2 blocks
    _case(65, 2, 1, 0.99, 64, 3, "inside window", grid=4, saturate=True, seed=8),  # 130 rows: 2 tiles, 2 surplus blocks
    _case(63, 6, 3, 0.99, 64, 3, "every row", seed=9),
    _case(1, 10, 5, 0.99, 32, 3, "inside window", grid=2, seed=10),      # 6 rows, one surplus block
)


def case_grid(case):
    tiles = -(-(case.T - case.n_step + 1) * case.E // TILE)
    return case.grid or tiles


def net_shapes(H, I):
    return (("W0", (H, I)), ("b0", (H,)), ("W1", (H, H)), ("b1", (H,)), ("Wo", (1, H)), ("bo", (1,)))


def net_floats(H, I):
    return sum(int(np.prod(s)) for _, s in net_shapes(H, I))


def _make_net(rng, H, I, head_gain=1.0):
    """torch's default Linear init (uniform +- 1 / sqrt(fan_in)); units 1 and H - 2 of the first layer and units 2 and
    H - 1 of the second have a zero row and a zero bias: their pre-activation is exactly 0 on every row, and the weights
    that LEAVE them are not zero"""
    net = {}
    for name, shape in net_shapes(H, I):
        fan_in = {"W0": I, "b0": I}.get(name, H)
        net[name] = rng.uniform(-1.0, 1.0, shape).astype(f32) / f32(np.sqrt(fan_in))
    for u in (1, H - 2):
        net["W0"][u], net["b0"][u] = 0.0, 0.0
    for u in (2, H - 1):
        net["W1"][u], net["b1"][u] = 0.0, 0.0
    net["Wo"] = (net["Wo"] * f32(head_gain)).astype(f32)
    return net


def flatten(actor, critic):
    return np.concatenate([net[p].reshape(-1) for net in (actor, critic) for p in PARTS]).astype(f32)


def unflatten(flat, H, O):
    out, at = [], 0
    for I in (O, O + 1):
        net = {}
        for name, shape in net_shapes(H, I):
            n = int(np.prod(shape))
            net[name] = flat[at:at + n].reshape(shape)
            at += n
        out.append(net)
    assert at == flat.size
    return out


def done_flags(case, rng):
    T, E = case.T, case.E
    done = np.zeros((T, E), np.int32)
    if case.done == "last row":
        done[-1] = 1
    elif case.done == "inside window":   # scattered; replica 0 has exactly one, inside the first row's window (so its
        done[:] = rng.random((T, E)) < 0.3   # later windows are whole: with E = 1 they are all there is)
        done[:, 0] = 0
        done[min(case.n_step - 1, T - 1) // 2, 0] = 1
        done[-1, ::2] = 0
    elif case.done == "every row":
        done[:] = 1 + (rng.random((T, E)) < 0.5)   # (2 = "reached the goal": any positive flag ends the episode)
    return done


def inputs(case):
    """{obs [T, E, O], actions [T, E], rewards [T, E], done [T, E] int32, theta, target (flat float32: actor, critic)}"""
    rng = np.random.default_rng(1000 + case.seed)
    T, E, H, O = case.T, case.E, case.H, case.O
    gain = 200.0 if case.saturate else 1.0
    return {
        "obs": rng.standard_normal((T, E, O)).astype(f32),
        "actions": (case.bias + case.scale * rng.uniform(-1.0, 1.0, (T, E))).astype(f32),
        "rewards": (rng.standard_normal((T, E)) - 1.0).astype(f32),
        "done": done_flags(case, rng),
        "theta": flatten(_make_net(rng, H, O, gain), _make_net(rng, H, O + 1)),
        "target": flatten(_make_net(rng, H, O, gain), _make_net(rng, H, O + 1)),
    }


# ------------------------------------------------------------------------------------------------------- returns
def returns_model(rewards, done, next_values, n_step, gamma, dtype=f32, mutate=None):
    """losses.DDPG.n_step_returns on [T, E] arrays, operation for operation in `dtype`.  mutate: "inner without done",
    "next value of row t", "final row as general"."""
    T = rewards.shape[0]
    V = T - n_step + 1
    r, nv = rewards.astype(dtype), next_values.astype(dtype)
    d = (done > 0).astype(dtype)
    one, g = dtype(1), dtype(gamma)
    out = np.empty((V,) + r.shape[1:], dtype)
    first = nv[:V - 1] if mutate == "next value of row t" else nv[n_step - 1:]
    out[:V - 1] = r[n_step - 1:T - 1] + ((one - d[n_step - 1:T - 1]) * g) * first
    if mutate == "final row as general":
        out[V - 1] = r[-1] + ((one - d[-1]) * g) * nv[-1]
    else:
        out[V - 1] = d[-1] * r[-1] + (one - d[-1]) * nv[-1]
    for j in range(1, n_step):
        lo = n_step - 1 - j
        keep = one if mutate == "inner without done" else (one - d[lo:lo + V])
        out = r[lo:lo + V] + (keep * g) * out
    return out


RETURNS_MUTATIONS = ("inner without done", "next value of row t", "final row as general")


def returns_mutation_applies(case, mutation):
    V = case.T - case.n_step + 1
    if mutation == "inner without done":
        return case.n_step > 1 and case.done in ("inside window", "every row")
    if mutation == "next value of row t":
        return case.n_step > 1 and V > 1 and case.done != "every row"   # (a finished row drops its next value)
    return case.done in ("none", "inside window")


# ---------------------------------------------------------------------------------- the written-out float64 passes
def _forward(net, x):
    z1 = x @ net["W0"].T + net["b0"]
    h1 = np.maximum(z1, 0)
    z2 = h1 @ net["W1"].T + net["b1"]
    h2 = np.maximum(z2, 0)
    return h2 @ net["Wo"][0] + net["bo"][0], (x, z1, h1, z2, h2)


def _backward(net, cache, dout, relu_at_zero=0.0):
    """gradient of sum(dout * out) with respect to the parameters and to the input"""
    x, z1, h1, z2, h2 = cache
    step = lambda z: np.where(z > 0, 1.0, np.where(z == 0, relu_at_zero, 0.0))
    d2 = dout[:, None] * net["Wo"][0][None] * step(z2)
    d1 = (d2 @ net["W1"]) * step(z1)
    grads = {"Wo": (dout @ h2)[None], "bo": dout.sum(keepdims=True), "W1": d2.T @ h1, "b1": d2.sum(0), "W0": d1.T @ x,
             "b0": d1.sum(0)}
    return grads, d1 @ net["W0"]


GRADIENT_MUTATIONS = ("relu'(0) = 1", "last tile left out", "critic leak")


def yardstick(case, inp, mutate=None, next_values=None):
    """float64: next_values [T - 1, E], returns [V, E], the twelve gradients, critic_loss, actor_loss.  next_values: use
    these instead of the target networks' (a later stage judged from the inputs it was given)."""
    T, E, O, n = case.T, case.E, case.O, case.n_step
    V = T - n + 1
    cast = lambda net: {k: v.astype(f64) for k, v in net.items()}
    actor, critic = map(cast, unflatten(inp["theta"], case.H, O))
    t_actor, t_critic = map(cast, unflatten(inp["target"], case.H, O))
    obs = inp["obs"].astype(f64)
    mu = lambda net, x: case.scale * np.tanh(_forward(net, x)[0]) + case.bias
    nxt = obs[1:].reshape(-1, O)
    if next_values is None:
        next_values = _forward(t_critic, np.concatenate([nxt, mu(t_actor, nxt)[:, None]], 1))[0].reshape(T - 1, E)
    next_values = np.asarray(next_values, f64).reshape(T - 1, E)
    returns = returns_model(inp["rewards"], inp["done"], next_values, n, case.gamma, f64,
                            mutate if mutate in RETURNS_MUTATIONS else None)
    rows = V * E
    used = rows if mutate != "last tile left out" else (-(-rows // TILE) - 1) * TILE
    x = obs[:V].reshape(rows, O)[:used]
    ret, act = returns.reshape(-1)[:used], inp["actions"].astype(f64)[:V].reshape(-1)[:used]
    at0 = 1.0 if mutate == "relu'(0) = 1" else 0.0
    q, cache = _forward(critic, np.concatenate([x, act[:, None]], 1))
    grads_c, _ = _backward(critic, cache, 2.0 * (q - ret) / rows, at0)
    z, cache_a = _forward(actor, x)
    th = np.tanh(z)
    j, cache_j = _forward(critic, np.concatenate([x, (case.scale * th + case.bias)[:, None]], 1))
    leak, dx = _backward(critic, cache_j, np.full(used, -1.0 / rows), at0)
    grads_a, _ = _backward(actor, cache_a, dx[:, O] * case.scale * (1.0 - th * th), at0)
    if mutate == "critic leak":
        grads_c = {k: grads_c[k] + leak[k] for k in grads_c}
    out = {"next_values": next_values, "returns": returns, "critic_loss": np.sum((ret - q) ** 2) / rows,
           "actor_loss": -np.sum(j) / rows}
    for net, grads in (("actor", grads_a), ("critic", grads_c)):
        for part in PARTS:
            out[f"{net}.{part}"] = grads[part]
    return out


def flat_gradient(result):
    return np.concatenate([np.asarray(result[name]).reshape(-1) for name in TENSOR_NAMES])


# ------------------------------------------------------------------------------------- the framework's computation
def build_modules(case, flat, dtype, device):
    """(actor, critic) modules of training/models_ddpg.py holding the flat float32 parameters, in `dtype` on `device`"""
    import torch
    from warp_drive_amd.training.models_ddpg import FullyConnectedActionValueCritic, FullyConnectedActor

    H, O = case.H, case.O
    actor = FullyConnectedActor(O, (H, H), case.scale, case.bias)
    critic = FullyConnectedActionValueCritic(O + 1, (H, H))
    for module, net in zip((actor, critic), unflatten(np.asarray(flat), H, O)):
        layers = [module.fc["0"][0], module.fc["1"][0], module.action_head if module is actor else module.q_head]
        with torch.no_grad():
            for layer, (w, b) in zip(layers, (("W0", "b0"), ("W1", "b1"), ("Wo", "bo"))):
                layer.weight.copy_(torch.from_numpy(net[w].copy()))
                layer.bias.copy_(torch.from_numpy(net[b].copy()))
    return actor.to(device=device, dtype=dtype), critic.to(device=device, dtype=dtype)


def module_parameters(actor, critic):
    """the twelve parameters in TENSOR_NAMES order"""
    out = []
    for module, head in ((actor, "action_head"), (critic, "q_head")):
        for layer in (module.fc["0"][0], module.fc["1"][0], getattr(module, head)):
            out += [layer.weight, layer.bias]
    return out


def framework(case, inp, dtype, device="cpu", next_values=None):
    """TrainerDDPG's framework update up to the gradients, in torch `dtype` on `device`: the keys of `yardstick`, numpy
    float64 arrays.  next_values: use these [T - 1, E] instead of the target networks' (to judge a later stage from the
    same inputs as the kernel had)."""
    import torch
    from warp_drive_amd.training.losses import DDPG

    T, E, O = case.T, case.E, case.O
    actor, critic = build_modules(case, inp["theta"], dtype, device)
    t_actor, t_critic = build_modules(case, inp["target"], dtype, device)
    dev = lambda a, dt=dtype: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dt)
    obs, actions = dev(inp["obs"]).reshape(T, E, 1, O), dev(inp["actions"]).reshape(T, E, 1, 1)
    rewards, done = dev(inp["rewards"]).reshape(T, E, 1), dev(inp["done"], torch.int32)
    with torch.no_grad():
        nv = t_critic(obs[1:], t_actor(obs[1:])) if next_values is None else dev(next_values).reshape(T - 1, E, 1)
    objective = DDPG(discount_factor_gamma=case.gamma, n_step=case.n_step)
    values, j_values = critic(obs, actions), critic(obs, actor(obs))
    actor_loss, critic_loss, _ = objective.compute_loss_and_metrics(0, actions, rewards, done, values, nv, j_values)
    a_params, c_params = list(actor.parameters()), list(critic.parameters())
    c_grads = torch.autograd.grad(critic_loss, c_params, retain_graph=True)
    a_grads = torch.autograd.grad(actor_loss, a_params)
    by_param = {id(p): g for p, g in zip(a_params + c_params, a_grads + c_grads)}
    num = lambda t: t.detach().double().cpu().numpy()
    out = {"next_values": num(nv).reshape(T - 1, E), "returns": num(objective.n_step_returns(rewards, done, nv)).reshape(-1, E),
           "critic_loss": float(critic_loss.detach()), "actor_loss": float(actor_loss.detach())}
    for name, p in zip(TENSOR_NAMES, module_parameters(actor, critic)):
        out[name] = num(by_param[id(p)])
    return out


# ------------------------------------------------------------------------------------------------- the apply stage
ApplyCase = collections.namedtuple("ApplyCase", "name H O step clip max_norm lr_actor lr_critic tau seed")
APPLY_CASES = tuple(
    ApplyCase(f"H{H}O{O}-step{step}-clip_{clip}", H, O, step, clip, 3.0, 1e-3, 2.5e-4, 0.05, 20 + i)
    for i, (H, O, step, clip) in enumerate([(32, 2, 1, "active"), (64, 3, 1, "inactive"), (64, 2, 1, "off"),
                                            (64, 3, 2, "active"), (32, 3, 2, "inactive"), (32, 2, 2, "off"),
                                            (64, 2, 1000, "active"), (32, 3, 1000, "inactive"), (64, 3, 1000, "off")]))
ZERO_EVERY = 7   # every 7th gradient entry is exactly 0 and so are its moments: Adam must leave that parameter alone


def apply_inputs(ac):
    """theta, target, exp_avg, exp_avg_sq, grads (flat float32).  clip "active": the networks' gradient norms are above
    max_norm; "inactive": far below it; "off": large, and no clipping asked for.  At step 1 the moments are zero."""
    rng = np.random.default_rng(ac.seed)
    n = net_floats(ac.H, ac.O) + net_floats(ac.H, ac.O + 1)
    size = {"active": 0.5, "inactive": 1e-3, "off": 0.5}[ac.clip]
    grads = (size * rng.standard_normal(n)).astype(f32)
    first = ac.step == 1
    exp_avg = np.zeros(n, f32) if first else (0.1 * size * rng.standard_normal(n)).astype(f32)
    exp_avg_sq = np.zeros(n, f32) if first else (size * size * rng.uniform(0.01, 1.0, n)).astype(f32)
    for a in (grads, exp_avg, exp_avg_sq):
        a[::ZERO_EVERY] = 0.0
    return {"theta": rng.uniform(-0.5, 0.5, n).astype(f32), "target": rng.uniform(-0.5, 0.5, n).astype(f32),
            "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq, "grads": grads}


def apply_max_norm(ac):
    return None if ac.clip == "off" else ac.max_norm


def tensor_bounds(H, O):
    out, at = [], 0
    for I in (O, O + 1):
        for _, shape in net_shapes(H, I):
            out.append((at, at + int(np.prod(shape))))
            at += int(np.prod(shape))
    return out


def apply_model(ac, inp, betas=(0.9, 0.999), eps=1e-8):
    """float64: clip_grad_norm_ per network, Adam's default expression, the soft update -> theta, target, exp_avg, exp_avg_sq"""
    g, p, t = (inp[k].astype(f64) for k in ("grads", "theta", "target"))
    m, v = inp["exp_avg"].astype(f64), inp["exp_avg_sq"].astype(f64)
    pa = net_floats(ac.H, ac.O)
    lr = np.where(np.arange(g.size) < pa, ac.lr_actor, ac.lr_critic)
    if apply_max_norm(ac) is not None:
        g = g.copy()
        for lo, hi in ((0, pa), (pa, g.size)):
            g[lo:hi] *= min(1.0, ac.max_norm / (np.sqrt(np.sum(g[lo:hi] ** 2)) + 1e-6))
    m = m + (1 - betas[0]) * (g - m)
    v = v * betas[1] + (1 - betas[1]) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - betas[1] ** ac.step) + eps
    p = p - (lr / (1 - betas[0] ** ac.step)) * (m / denom)
    return {"theta": p, "target": t * (1 - ac.tau) + p * ac.tau, "exp_avg": m, "exp_avg_sq": v}


def framework_apply(ac, inp, dtype, device="cpu"):
    """the same with torch's own functions: clip_grad_norm_, torch.optim.Adam (its state set to the case's moments and
    step - 1), trainer_ddpg.soft_update -- float64 numpy results"""
    import torch
    from warp_drive_amd.training.trainer_ddpg import soft_update

    dev = lambda a: torch.from_numpy(a.copy()).to(device=device, dtype=dtype)
    bounds, pa = tensor_bounds(ac.H, ac.O), net_floats(ac.H, ac.O)
    tensors = {k: [dev(inp[k][lo:hi]) for lo, hi in bounds] for k in ("theta", "target", "exp_avg", "exp_avg_sq", "grads")}

    class Holder(torch.nn.Module):
        def __init__(self, values):
            super().__init__()
            self.values = torch.nn.ParameterList([torch.nn.Parameter(v) for v in values])

    for net, lr in ((slice(0, 6), ac.lr_actor), (slice(6, 12), ac.lr_critic)):
        source, target = Holder(tensors["theta"][net]), Holder(tensors["target"][net])
        params = list(source.parameters())
        opt = torch.optim.Adam(params, lr=lr)
        for p, g, m, v in zip(params, tensors["grads"][net], tensors["exp_avg"][net], tensors["exp_avg_sq"][net]):
            p.grad = g
            if ac.step > 1:
                opt.state[p] = {"step": torch.tensor(float(ac.step - 1)), "exp_avg": m, "exp_avg_sq": v}
        if apply_max_norm(ac) is not None:
            torch.nn.utils.clip_grad_norm_(params, ac.max_norm)
        opt.step()
        soft_update(target, source, ac.tau)
        for i, (p, t) in enumerate(zip(params, target.parameters())):
            k = net.start + i
            tensors["theta"][k], tensors["target"][k] = p.detach(), t.detach()
            tensors["exp_avg"][k], tensors["exp_avg_sq"][k] = opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]
    assert pa == bounds[5][1]
    return {k: np.concatenate([t.double().cpu().numpy().reshape(-1) for t in tensors[k]])
            for k in ("theta", "target", "exp_avg", "exp_avg_sq")}


def compare(got, want64, yard32):
    """(ok, err, err_f32, scale, ratio) of one result tensor under the bound"""
    err, err_f32, scale = judge(got, want64, yard32)
    ratio = err / err_f32 if err_f32 else (0.0 if err == 0.0 else float("inf"))
    return within_bound(err, err_f32, scale), err, err_f32, scale, ratio
