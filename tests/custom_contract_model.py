"""What tests/test_gpu_custom_env_contract.py expects of the three custom-environment kits (include/wd_env.h,
wd_env_tick.h, wd_env_rollout.h), computed on the host alone: the crafted policies and the observation rows of the
logits entries, the preset epochs that lead a launch to the two ends of the draw and through the 2^32 wrap, the crafted
probability rows around the known uniforms, and the host replicas of tests/custom_envs/contract_probe.py.  Shared with
tests/test_custom_env_contract_build.py, which shows on the CPU that no case can pass vacuously."""
import functools

import numpy as np

from oracle.core_np import find_end_draws
from tests import custom_rollout_model as rollout_model
from tests import custom_tick_model as tick_model
from tests.classic_control_cases import NEAR_WINDOW, near_threshold
from tests.classic_control_policy import count_below
from tests.custom_envs.contract_probe import (ODD_AT_RESET, PER_ENV_AT_RESET, REWARD_AT_RESET, SHAPES, SOURCE,
                                              ContractProbe, probe_observation)

f32 = np.float32
TICK_TAG = rollout_model.TICK_TAG
ACTIONS = (1, 2, 5, 8)
UNIFORM_ACTIONS = (2, 3, 5, 7, 8)   # thresholds k / A: representable for 2 and 8, not for 3, 5 and 7
LOGIT_ROWS = 70                     # one wavefront and a partial one
# ---- the draw at preset epochs
END_SEED = 12                       # sampler seed with u == 1.0 and u == 2^-24 on all four words within END_EPOCHS epochs
END_E, END_N, END_EPOCHS, END_TICKS = 3, 70, 65536, 3
# ---- the done flag and the restart: episodes of 4 ticks under launches of 5, 9 and 6 ticks finish at ticks 4, 8, 12, 16
# (inside a launch, a flag standing when the next tick begins) and at tick 20, the LAST tick of the third launch
RESTART_E, RESTART_L, RESTART_LAUNCHES, RESTART_AGENTS = 3, 4, (5, 9, 6), (1, 5, 70, 130)
RESTART_SEED, RESTART_A = 17, 5


# ------------------------------------------------------------------------------------------------------ the network
def logit_rows(F):
    """[70, F]: the probe's signed rows of four time steps of 17 agents, an all-zero row and a row of -0.0"""
    rows = [probe_observation(t, 17, F) for t in range(4)] + [np.zeros((1, F), f32), np.full((1, F), -0.0, f32)]
    out = np.ascontiguousarray(np.concatenate(rows), dtype=f32)
    assert out.shape == (LOGIT_ROWS, F)
    return out


def _sections(F, H, A):
    return [("W0", (H, F)), ("b0", (H,)), ("W1", (H, H)), ("b1", (H,)), ("Wp", (A, H)), ("bp", (A,))]


def unpack(packed, F, H, A):
    out, at = {}, 0
    for name, shape in _sections(F, H, A):
        n = int(np.prod(shape))
        out[name] = np.asarray(packed[at:at + n], dtype=f32).reshape(shape)
        at += n
    assert at == len(packed) == rollout_model.policy_floats(F, H, A)
    return out


def pack(parts, F, H, A):
    return np.ascontiguousarray(np.concatenate([np.asarray(parts[name], dtype=f32).reshape(-1)
                                                for name, _ in _sections(F, H, A)]), dtype=f32)


def random_parts(F, H, A, seed):
    """random weights at O(1) scale (not the framework's default init): first layer and biases 0.5 sigma, the square
    layer and the head 0.3 sigma, so that the logits spread over a few units and every softmax term counts"""
    rng = np.random.RandomState(100000 * seed + 1000 * F + 10 * H + A)
    scale = {"W0": 0.5, "b0": 0.5, "W1": 0.3, "b1": 0.5, "Wp": 0.3, "bp": 0.5}
    return {name: (rng.standard_normal(shape) * scale[name]).astype(f32) for name, shape in _sections(F, H, A)}


def saturated_winners(A):
    return sorted({0, A // 2, A - 1})


def policies(F, H, A):
    """{name: (packed float32, exact)}; `exact`: no expf result can differ between two correct implementations (every
    term is expf(0) = 1 or underflows to 0), so the running sums are compared bit for bit"""
    out = {}
    for seed in (1, 2, 3):
        out[f"random{seed}"] = (pack(random_parts(F, H, A, seed), F, H, A), False)
    dead = random_parts(F, H, A, 4)
    dead["W0"] = (dead["W0"] * f32(0.04)).astype(f32)   # |W0 . x| <= 7 * 8 * 0.02 * (a few sigma) < 5
    dead["b0"] = np.full(H, -5.0, f32)
    out["dead"] = (pack(dead, F, H, A), False)
    if A >= 2:
        for w in saturated_winners(A):
            parts = random_parts(F, H, A, 5)
            parts["Wp"] = np.zeros((A, H), f32)
            parts["bp"] = np.zeros(A, f32)
            parts["bp"][w] = 120.0     # expf(-120) is 0 in float32 (the smallest subnormal is 1.4e-45 = e^-103.3)
            out[f"saturated{w}"] = (pack(parts, F, H, A), True)
        parts = random_parts(F, H, A, 6)
        parts["Wp"] = np.zeros((A, H), f32)
        parts["bp"] = np.zeros(A, f32)
        parts["bp"][:max(1, A // 4)] = -np.inf
        if A >= 3:
            parts["bp"][A - 1] = -np.inf
        out["masked"] = (pack(parts, F, H, A), True)
    return out


def uniform_policy(F, H, A):
    parts = random_parts(F, H, A, 7)
    parts["Wp"] = np.zeros((A, H), f32)
    parts["bp"] = np.full(A, 0.75, f32)
    return pack(parts, F, H, A)


def logit_cases(F, H):
    """[(name, A, packed, exact)] of one (F, H)"""
    cases = [(f"{name}-A{A}", A, packed, exact) for A in ACTIONS for name, (packed, exact) in policies(F, H, A).items()]
    cases += [(f"uniform-A{A}", A, uniform_policy(F, H, A), True) for A in UNIFORM_ACTIONS]
    return cases


def non_finite_policy(F, H, A):
    """a NaN and a +inf planted in W1 of a random policy"""
    parts = random_parts(F, H, A, 1)
    parts["W1"][0, 0] = np.nan
    parts["W1"][1, 1] = np.inf
    return pack(parts, F, H, A)


def policy_logits_fmax(packed, F, H, A, obs):
    """custom_rollout_model.policy_logits with the ReLU as C's fmaxf(acc, 0), which returns the OTHER operand when one is a
    NaN (np.fmax; np.maximum, which the model uses, hands the NaN on): what the header computes under non-finite weights"""
    parts = unpack(packed, F, H, A)

    def layer(v, W, b):
        acc = np.broadcast_to(b, (v.shape[0], W.shape[0])).astype(f32).copy()
        for j in range(W.shape[1]):
            acc = (W[None, :, j].astype(np.float64) * v[:, j:j + 1].astype(np.float64) + acc.astype(np.float64)).astype(f32)
        return acc

    with np.errstate(invalid="ignore", over="ignore"):
        h1 = np.fmax(layer(np.asarray(obs, f32), parts["W0"], parts["b0"]), f32(0))
        h2 = np.fmax(layer(h1, parts["W1"], parts["b1"]), f32(0))
        return layer(h2, parts["Wp"], parts["bp"])


def same_bits_or_both_nan(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | both).all())


def first_layer(packed, F, H, A, obs):
    """the first layer's units BEFORE the ReLU: [R, H]"""
    parts = unpack(packed, F, H, A)
    return np.asarray(obs, np.float64) @ parts["W0"].astype(np.float64).T + parts["b0"].astype(np.float64)


def model_logits_and_sums(packed, H, obs, A):
    with np.errstate(invalid="ignore", over="ignore"):
        return rollout_model.policy_logits(packed, H, obs, A), rollout_model.model_sums(packed, H, obs, A)


# ---------------------------------------------------------------------------------------------- epochs and the ends
@functools.lru_cache(maxsize=None)
def end_draws(seed_lo, seed_hi, n_rows=END_E * END_N, n_epochs=END_EPOCHS):
    """{(word, "hi" | "lo"): [(row, epoch), ...]} of the kit's counter word (5) under the stream tag of "tick", searched
    from the two key words the device holds"""
    return find_end_draws(int(seed_lo), int(seed_hi), TICK_TAG, tick_model.COUNTER_WORD3, n_rows, n_epochs,
                          words=(0, 1, 2, 3))


def preset_epochs(seed_lo, seed_hi, words, ticks=END_TICKS, n_rows=END_E * END_N):
    """(epochs uint32 [rows], roles {row: (word, "hi" | "lo")}, wrap rows): every end of every word in `words` is drawn by
    its row on the LAST tick of a launch of `ticks` ticks; two other rows start at 0xFFFFFFFF and 0xFFFFFFFE and wrap
    within the launch; the rest start at arbitrary epochs.  Fails when an end is not found."""
    ends = end_draws(seed_lo, seed_hi, n_rows)
    epochs = np.random.RandomState(7).randint(0, 2 ** 32, size=n_rows, dtype=np.uint64).astype(np.uint32)
    roles = {}
    for w in words:
        for kind in ("hi", "lo"):
            found = [(r, e) for r, e in ends[(w, kind)] if r not in roles and e >= ticks - 1]
            assert found, f"no {kind} end on word {w} in {END_EPOCHS} epochs of {n_rows} rows"
            roles[found[0][0]] = (w, kind)
            epochs[found[0][0]] = found[0][1] - (ticks - 1)
    wrap = [r for r in range(n_rows) if r not in roles][:2]
    epochs[wrap[0]], epochs[wrap[1]] = 0xFFFFFFFF, 0xFFFFFFFE
    return epochs, roles, wrap


def uniforms(seed_lo, seed_hi, epochs, tick):
    """float32 [rows, 4]: the uniform of every word at `epochs + tick` (mod 2^32)"""
    e = (np.asarray(epochs, np.uint64) + np.uint64(tick)).astype(np.uint32)
    return tick_model.uniform_of(tick_model.tick_bits(np.arange(len(e), dtype=np.uint32), e, seed_lo, seed_hi, TICK_TAG))


def _plateau(A):
    """k equal powers of two that sum to exactly 1.0, then zeros; k a power of two <= max(1, A - 1)"""
    k = 1
    while 2 * k <= max(1, A - 1):
        k *= 2
    row = np.zeros(A, f32)
    row[:k] = f32(1.0 / k)
    return row, k


def crafted_probabilities(u_last, roles, head, A, variant):
    """[rows, A] float32 around the uniform each row's head draws on the LAST tick (u_last [rows]).
    Rows without a role, by row % 4: the first running sum one ulp BELOW u (the pick is 1), EQUAL to u (0: `<` is strict),
    one ulp ABOVE (0), or a seeded Dirichlet row.  The row that draws u == 1.0 on this head: variant 0 the PLATEAU (sums
    reach exactly 1.0 and stay there over trailing zeros: the pick is the last action of non-zero probability), variant 1
    a row whose float32 sum stays BELOW 1.0 (every sum is < u: the count is A, the clamp gives A - 1).  The row that draws
    u == 2^-24: leading zeros (variant 0: the plateau reversed; variant 1: one zero, then all the mass)."""
    rows = len(u_last)
    p = np.random.RandomState(1000 + 10 * head + variant).dirichlet(np.ones(A), size=rows).astype(f32)
    if A >= 2:
        for r in range(rows):
            u = f32(u_last[r])
            first = {0: np.nextafter(u, f32(0)), 1: u, 2: min(np.nextafter(u, f32(2)), f32(1))}.get(r % 4)
            if first is not None:
                p[r] = 0
                p[r, 0], p[r, 1] = first, f32(1) - f32(first)
    plateau, k = _plateau(A)
    for r, (w, kind) in roles.items():
        if w != head:
            continue
        if kind == "hi":
            p[r] = plateau if variant == 0 else np.full(A, f32(1.0 / A) * f32(1 - 2.0 ** -10), f32)
        elif variant == 0:
            p[r] = plateau[::-1]
        else:
            p[r] = 0
            p[r, min(1, A - 1)] = 1
    return np.ascontiguousarray(p)


def tick_plan(seed_lo, seed_hi, head_sizes, variant, ticks=END_TICKS):
    """one launch of the Tick entry at E = 3, N = 70 -> {"epochs", "roles", "wrap", "probs": [per head [3, 70, A]],
    "u": [ticks][rows, 4], "want": int32 [ticks, 3, 70, H], "epochs_after"}"""
    H = len(head_sizes)
    epochs, roles, wrap = preset_epochs(seed_lo, seed_hi, range(H), ticks)
    u = [uniforms(seed_lo, seed_hi, epochs, k) for k in range(ticks)]
    probs = [crafted_probabilities(u[-1][:, h], roles, h, A, variant) for h, A in enumerate(head_sizes)]
    want = np.stack([np.stack([tick_model.pick(probs[h], u[k][:, h]) for h in range(H)], axis=-1) for k in range(ticks)])
    return {"epochs": epochs, "roles": roles, "wrap": wrap, "u": u,
            "probs": [p.reshape(END_E, END_N, -1) for p in probs], "want": want.reshape(ticks, END_E, END_N, H),
            "epochs_after": (epochs.astype(np.uint64) + np.uint64(ticks)).astype(np.uint32)}


def pick_variants(p, u):
    """(the count of sums < u without the clamp, the clamped count with <= in place of <): what two wrong picks give"""
    p = np.asarray(p, f32)
    cum = np.zeros(p.shape[:-1], f32)
    lt = np.zeros(p.shape[:-1], np.int64)
    le = np.zeros(p.shape[:-1], np.int64)
    for i in range(p.shape[-1]):
        cum = p[..., i] if i == 0 else (cum + p[..., i]).astype(f32)
        lt += cum < u
        le += cum <= u
    return lt, np.minimum(le, p.shape[-1] - 1)


# ------------------------------------------------------------------------------------- the rollout at preset epochs
def end_policies(F, H):
    """[(name, A, packed, crafted)] of the rollout at preset epochs: the masked, saturated and uniform policies (no
    excused draw: cap 0) and one random policy (near_cap's rule)"""
    out = [("masked-A8", 8, policies(F, H, 8)["masked"][0], True), ("masked-A2", 2, policies(F, H, 2)["masked"][0], True)]
    out += [(f"saturated{w}-A5", 5, policies(F, H, 5)[f"saturated{w}"][0], True) for w in saturated_winners(5)]
    # (A = 2: an exact threshold; A = 5: thresholds that are not representable.  A = 8 is left to the logits test: one of
    # the 630 modelled draws lies within NEAR_WINDOW of k / 8, and these cases excuse nothing)
    out += [(f"uniform-A{A}", A, uniform_policy(F, H, A), True) for A in (2, 5)]
    out += [("random1-A5", 5, policies(F, H, 5)["random1"][0], False)]
    return out


def near_inner_threshold(cum, u, window=NEAR_WINDOW):
    """near_threshold over the thresholds strictly between 0 and 1.  A crafted policy's thresholds of exactly 0.0 (in
    front of a masked or losing action) and exactly 1.0 (behind the last action of non-zero probability) are sums of
    exact zeros on every correct implementation -- expf(-inf) and expf of a gap over 110 are 0 -- and the end draws
    u == 2^-24 and u == 1.0 are aimed at them on purpose: they are what is tested, not what is excused."""
    cum = np.asarray(cum, f32)
    if cum.shape[1] < 2:
        return np.zeros(len(cum), bool)
    t = cum[:, :-1].astype(np.float64)
    return ((np.abs(t - np.asarray(u, np.float64)[:, None]) < window) & (t > 0) & (t < 1)).any(axis=1)


def rollout_plan(seed_lo, seed_hi, F, H, A, packed, crafted=False, ticks=END_TICKS):
    """the Rollout entry at E = 3, N = 70 with episodes longer than the launch: the observation before tick k is the
    probe's at time step k -> {"epochs", "roles", "wrap", "obs" [ticks][rows, F], "cum", "u" [ticks][rows], "want"
    [ticks, rows], "near" [ticks, rows] bool (crafted: near_inner_threshold), "epochs_after"}"""
    near = near_inner_threshold if crafted else near_threshold
    epochs, roles, wrap = preset_epochs(seed_lo, seed_hi, (0,), ticks)
    obs = [np.tile(probe_observation(k, END_N, F), (END_E, 1)) for k in range(ticks)]
    cum = [model_logits_and_sums(packed, H, o, A)[1] for o in obs]
    u = [uniforms(seed_lo, seed_hi, epochs, k)[:, 0] for k in range(ticks)]
    return {"epochs": epochs, "roles": roles, "wrap": wrap, "obs": obs, "cum": cum, "u": u,
            "want": np.stack([count_below(c, x) for c, x in zip(cum, u)]),
            "near": np.stack([near(c, x) for c, x in zip(cum, u)]),
            "epochs_after": (epochs.astype(np.uint64) + np.uint64(ticks)).astype(np.uint32)}


# ---------------------------------------------------------------------------------------------------- host replicas
def restart_config(N, F, A=RESTART_A):
    return dict(num_agents=N, episode_length=RESTART_L, n_actions=A, features=F, num_envs=RESTART_E)


class HostProbe(rollout_model.HostReplicas):
    """E host replicas of ContractProbe: `step(actions)` as HostReplicas, + what every device array holds behind it"""

    def __init__(self, config):
        super().__init__(ContractProbe, config, config["num_envs"])
        self.rewards = np.full((len(self.envs), self.N), REWARD_AT_RESET, f32)
        self.done = np.zeros(len(self.envs), np.int32)
        self.inside = self.on_last = 0

    def step(self, actions, last_tick=False):
        rewards, done = super().step(actions)
        self.rewards = np.where(done[:, None] > 0, REWARD_AT_RESET, rewards).astype(f32)  # restored behind the record
        self.done = done
        self.inside += int(done.sum()) if not last_tick else 0
        self.on_last += int(done.sum()) if last_tick else 0
        return rewards, done

    def state(self):
        return {"per_env": self.array("per_env").reshape(len(self.envs)), "odd": self.array("odd"),
                "wide": self.array("wide"), "_timestep_": self.timesteps(), "_done_": self.done,
                "seen_done": np.zeros((len(self.envs), self.N), np.int32)}


def restart_probabilities(N, A=RESTART_A):
    return np.ascontiguousarray(np.random.RandomState(50 + N).dirichlet(np.ones(A), size=(RESTART_E, N)).astype(f32))


__all__ = ["SHAPES", "SOURCE", "ContractProbe", "ODD_AT_RESET", "PER_ENV_AT_RESET", "REWARD_AT_RESET"]
