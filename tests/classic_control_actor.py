"""Cases, the actor and the host restatement of its arithmetic for the ClassicControl rollouts with a live deterministic
actor (csrc/kernels/classic_control.hip::cc_actor_mean, HipClassicControl<Pendulum|ContinuousMountainCar>EnvRollout_A<width>),
and a host replay of each case on the numpy steps.  Shared by tests/test_classic_control_actor_host.py and
tests/test_gpu_classic_control_actor.py.  Nothing here touches a GPU."""
import numpy as np

from tests import classic_control_cases as cc

f32, f64 = np.float32, np.float64

BOX_ENVS = ("continuous_mountain_car", "pendulum")
ENTRY = {env: cc.ENTRY[env] for env in BOX_ENVS}
# torch.manual_seed(SEED[env]) before FullyConnectedActor(O, [H, H], scale, bias); the head as `make_actor` sets it up.
# Searched on the host (seeds 0 .. 5 x scales 10, 30, 100, 300, 1000, 3000, 10000, in that order) for the first pair at
# which the host replay of EVERY case of the env meets test_classic_control_actor_host.py's conditions against passing
# vacuously: at least a tenth of the means in tanh's linear range and a tenth in its saturated one.
# (ContinuousMountainCar's observations move by ~1e-3 per tick: hence its scale.)
SEED = {"continuous_mountain_car": 3, "pendulum": 0}
HEAD_SCALE = {"continuous_mountain_car": 10000.0, "pendulum": 30.0}
Z_START = 0.25
GEOMETRIES = ("product", (256, 1), (64, 3), (64, "idle"))


def action_range(env, physics=None):
    """(action_scale, action_bias) = ((high - low) / 2, (high + low) / 2) of the env's Box action space"""
    if env == "pendulum":
        return 2.0, 0.0
    lo, hi = (physics or {}).get("min_action", -1.0), (physics or {}).get("max_action", 1.0)
    return (hi - lo) / 2.0, (hi + lo) / 2.0


def actor_weight_count(obs_size, hidden):
    """n_w of the packed actor: W0 [H][OP], b0 [H], W1 [H][H], b1 [H], Wa [H], ba [1], OP = O rounded up to even"""
    O, H = int(obs_size), int(hidden)
    OP = O + (O & 1)
    return OP * H + H + H * H + H + H + 1


class ActorCase(cc.TickCase):
    """...EnvRollout_A<hidden>: E replicas, 11 ticks per launch over episodes of 4 ticks (several restarts per launch,
    launches longer than an episode), "residue" epochs (the rows 8 .. 23 start at 0xfffffffd), batch tensors of 14 rows"""

    def __init__(self, env, hidden, pool=0, scale=1.0, physics=None, E=700):
        name = f"actor-A{hidden}-pool{pool}-scale{scale:g}" + ("-other-physics" if physics else "") + f"-E{E}"
        super().__init__(name, env, E=E, T=4, ticks=11, launches=3, rows=14, pool=pool, physics=physics)
        self.hidden, self.scale = hidden, float(scale)
        self.action_scale, self.action_bias = action_range(env, physics)

    @property
    def ou_params(self):
        return (cc.OU_PARAMS[0], cc.OU_PARAMS[1], self.scale)


CASES = [ActorCase(env, H, pool, scale) for env in BOX_ENVS for H in (32, 64)
         for pool, scale in ((0, 1.0), (7, 1.0), (7, 0.0))] + \
        [ActorCase("continuous_mountain_car", H, 7, 1.0, physics=cc.OTHER_PHYSICS["continuous_mountain_car"])
         for H in (32, 64)] + \
        [ActorCase(env, 32, 0, 1.0, E=1) for env in BOX_ENVS]


def start_observation(env):
    """the observation row every replica holds after a restart: that of the env's seeded fixed start state"""
    start = np.asarray(cc.make_env(env, 4).get_data_dictionary()["state"]["data"], f32).reshape(1, -1)
    return host_obs(env, start)


def make_actor(env, hidden, physics=None):
    """(model, packed float32 numpy weights) of the cases' actor for `env`.  Episodes are 4 ticks from ONE start
    observation, so the head is set up around it: its weights times HEAD_SCALE[env], its bias such that z = Z_START at
    the start observation -- a quarter of the means (the tick after a restart) lie in tanh's linear range, and the later
    ticks of an episode, whose observations have moved away, reach the saturated one."""
    import torch
    from warp_drive_amd.training.models_ddpg import FullyConnectedActor
    from warp_drive_amd.training.policy_kernel import pack_rollout_actor

    torch.manual_seed(SEED[env])
    scale, bias = action_range(env, physics)
    model = FullyConnectedActor(cc.OBS_DIM[env], [hidden, hidden], scale, bias)
    with torch.no_grad():
        model.action_head.weight.mul_(HEAD_SCALE[env])
        z0 = float(actor_z_f64(pack_rollout_actor(model).numpy(), hidden, start_observation(env))[0])
        model.action_head.bias.add_(Z_START - z0)
    return model, pack_rollout_actor(model).numpy()


def _unpack(packed, hidden, obs_size):
    H, O = int(hidden), int(obs_size)
    OP = O + (O & 1)
    w = np.asarray(packed, f32).reshape(-1)
    assert w.size == actor_weight_count(O, H), (w.size, O, H)
    o = 0
    W0 = w[o:o + OP * H].reshape(H, OP); o += OP * H
    b0 = w[o:o + H]; o += H
    W1 = w[o:o + H * H].reshape(H, H); o += H * H
    b1 = w[o:o + H]; o += H
    Wa = w[o:o + H].reshape(1, H); o += H
    return W0, b0, W1, b1, Wa, w[o:o + 1]


def _pad(obs, OP):
    x = np.asarray(obs, f32)
    out = np.zeros((x.shape[0], OP), f32)
    out[:, :x.shape[1]] = x
    return out


def actor_z_f32(packed, hidden, obs):
    """the kernel's pre-activation: acc = bias, then one fused multiply-add per input in index order (emulated in
    float64 as tests/classic_control_policy.py::policy_probabilities does), ReLU after each hidden layer"""
    W0, b0, W1, b1, Wa, ba = _unpack(packed, hidden, np.asarray(obs).shape[1])

    def layer(v, W, b):
        acc = np.broadcast_to(b, (v.shape[0], W.shape[0])).astype(f32).copy()
        for j in range(W.shape[1]):
            acc = (W[None, :, j].astype(f64) * v[:, j:j + 1].astype(f64) + acc.astype(f64)).astype(f32)
        return acc

    h1 = np.maximum(layer(_pad(obs, W0.shape[1]), W0, b0), f32(0))
    h2 = np.maximum(layer(h1, W1, b1), f32(0))
    return layer(h2, Wa, ba)[:, 0]


def actor_mean_f32(packed, hidden, obs, action_scale, action_bias):
    """float32 restatement of cc_actor_mean: the fmaf chain, np.tanh in float32, then one float32 fma"""
    t = np.tanh(actor_z_f32(packed, hidden, obs).astype(f32)).astype(f32)
    return (f64(f32(action_scale)) * t.astype(f64) + f64(f32(action_bias))).astype(f32)


def actor_z_f64(packed, hidden, obs):
    W0, b0, W1, b1, Wa, ba = (a.astype(f64) for a in _unpack(packed, hidden, np.asarray(obs).shape[1]))
    h1 = np.maximum(_pad(obs, W0.shape[1]).astype(f64) @ W0.T + b0, 0.0)
    h2 = np.maximum(h1 @ W1.T + b1, 0.0)
    return (h2 @ Wa.T + ba)[:, 0]


def actor_mean_f64(packed, hidden, obs, action_scale, action_bias):
    """the same network in float64 from the float32 weights (and the float32 scale and bias the kernel is given)"""
    return f64(f32(action_scale)) * np.tanh(actor_z_f64(packed, hidden, obs)) + f64(f32(action_bias))


def host_obs(env, state):
    from warp_drive_amd.envs import classic_control as ccenv

    return ccenv.pendulum_obs(state) if env == "pendulum" else np.asarray(state, f32).copy()


def simulate(case):
    """the case on the host alone (numpy step, the restated actor, the Philox replay of the OU draw and of the pool)
    -> {"tanh": |tanh z| of every mean [launches * ticks, E], "restarts": count, "pool_rows": set}.  It sizes the GPU
    test; it is not its yardstick."""
    from oracle.core_np import ou_step_f32, ou_uniforms, pool_pick, seed_words
    from warp_drive_amd.envs.classic_control import apply_done

    E, T = case.E, case.T
    env_obj = cc.make_env(case.env, T, case.pool, case.physics)
    start = np.asarray(env_obj.get_data_dictionary()["state"]["data"], f32).reshape(-1)
    pool_states = None
    if case.pool:
        pool_states = np.asarray(env_obj.get_reset_pool_dictionary()["state_reset_pool"]["data"], f32)[:, 0]
    obs0 = host_obs(case.env, start[None])[0]
    step = cc.numpy_step(case.env, case.physics)
    _, packed = make_actor(case.env, case.hidden, case.physics)
    state, ts = case.start_states(), case.start_timesteps().astype(np.int64)
    obs = np.broadcast_to(obs0, (E, len(obs0))).astype(f32).copy()   # (the device's observation rows before tick 0)
    epochs, pool_epochs = case.start_epochs(), case.start_pool_epochs()
    k0, k1 = seed_words(cc.SAMPLER_SEED)
    p0, p1 = seed_words(cc.POOL_SEED)
    rows = np.arange(E, dtype=np.uint32)
    ou = np.zeros(E, f32)
    tanh, restarts, pool_rows = [], 0, set()
    for k in range(case.launches * case.ticks):
        z = actor_z_f32(packed, case.hidden, obs)
        tanh.append(np.abs(np.tanh(z.astype(f64))))
        mean = actor_mean_f32(packed, case.hidden, obs, case.action_scale, case.action_bias)
        if case.scale >= 1e-8:
            u1, u2 = ou_uniforms(rows, epochs + np.uint32(k), k0, k1, cc.TICK_TAG)
            ou, a = ou_step_f32(ou, mean, u1, u2, *case.ou_params)
        else:
            a = mean
        state, obs, _, term = step(state, a)
        ts += 1
        fin = np.flatnonzero(apply_done(term, ts, T) > 0)
        restarts += len(fin)
        ts[fin] = 0
        obs[fin] = obs0
        if case.pool:
            pick = pool_pick(fin, pool_epochs[fin], p0, p1, case.pool)
            pool_rows.update(int(r) for r in pick)
            state[fin] = pool_states[pick]
            pool_epochs[fin] += np.uint32(1)
        else:
            state[fin] = start
    return {"tanh": np.stack(tanh), "restarts": restarts, "pool_rows": pool_rows}


def search(seeds=range(6), scales=(10.0, 30.0, 100.0, 300.0, 1000.0, 3000.0, 10000.0)):
    """the search that gave SEED and HEAD_SCALE (`python -m tests.classic_control_actor`): per env, the first (seed, scale)
    at which every case's host replay has a tenth of its means in each range of tanh"""
    found = {}
    for env in BOX_ENVS:
        kept = SEED[env], HEAD_SCALE[env]
        for seed in seeds:
            for scale in scales:
                SEED[env], HEAD_SCALE[env] = seed, scale
                shares = [simulate(c)["tanh"] for c in CASES if c.env == env]
                if all((t < 0.5).mean() >= 0.1 and (t > 0.99).mean() >= 0.1 for t in shares):
                    found.setdefault(env, (seed, scale))
            if env in found:
                break
        SEED[env], HEAD_SCALE[env] = kept
    return found


if __name__ == "__main__":
    print(search())
