"""Host restatement of the policy network the ClassicControl rollout kernels evaluate on every tick
(csrc/kernels/classic_control.hip::cc_policy_cum, HipClassicControl<Acrobot|MountainCar>EnvRollout_H<width>), and a host
replay of such a rollout on the numpy steps.  Shared by tests/test_classic_control_policy_host.py and
tests/test_gpu_classic_control_policy.py."""
import numpy as np

f32 = np.float32

# the parity test's sizes (tests/test_gpu_classic_control_policy.py) and the policy it runs: torch.manual_seed(SEED[env]),
# FullyConnected(O, [3], [H, H]), the head's weights times HEAD_SCALE -- chosen so that the HOST replay below, alone, meets
# the test's conditions against passing vacuously (tests/test_classic_control_policy_host.py checks that on the CPU)
PARITY = {"E": 1501, "episode_length": 23, "ticks": 12, "launches": 5, "sampler_seed": 4, "pool_seed": 23, "env_seed": 5}
SEED = {"acrobot": 5, "mountain_car": 5}
HEAD_SCALE = {"acrobot": 6.0, "mountain_car": 6.0}
OBS_SIZE = {"acrobot": 6, "mountain_car": 2}


def policy_weight_count(obs_size, hidden, n_actions):
    O, H, A = int(obs_size), int(hidden), int(n_actions)
    return O * H + H + H * H + H + A * H + A


def policy_probabilities(packed, hidden, obs, n_actions):
    """float32 restatement of the in-kernel rollout policy for an observation of any width (oracle/cartpole_np.py::
    policy_probabilities is the four-float case): two hidden layers of `hidden` ReLU units and one softmax head over
    `packed` = [W0 [H][O], b0, W1 [H][H], b1, Wp [A][H], bp]; acc = bias, then one fused multiply-add per input in
    index order (emulated in float64: the product of two float32 is exact there; the single rounding of the sum to
    float32 can differ from a hardware fma in the last bit about once in 2^29 operations), ReLU after each hidden
    layer, softmax with the maximum subtracted, the sum in action order, one division per action.
    obs [E, O] -> probs [E, A]."""
    H, A = int(hidden), int(n_actions)
    x = np.asarray(obs, dtype=f32)
    O = int(x.shape[1])
    w = np.asarray(packed, dtype=f32).reshape(-1)
    assert w.size == policy_weight_count(O, H, A), (w.size, O, H, A)
    o = 0
    W0 = w[o:o + O * H].reshape(H, O); o += O * H
    b0 = w[o:o + H]; o += H
    W1 = w[o:o + H * H].reshape(H, H); o += H * H
    b1 = w[o:o + H]; o += H
    Wp = w[o:o + A * H].reshape(A, H); o += A * H
    bp = w[o:o + A]

    def layer(v, W, b):
        acc = np.broadcast_to(b, (v.shape[0], W.shape[0])).astype(f32).copy()
        for j in range(W.shape[1]):
            acc = (W[None, :, j].astype(np.float64) * v[:, j:j + 1].astype(np.float64) + acc.astype(np.float64)).astype(f32)
        return acc

    h1 = np.maximum(layer(x, W0, b0), f32(0))
    h2 = np.maximum(layer(h1, W1, b1), f32(0))
    logits = layer(h2, Wp, bp)
    e = np.exp((logits - logits.max(axis=1, keepdims=True)).astype(f32)).astype(f32)
    s = np.zeros(e.shape[0], f32)
    for a in range(A):
        s = (s + e[:, a]).astype(f32)
    return (e / s[:, None]).astype(f32)


def running_sums(probs):
    """the float32 running sums the inverse-CDF draw compares the uniform with"""
    p = np.asarray(probs, dtype=f32)
    cum = np.empty_like(p)
    acc = np.zeros(p.shape[0], f32)
    for a in range(p.shape[1]):
        acc = p[:, a].copy() if a == 0 else (acc + p[:, a]).astype(f32)
        cum[:, a] = acc
    return cum


def count_below(cum, u):
    """the kernel's action: the number of running sums below u, clamped to the last action"""
    cnt = (np.asarray(cum, f32) < np.asarray(u, f32)[:, None]).sum(axis=1)
    return np.minimum(cnt, cum.shape[1] - 1).astype(np.int32)


def make_policy(env, hidden):
    """(model, packed float32 numpy weights) of the parity test's policy for `env`"""
    import torch
    from warp_drive_amd.training.models import FullyConnected
    from warp_drive_amd.training.policy_kernel import pack_rollout_policy

    torch.manual_seed(SEED[env])
    model = FullyConnected(OBS_SIZE[env], [3], [hidden, hidden])
    with torch.no_grad():  # decisive enough that the three actions occur with varied probabilities
        model.policy_head[0].weight.mul_(HEAD_SCALE[env])
    return model, pack_rollout_policy(model)


def device_class(env):
    from warp_drive_amd.envs import classic_control as cc

    return {"acrobot": cc.CUDAClassicControlAcrobotEnv, "mountain_car": cc.CUDAClassicControlMountainCarEnv}[env]


def numpy_step(env):
    from warp_drive_amd.envs import classic_control as cc

    return {"acrobot": cc.acrobot_step, "mountain_car": cc.mountain_car_step}[env]


def host_rollout(env, hidden, pool, stream_tag, packed=None):
    """The parity test's rollout replayed on the host alone: the numpy step, the policy restatement above (on `packed`
    float32 numpy weights; default: the parity test's policy), the Philox
    draws of the sampler and of the pool key from their seeds.  (The numpy step may differ from the device's by an ulp:
    this replay sizes the test, it is not its yardstick.)  Returns {"finished", "action_counts" [3], "pool_rows"}."""
    from oracle.core_np import pool_pick, seed_words, single_head_tick_uniform
    from warp_drive_amd.envs.classic_control import apply_done

    c = PARITY
    E, T = c["E"], c["episode_length"]
    e = device_class(env)(episode_length=T, seed=c["env_seed"], reset_pool_size=pool)
    start = np.asarray(e.get_data_dictionary()["state"]["data"], f32).reshape(-1)
    pool_states = None
    if pool:
        pool_states = np.asarray(e.get_reset_pool_dictionary()["state_reset_pool"]["data"], f32)[:, 0]
    step = numpy_step(env)
    if packed is None:
        packed = make_policy(env, hidden)[1].numpy()
    k0, k1 = seed_words(c["sampler_seed"])
    p0, p1 = seed_words(c["pool_seed"])
    state = np.broadcast_to(start, (E, start.size)).astype(f32).copy()
    obs0 = np.asarray(e._obs(start), f32).reshape(-1)
    obs = np.broadcast_to(obs0, (E, obs0.size)).astype(f32).copy()
    ts = np.zeros(E, np.int64)
    pool_epoch = np.zeros(E, np.uint32)
    finished, counts, rows = 0, np.zeros(3, np.int64), set()
    for tick in range(c["ticks"] * c["launches"]):
        u = single_head_tick_uniform(E, np.full(E, tick, np.uint32), k0, k1, stream_tag)
        a = count_below(running_sums(policy_probabilities(packed, hidden, obs, 3)), u)
        counts += np.bincount(a, minlength=3)
        state, obs, _, term = step(state, a)
        ts += 1
        done = apply_done(term, ts, T)
        fin = np.flatnonzero(done > 0)
        finished += len(fin)
        ts[fin] = 0
        obs[fin] = obs0
        if pool:
            pick = pool_pick(fin, pool_epoch[fin], p0, p1, pool)
            rows.update(int(r) for r in pick)
            state[fin] = pool_states[pick]
            pool_epoch[fin] += np.uint32(1)
        else:
            state[fin] = start
    return {"finished": finished, "action_counts": counts, "pool_rows": rows}
