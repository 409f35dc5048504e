"""Cases, a host replay and a numpy model for the evaluation kernels: HipClassicControl<CartPole|Acrobot|MountainCar>
EnvEvaluate_H<32|64> (one episode of every replica in one launch, greedy or sampled; csrc/kernels/cartpole.hip,
classic_control.hip) and HipEvaluateAccumulate (csrc/kernels/wd_core.hip).  Shared by
tests/test_classic_control_evaluate_host.py (every case replayed on the host alone must reach the coverage it is there
for) and tests/test_gpu_evaluate.py (the same cases on the device).  Nothing here touches a GPU.

The replay takes the step as an argument: the numpy step on the host (it sizes the cases), the device's Step kernel in
the GPU test (a float64 cos may differ from the host's in its last bit).  What is shared bit for bit either way is every
draw, the restated network and the float32 sums."""
import numpy as np

from oracle.core_np import seed_words, single_head_tick_uniform
from tests import classic_control_cases as cc
from tests.classic_control_policy import count_below, policy_probabilities, running_sums

F32 = np.float32
ENVS = cc.DISCRETE                     # cartpole, acrobot, mountain_car
WIDTHS = (32, 64)
MODES = ("greedy", "sampled")
N_ACTIONS = {"cartpole": 2, "acrobot": 3, "mountain_car": 3}
E_PARITY = 1501                        # (128, 3) takes three trips of the grid-stride loop only from 1153 replicas on
SMALL_E = (1, 65)                      # one replica; one replica into the second wavefront
GEOMETRIES = cc.ROLLOUT_GEOMETRIES     # (64, None), (128, 3), (64, "idle")
SENTINEL_F, SENTINEL_I, SURPLUS = F32(-7.5), np.int32(-77), 3
# seeds of the policy (torch.manual_seed, per env and width) and episode lengths, chosen so that the HOST replay alone meets
# the conditions tests/test_classic_control_evaluate_host.py asserts (terminations on >= 3 ticks, time-outs, every action's
# share >= 0.02 in greedy mode too: MountainCar's two small observations move an argmax only under few of the seeds)
POLICY_SEED = {("cartpole", 32): 10, ("cartpole", 64): 12, ("acrobot", 32): 10, ("acrobot", 64): 11,
               ("mountain_car", 32): 75, ("mountain_car", 64): 81}
EPISODE_LENGTH = {"cartpole": 24, "acrobot": 20, "mountain_car": 16}


class EvalCase:
    """one env x hidden width x mode at E replicas; timesteps: "zero" or "residue" (row % 4: the time-out arrives that
    much sooner)"""

    def __init__(self, env, hidden, mode, E=E_PARITY, timesteps="zero"):
        assert env in ENVS and hidden in WIDTHS and mode in MODES
        self.env, self.hidden, self.mode, self.E, self.timesteps = env, hidden, mode, E, timesteps
        self.T, self.A = EPISODE_LENGTH[env], N_ACTIONS[env]
        self.greedy = mode == "greedy"
        self.pool = 0 if env == "cartpole" else 7     # (a pool the launch must leave alone)
        self.physics = None
        self.name = f"{env}-H{hidden}-{mode}-E{E}" + ("" if timesteps == "zero" else "-t" + timesteps)

    def __repr__(self):
        return self.name

    def policy(self):
        """(model, packed float32 numpy weights): FullyConnected(O, [A], [H, H]), the head's weights times 6"""
        import torch
        from warp_drive_amd.training.models import FullyConnected
        from warp_drive_amd.training.policy_kernel import pack_rollout_policy

        torch.manual_seed(POLICY_SEED[self.env, self.hidden])
        model = FullyConnected(cc.OBS_DIM[self.env], [self.A], [self.hidden, self.hidden])
        with torch.no_grad():
            model.policy_head[0].weight.mul_(cc.HEAD_SCALE)
        return model, pack_rollout_policy(model).numpy()

    def start(self):
        """(state [E, S], timestep [E]): spread states, then the crafted rows of classic_control_cases (MountainCar's
        goal rows end with done 2; its goal on the last tick is a time-out) as far as they fit"""
        state = cc.spread_states(self.env, np.random.RandomState(11), self.E)
        ts = np.zeros(self.E, np.int32) if self.timesteps == "zero" else (np.arange(self.E) % 4).astype(np.int32)
        for i, (s, _, t0, _) in enumerate(cc.crafted_step_rows(self.env, self.T)[: self.E]):
            state[i] = np.asarray(s, F32)
            ts[i] = 0 if t0 is None else t0
        return state, ts

    def start_epochs(self):
        """row % 4 (a launch starts at every residue of the Philox quad); the rows WRAP_ROWS cross 2^32"""
        ep = (np.arange(self.E, dtype=np.uint32) % 4).astype(np.uint32)
        if self.E >= 63:
            ep[cc.WRAP_ROWS] = cc.WRAP_EPOCH
        return ep

    def near_cap(self, decisions):
        return (2 + decisions // 50000) * (self.A - 1)


PARITY_CASES = [EvalCase(env, H, mode) for env in ENVS for H in WIDTHS for mode in MODES]
SMALL_CASES = [EvalCase(env, 32, mode, E=E) for env in ENVS for mode in MODES for E in SMALL_E]
RESIDUE_CASES = [EvalCase(env, 32, "greedy", timesteps="residue") for env in ENVS]


def first_maximum(p):
    """the standalone sampler's strict-'<' scan"""
    p = np.asarray(p, F32)
    best, act = p[:, 0].copy(), np.zeros(len(p), np.int32)
    for i in range(1, p.shape[1]):
        better = best < p[:, i]
        best = np.where(better, p[:, i], best)
        act = np.where(better, i, act).astype(np.int32)
    return act


def near_top_two(p, window=cc.NEAR_WINDOW):
    p = np.sort(np.asarray(p, np.float64), axis=1)
    if p.shape[1] < 2:
        return np.zeros(len(p), bool)
    return (p[:, -1] - p[:, -2]) < window


def replay(case, ticks=None, step=None, trace=None, packed=None):
    """The evaluation on the host: per tick the restated network on the observation, the action (first maximum, or the
    number of running sums below the Philox uniform of (row, epoch0 + k)), the step, sum += reward / steps += 1 /
    done = time-out ? 1 : terminal code, up to the first done or `ticks`.  `step` (default: the numpy step) maps
    (state [E, S], action [E]) to (state, obs, reward, terminal code).  With `trace` [>= ticks, E] (the device's recorded
    actions) the replay FOLLOWS the device: a recorded action of a running replica must be the host's or the decision
    must lie in the near-tie set (a uniform within 2e-6 of a running sum; greedy: the top two probabilities within 2e-6).
    Returns a dict: reward_sum, steps, done, actions [ticks, E] (-1 where the replica no longer ran), epochs (the epoch
    words after a sampled launch), near (decisions in the near-tie set), decisions, followed (recorded actions that
    were not the host's), end_ticks (terminations per tick), timeouts, counts (per action)."""
    from warp_drive_amd.envs.classic_control import apply_done

    E, T, A = case.E, case.T, case.A
    ticks = T if ticks is None else int(ticks)
    step = cc.numpy_step(case.env) if step is None else step
    packed = case.policy()[1] if packed is None else packed
    state, ts = case.start()
    ts = ts.astype(np.int64)
    obs = cc.host_obs(case.env, state) if case.env != "cartpole" else state.copy()
    epoch0 = case.start_epochs()
    k0, k1 = seed_words(cc.SAMPLER_SEED)
    running = np.ones(E, bool)
    total, steps, done = np.zeros(E, F32), np.zeros(E, np.int32), np.zeros(E, np.int32)
    actions = np.full((ticks, E), -1, np.int32)
    near = decisions = followed = timeouts = 0
    counts, end_ticks = np.zeros(A, np.int64), {}
    for k in range(ticks):
        if not running.any():
            break
        p = policy_probabilities(packed, case.hidden, obs, A)
        if case.greedy:
            host, close = first_maximum(p), near_top_two(p)
        else:
            u = single_head_tick_uniform(E, epoch0 + np.uint32(k), k0, k1, cc.TICK_TAG)
            cum = running_sums(p)
            host, close = count_below(cum, u), cc.near_threshold(cum, u)
        a = host.copy()
        if trace is not None:
            got = np.asarray(trace[k], np.int32).reshape(E)
            assert ((got[running] >= 0) & (got[running] < A)).all(), (case.name, k)
            bad = running & (got != host)
            assert close[bad].all(), (case.name, k, np.flatnonzero(bad & ~close)[:5], p[bad & ~close][:5])
            followed += int(bad.sum())
            a[running] = got[running]
        near += int(close[running].sum())
        decisions += int(running.sum())
        counts += np.bincount(a[running], minlength=A)
        actions[k, running] = a[running]
        ns, no, rew, term = step(state, a)
        r = running
        state[r], obs[r] = np.asarray(ns, F32)[r], np.asarray(no, F32)[r]
        total[r] = (total[r] + np.asarray(rew, F32).reshape(E)[r]).astype(F32)
        steps[r] += 1
        ts[r] += 1
        d = apply_done(np.asarray(term).reshape(E), ts, T)
        fin = r & (d > 0)
        done[fin] = d[fin]
        timeouts += int((fin & (ts == T)).sum())
        ended = int((fin & (ts < T)).sum())
        if ended:
            end_ticks[k] = ended
        running = r & ~fin
    epochs = epoch0 if case.greedy else (epoch0 + steps.astype(np.uint32)).astype(np.uint32)
    return {"reward_sum": total, "steps": steps, "done": done, "actions": actions, "epochs": epochs, "near": near,
            "decisions": decisions, "followed": followed, "end_ticks": end_ticks, "timeouts": timeouts, "counts": counts}


# ------------------------------------------------------------------------------------------ HipEvaluateAccumulate
ACC_E, ACC_TICKS, ACC_AGENTS, ACC_BLOCKS = 130, 12, (1, 5, 105), (64, 256)


def accumulate_inputs(N, E=ACC_E, ticks=ACC_TICKS):
    """(rewards [ticks, E, N] float32, done [ticks, E] int32): random flags, then the crafted replicas -- 0: done on tick
    0; 1: never done; 2: done twice (the second episode must not count); 3: done value 2; 4: done on the last tick"""
    rng = np.random.RandomState(100 + N)
    rewards = rng.uniform(-3, 3, size=(ticks, E, N)).astype(F32)
    done = (rng.uniform(size=(ticks, E)) < 0.12).astype(np.int32)
    done[:, :5] = 0
    done[0, 0] = 1
    done[3, 2] = done[7, 2] = 1
    done[5, 3] = 2
    done[ticks - 1, 4] = 1
    return rewards, done


def accumulate_model(rewards, done):
    """numpy model of HipEvaluateAccumulate launched once per tick: (reward_sum [E, N] float32, end_tick [E] int32)"""
    ticks, E, N = rewards.shape
    total, end = np.zeros((E, N), F32), np.full(E, -1, np.int32)
    for k in range(ticks):
        live = (end < 0) | (end == k)
        total[live] = (total[live] + rewards[k][live]).astype(F32)
        end[live & (done[k] != 0)] = k
    return total, end
