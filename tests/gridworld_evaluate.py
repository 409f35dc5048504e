"""Cases, start states and a host replay for the TagGridWorld evaluation kernels HipTagGridWorldEvaluate_N5_H<32|64>
(one episode of every replica in one launch with the tagger and runner networks inside the kernel, greedy or sampled;
csrc/kernels/tag_gridworld_n5.hip, gw5_evaluate in tag_gridworld_n5_common.h).  Shared by tests/test_gridworld_evaluate_host.py (every case replayed on the host
alone must reach the coverage it is there for) and tests/test_gpu_gridworld_evaluate.py (the same cases on the device).
Nothing here touches a GPU.

After `reset_all_envs()` every replica holds the same start cells, so an evaluation from there is ONE trajectory E times
over (greedy at E = 257, T = 23: one end tick, no tag).  The cases therefore start every replica from its own state:
positions uniform on 0 .. L per replica and agent, `_timestep_` = row % 4, the observation rows the oracle's for exactly
that state."""
import zlib

import numpy as np

from oracle.core_np import seed_words, single_head_tick_uniform
from oracle.tag_gridworld_np import STEP_ACTIONS, TagGridWorldOracle, policy_probabilities, running_sums

F32 = np.float32
N, F, A = 5, 21, 5
WIDTHS = (32, 64)
MODES = ("greedy", "sampled")
E_PARITY = 257                       # 22 groups of 12 replicas, the last one of 5
EPB = 12                             # replicas per block (one wavefront)
SIZES = ((10, 23), (4, 16))          # (grid_length, episode_length) of the parity cases
TICK_TAG = np.int32(zlib.crc32(b"tick") & 0x7FFFFFFF)   # function_manager._stream_tag("tick")
SAMPLER_SEED, START_SEED = 5, 11
WRAP_EPOCH, WRAP_ROWS = 0xFFFFFFFD, slice(8, 24)   # sixteen replicas whose words cross 2^32 within three ticks
NEAR_WINDOW = 2e-6                   # device expf vs numpy exp: inside it the device may decide otherwise
SENTINEL_F, SENTINEL_I, SURPLUS = F32(-7.5), np.int32(-1), 3
HEAD_SCALE, FIRST_LAYER_SCALE = (4.0, 7.0), 2.0   # tagger, runner: as test_gridworld_rollout_with_the_policies_inside_the_kernel
REWARDS = dict(wall_hit_penalty=0.1, tag_reward_for_tagger=10.0, tag_penalty_for_runner=2.0, step_cost_for_tagger=0.01)
# torch.manual_seed of the two policies per (hidden, grid_length, mode): the first seed from 1 on under which the HOST
# replay meets every condition tests/test_gridworld_evaluate_host.py asserts (greedy needs three actions with a share of
# at least 0.05 each, which not every seed gives: a greedy policy of this size may settle on two moves) with NO decision
# inside the 2e-6 window on the host -- the cap of 2 + decisions // 50000 is then all headroom for the device.
# `python -m tests.gridworld_evaluate` repeats the search and prints the table.
POLICY_SEED = {
    (32, 10, "greedy"): 3, (32, 10, "sampled"): 1, (64, 10, "greedy"): 6, (64, 10, "sampled"): 1,
    (32, 4, "greedy"): 2, (32, 4, "sampled"): 1, (64, 4, "greedy"): 1, (64, 4, "sampled"): 2,
    # grid_length 63 (BOUND_CASES) is there for the last entry of the quotient table, not for tags: five agents on 4096
    # cells rarely meet within 12 ticks (no sampled seed below 200 gives 8 end ticks), so it is held to `reaches_bound`
    (32, 63, "greedy"): 1, (32, 63, "sampled"): 1,
}
# (threads per block is always 64: blocks are one wavefront) grids: the host's own, 3 blocks (8 trips of the stride
# loop at E = 257), the host's + 2 idle blocks
GEOMETRIES = ("product", 3, "idle")


def grid_blocks(E, geom):
    groups = -(-E // EPB)
    return groups if geom == "product" else groups + 2 if geom == "idle" else int(geom)


class GwCase:
    """one hidden width x mode at E replicas on a grid of side `grid_length` + 1 with episodes of T ticks"""

    def __init__(self, hidden, mode, grid_length=10, T=23, E=E_PARITY):
        assert hidden in WIDTHS and mode in MODES
        self.hidden, self.mode, self.L, self.T, self.E = hidden, mode, int(grid_length), int(T), int(E)
        self.greedy = mode == "greedy"
        self.name = f"H{hidden}-{mode}-L{grid_length}-T{T}-E{E}"

    def __repr__(self):
        return self.name

    def env_config(self):
        return dict(num_taggers=N - 1, grid_length=self.L, episode_length=self.T, use_full_observation=True, **REWARDS)

    def policies(self, seed=None):
        """([tagger model, runner model], [packed float32 numpy weights] * 2): FullyConnected(21, [5], [H, H]), the
        head's weights x 4 / x 7 and the first layer's x 2"""
        import torch
        from warp_drive_amd.training.models import FullyConnected
        from warp_drive_amd.training.policy_kernel import pack_gridworld_policy

        torch.manual_seed(POLICY_SEED[self.hidden, self.L, self.mode] if seed is None else seed)
        models = [FullyConnected(F, [A], [self.hidden, self.hidden]) for _ in range(2)]
        with torch.no_grad():
            for m, scale in zip(models, HEAD_SCALE):
                m.policy_head[0].weight.mul_(scale)
                m.fc["0"][0].weight.mul_(FIRST_LAYER_SCALE)
        return models, [pack_gridworld_policy(m).numpy().copy() for m in models]

    def oracle(self):
        """the oracle holding the start state: positions uniform on 0 .. L, timestep = row % 4, the observation of
        exactly that state"""
        orc = TagGridWorldOracle(num_envs=self.E, **self.env_config())
        rng = np.random.RandomState(START_SEED)
        orc.loc_x = rng.randint(0, self.L + 1, size=(self.E, N)).astype(np.int32)
        orc.loc_y = rng.randint(0, self.L + 1, size=(self.E, N)).astype(np.int32)
        orc.timestep = (np.arange(self.E) % 4).astype(np.int32)
        orc.obs = orc.generate_observation()
        return orc

    def start_epochs(self):
        """[E, 5] uint32: word % 4 (a launch starts at every residue of the Philox quad); the replicas WRAP_ROWS start
        three ticks before 2^32"""
        ep = (np.arange(self.E * N, dtype=np.uint32) % 4).astype(np.uint32).reshape(self.E, N)
        if self.E >= 24:
            ep[WRAP_ROWS] = WRAP_EPOCH
        return ep

    def near_cap(self, decisions):
        """the cap of test_gridworld_rollout_with_the_policies_inside_the_kernel"""
        return 2 + decisions // 50000


PARITY_CASES = [GwCase(H, mode, L, T) for (L, T) in SIZES for H in WIDTHS for mode in MODES]
SMALL_CASES = [GwCase(32, mode, E=E) for mode in MODES for E in (1, 13)]   # one replica; a one-replica second group
BOUND_CASES = [GwCase(32, mode, grid_length=63, T=12) for mode in MODES]   # the last entry of the quotient table


def probabilities(packed, hidden, obs):
    """[E, 5, 21] float32 observation rows -> [E, 5, 5] probabilities: the tagger network on agents 0 - 3, the runner's
    on agent 4"""
    E = obs.shape[0]
    p = np.empty((E, N, A), F32)
    p[:, :N - 1] = policy_probabilities(packed[0], hidden, obs[:, :N - 1].reshape(-1, F)).reshape(E, N - 1, A)
    p[:, N - 1] = policy_probabilities(packed[1], hidden, obs[:, N - 1])
    return p


def first_maximum(p):
    """best = 0; for a in 1 .. 4: if p[best] < p[a]: best = a"""
    best, act = p[..., 0].copy(), np.zeros(p.shape[:-1], np.int32)
    for i in range(1, p.shape[-1]):
        better = best < p[..., i]
        best = np.where(better, p[..., i], best)
        act = np.where(better, i, act).astype(np.int32)
    return act


def replay(case, ticks=None, trace=None, packed=None):
    """The evaluation on the host: per tick the restated networks on the oracle's observation rows, the action (first
    maximum, or the number of running sums below the Philox uniform of (word, epoch0 + k), at most 4),
    TagGridWorldOracle.step, total = float32(total + float32(reward)) and steps += 1 under the live mask, up to each
    replica's first done or `ticks`.  With `trace` [>= ticks, E, 5] (the device's recorded actions) the replay FOLLOWS
    the device: a recorded action of a live replica must be the host's, or that decision's margin -- sampled: the
    smallest |running sum - u| over the four thresholds; greedy: the gap between the two largest probabilities -- must
    be below 2e-6.  Returns a dict: reward_sum [E, 5], steps, done, actions [ticks, E, 5] (-1 where the replica no
    longer ran), epochs [E, 5], margins (per live decision, in order), near (decisions inside the window), decisions,
    followed, end_tick [E] (-1: unfinished), tagged [E], timed_out [E], wall_hits, max_coord (the largest coordinate a
    live agent stood on after a move), counts (per action)."""
    E, T = case.E, case.T
    ticks = T if ticks is None else int(ticks)
    packed = case.policies()[1] if packed is None else packed
    orc = case.oracle()
    epoch0 = case.start_epochs()
    k0, k1 = seed_words(SAMPLER_SEED)
    live = np.ones(E, bool)
    total, steps, done = np.zeros((E, N), F32), np.zeros(E, np.int32), np.zeros(E, np.int32)
    actions = np.full((ticks, E, N), -1, np.int32)
    end_tick, tagged, timed_out = np.full(E, -1, np.int32), np.zeros(E, bool), np.zeros(E, bool)
    near = decisions = followed = wall_hits = max_coord = 0
    counts, margins = np.zeros(A, np.int64), []
    for k in range(ticks):
        if not live.any():
            break
        p = probabilities(packed, case.hidden, orc.obs.astype(F32))
        if case.greedy:
            host = first_maximum(p)
            top = np.sort(p.astype(np.float64), axis=-1)
            margin = top[..., -1] - top[..., -2]
        else:
            u = single_head_tick_uniform(E * N, epoch0.reshape(-1) + np.uint32(k), k0, k1, TICK_TAG).reshape(E, N)
            cum = running_sums(p.reshape(-1, A)).reshape(E, N, A)
            host = np.minimum((cum < u[..., None]).sum(axis=-1), A - 1).astype(np.int32)
            margin = np.abs(cum[..., :A - 1].astype(np.float64) - u[..., None].astype(np.float64)).min(axis=-1)
        a = host.copy()
        if trace is not None:
            got = np.asarray(trace[k], np.int32).reshape(E, N)
            assert ((got[live] >= 0) & (got[live] < A)).all(), (case.name, k)
            bad = live[:, None] & (got != host)
            assert (margin[bad] < NEAR_WINDOW).all(), (case.name, k, np.argwhere(bad)[:5], margin[bad].max())
            followed += int(bad.sum())
            a[live] = got[live]
        margins.append(margin[live].reshape(-1))
        near += int((margin[live] < NEAR_WINDOW).sum())
        decisions += int(live.sum()) * N
        counts += np.bincount(a[live].reshape(-1), minlength=A)
        actions[k, live] = a[live]
        x0, y0 = orc.loc_x.astype(np.int64), orc.loc_y.astype(np.int64)
        _, rew, d = orc.step(a)
        max_coord = max(max_coord, int(orc.loc_x[live].max()), int(orc.loc_y[live].max()))
        ux, uy = x0 + STEP_ACTIONS[a, 0], y0 + STEP_ACTIONS[a, 1]
        wall_hits += int((((ux != orc.loc_x) | (uy != orc.loc_y)) & live[:, None]).sum())
        total[live] = (total[live] + rew.astype(F32)[live]).astype(F32)
        steps[live] += 1
        fin = live & (d > 0)
        tag_now = fin & (rew[:, 0] > 5.0)   # the taggers' reward on a tag is tag_reward_for_tagger (- the wall penalty)
        done[fin] = 1
        end_tick[fin] = k
        tagged |= tag_now
        timed_out |= fin & ~tag_now
        live = live & ~fin
    epochs = epoch0 if case.greedy else (epoch0 + steps.astype(np.uint32)[:, None]).astype(np.uint32)
    return {"reward_sum": total, "steps": steps, "done": done, "actions": actions, "epochs": epochs,
            "margins": np.concatenate(margins) if margins else np.zeros(0), "near": near, "decisions": decisions,
            "followed": followed, "end_tick": end_tick, "tagged": tagged, "timed_out": timed_out,
            "wall_hits": wall_hits, "max_coord": max_coord, "counts": counts}


def vacuity(case, r):
    """the conditions a GPU case must meet on the host replay alone -> (ok, figures)"""
    fin = r["end_tick"] >= 0
    share = r["counts"] / max(1, r["counts"].sum())
    groups = [slice(g, min(g + EPB, case.E)) for g in range(0, case.E, EPB)]
    mixed = sum(1 for g in groups if len(np.unique(r["end_tick"][g][r["tagged"][g]])) >= 2 and r["timed_out"][g].any())
    fig = {"end ticks": len(np.unique(r["end_tick"][fin])), "mixed groups": mixed, "tags": int(r["tagged"].sum()),
           "time-outs": int(r["timed_out"].sum()), "wall hits": r["wall_hits"], "shares": np.round(share, 3).tolist(),
           "near": r["near"], "decisions": r["decisions"], "steps": (int(r["steps"].min()), int(r["steps"].max()))}
    ok = (fig["end ticks"] >= 8 and mixed >= 1 and fig["tags"] > 0 and fig["time-outs"] > 0 and fig["wall hits"] > 0
          and r["near"] <= case.near_cap(r["decisions"])
          and ((np.sort(share)[-3] >= 0.05) if case.greedy else (share.min() >= 0.02)))
    return bool(ok), fig


def reaches_bound(case, r):
    """the condition of the BOUND_CASES: live agents stand on coordinate 63 after a move (the image update reads the last
    entry of the quotient table), walk into walls, and the near-tie count stays under the cap"""
    return bool(case.L == 63 and r["max_coord"] == 63 and r["wall_hits"] > 0 and r["timed_out"].any()
                and r["near"] <= case.near_cap(r["decisions"]))


if __name__ == "__main__":   # the seed search: the first seed per (hidden, grid_length, mode) that meets `vacuity`
    for key in sorted(POLICY_SEED):
        H, L, mode = key
        case = GwCase(H, mode, L, dict(SIZES).get(L, 12))
        for seed in range(1, 200):
            r = replay(case, packed=case.policies(seed)[1])
            ok, fig = vacuity(case, r)
            if (ok or (L == 63 and reaches_bound(case, r))) and r["near"] == 0:
                print(f"{key}: {seed},   # {fig}")
                break
        else:
            print(key, "no seed below 200")
