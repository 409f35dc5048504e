"""The in-kernel policies of the in-tree rollout and evaluation entries on the MI355X, with no excused draw:
HipClassicControl<CartPole|Acrobot|MountainCar>EnvRollout_H<32|64> and ...Evaluate_H<32|64>, HipTagGridWorldRollout_N5_H<32|64>
and HipTagGridWorldEvaluate_N5_H<32|64>, and in reduced form ...CartPoleEnvRollout_P_H<32|64> and
HipTagGridWorldRollout_N5P_H<32|64>, under the crafted policies of tests/crafted_policies.py (uniform, constant, switched:
every probability exactly 0, 0.5, 1 or 1 / A) and the preset epochs of tests/inkernel_policy_exact_cases.py (rows that draw
u == 1.0 and u == 2^-24 on each word of a Philox block inside the launch, two rows across the 2^32 wrap).  Every recorded
action equals the host model's -- the project's restatements, unchanged -- at tolerance 0: no window around a threshold,
no cap, and the replay never follows the device.  Everything the entries' existing harnesses compare still holds (rows,
final arrays, RNG and pool words; one T-tick launch equals T one-tick launches).  The random policy appears once per
entry family, under the existing near-threshold rule, for the rows only the clamp min(cnt, A - 1) can decide: u == 1.0
over a float32 running sum that ends below 1.0.  tests/test_inkernel_policy_exact_host.py shows on the host that no case
passes vacuously.  `pytest -s` prints one line per entry and policy kind."""
import numpy as np
import pytest
import torch

from tests import classic_control_cases as cc
from tests import classic_control_evaluate as ev
from tests import crafted_policies as cp
from tests import gridworld_evaluate as gev
from tests import inkernel_policy_exact_cases as xc

pytestmark = pytest.mark.gpu

F32 = np.float32
N = xc.N
SHORT = 3   # ticks of the short launches the nine-tick TagGridWorld launch is compared with


def _sh():
    from tests import test_gpu_classic_control_shapes as shapes   # (its plumbing and the two yardsticks)

    return shapes


def _fill(t, arr):
    t.copy_(torch.from_numpy(np.ascontiguousarray(arr)).to(t.device))
    torch.cuda.synchronize()


def _hits(roles, ticks_run=None):
    """end rows per (word, end) that the run reached"""
    out = {}
    for r, (w, kind, t) in roles.items():
        if ticks_run is None or ticks_run(r, t):
            out[f"{kind}{w}"] = out.get(f"{kind}{w}", 0) + 1
    return dict(sorted(out.items()))


# ------------------------------------------------------------------------------------------- single-agent rollouts
class _SingleRollout:
    """one case on the device: the entry under test at `ticks_per_launch` = 9, the same entry at one tick per launch, and
    the yardstick (Cartpole: oracle/cartpole_np.py; else a third wrapper driven by the Step kernel + reset_when_done)"""

    def __init__(self, case):
        sh = _sh()
        self.case = case
        self.w, self.sampler, self.packed, _, _, self.batch, self.launch, self.start = sh._rollout_setup(case)
        one = xc.SingleCase(case.env, case.hidden, case.T, E=case.E, geom=case.geom)
        one.ticks = one.rows = 1
        self.one = one
        self.w1, self.sampler1, self.packed1, _, _, self.batch1, self.launch1, _ = sh._rollout_setup(one)
        state = self.start["state"]
        self.start["obs"] = xc.single_start_obs(case.env, state).reshape(case.E, 1, -1)
        fn, args, block, grid, shared = self.launch
        O, H, A = cc.OBS_DIM[case.env], case.hidden, case.A
        assert fn.name == cc.ENTRY[case.env] + f"Rollout_H{H}" and self.launch1[0].name == fn.name
        assert shared == 4 * (O * H + H + H * H + H + A * H + A) == 4 * len(case.packed)
        self.yard = None

    def rewind(self, packed_np, shift=0):
        sh, case = _sh(), self.case
        case.packed, case.shift, self.one.shift = packed_np, shift, shift
        _fill(self.packed, packed_np), _fill(self.packed1, packed_np)
        words0 = sh._tick_start(self.w, case, self.sampler, self.start)
        sh._tick_start(self.w1, self.one, self.sampler1, self.start)
        if case.env == "cartpole":
            self.yard = sh._CartpoleYardstick(case, self.start["state"], self.start["ts"], self.start["row"],
                                              self.start["obs"][:, 0])
        else:
            if self.yard is None:
                self.yard = sh._DeviceYardstick(case, self.start["state"], self.start["ts"])
                self.yard.obs0 = self.start["obs"].copy()
            self.yard.rewind()
        return words0

    def run(self, packed_np, tag, exact=True, shift=0):
        """the two launches from the rewound start -> {"draws", "differ", "near", "restarts", "cum" [K, E, A], "u", "actions"
        [K, E]}.  exact: every action is the model's; else the existing rule (a mismatch only where the uniform lies within
        NEAR_WINDOW of a threshold; the yardstick follows the device)"""
        from oracle.core_np import seed_words, single_head_tick_uniform
        from tests.classic_control_policy import count_below, running_sums
        from tests.hip_harness import ACT, OBS, REW, pull

        sh, case = _sh(), self.case
        E, A, T = case.E, case.A, case.ticks
        words0 = self.rewind(packed_np, shift)
        k0, k1 = seed_words(cc.SAMPLER_SEED)
        threads, blocks, _ = cc.geometry(E, case.geom)
        fn, args, block, grid, shared = self.launch
        fn1, args1, block1, grid1, shared1 = self.launch1
        out = {"draws": 0, "differ": 0, "near": 0, "restarts": 0, "cum": [], "u": [], "actions": []}
        for li in range(case.launches):
            sh._refill(self.batch)
            fn(*args, block=(threads, 1, 1), grid=(blocks, 1), shared=shared)
            sh._sync()
            b = {k: v.cpu().numpy() for k, v in self.batch.items()}
            acts = b["actions"][:T, :, 0, 0]
            assert acts.min() >= 0 and acts.max() <= A - 1, tag
            ep0 = words0[4:] + np.uint32(li * T)
            for k in range(T):
                sh._refill(self.batch1)
                fn1(*args1, block=(threads, 1, 1), grid=(blocks, 1), shared=shared1)   # the same tick as its own launch
                sh._sync()
                for key, v in self.batch1.items():
                    sh.EQ(v[0].cpu().numpy(), b[key][k], f"{tag} launch {li}: {key} row {k} of a one-tick launch")
                obs_k = self.yard.obs()
                cum = running_sums(cc.rollout_probabilities(case, packed_np, obs_k))
                u = single_head_tick_uniform(E, ep0 + np.uint32(k), k0, k1, cc.TICK_TAG)
                want = count_below(cum, u)
                bad = acts[k] != want
                if exact:
                    assert not bad.any(), (tag, li, k, np.flatnonzero(bad)[:5], cum[bad][:5], u[bad][:5], acts[k][bad][:5])
                else:
                    near_k = cc.near_threshold(cum, u)
                    assert not (bad & ~near_k).any(), (tag, li, k, cum[bad & ~near_k], u[bad & ~near_k])
                    out["near"] += int(near_k.sum())
                out["differ"] += int(bad.sum())
                out["draws"] += E
                out["cum"].append(cum), out["u"].append(u), out["actions"].append(acts[k].copy())
                sh.EQ(b["obs"][k, :, 0], obs_k, f"{tag} launch {li} obs row {k}")
                done_k, rew_k = self.yard.step(acts[k])
                sh.EQ(b["rewards"][k, :, 0], rew_k, f"{tag} launch {li} reward row {k}")
                sh.EQ(b["done"][k], done_k, f"{tag} launch {li} done row {k}")
                out["restarts"] += int((done_k > 0).sum())
                self.yard.restart()
            fin = self.yard.final()
            for w, sampler in ((self.w, self.sampler), (self.w1, self.sampler1)):
                got = {n: pull(w, n) for n in ("state", OBS, "_timestep_", "_done_", REW, ACT)}
                sh.EQ(got["state"][:, 0], fin["state"], f"{tag} launch {li} state")
                sh.EQ(got[OBS][:, 0], fin["obs"], f"{tag} launch {li} observation")
                sh.EQ(got["_timestep_"], fin["ts"], f"{tag} launch {li} timestep")
                sh.EQ(got["_done_"], done_k, f"{tag} launch {li} done")
                sh.EQ(got[REW][:, 0], rew_k, f"{tag} launch {li} reward")
                sh.EQ(got[ACT].reshape(-1), acts[-1], f"{tag} launch {li} sampled_actions")
                rng = sh._words(sampler.rng_state, E)
                sh.EQ(rng[:4], words0[:4], f"{tag} launch {li} RNG header")
                sh.EQ(rng[4:], words0[4:] + np.uint32((li + 1) * T), f"{tag} launch {li} RNG epochs")
                if case.pool:
                    sh.EQ(sh._words(w.env_resetter._pool_rng, E), fin["pool_words"], f"{tag} launch {li} pool RNG words")
        for key in ("cum", "u", "actions"):
            out[key] = np.stack(out[key])
        return out


@pytest.mark.parametrize("which", range(4), ids=["T7", "T13", "E1", "idle"])
@pytest.mark.parametrize("hidden", xc.WIDTHS)
@pytest.mark.parametrize("env", xc.SINGLE)
def test_single_agent_rollouts_excuse_no_draw(env, hidden, which):
    """...EnvRollout_H<hidden> at E = 130 with episodes of 7 and of 13 ticks, at E = 1, and under the geometry with two
    idle blocks: two launches of nine ticks from spread states under every crafted kind.  Every recorded action is the
    count of the restatement's running sums below the host's uniform, at tolerance 0; the observation, reward and done
    rows, the final state, observation, time step, RNG words and pool words; nine one-tick launches record the same rows
    and leave the same arrays.  The row that draws u == 1.0 takes the FIRST action whose sum is 1.0, the row that draws
    u == 2^-24 skips a leading action of probability 0."""
    case = xc.single_cases(env, hidden)[which]
    dev = _SingleRollout(case)
    roles = case.preset()[1]
    for kind, packed in cp.kinds(env, hidden).items():
        tag = f"{case.name} {kind}"
        r = dev.run(packed, tag)
        for row, w, t in xc.end_rows(roles, "hi"):
            assert r["u"][t, row] == 1.0 and r["actions"][t, row] == int(np.argmax(r["cum"][t, row] == 1.0)), (tag, row)
        for row, w, t in xc.end_rows(roles, "lo"):
            assert r["u"][t, row] == F32(2.0 ** -24) and r["actions"][t, row] == int(np.argmax(r["cum"][t, row] > 0)), (tag, row)
        assert r["differ"] == 0 and r["draws"] == case.E * xc.TOTAL and r["restarts"] >= case.E
        print(f"{tag} [{dev.launch[0].name}]: {r['draws']} draws, {r['differ']} mismatches, {r['restarts']} restarts, "
              f"end rows hit {_hits(roles)}")


@pytest.mark.parametrize("hidden", xc.WIDTHS)
@pytest.mark.parametrize("env", xc.SINGLE)
def test_single_agent_rollouts_clamp_a_draw_of_one(env, hidden):
    """the random policy (FullyConnected under CLAMP_SEED, the head times HEAD_SCALE) under six presets and both episode
    lengths, by the rule of tests/test_gpu_classic_control_shapes.py (a mismatch only within NEAR_WINDOW of a threshold,
    the yardstick follows the device, the count under the case's cap).  On the rows that draw u == 1.0 while the model's
    last running sum is below 1.0 and the one before it below 1 - 1e-3 the action is A - 1, exactly: only the clamp gives
    it (Cartpole: the clamp of the two-compare path).  At least 8 such rows."""
    rows = near = draws = 0
    for T in xc.LENGTHS:
        case = xc.SingleCase(env, hidden, T)
        dev = _SingleRollout(case)
        packed = case.random_policy(xc.CLAMP_SEED[env, hidden])
        for shift in xc.CLAMP_SHIFTS:
            r = dev.run(packed, f"{case.name} random shift {shift}", exact=False, shift=shift)
            clamp = xc.clamp_rows(r["cum"], r["u"], case.A, case.preset()[1])
            for t, row in clamp:
                assert r["actions"][t, row] == case.A - 1, (case.name, shift, t, row, r["cum"][t, row])
            rows, near, draws = rows + len(clamp), near + r["near"], draws + r["draws"]
            assert r["near"] <= case.near_cap()
    print(f"{env} H{hidden} random policy: {rows} clamp rows all at action A - 1, {near} of {draws} draws within "
          f"{cc.NEAR_WINDOW} of a threshold")
    assert rows >= xc.CLAMP_ROWS


# ----------------------------------------------------------------------------------------- single-agent evaluations
def _check_evaluation(got, r, words0, E, surplus, sent_f, sent_i, tag, greedy):
    sh = _sh()
    for key in ("reward_sum", "steps", "done"):
        sh.EQ(got[key][:E], r[key], (tag, key))
        sent = sent_f if key == "reward_sum" else sent_i
        assert (got[key][E:] == sent).all() and len(got[key]) == E + surplus, (tag, key)
    want = np.full(got["trace"].shape, sent_i, np.int32)
    want[: len(r["actions"])] = np.where(r["actions"] >= 0, r["actions"], sent_i)
    sh.EQ(got["trace"], want, (tag, "trace"))
    words = words0.copy()
    words[4:] = np.asarray(r["epochs"]).reshape(-1)
    sh.EQ(got["words"], words, (tag, "rng words"))
    if greedy:
        sh.EQ(got["words"], words0, (tag, "a greedy evaluation leaves the RNG words alone"))


@pytest.mark.parametrize("mode", ev.MODES)
@pytest.mark.parametrize("hidden", xc.WIDTHS)
@pytest.mark.parametrize("env", xc.SINGLE)
def test_single_agent_evaluations_excuse_no_decision(env, hidden, mode):
    """...EnvEvaluate_H<hidden>, greedy and sampled, episodes of 7 and of 13 ticks at E = 130 under every crafted kind:
    reward sums, step counts, done flags, the action trace and the RNG words equal the replay of
    tests/classic_control_evaluate.py, which is NOT given the device's trace (it follows nothing; `near_top_two` and
    `near_threshold` decide nothing).  Greedy: uniform gives action 0 on every tick, two tied winners the lower index.
    Sampled: the preset epochs; the epoch words advance by the steps taken.  The idle-block geometry gives the same bytes."""
    from tests.test_gpu_evaluate import _Launch, _device_step

    A = cp.LAYOUT[env][2]
    for T in xc.LENGTHS:
        case = xc.SingleEvalCase(env, hidden, mode, T)
        L = _Launch(case)
        roles = case.preset()[1]
        for kind, packed in cp.kinds(env, hidden).items():
            tag = f"{case.name} {kind}"
            case.packed = L.packed_np = packed
            _fill(L.packed, packed)
            got = L.run("product")
            r = ev.replay(case, ticks=L.ticks, step=_device_step(case), trace=None, packed=packed)
            _check_evaluation(got, r, L.words0, case.E, ev.SURPLUS, ev.SENTINEL_F, ev.SENTINEL_I, tag, case.greedy)
            live = r["actions"] >= 0
            if case.greedy and kind == "uniform":
                assert (got["trace"][:T][live] == 0).all(), tag
            if case.greedy and kind == "tied":
                assert (got["trace"][:T][live] == A - 2).all(), tag
            if case.greedy and kind in ("towards", "away", "switched"):
                assert got["trace"][0, xc.TIE_ROW] == min(cp.FORMS[env][1]), tag
            other = L.run((64, "idle"))
            for key in got:
                assert other[key].tobytes() == got[key].tobytes(), (tag, key)
            reached = _hits(roles, lambda row, t: r["actions"][t, row] >= 0)
            print(f"{tag} [{L.fn.name}]: {r['decisions']} decisions, 0 mismatches, terminations on {len(r['end_ticks'])} "
                  f"ticks, {r['timeouts']} time-outs" + ("" if case.greedy else f", end rows reached {reached}"))


# --------------------------------------------------------------------------------------------------- TagGridWorld
class _GridRollout:
    """HipTagGridWorldRollout_N5_H<hidden> at nine ticks and at three ticks per launch (the live-policy entry takes no
    one-tick launch), from GridCase's start"""

    def __init__(self, case):
        from tests.hip_harness import make_wrapper, require_gpu
        from warp_drive_amd.envs.tag_gridworld import CUDATagGridWorld
        from warp_drive_amd.managers.function_manager import HIPSampler

        require_gpu()
        self.case, E = case, case.E
        self.sides = []
        for ticks in (xc.TICKS, SHORT):
            w = make_wrapper(CUDATagGridWorld(seed=27, **case.env_config()), E)
            w.env.ticks_per_launch = ticks
            sampler = HIPSampler(w.cuda_function_manager)
            sampler.init_random(seed=gev.SAMPLER_SEED)
            packed = [torch.from_numpy(p.copy()).cuda() for p in case.packed]
            probs = torch.full((E, N, 5), 0.2, device="cuda")   # (not read: the kernel evaluates the policies)
            batch = {"obs": torch.full((ticks, E, N, gev.F), 7.0, device="cuda"),
                     "actions": torch.full((ticks, E, N, 1), -1, dtype=torch.int32, device="cuda"),
                     "rewards": torch.full((ticks, E, N), -7.0, device="cuda"),
                     "done": torch.full((ticks, E), -1, dtype=torch.int32, device="cuda")}
            assert w.env.has_live_policy_rollout(case.hidden, 5)
            launch = w.env.tick_launch(sampler, [probs], w.env_resetter, batch=batch, policy=(packed, case.hidden))
            assert launch[0].name == f"HipTagGridWorldRollout_N5_H{case.hidden}" and launch[2] == (64, 1, 1)
            self.sides.append(dict(w=w, sampler=sampler, packed=packed, probs=probs, batch=batch, launch=launch))

    def rewind(self, packed_np, shift):
        from tests.hip_harness import OBS
        from tests.test_gpu_gridworld_evaluate import _put, _put_words, _words

        case = self.case
        case.packed, case.shift = packed_np, shift
        orc = case.oracle()
        for side in self.sides:
            w = side["w"]
            for t, p in zip(side["packed"], packed_np):
                _fill(t, p)
            _put(w, "loc_x", orc.loc_x), _put(w, "loc_y", orc.loc_y), _put(w, "_timestep_", orc.timestep)
            _put(w, "_done_", np.zeros(case.E, np.int32)), _put(w, OBS, orc.obs.astype(F32))
            side["sampler"].init_random(seed=gev.SAMPLER_SEED)
            words0 = _words(side["sampler"].rng_state, case.E * N)
            assert (words0[:2] == np.array(gev.seed_words(gev.SAMPLER_SEED), np.uint32)).all() and (words0[4:] == 0).all()
            words0[4:] = case.start_epochs().reshape(-1)
            _put_words(side["sampler"].rng_state, words0)
        return orc, words0

    def run(self, packed_np, tag, exact=True, shift=0):
        from oracle.core_np import single_head_tick_uniform
        from oracle.tag_gridworld_np import running_sums
        from tests.hip_harness import OBS, pull
        from tests.test_gpu_gridworld_evaluate import EQ, _words

        case, E, T = self.case, self.case.E, xc.TICKS
        orc, words0 = self.rewind(packed_np, shift)
        main, short = self.sides
        out = {"draws": 0, "differ": 0, "near": 0, "restarts": 0, "tags": 0, "cum": [], "u": [], "actions": []}
        for li in range(xc.LAUNCHES):
            for side in self.sides[:1]:
                for key, t in side["batch"].items():
                    t.fill_(-1 if t.dtype == torch.int32 else 7.0)
            fn, args, block, grid, shared = main["launch"]
            fn(*args, block=block, grid=grid, shared=shared)
            torch.cuda.synchronize()
            b = {k: v.cpu().numpy() for k, v in main["batch"].items()}
            for j in range(T // SHORT):
                fn1, args1, block1, grid1, shared1 = short["launch"]
                fn1(*args1, block=block1, grid=grid1, shared=shared1)   # the same ticks as three launches of three
                torch.cuda.synchronize()
                for key, v in short["batch"].items():
                    EQ(v.cpu().numpy(), b[key][SHORT * j:SHORT * (j + 1)], f"{tag} launch {li}: {key} rows of short launch {j}")
            for k in range(T):
                obs = orc.obs.astype(F32)
                EQ(b["obs"][k], obs, f"{tag} launch {li} obs row {k}")
                cum = running_sums(gev.probabilities(packed_np, case.hidden, obs).reshape(-1, 5)).reshape(E, N, 5)
                u = single_head_tick_uniform(E * N, words0[4:] + np.uint32(li * T + k), words0[0], words0[1],
                                             gev.TICK_TAG).reshape(E, N)
                want = np.minimum((cum < u[..., None]).sum(axis=-1), 4).astype(np.int32)
                got = b["actions"][k, :, :, 0]
                assert got.min() >= 0 and got.max() <= 4, tag
                bad = got != want
                if exact:
                    assert not bad.any(), (tag, li, k, np.argwhere(bad)[:5], cum[bad][:5], u[bad][:5], got[bad][:5])
                elif bad.any():
                    gap = np.abs(cum[bad] - u[bad][:, None]).min(axis=1)
                    assert (gap < gev.NEAR_WINDOW).all(), (tag, li, k, gap.max())
                out["differ"] += int(bad.sum())
                out["near"] += int(bad.sum())
                out["draws"] += E * N
                out["cum"].append(cum.reshape(E * N, 5)), out["u"].append(u.reshape(-1))
                out["actions"].append(got.reshape(-1).copy())
                _, rew, done = orc.step(got)
                EQ(b["rewards"][k], orc.rewards.astype(F32), f"{tag} launch {li} reward row {k}")
                EQ(b["done"][k], orc.done, f"{tag} launch {li} done row {k}")
                out["restarts"] += int((done > 0).sum())
                out["tags"] += int(((done > 0) & (rew[:, 0] > 5.0)).sum())
                last_done = orc.done.copy()
                orc.reset_done_envs()
            for side in self.sides:
                w = side["w"]
                EQ(pull(w, "loc_x"), orc.loc_x, f"{tag} launch {li} loc_x")
                EQ(pull(w, "loc_y"), orc.loc_y, f"{tag} launch {li} loc_y")
                EQ(pull(w, "_timestep_"), orc.timestep, f"{tag} launch {li} timestep")
                EQ(pull(w, "_done_"), last_done, f"{tag} launch {li} done")
                EQ(pull(w, OBS), orc.obs.astype(F32), f"{tag} launch {li} observations")
                words = _words(side["sampler"].rng_state, E * N)
                EQ(words[:4], words0[:4], f"{tag} launch {li} RNG header")
                EQ(words[4:], words0[4:] + np.uint32((li + 1) * T), f"{tag} launch {li} RNG epochs")
        for key in ("cum", "u", "actions"):
            out[key] = np.stack(out[key])
        return out


@pytest.mark.parametrize("T", xc.LENGTHS)
@pytest.mark.parametrize("hidden", xc.WIDTHS)
def test_gridworld_rollouts_excuse_no_draw(hidden, T):
    """HipTagGridWorldRollout_N5_H<hidden> at E = 25 (two full groups of 12 replicas and a group of one) on a grid of side
    11: two launches of nine ticks under every crafted kind, the tagger's policy on rows env * 5 + 0 .. 3 and the runner's
    on row env * 5 + 4.  Every action at tolerance 0; the observation, reward and done rows; positions, time steps,
    observations and RNG words after every launch; three launches of three ticks the same (the entry takes no one-tick
    launch)."""
    case = xc.GridCase(hidden, "sampled", T)
    dev = _GridRollout(case)
    roles = case.preset()[1]
    for kind, packed in cp.kinds("gridworld", hidden).items():
        tag = f"{case.name} {kind}"
        r = dev.run(packed, tag)
        for row, w, t in xc.end_rows(roles, "hi"):
            assert r["u"][t, row] == 1.0 and r["actions"][t, row] == int(np.argmax(r["cum"][t, row] == 1.0)), (tag, row)
        for row, w, t in xc.end_rows(roles, "lo"):
            assert r["u"][t, row] == F32(2.0 ** -24) and r["actions"][t, row] == int(np.argmax(r["cum"][t, row] > 0)), (tag, row)
        assert r["differ"] == 0 and r["draws"] == case.E * N * xc.TOTAL and r["restarts"] >= case.E
        assert kind != "switched" or r["tags"] > 0
        print(f"{tag} [{dev.sides[0]['launch'][0].name}]: {r['draws']} draws, {r['differ']} mismatches, {r['restarts']} "
              f"restarts ({r['tags']} tags), end rows hit {_hits(roles)}")


@pytest.mark.parametrize("hidden", xc.WIDTHS)
def test_gridworld_rollouts_clamp_a_draw_of_one(hidden):
    """two random policies (tests/gridworld_evaluate.py's, under CLAMP_SEED) under six presets and both episode lengths, by
    the existing rule (a mismatch only within 2e-6 of a threshold, the oracle follows the device, at most
    2 + draws // 50000 of them).  On the rows that draw u == 1.0 over a model sum that ends below 1.0 (the fourth sum
    below 1 - 1e-3) the action is 4, exactly.  At least 8 such rows."""
    rows = near = draws = 0
    for T in xc.LENGTHS:
        case = xc.GridCase(hidden, "sampled", T)
        dev = _GridRollout(case)
        packed = gev.GwCase.policies(case, xc.CLAMP_SEED["gridworld", hidden])[1]
        for shift in xc.CLAMP_SHIFTS:
            r = dev.run(packed, f"{case.name} random shift {shift}", exact=False, shift=shift)
            clamp = xc.clamp_rows(r["cum"], r["u"], 5, case.preset()[1])
            for t, row in clamp:
                assert r["actions"][t, row] == 4, (case.name, shift, t, row, r["cum"][t, row])
            rows, near, draws = rows + len(clamp), near + r["near"], draws + r["draws"]
    print(f"gridworld H{hidden} random policies: {rows} clamp rows all at action 4, {near} of {draws} draws decided "
          f"otherwise within {gev.NEAR_WINDOW} of a threshold")
    assert rows >= xc.CLAMP_ROWS and near <= 2 + draws // 50000


@pytest.mark.parametrize("mode", gev.MODES)
@pytest.mark.parametrize("hidden", xc.WIDTHS)
def test_gridworld_evaluations_excuse_no_decision(hidden, mode):
    """HipTagGridWorldEvaluate_N5_H<hidden>, greedy and sampled, episodes of 7 and of 13 ticks at E = 25 under every crafted
    kind: reward sums, step counts, done flags, the action trace and the RNG words equal the replay of
    tests/gridworld_evaluate.py, which is NOT given the device's trace.  Greedy: uniform gives action 0 on every tick, two
    tied winners the lower index (1 for the taggers, 2 for the runner)."""
    from tests.test_gpu_gridworld_evaluate import _Launch

    for T in xc.LENGTHS:
        case = xc.GridCase(hidden, mode, T, span=xc.EVAL_SPAN)
        L = _Launch(case)
        roles = case.preset()[1]
        for kind, packed in cp.kinds("gridworld", hidden).items():
            tag = f"{case.name} {kind}"
            case.packed = L.packed_np = packed
            for t, p in zip(L.packed, packed):
                _fill(t, p)
            got = L.run("product")
            r = gev.replay(case, ticks=L.ticks, trace=None, packed=packed)
            _check_evaluation(got, r, L.words0, case.E, gev.SURPLUS, gev.SENTINEL_F, gev.SENTINEL_I, tag, case.greedy)
            live = r["actions"][:, :, 0] >= 0
            if case.greedy and kind == "uniform":
                assert (got["trace"][:T][live] == 0).all(), tag
            if case.greedy and kind == "tied":
                assert (got["trace"][:T, :, :4][live] == 1).all() and (got["trace"][:T, :, 4][live] == 2).all(), tag
            other = L.run("idle")
            for key in got:
                assert other[key].tobytes() == got[key].tobytes(), (tag, key)
            reached = _hits(roles, lambda row, t: r["actions"][t, row // N, row % N] >= 0)
            print(f"{tag} [{L.fn.name}]: {r['decisions']} decisions, 0 mismatches, {int(r['tagged'].sum())} tags, "
                  f"{int(r['timed_out'].sum())} time-outs" + ("" if case.greedy else f", end rows reached {reached}"))


# ----------------------------------------------------------------------------------------- the pooled entries, reduced
@pytest.mark.parametrize("hidden", xc.WIDTHS)
def test_pooled_cartpole_rollout_excuses_no_draw(hidden):
    """HipClassicControlCartPoleEnvRollout_P_H<hidden> at E = 130, T = 7 under the uniform policy and one switched policy:
    everything tests/test_gpu_cartpole_pool_rollout.py compares against tests/cartpole_pool_cases.py::PoolModel, with the
    model's own actions (the counting draw on the restatement) in place of the device's"""
    from tests import cartpole_pool_cases as cpool
    from tests import test_gpu_cartpole_pool_rollout as pooled
    from tests.hip_harness import ACT, OBS, REW

    sh = _sh()
    case = xc.CartpolePoolCase(hidden)
    dev = pooled._device(case)
    fn, args, block, grid, shared = dev["launch"]
    assert fn.name == cpool.ENTRY[hidden]
    kinds = cp.kinds("cartpole", hidden)
    T, E = case.ticks, case.E
    for kind in ("uniform", "towards"):
        tag = f"{case.name} {kind}"
        case.packed = kinds[kind]
        _fill(dev["packed"], kinds[kind])
        words0 = sh._tick_start(dev["w"], case, dev["sampler"], dev["start"])
        model = cpool.PoolModel(case)
        for li in range(case.launches):
            for key, fill in (("obs", 7.0), ("actions", -1), ("rewards", 7.0), ("done", -1)):
                dev["batch"][key].fill_(fill)
            fn(*args, block=block, grid=grid, shared=shared)
            sh._sync()
            snap = pooled._snapshot(dev, case)
            rows = model.launch(cpool.HostChoice(case, packed=kinds[kind]))   # the host's own action: nothing followed
            sh.EQ(snap["batch_actions"][:T, :, 0, 0], rows["actions"], f"{tag} launch {li} action rows")
            sh.EQ(snap["batch_obs"][:T, :, 0], rows["obs"], f"{tag} launch {li} obs rows")
            sh.EQ(snap["batch_rewards"][:T, :, 0], rows["rewards"], f"{tag} launch {li} reward rows")
            sh.EQ(snap["batch_done"][:T], rows["done"], f"{tag} launch {li} done rows")
            assert (snap["batch_obs"][T:] == 7.0).all() and (snap["batch_actions"][T:] == -1).all(), tag
            st = model.state()
            sh.EQ(snap["state"][:, 0], st["state"], f"{tag} launch {li} state")
            sh.EQ(snap[OBS][:, 0], st["obs"], f"{tag} launch {li} observation")
            sh.EQ(snap["_timestep_"], st["timestep"], f"{tag} launch {li} timestep")
            sh.EQ(snap["_done_"], st["done"], f"{tag} launch {li} done")
            sh.EQ(snap[REW][:, 0], st["rewards"], f"{tag} launch {li} reward")
            sh.EQ(snap[ACT].reshape(-1), st["actions"], f"{tag} launch {li} sampled_actions")
            sh.EQ(snap["rng"][:4], words0[:4], f"{tag} launch {li} RNG header")
            sh.EQ(snap["rng"][4:], st["epochs"], f"{tag} launch {li} RNG epochs")
            sh.EQ(snap["pool_rng"][4:], st["pool_epochs"], f"{tag} launch {li} pool epochs")
        restarts = int(model.restarts.sum())
        assert restarts >= E and (kind == "uniform" or (model.actions > 0).all())
        print(f"{tag} [{fn.name}]: {E * xc.TOTAL} draws, 0 mismatches, {restarts} restarts ({model.terminal} terminal), pool "
              f"rows {sorted(model.rows_drawn)}")


@pytest.mark.parametrize("hidden", xc.WIDTHS)
def test_pooled_gridworld_rollout_excuses_no_draw(hidden):
    """HipTagGridWorldRollout_N5P_H<hidden> at E = 25, T = 7 under the uniform policies and the switched ones: everything
    tests/test_gpu_gridworld_pool_rollout.py compares against tests/gridworld_pool_cases.py::PoolModel, with the model's
    own actions in place of the device's"""
    from tests import gridworld_pool_cases as gpool
    from tests import test_gpu_gridworld_pool_rollout as pooled

    case = xc.GridPoolCase(hidden)
    start = case.start_oracle()
    dev = pooled._Device(case.env(), case.E, start, case.start_epochs(), case.start_pool_epochs())
    env, E, T = dev.w.env, case.E, case.ticks
    env.ticks_per_launch = T
    kinds = cp.kinds("gridworld", hidden)
    packed = [torch.from_numpy(p.copy()).cuda() for p in kinds["uniform"]]
    probs = torch.full((E, N, 5), 0.2, device="cuda")
    batch = pooled._batch(T, E)
    assert env.has_live_policy_rollout(hidden, 5)
    fn, args, block, grid, shared = env.tick_launch(dev.sampler, [probs], dev.w.env_resetter, batch=batch,
                                                    policy=(packed, hidden))
    assert fn.name == f"HipTagGridWorldRollout_N5P_H{hidden}" and block == (64, 1, 1) and grid == (-(-E // gpool.EPB), 1)
    for kind in ("uniform", "switched"):
        tag = f"{case.name} {kind}"
        for t, p in zip(packed, kinds[kind]):
            _fill(t, p)
        dev.rewind()
        model = gpool.PoolModel(case, dev.pool_x, dev.pool_y)
        model.orc.loc_x, model.orc.loc_y = start.loc_x.copy(), start.loc_y.copy()
        model.orc.timestep, model.orc.obs = start.timestep.copy(), start.obs.copy()
        for li in range(case.launches):
            pooled._refill(batch)
            fn(*args, block=block, grid=grid, shared=shared)
            torch.cuda.synchronize()
            rows = model.launch(T, choose=xc.grid_exact_choice(kinds[kind], hidden))
            pooled._check_rows({k: v.cpu().numpy() for k, v in batch.items()}, rows, T, (tag, li))
            pooled._check_state(dev, model.state(), (tag, li))
        restarts = int(model.restarts.sum())
        assert restarts >= E and (kind == "uniform" or model.tags > 0)
        print(f"{tag} [{fn.name}]: {E * N * xc.TOTAL} draws, 0 mismatches, {restarts} restarts ({model.tags} tags), pool rows "
              f"{len(model.rows_drawn)} of {case.n_pool}")
