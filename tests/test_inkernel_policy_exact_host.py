"""On the host alone: no case of tests/test_gpu_inkernel_policy_exact.py can pass vacuously, and each defect planted in the
MODEL is caught wherever it applies.  The builders of tests/crafted_policies.py pack the bytes the project's packers
pack; the defect-free model of tests/inkernel_policy_exact_cases.py is the project's restatements bit for bit; every
modelled probability of a crafted policy is one of the exact values its kind allows; the switched policies reach both
actions and both kinds of episode end; the tie row is a tie; the end rows exist on all four words; the plateau row would
pick another action under `<=`; the clamp rows are at least 8; the wrap happens."""
import numpy as np
import pytest

from tests import classic_control_evaluate as ev
from tests import crafted_policies as cp
from tests import gridworld_evaluate as gev
from tests import inkernel_policy_exact_cases as xc

F32 = np.float32
ENVS = xc.SINGLE + ("gridworld",)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _parts_of_every_kind(env, H):
    out = {"uniform": cp.uniform(env, H)}
    for name, winners in cp.constant_kinds(env).items():
        out[name] = cp.constant(env, H, winners)
    for form in (("tagger", "runner") if env == "gridworld" else (env,)):
        for sign in (1, -1):
            out[f"{form}{sign:+d}"] = cp.switched(form, env, H, sign)
    rng = np.random.RandomState(3)
    out["random"] = {k: rng.standard_normal(v.shape).astype(F32) for k, v in cp.blank(env, H).items()}
    return out


# ------------------------------------------------------------------------------------------------------- the builders
@pytest.mark.parametrize("H", cp.WIDTHS)
@pytest.mark.parametrize("env", ENVS)
def test_builders_pack_the_bytes_of_the_projects_packers(env, H):
    """the same weights as a FullyConnected model through pack_rollout_policy (I = 4, 2, 6) / pack_gridworld_policy (21
    inputs at stride 24, the block padded to four floats): byte for byte; `unpack` inverts `pack`; the placements are the
    awkward ones"""
    I, stride, A = cp.LAYOUT[env]
    for name, parts in _parts_of_every_kind(env, H).items():
        mine = cp.pack(env, parts)
        assert mine.dtype == F32 and mine.tobytes() == cp.packed_by_the_project(env, parts).tobytes(), (env, H, name)
        back = cp.unpack(env, mine, H)
        assert all(back[k].tobytes() == np.asarray(parts[k], F32).tobytes() for k in parts), name
    if env == "gridworld":
        from warp_drive_amd.envs.tag_gridworld import gridworld_policy_floats

        assert len(cp.pack(env, cp.uniform(env, H))) == gridworld_policy_floats(H) and stride == 24 and I == 21
    u = cp.units(H)
    assert u["pos"] == H - 1 and u["neg"] >= H // 2 and u["neg2"] == H - 1 and u["pos2"] != u["pos"] and u["neg2"] != u["neg"]
    for form in (("tagger", "runner") if env == "gridworld" else (env,)):
        p = cp.switched(form, env, H)
        cols = sorted(cp.FORMS[form][0])
        assert np.flatnonzero(p["W0"][u["pos"]]).tolist() == cols and np.flatnonzero(p["W0"][u["neg"]]).tolist() == cols
        assert (p["W0"][u["pos"]] == -p["W0"][u["neg"]]).all()
    # the last column of a W0 row: column 3 of the float4, the odd column of a float2 row, column 20 behind five float4s
    assert 3 in cp.FORMS["cartpole"][0] and 1 in cp.FORMS["mountain_car"][0] and 20 in cp.FORMS["runner"][0]
    for name, winners in cp.constant_kinds(env).items():
        p = cp.constant(env, H, winners)
        assert not p["W0"].any() and (p["b0"] < 0).all() and np.flatnonzero(p["b1"]).tolist() == [H - 1]
    kinds = cp.constant_kinds(env)
    assert (0,) in kinds.values() and (A - 1,) in kinds.values()
    if A >= 3:
        assert 0 not in kinds["tied"] and len(kinds["tied"]) == 2


@pytest.mark.parametrize("H", cp.WIDTHS)
@pytest.mark.parametrize("env", ENVS)
def test_the_model_without_a_defect_is_the_projects_restatement(env, H):
    """`probabilities`, `running_sums`, `pick` and `greedy` against oracle/cartpole_np.py, tests/classic_control_policy.py,
    oracle/tag_gridworld_np.py and tests/classic_control_evaluate.py::first_maximum: bit for bit on a random policy and
    on every crafted kind, on signed rows, a zero row and a row of -0.0"""
    from oracle.cartpole_np import policy_probabilities as cartpole_probabilities
    from oracle.tag_gridworld_np import policy_probabilities as grid_probabilities
    from tests import classic_control_policy as ccp

    I, _, A = cp.LAYOUT[env]
    rng = np.random.RandomState(5)
    obs = np.concatenate([rng.standard_normal((40, I)), rng.uniform(0, 1, (28, I)), np.zeros((1, I)),
                          np.full((1, I), -0.0)]).astype(F32)
    u = rng.uniform(0, 1, len(obs)).astype(F32)
    for name, parts in _parts_of_every_kind(env, H).items():
        packed = cp.pack(env, parts)
        mine = xc.probabilities(env, packed, H, obs)
        if env == "gridworld":
            theirs = [grid_probabilities(packed, H, obs)]
        else:
            theirs = [ccp.policy_probabilities(packed, H, obs, A)]
            if env == "cartpole":
                theirs.append(cartpole_probabilities(packed, H, obs, A))
        for t in theirs:
            assert (_bits(mine) == _bits(t)).all(), (env, H, name)
        cum = xc.running_sums(mine)
        assert (_bits(cum) == _bits(ccp.running_sums(mine))).all()
        assert (xc.pick(cum, u) == ccp.count_below(cum, u)).all()
        assert (xc.greedy(mine) == ev.first_maximum(mine)).all() and (xc.greedy(mine) == gev.first_maximum(mine)).all()


def test_m_tied_winners_sum_to_exactly_one():
    """why a crafted policy cannot reach the clamp: m terms of 1 / m sum to exactly 1.0 in float32 for m = 1 .. 8"""
    for m in range(1, 9):
        p = np.full((1, m), F32(1.0) / F32(m), F32)
        assert float(xc.running_sums(p)[0, -1]) == 1.0, m


# ------------------------------------------------------------------------------------------- the epochs and the ends
@pytest.mark.parametrize("n_rows", [xc.E_SINGLE, xc.E_GRID * xc.N])
def test_end_rows_exist_on_all_four_words_and_the_wrap_happens(n_rows):
    for span, shifts in ((xc.TOTAL, xc.CLAMP_SHIFTS), (xc.EVAL_SPAN, (0,))):
        for shift in shifts:
            epochs, roles, wrap = xc.preset_epochs(n_rows, span, shift)
            assert {(w, k) for w, k, _ in roles.values()} == {(w, k) for w in range(4) for k in ("hi", "lo")}
            assert len(xc.end_rows(roles, "hi")) >= 8 and len(xc.end_rows(roles, "lo")) >= 4
            for r, (w, kind, tick) in roles.items():
                assert 0 <= tick < span and (int(epochs[r]) + tick) & 3 == w
                u = xc.uniforms(epochs, tick)[r]
                assert float(u) == (1.0 if kind == "hi" else 2.0 ** -24), (r, w, kind, tick, u)
            assert any(int(epochs[r]) & 3 for r in roles), "no end row starts inside a Philox quad"
            assert len(wrap) == 2 and not set(wrap) & set(roles) and xc.TIE_ROW not in wrap and xc.TIE_ROW not in roles
            assert [int(epochs[r]) for r in wrap] == [0xFFFFFFFF, 0xFFFFFFFE]
            rest = [r for r in range(n_rows) if r not in roles and r not in wrap]
            assert len({int(epochs[r]) & 3 for r in rest}) == 4 and len({int(epochs[r]) for r in rest}) == len(rest)
    ticks = {t for _, _, t in xc.preset_epochs(n_rows)[1].values()}
    assert {0, xc.TICKS - 1, xc.TOTAL - 1} <= ticks and any(t < xc.TICKS for t in ticks) and any(t >= xc.TICKS for t in ticks)
    assert xc.preset_epochs(1)[0].tolist() == [0xFFFFFFFF] and not xc.preset_epochs(1)[1]


# ------------------------------------------------------------------------------------------------ what the rows show
def _check_end_rows(kind, probs, cum, actions, u, roles, A, tag):
    """probs / cum [K, rows, A], actions / u [K, rows] of one crafted kind -> (plateau rows, leading-zero rows)"""
    plateau = zero = 0
    for r, w, t in xc.end_rows(roles, "hi"):
        first_one = int(np.argmax(cum[t, r] == 1.0))
        assert cum[t, r, -1] == 1.0 and actions[t, r] == first_one, tag     # a crafted policy never reaches the clamp
        if first_one < A - 1:       # the sum reaches 1.0 before the last action: `<=` would pick a later one
            le = xc.pick(cum[t, r][None], u[t, r][None], "le")[0]
            assert le > first_one, tag
            plateau += 1
    for r, w, t in xc.end_rows(roles, "lo"):
        if probs[t, r, 0] == 0.0:   # a leading exact zero: the smallest uniform skips action 0
            assert actions[t, r] == int(np.argmax(probs[t, r] > 0)) >= 1, tag
            zero += 1
        else:
            assert actions[t, r] == 0, tag
    return plateau, zero


def _clamp_holds(r, A, roles):
    rows = xc.clamp_rows(r["cum"], r["u"], A, roles)
    for t, row in rows:
        assert r["actions"][t, row] == A - 1
        assert xc.pick(r["cum"][t, row][None], r["u"][t, row][None], "no_clamp")[0] == A
    return len(rows)


@pytest.mark.parametrize("H", cp.WIDTHS)
@pytest.mark.parametrize("env", xc.SINGLE)
def test_single_agent_cases_cannot_pass_vacuously(env, H):
    A = cp.LAYOUT[env][2]
    _, (hi_act, lo_act) = cp.FORMS[env]
    clamp = 0
    for T in xc.LENGTHS:
        case = xc.SingleCase(env, H, T)
        roles = case.preset()[1]
        plateau = zero = 0
        for kind, packed in cp.kinds(env, H).items():
            r = xc.simulate_single(case, packed)
            tag = (env, H, T, kind)
            assert set(np.unique(r["probs"]).tolist()) <= cp.allowed_probabilities(env, kind), tag
            assert r["wrapped"] == 2 and r["actions"].min() >= 0 and r["actions"].max() < A
            pl, ze = _check_end_rows(kind, r["probs"], r["cum"], r["actions"], r["u"], roles, A, tag)
            plateau, zero = plateau + pl, zero + ze
            limit, early = ((r["done"] > 0) & ~r["early"]).sum(), r["early"].sum()
            last_tick = (r["done"][xc.TICKS - 1] > 0).sum() + (r["done"][xc.TOTAL - 1] > 0).sum()
            assert limit > 0 and last_tick > 0, tag      # at the time limit; on the last tick of a launch
            if kind in ("towards", "away", "switched"):
                counts = np.bincount(r["actions"].ravel(), minlength=A)
                assert counts[hi_act] > 0 and counts[lo_act] > 0 and counts.sum() == counts[hi_act] + counts[lo_act], tag
                assert early > 0, tag                     # both kinds of episode end
                assert env != "mountain_car" or (r["done"] == 2).sum() > 0, tag   # the car reaches the goal
                tie = r["probs"][0, xc.TIE_ROW]
                assert tie[hi_act] == 0.5 and tie[lo_act] == 0.5 and tie.sum() == 1.0, tag
                assert (r["probs"][:, :, [hi_act, lo_act]] == 0.5).all(axis=2).sum() >= 1
        assert plateau >= 8 and zero >= 4, (env, H, T, plateau, zero)
        for shift in xc.CLAMP_SHIFTS:
            c = xc.SingleCase(env, H, T, shift=shift)
            clamp += _clamp_holds(xc.simulate_single(c, c.random_policy(xc.CLAMP_SEED[env, H])), A, c.preset()[1])
    assert clamp >= xc.CLAMP_ROWS_ON_THE_HOST >= xc.CLAMP_ROWS + 4, (env, H, clamp)
    small = xc.SingleCase(env, H, 7, E=1)
    assert small.start_epochs().tolist() == [0xFFFFFFFF] and xc.simulate_single(small, small.packed)["wrapped"] == 1


@pytest.mark.parametrize("H", cp.WIDTHS)
def test_the_cartpole_construction(H):
    """700 spread start states, 40 ticks, T = 13 on oracle/cartpole_np.py: with the gain 2^40 every probability is exactly
    0, 0.5 or 1, both actions occur, "towards the lean" ends most episodes at the time limit and "away from it" ends
    them early; with a gain of 2^20 some rows land in gaps below 104 and the exactness FAILS"""
    case = xc.SingleCase("cartpole", H, 13, E=700)
    ends = {}
    for sign, name in ((1, "towards"), (-1, "away")):
        r = xc.simulate_single(case, cp.pack("cartpole", cp.switched("cartpole", "cartpole", H, sign)), ticks=40)
        assert r["probs"].shape == (40, 700, 2) and set(np.unique(r["probs"]).tolist()) == {0.0, 0.5, 1.0}, name
        assert (np.bincount(r["actions"].ravel(), minlength=2) > 0).all()
        ends[name] = (int(((r["done"] > 0) & ~r["early"]).sum()), int(r["early"].sum()))
    assert ends["towards"][0] > 10 * ends["towards"][1] > 0, ends
    # (the time steps start at row % 13, so some replicas meet the time limit within a few ticks under either sign)
    assert ends["away"][1] > 5 * ends["away"][0] and ends["away"][1] > ends["towards"][0] > 5 * ends["away"][0], ends
    weak = cp.pack("cartpole", cp.switched("cartpole", "cartpole", H, 1, gain=2.0 ** 20))
    r = xc.simulate_single(case, weak, ticks=40)
    assert not set(np.unique(r["probs"]).tolist()) <= {0.0, 0.5, 1.0}


@pytest.mark.parametrize("H", cp.WIDTHS)
def test_gridworld_cases_cannot_pass_vacuously(H):
    clamp = 0
    for T in xc.LENGTHS:
        case = xc.GridCase(H, "sampled", T)
        roles = case.preset()[1]
        plateau = zero = plateau_half = 0
        for kind, packed in cp.kinds("gridworld", H).items():
            r = xc.simulate_grid(case, packed)
            tag = (H, T, kind)
            K, E = xc.TOTAL, case.E
            assert set(np.unique(r["probs"]).tolist()) <= cp.allowed_probabilities("gridworld", kind), tag
            flat = lambda a: a.reshape(K, E * xc.N, *a.shape[3:])   # noqa: E731
            pl, ze = _check_end_rows(kind, flat(r["probs"]), flat(r["cum"]), flat(r["actions"]), flat(r["u"]), roles, 5, tag)
            plateau, zero = plateau + pl, zero + ze
            timed_out = (r["done"] > 0) & ~r["tagged"]
            assert timed_out.sum() > 0 and (r["done"][xc.TICKS - 1] > 0).sum() + (r["done"][K - 1] > 0).sum() > 0, tag
            if kind == "tied":   # the tagger's sums: 0, 0.5, 0.5, 1.0, 1.0 -- a plateau at 0.5 and one at 1.0
                assert (r["cum"][0, 0, 0] == np.array([0, 0.5, 0.5, 1, 1], F32)).all()
                plateau_half += 1
            if kind == "switched":
                tagger = np.bincount(r["actions"][:, :, :4].ravel(), minlength=5)
                runner = np.bincount(r["actions"][:, :, 4].ravel(), minlength=5)
                assert tagger[1] > 0 and tagger[2] > 0 and tagger[[0, 3, 4]].sum() == 0, tag
                assert runner[3] > 0 and runner[4] > 0 and runner[[0, 1, 2]].sum() == 0, tag
                assert r["tagged"].sum() > 0, tag           # both kinds of episode end
                p0 = r["probs"][0, xc.TIE_REPLICA]
                assert (p0[0] == np.array([0, 0.5, 0.5, 0, 0], F32)).all() and (p0[4] == np.array([0, 0, 0, 0.5, 0.5], F32)).all()
        assert plateau >= 8 and zero >= 4 and plateau_half, (H, T, plateau, zero)
        for shift in xc.CLAMP_SHIFTS:
            c = xc.GridCase(H, "sampled", T, shift=shift)
            r = xc.simulate_grid(c, c.policies(xc.CLAMP_SEED["gridworld", H])[1])
            flat = {k: r[k].reshape(xc.TOTAL, c.E * xc.N, *r[k].shape[3:]) for k in ("cum", "u", "actions")}
            clamp += _clamp_holds(flat, 5, c.preset()[1])
    assert clamp >= xc.CLAMP_ROWS_ON_THE_HOST, (H, clamp)


# ------------------------------------------------------------------------------------------------------- evaluation
@pytest.mark.parametrize("H", cp.WIDTHS)
@pytest.mark.parametrize("env", xc.SINGLE)
def test_single_agent_evaluation_cases(env, H):
    """the replay of tests/classic_control_evaluate.py on the crafted kinds: greedy -- uniform gives action 0 on every
    tick, two tied winners the lower index; sampled -- the end rows are reached while their replica still runs, the epoch
    words advance by the steps taken"""
    A = cp.LAYOUT[env][2]
    kinds = cp.kinds(env, H)
    for T in xc.LENGTHS:
        greedy = xc.SingleEvalCase(env, H, "greedy", T)
        r = ev.replay(greedy, packed=kinds["uniform"])
        assert (r["actions"][r["actions"] >= 0] == 0).all() and (r["done"] > 0).all() and r["timeouts"] > 0
        if "tied" in kinds:
            r = ev.replay(greedy, packed=kinds["tied"])
            assert (r["actions"][r["actions"] >= 0] == A - 2).all()
        for kind in ("towards", "away", "switched"):
            if kind in kinds:
                r = ev.replay(greedy, packed=kinds[kind])
                assert r["actions"][0, xc.TIE_ROW] == min(cp.FORMS[env][1])      # the exact tie: the lower index
                assert len(r["end_ticks"]) >= 1 and r["timeouts"] > 0 and (r["counts"] > 0).sum() == 2
        sampled = xc.SingleEvalCase(env, H, "sampled", T)
        epochs, roles, wrap = sampled.preset()
        for kind, packed in kinds.items():
            r = ev.replay(sampled, packed=packed)
            reached = [(r_, t) for r_, (w, k, t) in roles.items() if r["actions"][t, r_] >= 0]
            assert len(reached) >= 10, (env, H, T, kind, len(reached))
            assert (r["epochs"] == epochs + r["steps"].astype(np.uint32)).all() and (r["steps"] > 0).all()


@pytest.mark.parametrize("H", cp.WIDTHS)
def test_gridworld_evaluation_cases(H):
    kinds = cp.kinds("gridworld", H)
    for T in xc.LENGTHS:
        greedy = xc.GridCase(H, "greedy", T, span=xc.EVAL_SPAN)
        r = gev.replay(greedy, packed=kinds["uniform"])
        assert (r["actions"][r["actions"] >= 0] == 0).all() and (r["done"] == 1).all()
        r = gev.replay(greedy, packed=kinds["tied"])
        live = r["actions"][:, :, 0] >= 0
        assert (r["actions"][:, :, :4][live] == 1).all() and (r["actions"][:, :, 4][live] == 2).all()
        r = gev.replay(greedy, packed=kinds["switched"])
        assert r["actions"][0, xc.TIE_REPLICA, 0] == 1 and r["actions"][0, xc.TIE_REPLICA, 4] == 3
        assert r["tagged"].any() and r["timed_out"].any()
        sampled = xc.GridCase(H, "sampled", T, span=xc.EVAL_SPAN)
        epochs, roles, wrap = sampled.preset()
        for kind, packed in kinds.items():
            r = gev.replay(sampled, packed=packed)
            reached = [row for row, (w, k, t) in roles.items() if r["actions"][t, row // xc.N, row % xc.N] >= 0]
            assert len(reached) >= 10, (H, T, kind, len(reached))
            assert (r["epochs"] == sampled.start_epochs() + r["steps"].astype(np.uint32)[:, None]).all()


# ------------------------------------------------------------------------------------------------- planted defects
def _differs(a, b):
    return bool((np.asarray(a) != np.asarray(b)).any())


@pytest.mark.parametrize("H", cp.WIDTHS)
@pytest.mark.parametrize("env", ENVS)
def test_every_planted_defect_is_caught_where_it_applies(env, H):
    """each defect in the MODEL changes the actions of at least one case of this env; the kinds that must catch it do"""
    A = cp.LAYOUT[env][2]
    grid = env == "gridworld"
    case = xc.GridCase(H, "sampled", 7) if grid else xc.SingleCase(env, H, 7)
    sim = xc.simulate_grid if grid else xc.simulate_single
    kinds = cp.kinds(env, H)
    good = {kind: sim(case, packed)["actions"] for kind, packed in kinds.items()}
    caught = {d: {kind for kind, packed in kinds.items() if _differs(sim(case, packed, d)["actions"], good[kind])}
              for d in ("le", "drop_w0_last_column", "drop_last_hidden", "bias_after_relu")}
    constants = set(cp.constant_kinds(env))
    switched = {"switched"} if env != "cartpole" else {"towards", "away"}
    assert caught["le"] >= {"winner0"} | ({f"winner{A // 2}"} if A >= 3 else set()), caught     # the plateau at 1.0
    assert caught["drop_last_hidden"] >= constants | switched, caught
    assert caught["bias_after_relu"] >= constants, caught
    if env != "acrobot":   # (Acrobot's form reads theta_dot_1, column 4 of 6)
        assert caught["drop_w0_last_column"] >= switched, caught
    # no clamp: the random policy's clamp rows give A
    rand = case.policies(xc.CLAMP_SEED[env, H])[1] if grid else case.random_policy(xc.CLAMP_SEED[env, H])
    found = False
    for shift in xc.CLAMP_SHIFTS:
        c = xc.GridCase(H, "sampled", 7, shift=shift) if grid else xc.SingleCase(env, H, 7, shift=shift)
        found = found or _differs(sim(c, rand, "no_clamp")["actions"], sim(c, rand)["actions"])
    assert found
    # the last maximum instead of the first: every greedy tie
    for kind in ["uniform"] + (["tied"] if A >= 3 else []):
        obs = np.zeros((3, cp.LAYOUT[env][0]), F32)
        p = xc.probabilities(env, kinds[kind][0] if grid else kinds[kind], H, obs)
        assert (xc.greedy(p) < xc.greedy(p, "last_max")).all(), kind
    if grid:   # tagger and runner swapped
        swapped = {kind for kind, packed in kinds.items() if _differs(sim(case, packed, "swap_policies")["actions"], good[kind])}
        assert swapped >= {"winner0", "winner4", "tied", "switched"}, swapped


# ------------------------------------------------------------------------------- the logits entries' host side
def test_rational_rounding_and_the_exact_row():
    """`round_to_float32` is numpy's rounding of a double on doubles (ties, subnormals and both signs included), and one row
    redone in exact rational arithmetic gives the restatement's logits"""
    from fractions import Fraction

    from tests import inkernel_policy_logit_cases as lc

    rng = np.random.RandomState(9)
    base = (rng.standard_normal(300) * 10.0 ** rng.randint(-44, 30, 300)).astype(F32)
    up = np.nextafter(base, F32(np.inf))
    doubles = np.concatenate([base.astype(np.float64), (base.astype(np.float64) + up.astype(np.float64)) / 2,   # exact ties
                              rng.standard_normal(300) * 10.0 ** rng.randint(-46, 30, 300), [0.0, 2.0 ** -150, 2.0 ** -149]])
    for d in doubles:
        assert lc.round_to_float32(Fraction(float(d))).tobytes() == np.float32(d).tobytes() or d == 0, d
    for form in sorted(lc.FORMS):
        parts = lc.random_parts(lc.FORMS[form], 32, 5, 2)
        obs = lc.rows(form)
        want = lc.restated(form, parts, obs)[0]
        for r in (0, 41, 68, 69):
            assert lc.exact_logits_row(parts, obs[r]).tobytes() == want[r].tobytes(), (form, r)


@pytest.mark.parametrize("form", ["f4", "f2o2", "f2o6", "s21"])
def test_logit_cases_on_the_host(form):
    """the crafted kinds are exact on the 70 rows (every probability 0, 0.5, 1 or 1 / A in the restatement), the float32
    restatement lies within a few ulps of the float64 reference, and the rows hold what they should"""
    from tests import inkernel_policy_logit_cases as lc

    obs = lc.rows(form)
    assert obs.shape[0] == 70 and (obs[:40] < 0).any() and (obs[40:68] >= 0).all() and not obs[68].any()
    assert np.signbit(obs[69]).all() and not np.signbit(obs[68]).any()
    for H in lc.WIDTHS:
        for A in lc.ACTIONS:
            pols = lc.policies(form, H, A)
            assert sum(1 for _, exact in pols.values() if not exact) == 3
            for name, (parts, exact) in pols.items():
                logits, probs, cum, best = lc.restated(form, parts, obs)
                l64, p64, c64 = lc.reference_f64(parts, obs)
                assert np.abs(probs - p64).max() < 1e-5 and (best >= 0).all() and (best < A).all(), (form, H, A, name)
                if exact:
                    allowed = {0.0, 0.5, 1.0, float(F32(1.0) / F32(A))}
                    assert set(np.unique(probs).tolist()) <= allowed, (form, H, A, name)
                    assert (cum[:, -1] == 1.0).all()
