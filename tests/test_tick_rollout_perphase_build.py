"""Build-time checks of the per-agent phases of the multi-tick TagContinuous entry (HipTagContinuousRollout_K10_N105A21):
the divisions by launch constants are products with reciprocals formed in front of the loop (tc_div_const, tc_divide.h), and
the five square roots of the tag scan lie behind a wave-uniform vote on the squared distances (tc_find_tag<SKIP>, tc_tags.h).
Read off the disassembly with the helpers of tests/test_tick_rollout_build.py and tests/test_tick_rollout_carry_build.py; no
GPU needed.

How "cold" is read.  The true divisions that remain (float32 only: dividends outside the class the reciprocal form is proved
for send their wavefront there) may be laid out in line, behind a wave-uniform forward branch that jumps over them, or out of
line, as the compiler does for a block marked unlikely: an island that starts right behind an unconditional branch (nothing
falls into it), ends with an unconditional branch back, and is entered only through wave-uniform conditional branches
(`s_cbranch_vcc*` / `s_cbranch_scc*`) that lie in front of it.  Either way a wavefront whose dividends are ordinary executes
none of them.  Exec-mask skips (`s_cbranch_execz`) do not count: every trip walks up to them."""
import os
import re
import subprocess

from tests.test_tick_rollout_build import ROLLOUT, UNIT, _body, _elf, built  # noqa: F401  (`built`: the module's fixture)
from tests.test_tick_rollout_carry_build import _ADDR, _BRANCH, _loop_body, _op

PARENT_LOOP_BODY = 4260   # static instructions of the loop body before this change
ISLAND_MAX = 64           # a cold block is short
_DIV = re.compile(r"^(v_div_scale_|v_div_fixup_|v_div_fmas_|v_rcp_f64)")


def _kernel(built, tmp_path):
    """every instruction of the kernel as (address, text, branch mnemonic, branch target), and the loop body's address range"""
    llvm, elf = _elf(built, UNIT, tmp_path)
    text = _body(llvm, elf, ROLLOUT)
    rows = [(int(m.group(1), 16), l.strip()) for l in text.splitlines() for m in [_ADDR.search(l)] if m]
    base = rows[0][0]
    ins = []
    for a, l in rows:
        b = _BRANCH.search(l)
        ins.append((a, l, b.group(1) if b else None, base + int(b.group(2), 16) if b else None))
    body = _loop_body(text)
    return ins, body


def _uniform(b):
    return b is not None and (b.startswith("s_cbranch_scc") or b.startswith("s_cbranch_vcc"))


def _is_cold(ins, i):
    """instruction i lies in line behind a wave-uniform forward branch that jumps over it, or in an out-of-line island"""
    a = ins[i][0]
    for j in range(max(0, i - ISLAND_MAX), i):  # in line
        aj, _, b, t = ins[j]
        if _uniform(b) and aj < a < t:
            return True
    s = i
    while s > 0 and not (ins[s - 1][2] == "s_branch" or _op(ins[s - 1][1]) == "s_endpgm"):
        s -= 1
    e = i
    while e < len(ins) - 1 and ins[e][2] != "s_branch":
        e += 1
    if s == 0 or ins[e][2] != "s_branch" or e - s + 1 > ISLAND_MAX:
        return False
    lo, hi = ins[s][0], ins[e][0]
    entries = [(aj, b, t) for aj, _, b, t in ins if t is not None and lo <= t <= hi and not (lo <= aj <= hi)]
    return bool(entries) and all(_uniform(b) and aj < lo and t == lo for aj, b, t in entries)


def test_no_true_division_on_the_hot_path_of_the_loop(built, tmp_path):
    ins, body = _kernel(built, tmp_path)
    loop_lo = body[0][0]
    div = [i for i, (a, l, _, _) in enumerate(ins) if a >= loop_lo and _DIV.match(_op(l))]
    hot = [ins[i][1] for i in div if not _is_cold(ins, i)]
    assert hot == [], hot
    # no float64 division is left at all, hot or cold: positions and the time column have no dividend class to exclude
    assert not [ins[i][1] for i in div if "f64" in _op(ins[i][1])]
    # ... and the reciprocals ARE formed by true divisions in front of the loop: one float32, two float64
    front = [_op(l) for a, l, _, _ in ins if a < loop_lo]
    assert front.count("v_div_fixup_f32") == 1 and front.count("v_div_fixup_f64") == 2
    # the reciprocal form itself: float64 FMAs in the body with a negated product operand (the residual's sign, tc_divide.h)
    assert sum(1 for _, l, _, _ in body if _op(l) == "v_fma_f64") >= 6


def test_tag_roots_lie_behind_one_vote_on_the_squared_distances(built, tmp_path):
    _, body = _kernel(built, tmp_path)
    ops = [_op(l) for _, l, _, _ in body]
    roots = [i for i, o in enumerate(ops) if o.startswith("v_sqrt_f32")][:5]  # the tag scan is the first user of sqrtf in a trip
    assert len(roots) == 5 and roots[4] - roots[0] < 120
    guards = [i for i in range(max(0, roots[0] - 12), roots[0])
              if _uniform(body[i][2]) and body[i][3] > body[roots[4]][0]]
    assert len(guards) == 1, [body[i][1] for i in guards]
    g = guards[0]
    # what the vote reads was computed right in front of it: five sums of two squares, their unsigned minimum and maximum
    before = ops[max(0, g - 60):g]
    assert before.count("v_mul_f32_e32") + 2 * before.count("v_pk_mul_f32") >= 10
    assert before.count("v_add_f32_e32") + 2 * before.count("v_pk_add_f32") >= 5
    assert "v_min3_u32" in before and "v_max3_u32" in before
    assert not any(o.startswith("v_sqrt_f32") for o in before)
    # nothing else enters the guarded block from outside: the roots are reached through the vote alone
    lo, hi = body[g][0], body[g][3]
    assert not [l for a, l, _, t in body if t is not None and lo < t < hi and not (lo <= a < hi)]


def test_body_is_no_longer_than_the_parents_and_resources_hold(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    body = _loop_body(_body(llvm, elf, ROLLOUT))
    print(f"loop body: {len(body)} static instructions (parent: {PARENT_LOOP_BODY})")
    assert len(body) <= PARENT_LOOP_BODY
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                           text=True).stdout
    field = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", notes).group(1))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0
    assert field("vgpr_count") <= 128
    assert field("agpr_count") == 0
    assert "scratch_" not in _body(llvm, elf, ROLLOUT)
    from warp_drive_amd.envs.tag_continuous import TagContinuous
    from tests.test_gpu_tag_continuous import BENCH_CFG

    assert TagContinuous(**BENCH_CFG).lds_bytes(1, fused=True, threads=128) <= 20480


def test_verifier_is_not_in_the_rollout_object(built):
    from warp_drive_amd import build as wd_build

    assert built.manifest()["HipTagContinuousVerifyInvariantDivide"] == "wd_kernels_tc.hsaco"
    assert wd_build.kernels_in(built.code_object_path(UNIT)) == [ROLLOUT]
