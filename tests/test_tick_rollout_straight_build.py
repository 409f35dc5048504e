"""Build-time checks of the slab issue of the multi-tick TagContinuous entry (HipTagContinuousRollout_K10_N105A21): the two
probability slabs go out as straight-line code (tc_fetch_slabs_straight, tc_fetch.h), not as the divergent exec-mask loops
that the generic fetch compiles to, and the loop body stays as short as that made it.  Read off the disassembly of the code
object with the helpers of tests/test_tick_rollout_build.py and tests/test_tick_rollout_carry_build.py; no GPU needed.

The counts are STATIC instruction counts in address order (both wavefronts' code, every branch of the trip), so they say how
much code there is, not how much of it one wavefront executes; docs/rounds/r23.md has the executed counts.

The resources (at most 128 VGPRs, no spill, no scratch, no AGPR, LDS at most 20 480 bytes) are asserted by the two files
named above."""
from tests.test_tick_rollout_build import ROLLOUT, UNIT, _body, _elf, built  # noqa: F401  (`built`: the module's fixture)
from tests.test_tick_rollout_carry_build import _loop_body, _op

# Before the straight-line slab issue and the full-chunk row flush (the parent commit, same flags): 166 instructions from the
# first global_load_lds to the slab wait, 4345 in the whole loop body.
# Achieved: 166 again and 4335.  The span from the first global_load_lds to the slab wait now holds the straight-line issue
# of BOTH wavefronts side by side (a wavefront walks through one of them) where it held the tail of one shared loop; what
# fell is the code in front of the first global_load_lds (245 -> 232) and what a wavefront executes (docs/rounds/r23.md).
SLAB_TO_WAIT_MAX = 170
LOOP_BODY_MAX = 4345


def _spans(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    body = _loop_body(_body(llvm, elf, ROLLOUT))
    ops = [_op(l) for _, l, _, _ in body]
    lds = [i for i, o in enumerate(ops) if o.startswith("global_load_lds")]
    assert lds, "the loop body fetches no slab"
    wait = next(i for i in range(lds[-1] + 1, len(body)) if ops[i] == "s_waitcnt" and "vmcnt" in body[i][1])
    return body, ops, lds, wait


def test_no_backward_branch_inside_the_slab_issue(built, tmp_path):
    body, ops, lds, _ = _spans(built, tmp_path)
    back = [l for a, l, b, t in body[lds[0]:lds[-1] + 1] if b and t <= a]
    assert back == []
    # every piece of both wavefronts is a site of its own: 2 slabs x (6 pieces of wavefront 0 + 4 pieces and a dword of wavefront 1)
    assert len(lds) == 22
    assert sum(o == "global_load_lds_dword" for o in ops) == 2


def test_m0_is_written_once_per_base_not_once_per_piece(built, tmp_path):
    """a wavefront's pieces of a slab share their LDS base through the instruction's immediate offset: fewer writes of m0 than
    loads, and no v_readfirstlane (the generic fetch's per-piece chain) anywhere in the slab issue"""
    body, ops, lds, _ = _spans(built, tmp_path)
    span = body[lds[0] - 12:lds[-1] + 1]
    m0 = [l for _, l, _, _ in span if " m0," in l and not l.startswith("global_")]
    assert 0 < len(m0) <= 14, m0   # wavefront 0: 4 bases + 2 in the masked piece; wavefront 1: 2 + 2 + 2, and slack of 2
    assert not [l for _, l, _, _ in span if l.startswith("v_readfirstlane")]


def test_instruction_counts_stay_at_or_below_their_ceilings(built, tmp_path):
    body, ops, lds, wait = _spans(built, tmp_path)
    print(f"first global_load_lds -> slab wait: {wait - lds[0]} instructions; loop body: {len(body)}")
    assert wait - lds[0] <= SLAB_TO_WAIT_MAX
    assert len(body) <= LOOP_BODY_MAX
