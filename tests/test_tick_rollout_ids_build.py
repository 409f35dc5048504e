"""Build-time checks of the neighbour-id rows of the multi-tick TagContinuous entry (HipTagContinuousRollout_K10_N105A21):
the lanes that found the ids store the rows of `nearest_neighbor_ids` from registers, so the loop that read every 16-bit id
back from LDS and stored it widened (tc_flush_ids, which the one-tick entries keep) is gone from the loop body, and the body
is shorter than its parent's.  Read off the disassembly with the helpers of tests/test_tick_rollout_build.py; no GPU needed.

How the id flush is recognised: an INNERMOST backward-branch span (one that holds no other backward branch: a backward
branch is also how a block laid out of line returns, and such a span holds whole phases of the tick) with an LDS
read, the sign extension of 16-bit values (0xffff becomes -1: `ds_read_i16`, or `v_bfe_i32 .., 0, 16` on the halves of a
wider read, which is what the compiler makes of four adjacent 16-bit reads) and a 16-byte global store in it.  The dense
gather also reads the ids, but zero-extended and as indices of LDS records, never as store data.  The detector is checked
against the one-tick entry of the same shape, which must have exactly such a loop."""
import os
import re
import subprocess

from tests.test_tick_rollout_build import ROLLOUT, TICK, UNIT, _body, _elf, built  # noqa: F401  (`built`: the module's fixture)
from tests.test_tick_rollout_carry_build import _ADDR, _loop_body

PARENT_LOOP_BODY = 4247   # static instructions of the loop body before this change
TICK_UNIT = "wd_kernels_tc_k10_n105a21.hsaco"


def _inner_loops(text, kernel):
    """the instruction lines of every innermost backward-branch span of a kernel"""
    rows = [(int(m.group(1), 16), l.strip()) for l in text.splitlines() for m in [_ADDR.search(l)] if m]
    base = rows[0][0]
    spans = []
    for a, l in rows:
        m = re.search(r"\bs_c?branch\w*\s+\d+\s+//.*<" + kernel + r"\+0x([0-9a-f]+)>", l)
        if m and base + int(m.group(1), 16) < a:
            spans.append((a - (base + int(m.group(1), 16)), base + int(m.group(1), 16), a))
    spans = [s for s in spans if not any(o != s and s[1] <= o[1] and o[2] <= s[2] for o in spans)]
    return [[l for a, l in rows if lo <= a <= hi] for _, lo, hi in spans]


def _id_flush_loops(text, kernel):
    return [b for b in _inner_loops(text, kernel)
            if any(l.startswith("ds_read") for l in b) and any(l.startswith("global_store_dwordx4") for l in b) and
            any(l.startswith("ds_read_i16") or re.match(r"v_bfe_i32 v\d+, v\d+, 0, 16\b", l) for l in b)]


def test_body_is_shorter_than_the_parents(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    body = _loop_body(_body(llvm, elf, ROLLOUT))
    print(f"loop body: {len(body)} static instructions (parent: {PARENT_LOOP_BODY})")
    assert len(body) < PARENT_LOOP_BODY


def test_no_loop_reads_the_ids_back_and_stores_them(built, tmp_path):
    llvm, elf1 = _elf(built, TICK_UNIT, tmp_path)
    assert len(_id_flush_loops(_body(llvm, elf1, TICK), TICK)) >= 1  # the detector finds tc_flush_ids where it is
    llvm, elf = _elf(built, UNIT, tmp_path)
    text = _body(llvm, elf, ROLLOUT)
    found = _id_flush_loops(text, ROLLOUT)
    assert found == [], found[0]
    # the rows leave from registers instead: 16-byte and 8-byte stores that are not write-through row flushes
    body = [l for _, l, _, _ in _loop_body(text)]
    assert sum(l.startswith("global_store_dwordx4") and "sc1" not in l for l in body) >= 2
    assert sum(l.startswith("global_store_dwordx2") for l in body) >= 2  # (the actions, and the tail of an id row)


def test_resources_hold(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
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
