"""Build-time checks of the observation-row gather of the multi-tick TagContinuous entry
(HipTagContinuousRollout_K10_N105A21): the dense chunk loop is the lean form built for the one shape (tc_rows.h,
tc_gather_rows_dense_lean), so it is shorter than the generic chunk loop the one-tick entries keep; the entry keeps its
resources, its loop body the store sites it had; every other code object is the byte-identical file of the parent.
Read off the disassembly with the helpers of tests/test_tick_rollout_rows_build.py; no GPU needed.

How the chunk loops are recognised.  A chunk of either row form narrows float64 differences (`v_cvt_f32_f64`) and ends in
write-through 16-byte stores (`global_store_dwordx4 .. sc1`); nothing else in the kernel does both.  The sparse chunk loop
is the smallest backward-branch span with both that also fetches descriptors (`ds_bpermute_b32`) -- its flush loop
(sparse_flush_loop of tests/test_tick_rollout_rows_build.py) is counted apart; the dense chunk loop is the smallest span
with both and no `ds_bpermute_b32`.  The detectors are checked against each other: the two loops do not overlap."""
import hashlib
import os
import re
import subprocess

from tests.test_tick_rollout_build import ROLLOUT, UNIT, _body, _elf, built  # noqa: F401  (`built`: the module's fixture)
from tests.test_tick_rollout_carry_build import _loop_body
from tests.test_tick_rollout_rows_build import kernel_lines, sparse_flush_loop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# static instructions of the parent's object (commit 83eaa92), counted by the functions below
PARENT_DENSE_CHUNK_LOOP = 318
PARENT_SPARSE_GATHER = 245          # the sparse chunk loop, 418, less its flush loop, 173
# ceilings: what the finished build of this change shows (docs/rounds/r35.md)
DENSE_CHUNK_LOOP_MAX = 242
SPARSE_GATHER_MAX = 210
LOOP_BODY_FENCE = 4260
STORE_SITES = {"dword": 36, "dwordx2": 2, "dwordx4": 14}   # the parent's loop body (docs/rounds/r32.md)
SHA_LIST = os.path.join(ROOT, "profiles", "r35_code_object_sha256.txt")


def _spans(lines, kernel=ROLLOUT):
    """[(lo, hi)] of every backward branch of the kernel"""
    base = lines[0][0]
    out = []
    for a, line in lines:
        m = re.search(r"s_c?branch\w*\s+\d+\s+//.*<" + kernel + r"\+0x([0-9a-f]+)>", line)
        if m and base + int(m.group(1), 16) < a:
            out.append((base + int(m.group(1), 16), a))
    return out


def _chunk_loop(lines, with_descriptors):
    hits = []
    for lo, hi in _spans(lines):
        body = [(a, line) for a, line in lines if lo <= a <= hi]
        text = "\n".join(line for _, line in body)
        if re.search(r"global_store_dwordx4\b.*\bsc1\b", text) and re.search(r"\bv_cvt_f32_f64", text) and \
                bool(re.search(r"\bds_bpermute_b32\b", text)) == with_descriptors:
            hits.append((hi - lo, body))
    assert hits, "no chunk loop of the %s row form" % ("sparse" if with_descriptors else "dense")
    return min(hits, key=lambda h: h[0])[1]


def dense_chunk_loop(lines):
    return [line for _, line in _chunk_loop(lines, False)]


def sparse_chunk_loop(lines):
    """(the sparse chunk loop, its flush loop)"""
    return [line for _, line in _chunk_loop(lines, True)], sparse_flush_loop(lines)


def _lines(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    return kernel_lines(elf, ROLLOUT)


def test_dense_chunk_loop_is_the_lean_form(built, tmp_path):
    lines = _lines(built, tmp_path)
    dense = _chunk_loop(lines, False)
    sparse = _chunk_loop(lines, True)
    assert dense[-1][0] < sparse[0][0] or sparse[-1][0] < dense[0][0], "the two chunk loops are one span"
    n = len(dense)
    print(f"dense chunk loop: {n} static instructions (parent: {PARENT_DENSE_CHUNK_LOOP}, ceiling: {DENSE_CHUNK_LOOP_MAX})")
    assert DENSE_CHUNK_LOOP_MAX < PARENT_DENSE_CHUNK_LOOP   # (the test fails on the parent's object)
    assert n <= DENSE_CHUNK_LOOP_MAX
    text = "\n".join(line for _, line in dense)
    # the items' records are not fetched under a branch on the own record, and no lane clamps its item index per chunk
    gather = text[:text.rindex("v_cvt_f32_f64")]   # (up to the last item's differences; the flush's reads come later)
    assert len(re.findall(r"\bds_read_b128\b|\bds_read_b96\b", gather)) == 12   # two records of two halves per item
    assert "s_cbranch_execz" not in gather
    assert "v_min_i32" not in gather and "v_min_u32" not in gather
    # the time fraction is not fetched per row: no float conversion of a row index in front of the flush
    front = text[:text.index("global_store_dwordx4")]
    assert "v_cvt_f32_i32" not in front and "v_cvt_i32_f32" not in front
    # the flush is the one it was: six write-through 16-byte store sites and the two single-dword ends
    assert len(re.findall(r"\bglobal_store_dwordx4\b.*\bsc1\b", text)) == 6
    assert len(re.findall(r"\bglobal_store_dword\b", text)) == 2


def test_sparse_gather_side_is_the_lean_form(built, tmp_path):
    chunk, flush = sparse_chunk_loop(_lines(built, tmp_path))
    n = len(chunk) - len(flush)
    print(f"sparse chunk loop: {len(chunk)} static instructions, {len(flush)} of them the flush loop; gather side {n} "
          f"(parent: {PARENT_SPARSE_GATHER}, ceiling: {SPARSE_GATHER_MAX})")
    assert SPARSE_GATHER_MAX < PARENT_SPARSE_GATHER   # (the test fails on the parent's object)
    assert n <= SPARSE_GATHER_MAX
    text = "\n".join(chunk)
    gather = text[:text.index("\n".join(flush[:3]))]
    # the row of an item comes from its slot's lane, not from the row list: one byte read per chunk (the slot's own
    # lane), three fetches across lanes; no replica index is worked out for the time column
    assert len(re.findall(r"\bds_read_u8\b", gather)) == 1
    assert len(re.findall(r"\bds_bpermute_b32\b", gather)) == 3
    assert "v_cvt_f32_i32" not in gather and "v_cvt_i32_f32" not in gather


def test_resources_fence_and_store_sites(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                           text=True).stdout
    field = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", notes).group(1))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0
    assert field("vgpr_count") <= 128
    assert field("agpr_count") == 0
    text = _body(llvm, elf, ROLLOUT)
    assert "scratch_" not in text
    from warp_drive_amd.envs.tag_continuous import TagContinuous
    from tests.test_gpu_tag_continuous import BENCH_CFG

    assert TagContinuous(**BENCH_CFG).lds_bytes(1, fused=True, threads=128) == 20468
    body = [l for _, l, _, _ in _loop_body(text)]
    print(f"loop body: {len(body)} static instructions (fence: {LOOP_BODY_FENCE})")
    assert len(body) <= LOOP_BODY_FENCE
    sites = {w: sum(1 for l in body if re.match(rf"global_store_{w}\b", l)) for w in STORE_SITES}
    assert sites == STORE_SITES, sites


def _sha_sections():
    """{"parent": {file: sha256}, "this tree": {...}} of profiles/r35_code_object_sha256.txt"""
    out, cur = {}, None
    for line in open(SHA_LIST):
        line = line.strip()
        if line in ("# parent", "# this tree"):
            cur = out.setdefault(line[2:], {})
        elif line and not line.startswith("#"):
            sha, name = line.split()
            cur[name] = sha
    return out


def test_every_other_code_object_is_the_parents(built):
    from warp_drive_amd import build as wd_build

    rec = _sha_sections()
    parent, new = rec["parent"], rec["this tree"]
    assert set(parent) == set(new) == set(wd_build.UNITS)
    assert [n for n in parent if parent[n] != new[n]] == [UNIT]
    sha = lambda path: hashlib.sha256(open(path, "rb").read()).hexdigest()
    differ = [n for n in new if n != UNIT and sha(built.code_object_path(n)) != parent[n]]
    assert differ == [], differ
    assert sha(built.code_object_path(UNIT)) == new[UNIT]
