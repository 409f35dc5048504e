"""Build-time checks of the sparse row flush of the multi-tick TagContinuous entry (HipTagContinuousRollout_K10_N105A21):
the flush loop of tc_gather_rows_sparse's LOOP variant works from per-row descriptors, so it is much shorter than the
form the one-tick entries keep, and the entry still fits eight blocks per CU.  No GPU needed: hipcc cross-compiles gfx950."""
import os
import re
import subprocess

import pytest

ROLLOUT = "HipTagContinuousRollout_K10_N105A21"
UNIT = "wd_kernels_tc_k10_n105a21_rollout.hsaco"
# static instructions of the sparse flush loop in the parent of the descriptor form (commit 0e4e6e2), counted by
# sparse_flush_loop() below on that commit's code object
PARENT_FLUSH_INSTRUCTIONS = 329


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge

    ge.build()
    from warp_drive_amd.managers import hip_driver as drv

    return drv


def _llvm():
    from warp_drive_amd import build as wd_build

    return os.path.join(wd_build.ROCM, "lib", "llvm", "bin")


def unbundle(hsaco, tmp_path):
    elf = str(tmp_path / (os.path.basename(hsaco) + ".elf"))
    subprocess.run([os.path.join(_llvm(), "clang-offload-bundler"), "--unbundle", "--type=o",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={hsaco}", f"--output={elf}"],
                   check=True, capture_output=True)
    return elf


def kernel_lines(elf, kernel):
    """[(address, text)] of one kernel's instructions"""
    text = subprocess.run([os.path.join(_llvm(), "llvm-objdump"), "-d", elf], check=True, capture_output=True,
                          text=True).stdout
    m = re.search(rf"^[0-9a-f]+ <{kernel}>:\n(.*?)(?=^[0-9a-f]+ <[A-Za-z_]|\Z)", text, re.M | re.S)
    assert m, kernel
    out = []
    for line in m.group(1).splitlines():
        a = re.search(r"//\s*([0-9A-Fa-f]+):", line)
        if a:
            out.append((int(a.group(1), 16), line))
    return out


def sparse_flush_loop(lines, kernel=ROLLOUT):
    """the innermost backward-branch loop that holds a write-through (sc1) 16-byte store and a ds_read_u8 or a
    ds_bpermute_b32: the flush loop of the sparse row form.  Returns its instruction lines."""
    base = lines[0][0]
    spans = []
    for a, line in lines:
        m = re.search(r"s_c?branch\w*\s+\d+\s+//.*<" + kernel + r"\+0x([0-9a-f]+)>", line)
        if m and base + int(m.group(1), 16) < a:
            spans.append((base + int(m.group(1), 16), a))
    hits = []
    for lo, hi in spans:
        body = [line for a, line in lines if lo <= a <= hi]
        text = "\n".join(body)
        if re.search(r"global_store_dwordx4\b.*\bsc1\b", text) and re.search(r"\bds_read_u8\b|\bds_bpermute_b32\b", text):
            hits.append((hi - lo, body))
    assert hits, "no loop with a write-through 16-byte store and a byte read / bpermute: where is the sparse flush?"
    return min(hits, key=lambda h: h[0])[1]


def test_sparse_flush_loop_is_at_most_60_percent_of_the_parents(built, tmp_path):
    """The parent's flush loop (three rounds of three rows per trip, every per-row quantity recomputed per round) has
    329 static instructions (PARENT_FLUSH_INSTRUCTIONS, counted by sparse_flush_loop on the parent's object); the
    descriptor form may have at most 60 % of that, 197.  It has 173."""
    body = sparse_flush_loop(kernel_lines(unbundle(built.code_object_path(UNIT), tmp_path), ROLLOUT))
    n = len(body)
    print("sparse flush loop:", n, "static instructions; parent:", PARENT_FLUSH_INSTRUCTIONS)
    assert n * 100 <= PARENT_FLUSH_INSTRUCTIONS * 60, (n, PARENT_FLUSH_INSTRUCTIONS)
    # the loop still holds its own-dword store sites (four per round) and the three 16-byte stores
    text = "\n".join(body)
    assert len(re.findall(r"\bglobal_store_dword\b", text)) >= 12
    assert len(re.findall(r"\bglobal_store_dwordx4\b.*\bsc1\b", text)) >= 3


def test_rollout_entry_keeps_its_resources(built, tmp_path):
    elf = unbundle(built.code_object_path(UNIT), tmp_path)
    notes = subprocess.run([os.path.join(_llvm(), "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                           text=True).stdout
    field = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", notes).group(1))
    assert field("vgpr_count") <= 128
    assert field("vgpr_spill_count") == 0
    assert field("private_segment_fixed_size") == 0
    assert field("agpr_count") == 0
    assert "scratch_" not in "\n".join(line for _, line in kernel_lines(elf, ROLLOUT))
    from warp_drive_amd.envs.tag_continuous import TagContinuous
    from tests.test_gpu_tag_continuous import BENCH_CFG

    assert TagContinuous(**BENCH_CFG).lds_bytes(1, fused=True, threads=128) <= 20480
