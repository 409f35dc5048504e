"""Build-time checks of the multi-tick TagContinuous entry (HipTagContinuousRollout_K10_N105A21, a code object of its own):
it is in the manifest, it fits the resources that keep eight blocks on a CU (128 VGPRs, no spills, no scratch, 20 480
bytes of LDS), and its loop body stores what the one-tick entry stores.  No GPU needed: hipcc cross-compiles gfx950."""
import os
import re
import subprocess

import pytest

ROLLOUT = "HipTagContinuousRollout_K10_N105A21"
TICK = "HipTagContinuousTick_K10_N105A21"
UNIT = "wd_kernels_tc_k10_n105a21_rollout.hsaco"


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge

    ge.build()
    from warp_drive_amd.managers import hip_driver as drv

    return drv


def _elf(drv, obj, tmp_path):
    from warp_drive_amd import build as wd_build

    llvm = os.path.join(wd_build.ROCM, "lib", "llvm", "bin")
    elf = str(tmp_path / (obj + ".elf"))
    subprocess.run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={drv.code_object_path(obj)}",
                    f"--output={elf}"], check=True, capture_output=True)
    return llvm, elf


def _body(llvm, elf, kernel):
    """disassembly of one kernel: the lines between its label and the next symbol's"""
    text = subprocess.run([os.path.join(llvm, "llvm-objdump"), "-d", elf], check=True, capture_output=True, text=True).stdout
    m = re.search(rf"^[0-9a-f]+ <{kernel}>:\n(.*?)(?=^[0-9a-f]+ <[A-Za-z_]|\Z)", text, re.M | re.S)
    assert m, kernel
    return m.group(1)


def test_rollout_entry_is_in_the_manifest_in_its_own_object(built):
    from warp_drive_amd import build as wd_build

    assert UNIT in wd_build.UNITS
    assert built.manifest()[ROLLOUT] == UNIT
    assert built.manifest()[TICK] == "wd_kernels_tc_k10_n105a21.hsaco"  # the one-tick object is not touched
    assert wd_build.kernels_in(built.code_object_path(UNIT)) == [ROLLOUT]


def test_rollout_entry_fits_eight_blocks_per_cu(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                           text=True).stdout
    assert len(re.findall(r"\.name:\s+Hip\w+\n", notes)) == 1 and f".name:           {ROLLOUT}\n" in notes  # one kernel
    field = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", notes).group(1))
    assert field("private_segment_fixed_size") == 0   # no scratch
    assert field("vgpr_spill_count") == 0
    assert field("vgpr_count") <= 128                  # four wavefronts per SIMD
    assert field("agpr_count") == 0
    assert "scratch_" not in _body(llvm, elf, ROLLOUT)
    # LDS as the host sizes it for the launch: eight blocks of at most 20 480 bytes are the 160 KiB of a CU
    from warp_drive_amd.envs.tag_continuous import TagContinuous
    from tests.test_gpu_tag_continuous import BENCH_CFG

    env = TagContinuous(**BENCH_CFG)
    assert env.lds_bytes(1, fused=True, threads=128) <= 20480


def test_rollout_loop_stores_what_the_tick_stores(built, tmp_path):
    """no store of a tick may be dropped because a later tick overwrites it: the loop body (from the loop's first
    instruction to its backward branch) holds at least as many global stores, of every width, as the one-tick entry"""
    llvm, elf = _elf(built, UNIT, tmp_path)
    loop = _body(llvm, elf, ROLLOUT)
    llvm, elf1 = _elf(built, "wd_kernels_tc_k10_n105a21.hsaco", tmp_path)
    tick = _body(llvm, elf1, TICK)
    count = lambda text: {w: len(re.findall(rf"\bglobal_store_{w}\b", text))
                          for w in ("byte", "short", "dword", "dwordx2", "dwordx3", "dwordx4")}
    # the body of the tick loop: the code between the target of the LAST backward branch whose span holds stores and the branch
    lines = loop.splitlines()
    addr = lambda l: int(re.search(r"//\s*([0-9A-Fa-f]+):", l).group(1), 16)
    spans = []
    for i, l in enumerate(lines):
        m = re.search(r"s_cbranch_\w+\s+\d+\s+//.*<" + ROLLOUT + r"\+0x([0-9a-f]+)>", l) or \
            re.search(r"s_branch\s+\d+\s+//.*<" + ROLLOUT + r"\+0x([0-9a-f]+)>", l)
        if m:
            target = addr(lines[0]) + int(m.group(1), 16)
            if target < addr(l):
                spans.append((addr(l) - target, target, addr(l)))
    assert spans, "no backward branch: the entry has no loop"
    _, lo, hi = max(spans)  # the outermost loop
    body = "\n".join(l for l in lines if re.search(r"//\s*[0-9A-Fa-f]+:", l) and lo <= addr(l) <= hi)
    c_loop, c_tick = count(body), count(tick)
    assert c_tick["dwordx4"] >= 11  # (the row flush, the id rows, the restore)
    for w in c_tick:
        assert c_loop[w] >= c_tick[w], (w, c_loop, c_tick)
    assert sum(c_loop.values()) >= sum(c_tick.values())
