"""Build-time checks of the phase-scoped argument views of the multi-tick TagContinuous entry
(HipTagContinuousRollout_K10_N105A21; csrc/kernels/tc_kernarg.h).  No GPU needed: hipcc cross-compiles gfx950.

The loop of the entry no longer keeps its ~45 pointer arguments alive from trip to trip (they did not fit the scalar
register file: the parent commit's object parks 97 scalar values in lanes of a vector register and reads them back with 174
`v_readlane_b32` in the loop body -- VALU instructions, on the unit the kernel saturates).  Every phase of a trip reads the
pointers it needs from the kernel-argument segment with scalar loads, through `TcRolloutKernarg`, a struct that mirrors
the segment field for field.  Checked here:

  * the mirror IS the segment: offset and size of every field, from a host build of the header, equal the `.args` record
    of the compiled entry (a wrong field would read another array's pointer; tests/test_gpu_tick_rollout_kernarg.py is
    built to show that on the device);
  * what the parent's object had is gone: `.sgpr_spill_count` (parent 97; the issue's target is 0, the bound a quarter of the
    parent's; the ceiling is what this build shows: 3 -- one launch constant and the 64-bit mask `wave == 0`, which the
    compiler shares between the slab issue and the row gather), the lane reads and writes of the loop body (parent 174 and
    8), its length (parent 4228);
  * the lane reads that remain are located: a read of the compiler's own has a CONSTANT lane (the slot the value was parked
    in); a read the source asks for (`__builtin_amdgcn_readlane`, SOURCE_READLANES below) selects the lane with a scalar
    register.  All of the latter must be accounted for by the source's calls;
  * scalar loads off the kernel-argument pointer inside the loop body; no flat, buffer or scratch access; at most 128 VGPRs,
    no AGPR.

Every count check below fails on the parent's object (PARENT holds its figures)."""
import os
import re
import subprocess

from tests.test_tick_rollout_build import ROLLOUT, UNIT, _body, _elf, built  # noqa: F401  (`built`: the module's fixture)
from tests.test_tick_rollout_carry_build import _loop_body, _op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KDIR = os.path.join(ROOT, "warp_drive_amd", "csrc", "kernels")

PARENT = {"sgpr_spill_count": 97, "v_readlane_b32": 174, "v_writelane_b32": 8, "loop_body": 4228}
SGPR_SPILL_CEILING = 3      # as built; the issue's bound: at most a quarter of the parent's count
PARKED_READS_CEILING = 3    # v_readlane_b32 with a constant lane inside the loop body, as built
PARKED_WRITES_CEILING = 2   # v_writelane_b32 inside the loop body, as built (the two halves of `wave == 0`, once per trip)
assert SGPR_SPILL_CEILING * 4 <= PARENT["sgpr_spill_count"]

# the calls of __builtin_amdgcn_readlane that the LOOP instantiation of tc_fast_impl compiles (tc_fast.h; the other calls of
# the file sit behind `if constexpr (PRE)` / `cells_C`, replicas of more than 128 agents): the whole-wavefront resolution of
# a near-tie at the cut hands the lane's searcher to every lane
SOURCE_READLANES = ("__builtin_amdgcn_readlane(__builtin_bit_cast(int, mx), fl)",
                    "__builtin_amdgcn_readlane(__builtin_bit_cast(int, my), fl)",
                    "__builtin_amdgcn_readlane((int)zone_hi, fl)",
                    "__builtin_amdgcn_readlane(ag, fl)")

_PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include "tc_kernarg.h"
#define SHOW(type, name) std::printf("%s %zu %zu\n", #name, offsetof(TcRolloutKernarg, name), sizeof(((TcRolloutKernarg *)0)->name));
int main() {
  WD_TC_PARAM_LIST(SHOW, WD_TC_NOTHING)
  WD_TC_FUSE_PARAM_LIST(SHOW, WD_TC_NOTHING)
  WD_TC_ROLLOUT_PARAM_LIST(SHOW, WD_TC_NOTHING)
  std::printf("sizeof %zu\n", sizeof(TcRolloutKernarg));
  return 0;
}
"""


def _mirror_layout(tmp_path):
    """[(field, offset, size)] of TcRolloutKernarg and its size, from a host build of the header"""
    src, exe = tmp_path / "kernarg_layout.cpp", tmp_path / "kernarg_layout"
    src.write_text(_PROGRAM)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", f"-I{KDIR}", str(src), "-o", str(exe)], check=True)
    rows = [l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert rows[-1][0] == "sizeof"
    return [(n, int(o), int(s)) for n, o, s in rows[:-1]], int(rows[-1][1])


def _notes(llvm, elf):
    return subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                          text=True).stdout


def _entry_args(notes):
    """[(offset, size, value_kind)] of the `.args` record of the one kernel of the object"""
    block = notes[notes.index(".args:"):]
    block = block[:block.index(".group_segment_fixed_size")]
    out = []
    for item in re.split(r"\n\s+- ", block)[1:]:
        field = lambda k: re.search(rf"\.{k}:\s+(\S+)", item).group(1)
        out.append((int(field("offset")), int(field("size")), field("value_kind")))
    return out


def test_mirror_struct_is_the_kernarg_segment(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    args = _entry_args(_notes(llvm, elf))
    explicit = [a for a in args if not a[2].startswith("hidden_")]
    fields, size = _mirror_layout(tmp_path)
    assert len(fields) == len(explicit) == 46
    for (name, off, sz), (a_off, a_sz, kind) in zip(fields, explicit):
        assert (off, sz) == (a_off, a_sz), (name, off, sz, a_off, a_sz)
        assert (kind == "global_buffer") == (sz == 8), (name, kind)   # every pointer of the list is one of the segment
    assert fields[0] == ("loc_x_arr", 0, 8) and fields[-1][0] == "kNumTicks"
    hidden = [a for a in args if a[2].startswith("hidden_")]
    assert not hidden or min(a[0] for a in hidden) >= fields[-1][1] + fields[-1][2]
    assert size >= fields[-1][1] + fields[-1][2]
    # the host's launch tuple is what it was: as many arguments as the segment has fields
    from warp_drive_amd.envs.tag_continuous import TagContinuous

    assert len(TagContinuous._STEP_ARGS) + 1 + 6 + 1 == len(fields)   # + kEnvBegin, the fused tick's six, the ticks


def test_nothing_is_parked_in_lanes(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    notes = _notes(llvm, elf)
    field = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", notes).group(1))
    print("sgpr_spill_count", field("sgpr_spill_count"), "sgpr_count", field("sgpr_count"), "vgpr_count", field("vgpr_count"))
    assert field("sgpr_spill_count") <= SGPR_SPILL_CEILING < PARENT["sgpr_spill_count"]
    assert field("vgpr_spill_count") == 0 and field("private_segment_fixed_size") == 0
    assert field("vgpr_count") <= 128 and field("agpr_count") == 0
    body = _loop_body(_body(llvm, elf, ROLLOUT))
    text = [l for _, l, _, _ in body]
    reads = [l for l in text if _op(l) == "v_readlane_b32"]
    writes = [l for l in text if _op(l) == "v_writelane_b32"]
    # `v_readlane_b32 s8, v102, 1`: a parked value comes back from its slot; `v_readlane_b32 s26, v28, s24`: the source's
    lane = lambda l: l.split("//")[0].split(",")[-1].strip()
    parked = [l for l in reads if re.fullmatch(r"\d+", lane(l))]
    asked = [l for l in reads if re.fullmatch(r"s\d+|m0|vcc_lo|vcc_hi", lane(l))]
    print(f"loop body: {len(body)} instructions, {len(reads)} v_readlane_b32 ({len(parked)} parked, {len(asked)} asked for), "
          f"{len(writes)} v_writelane_b32")
    for l in parked + writes:
        print("   ", l.split("//")[0].strip())
    assert len(parked) + len(asked) == len(reads)
    assert len(parked) <= PARKED_READS_CEILING and len(writes) <= PARKED_WRITES_CEILING
    assert len(reads) < PARENT["v_readlane_b32"] and len(writes) < PARENT["v_writelane_b32"]
    # every other read is one the source asks for: its calls are there, and there is one instruction per call
    src = open(os.path.join(KDIR, "tc_fast.h")).read()
    for call in SOURCE_READLANES:
        assert src.count(call) == 1, call
    assert len(asked) == len(SOURCE_READLANES)
    # the parked slots live in ONE vector register, and nothing else reads or writes lanes of it
    regs = {l.split("//")[0].split(",")[1].strip() for l in parked} | {_ops(l)[0] for l in writes}
    assert len(regs) <= 1, regs
    assert len(body) < PARENT["loop_body"]


def _ops(l):
    return [o.strip() for o in l.split("//")[0].split(None, 1)[1].split(",")]


def test_views_are_scalar_loads_inside_the_loop(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    whole = _body(llvm, elf, ROLLOUT)
    body = _loop_body(whole)
    text = [l for _, l, _, _ in body]
    loads = [l for l in text if _op(l).startswith("s_load_dword")]
    # the kernel-argument pointer arrives in s[0:1]; a view is a copy of it (`s_mov_b64 s[6:7], s[0:1]`: the opaque asm)
    views = {_ops(l)[0] for l in text if _op(l) == "s_mov_b64" and _ops(l)[1] == "s[0:1]"}
    assert len([l for l in text if _op(l) == "s_mov_b64" and _ops(l)[1] == "s[0:1]"]) >= 8   # one per phase
    through_views = [l for l in loads if _ops(l)[1] in views]
    pointers = [l for l in through_views if _op(l) in ("s_load_dwordx2", "s_load_dwordx4", "s_load_dwordx8")]
    print(f"{len(loads)} scalar loads in the loop body, {len(through_views)} through a view, {len(pointers)} of 8 bytes or more")
    assert len(pointers) >= 20
    # ... and nothing else changed kind: no flat, buffer or scratch access anywhere in the kernel
    ops = [l.split()[0] for l in whole.splitlines() if re.search(r"//\s*[0-9A-Fa-f]+:", l)]
    assert not [o for o in ops if o.startswith(("flat_", "buffer_", "scratch_"))]
    # the slab window holds no wait on lgkmcnt merged with a vmcnt count (tests/test_tick_rollout_carry_build.py checks
    # the window itself): the views' waits are in front of the first piece or behind the slab wait
    o = [_op(l) for l in text]
    first = next(i for i, x in enumerate(o) if x.startswith("global_load_lds"))
    last = max(i for i, x in enumerate(o) if x.startswith("global_load_lds"))
    wait = next(i for i in range(last + 1, len(o)) if o[i] == "s_waitcnt" and "vmcnt" in text[i])
    assert not [text[i] for i in range(first + 1, wait) if o[i] == "s_waitcnt" and "vmcnt" in text[i]]
