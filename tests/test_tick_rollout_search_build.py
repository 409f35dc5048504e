"""Build-time checks of the neighbour search of the multi-tick TagContinuous entry (HipTagContinuousRollout_K10_N105A21):
wavefront 1 splits its chain over the two halves of its lanes while 65 .. 96 agents are in the game (tc_fast.h "LANE
HALVES"), so the loop body holds the exchange between the lane halves -- one v_permlane32_swap per key -- and still ONE
chain and ONE merge network, which the split over the wavefronts and the split over the lane halves share; the entry keeps
its resources and its store sites.  Read off the disassembly with the helpers of tests/test_tick_rollout_build.py; no GPU
needed.

The search span = the loop body from its first `v_med3_u32` (the chain) to the first global store behind its last one (the
id row of the searcher, stored from registers).  Its ceiling is what the finished build shows (docs/rounds/r38.md).  The
change adds the exchange to the span and takes nothing measurable out of it (the three sub-items of the search tail were
found done by the compiler in the parent's object already: docs/rounds/r38.md, section 3), so no ceiling here is below the
parent's count; what fails on the parent's object is the exchange itself."""
import os
import re
import subprocess
from collections import Counter

from tests.test_tick_rollout_build import ROLLOUT, UNIT, _body, _elf, built  # noqa: F401  (`built`: the module's fixture)
from tests.test_tick_rollout_carry_build import _loop_body

L_KEYS = 12                       # self + K = 10 others + one look-ahead entry
PARENT_LOOP_BODY = 4154           # static instructions of the parent's object (commit 6c63a1c), counted as below
PARENT_SEARCH_SPAN = 1869
LOOP_BODY_FENCE = 4260            # the standing fence (tests/test_tick_rollout_gather_build.py)
LOOP_BODY_MAX = 4228              # ceilings: the finished build
SEARCH_SPAN_MAX = 1894
CHAIN_MED3 = 143                  # 11 per candidate: two groups of four in the loop, one group behind it, one candidate
MERGE_MAX_U32 = 24                # the bitonic network behind the 12 partner minima keeps 12 of its 16 entries


def _ops(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    body = _loop_body(_body(llvm, elf, ROLLOUT))
    return llvm, elf, [re.sub(r"_e(32|64)$", "", l.split()[0]) for _, l, _, _ in body]


def search_span(ops):
    """(first, last) index into the loop body: the first v_med3_u32 .. the first global store behind the last one"""
    med = [i for i, o in enumerate(ops) if o == "v_med3_u32"]
    assert med, "no chain in the loop body"
    store = next(i for i in range(med[-1], len(ops)) if ops[i].startswith("global_store_"))
    return med[0], store


def test_lane_half_exchange_is_in_the_loop_body(built, tmp_path):
    _, _, ops = _ops(built, tmp_path)
    lo, hi = search_span(ops)
    swaps = [i for i, o in enumerate(ops) if o.startswith("v_permlane32_swap")]
    print(f"v_permlane32_swap in the loop body: {len(swaps)}")
    assert len(swaps) == L_KEYS                     # (the parent's object has none)
    assert all(lo < i < hi for i in swaps)
    # behind the chain, in front of the one block barrier of the search (the split over the wavefronts meets there)
    last_med = max(i for i, o in enumerate(ops) if o == "v_med3_u32")
    assert all(i > last_med for i in swaps)


def test_one_chain_and_one_merge(built, tmp_path):
    _, _, ops = _ops(built, tmp_path)
    lo, hi = search_span(ops)
    c = Counter(ops[lo:hi])
    print(f"search span: v_med3_u32 {c['v_med3_u32']}, v_max_u32 {c['v_max_u32']}, v_min_u32 {c['v_min_u32']}, "
          f"v_min3_u32 {c['v_min3_u32']}, s_barrier {c['s_barrier']}, s_setprio {c['s_setprio']}")
    assert c["v_med3_u32"] == CHAIN_MED3            # the chain is not instantiated a second time for the lane halves
    assert c["v_max_u32"] == MERGE_MAX_U32          # nor is the merge network
    assert c["s_barrier"] == 1 and c["s_setprio"] == 4   # the barriers and the priority schedule are the parent's
    # the gap test of the search tail folds its ten differences with v_min3_u32 (the parent's object did so already)
    assert c["v_min3_u32"] >= 4


def test_search_span_and_loop_body_ceilings(built, tmp_path):
    _, _, ops = _ops(built, tmp_path)
    lo, hi = search_span(ops)
    print(f"loop body: {len(ops)} static instructions (parent {PARENT_LOOP_BODY}, ceiling {LOOP_BODY_MAX}, fence "
          f"{LOOP_BODY_FENCE}); search span: {hi - lo} (parent {PARENT_SEARCH_SPAN}, ceiling {SEARCH_SPAN_MAX})")
    assert LOOP_BODY_MAX <= LOOP_BODY_FENCE
    assert len(ops) <= LOOP_BODY_MAX
    assert hi - lo <= SEARCH_SPAN_MAX
    # what the exchange may cost: an add, a copy and the swap per key, and the votes around it
    assert SEARCH_SPAN_MAX - PARENT_SEARCH_SPAN <= 3 * L_KEYS


def test_resources_and_store_sites(built, tmp_path):
    llvm, elf, ops = _ops(built, tmp_path)
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

    assert TagContinuous(**BENCH_CFG).lds_bytes(1, fused=True, threads=128) == 20468
    sites = {w: sum(1 for o in ops if o == f"global_store_{w}") for w in ("dword", "dwordx2", "dwordx4")}
    assert sites == {"dword": 36, "dwordx2": 2, "dwordx4": 14}, sites
    assert sum(1 for o in ops if o.startswith("global_load_lds")) == 22
