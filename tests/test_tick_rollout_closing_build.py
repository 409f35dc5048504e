"""Build-time checks of the closing trips of the multi-tick TagContinuous entry (HipTagContinuousRollout_K10_N105A21): the
state a thread carries in registers (position, speed, heading, acceleration, the edge penalty, the RNG epoch word; from lane
0 the time step and the runner count) is stored on the last trip of a launch and on the trip a replica's episode ends on,
not on every trip (tc_store_carried, tc_fast.h).  Read off the disassembly with the helpers of
tests/test_tick_rollout_build.py and tests/test_tick_rollout_carry_build.py; no GPU needed.

How the disassembly is read.  The loop body in address order, as in the carry test.  Its landmarks: the slab wait (the first
`s_waitcnt` that names vmcnt behind the last `global_load_lds`), the block barrier behind it (tables published: the sampling
lies in between) and the next block barrier (the move lies in between).  The closing block is the one stretch of the body
that a WAVE-UNIFORM forward branch (`s_cbranch_scc*`, `s_cbranch_vcc*`: not an exec-mask skip, which every trip walks
through) jumps over and that holds at least seven single-dword stores, no wider store and no block barrier.  Counts are
"as built"; on the parent's object the sampling holds the epoch store, the move eight single-dword stores, there is no
closing block and the body has 55 `v_lshl_add_u64`.
It cannot tell WHICH condition the branch tests; that the block is taken exactly when it has to be is what
tests/test_gpu_tick_rollout_closing.py checks."""
import re

from tests.test_tick_rollout_build import ROLLOUT, UNIT, _body, _elf, built  # noqa: F401  (`built`: the module's fixture)
from tests.test_tick_rollout_carry_build import _loop_body, _op, _steady_state_violations

PARENT_LSHL_ADD_U64 = 55   # in the loop body before this change
LSHL_ADD_U64_MAX = 46      # as built
CLOSING_STORES = 9         # six [E, N] arrays, the epoch word, the time step, the runner count
MOVE_STORES_MAX = 1        # obs_rows_cleared, change-only (the parent: eight)


def _uniform(b):
    return b is not None and (b.startswith("s_cbranch_scc") or b.startswith("s_cbranch_vcc"))


def _read(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    body = _loop_body(_body(llvm, elf, ROLLOUT))
    return body, [_op(l) for _, l, _, _ in body]


def _closing_blocks(body, ops):
    """[(index of the branch, index of the first instruction behind the block)] of every wave-uniform forward branch whose
    skipped stretch holds at least seven single-dword stores, no store of another width (the row flush has both) and no
    block barrier"""
    at = {a: i for i, (a, _, _, _) in enumerate(body)}
    found = []
    for i, (a, _, b, t) in enumerate(body):
        if not (_uniform(b) and t > a and t in at):
            continue
        inside = ops[i + 1:at[t]]
        wider = [o for o in inside if o.startswith("global_store_") and o != "global_store_dword"]
        if inside.count("global_store_dword") >= 7 and "s_barrier" not in inside and not wider:
            found.append((i, at[t]))
    return found


def test_steady_path_no_longer_stores_the_carried_state(built, tmp_path):
    body, ops = _read(built, tmp_path)
    last = max(i for i, o in enumerate(ops) if o.startswith("global_load_lds"))
    wait = next(i for i in range(last + 1, len(ops)) if ops[i] == "s_waitcnt" and "vmcnt" in body[i][1])
    b1 = next(i for i in range(wait, len(ops)) if ops[i] == "s_barrier")
    b2 = next(i for i in range(b1 + 1, len(ops)) if ops[i] == "s_barrier")
    sampling, move = ops[wait:b1], ops[b1:b2]
    # behind the slab wait: the actions (one 8-byte store) and no epoch word
    assert sampling.count("global_store_dwordx2") == 1
    assert sampling.count("global_store_dword") == 0, [body[wait + i][1] for i, o in enumerate(sampling) if o.startswith("global_store")]
    # the move (the phase that ends with the float64 products of tc_div_const): position, speed, heading, acceleration, edge
    # penalty and time step are not stored in it
    assert move.count("v_fma_f64") >= 4
    print(f"single-dword stores in the move span: {move.count('global_store_dword')} (parent: 8)")
    assert move.count("global_store_dword") <= MOVE_STORES_MAX
    assert not [o for o in move if o.startswith("global_store_dwordx")]


def test_closing_block_in_the_rewards_phase(built, tmp_path):
    body, ops = _read(built, tmp_path)
    blocks = _closing_blocks(body, ops)
    assert len(blocks) == 1, [body[g][1] for g, _ in blocks]
    g, end = blocks[0]
    inside = [body[i][1] for i in range(g + 1, end)]
    stores = [l for l in inside if _op(l).startswith("global_store")]
    print(f"closing block: {end - g - 1} instructions, {len(stores)} stores")
    assert len(stores) == CLOSING_STORES and all(_op(l) == "global_store_dword" for l in stores)
    # every one of them off a scalar base with a 32-bit vector offset: no 64-bit vector address is formed in the block
    assert all(re.search(r"global_store_dword v\d+, v\d+, s\[\d+:\d+\]", l) for l in stores), stores
    assert not [l for l in inside if _op(l) in ("v_lshl_add_u64", "v_lshlrev_b64", "v_ashrrev_i32_e32")]
    # its pointers come from a view of its own, inside the block: a trip that does not close loads none of them
    assert sum(_op(l).startswith("s_load_dword") for l in inside) >= 4
    # no vector load, no LDS write, no barrier, nothing that waits for memory
    assert not [l for l in inside if _op(l).startswith("global_load") or _op(l).startswith("ds_write")]
    assert not [l for l in inside if _op(l) == "s_waitcnt" and "vmcnt" in l]
    # where it lies: behind the barrier that follows the row flush (every 16-byte store of the trip is in front of it), in
    # front of the `doneflag` barrier, with no barrier in between; the restore and its guard follow that barrier
    barriers = [i for i, o in enumerate(ops) if o == "s_barrier"]
    before = max(i for i in barriers if i < g)
    assert not [i for i in range(before, len(ops)) if ops[i] == "global_store_dwordx4" and "sc1" in body[i][1]]
    after = min(i for i in barriers if i > end - 1)
    assert not [i for i in barriers if g < i < after]
    loads = [i for i, (_, l, _, _) in enumerate(body) if re.match(r"global_load_(dword|ubyte|sbyte|ushort|sshort|short)", l)]
    assert [i for i in loads if i > after], "the restore's copy loop is not behind the doneflag barrier"
    assert not [i for i in loads if before < i < after]
    assert _steady_state_violations(body) == []


def test_fewer_64_bit_address_formations_than_the_parent(built, tmp_path):
    body, ops = _read(built, tmp_path)
    n = ops.count("v_lshl_add_u64")
    print(f"v_lshl_add_u64 in the loop body: {n} (parent: {PARENT_LSHL_ADD_U64})")
    assert n <= LSHL_ADD_U64_MAX < PARENT_LSHL_ADD_U64
    # the stores moved, they did not vanish or multiply: the sites of the body are what they were
    sites = {w: ops.count(f"global_store_{w}") for w in ("dword", "dwordx2", "dwordx4")}
    assert sites == {"dword": 36, "dwordx2": 2, "dwordx4": 14}, sites
    (g, end), = _closing_blocks(body, ops)
    assert ops.count("global_store_dword") - ops[g + 1:end].count("global_store_dword") == 36 - CLOSING_STORES
    assert not [o for o in ops if o.startswith("flat_") or o.startswith("buffer_") or o.startswith("scratch_")]
