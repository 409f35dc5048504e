"""Build-time checks of the steady-state trip of the multi-tick TagContinuous entry (HipTagContinuousRollout_K10_N105A21):
a thread carries its state in registers from trip to trip, so a trip that neither starts a launch nor follows a restore
loads nothing but the two probability slabs, and the Philox rounds run between the slab issue and the slab wait.  Read off
the disassembly of the code object; no GPU needed.

How the disassembly is read.  The outermost loop is the longest backward branch of the kernel (as in
tests/test_tick_rollout_build.py); its body is every instruction from the branch target to the branch, in address order.
"The fall-through path" is that address order: the slab issue is a run of short exec-mask skips (`s_cbranch_execz` over one
global_load_lds each) and two small loops, all of which rejoin the straight line, so the instructions between the first /
last `global_load_lds` and the first `s_waitcnt` that names vmcnt after them are what a wavefront walks through.
"Behind a branch", in two parts.  (a) Every non-LDS global load of the loop body sits in a block that a WAVE-UNIFORM forward
branch (`s_branch`, `s_cbranch_scc*`, `s_cbranch_vcc*`; not an exec-mask skip, which every trip walks through) in front of
it jumps over: the reload (trip 0, the trip after a restore) in front of the slab issue, the restore behind it.  That alone
says little behind the slab issue: the trip's early-out (`env0 >= a.E`, in front of the slab issue) and the long
block-uniform branches of the search span most of the trip.  So (b) the loads BEHIND the slab issue must all lie in the one
block that the restore is: there is a wave-uniform forward branch G in front of the first of them, with its target beyond the
last of them, such that
  * no global store lies between G and the first load -- every phase of the tick stores (`done = 0` in front of the slab
    issue, the actions behind the slab wait, state in the move, rewards at the end), so G cannot be the early-out or a branch
    of an earlier phase: a state or key load put back behind the slab wait, in the sampling, the move or the rewards, has
    a store between any branch that spans it together with the restore's loads and itself; and
  * G follows a block barrier closely (at most 24 instructions, none of them a global access or an LDS write): it is the
    branch on the `doneflag` votes right behind the barrier that publishes them.
`_steady_state_violations` returns what it finds wrong, so that the check can be pointed at another disassembly: a build
with `in.x = a.loc_x[gi]` put back into the move phase gives "no restore guard" (docs/rounds/r21.md).
It cannot tell WHICH condition a branch tests; that the reload is taken exactly when it has to be is what
tests/test_gpu_tick_rollout_carry.py checks."""
import re
import subprocess
import os

from tests.test_tick_rollout_build import ROLLOUT, UNIT, _body, _elf, built  # noqa: F401  (`built`: the module's fixture)

_ADDR = re.compile(r"//\s*([0-9A-Fa-f]+):")
_BRANCH = re.compile(r"\b(s_cbranch_\w+|s_branch)\s+\d+\s+//.*<" + ROLLOUT + r"\+0x([0-9a-f]+)>")


def _loop_body(text):
    """[(address, instruction text, branch mnemonic or None, branch target or None)] of the outermost loop, in address order"""
    rows = []
    for l in text.splitlines():
        m = _ADDR.search(l)
        if m:
            rows.append((int(m.group(1), 16), l.strip()))
    base = rows[0][0]
    ins = []
    for a, l in rows:
        b = _BRANCH.search(l)
        ins.append((a, l, b.group(1) if b else None, base + int(b.group(2), 16) if b else None))
    spans = [(a - t, t, a) for a, _, b, t in ins if b and t < a]
    assert spans, "no backward branch: the entry has no loop"
    _, lo, hi = max(spans)
    return [i for i in ins if lo <= i[0] <= hi]


def _op(l):
    return l.split()[0]


def test_steady_state_trip_loads_only_the_slabs(built, tmp_path):
    llvm, elf = _elf(built, UNIT, tmp_path)
    body = _loop_body(_body(llvm, elf, ROLLOUT))
    ops = [_op(l) for _, l, _, _ in body]
    lds = [i for i, o in enumerate(ops) if o.startswith("global_load_lds")]
    assert lds, "the loop body fetches no slab"
    first, last = lds[0], lds[-1]
    wait = next(i for i in range(last + 1, len(body)) if ops[i] == "s_waitcnt" and "vmcnt" in body[i][1])
    # the Philox rounds (two v_mul_hi_u32 each) run between the slab issue and the slab wait
    assert sum(o == "v_mul_hi_u32" for o in ops[last + 1:wait]) >= 10
    # ... and nothing else that touches memory: no other wait on vmcnt (`wait` is the first), no non-LDS load, no LDS access,
    # no store (its acknowledgement would be waited for in order with the slabs)
    between = ops[first + 1:wait]
    assert not any(o == "s_waitcnt" and "vmcnt" in body[first + 1 + i][1] for i, o in enumerate(between))
    assert not [o for o in between if o.startswith("global_load_") and not o.startswith("global_load_lds")]
    assert not [o for o in between if o.startswith("ds_")]
    assert not [o for o in between if o.startswith("global_store") or o.startswith("flat_") or o.startswith("buffer_")]
    assert _steady_state_violations(body) == []
    assert not [o for o in ops if o.startswith("flat_load") or o.startswith("buffer_load")]


def _steady_state_violations(body):
    """parts (a) and (b) of the module docstring on one loop body; [] if nothing is wrong"""
    ops = [_op(l) for _, l, _, _ in body]
    bad = []
    first = next(i for i, o in enumerate(ops) if o.startswith("global_load_lds"))
    is_uniform = lambda b: b == "s_branch" or b.startswith("s_cbranch_scc") or b.startswith("s_cbranch_vcc")
    uniform = [(i, a, t) for i, (a, _, b, t) in enumerate(body) if b and is_uniform(b) and t > a]
    loads = [(i, a, l) for i, (a, l, _, _) in enumerate(body)
             if re.match(r"global_load_(dword|ubyte|sbyte|ushort|sshort|short)", l)]
    if not loads:
        bad.append("the reload path is gone: trip 0 must read its state from memory")
    for _, a, l in loads:  # (a)
        if not any(b < a < t for _, b, t in uniform):
            bad.append(f"on the steady-state path: {l}")
    before = [x for x in loads if x[0] < first]
    after = [x for x in loads if x[0] > first]
    if len(before) < 13:  # the state arrays, the RNG word, the time step and runner count
        bad.append(f"only {len(before)} loads on the reload path")
    if not after:
        bad.append("no load of the restore's copy loop behind the slab issue")
        return bad
    lo, hi = after[0], after[-1]  # (b)
    guards = []
    for gi, ga, gt in uniform:
        if not (ga < lo[1] and gt > hi[1]):
            continue
        if any(o.startswith("global_store") for o in ops[gi:lo[0]]):
            continue
        back = ops[max(0, gi - 24):gi]
        if "s_barrier" not in back:
            continue
        tail = back[len(back) - back[::-1].index("s_barrier"):]
        if any(o.startswith("global_") or o.startswith("ds_write") or o.startswith("ds_add") for o in tail):
            continue
        guards.append(ga)
    if not guards:
        bad.append(f"no restore guard: loads behind the slab issue from {lo[2]} to {hi[2]} are not all inside the block "
                   "behind the doneflag barrier")
    return bad


def test_carried_rollout_keeps_its_resources(built, tmp_path):
    """as tests/test_tick_rollout_build.py asserts them: at most 128 VGPRs, no spill, no scratch, no AGPR"""
    llvm, elf = _elf(built, UNIT, tmp_path)
    notes = subprocess.run([os.path.join(llvm, "llvm-readelf"), "--notes", elf], check=True, capture_output=True,
                           text=True).stdout
    field = lambda k: int(re.search(rf"\.{k}:\s+(\d+)", notes).group(1))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0
    assert field("vgpr_count") <= 128
    assert field("agpr_count") == 0
    assert "scratch_" not in _body(llvm, elf, ROLLOUT)
