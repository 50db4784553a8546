"""CPU tests of nexrReduceCopyLL128StepsGroup (include/nexr.h) and of nexrRingCommSetLLGroup on LL128
communicators (include/nexr_ring.h): every rejection happens before any device call, so the return codes
are checked here without a GPU — the argument checks (4, nexrInvalidArgument), the workspace that holds too
few launches (4), the host dry run (5, nexrInvalidUsage) and the residency refusal through the library's
test hook (5). The host planner is the LL group call's; what differs for LL128 is checked: slots of whole
2 KiB slices, 1920 data bytes per slice, no flag rule."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

from conftest import ROOT

F32, U8 = 7, 1
SLOT = 1 << 16                       # 32 slices: G = 16 workgroups a member
CAP = SLOT // 2048 * 1920            # data bytes a step may fill
X_FIFO, X_HEAD = 0x100000, 0x100000 + 8 * SLOT   # made-up device addresses: nothing here reaches the device
Y_FIFO, Y_HEAD = 0x300000, 0x300000 + 8 * SLOT
WS = 0x800000


def _call(nexr, members, dt=F32, op=0, arg=0, ws=WS, ws_bytes=None, slot=SLOT, n_members=None, null=None, n_slots=8):
    """members: (recv, send, steps) per member, recv / send as (fifo, head, step) lists. Returns the code."""
    L = nexr.lib()
    n = len(members) if n_members is None else n_members
    sets = [nexr.ll_conn_set(0x10000 * (m + 1), 0x20000000 + 0x10000 * m, r, s, slot[m] if isinstance(slot, list)
                             else slot, n_slots) for m, (r, s, _steps) in enumerate(members)]
    cs = (nexr.LLConnSet * max(1, len(sets)))(*sets)
    arrs = [(nexr.LLStep * max(1, len(st)))(*st) for _r, _s, st in members]
    ptrs = (ctypes.POINTER(nexr.LLStep) * max(1, len(arrs)))(*[ctypes.cast(a, ctypes.POINTER(nexr.LLStep))
                                                               for a in arrs])
    counts = (ctypes.c_int * max(1, len(members)))(*[len(st) for _r, _s, st in members])
    if ws_bytes is None:
        ws_bytes = nexr.ll_group_workspace_bytes(max(1, min(n, 32)))
    return L.nexrReduceCopyLL128StepsGroup(n, None if null == "conns" else cs, None if null == "steps" else ptrs,
                                           None if null == "counts" else counts, dt, op, arg, None, 0,
                                           ctypes.c_void_p(ws) if ws else None, ws_bytes, None)


def _pair(nexr, per=CAP // 4):
    """Member 0 sends on X, member 1 receives on X: a valid two-member group of one step each."""
    return [([], [(X_FIFO, X_HEAD, 0)], [nexr.ll_step(0, 0, -1, 0, per, send=True)]),
            ([(X_FIFO, X_HEAD, 0)], [], [nexr.ll_step(0, 0, 1, 0, per, recv=True)])]


def test_the_symbol_is_declared_exported_and_wrapped(nexr):
    hdr = open(os.path.join(ROOT, "include", "nexr.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", nexr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    name = "nexrReduceCopyLL128StepsGroup"
    assert re.search(r"NEXR_API\s+nexrResult_t\s+" + name + r"\s*\(", hdr)
    assert name in exported and name in nexr.ABI_SYMBOLS
    assert callable(nexr.reduce_copy_ll128_steps_group)
    assert nexr.version() == 300                       # additions only
    ring = importlib.import_module("nex-nccl_amd.ring")
    assert "nexrRingCommSetLLGroup" in ring.RING_ABI_SYMBOLS and hasattr(ring.ring_lib(), "nexrRingCommSetLLGroup")


def test_the_structs_are_the_ll_calls(nexr):
    """nexrLLConnSet and nexrLLStep are reused unchanged, and one workspace size serves both group calls."""
    assert ctypes.sizeof(nexr.LLStep) == 32 and ctypes.sizeof(nexr.LLConnSet) == 184
    assert nexr.LLConnSet.slotBytes.offset == 168 and nexr.LLConnSet.nSlots.offset == 176
    hdr = open(os.path.join(ROOT, "include", "nexr.h")).read()
    assert len(re.findall(r"\}\s*nexrLLConnSet\s*;", hdr)) == 1 and len(re.findall(r"\}\s*nexrLLStep\s*;", hdr)) == 1
    assert "nexrLL128" not in hdr.replace("nexrLL128StepsGroup", "")   # no LL128-only struct or size query


def test_bad_arguments_fail_before_the_device(nexr):
    pair = _pair(nexr)
    assert _call(nexr, pair, ws_bytes=8) == 4                            # valid so far: only the workspace is short
    assert _call(nexr, pair, n_members=0) == 4
    one = ([], [], [nexr.ll_step(0, 0, 1, 0, 100)])
    assert _call(nexr, [one] * 33) == 4                                  # > NEXR_LL_GROUP_MAX_MEMBERS
    for null in ("conns", "steps", "counts"):
        assert _call(nexr, pair, null=null) == 4
    # slotBytes: whole 2 KiB slices (a 16-byte multiple is not enough here)
    for bad in (0, 16, 2048 + 16, 4096 + 1024, SLOT - 16):
        assert _call(nexr, pair, slot=bad) == 4, bad
    assert _call(nexr, _pair(nexr, 1920 // 4), slot=2048, ws_bytes=8) == 4  # 2048 passes: the workspace's 4 ...
    assert _call(nexr, [([], [], [])] * 2, slot=2048, ws=0) == 0            # ... as empty lists show
    assert _call(nexr, [([], [], [])] * 2, slot=2048 + 16, ws=0) == 4
    # a step larger than a slot: 1920 data bytes per slice, not 2048 and not half the slot
    assert _call(nexr, _pair(nexr, CAP // 4 + 1)) == 4                   # (CAP // 4 is the valid pair above)
    assert _call(nexr, _pair(nexr, CAP + 1), dt=U8) == 4
    assert _call(nexr, _pair(nexr, 1921), dt=U8, slot=2048) == 4
    # nSlots
    assert _call(nexr, pair, n_slots=0) == 4
    empty = [(r, s, []) for r, s, _st in pair]
    assert _call(nexr, empty, n_slots=0x80000000, ws=0) == 4             # above INT_MAX
    assert _call(nexr, empty, n_slots=0x7FFFFFFF, ws=0) == 0
    # datatypes and ops nexrReduceCopyLL128 refuses
    assert _call(nexr, pair, dt=10) == 4 and _call(nexr, pair, dt=11) == 4   # fp8
    assert _call(nexr, pair, dt=12) == 4 and _call(nexr, pair, dt=-1) == 4
    assert _call(nexr, pair, op=5) == 4 and _call(nexr, pair, op=-1) == 4
    assert _call(nexr, pair, dt=F32, op=4) == 4                          # SumPostDiv on a float
    assert _call(nexr, _pair(nexr, 64), dt=0, op=4, arg=(256 << 1) | 1) == 4  # int8 divisor that wraps to 0
    # unequal slotBytes / nSlots across members: one G and one credit window serve the launch
    assert _call(nexr, pair, slot=[SLOT, SLOT // 2]) == 4
    L = nexr.lib()
    sets = (nexr.LLConnSet * 2)(nexr.ll_conn_set(0x10000, 0x20000, [], [(X_FIFO, X_HEAD, 0)], SLOT, 8),
                                nexr.ll_conn_set(0x30000, 0x40000, [(X_FIFO, X_HEAD, 0)], [], SLOT, 4))
    arrs = [(nexr.LLStep * 1)(st[0]) for _r, _s, st in pair]
    ptrs = (ctypes.POINTER(nexr.LLStep) * 2)(*[ctypes.cast(a, ctypes.POINTER(nexr.LLStep)) for a in arrs])
    assert L.nexrReduceCopyLL128StepsGroup(2, sets, ptrs, (ctypes.c_int * 2)(1, 1), F32, 0, 0, None, 0,
                                           ctypes.c_void_p(WS), 1 << 20, None) == 4
    # misaligned FIFO of a later member, workspace missing or misaligned
    bad = [pair[0], ([(X_FIFO + 8, X_HEAD, 0)], [], pair[1][2])]
    assert _call(nexr, bad) == 4
    assert _call(nexr, pair, ws=0) == 4
    assert _call(nexr, pair, ws=WS + 4) == 4


def test_a_workspace_that_holds_too_few_launches(nexr):
    region = nexr.ll_group_workspace_bytes(2, 1)
    long = [([], [(X_FIFO, X_HEAD, 0)], [nexr.ll_step(0, 0, -1, 0, 64, send=True)] * 97),
            ([(X_FIFO, X_HEAD, 0)], [], [nexr.ll_step(0, 0, 1, 0, 64, recv=True)] * 97)]
    assert _call(nexr, long, ws_bytes=region) == 4          # 97 steps are two launches
    assert _call(nexr, long, ws_bytes=2 * region - 8) == 4
    assert _call(nexr, _pair(nexr), ws_bytes=region - 8) == 4
    assert _call(nexr, _pair(nexr), ws_bytes=0) == 4
    # a user-range conflict cuts as well: the second step writes bytes the first wrote, one element on
    overlap = [([], [(X_FIFO, X_HEAD, 0)], [nexr.ll_step(0, 0, -1, 0, 64, send=True)] * 2),
               ([(X_FIFO, X_HEAD, 0)], [], [nexr.ll_step(-1, 0, 1, 0, 64, recv=True),
                                            nexr.ll_step(-1, 0, 1, 1, 64, recv=True)])]
    assert _call(nexr, overlap, ws_bytes=region) == 4


def test_empty_groups_are_noops(nexr):
    assert _call(nexr, [([], [(X_FIFO, X_HEAD, 0)], []), ([(X_FIFO, X_HEAD, 0)], [], [])], ws=0, ws_bytes=0) == 0


def _crossed(nexr, order0, order1):
    n = 64
    recv, send = nexr.ll_step(-1, 0, 1, 0, n, recv=True), nexr.ll_step(0, 0, -1, 0, n, send=True)
    steps = {"rs": [recv, send], "sr": [send, recv]}
    return [([(X_FIFO, X_HEAD, 0)], [(Y_FIFO, Y_HEAD, 0)], steps[order0]),
            ([(Y_FIFO, Y_HEAD, 0)], [(X_FIFO, X_HEAD, 0)], steps[order1])]


def test_a_group_that_cannot_finish_is_refused_by_the_dry_run(nexr):
    assert _call(nexr, _crossed(nexr, "rs", "rs")) == 5
    assert _call(nexr, _crossed(nexr, "rs", "rs"), ws_bytes=8) == 5      # before the workspace is looked at
    for o0, o1 in (("sr", "rs"), ("rs", "sr"), ("sr", "sr")):
        assert _call(nexr, _crossed(nexr, o0, o1), ws_bytes=8) == 4, (o0, o1)
    behind = _pair(nexr)
    behind[1] = ([(X_FIFO, X_HEAD, 3)], [], behind[1][2])                # more read than sent
    assert _call(nexr, behind, ws_bytes=8) == 5
    starved = [([], [(X_FIFO, X_HEAD, 0)], [nexr.ll_step(0, 0, -1, 0, 64, send=True)] * 10),
               ([(X_FIFO, X_HEAD, 0)], [], [nexr.ll_step(0, 0, 1, 0, 64, recv=True)])]
    assert _call(nexr, starved, ws_bytes=8) == 5                         # the tenth send has no credit
    starved[0] = (starved[0][0], starved[0][1], starved[0][2][:9])
    assert _call(nexr, starved, ws_bytes=8) == 4
    assert _call(nexr, starved[:1], ws_bytes=8) == 4                     # one-ended: always ready (the run form)


def test_a_grid_that_is_not_resident_at_once_is_refused(nexr, monkeypatch):
    """64 KiB slots are 16 tiles of 4 KiB: two members need 32 workgroups resident, the hook says 31."""
    monkeypatch.setenv("NEXR_TEST_LL_GROUP_RESIDENT", "31")
    assert _call(nexr, _pair(nexr)) == 5
    assert _call(nexr, _pair(nexr), ws_bytes=8) == 4      # the workspace is looked at before the device
    # G comes from slotBytes alone: 2 KiB and 4 KiB slots are one workgroup a member, 12 KiB three
    monkeypatch.setenv("NEXR_TEST_LL_GROUP_RESIDENT", "1")
    assert _call(nexr, _pair(nexr, 16), slot=2048) == 5
    assert _call(nexr, _pair(nexr, 16)[:1], slot=12 << 10) == 5
    monkeypatch.setenv("NEXR_TEST_LL_GROUP_RESIDENT", "127")
    assert _call(nexr, _pair(nexr, 16), slot=1 << 20) == 5              # on the cap of 64 a member


def test_set_ll_group_still_needs_device_memory(nexr, oracle):
    """Host-memory communicators refuse the option, LL128 ones too (the oracle's CPU step functions
    underneath, so no GPU is touched)."""
    ring = importlib.import_module("nex-nccl_amd.ring")
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value
    ll128_fn = ctypes.cast(oracle.lib().oracle_reduce_copy_ll128_fn, ctypes.c_void_p).value
    with ring.RingComm(2, ring.HOST_MEMORY, 8 * 4096, fn, 20000, ring.PROTO_LL128, None, ll128_fn) as comm:
        for on in (True, False):
            with pytest.raises(nexr.NexrError) as e:
                comm.set_ll_group(on)
            assert e.value.code == nexr.Result.InvalidUsage
        assert comm.queued() == 0
