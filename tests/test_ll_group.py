"""CPU tests of nexrReduceCopyLLStepsGroup / nexrLLGroupWorkspaceBytes (include/nexr.h) and of
nexrRingCommSetLLGroup (include/nexr_ring.h): every rejection happens before any device call, so the
return codes are checked here without a GPU — the argument checks (4, nexrInvalidArgument), the workspace
that holds too few launches (4) and the host dry run that refuses a group whose launch could not finish
by itself (5, nexrInvalidUsage)."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

from conftest import ROOT

F32 = 7
SLOT = 1 << 16
# made-up device addresses: nothing here reaches the device
X_FIFO, X_HEAD = 0x100000, 0x100000 + 8 * SLOT
Y_FIFO, Y_HEAD = 0x300000, 0x300000 + 8 * SLOT
WS = 0x800000


def _call(nexr, members, dt=F32, op=0, rule=None, ws=WS, ws_bytes=None, slot=SLOT, n_members=None, null=None,
          n_slots=8):
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
    return L.nexrReduceCopyLLStepsGroup(n, None if null == "conns" else cs, None if null == "steps" else ptrs,
                                        None if null == "counts" else counts, dt, op, 0,
                                        ctypes.byref(nexr.LLFlagRule(*rule)) if rule else None, None, 0,
                                        ctypes.c_void_p(ws) if ws else None, ws_bytes, None)


def _pair(nexr):
    """Member 0 sends on X, member 1 receives on X: a valid two-member group of one step each."""
    per = SLOT // 2 // 4
    return [([], [(X_FIFO, X_HEAD, 0)], [nexr.ll_step(0, 0, -1, 0, per, send=True)]),
            ([(X_FIFO, X_HEAD, 0)], [], [nexr.ll_step(0, 0, 1, 0, per, recv=True)])]


def test_both_symbols_are_declared_and_exported(nexr):
    hdr = open(os.path.join(ROOT, "include", "nexr.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", nexr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("nexrLLGroupWorkspaceBytes", "nexrReduceCopyLLStepsGroup"):
        assert re.search(r"NEXR_API\s+nexrResult_t\s+" + name + r"\s*\(", hdr), name
        assert name in exported and name in nexr.ABI_SYMBOLS
    assert re.search(r"#define\s+NEXR_LL_GROUP_MAX_MEMBERS\s+(\d+)", hdr).group(1) == str(nexr.LL_GROUP_MAX_MEMBERS)
    assert re.search(r"#define\s+NEXR_LL_GROUP_LAUNCHES\s+(\d+)", hdr).group(1) == str(nexr.LL_GROUP_LAUNCHES)
    ring = importlib.import_module("nex-nccl_amd.ring")
    assert "nexrRingCommSetLLGroup" in ring.RING_ABI_SYMBOLS and hasattr(ring.ring_lib(), "nexrRingCommSetLLGroup")
    assert nexr.version() == 300


def test_workspace_bytes_grow_with_the_members(nexr):
    L = nexr.lib()
    b = ctypes.c_size_t(0)
    sizes = []
    for n in range(1, 33):
        assert L.nexrLLGroupWorkspaceBytes(n, ctypes.byref(b)) == 0
        sizes.append(b.value)
    assert sizes[0] > 0 and all(y >= x for x, y in zip(sizes, sizes[1:]))
    assert L.nexrLLGroupWorkspaceBytes(0, ctypes.byref(b)) == 4
    assert L.nexrLLGroupWorkspaceBytes(33, ctypes.byref(b)) == 4
    assert L.nexrLLGroupWorkspaceBytes(2, None) == 4


def test_bad_arguments_fail_before_the_device(nexr):
    pair = _pair(nexr)
    assert _call(nexr, pair, n_members=0) == 4
    one = ([], [], [nexr.ll_step(0, 0, 1, 0, 100)])
    assert _call(nexr, [one] * 33) == 4                                  # > NEXR_LL_GROUP_MAX_MEMBERS
    for null in ("conns", "steps", "counts"):
        assert _call(nexr, pair, null=null) == 4                         # null tables
    assert _call(nexr, pair, slot=[SLOT, SLOT // 2]) == 4                # one G serves the launch
    assert _call(nexr, pair, rule=(0x100, 0x7c)) == 4                    # cleanMask not a multiple of the 8 slots
    assert _call(nexr, pair, rule=(0x60, 0x78)) == 4                     # flagMax not a power of two
    assert _call(nexr, pair, dt=10) == 4                                 # fp8
    assert _call(nexr, pair, dt=F32, op=4) == 4                          # SumPostDiv on a float
    bad = [pair[0], ([(X_FIFO + 8, X_HEAD, 0)], [], pair[1][2])]         # a later member's FIFO misaligned
    assert _call(nexr, bad) == 4
    assert _call(nexr, pair, ws=0) == 4                                  # no workspace
    assert _call(nexr, pair, ws=WS + 4) == 4                             # misaligned workspace
    # nSlots above INT_MAX (the kernels keep it as an int), under a rule that is valid for that many slots
    # (checked with empty step lists, which return 0 once the arguments have passed: the largest int does)
    empty = [(r, s, []) for r, s, _st in pair]
    assert _call(nexr, empty, rule=(0, 0x80000000), n_slots=0x80000000, ws=0) == 4
    assert _call(nexr, pair, rule=(0, 0x80000000), n_slots=0x80000000, ws_bytes=8) == 4
    assert _call(nexr, empty, rule=(0, 0x7FFFFFFF), n_slots=0x7FFFFFFF, ws=0) == 0


def test_a_workspace_that_holds_too_few_launches(nexr):
    """Region per launch = nexrLLGroupWorkspaceBytes / NEXR_LL_GROUP_LAUNCHES. 97 steps are two launches
    (96 per launch): one region is too small; so is anything under one region for a single launch."""
    per = SLOT // 2 // 4
    region = nexr.ll_group_workspace_bytes(2, 1)
    assert region * nexr.LL_GROUP_LAUNCHES == nexr.ll_group_workspace_bytes(2)
    long = [([], [(X_FIFO, X_HEAD, 0)], [nexr.ll_step(0, 0, -1, 0, per, send=True)] * 97),
            ([(X_FIFO, X_HEAD, 0)], [], [nexr.ll_step(0, 0, 1, 0, per, recv=True)] * 97)]
    assert _call(nexr, long, ws_bytes=region) == 4
    assert _call(nexr, long, ws_bytes=2 * region - 8) == 4
    assert _call(nexr, _pair(nexr), ws_bytes=region - 8) == 4
    assert _call(nexr, _pair(nexr), ws_bytes=0) == 4


def test_empty_groups_are_noops(nexr):
    assert _call(nexr, [([], [(X_FIFO, X_HEAD, 0)], []), ([(X_FIFO, X_HEAD, 0)], [], [])], ws=0, ws_bytes=0) == 0


def _crossed(nexr, order0, order1):
    """Member 0 receives on X and sends on Y, member 1 receives on Y and sends on X, one step each way,
    in the given orders ("rs": receive first, then send; "sr": send first)."""
    n = 64
    recv, send = nexr.ll_step(-1, 0, 1, 0, n, recv=True), nexr.ll_step(0, 0, -1, 0, n, send=True)
    steps = {"rs": [recv, send], "sr": [send, recv]}
    return [([(X_FIFO, X_HEAD, 0)], [(Y_FIFO, Y_HEAD, 0)], steps[order0]),
            ([(Y_FIFO, Y_HEAD, 0)], [(X_FIFO, X_HEAD, 0)], steps[order1])]


def test_a_group_that_cannot_finish_is_refused_by_the_dry_run(nexr):
    """Both members receive first and send only afterwards: each waits for the other's later step, which
    no launch would ever produce: nexrInvalidUsage (5), nothing launched. The dry run comes before the
    workspace's capacity is looked at, so with a workspace of 8 bytes the same call still returns 5, and
    the same two members with either order swapped (a group that can finish) return the workspace's 4:
    they passed the dry run, and nothing reaches the device."""
    assert _call(nexr, _crossed(nexr, "rs", "rs")) == 5
    assert _call(nexr, _crossed(nexr, "rs", "rs"), ws_bytes=8) == 5
    for o0, o1 in (("sr", "rs"), ("rs", "sr"), ("sr", "sr")):
        assert _call(nexr, _crossed(nexr, o0, o1), ws_bytes=8) == 4, (o0, o1)
    # a sender behind its receiver on an internal connection is refused as well
    behind = _pair(nexr)
    behind[1] = ([(X_FIFO, X_HEAD, 3)], [], behind[1][2])
    assert _call(nexr, behind, ws_bytes=8) == 5
    # ten sends but one receive step in the group: 8 slots and one credit carry nine, the tenth has none
    per = SLOT // 2 // 4
    starved = [([], [(X_FIFO, X_HEAD, 0)], [nexr.ll_step(0, 0, -1, 0, per, send=True)] * 10),
               ([(X_FIFO, X_HEAD, 0)], [], [nexr.ll_step(0, 0, 1, 0, per, recv=True)])]
    assert _call(nexr, starved, ws_bytes=8) == 5
    starved[0] = (starved[0][0], starved[0][1], starved[0][2][:9])
    assert _call(nexr, starved, ws_bytes=8) == 4
    # one-ended connections count as always ready: the sender alone, its receiver outside the group
    assert _call(nexr, starved[:1], ws_bytes=8) == 4


def test_a_grid_that_is_not_resident_at_once_is_refused(nexr, monkeypatch):
    """nMembers x G workgroups must fit the GPU together (occupancy x CUs), else nexrInvalidUsage with
    nothing launched. The library's test hook stands in for the device's answer: two members of one
    workgroup each (64 KiB slots are G = 8, so 16) against room for 15."""
    monkeypatch.setenv("NEXR_TEST_LL_GROUP_RESIDENT", "15")
    assert _call(nexr, _pair(nexr)) == 5
    assert _call(nexr, _pair(nexr), ws_bytes=8) == 4      # the workspace is looked at before the device


def test_set_ll_group_needs_an_ll_device_memory_communicator(nexr, oracle):
    """Host-memory communicators (here with the oracle's CPU step functions underneath, so no GPU is
    touched), SIMPLE and LL alike, refuse the option with nexrInvalidUsage."""
    ring = importlib.import_module("nex-nccl_amd.ring")
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value
    ll_fn = ctypes.cast(oracle.lib().oracle_reduce_copy_ll_fn, ctypes.c_void_p).value
    for kw in (dict(fn_address=fn), dict(fn_address=fn, protocol=ring.PROTO_LL, ll_fn_address=ll_fn)):
        with ring.RingComm(2, ring.HOST_MEMORY, 32 << 10, timeout_ms=20000, **kw) as comm:
            for on in (True, False):
                with pytest.raises(nexr.NexrError) as e:
                    comm.set_ll_group(on)
                assert e.value.code == nexr.Result.InvalidUsage
            assert comm.queued() == 0
    assert ring.ring_lib().nexrRingCommSetLLGroup(None, 1) == 4
