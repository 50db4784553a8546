"""CPU tests of nexrReduceCopySimpleStepsGroup / nexrSimpleGroupWorkspaceBytes (include/nexr.h) and of
nexrRingCommSetSimpleGroup (include/nexr_ring.h): every rejection happens before any device call, so the
return codes are checked here without a GPU — the argument checks (4, nexrInvalidArgument), the workspace
that holds too few launches (4), the host dry run (5, nexrInvalidUsage) and the residency refusal through
the library's test hook (5). The host planner is the LL group calls'; what differs for SIMPLE is checked:
slices of stepPerSlice slots, counters that advance by stepPerSlice, a grid the caller may choose."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

from conftest import ROOT

F32, U8 = 7, 1
SLOT = 1 << 14                      # with 2-step slices: 8 tiles of 4 KiB a slice, G = 8 by default
X = (0x100000, 0x180000, 0x190000)  # made-up device addresses (fifo, tail block, head block): nothing reaches the device
Y = (0x300000, 0x380000, 0x390000)
WS = 0x800000


def _call(nexr, members, dt=F32, op=0, arg=0, ws=WS, ws_bytes=None, slot=SLOT, n_members=None, null=None, n_slots=8,
          sps=2, wpm=0):
    """members: (recv, send, steps) per member, recv / send as (fifo, tail, head, step) lists. Returns the code."""
    L = nexr.lib()
    n = len(members) if n_members is None else n_members

    def pick(v, m):
        return v[m] if isinstance(v, list) else v
    sets = [nexr.simple_conn_set(0x10000 * (m + 1), 0x20000000 + 0x10000 * m, r, s, pick(slot, m), pick(n_slots, m),
                                 pick(sps, m)) for m, (r, s, _steps) in enumerate(members)]
    cs = (nexr.SimpleConnSet * max(1, len(sets)))(*sets)
    arrs = [(nexr.LLStep * max(1, len(st)))(*st) for _r, _s, st in members]
    ptrs = (ctypes.POINTER(nexr.LLStep) * max(1, len(arrs)))(*[ctypes.cast(a, ctypes.POINTER(nexr.LLStep))
                                                               for a in arrs])
    counts = (ctypes.c_int * max(1, len(members)))(*[len(st) for _r, _s, st in members])
    if ws_bytes is None:
        ws_bytes = nexr.simple_group_workspace_bytes(max(1, min(n, 32)))
    return L.nexrReduceCopySimpleStepsGroup(n, None if null == "conns" else cs, None if null == "steps" else ptrs,
                                            None if null == "counts" else counts, dt, op, arg, wpm, None, 0,
                                            ctypes.c_void_p(ws) if ws else None, ws_bytes, None)


def _conn(c, step=0):
    return (c[0], c[1], c[2], step)


def _pair(nexr, per=SLOT * 2 // 4, step=0):
    """Member 0 sends on X, member 1 receives on X: a valid two-member group of one slice each."""
    return [([], [_conn(X, step)], [nexr.ll_step(0, 0, -1, 0, per, send=True)]),
            ([_conn(X, step)], [], [nexr.ll_step(0, 0, 1, 0, per, recv=True)])]


def test_the_symbols_are_declared_exported_and_wrapped(nexr):
    hdr = open(os.path.join(ROOT, "include", "nexr.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", nexr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in ("nexrSimpleGroupWorkspaceBytes", "nexrReduceCopySimpleStepsGroup"):
        assert re.search(r"NEXR_API\s+nexrResult_t\s+" + name + r"\s*\(", hdr)
        assert name in exported and name in nexr.ABI_SYMBOLS
    assert callable(nexr.reduce_copy_simple_steps_group) and callable(nexr.simple_conn_set)
    assert callable(nexr.simple_group_workspace_bytes)
    assert nexr.version() == 300                       # additions only
    assert re.search(r"#define\s+NEXR_SIMPLE_CREDIT_BYTES\s+(\d+)", hdr).group(1) == str(nexr.SIMPLE_CREDIT_BYTES)
    assert re.search(r"#define\s+NEXR_SIMPLE_GROUP_MAX_GRID\s+(\d+)", hdr).group(1) == str(nexr.SIMPLE_GROUP_MAX_GRID)
    assert nexr.SIMPLE_GROUP_MAX_GRID == nexr.SIMPLE_CREDIT_BYTES // 16
    ring = importlib.import_module("nex-nccl_amd.ring")
    rhdr = open(os.path.join(ROOT, "include", "nexr_ring.h")).read()
    assert re.search(r"NEXR_API\s+nexrResult_t\s+nexrRingCommSetSimpleGroup\s*\(", rhdr)
    assert "nexrRingCommSetSimpleGroup" in ring.RING_ABI_SYMBOLS and hasattr(ring.ring_lib(), "nexrRingCommSetSimpleGroup")
    assert callable(ring.RingComm.set_simple_group)


_LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "nexr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(nexrSimpleConnSet),
         offsetof(nexrSimpleConnSet, input), offsetof(nexrSimpleConnSet, output), offsetof(nexrSimpleConnSet, nRecv),
         offsetof(nexrSimpleConnSet, nSend), offsetof(nexrSimpleConnSet, recvFifo), offsetof(nexrSimpleConnSet, recvTail),
         offsetof(nexrSimpleConnSet, recvHead), offsetof(nexrSimpleConnSet, recvStep), offsetof(nexrSimpleConnSet, sendFifo),
         offsetof(nexrSimpleConnSet, sendTail), offsetof(nexrSimpleConnSet, sendHead), offsetof(nexrSimpleConnSet, sendStep),
         offsetof(nexrSimpleConnSet, slotBytes), offsetof(nexrSimpleConnSet, nSlots),
         offsetof(nexrSimpleConnSet, stepPerSlice));
  return 0;
}
"""


def test_the_conn_set_matches_its_ctypes_mirror(nexr, tmp_path):
    src = tmp_path / "simple_layout.c"
    src.write_text(_LAYOUT)
    exe = tmp_path / "simple_layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True, timeout=120)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    C = nexr.SimpleConnSet
    assert got == [str(v) for v in (ctypes.sizeof(C), C.input.offset, C.output.offset, C.nRecv.offset, C.nSend.offset,
                                    C.recvFifo.offset, C.recvTail.offset, C.recvHead.offset, C.recvStep.offset,
                                    C.sendFifo.offset, C.sendTail.offset, C.sendHead.offset, C.sendStep.offset,
                                    C.slotBytes.offset, C.nSlots.offset, C.stepPerSlice.offset)]
    assert ctypes.sizeof(C) == 16 + 8 + 8 * 24 + 16 == 232
    assert ctypes.sizeof(nexr.LLStep) == 32            # nexrLLStep is reused unchanged


def test_workspace_bytes(nexr):
    L = nexr.lib()
    b = ctypes.c_size_t(0)
    sizes = []
    for n in (1, 2, 32):
        assert L.nexrSimpleGroupWorkspaceBytes(n, ctypes.byref(b)) == 0
        sizes.append(b.value)
    assert sizes[1] == 2 * sizes[0] and sizes[2] == 32 * sizes[0] and sizes[0] % (8 * 8) == 0
    assert sizes[0] // 8 >= 96 * 32                    # a region holds a member's 96 records
    assert L.nexrSimpleGroupWorkspaceBytes(0, ctypes.byref(b)) == 4
    assert L.nexrSimpleGroupWorkspaceBytes(33, ctypes.byref(b)) == 4
    assert L.nexrSimpleGroupWorkspaceBytes(2, None) == 4


def test_bad_arguments_fail_before_the_device(nexr):
    pair = _pair(nexr)
    assert _call(nexr, pair, ws_bytes=8) == 4                            # valid so far: only the workspace is short
    assert _call(nexr, pair, n_members=0) == 4
    one = ([], [], [nexr.ll_step(0, 0, 1, 0, 100)])
    assert _call(nexr, [one] * 33) == 4                                  # > NEXR_LL_GROUP_MAX_MEMBERS
    for null in ("conns", "steps", "counts"):
        assert _call(nexr, pair, null=null) == 4
    empty = [(r, s, []) for r, s, _st in pair]
    # slotBytes: a 16-byte multiple
    for bad in (0, 8, SLOT + 4):
        assert _call(nexr, empty, slot=bad, ws=0) == 4, bad
    assert _call(nexr, empty, slot=16, ws=0) == 0
    # nElts * size <= slotBytes * stepPerSlice
    assert _call(nexr, _pair(nexr, SLOT * 2 // 4 + 1), ws_bytes=8) == 4 and _call(nexr, _pair(nexr, SLOT * 2 // 4 + 1)) == 4
    assert _call(nexr, _pair(nexr, SLOT // 4 + 1), sps=1) == 4           # one slot only at 1-step slices
    assert _call(nexr, _pair(nexr, SLOT // 4), sps=1, ws_bytes=8) == 4   # ... which this fits: the workspace's 4,
    assert _call(nexr, empty, sps=1, ws=0) == 0                          # as empty lists show
    assert _call(nexr, _pair(nexr, SLOT * 4 + 1), dt=U8, sps=4) == 4
    # stepPerSlice >= 1, nSlots % stepPerSlice == 0, counters on multiples of stepPerSlice
    assert _call(nexr, empty, sps=0, ws=0) == 4
    assert _call(nexr, empty, sps=3, ws=0) == 4
    assert _call(nexr, empty, sps=8, ws=0) == 0
    assert _call(nexr, empty, sps=16, ws=0) == 4
    assert _call(nexr, [(r, s, []) for r, s, _st in _pair(nexr, 1, step=3)], ws=0) == 4
    assert _call(nexr, [(r, s, []) for r, s, _st in _pair(nexr, 1, step=4)], ws=0) == 0
    assert _call(nexr, [(r, s, []) for r, s, _st in _pair(nexr, 1, step=3)], sps=1, ws=0) == 0
    # nSlots
    assert _call(nexr, empty, n_slots=0, ws=0) == 4
    assert _call(nexr, empty, n_slots=0x80000000, ws=0) == 4             # above INT_MAX
    # slotBytes, nSlots and stepPerSlice equal across members
    assert _call(nexr, pair, slot=[SLOT, SLOT * 2]) == 4
    assert _call(nexr, pair, n_slots=[8, 4]) == 4
    assert _call(nexr, _pair(nexr, 16), sps=[2, 1]) == 4
    # workgroupsPerMember in 0..256
    assert _call(nexr, pair, wpm=-1) == 4 and _call(nexr, pair, wpm=257) == 4
    assert _call(nexr, pair, wpm=256, ws_bytes=8) == 4 and _call(nexr, empty, wpm=256, ws=0) == 0
    # datatypes and ops nexrReduceCopy's step lists refuse
    assert _call(nexr, pair, dt=10) == 4 and _call(nexr, pair, dt=11) == 4   # fp8
    assert _call(nexr, pair, dt=12) == 4 and _call(nexr, pair, dt=-1) == 4
    assert _call(nexr, pair, op=5) == 4 and _call(nexr, pair, op=-1) == 4
    assert _call(nexr, pair, dt=F32, op=4) == 4                          # SumPostDiv on a float
    assert _call(nexr, _pair(nexr, 64), dt=0, op=4, arg=(256 << 1) | 1) == 4  # int8 divisor that wraps to 0
    # records: buffers out of range, a buffer the member does not have, recv / send without a connection, no source
    bad_steps = [nexr.ll_step(2, 0, 1, 0, 4), nexr.ll_step(0, 0, -2, 0, 4), nexr.ll_step(0, -1, 1, 0, 4),
                 nexr.ll_step(0, 0, 1, 0, 4, recv=True), nexr.ll_step(0, 0, 1, 0, 4, send=True),
                 nexr.ll_step(-1, 0, 1, 0, 4), nexr.ll_step(0, 0, -1, 0, 4)]
    for st in bad_steps:
        assert _call(nexr, [([], [], [st])]) == 4
    # misaligned FIFO, missing or misaligned tail / head block, workspace missing or misaligned
    for bad in ((X[0] + 8, X[1], X[2], 0), (X[0], 0, X[2], 0), (X[0], X[1], 0, 0), (X[0], X[1] + 4, X[2], 0),
                (X[0], X[1], X[2] + 4, 0), (0, X[1], X[2], 0)):
        assert _call(nexr, [pair[0], ([bad], [], pair[1][2])]) == 4, bad
        assert _call(nexr, [([], [bad], pair[0][2]), pair[1]]) == 4, bad
    assert _call(nexr, pair, ws=0) == 4
    assert _call(nexr, pair, ws=WS + 4) == 4


def test_a_workspace_that_holds_too_few_launches(nexr):
    region = nexr.simple_group_workspace_bytes(2, 1)
    long = [([], [_conn(X)], [nexr.ll_step(0, 0, -1, 0, 64, send=True)] * 97),
            ([_conn(X)], [], [nexr.ll_step(0, 0, 1, 0, 64, recv=True)] * 97)]
    assert _call(nexr, long, ws_bytes=region) == 4          # 97 records are two launches
    assert _call(nexr, long, ws_bytes=2 * region - 8) == 4
    assert _call(nexr, _pair(nexr), ws_bytes=region - 8) == 4
    assert _call(nexr, _pair(nexr), ws_bytes=0) == 4
    # a user-range conflict cuts as well: the second record writes bytes the first wrote, one element on
    overlap = [([], [_conn(X)], [nexr.ll_step(0, 0, -1, 0, 64, send=True)] * 2),
               ([_conn(X)], [], [nexr.ll_step(-1, 0, 1, 0, 64, recv=True), nexr.ll_step(-1, 0, 1, 1, 64, recv=True)])]
    assert _call(nexr, overlap, ws_bytes=region) == 4


def test_empty_groups_are_noops(nexr):
    assert _call(nexr, [([], [_conn(X)], []), ([_conn(X)], [], [])], ws=0, ws_bytes=0) == 0


def _crossed(nexr, order0, order1):
    n = 64
    recv, send = nexr.ll_step(-1, 0, 1, 0, n, recv=True), nexr.ll_step(0, 0, -1, 0, n, send=True)
    steps = {"rs": [recv, send], "sr": [send, recv]}
    return [([_conn(X)], [_conn(Y)], steps[order0]), ([_conn(Y)], [_conn(X)], steps[order1])]


def test_a_group_that_cannot_finish_is_refused_by_the_dry_run(nexr):
    assert _call(nexr, _crossed(nexr, "rs", "rs")) == 5
    assert _call(nexr, _crossed(nexr, "rs", "rs"), ws_bytes=8) == 5      # before the workspace is looked at
    for o0, o1 in (("sr", "rs"), ("rs", "sr"), ("sr", "sr")):
        assert _call(nexr, _crossed(nexr, o0, o1), ws_bytes=8) == 4, (o0, o1)
    behind = _pair(nexr)
    behind[1] = ([_conn(X, 4)], [], behind[1][2])                        # more read than sent
    assert _call(nexr, behind, ws_bytes=8) == 5
    # the counters advance by stepPerSlice and the credit test is sendStep + stepPerSlice - nSlots <= head:
    # 8 slots hold four 2-step slices, eight 1-step ones, two 4-step ones
    for sps, fit in ((2, 4), (1, 8), (4, 2)):
        send = nexr.ll_step(0, 0, -1, 0, 64, send=True)
        starved = [([], [_conn(X)], [send] * (fit + 2)), ([_conn(X)], [], [nexr.ll_step(0, 0, 1, 0, 64, recv=True)])]
        assert _call(nexr, starved, ws_bytes=8, sps=sps) == 5, sps       # the receiver frees one slice: one too many
        starved[0] = ([], [_conn(X)], [send] * (fit + 1))
        assert _call(nexr, starved, ws_bytes=8, sps=sps) == 4, sps
        assert _call(nexr, [([], [_conn(X)], [send] * (fit + 2))], ws_bytes=8, sps=sps) == 4   # one-ended: the run form


def test_a_grid_that_is_not_resident_at_once_is_refused(nexr, monkeypatch):
    """16 KiB slots in 2-step slices are 8 tiles of 4 KiB: two members need 16 workgroups resident."""
    monkeypatch.setenv("NEXR_TEST_SIMPLE_GROUP_RESIDENT", "15")
    assert _call(nexr, _pair(nexr)) == 5
    assert _call(nexr, _pair(nexr), ws_bytes=8) == 4      # the workspace is looked at before the device
    assert _call(nexr, _pair(nexr, 16), wpm=8) == 5       # the caller's grid counts, not the slices' sizes
    assert _call(nexr, _pair(nexr), sps=4) == 5           # 16 tiles a slice
    monkeypatch.setenv("NEXR_TEST_SIMPLE_GROUP_RESIDENT", "1")
    assert _call(nexr, _pair(nexr, 4), slot=16, sps=1) == 5   # one workgroup a member at the least
    assert _call(nexr, _pair(nexr, 4), wpm=1) == 5
    monkeypatch.setenv("NEXR_TEST_SIMPLE_GROUP_RESIDENT", "511")
    assert _call(nexr, _pair(nexr, 16), slot=1 << 20) == 5    # on the cap of 256 a member
    assert _call(nexr, _pair(nexr, 16), wpm=256) == 5


def test_set_simple_group_needs_simple_thread_ranks_in_device_memory(nexr, oracle):
    """Host-memory communicators refuse the option, LL ones too (the oracle's CPU step functions underneath,
    so no GPU is touched), and nexrRingCommSetLLGroup keeps refusing SIMPLE."""
    ring = importlib.import_module("nex-nccl_amd.ring")
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value
    ll_fn = ctypes.cast(oracle.lib().oracle_reduce_copy_ll_fn, ctypes.c_void_p).value
    with ring.RingComm(2, ring.HOST_MEMORY, 8 * 4096, fn, 20000) as comm:
        for on in (True, False):
            with pytest.raises(nexr.NexrError) as e:
                comm.set_simple_group(on)
            assert e.value.code == nexr.Result.InvalidUsage
            with pytest.raises(nexr.NexrError) as e:
                comm.set_ll_group(on)
            assert e.value.code == nexr.Result.InvalidUsage
        assert comm.queued() == 0
    with ring.RingComm(2, ring.HOST_MEMORY, 8 * 4096, fn, 20000, ring.PROTO_LL, ll_fn) as comm:
        for on in (True, False):
            with pytest.raises(nexr.NexrError) as e:
                comm.set_simple_group(on)
            assert e.value.code == nexr.Result.InvalidUsage
        assert comm.queued() == 0
