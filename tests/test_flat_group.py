"""Grouped flat collectives without a GPU: nexrFlatGroup / nexrFlatGroupPlan (include/nexr.h). The header, the
exports and the ctypes mirror agree; every refusal answers before a device call; and nexrFlatGroupPlan, which makes
no device call at all, shows on made-up addresses how the works of a call are binned into launches: one open launch
per (datatype, op, min-or-max) and one for copies, all of them closed by a work that conflicts with a work of any of
them, a table in the kernel arguments up to NEXR_FLAT_GROUP_INLINE_BYTES and in fill launches beyond."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "nexr.h")
AR, RS, RD, CP = 0, 1, 2, 3
F32, F16, I32 = 7, 6, 2          # nexrFloat32, nexrFloat16, nexrInt32
SUM, MINMAX = 0, 2               # nexrDevSum, nexrDevMinMax


def work(coll, ins, outs, n_elts, dt=F32, op=SUM, arg=0, root=0, chunk=16):
    """One work as nexr.flat_group_works takes it; an all-reduce gets one part over its elements."""
    w = {"coll": coll, "inputs": ins, "outputs": outs, "n_elts": n_elts, "datatype": dt, "dev_red_op": op,
         "red_op_arg": arg, "root": root}
    if coll == AR and n_elts:
        w["parts"] = [(0, n_elts, chunk)]
    return w


def bufs(base, n, stride=0x10000):
    return [base + r * stride for r in range(n)]


def independent(k, n=2, elts=64, **kw):
    """All-reduce k of a series whose buffers never meet."""
    return work(AR, bufs(0x100000 * (2 * k + 1), n), bufs(0x100000 * (2 * k + 2), n), elts, **kw)


# ---- the ABI --------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_listed(nexr):
    text = open(HEADER).read()
    for name in ("nexrFlatGroup", "nexrFlatGroupPlan"):
        assert re.search(r"NEXR_API\s+nexrResult_t\s+%s\s*\(" % name, text), name
        assert name in nexr.ABI_SYMBOLS
        assert hasattr(nexr.lib(), name)
    out = subprocess.run(["nm", "-D", "--defined-only", nexr.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"nexrFlatGroup", "nexrFlatGroupPlan"} <= exported
    for define, value in (("NEXR_FLAT_GROUP_ALL_REDUCE", nexr.FLAT_GROUP_ALL_REDUCE),
                          ("NEXR_FLAT_GROUP_REDUCE_SCATTER", nexr.FLAT_GROUP_REDUCE_SCATTER),
                          ("NEXR_FLAT_GROUP_REDUCE", nexr.FLAT_GROUP_REDUCE), ("NEXR_FLAT_GROUP_COPY", nexr.FLAT_GROUP_COPY),
                          ("NEXR_FLAT_GROUP_INLINE_BYTES", nexr.FLAT_GROUP_INLINE_BYTES),
                          ("NEXR_FLAT_GROUP_FILL_BYTES", nexr.FLAT_GROUP_FILL_BYTES)):
        assert re.search(r"#define\s+%s\s+(\d+)" % define, text).group(1) == str(value), define
    assert (AR, RS, RD, CP) == (nexr.FLAT_GROUP_ALL_REDUCE, nexr.FLAT_GROUP_REDUCE_SCATTER, nexr.FLAT_GROUP_REDUCE,
                                nexr.FLAT_GROUP_COPY)


_LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "nexr.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(nexrFlatGroupWork),
         offsetof(nexrFlatGroupWork, coll), offsetof(nexrFlatGroupWork, datatype), offsetof(nexrFlatGroupWork, devRedOp),
         offsetof(nexrFlatGroupWork, root), offsetof(nexrFlatGroupWork, redOpArg), offsetof(nexrFlatGroupWork, inputs),
         offsetof(nexrFlatGroupWork, outputs), offsetof(nexrFlatGroupWork, nOutputs),
         offsetof(nexrFlatGroupWork, nParts), offsetof(nexrFlatGroupWork, parts), offsetof(nexrFlatGroupWork, nElts));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(nexrFlatGroupInfo), offsetof(nexrFlatGroupInfo, works),
         offsetof(nexrFlatGroupInfo, launches), offsetof(nexrFlatGroupInfo, fillLaunches),
         offsetof(nexrFlatGroupInfo, cuts), offsetof(nexrFlatGroupInfo, tableBytes), offsetof(nexrFlatGroupInfo, workgroups));
  return 0;
}
"""


def test_structs_match_the_header(nexr, tmp_path):
    """nexrFlatGroupWork / nexrFlatGroupInfo: the C layout, compiled from include/nexr.h, and the ctypes mirror."""
    src = tmp_path / "flat_group_layout.c"
    src.write_text(_LAYOUT)
    exe = tmp_path / "flat_group_layout"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True, timeout=120)
    w, i = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    W, I = nexr.FlatGroupWork, nexr.FlatGroupInfo
    assert w.split() == [str(v) for v in (ctypes.sizeof(W), W.coll.offset, W.datatype.offset, W.devRedOp.offset,
                                            W.root.offset, W.redOpArg.offset, W.inputs.offset, W.outputs.offset,
                                            W.nOutputs.offset, W.nParts.offset, W.parts.offset, W.nElts.offset)]
    assert i.split() == [str(v) for v in (ctypes.sizeof(I), I.works.offset, I.launches.offset, I.fillLaunches.offset,
                                            I.cuts.offset, I.tableBytes.offset, I.workgroups.offset)]


# ---- refusals, before any device call -------------------------------------------------------------------------------
def _both(nexr, n, works, user_first=True, max_wgs=0):
    """The result codes of nexrFlatGroupPlan and of nexrFlatGroup for the same arguments."""
    L = nexr.lib()
    arr, keep = nexr.flat_group_works(works)
    a = L.nexrFlatGroupPlan(n, arr, len(works), int(user_first), max_wgs, None, None)
    b = L.nexrFlatGroup(n, arr, len(works), int(user_first), max_wgs, None, None, None)
    del keep
    return a, b


def test_refusals(nexr):
    bad, ok = int(nexr.Result.InvalidArgument), int(nexr.Result.Success)
    n = 3
    a, b = bufs(0x100000, n), bufs(0x200000, n)
    good = work(AR, a, b, 64)
    L = nexr.lib()
    assert _both(nexr, n, []) == (ok, ok)                                   # nWorks == 0: no launch
    assert _both(nexr, n, [work(AR, a, b, 0), work(CP, a[:1], b, 0)]) == (ok, ok)   # empty works cost nothing
    assert L.nexrFlatGroupPlan(n, None, 1, 1, 0, None, None) == bad
    assert L.nexrFlatGroup(n, None, 1, 1, 0, None, None, None) == bad
    arr, keep = nexr.flat_group_works([good])
    assert L.nexrFlatGroupPlan(n, arr, -1, 1, 0, None, None) == bad
    assert L.nexrFlatGroupPlan(n, arr, 1, 1, -1, None, None) == bad         # maxWorkgroups < 0
    assert L.nexrFlatGroup(n, arr, 1, 1, -1, None, None, None) == bad
    assert L.nexrFlatGroupPlan(1, arr, 1, 1, 0, None, None) == bad and L.nexrFlatGroupPlan(65, arr, 1, 1, 0, None, None) == bad
    assert L.nexrFlatGroupPlan(n, arr, 1, 1, 0, None, None) == ok

    def refused(w):
        assert _both(nexr, n, [good, w]) == (bad, bad), w

    refused(dict(good, coll=4))
    refused(dict(good, coll=-1))
    # what the single entries refuse, per work
    for coll in (AR, RS, RD):
        base = work(coll, a, b, 64, root=1)
        refused(dict(base, datatype=10))                                    # fp8
        refused(dict(base, datatype=12))
        refused(dict(base, dev_red_op=5))
        refused(dict(base, dev_red_op=4))                                   # SumPostDiv on a float
        refused(dict(base, datatype=0, dev_red_op=4, red_op_arg=(256 << 1) | 1, parts=[(0, 64, 16)]))
        refused(dict(base, inputs=[a[0], 0, a[2]]))
        refused(dict(base, inputs=[a[0], a[1] + 2, a[2]]))                  # not aligned to 4
        refused(dict(base, n_elts=1 << 62, parts=[(0, 1 << 62, 16)]))
    refused(dict(work(AR, a, b, 64), outputs=[b[0], b[1], 0]))
    refused(dict(work(RS, a, b, 64), outputs=[b[0], b[1] + 1, b[2]]))
    refused(work(RD, a, b, 64, root=3))
    refused(work(RD, a, b, 64, root=-1))
    refused(dict(work(RD, a, b, 64, root=1), outputs=[b[0], 0, b[2]]))
    for parts in ([], [(0, 32, 16)], [(0, 32, 16), (48, 16, 16)], [(0, 64, 0)], [(0, 64, 6)], [(4, 60, 16)]):
        refused(dict(good, parts=parts))
    # copies
    refused(work(CP, [0], b, 100))
    refused(work(CP, a[:1], [], 100))                                       # nOutputs 0
    refused(work(CP, a[:1], [0x1000] * 65, 100))                            # nOutputs 65
    refused(work(CP, a[:1], [b[0], 0], 100))


def test_a_reduce_reads_its_roots_output_only(nexr):
    """outputs[r] of a reduce may be null for every r but the root."""
    n = 3
    a, b = bufs(0x100000, n), bufs(0x200000, n)
    launch_of, info = nexr.flat_group_plan(n, [dict(work(RD, a, b, 64, root=1), outputs=[0, b[1], 0])], True)
    assert launch_of == [0] and info["launches"] == 1


def cut_by(nexr, n, first, second):
    """Whether `second` (of another kind than `first`) closes first's launch: a third work of first's kind then
    cannot join it."""
    launch_of, _ = nexr.flat_group_plan(n, [first, second, independent(9, n=n)], True)
    assert launch_of[:2] == [0, 1] and launch_of[2] in (0, 2)
    return launch_of[2] == 2


# ---- the plan ---------------------------------------------------------------------------------------------------------
def test_independent_works_of_one_kind_share_a_launch(nexr):
    works = [independent(k) for k in range(7)]
    launch_of, info = nexr.flat_group_plan(2, works, True)
    assert launch_of == [0] * 7
    assert info == {"works": 7, "launches": 1, "fill_launches": 0, "cuts": 0, "table_bytes": 7 * (40 + 32 + 24), "workgroups": 2}
    # 7 works of one 256-byte piece each: 7 items, four waves per workgroup
    assert nexr.flat_group_plan(2, works, True, max_workgroups=1)[1]["workgroups"] == 1


def test_kinds_get_a_launch_each(nexr):
    abab = [independent(k, dt=F32 if k % 2 == 0 else F16) for k in range(4)]
    launch_of, info = nexr.flat_group_plan(2, abab, True)
    assert launch_of == [0, 1, 0, 1] and info["launches"] == 2
    minmax = [independent(k, op=MINMAX, arg=k % 2) for k in range(4)]       # bit 0: min or max
    launch_of, info = nexr.flat_group_plan(2, minmax, True)
    assert launch_of == [0, 1, 0, 1] and info["launches"] == 2
    ops = [independent(0), independent(1, op=1), independent(2)]            # Sum, Prod, Sum
    assert nexr.flat_group_plan(2, ops, True)[0] == [0, 1, 0]
    # the three reductions of one kind share a launch; copies have their own
    mixed = [independent(0), work(RS, bufs(0x700000, 2), bufs(0x800000, 2), 8),
             work(RD, bufs(0x900000, 2), bufs(0xA00000, 2), 8, root=1), work(CP, [0xB00000], bufs(0xC00000, 2), 100),
             independent(7), work(CP, [0xD00000], bufs(0xE00000, 2), 5)]
    launch_of, info = nexr.flat_group_plan(2, mixed, True)
    assert launch_of == [0, 0, 0, 1, 0, 1] and info["launches"] == 2 and info["works"] == 6


def test_conflicts_cut(nexr):
    n = 2
    A, B, C = bufs(0x100000, n), bufs(0x200000, n), bufs(0x300000, n)
    first = work(AR, A, B, 64)
    # read after write: the second reads what the first writes
    assert nexr.flat_group_plan(n, [first, work(AR, B, C, 64)], True)[0] == [0, 1]
    # write after read: the second writes what the first reads
    assert nexr.flat_group_plan(n, [first, work(AR, C, A, 64)], True)[0] == [0, 1]
    # write after write
    assert nexr.flat_group_plan(n, [first, work(AR, C, B, 64)], True)[0] == [0, 1]
    # shared inputs alone do not conflict
    assert nexr.flat_group_plan(n, [first, work(AR, A, C, 64)], True)[0] == [0, 0]
    # one byte is enough, and ranges are half-open: the next byte is free
    last = [B[0] + 255, 0x400000]
    assert cut_by(nexr, n, first, work(CP, [0x500000], last, 1))
    after = [B[0] + 256, 0x400000]
    assert not cut_by(nexr, n, first, work(CP, [0x500000], after, 1))
    # a conflict with a work of ANY open launch closes all of them, in the order they were opened
    other = independent(5, dt=F16)
    third = independent(6, dt=F16)
    launch_of, info = nexr.flat_group_plan(n, [first, other, work(AR, B, C, 64), third], True)
    assert launch_of == [0, 1, 2, 3] and info["launches"] == 4 and info["cuts"] == 1
    # in place inside one work: no cut, and the next independent work still joins
    launch_of, _ = nexr.flat_group_plan(n, [work(AR, A, A, 64), independent(7)], True)
    assert launch_of == [0, 0]


def test_a_reduce_scatter_reads_n_chunks(nexr):
    n = 4
    ins, outs = bufs(0x100000, n), bufs(0x200000, n)
    rs = work(RS, ins, outs, 64)                                            # reads 4 * 64 * 4 = 1024 bytes per input
    inside = work(CP, [0x500000], [ins[0] + 1023], 1)
    beyond = work(CP, [0x500000], [ins[0] + 1024], 1)
    assert cut_by(nexr, n, rs, inside) and not cut_by(nexr, n, rs, beyond)
    # a reduce writes its root's output only
    rd = work(RD, ins, outs, 64, root=2)
    assert not cut_by(nexr, n, rd, work(CP, [0x500000], [outs[1]], 8))
    assert cut_by(nexr, n, rd, work(CP, [0x500000], [outs[2]], 8))


def test_empty_works_get_no_launch(nexr):
    n = 2
    works = [independent(0), independent(1, elts=0), work(CP, [0x900000], bufs(0xA00000, 2), 0), independent(2),
             work(CP, [0xB00000], [0xB00000], 64)]                          # a copy onto itself writes nothing
    launch_of, info = nexr.flat_group_plan(n, works, True)
    assert launch_of == [0, -1, -1, 0, -1]
    assert info["works"] == 2 and info["launches"] == 1
    launch_of, info = nexr.flat_group_plan(n, [independent(1, elts=0)], True)
    assert launch_of == [-1] and info == {"works": 0, "launches": 0, "fill_launches": 0, "cuts": 0, "table_bytes": 0, "workgroups": 0}


@pytest.mark.parametrize("n", (2, 8))
def test_inline_and_workspace_boundary(nexr, n):
    """The largest table that fits the kernel arguments, and one work more."""
    rec = 40 + 16 * n + 24                                                  # a record and one part
    most = nexr.FLAT_GROUP_INLINE_BYTES // rec
    assert n != 8 or most == 20
    works = [work(AR, bufs(0x1000000 * (2 * k + 1), n), bufs(0x1000000 * (2 * k + 2), n), 64) for k in range(most + 1)]
    launch_of, info = nexr.flat_group_plan(n, works[:most], True)
    assert launch_of == [0] * most
    assert info["table_bytes"] == most * rec and info["fill_launches"] == 0 and info["launches"] == 1
    launch_of, info = nexr.flat_group_plan(n, works, True)
    assert launch_of == [0] * (most + 1) and info["launches"] == 1
    assert info["table_bytes"] == (most + 1) * rec > nexr.FLAT_GROUP_INLINE_BYTES
    assert info["fill_launches"] == -(-info["table_bytes"] // nexr.FLAT_GROUP_FILL_BYTES) == 2
    # copies: records of 24 + 8 * (the longest destination list)
    cp = [work(CP, [0x10000 * (3 * k + 1)], [0x10000 * (3 * k + 2), 0x10000 * (3 * k + 3)], 10) for k in range(99)]
    assert nexr.FLAT_GROUP_INLINE_BYTES // 40 == 98
    assert nexr.flat_group_plan(n, cp[:98], True)[1]["fill_launches"] == 0
    assert nexr.flat_group_plan(n, cp, True)[1]["fill_launches"] == 1


def test_workgroups_follow_the_items(nexr):
    """A wave per 2048-byte piece over the launch's summed pieces (a reduce-scatter: times n), four waves per
    workgroup; maxWorkgroups caps every launch."""
    n = 2
    works = [independent(0, elts=512 * 5), independent(1, elts=1),                      # 5 pieces + 1
             work(RS, bufs(0x5000000, n), bufs(0x6000000, n), 513)]                     # 2 pieces x 2 chunks
    _, info = nexr.flat_group_plan(n, works, True)
    assert info["workgroups"] == 3                                                      # 10 items
    _, info = nexr.flat_group_plan(n, works + [independent(3, dt=F16)], True, max_workgroups=2)
    assert info["launches"] == 2 and info["workgroups"] == 2 + 1


# ---- the ring library: nexrRingGroupStart / nexrRingGroupEnd on a host-memory communicator --------------------------
import importlib  # noqa: E402

import numpy as np  # noqa: E402

import ring_modes_cases as rm  # noqa: E402
from oracle import ring as oring  # noqa: E402


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


@pytest.fixture(scope="module")
def fns(oracle):
    L = oracle.lib()
    cast = lambda f: ctypes.cast(f, ctypes.c_void_p).value  # noqa: E731
    return cast(L.oracle_reduce_copy_fn), cast(L.oracle_reduce_copy_ll_fn), cast(L.oracle_reduce_copy_ll128_fn)


def host_comm(ring, fns, protocol, n, channels=1):
    f, fll, fll128 = fns
    return ring.RingComm(n, ring.HOST_MEMORY, rm.BUFF[protocol], f, 20000, rm.PROTO_ID[protocol], fll, fll128,
                         rm.tree_per_node(n), 0, channels)


def chunk_of(coll, protocol, esz):
    return oring.chunk_count(coll, protocol, esz, rm.BUFF[protocol])


def test_ring_symbols(ring):
    text = open(os.path.join(ROOT, "include", "nexr_ring.h")).read()
    L = ring.ring_lib()
    for name in ("nexrRingGroupStart", "nexrRingGroupEnd", "nexrRingGroupGetStats"):
        assert re.search(r"NEXR_API\s+nexrResult_t\s+%s\s*\(" % name, text), name
        assert name in ring.RING_ABI_SYMBOLS and hasattr(L, name)


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_ring_group_gives_the_single_calls_bytes(ring, nexr, oracle, fns, protocol):
    """Mixed calls of all six collectives inside a group on a host-memory communicator (every call runs alone at its
    place there): nothing runs before the outermost End, and then every arena holds the bytes of the call alone."""
    n = 3
    with host_comm(ring, fns, protocol, n, 2) as comm:
        calls = [rm.make_call(sp, n, rm.SEED, oring, protocol, 2) for sp in rm.mixed_plan(protocol, n, chunk_of, 11, 12)]
        arenas = [c.arena0.copy() for c in calls]
        comm.group_stats(reset=True)
        with comm.group():
            with comm.group():                                 # nesting: the inner End runs nothing
                for call, arena in zip(calls[:5], arenas):
                    rm.issue(comm, call, arena.ctypes.data)
            for call, arena in zip(calls[:5], arenas):
                np.testing.assert_array_equal(arena, call.arena0)
            for call, arena in zip(calls[5:], arenas[5:]):
                rm.issue(comm, call, arena.ctypes.data)
            assert comm.group_stats() == {"calls": 12, "group_launches": 0, "fill_launches": 0, "singles": 0, "cuts": 0}
        for call, arena in zip(calls, arenas):
            rm.check(call, arena, (protocol, "group", n))
        assert comm.group_stats() == {"calls": 12, "group_launches": 0, "fill_launches": 0, "singles": 12, "cuts": 0}
        assert comm.queued() != 5
        # and the communicator goes on working outside a group
        again = calls[0].arena0.copy()
        rm.issue(comm, calls[0], again.ctypes.data)
        rm.check(calls[0], again, (protocol, "after the group", n))


def test_ring_group_runs_a_chain_in_call_order(ring, nexr, oracle, fns):
    """One call's output is the next one's input: an all-reduce, a broadcast of its result, an all-gather of that."""
    n, count = 3, 100
    F32 = int(nexr.DataType.Float32)
    rng = np.random.default_rng(5)

    def run(grouped):
        x = [rng0.integers(1, 50, count).astype(np.float32) for _ in range(n)]
        y = [np.zeros(count, np.float32) for _ in range(n)]
        z = [np.zeros(count, np.float32) for _ in range(n)]
        g = [np.zeros(n * count, np.float32) for _ in range(n)]
        with host_comm(ring, fns, "simple", n) as comm:
            def body():
                comm.all_reduce([a.ctypes.data for a in x], [a.ctypes.data for a in y], count, F32, rm.SUM)
                comm.broadcast([a.ctypes.data for a in y], [a.ctypes.data for a in z], count, F32, 1)
                comm.all_gather([a.ctypes.data for a in z], [a.ctypes.data for a in g], count, F32)
            if grouped:
                with comm.group():
                    body()
                    assert not g[0].any()
            else:
                body()
        return x, g

    rng0 = np.random.default_rng(5)
    x, plain = run(False)
    rng0 = np.random.default_rng(5)
    _, grouped = run(True)
    want = np.tile(x[0] + x[1] + x[2], n)
    for r in range(n):
        np.testing.assert_array_equal(plain[r], want)
        np.testing.assert_array_equal(grouped[r], want)
    del rng


def test_ring_group_usage(ring, nexr, oracle, fns):
    bad_use, bad_arg = nexr.Result.InvalidUsage, nexr.Result.InvalidArgument
    L = ring.ring_lib()
    assert L.nexrRingGroupStart(None) == bad_arg and L.nexrRingGroupEnd(None) == bad_arg
    assert L.nexrRingGroupGetStats(None, None, 0) == bad_arg
    n = 2
    F32 = int(nexr.DataType.Float32)
    with host_comm(ring, fns, "simple", n) as comm:
        with pytest.raises(nexr.NexrError) as e:                # End without Start
            comm.group_end()
        assert e.value.code == bad_use
        x = [np.arange(8, dtype=np.float32) + r for r in range(n)]
        y = [np.zeros(8, np.float32) for _ in range(n)]
        xs, ys = [a.ctypes.data for a in x], [a.ctypes.data for a in y]
        comm.group_stats(reset=True)
        with comm.group():
            # a failing call is returned at once and is not recorded
            for call in (lambda: comm.all_reduce(xs, ys, 8, 10, rm.SUM),           # fp8
                         lambda: comm.all_reduce(xs, ys, 8, F32, 99),               # no such op
                         lambda: comm.reduce(xs, ys, 8, F32, rm.SUM, 2),            # no such root
                         lambda: comm.broadcast(xs, ys, 8, F32, -1),
                         lambda: comm.all_reduce([xs[0], 0], ys, 8, F32, rm.SUM),   # a null buffer
                         lambda: comm.all_reduce_flat(xs, ys, 8, F32, rm.SUM)):     # host memory with a caller's fn
                with pytest.raises(nexr.NexrError) as e:
                    call()
                assert e.value.code in (bad_arg, bad_use)
            assert e.value.code == bad_use
            comm.all_reduce(xs, ys, 8, F32, rm.SUM)
            assert comm.group_stats()["calls"] == 1 and not y[0].any()
        np.testing.assert_array_equal(y[0], x[0] + x[1])
        np.testing.assert_array_equal(y[1], x[0] + x[1])
        assert comm.group_stats()["singles"] == 1
        with pytest.raises(nexr.NexrError):                     # the depth is back at 0
            comm.group_end()


def test_the_group_kernels_are_46_and_two_without_scratch():
    """flat_group_kernel has one instance per (datatype, device op) as flat_kernel, beside flat_group_copy_kernel and
    flat_group_fill_kernel; none has a private segment, a spilled vector register or a dynamic stack (read out of the
    shipped code object)."""
    import test_code_objects as tco
    path = os.path.join(tco.PKG, "libnexr.so")
    assert os.path.exists(path), "libnexr.so not built"
    seen = {}
    for co in tco.gfx950_code_objects(tco._read(path)):
        _tables, notes = tco.elf_tables(co)
        for k in (k for note in notes for k in note["amdhsa.kernels"]):
            if "flat_group" in k[".name"]:
                seen[k[".name"]] = (k[".private_segment_fixed_size"], k.get(".vgpr_spill_count", 0),
                                    k.get(".uses_dynamic_stack", False))
    assert len([name for name in seen if "flat_group_kernel" in name]) == 46, sorted(seen)
    assert len([name for name in seen if "flat_group_copy_kernel" in name]) == 1
    assert len([name for name in seen if "flat_group_fill_kernel" in name]) == 1 and len(seen) == 48
    assert {name: v for name, v in seen.items() if v != (0, 0, False)} == {}
