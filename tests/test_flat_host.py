"""The flat collectives over host memory (nexrFlatHost*) without a GPU: the new symbols and the stats struct, every
argument check of the six entries (those of nexrFlatAllReduce, nexrFlatReduceScatter, nexrFlatReduce,
nexrFlatTreeAllReduce, nexrFlatBroadcast and nexrSymAllGather, answered before any device call), and the
host-memory communicators that the ring library's flat entries still refuse: a caller's fn, and LL and LL128 with
the caller's step functions. A peer (process-rank) communicator opens its GPU when it is created, so that refusal
is tested in tests/test_flat_host_gpu.py, which also runs the calls."""
import ctypes
import importlib
import os
import re

import pytest

from oracle import ring as oring

HOST_ENTRIES = ("nexrFlatHostAllReduce", "nexrFlatHostReduceScatter", "nexrFlatHostReduce",
                "nexrFlatHostTreeAllReduce", "nexrFlatHostBroadcast", "nexrFlatHostAllGather")


@pytest.fixture(scope="module")
def L(nexr):
    return nexr.lib()


def _arr(vals):
    a = (ctypes.c_void_p * max(1, len(vals)))()
    for i, v in enumerate(vals):
        a[i] = v
    return a


def _parts(nexr, parts):
    return (nexr.FlatPart * max(1, len(parts)))(*[nexr.FlatPart(*p) for p in parts])


def _tree_parts(nexr, parts):
    return (nexr.FlatTreePart * max(1, len(parts)))(*[nexr.FlatTreePart(o, c, t, 0) for o, c, t in parts])


def test_symbols_and_stats_struct(nexr):
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "nexr.h")).read()
    for name in HOST_ENTRIES + ("nexrGetFlatHostStats",):
        assert re.search(r"NEXR_API nexrResult_t %s\(" % name, header), name
        assert name in nexr.ABI_SYMBOLS and hasattr(nexr.lib(), name)
    body = re.search(r"typedef struct \{([^}]*)\} nexrFlatHostStats;", header).group(1)
    fields = [f.strip() for f in re.sub(r"uint64_t|;", "", body).split(",")]
    assert fields == [f for f, _ in nexr.FlatHostStats._fields_]
    assert fields == ["calls", "zeroCopyCalls", "stagedBuffers", "registeredHits", "pointerQueries", "windows"]
    assert ctypes.sizeof(nexr.FlatHostStats) == 48
    # nexrGetHostPathStats' struct is as it was
    assert ctypes.sizeof(nexr.HostPathStats) == 64
    assert nexr.lib().nexrGetFlatHostStats(None, 0) == nexr.Result.InvalidArgument
    st = nexr.flat_host_stats(reset=True)
    assert set(st) == set(fields)
    assert nexr.flat_host_stats() == dict.fromkeys(fields, 0)


def test_ring_flat_argument_checks(nexr, L):
    """test_flat.py's list for nexrFlatAllReduce / ReduceScatter / Reduce, on the host forms."""
    bad, ok = nexr.Result.InvalidArgument, nexr.Result.Success
    F32, SUM, DIV = nexr.DataType.Float32, nexr.DevRedOp.Sum, nexr.DevRedOp.SumPostDiv
    a = _arr([0x1000, 0x2000, 0x3000])
    one = _parts(nexr, [(0, 64, 16)])

    def ar(n=3, ins=a, outs=a, elts=64, dt=F32, op=SUM, arg=0, parts=one, nparts=1):
        return L.nexrFlatHostAllReduce(n, ins, outs, elts, int(dt), int(op), arg, 1, parts, nparts, None)

    def rs(n=3, ins=a, outs=a, elts=64, dt=F32, op=SUM, arg=0):
        return L.nexrFlatHostReduceScatter(n, ins, outs, elts, int(dt), int(op), arg, 1, None)

    def rd(n=3, ins=a, out=0x1000, root=0, elts=64, dt=F32, op=SUM, arg=0):
        return L.nexrFlatHostReduce(n, ins, out, root, elts, int(dt), int(op), arg, 0, None)

    nexr.flat_host_stats(reset=True)
    assert ar(elts=0, parts=None, nparts=0) == ok and rs(elts=0) == ok and rd(elts=0) == ok
    for call in (ar, rs):
        assert call(ins=None) == bad and call(outs=None) == bad
        assert call(ins=_arr([0x1000, None, 0x3000])) == bad and call(outs=_arr([0x1000, 0x2000, None])) == bad
        assert call(outs=_arr([0x1000, 0x2002, 0x3000])) == bad
    assert rd(ins=None) == bad and rd(out=None) == bad and rd(ins=_arr([None, 0x2000, 0x3000])) == bad
    assert rd(out=0x1002) == bad and rd(root=-1) == bad and rd(root=3) == bad
    big = _arr([0x1000] * 65)
    for call in (ar, rs, rd):
        assert call(n=1) == bad and call(n=65, ins=big) == bad
        assert call(dt=nexr.DataType.Float8e4m3) == bad and call(dt=nexr.DataType.Float8e5m2) == bad
        assert call(dt=12) == bad and call(dt=-1) == bad and call(op=5) == bad and call(op=-1) == bad
        assert call(op=DIV) == bad
        assert call(dt=nexr.DataType.Int8, op=DIV, arg=(256 << 1) | 1) == bad
        assert call(ins=_arr([0x1000, 0x2001, 0x3000])) == bad
    assert rs(elts=(1 << 62)) == bad and ar(elts=(1 << 62), parts=_parts(nexr, [(0, 1 << 62, 16)])) == bad
    assert rd(elts=(1 << 62)) == bad
    assert ar(parts=None) == bad and ar(nparts=-1) == bad and ar(nparts=0) == bad
    for parts in ([(0, 32, 16)], [(0, 65, 16)], [(0, 32, 16), (48, 16, 16)], [(0, 48, 16), (32, 32, 16)],
                  [(32, 32, 16), (0, 32, 16)], [(0, 32, 16), (32, 0, 16), (32, 32, 16)], [(0, 30, 16), (30, 34, 16)],
                  [(0, 64, 0)], [(0, 64, 6)], [(0, 64, 1 << 63)], [(4, 60, 16)]):
        assert ar(parts=_parts(nexr, parts), nparts=len(parts)) == bad, parts
    assert ar(dt=nexr.DataType.Uint8, parts=_parts(nexr, [(0, 64, 8)])) == bad
    # nothing above classified a buffer, let alone launched
    assert nexr.flat_host_stats() == dict.fromkeys(nexr.flat_host_stats(), 0)


def test_tree_and_copies_argument_checks(nexr, L):
    """test_flat_tree.py's lists for nexrFlatTreeAllReduce and nexrFlatBroadcast, test_sym_rs_ag.py's for
    nexrSymAllGather, on the host forms."""
    bad, ok = nexr.Result.InvalidArgument, nexr.Result.Success
    F32, SUM, DIV = nexr.DataType.Float32, nexr.DevRedOp.Sum, nexr.DevRedOp.SumPostDiv
    a = _arr([0x1000, 0x2000, 0x3000])
    chain = [(-1, [1]), (0, [2]), (1, [])]
    keep = []

    def trees_of(*trees):
        arr, rows = nexr.flat_tree_links(trees)
        keep.append(rows)
        return arr

    one = _tree_parts(nexr, [(0, 64, 0)])
    T1 = trees_of(chain)

    def ar(n=3, ins=a, outs=a, elts=64, dt=F32, op=SUM, arg=0, trees=T1, ntrees=1, parts=one, nparts=1):
        return L.nexrFlatHostTreeAllReduce(n, ins, outs, elts, int(dt), int(op), arg, 1, trees, ntrees, parts, nparts,
                                           None)

    def empty(**kw):
        return ar(elts=0, parts=None, nparts=0, **kw)

    nexr.flat_host_stats(reset=True)
    assert empty() == ok
    assert ar(ins=None) == bad and ar(outs=None) == bad
    assert ar(ins=_arr([0x1000, None, 0x3000])) == bad and ar(outs=_arr([0x1000, 0x2000, None])) == bad
    assert ar(outs=_arr([0x1000, 0x2002, 0x3000])) == bad and ar(ins=_arr([0x1000, 0x2001, 0x3000])) == bad
    assert ar(n=1) == bad and ar(n=65, ins=_arr([0x1000] * 65)) == bad
    assert ar(dt=nexr.DataType.Float8e4m3) == bad and ar(dt=nexr.DataType.Float8e5m2) == bad
    assert ar(dt=12) == bad and ar(dt=-1) == bad and ar(op=5) == bad and ar(op=-1) == bad and ar(op=DIV) == bad
    assert ar(dt=nexr.DataType.Int8, op=DIV, arg=(256 << 1) | 1) == bad
    assert ar(elts=(1 << 62), parts=_tree_parts(nexr, [(0, 1 << 62, 0)])) == bad
    assert empty(ntrees=0) == bad and empty(ntrees=3) == bad and empty(trees=None) == bad
    null_tree = (ctypes.POINTER(nexr.FlatTreeLinks) * 2)()
    null_tree[0] = T1[0]
    assert empty(trees=null_tree, ntrees=2) == bad
    assert empty(trees=trees_of(chain, oring.tree_topology(3, 1, 1)), ntrees=2) == ok
    for links in ([(-1, [1]), (0, []), (-1, [])], [(1, [1]), (0, [0]), (0, [])], [(-1, [1]), (0, [2]), (0, [])],
                  [(-1, [1, 2]), (0, []), (1, [])], [(-1, []), (2, [2]), (1, [1])], [(-1, [1, 1]), (0, []), (0, [])],
                  [(-1, [-1, 1, 2]), (0, []), (0, [])], [(-1, [1]), (0, [3]), (1, [])], [(-1, [1]), (0, [2]), (5, [])],
                  [(0, [1]), (0, [2]), (1, [])]):
        assert empty(trees=trees_of(links)) == bad, links
    assert ar(parts=None) == bad and ar(nparts=-1) == bad and ar(nparts=0) == bad
    for parts in ([(0, 64, 1)], [(0, 32, 0)], [(0, 65, 0)], [(0, 32, 0), (48, 16, 0)], [(0, 48, 0), (32, 32, 0)],
                  [(32, 32, 0), (0, 32, 0)], [(0, 32, 0), (32, 0, 0), (32, 32, 0)], [(0, 30, 0), (30, 34, 0)],
                  [(4, 60, 0)], [(0, 32, 0), (32, 32, 2)]):
        assert ar(parts=_tree_parts(nexr, parts), nparts=len(parts)) == bad, parts
    # the broadcast
    B = L.nexrFlatHostBroadcast
    assert B(3, 0x1000, a, 0, None) == ok
    assert B(3, 0x1001, _arr([0x1001] * 3), 5, None) == ok          # nothing to write: no launch
    assert B(3, None, a, 0, None) == bad and B(3, 0x1000, None, 0, None) == bad
    assert B(3, 0x1000, _arr([0x1000, None, 0x3000]), 0, None) == bad
    assert B(1, 0x1000, a, 0, None) == bad and B(65, 0x1000, _arr([0x1000] * 65), 0, None) == bad
    # the all-gather
    G = L.nexrFlatHostAllGather
    assert G(3, a, a, 0, None) == ok
    assert G(3, None, a, 0, None) == bad and G(3, a, None, 0, None) == bad
    assert G(3, _arr([0x1000, None, 0x3000]), a, 0, None) == bad and G(3, a, _arr([None, 0x2000, 0x3000]), 0, None) == bad
    assert G(1, a, a, 0, None) == bad and G(65, _arr([0x1000] * 65), _arr([0x1000] * 65), 0, None) == bad
    assert G(3, a, a, (1 << 63), None) == bad                         # nRanks * nBytes overflows
    assert nexr.flat_host_stats() == dict.fromkeys(nexr.flat_host_stats(), 0)


def test_refused_host_memory_communicators(nexr, oracle):
    """A host-memory communicator with a caller's fn and one with LL or LL128 (the caller's step functions) stay
    nexrInvalidUsage for nexrRingCommSetFlat and the six flat entries."""
    ring = importlib.import_module("nex-nccl_amd.ring")
    usage = nexr.Result.InvalidUsage
    F32 = nexr.DataType.Float32
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value

    def refused(comm):
        for kw in ({}, {"tree": True}, {"copies": True}):
            with pytest.raises(nexr.NexrError) as e:
                comm.set_flat(not kw, **kw)
            assert e.value.code == usage
        for call in (lambda: comm.all_reduce_flat([1, 1], [1, 1], 4, F32, 0),
                     lambda: comm.reduce_scatter_flat([1, 1], [1, 1], 4, F32, 0),
                     lambda: comm.reduce_flat([1, 1], [1, 1], 4, F32, 0, 0),
                     lambda: comm.tree_all_reduce_flat([1, 1], [1, 1], 4, F32, 0),
                     lambda: comm.broadcast_flat([1, 1], [1, 1], 4, F32, 0),
                     lambda: comm.all_gather_flat([1, 1], [1, 1], 4, F32)):
            with pytest.raises(nexr.NexrError) as e:
                call()
            assert e.value.code == usage
        assert comm.queued() == 0

    nexr.flat_host_stats(reset=True)
    with ring.RingComm(2, ring.HOST_MEMORY, 8 * 1024, fn) as comm:
        refused(comm)
    # LL and LL128 with the caller's step functions and the library's own fn: the protocol alone refuses them
    ll_fn = ctypes.cast(oracle.lib().oracle_reduce_copy_ll_fn, ctypes.c_void_p).value
    ll128_fn = ctypes.cast(oracle.lib().oracle_reduce_copy_ll128_fn, ctypes.c_void_p).value
    with ring.RingComm(2, ring.HOST_MEMORY, 8 * 16 * 512, None, 0, ring.PROTO_LL, ll_fn, ll128_fn) as comm:
        refused(comm)
    with ring.RingComm(2, ring.HOST_MEMORY, 8 * 2048 * 8, None, 0, ring.PROTO_LL128, ll_fn, ll128_fn) as comm:
        refused(comm)
    assert nexr.flat_host_stats()["calls"] == 0
