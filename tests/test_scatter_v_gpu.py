"""nexrFlatReduceScatterv / nexrFlatAllGatherv and their ring entries on the MI355X. Piece d of a reduce-scatter-v is
compared bit for bit (float32 / float64 NaNs by class, arith_edges.canon, as everywhere) with
oracle.ring.reduce_expected(piece inputs, datatype, op, root=d, proto), the CPU oracle that pins nexrFlatReduce; the
all-gather-v with numpy concatenation. Every output sits in an arena of BLANK bytes (64 guard bytes, the capacity,
64 guard bytes) of which everything but the written prefix must survive."""
import ctypes
import importlib
import os

import numpy as np
import pytest

import arith_edges as ae
import ring_modes_cases as rm
from oracle import ring as oring

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, BLANK = 64, 0xC3
HOST, DEVICE = 1, 0  # nexrScalarResidence_t
BOTH = pytest.mark.parametrize("residence", [HOST, DEVICE], ids=["host-counts", "device-counts"])
OPS = (rm.SUM, rm.PROD, rm.MIN, rm.MAX, rm.AVG)


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


def vectors(n, esz):
    """One pattern, in windows of n or tiled to n: one element first (under 16 bytes; every later off(d) * esz is off the
    outputs' 16-byte phase), two empty pieces, one pack, five packs and a tail, two 2048-byte items and a few bytes."""
    p = [1, 0, 0, 16 // esz, 80 // esz + 1, 4096 // esz + 3, 3]
    return [[p[(i + k) % len(p)] for k in range(n)] for i in range(0, len(p) if n < len(p) else 1, n)]


class Pieces:
    """Seeded inputs and BLANK output arenas on the device; capacities `slack` elements above what `counts` needs."""

    def __init__(self, nexr, kind, counts, dt, op=rm.SUM, proto="simple", slack=3, rows=None):
        self.nexr, self.scatter, self.dt, self.op, self.proto = nexr, kind == "reduce_scatter", dt, op, proto
        self.n, self.esz, total = len(counts), rm.esz_of(dt), int(sum(counts))
        self.in_elts = [total + slack] * self.n if self.scatter else [int(c) + slack for c in counts]
        self.out_elts = [int(c) + slack for c in counts] if self.scatter else [total + slack] * self.n
        rng = np.random.default_rng(rm.SEED + total + dt)
        self.rows = rows or [rm.gen_inputs(rng, dt, op if self.scatter else None, 1, e)[0] for e in self.in_elts]
        self.ins = [torch.from_numpy(r.view(np.uint8).copy()).cuda() for r in self.rows]
        self.arenas = [torch.full((2 * GUARD + e * self.esz,), BLANK, dtype=torch.uint8).cuda() for e in self.out_elts]
        self.dev_counts = torch.zeros(self.n, dtype=torch.int64).cuda()
        self.status = torch.full((1,), 7, dtype=torch.int32).cuda()

    def pointers(self):
        return [t.data_ptr() for t in self.ins], [a.data_ptr() + GUARD for a in self.arenas]

    def counts_arg(self, counts, residence):
        if residence == HOST:
            return [int(c) for c in counts]
        self.dev_counts.copy_(torch.from_numpy(np.asarray(counts, np.uint64).view(np.int64)).pin_memory(), non_blocking=True)
        return self.dev_counts.data_ptr()

    def call(self, counts, residence, max_workgroups=0, in_elts=None, out_elts=None, stream=None):
        ins, outs = self.pointers()
        arg = self.dev_counts.data_ptr() if counts is None else self.counts_arg(counts, residence)
        tail = (in_elts or self.in_elts, out_elts or self.out_elts, self.status.data_ptr(), max_workgroups, stream)
        if self.scatter:
            dev_op, red_arg = oring.host_to_dev_red_op(self.op, self.dt, self.n)
            self.nexr.flat_reduce_scatter_v(ins, outs, arg, self.dt, dev_op, red_arg, self.proto == "simple", *tail)
        else:
            self.nexr.flat_all_gather_v(ins, outs, arg, self.esz, *tail)

    def expected(self, counts):
        off = np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))])
        if not self.scatter:
            return [np.concatenate([r[:c] for r, c in zip(self.rows, counts)])] * self.n
        return [oring.reduce_expected([r[off[d]:off[d + 1]] for r in self.rows], self.dt, self.op, d, self.proto)
                if counts[d] else self.rows[0][:0] for d in range(self.n)]

    def check(self, counts, arenas=None, status=0):
        for d, (arena, want) in enumerate(zip(arenas or self.arenas, self.expected(counts))):
            got, end = arena.cpu().numpy(), GUARD + want.size * self.esz
            np.testing.assert_array_equal(ae.canon(self.dt, got[GUARD:end]), ae.canon(self.dt, want), "output %d" % d)
            assert (got[:GUARD] == BLANK).all() and (got[end:] == BLANK).all(), "arena of output %d" % d
        if status is not None:
            assert int(self.status.item()) == status

    def blank(self):
        kept = [a.clone() for a in self.arenas]  # stream-ordered copies, then the arenas blank again
        for a in self.arenas:
            a.fill_(BLANK)
        return kept


def run(nexr, kind, counts, dt, residence, op=rm.SUM, max_workgroups=0, **how):
    x = Pieces(nexr, kind, counts, dt, op, **how)
    x.call(counts, residence, max_workgroups)
    torch.cuda.synchronize()
    x.check(counts, status=0 if residence == DEVICE or any(counts) else None)  # no launch, no report


@BOTH
@pytest.mark.parametrize("n", [2, 3, 9, 64])
@pytest.mark.parametrize("kind, dt, op", [("reduce_scatter", ae.F32, rm.SUM), ("reduce_scatter", ae.BF16, rm.AVG),
                                          ("reduce_scatter", ae.I8, rm.MIN), ("all_gather", ae.U8, None),
                                          ("all_gather", ae.U64, None)])
def test_counts_that_reach_every_branch(nexr, oracle, kind, dt, op, n, residence):
    """9 ranks pass flat_fold's group of kSymPeers loads, 64 fill the lanes of the prologue."""
    for counts in vectors(n, rm.esz_of(dt)):
        run(nexr, kind, counts, dt, residence, op)


def edge_rows(dt, n, size):
    s = (np.arange(256).astype(np.uint8) if ae.BITS[dt] == 8 else ae.int_edge_set(dt) if dt in ae.INTS
         else ae.edge_set(dt))
    return [np.resize(np.roll(s, 29 * k), size) for k in range(n)]


@pytest.mark.parametrize("proto", ["simple", "ll"], ids=["user-first", "partial-first"])
@pytest.mark.parametrize("op", OPS, ids=[rm.OP_NAMES[o] for o in OPS])
@pytest.mark.parametrize("dt", range(10), ids=[ae.NAMES[d] for d in range(10)])
def test_every_datatype_and_op_on_edge_operands(nexr, oracle, dt, op, proto):
    """Avg is SumPostDiv on integers and PreMulSum on floats; NaN canonicalisation and the signedness of min / max."""
    counts = [int(c) for c in np.random.default_rng(rm.SEED).integers(1, 160, 3)]
    run(nexr, "reduce_scatter", counts, dt, DEVICE, op, proto=proto, rows=edge_rows(dt, 3, sum(counts) + 3))


@pytest.mark.parametrize("kind, dt", [("reduce_scatter", ae.F16), ("all_gather", ae.U32)])
def test_device_counts_rewritten_between_two_calls(nexr, oracle, kind, dt):
    """The same pointers twice, the counts rewritten on the stream in between, no host synchronisation in between."""
    first, second = [300, 0, 17, 5, 1100], [2, 1100, 0, 300, 9]
    x = Pieces(nexr, kind, np.maximum(first, second), dt)
    x.call(first, DEVICE)
    kept = x.blank()
    x.call(second, DEVICE)
    torch.cuda.synchronize()
    x.check(first, kept, status=None)
    x.check(second)


@pytest.mark.parametrize("kind, dt", [("reduce_scatter", ae.F32), ("all_gather", ae.F16)])
def test_a_captured_graph_replays_over_rewritten_counts(nexr, oracle, kind, dt):
    """One capture, three replays over three count vectors: each equals what the eager call gives for that vector."""
    vecs = [[40, 0, 700, 3], [0, 513, 1, 90], [700, 40, 3, 0]]
    x = Pieces(nexr, kind, np.max(vecs, axis=0), dt)
    x.call(vecs[0], DEVICE)  # eager first: nothing of the library is set up under capture
    torch.cuda.synchronize()
    x.check(vecs[0])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x.call(None, DEVICE, stream=torch.cuda.current_stream().cuda_stream)  # counts None: the buffer as it is
    for counts in vecs[1:] + vecs[:1]:
        x.blank()
        x.counts_arg(counts, DEVICE)
        graph.replay()
        torch.cuda.synchronize()
        x.check(counts)


@pytest.mark.parametrize("kind", ["reduce_scatter", "all_gather"])
@pytest.mark.parametrize("what", ["a count above the capacity of its own buffer", "a total above one shared capacity"])
def test_violations_with_device_counts_write_nothing(nexr, oracle, kind, what):
    counts = [70, 9, 300]
    x = Pieces(nexr, kind, counts, ae.I32, slack=0)
    own, shared = ("out_elts", "in_elts") if kind == "reduce_scatter" else ("in_elts", "out_elts")
    if what.startswith("a count"):
        caps = list(getattr(x, own))
        caps[1] -= 1
        x.call(counts, DEVICE, **{own: caps})
    else:
        caps = list(getattr(x, shared))
        caps[2] -= 1
        x.call(counts, DEVICE, **{shared: caps})
    torch.cuda.synchronize()
    x.check([0, 0, 0], status=1)  # every arena wholly BLANK
    x.call(counts, DEVICE)
    torch.cuda.synchronize()
    x.check(counts, status=0)


@BOTH
@pytest.mark.parametrize("kind, dt", [("reduce_scatter", ae.I64), ("all_gather", ae.U8)])
def test_one_workgroup_strides(nexr, oracle, kind, dt, residence):
    run(nexr, kind, vectors(9, rm.esz_of(dt))[0], dt, residence, rm.PROD, max_workgroups=1)


@BOTH
def test_process_ranks_are_refused(ring, nexr, residence):
    L, buf, counts = ring.ring_lib(), np.zeros(64, np.float32), np.array([4], np.uint64)
    arr, cap = (ctypes.c_void_p * 1)(buf.ctypes.data), (ctypes.c_size_t * 1)(8)
    status = np.full(1, 7, np.uint32)
    with ring.PeerRingComm(1, 0, "/nexr_scatterv_%d_%d" % (residence, os.getpid()), device=0,
                           buff_bytes=rm.BUFF["simple"], timeout_ms=20000) as comm:
        head = (comm._h, arr, arr, counts.ctypes.data, residence, ae.F32)
        assert L.nexrRingReduceScatterv(*head, rm.SUM, cap, cap, status.ctypes.data) == nexr.Result.InvalidUsage
        assert L.nexrRingAllGatherv(*head, cap, cap, status.ctypes.data) == nexr.Result.InvalidUsage
    assert not buf.any() and status[0] == 7


@BOTH
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
@pytest.mark.parametrize("kind, dt, op", [("reduce_scatter", ae.BF16, rm.SUM), ("reduce_scatter", ae.I32, rm.AVG),
                                          ("all_gather", ae.F64, rm.SUM)])
def test_ring_entries_equal_the_calls_on_the_pieces(ring, nexr, oracle, kind, dt, op, protocol, residence):
    """4 ranks in device memory: byte for byte n comm.reduce (root d) / comm.broadcast (root r) calls on the pieces,
    alone and inside a group, where the call is one more of `singles`."""
    n, counts = 4, [33, 0, 1030, 5]
    x = Pieces(nexr, kind, counts, dt, op, protocol)
    ins, outs = x.pointers()
    off = [sum(counts[:d]) * x.esz for d in range(n)]
    with ring.RingComm(n, ring.DEVICE_MEMORY, rm.BUFF[protocol], None, 20000, rm.PROTO_ID[protocol],
                       tree_ranks_per_node=rm.tree_per_node(n), n_channels=1) as comm:
        def entry():
            arg = x.counts_arg(counts, residence)
            torch.cuda.synchronize()  # the communicator's streams are not torch's
            tail = (x.in_elts, x.out_elts, x.status.data_ptr())
            if x.scatter:
                comm.reduce_scatter_v(ins, outs, arg, dt, op, *tail)
            else:
                comm.all_gather_v(ins, outs, arg, dt, *tail)

        torch.cuda.synchronize()
        for d, c in enumerate(counts):  # the reference: the non-empty pieces one by one
            if c and x.scatter:
                comm.reduce([p + off[d] for p in ins], [outs[d]] * n, c, dt, op, d)
            elif c:
                comm.broadcast([ins[d]] * n, [p + off[d] for p in outs], c, dt, d)
        x.check(counts, status=None)
        want, queued = [a.cpu().numpy() for a in x.blank()], comm.queued()
        entry()
        assert comm.queued() == queued and int(x.status.item()) == 0
        alone = [a.cpu().numpy() for a in x.blank()]
        comm.group_stats(reset=True)
        with comm.group():
            entry()
        assert comm.group_stats()["singles"] == 1
        for d in range(n):
            np.testing.assert_array_equal(alone[d], want[d], "alone, output %d" % d)
            np.testing.assert_array_equal(x.arenas[d].cpu().numpy(), want[d], "in a group, output %d" % d)
