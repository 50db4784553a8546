"""nexrFlatReduceScatterv / nexrFlatAllGatherv and nexrRingReduceScatterv / nexrRingAllGatherv without a GPU: every
refusal answers before a device call (made-up addresses that would fault if touched), and a host-memory thread-rank
communicator runs the pieces as its own reduce / broadcast calls, bit for bit oracle.ring.reduce_expected with root d
on piece d (numpy concatenation for the all-gather), under host counts and under "device" counts, which are host
memory there."""
import ctypes
import importlib

import numpy as np
import pytest

import arith_edges as ae
import ring_modes_cases as rm
import test_alltoallv as tv
from oracle import ring as oring

HOST, DEVICE = 1, 0  # nexrScalarResidence_t
A, Z = tv.A, tv.Z  # made-up inputs and outputs
RESIDENCES = pytest.mark.parametrize("residence", [HOST, DEVICE], ids=["host-counts", "device-counts"])
KINDS = pytest.mark.parametrize("kind", ["reduce_scatter", "all_gather"])


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


@pytest.fixture(scope="module")
def fns(oracle):
    L = oracle.lib()
    return [ctypes.cast(f, ctypes.c_void_p).value
            for f in (L.oracle_reduce_copy_fn, L.oracle_reduce_copy_ll_fn, L.oracle_reduce_copy_ll128_fn)]


def _flat(nexr, kind, ins=(A, A + 0x1000), outs=(Z, Z + 0x1000), counts=(0, 0), residence=HOST, dt=ae.F32, op=0, arg=0,
          esz=4, in_elts=(0x100, 0x100), out_elts=(0x100, 0x100), status=0, max_wgs=0, n=None):
    ptrs = lambda ps: None if ps is None else (ctypes.c_void_p * len(ps))(*[p or None for p in ps])  # noqa: E731
    sizes = lambda es: None if es is None else (ctypes.c_size_t * len(es))(*es)  # noqa: E731
    keep = None if counts is None or isinstance(counts, int) else (ctypes.c_uint64 * len(counts))(*counts)
    cnt = ctypes.c_void_p(counts) if isinstance(counts, int) else keep and ctypes.cast(keep, ctypes.c_void_p)
    head = (len(ins) if n is None else n, ptrs(ins), ptrs(outs), cnt, residence)
    tail = (sizes(in_elts), sizes(out_elts), ctypes.c_void_p(status) if status else None, max_wgs, None)
    if kind == "reduce_scatter":
        return nexr.lib().nexrFlatReduceScatterv(*head, dt, op, arg, 1, *tail)
    return nexr.lib().nexrFlatAllGatherv(*head, esz, *tail)


# tests/test_alltoallv.py's refusal table but for what is about its n x n matrix (all-zero host counts: no launch)
BOTH_KINDS = {why: how for why, how in tv.FLAT_CASES.items()
              if "sum" not in why and "count above" not in why and why != "esz 3"}
ONE_KIND = {
    ("reduce_scatter", "a count above its output"): dict(counts=[0, 0x101], in_elts=[0x200, 0x200]),
    ("reduce_scatter", "a total above one inElts"): dict(counts=[0x80, 0x81], in_elts=[0x101, 0x100]),
    ("reduce_scatter", "a total that overflows"): dict(counts=[2 ** 63, 2 ** 63]),
    ("reduce_scatter", "fp8"): dict(dt=10),
    ("reduce_scatter", "no such datatype"): dict(dt=99),
    ("reduce_scatter", "no such op"): dict(op=5),
    ("reduce_scatter", "SumPostDiv on a float"): dict(op=ae.SUMPOSTDIV),
    ("reduce_scatter", "an input off element alignment"): dict(ins=[A, A + 0x1002]),
    ("reduce_scatter", "an output off element alignment"): dict(outs=[Z + 1, Z + 0x1000]),
    ("all_gather", "a count above its input"): dict(counts=[0, 0x101], out_elts=[0x200, 0x200]),
    ("all_gather", "a total above one outElts"): dict(counts=[0x80, 0x81], out_elts=[0x100, 0x101]),
    ("all_gather", "esz 3"): dict(esz=3),
    ("all_gather", "accepted: bases off alignment"): dict(ins=[A + 1, A + 0x1003], outs=[Z + 5, Z + 0x1007]),
}
REFUSALS = [(k, why, how) for k in ("reduce_scatter", "all_gather") for why, how in BOTH_KINDS.items()]
REFUSALS += [(k, why, how) for (k, why), how in ONE_KIND.items()]


@pytest.mark.parametrize("kind, why, how", REFUSALS, ids=["%s: %s" % r[:2] for r in REFUSALS])
def test_flat_checks_answer_before_any_device_call(nexr, kind, why, how):
    want = nexr.Result.Success if why.startswith("accepted") else nexr.Result.InvalidArgument
    assert _flat(nexr, kind, **how) == int(want)


COUNTS = {1: [5], 3: [2, 0, 7], 4: [0, 33, 0, 9]}
PAIRS = [(ae.F32, rm.SUM), (ae.BF16, rm.AVG), (ae.I8, rm.MIN), (ae.U64, rm.PROD)]


class Host:
    """Seeded inputs and zeroed outputs with two elements of slack; device counts are host memory here."""

    def __init__(self, kind, n, dt=ae.F32, op=rm.SUM):
        self.kind, self.n, self.dt, self.op, self.counts = kind, n, dt, op, COUNTS[n]
        total, rng, u = sum(self.counts), np.random.default_rng(rm.SEED + n + dt), ae.UINT[dt]
        scatter = kind == "reduce_scatter"
        self.ins = rm.gen_inputs(rng, dt, op, n, total + 2) if scatter else \
            [rm.gen_inputs(rng, dt, None, 1, c + 2)[0] for c in self.counts]
        self.outs = [np.zeros((c if scatter else total) + 2, u) for c in self.counts]
        self.status = np.full(1, 7, np.uint32)

    def call(self, comm, residence, counts=None, outs=None, dt=None, status=True):
        self.vec = np.asarray(self.counts if counts is None else counts, np.uint64).copy()
        outs = outs or self.outs
        args = ([a.ctypes.data for a in self.ins], [a.ctypes.data for a in outs],
                [int(c) for c in self.vec] if residence == HOST else self.vec.ctypes.data,
                self.dt if dt is None else dt)
        caps = ([a.size for a in self.ins], [a.size for a in outs], self.status.ctypes.data if status else 0)
        if self.kind == "reduce_scatter":
            comm.reduce_scatter_v(*args, self.op, *caps)
        else:
            comm.all_gather_v(*args, *caps)

    def check(self, proto):
        off = np.concatenate([[0], np.cumsum(self.counts)])
        for d, out in enumerate(self.outs):
            if self.kind == "reduce_scatter":
                piece = [x[off[d]:off[d + 1]] for x in self.ins]
                want = oring.reduce_expected(piece, self.dt, self.op, d, proto) if self.counts[d] else piece[0]
            else:
                want = np.concatenate([x[:c] for x, c in zip(self.ins, self.counts)])
            np.testing.assert_array_equal(ae.canon(self.dt, out[:want.size]), ae.canon(self.dt, want), "output %d" % d)
            assert not out[want.size:].any(), "tail of output %d" % d


def host_comm(ring, fns, n, protocol="simple"):
    return ring.RingComm(n, ring.HOST_MEMORY, rm.BUFF[protocol], fns[0], 20000, rm.PROTO_ID[protocol], fns[1], fns[2],
                         rm.tree_per_node(n), 0, 1)


@RESIDENCES
@KINDS
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
@pytest.mark.parametrize("n", [1, 3, 4])
def test_pieces_on_host_memory(ring, nexr, oracle, fns, protocol, n, kind, residence):
    """Alone, then inside a group: nothing is written before the End, and the call counts as one of `singles`."""
    dt, op = PAIRS[(n + rm.PROTO_ID[protocol]) % len(PAIRS)]
    x = Host(kind, n, dt, op)
    with host_comm(ring, fns, n, protocol) as comm:
        x.call(comm, residence)
        x.check(protocol)
        assert x.status[0] == 0
        x.outs = [np.zeros_like(o) for o in x.outs]
        comm.group_stats(reset=True)
        with comm.group():
            x.call(comm, residence)
            assert not any(o.any() for o in x.outs)
        x.check(protocol)
        assert comm.group_stats()["singles"] == 1


@KINDS
def test_ring_refusals(ring, nexr, fns, kind):
    x, bad = Host(kind, 3), nexr.Result.InvalidArgument
    over = [2, 0, 10]  # piece 2 (its buffer, or every buffer that holds the total): one element above sum + 2
    entry = getattr(ring.ring_lib(), "nexrRingReduceScatterv" if kind == "reduce_scatter" else "nexrRingAllGatherv")
    nothing = (None, None, None, HOST, ae.F32) + ((rm.SUM,) if kind == "reduce_scatter" else ()) + (None, None, None)
    assert entry(None, *nothing) == bad
    with host_comm(ring, fns, 3) as comm:
        assert entry(comm._h, *nothing) == bad
        cases = {"fp8": (7, lambda: x.call(comm, HOST, dt=10)),
                 "no such datatype": (7, lambda: x.call(comm, HOST, dt=99)),
                 "in place": (7, lambda: x.call(comm, HOST, outs=x.ins)),
                 "device counts without a status word": (7, lambda: x.call(comm, DEVICE, status=False)),
                 "a violation": (1, lambda: x.call(comm, HOST, counts=over)),
                 "the same, read from the counts' memory": (1, lambda: x.call(comm, DEVICE, counts=over))}
        for why, (status, run) in cases.items():
            x.status[0] = 7
            with pytest.raises(nexr.NexrError) as e:
                run()
            assert e.value.code == bad and x.status[0] == status and not any(o.any() for o in x.outs), why
        with comm.group():  # refused at once, not recorded: host counts above a capacity too, with their report
            x.status[0] = 7
            for how in (dict(outs=x.ins), dict(counts=over)):
                with pytest.raises(nexr.NexrError) as e:
                    x.call(comm, HOST, **how)
                assert e.value.code == bad
            assert x.status[0] == 1 and comm.group_stats(reset=True)["calls"] == 0
