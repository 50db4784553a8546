"""nexrFlatAllToAllv and nexrRingAllToAllv without a GPU: every refusal answers before a device call (made-up
addresses that would fault if touched), and a host-memory communicator gives the packed rule under both residences,
through the oracle's step functions and through a recording fn that sees the non-empty blocks in (d, s) order."""
import ctypes
import importlib

import numpy as np
import pytest

import ring_modes_cases as rm

F32, HOST, DEVICE = 7, 1, 0  # nexrFloat32; nexrScalarResidence_t
A, Z, C, S = 0x10000000, 0x20000000, 0x30000000, 0x40000000  # made-up inputs, outputs, device counts, status word
ROW = 0x100 * 4  # bytes of a capacity range in _flat's defaults
RESIDENCES = pytest.mark.parametrize("residence", [HOST, DEVICE], ids=["host-counts", "device-counts"])


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


@pytest.fixture(scope="module")
def fns(oracle):
    L = oracle.lib()
    return [ctypes.cast(f, ctypes.c_void_p).value
            for f in (L.oracle_reduce_copy_fn, L.oracle_reduce_copy_ll_fn, L.oracle_reduce_copy_ll128_fn)]


def _flat(nexr, ins=(A, A + 0x1000), outs=(Z, Z + 0x1000), counts=(0, 0, 0, 0), residence=HOST, esz=4,
          in_elts=(0x100, 0x100), out_elts=(0x100, 0x100), status=0, max_wgs=0, n=None):
    ptrs = lambda ps: None if ps is None else (ctypes.c_void_p * len(ps))(*[p or None for p in ps])  # noqa: E731
    sizes = lambda es: None if es is None else (ctypes.c_size_t * len(es))(*es)  # noqa: E731
    keep = None if counts is None or isinstance(counts, int) else (ctypes.c_uint64 * len(counts))(*counts)
    arg = ctypes.c_void_p(counts) if isinstance(counts, int) else keep and ctypes.cast(keep, ctypes.c_void_p)
    return nexr.lib().nexrFlatAllToAllv(len(ins) if n is None else n, ptrs(ins), ptrs(outs), arg, residence, esz,
                                        sizes(in_elts), sizes(out_elts), ctypes.c_void_p(status) if status else None,
                                        max_wgs, None)


DEV = dict(counts=C, residence=DEVICE, status=S)
FLAT_CASES = {  # the arguments that differ from _flat's; refused unless named accepted (all-zero host counts: no launch)
    "one rank": dict(ins=[A], outs=[Z], counts=[0], in_elts=[4], out_elts=[4]),
    "65 ranks": dict(ins=[A] * 65, outs=[Z] * 65, counts=[0], in_elts=[0] * 65, out_elts=[0] * 65),
    "null inputs": dict(ins=None, n=2),
    "null outputs": dict(outs=None, n=2),
    "null counts": dict(counts=None),
    "null inElts": dict(in_elts=None),
    "null outElts": dict(out_elts=None),
    "a null input with a capacity": dict(ins=[A, 0]),
    "a null output with a capacity": dict(outs=[Z, 0]),
    "esz 3": dict(esz=3),
    "maxWorkgroups < 0": dict(max_wgs=-1),
    "an unknown residence": dict(residence=2),
    "device counts without a status word": dict(DEV, status=0),
    "device counts off 8-byte alignment": dict(DEV, counts=C + 4),
    "a capacity whose bytes overflow": dict(in_elts=[0x100, 2 ** 62]),
    "a capacity above 2**56 bytes": dict(out_elts=[2 ** 54 + 1, 0x100]),
    "one byte of an input in an output": dict(ins=[A, Z + ROW - 1], outs=[Z + ROW, Z]),
    "one byte of an output in an input": dict(outs=[Z, A + ROW - 1]),
    "two outputs meet": dict(outs=[Z, Z + ROW - 1]),
    "device counts in an output": dict(DEV, counts=Z + ROW - 8),
    "the status word in an output": dict(DEV, status=Z + 0x1000 + ROW - 4),
    "a count above its output": dict(counts=[0, 0x101, 0, 0], in_elts=[0x200, 0x100]),
    "a row sum above inElts": dict(counts=[0x80, 0x81, 0, 0]),
    "a column sum above outElts": dict(counts=[0x80, 0, 0x81, 0]),
    "sums that overflow": dict(counts=[2 ** 63, 2 ** 63, 0, 0]),
    "accepted: ranges that end where others begin": dict(ins=[A, Z + ROW], outs=[Z + 2 * ROW, Z]),
    "accepted: null buffers of no capacity": dict(ins=[A, 0], outs=[0, Z], in_elts=[0x100, 0], out_elts=[0, 0x100]),
    "accepted: an empty range inside an output": dict(ins=[A, Z + 8], in_elts=[0x100, 0]),
    "accepted: inputs alias each other": dict(ins=[A, A]),
}


@pytest.mark.parametrize("why", list(FLAT_CASES))
def test_flat_checks_answer_before_any_device_call(nexr, why):
    want = nexr.Result.Success if why.startswith("accepted") else nexr.Result.InvalidArgument
    assert _flat(nexr, **FLAT_CASES[why]) == int(want), why


COUNTS = {1: [[5]], 3: [[2, 0, 5], [0, 0, 7], [1, 0, 0]], 4: [[0, 3, 0, 0], [9, 1, 0, 4], [0, 0, 0, 0], [33, 0, 0, 2]]}


class Host:
    """Seeded inputs and zeroed outputs of float32 with two elements of slack; device counts are host memory here."""
    def __init__(self, n):
        self.byts = np.asarray(COUNTS[n], np.int64) * 4
        rng = np.random.default_rng(rm.SEED + n)
        self.ins = [rng.integers(0, 256, int(r) + 8, dtype=np.uint8).view(np.float32) for r in self.byts.sum(axis=1)]
        self.outs = [np.zeros(int(c) // 4 + 2, np.float32) for c in self.byts.sum(axis=0)]
        self.send_off, self.recv_off = np.cumsum(self.byts, axis=1) - self.byts, np.cumsum(self.byts, axis=0) - self.byts
        self.status = np.full(1, 7, np.uint32)

    def call(self, comm, residence, counts=None, outs=None, dt=F32, status=True):
        self.mat = np.asarray(COUNTS[len(self.ins)] if counts is None else counts, np.uint64).reshape(-1).copy()
        comm.all_to_all_v([a.ctypes.data for a in self.ins], [a.ctypes.data for a in outs or self.outs],
                          [int(c) for c in self.mat] if residence == HOST else self.mat.ctypes.data, dt,
                          [a.size for a in self.ins], [a.size for a in outs or self.outs],
                          self.status.ctypes.data if status else 0)

    def check(self):
        n = len(self.ins)
        for d, out in enumerate(self.outs):
            want = np.concatenate([self.ins[s].view(np.uint8)[self.send_off[s, d]:][:self.byts[s, d]] for s in range(n)])
            got = out.view(np.uint8)
            np.testing.assert_array_equal(got[:want.size], want, err_msg="output %d" % d)
            assert not got[want.size:].any(), "tail of output %d" % d


def host_comm(ring, fns, n, protocol="simple", fn=None):
    return ring.RingComm(n, ring.HOST_MEMORY, rm.BUFF[protocol], fn or fns[0], 20000, rm.PROTO_ID[protocol], fns[1],
                         fns[2], rm.tree_per_node(n), 0, 1)


@RESIDENCES
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
@pytest.mark.parametrize("n", [1, 3, 4])
def test_ring_all_to_all_v_on_host_memory(ring, nexr, fns, protocol, n, residence):
    """Alone, then inside a group: nothing is written before the End, and the call counts as one of `singles`."""
    x = Host(n)
    with host_comm(ring, fns, n, protocol) as comm:
        x.call(comm, residence)
        x.check()
        assert x.status[0] == 0
        x.outs = [np.zeros_like(o) for o in x.outs]
        comm.group_stats(reset=True)
        with comm.group():
            x.call(comm, residence)
            assert not any(o.any() for o in x.outs)
        x.check()
        assert comm.group_stats()["singles"] == 1


@RESIDENCES
def test_a_callers_fn_sees_the_non_empty_blocks_in_order(ring, nexr, fns, residence):
    x, n, seen = Host(4), 4, []

    def record(n_srcs, srcs, n_dsts, dsts, n_elts, datatype, op, arg, n_pre, pre, post, stream):
        seen.append((n_srcs, srcs[0], n_dsts, dsts[0], n_elts, datatype, op))
        ctypes.memmove(dsts[0], srcs[0], n_elts)
        return 0

    fn = ring.REDUCE_COPY_FN(record)
    want = [(1, x.ins[s].ctypes.data + x.send_off[s, d], 1, x.outs[d].ctypes.data + x.recv_off[s, d], x.byts[s, d], 1, 0)
            for d in range(n) for s in range(n) if x.byts[s, d]]  # nexrUint8, nexrDevSum
    with host_comm(ring, fns, n, fn=ctypes.cast(fn, ctypes.c_void_p).value) as comm:
        x.call(comm, residence)
    assert seen == want
    x.check()


def test_ring_refusals(ring, nexr, fns):
    x, bad = Host(3), nexr.Result.InvalidArgument
    over = np.array(COUNTS[3])
    over[2, 1] += 3  # column 1: one element above its capacity of sum + 2
    assert ring.ring_lib().nexrRingAllToAllv(None, None, None, None, HOST, F32, None, None, None) == bad
    with host_comm(ring, fns, 3) as comm:
        assert ring.ring_lib().nexrRingAllToAllv(comm._h, None, None, None, HOST, F32, None, None, None) == bad
        cases = {"fp8": (7, lambda: x.call(comm, HOST, dt=10)),
                 "no such datatype": (7, lambda: x.call(comm, HOST, dt=99)),
                 "in place": (7, lambda: x.call(comm, HOST, outs=x.ins)),
                 "device counts without a status word": (7, lambda: x.call(comm, DEVICE, status=False)),
                 "a column sum above recvElts": (1, lambda: x.call(comm, HOST, counts=over)),
                 "the same, read from the matrix's memory": (1, lambda: x.call(comm, DEVICE, counts=over))}
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
