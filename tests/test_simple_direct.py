"""DirectWrite for SIMPLE, the parts that need no GPU: every rejection of
nexrReduceCopySimpleStepsGroupDirect before a device call, the ring option's usage errors, and host-memory
rings with the oracle's reduce-copy as `fn` behind a trampoline that records every call: exact against
oracle/ring.py, the slice counts nexrRingCommGetDirect reports, no FIFO address among the recorded
destinations, and fewer calls than through FIFOs by the number of directRecv slices."""
import ctypes
import importlib
import threading

import numpy as np
import pytest

import make_golden as mg
import simple_direct_model as dm
from oracle.ring import (all_gather_expected, broadcast_expected, reduce_expected, reduce_scatter_expected,
                         ring_allreduce_expected)

F32 = mg.F32
BUFF = 8 * 1024          # 1 KiB steps
STEP = BUFF // 8 // 4    # fp32 elements per step


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


# ---- the group call's checks ----------------------------------------------------------------------------------
SLOT = 4096
WS = (0x10000, 1 << 20)   # never dereferenced: every case below returns before the workspace is used


def _bufs():
    """Two user buffers and one connection's FIFO + credit blocks, host memory (only addresses are used)."""
    return [np.zeros(4096, dtype=np.uint8) for _ in range(4)], np.zeros(SLOT * 8 + 8192 + 64, dtype=np.uint8)


def _pair(nexr, out1, fifo_arr, send_bits=3, recv_bits=3):
    """Member 0 sends 16 floats into member 1, which reduces them into its output."""
    p = (fifo_arr.ctypes.data + 15) & ~15
    conn = (p, p + SLOT * 8, p + SLOT * 8 + 4096, 0)
    a = [nexr.ll_step(0, 0, -1, 0, 16, send=True, direct=send_bits)]
    b = [nexr.ll_step(0, 0, 1, 0, 16, recv=True, direct=recv_bits)]
    return conn, a, b


def _call(nexr, members, direct, **kw):
    try:
        nexr.reduce_copy_simple_steps_group_direct(members, direct, SLOT, F32, 0, workspace=kw.pop("workspace", WS), **kw)
    except nexr.NexrError as e:
        return e.code
    return 0


def test_group_call_rejections_come_before_any_device_call(nexr):
    (i0, i1, o1, other), fifo = _bufs()
    conn, a, b = _pair(nexr, o1, fifo)
    m0 = (i0.ctypes.data, 0, [], [conn], a)
    m1 = (i1.ctypes.data, o1.ctypes.data, [conn], [], b)
    out1 = o1.ctypes.data
    bad = nexr.Result.InvalidArgument
    # an internal connection direct on one end only
    assert _call(nexr, [m0, m1], [([out1], []), ([], [0])]) == bad
    assert _call(nexr, [m0, m1], [([0], []), ([], [1])]) == bad
    # sendDirect is not the receiver's output
    assert _call(nexr, [m0, m1], [([other.ctypes.data], []), ([], [1])]) == bad
    assert _call(nexr, [m0, m1], [([out1 + 4], []), ([], [1])]) == bad
    # recvDirect with nRecv != 1, or set on a connection the member does not have
    p2 = conn[0]
    two = (i1.ctypes.data, out1, [conn, (p2, conn[1], conn[2], 0)], [], b)
    assert _call(nexr, [two], [([], [1, 0])]) == bad
    none = (i1.ctypes.data, out1, [], [], [nexr.ll_step(0, 0, 1, 0, 16)])
    assert _call(nexr, [none], [([], [1])]) == bad
    assert _call(nexr, [m1], [([], [0, 1])]) == bad
    # recvDirect without an output
    no_out = (i1.ctypes.data, 0, [conn], [(conn[0] + 64, conn[1], conn[2], 0)],
              [nexr.ll_step(0, 0, -1, 0, 16, recv=True, send=True, direct=3)])
    assert _call(nexr, [no_out], [([0], [1])]) == bad
    # the existing checks still apply with direct sets: a misaligned FIFO, a slice larger than its slots
    odd = (conn[0] + 8, conn[1], conn[2], 0)
    assert _call(nexr, [(i0.ctypes.data, 0, [], [odd], a)], [([0], [])]) == bad
    big = [nexr.ll_step(0, 0, -1, 0, SLOT // 4 + 1, send=True, direct=2)]
    assert _call(nexr, [(i0.ctypes.data, 0, [], [conn], big)], [([out1], [])]) == bad
    # a valid direct pair gets as far as the workspace: too small a one is refused, still before the device
    assert _call(nexr, [m0, m1], [([out1], []), ([], [1])], workspace=(0x10000, 8)) == bad


def test_direct_null_is_accepted_wherever_the_existing_call_is(nexr):
    (i0, i1, o1, _other), fifo = _bufs()
    conn, a, b = _pair(nexr, o1, fifo)
    empty0 = (i0.ctypes.data, 0, [], [conn], [])
    empty1 = (i1.ctypes.data, o1.ctypes.data, [conn], [], [])
    assert _call(nexr, [empty0, empty1], None) == 0                       # nothing to do: no workspace, no device
    assert _call(nexr, [empty0, empty1], [([o1.ctypes.data], []), ([], [1])]) == 0
    m0 = (i0.ctypes.data, 0, [], [conn], a)
    m1 = (i1.ctypes.data, o1.ctypes.data, [conn], [], b)
    for members, kw in (([m0, m1], dict(workspace=(0x10000, 8))),          # the workspace of the FIFO call's size rule
                        ([m0, m1], dict(workgroups_per_member=257)),
                        ([m0, m1], dict(step_per_slice=3)),
                        ([m0] * 33, {})):
        want = None
        try:
            nexr.reduce_copy_simple_steps_group(members, SLOT, F32, 0, **dict(dict(workspace=WS), **kw))
        except nexr.NexrError as e:
            want = e.code
        assert want is not None and _call(nexr, members, None, **kw) == want
    # and the two size functions: the direct table entry is larger, the FIFO one's answers are as they were
    assert nexr.simple_group_direct_workspace_bytes(2) > nexr.simple_group_workspace_bytes(2)


def test_set_direct_usage_errors(nexr, oracle, ring):
    """LL and LL128 communicators refuse the option; SIMPLE thread ranks in host memory take it. (Process ranks
    need a GPU: tests/test_simple_direct_gpu.py.)"""
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value
    ll_fn = ctypes.cast(oracle.lib().oracle_reduce_copy_ll_fn, ctypes.c_void_p).value
    ll128_fn = ctypes.cast(oracle.lib().oracle_reduce_copy_ll128_fn, ctypes.c_void_p).value
    for kw in (dict(protocol=ring.PROTO_LL, ll_fn_address=ll_fn), dict(protocol=ring.PROTO_LL128, ll128_fn_address=ll128_fn)):
        with ring.RingComm(2, ring.HOST_MEMORY, 0, fn, 20000, **kw) as comm:
            for on in (True, False):
                with pytest.raises(nexr.NexrError) as e:
                    comm.set_direct(on)
                assert e.value.code == nexr.Result.InvalidUsage
    with ring.RingComm(2, ring.HOST_MEMORY, BUFF, fn, 20000) as comm:
        comm.set_direct(True)
        comm.set_direct(False)
        assert comm.direct_slices() == (0, 0)
    L = ring.ring_lib()
    assert L.nexrRingCommSetDirect(None, 1) == 4
    d = ctypes.c_uint64()
    assert L.nexrRingCommGetDirect(None, ctypes.byref(d), ctypes.byref(d)) == 4


# ---- host-memory rings ---------------------------------------------------------------------------------------
_ARGS = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
         ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]


class Recorder:
    """A nexrReduceCopyFn that forwards to the oracle and keeps (srcs, dsts, n) of every call."""

    def __init__(self, oracle):
        self.target = oracle.lib().oracle_reduce_copy_fn
        self.target.argtypes, self.target.restype = _ARGS, ctypes.c_int
        self.calls, self.lock = [], threading.Lock()
        self.cb = ctypes.CFUNCTYPE(ctypes.c_int, *_ARGS)(self._call)

    def _call(self, n_srcs, srcs, n_dsts, dsts, n, *rest):
        s = list((ctypes.c_void_p * n_srcs).from_address(srcs))
        d = list((ctypes.c_void_p * n_dsts).from_address(dsts))
        with self.lock:
            self.calls.append((s, d, n))
        return self.target(n_srcs, srcs, n_dsts, dsts, n, *rest)

    @property
    def address(self):
        return ctypes.cast(self.cb, ctypes.c_void_p).value

    def take(self):
        with self.lock:
            out, self.calls = self.calls, []
        return out


def _ptrs(arrs):
    return [a.ctypes.data for a in arrs]


def _in_user(calls, arrs):
    """Every recorded destination lies inside one of the user arrays (so: no FIFO address)."""
    spans = [(a.ctypes.data, a.ctypes.data + a.nbytes) for a in arrs]
    return all(any(lo <= d < hi for lo, hi in spans) for _s, ds, _n in calls for d in ds)


@pytest.mark.parametrize("n", [2, 3, 5])
def test_all_reduce_out_of_place(nexr, oracle, ring, n):
    rec = Recorder(oracle)
    count = 2 * n * STEP * 4 + n * 40 + 5
    xs = mg.gen_inputs(F32, n, count, 1200 + n, special=True)
    exp = ring_allreduce_expected(xs, F32, 0, buff_bytes=BUFF)
    lists = dm.all_reduce_lists(n, count, 4, STEP, 2, 2)
    sends = sum(1 for L in lists for s in L.steps if s.send)
    recv_only = sum(L.direct_recv_only for L in lists)
    with ring.RingComm(n, ring.HOST_MEMORY, BUFF, rec.address, 20000) as comm:
        out = [np.zeros(count, dtype=np.float32) for _ in range(n)]
        comm.all_reduce(_ptrs(xs), _ptrs(out), count, F32, 0)
        fifo_calls = rec.take()
        assert comm.direct_slices() == (0, sends)
        comm.set_direct(True)
        out = [np.zeros(count, dtype=np.float32) for _ in range(n)]
        comm.all_reduce(_ptrs(xs), _ptrs(out), count, F32, 0)
        calls = rec.take()
        assert comm.direct_slices() == (sends, 0)
        for r in range(n):
            assert mg.canon_bytes(F32, out[r]) == mg.canon_bytes(F32, exp[r]), r
        assert _in_user(calls, out) and not _in_user(fifo_calls, out)
        assert len(calls) == len(fifo_calls) - recv_only and recv_only > 0
        # in place: the reduce-scatter half would overwrite the inputs, so it runs through the FIFOs
        io = [x.copy() for x in xs]
        comm.all_reduce(_ptrs(io), _ptrs(io), count, F32, 0)
        assert comm.direct_slices() == (0, sends)
        for r in range(n):
            assert mg.canon_bytes(F32, io[r]) == mg.canon_bytes(F32, exp[r]), r
        # off and on again on the same communicator
        for on in (False, True):
            comm.set_direct(on)
            out = [np.zeros(count, dtype=np.float32) for _ in range(n)]
            comm.all_reduce(_ptrs(xs), _ptrs(out), count, F32, 0)
            assert comm.direct_slices() == ((sends, 0) if on else (0, sends))
            for r in range(n):
                assert mg.canon_bytes(F32, out[r]) == mg.canon_bytes(F32, exp[r]), (on, r)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_all_gather(nexr, oracle, ring, n, in_place):
    rec = Recorder(oracle)
    per = 2 * STEP * 4 + 37
    xs = mg.gen_inputs(F32, n, per, 1300 + n, special=False)
    exp = all_gather_expected(xs)
    lists = dm.all_gather_lists(n, per, STEP, in_place, 2, 2)
    sends = sum(1 for L in lists for s in L.steps if s.send)
    recv_only = sum(L.direct_recv_only for L in lists)

    def run(comm):
        out = [np.zeros(per * n, dtype=np.float32) for _ in range(n)]
        if in_place:
            for r in range(n):
                out[r][r * per:(r + 1) * per] = xs[r]
        src = [out[r][r * per:].ctypes.data for r in range(n)] if in_place else _ptrs(xs)
        comm.all_gather(src, _ptrs(out), per, F32)
        return out

    with ring.RingComm(n, ring.HOST_MEMORY, BUFF, rec.address, 20000) as comm:
        run(comm)
        fifo_calls = rec.take()
        comm.set_direct(True)
        out = run(comm)
        calls = rec.take()
        assert comm.direct_slices() == (sends, 0)
        for r in range(n):
            assert out[r].tobytes() == exp[r].tobytes(), r
        assert _in_user(calls, out)
        assert len(calls) == len(fifo_calls) - recv_only and recv_only > 0


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_broadcast_from_every_root(nexr, oracle, ring, n, in_place):
    rec = Recorder(oracle)
    count = 5 * STEP + 3
    xs = mg.gen_inputs(F32, n, count, 1400 + n, special=False)
    with ring.RingComm(n, ring.HOST_MEMORY, BUFF, rec.address, 20000) as comm:
        for root in range(n):
            exp = broadcast_expected(xs, root)
            lists = dm.broadcast_lists(n, count, STEP, root, in_place)
            sends = sum(1 for L in lists for s in L.steps if s.send)
            recv_only = sum(L.direct_recv_only for L in lists)
            got = {}
            for on in (False, True):
                comm.set_direct(on)
                out = [xs[r].copy() if (in_place and r == root) else np.zeros(count, dtype=np.float32) for r in range(n)]
                src = _ptrs(out) if in_place else _ptrs(xs)
                comm.broadcast(src, _ptrs(out), count, F32, root)
                got[on] = rec.take()
                assert comm.direct_slices() == ((sends, 0) if on else (0, sends)), (root, on)
                for r in range(n):
                    assert out[r].tobytes() == np.asarray(exp[r]).tobytes(), (root, on, r)
                if on:
                    assert _in_user(got[on], out)
            assert len(got[True]) == len(got[False]) - recv_only and recv_only > 0


@pytest.mark.parametrize("n", [2, 3, 5])
def test_reduce_and_reduce_scatter_never_run_direct(nexr, oracle, ring, n):
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value
    per = STEP * 4 + 21
    count = per * n
    xs = mg.gen_inputs(F32, n, count, 1500 + n, special=True)
    with ring.RingComm(n, ring.HOST_MEMORY, BUFF, fn, 20000) as comm:
        comm.set_direct(True)
        out = [np.zeros(count, dtype=np.float32) for _ in range(n)]
        comm.reduce(_ptrs(xs), _ptrs(out), count, F32, 0, 1)
        d, f = comm.direct_slices()
        assert d == 0 and f > 0
        assert mg.canon_bytes(F32, out[1]) == mg.canon_bytes(F32, reduce_expected(xs, F32, 0, 1))
        rs = [np.zeros(per, dtype=np.float32) for _ in range(n)]
        comm.reduce_scatter(_ptrs(xs), _ptrs(rs), per, F32, 0)
        d, f = comm.direct_slices()
        assert d == 0 and f > 0
        exp = reduce_scatter_expected(xs, F32, 0)
        for r in range(n):
            assert mg.canon_bytes(F32, rs[r]) == mg.canon_bytes(F32, exp[r]), r
