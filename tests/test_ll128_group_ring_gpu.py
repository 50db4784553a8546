"""The ring's group launches for LL128 (nexrRingCommSetLLGroup on an LL128 device-memory communicator,
nexrReduceCopyLL128StepsGroup underneath, queued() == 3): every rank and channel of a collective in the
same launches on one stream, the LL128 hand-off ordered inside the kernel. Small FIFOs (8 slots of 4-12
KiB) and counts of a few slots a rank: many steps, FIFO wrap, several loops, a short last one. Every
result is compared with the oracle's LL128 fold order; each fall-back keeps queued() == 0 and exact
results."""
import ctypes
import importlib

import numpy as np
import pytest

import make_golden as mg
from oracle.ring import (all_gather_expected, broadcast_expected, reduce_expected, reduce_scatter_expected,
                         ring_allreduce_expected_ll)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BUFF = 8 * (12 << 10)


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("nex-nccl_amd.ring")


def _want(on=True):
    return 3 if on and torch.cuda.device_count() == 1 else 0


def _dev(arrs):
    out = [torch.from_numpy(a.copy()).cuda() for a in arrs]
    torch.cuda.synchronize()
    return out


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _all_reduce(comm, n, dt, op, count, seed, buff, want, in_place=False, ch=1):
    inputs = mg.gen_inputs(dt, n, count, seed, special=True)
    send = _dev(inputs)
    recv = send if in_place else [torch.zeros_like(s) for s in send]
    torch.cuda.synchronize()
    comm.all_reduce(_ptrs(send), _ptrs(recv), count, dt, op)
    assert comm.queued() == want, (comm.queued(), want)
    exp = ring_allreduce_expected_ll(inputs, dt, op, buff, proto="ll128", n_channels=ch)
    for r in range(n):
        assert mg.canon_bytes(dt, recv[r].cpu().numpy()) == mg.canon_bytes(dt, exp[r]), (seed, r)


@pytest.mark.parametrize("n_ranks", [2, 3, 4, 8])
def test_three_all_reduces_in_a_row(ring, oracle, n_ranks):
    """Three all-reduces on one communicator (at 3 ranks the shape of the queued LL128 failure that kept
    LL128 host-sequenced: third call, rank 0), the last one in place."""
    count = 3 * n_ranks * (BUFF // 8 // 16 * 15 // 4) + 4321
    with ring.RingComm(n_ranks, ring.DEVICE_MEMORY, BUFF, None, 20000, ring.PROTO_LL128) as comm:
        assert comm.queued() == 0
        comm.set_ll_group(True)
        for call in range(3):
            _all_reduce(comm, n_ranks, mg.F32, 0, count, 3100 + 7 * call + n_ranks, BUFF, _want(), in_place=call == 2)


@pytest.mark.parametrize("in_place", [False, True])
def test_all_five_collectives_in_a_row(ring, oracle, in_place):
    n, dt, op, root = 4, mg.BF16, 4, 1
    buff = 8 * 4096
    count = 4 * 9000 + 4
    per = count // n
    with ring.RingComm(n, ring.DEVICE_MEMORY, buff, None, 20000, ring.PROTO_LL128) as comm:
        comm.set_ll_group(True)
        _all_reduce(comm, n, dt, op, count, 3300, buff, _want(), in_place)
        inputs = mg.gen_inputs(dt, n, count, 3301, special=True)
        send = _dev(inputs)
        rs = [s[r * per:(r + 1) * per] for r, s in enumerate(send)] if in_place else \
            [torch.zeros(per, dtype=send[0].dtype, device="cuda") for _ in range(n)]
        comm.reduce_scatter(_ptrs(send), _ptrs(rs), per, dt, op)
        assert comm.queued() == _want()
        exp = reduce_scatter_expected(inputs, dt, op, "ll128")
        for r in range(n):
            assert mg.canon_bytes(dt, rs[r].cpu().numpy()) == mg.canon_bytes(dt, exp[r]), ("rs", r)
        send = _dev(inputs)
        ag = [torch.zeros(per * n, dtype=send[0].dtype, device="cuda") for _ in range(n)]
        if in_place:
            for r in range(n):
                ag[r][r * per:(r + 1) * per] = send[r][:per]
            torch.cuda.synchronize()
        src = [ag[r][r * per:(r + 1) * per].data_ptr() for r in range(n)] if in_place else [s.data_ptr() for s in send]
        comm.all_gather(src, _ptrs(ag), per, dt)
        assert comm.queued() == _want()
        exp = all_gather_expected([x[:per] for x in inputs])
        for r in range(n):
            assert ag[r].cpu().numpy().tobytes() == exp[r].tobytes(), ("ag", r)
        send = _dev(inputs)
        rout = send if in_place else [torch.zeros_like(s) for s in send]
        comm.reduce(_ptrs(send), _ptrs(rout), count, dt, op, root)
        assert comm.queued() == _want()
        exp = reduce_expected(inputs, dt, op, root, "ll128")
        assert mg.canon_bytes(dt, rout[root].cpu().numpy()) == mg.canon_bytes(dt, exp), "reduce"
        send = _dev(inputs)
        bout = send if in_place else [torch.zeros_like(s) for s in send]
        comm.broadcast(_ptrs(send), _ptrs(bout), count, dt, root)
        assert comm.queued() == _want()
        exp = broadcast_expected(inputs, root)
        for r in range(n):
            assert bout[r].cpu().numpy().tobytes() == np.asarray(exp[r]).tobytes(), ("bcast", r)


@pytest.mark.parametrize("n_ranks", [3, 4])
def test_two_channels(ring, oracle, n_ranks):
    count = 60_001
    with ring.RingComm(n_ranks, ring.DEVICE_MEMORY, BUFF, None, 20000, ring.PROTO_LL128, n_channels=2) as comm:
        comm.set_ll_group(True)
        for call in range(2):
            _all_reduce(comm, n_ranks, mg.F32, 0, count, 3500 + call, BUFF, _want(), ch=2)


def test_toggling_the_option_between_collectives(ring, oracle):
    """On, off, on, off, on: host-sequenced steps and group launches keep the same step counters, and every
    group launch re-stores the head words from them."""
    n, count = 3, 50_003
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF, None, 20000, ring.PROTO_LL128) as comm:
        for call, on in enumerate((True, False, True, False, True)):
            comm.set_ll_group(on)
            _all_reduce(comm, n, mg.F32, 0, count, 3700 + call, BUFF, _want(on))


def test_falls_back_when_the_grid_is_not_resident(ring, oracle, monkeypatch):
    n, count = 4, 40_001
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF, None, 20000, ring.PROTO_LL128) as comm:
        comm.set_ll_group(True)
        for call, fits in enumerate((True, False, True)):
            if fits:
                monkeypatch.delenv("NEXR_TEST_LL_GROUP_RESIDENT", raising=False)
            else:
                monkeypatch.setenv("NEXR_TEST_LL_GROUP_RESIDENT", "1")
            _all_reduce(comm, n, mg.F32, 0, count, 3900 + call, BUFF, _want(fits))


def test_falls_back_with_a_callers_ll128_fn(nexr, ring, oracle):
    """A caller's ll128Fn (here the library's own single step under another address than the default's) is
    driven host-sequenced: its kernel is not the one with the ordered hand-off."""
    fn = ctypes.cast(nexr.lib().nexrReduceCopyLL128, ctypes.c_void_p).value
    with ring.RingComm(2, ring.DEVICE_MEMORY, BUFF, None, 20000, ring.PROTO_LL128, None, fn) as comm:
        comm.set_ll_group(True)
        _all_reduce(comm, 2, mg.F32, 0, 30_001, 4100, BUFF, 0)


def test_falls_back_above_thirty_two_members(ring, oracle):
    n, ch, count = 8, 5, 400_003
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF, None, 20000, ring.PROTO_LL128, n_channels=ch) as comm:
        comm.set_ll_group(True)
        _all_reduce(comm, n, mg.F32, 0, count, 4300, BUFF, 0, ch=ch)
