"""nexrReduceCopySimpleStepsGroupDirect (reduce_copy_simple_group_direct_kernel, nexr_simple.hip) against the
direct interpreter (tests/simple_direct_model.py), byte for byte: the user buffers whole with guard bytes,
every FIFO byte (pre-filled with a pattern: under the interpreter's mask of written bytes it must hold the
slice, everywhere else the pattern; a direct connection's mask is empty), and the tail and head words of
every workgroup. The lists are the direct ring schedules of the interpreter's module, so the interpreter has
checked the bounds of every direct destination before the device call is made. ONE plain stream, a status
word and a 2 s timeout.

Then the ring option (nexrRingCommSetDirect) against oracle.ring's expected results, host-sequenced and in
group launches, with nexrRingCommGetDirect's counts saying which path ran.

fp32 / fp64 NaNs are compared by class (mg.canon_bytes' rule), everything else exactly."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import ll_steps_cases as cases
import make_golden as mg
import simple_direct_model as dm
import simple_steps_model as model
from simple_direct_cases import DCase, all_reduce_case, types_and_ops_case
from simple_direct_cases import blank as _blank
from oracle.ring import (all_gather_expected, broadcast_expected, reduce_expected, reduce_scatter_expected,
                         ring_allreduce_expected)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TIMEOUT_US = 2_000_000
GUARD = 64
SLOTS = 8
CREDIT = model.CREDIT_BYTES


@pytest.fixture(scope="module")
def stream():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    s = torch.cuda.Stream(device=torch.device("cuda:0"))
    yield s.cuda_stream
    torch.cuda.synchronize()


def all_gather_case(in_place, dt=mg.F16, slot=4096, sps=2, spc=2, n=3, seed=67):
    esz = cases.esz_of(dt)
    step = slot // esz
    per = 2 * step * sps * spc + (16 * 1024 + 6) // esz
    xs = mg.gen_inputs(dt, n, per, seed, special=False)

    def build():
        outs = [_blank(per * n, dt) for _ in range(n)]
        if in_place:
            for r in range(n):
                outs[r][r * per:(r + 1) * per] = xs[r]
        lists = dm.all_gather_lists(n, per, step, in_place, sps, spc)
        return dm.ring_members(lists, outs if in_place else xs, outs, slot, sps, start=4 * sps)
    return DCase(f"all-gather in_place={in_place}", dt, mg.SUM, 0, slot, sps, build)


def broadcast_case(in_place, dt=mg.I8, slot=12288, n=3, root=1, seed=71):
    step = slot // cases.esz_of(dt)
    count = 9 * step + 16 * 1024 + 5
    xs = mg.gen_inputs(dt, n, count, seed, special=False)

    def build():
        outs = [xs[r].copy() if (in_place and r == root) else _blank(count, dt) for r in range(n)]
        ins = [outs[r] if in_place else (xs[r] if r == root else None) for r in range(n)]
        lists = dm.broadcast_lists(n, count, step, root, in_place)
        return dm.ring_members(lists, ins, outs, slot, 1, start=5)
    return DCase(f"broadcast in_place={in_place}", dt, mg.SUM, 0, slot, 1, build)


def mixed_case(dt=mg.F32, slot=4096, seed=73):
    """send -> recv-reduce-copy-send -> recv-reduce-copy, every record permitting both ends: connection 0 is
    direct (into member 1's output), connection 1 uses its FIFO."""
    esz = cases.esz_of(dt)
    cap = slot // esz
    sizes = [cap, 3, 0, cap - 1, (cap // 2) + 1] * 4
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offs[-1]) + 1
    xs = mg.gen_inputs(dt, 3, total, seed, special=True)

    def build():
        conns = [dm.Conn(slot, SLOTS, 3, 1), dm.Conn(slot, SLOTS, 9, 1)]
        a = [dm.DStep(0, int(o), -1, int(o), n, False, True, False, 3) for o, n in zip(offs, sizes)]
        b = [dm.DStep(0, int(o), 1, int(o), n, True, True, False, 3) for o, n in zip(offs, sizes)]
        c = [dm.DStep(0, int(o), 1, int(o), n, True, False, True, 3) for o, n in zip(offs, sizes)]
        m1 = dm.DMember(xs[1], _blank(total, dt), [conns[0]], [conns[1]], b, recv_direct=True)
        m0 = dm.DMember(xs[0], None, [], [conns[0]], a, send_direct=[m1])
        m2 = dm.DMember(xs[2], _blank(total, dt), [conns[1]], [], c)
        return [m0, m1, m2], conns
    return DCase("mixed", dt, mg.SUM, 0, slot, 1, build)


class Rig:
    """The device side of a DCase: user buffers with guards (an in-place member's input IS its output), per
    connection the FIFO, then its tail block, then its head block."""

    def __init__(self, case):
        self.c = case
        off = GUARD + case.misalign
        self.off = off
        self.d_out = [self._guarded(m.output) for m in case.members]
        self.d_in = [self.d_out[i] if (m.input is m.output) else self._guarded(m.input)
                     for i, m in enumerate(case.members)]
        self.d_conn = []
        for c in case.conns:
            host = np.zeros(case.slot * SLOTS + 2 * CREDIT, dtype=np.uint8)
            host[:case.slot * SLOTS] = c.fifo
            self.d_conn.append(torch.from_numpy(host).cuda())
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def _guarded(self, raw):
        if raw is None:
            return None
        host = np.full(raw.size + 2 * GUARD + 16, cases.FILL, dtype=np.uint8)
        host[self.off:self.off + raw.size] = raw
        return torch.from_numpy(host).cuda()

    def _ptr(self, dev):
        return dev.data_ptr() + self.off if dev is not None else 0

    def run(self, nexr, stream, wpm=0, direct=True):
        case = self.c
        before = [c.fifo.copy() for c in case.conns]
        starts = [(c.sent, c.read) for c in case.conns]
        index = {id(c): i for i, c in enumerate(case.conns)}
        fifo_bytes = case.slot * SLOTS
        dm.run(case.members, case.dt, case.op, case.arg)   # also checks every direct destination's bounds

        def conn_arg(c, recv):
            i = index[id(c)]
            p = self.d_conn[i].data_ptr()
            return (p, p + fifo_bytes, p + fifo_bytes + CREDIT, starts[i][1] if recv else starts[i][0])

        args, sets = [], []
        who = {id(m): i for i, m in enumerate(case.members)}
        for m, mb in enumerate(case.members):
            steps = [nexr.ll_step(s.src_buf, s.src_ix, s.dst_buf, s.dst_ix, s.n_elts, recv=s.recv, send=s.send,
                                  post_op=s.post_op, direct=s.direct) for s in mb.steps]
            args.append((self._ptr(self.d_in[m]), self._ptr(self.d_out[m]), [conn_arg(c, True) for c in mb.recv],
                         [conn_arg(c, False) for c in mb.send], steps))
            sets.append(([self._ptr(self.d_out[who[id(t)]]) if t is not None else 0 for t in mb.send_direct],
                         [1 if mb.recv_direct else 0] * len(mb.recv)))
        torch.cuda.synchronize()
        keep = nexr.reduce_copy_simple_steps_group_direct(args, sets if direct else None, case.slot, case.dt, case.op,
                                                          case.arg, n_slots=SLOTS, step_per_slice=case.sps,
                                                          workgroups_per_member=wpm, status=self.status.data_ptr(),
                                                          timeout_us=TIMEOUT_US, stream=stream)
        torch.cuda.synchronize()
        del keep
        self.check(before, wpm)

    def user_bytes(self):
        return [None if d is None else d.cpu().numpy().tobytes() for d in self.d_in + self.d_out]

    def check(self, before, wpm=0):
        case, dt, slot, what = self.c, self.c.dt, self.c.slot, self.c.what
        assert int(self.status.item()) == 0, (what, "status")
        store = mg.STORE[dt]
        for m, mb in enumerate(case.members):
            for name, dev, exp in (("input", self.d_in[m], mb.input), ("output", self.d_out[m], mb.output)):
                if dev is None:
                    continue
                h = dev.cpu().numpy()
                assert (h[:self.off] == cases.FILL).all() and (h[self.off + exp.size:] == cases.FILL).all(), \
                    (what, m, name, "guard")
                got = h[self.off:self.off + exp.size].copy()
                if mg.canon_bytes(dt, got.view(store)) != mg.canon_bytes(dt, exp.view(store)):
                    bad = np.flatnonzero(got != exp)
                    raise AssertionError((what, m, name, "first differing bytes", bad[:8].tolist(), len(bad)))
        g = wpm or model.default_grid(slot, case.sps)
        fifo_bytes = slot * SLOTS
        for i, c in enumerate(case.conns):
            h = self.d_conn[i].cpu().numpy()
            got, exp = h[:fifo_bytes], c.fifo
            if dt in (mg.F32, mg.F64):   # slices start on 16-byte boundaries: elements stay aligned
                wide = np.float32 if dt == mg.F32 else np.float64
                got, exp = got.copy().view(wide), exp.copy().view(wide)
                got[np.isnan(got)] = np.nan
                exp[np.isnan(exp)] = np.nan
                got, exp = got.view(np.uint8), exp.view(np.uint8)
            bad = np.flatnonzero((got != exp) & c.mask)
            assert bad.size == 0, (what, "fifo", i, [(int(b) // slot, int(b) % slot) for b in bad[:6]], bad.size)
            untouched = ~c.mask
            assert (h[:fifo_bytes][untouched] == before[i][untouched]).all(), (what, "bytes no slice sent changed", i)
            tails = h[fifo_bytes:fifo_bytes + CREDIT].view(np.uint64)
            heads = h[fifo_bytes + CREDIT:].view(np.uint64)
            # one word per workgroup at a 16-byte stride: every workgroup has posted every slice, direct or not
            assert tails[0:2 * g:2].tolist() == [c.sent] * g, (what, "tails", i, tails[:2 * g:2].tolist())
            assert not tails[1::2].any(), (what, "between the tail words", i)
            assert heads[0:2 * g:2].tolist() == [c.head] * g, (what, "heads", i, heads[:2 * g:2].tolist())
            assert not heads[1::2].any(), (what, "between the head words", i)


# ---- the kernel against the interpreter ---------------------------------------------------------------------
@pytest.mark.parametrize("slot,sps,spc", [(4096, 1, 1), (4096, 2, 2), (12288, 1, 1), (12288, 2, 1)])
def test_two_member_all_reduce_forty_slices_over_eight_slots(nexr, oracle, stream, slot, sps, spc):
    """40 send slices a connection (10 with 2-slice chunks of 2-step slices: 40 steps), then a last loop whose
    slices end in a partial pack; the credits wrap the 8 slots five times."""
    Rig(all_reduce_case(slot=slot, sps=sps, spc=spc, loops=20 // spc)).run(nexr, stream)


@pytest.mark.parametrize("tail", [0, 3, 1])
def test_all_reduce_with_slices_of_zero_elements(nexr, oracle, stream, tail):
    """A last loop of 3 elements (rank 1's chunk is empty) and of 1; 2-slice chunks: every second slice empty."""
    Rig(all_reduce_case(spc=2, sps=2, loops=2, tail=tail)).run(nexr, stream)


@pytest.mark.parametrize("dt,name", cases.STAR_PAIRS)
def test_all_reduce_types_and_ops(nexr, oracle, stream, dt, name):
    """Every (datatype, op) pair the API accepts: every instance of the kernel is launched."""
    Rig(types_and_ops_case(dt, name)).run(nexr, stream)


@pytest.mark.parametrize("dt", [mg.I8, mg.F16])
def test_user_pointers_one_element_off_alignment(nexr, oracle, stream, dt):
    Rig(all_reduce_case(dt, "sum", loops=2, misalign=cases.esz_of(dt))).run(nexr, stream)


@pytest.mark.parametrize("in_place", [False, True])
def test_three_member_all_gather(nexr, oracle, stream, in_place):
    Rig(all_gather_case(in_place)).run(nexr, stream)


@pytest.mark.parametrize("in_place", [False, True])
def test_three_member_broadcast_chain(nexr, oracle, stream, in_place):
    Rig(broadcast_case(in_place)).run(nexr, stream)


def test_one_direct_connection_and_one_fifo_connection(nexr, oracle, stream):
    Rig(mixed_case()).run(nexr, stream)


def test_workgroups_per_member_one_two_and_default_give_identical_bytes(nexr, oracle, stream):
    seen = []
    for wpm in (1, 2, 0):
        rig = Rig(all_reduce_case(mg.BF16, "sum", slot=12288, sps=2, spc=2, loops=3))
        rig.run(nexr, stream, wpm=wpm)
        seen.append(rig.user_bytes())
    assert seen[0] == seen[1] == seen[2]


def test_direct_sets_of_null_run_the_fifo_call(nexr, oracle, stream):
    """direct = NULL: the records' bits are ignored, every slice goes through its FIFO."""
    case = all_reduce_case(loops=2)
    for mb in case.members:
        mb.send_direct, mb.recv_direct = [None] * len(mb.send), False
    Rig(case).run(nexr, stream, direct=False)
    assert all(c.mask.any() for c in case.conns)


_WORKER = r"""
import importlib, sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import oracle
import make_golden as mg
import test_simple_direct_gpu as t
nexr = importlib.import_module("nex-nccl_amd")
oracle.lib()
s = torch.cuda.Stream(device=torch.device("cuda:0"))
for mode in (1, 2):
    nexr.set_semantics(mode)
    assert nexr.get_semantics() == mode
    with oracle.semantics(mode):
        for dt, name in ((mg.I8, "min"), (mg.I32, "max"), (mg.F16, "premulsum"), (mg.I32, "sumpostdiv")):
            t.Rig(t.all_reduce_case(dt, name, loops=2, n=3)).run(nexr, s.cuda_stream)
        t.Rig(t.mixed_case()).run(nexr, s.cuda_stream)
torch.cuda.synchronize()
print("SEMANTICS-OK")
"""


def test_fork_and_shipped_semantics_in_a_worker_process():
    from conftest import GOLDEN, ROOT
    code = _WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=GOLDEN)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SEMANTICS-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ---- the ring option, device memory -------------------------------------------------------------------------
BUFF = 8 * 4096


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("nex-nccl_amd.ring")


def _want(group):
    return 3 if group and torch.cuda.device_count() == 1 else 0


def _dev(arrs):
    out = [torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() for a in arrs]
    torch.cuda.synchronize()
    return out


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _count(n, esz=4, slots=9, odd=37):
    """More than 8 slots a connection and an odd remainder."""
    return slots * n * (BUFF // 8 // esz) + odd


def _all_reduce(comm, n, dt, count, seed, group, direct=True, in_place=False, ch=1):
    inputs = mg.gen_inputs(dt, n, count, seed, special=True)
    send = _dev(inputs)
    recv = send if in_place else [torch.zeros_like(s) for s in send]
    torch.cuda.synchronize()
    comm.all_reduce(_ptrs(send), _ptrs(recv), count, dt, 0)
    assert comm.queued() == _want(group), (comm.queued(), group)
    d, f = comm.direct_slices()
    assert d + f > 0 and (f == 0 if direct and not in_place else d == 0), (d, f, direct, in_place)
    exp = ring_allreduce_expected(inputs, dt, 0, buff_bytes=BUFF, n_channels=ch)
    for r in range(n):
        assert mg.canon_bytes(dt, recv[r].cpu().numpy()) == mg.canon_bytes(dt, exp[r]), (seed, r)
        if not in_place:
            assert send[r].cpu().numpy().tobytes() == np.asarray(inputs[r]).tobytes(), ("input changed", r)
    return d, f


@pytest.mark.parametrize("group", [False, True])
@pytest.mark.parametrize("n_ranks", [2, 3, 4, 8])
def test_ring_three_all_reduces_in_a_row(ring, oracle, n_ranks, group):
    with ring.RingComm(n_ranks, ring.DEVICE_MEMORY, BUFF, None, 20000) as comm:
        comm.set_direct(True)
        comm.set_simple_group(group)
        seen = set()
        for call in range(3):
            seen.add(_all_reduce(comm, n_ranks, mg.F32, _count(n_ranks), 6100 + 7 * call + n_ranks, group))
        assert len(seen) == 1    # the same schedule: the same slice count every time


@pytest.mark.parametrize("group", [False, True])
@pytest.mark.parametrize("in_place", [False, True])
def test_ring_all_five_collectives_in_a_row(ring, oracle, in_place, group):
    """With the option on: AllGather and Broadcast direct in either placement, AllReduce only out of place,
    Reduce and ReduceScatter never."""
    n, dt, op, root = 4, mg.F32, 0, 1
    count = 4 * 5000 + 4
    per = count // n
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF, None, 20000) as comm:
        comm.set_direct(True)
        comm.set_simple_group(group)
        inputs = mg.gen_inputs(dt, n, count, 6301, special=True)
        send = _dev(inputs)
        rout = send if in_place else [torch.zeros_like(s) for s in send]
        comm.reduce(_ptrs(send), _ptrs(rout), count, dt, op, root)
        d, f = comm.direct_slices()
        assert d == 0 and f > 0 and comm.queued() == _want(group)
        exp = reduce_expected(inputs, dt, op, root)
        assert mg.canon_bytes(dt, rout[root].cpu().numpy()) == mg.canon_bytes(dt, exp), "reduce"
        _all_reduce(comm, n, dt, count, 6300, group, in_place=in_place)
        send = _dev(inputs)
        bout = send if in_place else [torch.zeros_like(s) for s in send]
        comm.broadcast(_ptrs(send), _ptrs(bout), count, dt, root)
        d, f = comm.direct_slices()
        assert d > 0 and f == 0 and comm.queued() == _want(group)
        exp = broadcast_expected(inputs, root)
        for r in range(n):
            assert bout[r].cpu().numpy().tobytes() == np.asarray(exp[r]).tobytes(), ("bcast", r)
        send = _dev(inputs)
        rs = [s[r * per:(r + 1) * per] for r, s in enumerate(send)] if in_place else \
            [torch.zeros(per, dtype=send[0].dtype, device="cuda") for _ in range(n)]
        comm.reduce_scatter(_ptrs(send), _ptrs(rs), per, dt, op)
        d, f = comm.direct_slices()
        assert d == 0 and f > 0 and comm.queued() == _want(group)
        exp = reduce_scatter_expected(inputs, dt, op)
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
        d, f = comm.direct_slices()
        assert d > 0 and f == 0 and comm.queued() == _want(group)
        exp = all_gather_expected([x[:per] for x in inputs])
        for r in range(n):
            assert ag[r].cpu().numpy().tobytes() == exp[r].tobytes(), ("ag", r)


@pytest.mark.parametrize("group", [False, True])
def test_ring_toggling_between_collectives(ring, oracle, group):
    """Direct and FIFO slices share the step counters (and, in group launches, the tail and head words)."""
    n = 3
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF, None, 20000) as comm:
        comm.set_simple_group(group)
        for call, on in enumerate((True, False, True, False, True)):
            comm.set_direct(on)
            _all_reduce(comm, n, mg.F32, _count(n, slots=2, odd=5 + call), 6700 + call, group, direct=on)


@pytest.mark.parametrize("group", [False, True])
def test_ring_four_ranks_two_channels(ring, oracle, group):
    with ring.RingComm(4, ring.DEVICE_MEMORY, BUFF, None, 20000, n_channels=2) as comm:
        comm.set_direct(True)
        comm.set_simple_group(group)
        for call in range(2):
            _all_reduce(comm, 4, mg.F32, 2 * _count(4), 6500 + call, group, ch=2)


@pytest.mark.parametrize("group", [False, True])
def test_ring_bf16_sum_at_eight_ranks(ring, oracle, group):
    with ring.RingComm(8, ring.DEVICE_MEMORY, BUFF, None, 20000) as comm:
        comm.set_direct(True)
        comm.set_simple_group(group)
        _all_reduce(comm, 8, mg.BF16, _count(8, esz=2), 6600, group)


def test_process_ranks_refuse_the_option(ring, nexr):
    name = "/nexr_direct_%d" % os.getpid()
    with ring.PeerRingComm(1, 0, name, device=0, buff_bytes=BUFF, timeout_ms=20000) as comm:
        assert ring.ring_lib().nexrRingCommSetDirect(comm._h, 1) == nexr.Result.InvalidUsage
