"""nexrReduceCopySimpleStepsGroup (reduce_copy_simple_group_kernel, nexr_simple.hip) against the sequential
interpreter of SIMPLE step lists (tests/simple_steps_model.py), byte for byte: the user buffers whole with
guard bytes, every FIFO byte under the interpreter's mask of written bytes (the rest must be as it was),
and the tail and head words of every workgroup. The step lists are tests/simple_steps_cases.py's.
Everything runs on ONE plain stream with a status word and a 2 s timeout (50 ms where the timeout is the
expected outcome). Small slots and many slices: a slot re-read after a FIFO wrap is where a missing
acquire shows stale bytes.

Then the ring option (nexrRingCommSetSimpleGroup, queued() == 3) against oracle.ring's expected results.

fp32 / fp64 NaNs are compared by class (mg.canon_bytes' rule, as everywhere in the suite), in the user
buffers and in the FIFOs; everything else exactly."""
import importlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import ll_steps_cases as cases
import make_golden as mg
import simple_steps_cases as sc
import simple_steps_model as model
from oracle.ring import (all_gather_expected, broadcast_expected, reduce_expected, reduce_scatter_expected,
                         ring_allreduce_expected)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S = model.Step
TIMEOUT_US = 2_000_000
GUARD = 64
SLOTS = cases.SLOTS
CREDIT = model.CREDIT_BYTES


@pytest.fixture(scope="module")
def stream():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    s = torch.cuda.Stream(device=torch.device("cuda:0"))
    yield s.cuda_stream
    torch.cuda.synchronize()


def _canon(dt, raw):
    """NaNs made one NaN for fp32 / fp64 (slices start on 16-byte boundaries: elements stay aligned)."""
    if dt not in (mg.F32, mg.F64):
        return raw
    v = raw.copy().view(np.float32 if dt == mg.F32 else np.float64)
    v[np.isnan(v)] = np.nan
    return v.view(np.uint8)


class Rig:
    """The device side of a SimpleCase, kept over several calls: user buffers with guards; per connection the
    FIFO, then its tail block, then its head block."""

    def __init__(self, scase):
        self.scase, self.case, self.sps = scase, scase.case, scase.step_per_slice
        case = self.case
        self.slot = case.slot_bytes
        self.members, self.conns = model.model(case, self.sps)
        self.has_receiver = {i for m in case.members for i in m.recv}
        self.has_sender = {i for m in case.members for i in m.send}
        self.d_in = [self._guarded(m.input) if m.input is not None else None for m in case.members]
        self.d_out = [self._guarded(m.output) if m.output is not None else None for m in case.members]
        self.d_conn = []
        for i, c in enumerate(self.conns):
            host = np.zeros(self.slot * SLOTS + 2 * CREDIT, dtype=np.uint8)
            host[:self.slot * SLOTS] = c.fifo
            if i not in self.has_sender:   # its sender, elsewhere, has published what it wrote
                host[self.slot * SLOTS:self.slot * SLOTS + CREDIT].view(np.uint64)[:] = c.sent
            self.d_conn.append(torch.from_numpy(host).cuda())
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")

    @staticmethod
    def _guarded(a):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        host = np.full(raw.size + 2 * GUARD, cases.FILL, dtype=np.uint8)
        host[GUARD:GUARD + raw.size] = raw
        return torch.from_numpy(host).cuda()

    def run(self, nexr, stream, step_lists=None, wpm=0, timeout_us=TIMEOUT_US, check=True):
        """One group call of step_lists (default: the case's) from the connections' counters as they stand;
        the interpreter runs the same lists; then everything is compared."""
        case = self.case
        before = [c.fifo.copy() for c in self.conns]
        starts = [(c.sent, c.read) for c in self.conns]
        if step_lists is not None:
            for mb, steps in zip(self.members, step_lists):
                mb.steps = [S(*s) for s in steps]
        model.run(self.members, case.dt, case.op, case.arg)
        fifo_bytes = self.slot * SLOTS
        for i, c in enumerate(self.conns):  # a receiver elsewhere has released everything this call will send
            if i not in self.has_receiver:
                self.d_conn[i][fifo_bytes + CREDIT:].view(torch.int64)[:] = c.sent

        def conn_arg(i, recv):
            p = self.d_conn[i].data_ptr()
            return (p, p + fifo_bytes, p + fifo_bytes + CREDIT, starts[i][1] if recv else starts[i][0])

        args = []
        for m, spec in enumerate(case.members):
            steps = [nexr.ll_step(s.src_buf, s.src_ix, s.dst_buf, s.dst_ix, s.n_elts, recv=s.recv, send=s.send,
                                  post_op=s.post_op) for s in self.members[m].steps]
            args.append((self.d_in[m].data_ptr() + GUARD if self.d_in[m] is not None else 0,
                         self.d_out[m].data_ptr() + GUARD if self.d_out[m] is not None else 0,
                         [conn_arg(i, True) for i in spec.recv], [conn_arg(i, False) for i in spec.send], steps))
        self.status.zero_()
        torch.cuda.synchronize()
        keep = nexr.reduce_copy_simple_steps_group(args, self.slot, case.dt, case.op, case.arg, n_slots=SLOTS,
                                                   step_per_slice=self.sps, workgroups_per_member=wpm,
                                                   status=self.status.data_ptr(), timeout_us=timeout_us, stream=stream)
        torch.cuda.synchronize()
        del keep
        if check:
            self.check(before, wpm)

    def user_bytes(self):
        out = []
        for m in range(len(self.members)):
            for dev in (self.d_in[m], self.d_out[m]):
                out.append(None if dev is None else dev.cpu().numpy().tobytes())
        return out

    def check(self, before, wpm=0):
        case, dt, slot, what = self.case, self.case.dt, self.slot, self.scase.what
        assert int(self.status.item()) == 0, (what, "status")
        store = mg.STORE[dt]
        for m, mb in enumerate(self.members):
            for name, dev, exp in (("input", self.d_in[m], mb.input), ("output", self.d_out[m], mb.output)):
                if dev is None:
                    continue
                h = dev.cpu().numpy()
                assert (h[:GUARD] == cases.FILL).all() and (h[GUARD + exp.size:] == cases.FILL).all(), (what, m, name, "guard")
                got = h[GUARD:GUARD + exp.size]
                if mg.canon_bytes(dt, got.view(store)) != mg.canon_bytes(dt, exp.view(store)):
                    bad = np.flatnonzero(got != exp)
                    raise AssertionError((what, m, name, "first differing bytes", bad[:8].tolist(), len(bad)))
        g = wpm or model.default_grid(slot, self.sps)
        fifo_bytes = slot * SLOTS
        for i, c in enumerate(self.conns):
            h = self.d_conn[i].cpu().numpy()
            got, exp = _canon(dt, h[:fifo_bytes]), _canon(dt, c.fifo)
            bad = np.flatnonzero((got != exp) & c.mask)
            assert bad.size == 0, (what, "fifo", i, "(slot, byte) of the first differing bytes",
                                   [(int(b) // slot, int(b) % slot) for b in bad[:6]], bad.size)
            untouched = ~c.mask
            assert (h[:fifo_bytes][untouched] == before[i][untouched]).all(), (what, "bytes no slice sent changed", i)
            tails = h[fifo_bytes:fifo_bytes + CREDIT].view(np.uint64)
            heads = h[fifo_bytes + CREDIT:].view(np.uint64)
            # one word per workgroup at a 16-byte stride: every workgroup has posted every slice, with or without a tile
            if i in self.has_sender:
                assert tails[0:2 * g:2].tolist() == [c.sent] * g, (what, "tails", i, tails[:2 * g:2].tolist())
                assert not tails[1::2].any(), (what, "between the tail words", i)
            else:
                assert (tails == c.sent).all(), (what, "the sender's tail words were written", i)
            if i in self.has_receiver:
                assert heads[0:2 * g:2].tolist() == [c.head] * g, (what, "heads", i, heads[:2 * g:2].tolist())
                assert not heads[1::2].any(), (what, "between the head words", i)
            else:
                assert (heads == c.sent).all(), (what, "the receiver's head words were written", i)


# ---- 1 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sps", [1, 2])
def test_forty_slices_over_eight_slots(nexr, oracle, stream, sps):
    """Send -> recv-reduce-copy with fresh data in every slice; every slot is re-read after each wrap."""
    Rig(sc.pair_case(sps)).run(nexr, stream)


# ---- 2 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,name", sc.CHAIN_PAIRS)
def test_three_member_chain(nexr, oracle, stream, dt, name):
    Rig(sc.chain_case(dt, name)).run(nexr, stream)


def test_three_member_chain_with_two_step_slices(nexr, oracle, stream):
    Rig(sc.chain_case(mg.BF16, "sum", sps=2, slot=512, n_slices=24)).run(nexr, stream)


# ---- 3 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,name", cases.STAR_PAIRS)
def test_the_fan_of_four_sources_and_four_destinations(nexr, oracle, stream, dt, name):
    Rig(sc.fan_case(dt, name)).run(nexr, stream)


# ---- 4 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [mg.I8, mg.F16])
def test_user_pointers_off_by_one_element(nexr, oracle, stream, dt):
    Rig(sc.offset_case(dt)).run(nexr, stream)


# ---- 5 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wpm", [0, 2])
def test_one_ended_connections(nexr, oracle, stream, wpm):
    """The "run" form: FIFO and tail words from the host; afterwards the head words hold what the
    interpreter says, the tail words of the send connection too (Rig.check), also for a workgroup that
    owns no tile of any slice (wpm = 2 at one tile a slice)."""
    Rig(sc.one_ended_case()).run(nexr, stream, wpm=wpm)


# ---- 6 -----------------------------------------------------------------------------------------------------
def test_launch_cuts_leave_the_results_unchanged(nexr, oracle, stream):
    Rig(sc.cut_case()).run(nexr, stream)
    Rig(sc.long_case()).run(nexr, stream)


def test_counters_carried_over_three_calls(nexr, oracle, stream):
    """The same rig, three calls: each starts at the counters the last one left (and re-stores its words)."""
    scase = sc.pair_case(2, n_slices=9)
    rig = Rig(scase)
    lists = [m.steps for m in scase.case.members]
    for call in range(3):
        rig.run(nexr, stream, [lists[0][3 * call:3 * call + 3], lists[1][3 * call:3 * call + 3]])


# ---- 7 -----------------------------------------------------------------------------------------------------
def test_workgroups_per_member_one_two_and_default_give_identical_bytes(nexr, oracle, stream):
    seen = []
    for wpm in (1, 2, 0):
        rig = Rig(sc.grid_case())
        rig.run(nexr, stream, wpm=wpm)
        seen.append((rig.user_bytes(), [d[:rig.slot * SLOTS].cpu().numpy().tobytes() for d in rig.d_conn]))
    assert seen[0] == seen[1] == seen[2]
    rig = Rig(sc.pair_case(2, n_slices=12))
    rig.run(nexr, stream, wpm=1)


# ---- 8 -----------------------------------------------------------------------------------------------------
_WORKER = r"""
import importlib, sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import oracle
import simple_steps_cases as sc
import test_simple_group_gpu as t
nexr = importlib.import_module("nex-nccl_amd")
oracle.lib()
s = torch.cuda.Stream(device=torch.device("cuda:0"))
for mode in (1, 2):
    nexr.set_semantics(mode)
    assert nexr.get_semantics() == mode
    with oracle.semantics(mode):
        for scase in sc.semantics_cases():
            t.Rig(scase).run(nexr, s.cuda_stream)
torch.cuda.synchronize()
print("SEMANTICS-OK")
"""


def test_fork_and_shipped_semantics_in_a_worker_process():
    from conftest import GOLDEN, ROOT
    code = _WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=GOLDEN)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "SEMANTICS-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ---- 9 -----------------------------------------------------------------------------------------------------
def test_a_tail_that_never_comes_ends_the_group_within_its_timeout(nexr, oracle, stream):
    """One member receives on a one-ended connection nobody publishes (the dry run takes it as ready: its
    peer is outside the group); the other member only copies. Every poll is bounded: the stream completes,
    the shared status word is 1, and no slice's output of the waiting member is written. A valid group call
    on the same stream right after it is exact."""
    slot, per = 4096, 1024
    conn = torch.zeros(slot * SLOTS + 2 * CREDIT, dtype=torch.uint8, device="cuda")
    p = conn.data_ptr()
    x = torch.ones(6 * per, dtype=torch.float32, device="cuda")
    out = torch.zeros_like(x)
    y = torch.arange(5000, dtype=torch.float32, device="cuda")
    yout = torch.zeros_like(y)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.time()
    _ws = nexr.reduce_copy_simple_steps_group(
        [(x.data_ptr(), out.data_ptr(), [(p, p + slot * SLOTS, p + slot * SLOTS + CREDIT, 0)], [],
          [nexr.ll_step(0, k * per, 1, k * per, per, recv=True) for k in range(6)]),
         (y.data_ptr(), yout.data_ptr(), [], [], [nexr.ll_step(0, 0, 1, 0, 1024), nexr.ll_step(0, 1024, 1, 1024, 1024)])],
        slot, mg.F32, 0, status=st.data_ptr(), timeout_us=50_000, stream=stream)
    torch.cuda.synchronize()
    took = time.time() - t0
    assert int(st.item()) == 1
    assert took < 5.0, took
    assert not out.any()
    assert torch.equal(yout[:2048], y[:2048])
    Rig(sc.pair_case(1, n_slices=12)).run(nexr, stream)


def test_a_head_that_never_comes_sets_the_status(nexr, oracle, stream):
    """A one-ended send connection whose receiver never releases: the ninth 1-step slice has no credit."""
    slot, per = 512, 128
    conn = torch.zeros(slot * SLOTS + 2 * CREDIT, dtype=torch.uint8, device="cuda")
    p = conn.data_ptr()
    x = torch.ones(9 * per, dtype=torch.float32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _ws = nexr.reduce_copy_simple_steps_group(
        [(x.data_ptr(), 0, [], [(p, p + slot * SLOTS, p + slot * SLOTS + CREDIT, 0)],
          [nexr.ll_step(0, k * per, -1, 0, per, send=True) for k in range(9)])],
        slot, mg.F32, 0, status=st.data_ptr(), timeout_us=20_000, stream=stream)
    torch.cuda.synchronize()
    assert int(st.item()) == 1
    h = conn.cpu().numpy()
    assert h[slot * SLOTS:slot * SLOTS + 8].view(np.uint64)[0] == 8      # eight slices published, the ninth not
    assert (h[:slot * SLOTS].view(np.float32) == 1.0).all()


# ---- the ring option ---------------------------------------------------------------------------------------
BUFF = 8 * 4096


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


def _count(n, esz=4, slots=9, odd=37):
    """A few slots a rank and an odd remainder."""
    return slots * n * (BUFF // 8 // esz) + odd


def _all_reduce(comm, n, dt, op, count, seed, want, in_place=False, ch=1):
    inputs = mg.gen_inputs(dt, n, count, seed, special=True)
    send = _dev(inputs)
    recv = send if in_place else [torch.zeros_like(s) for s in send]
    torch.cuda.synchronize()
    comm.all_reduce(_ptrs(send), _ptrs(recv), count, dt, op)
    assert comm.queued() == want, (comm.queued(), want)
    exp = ring_allreduce_expected(inputs, dt, op, buff_bytes=BUFF, n_channels=ch)
    for r in range(n):
        assert mg.canon_bytes(dt, recv[r].cpu().numpy()) == mg.canon_bytes(dt, exp[r]), (seed, r)


@pytest.mark.parametrize("n_ranks", [2, 3, 4, 8])
def test_three_all_reduces_in_a_row(ring, oracle, n_ranks):
    with ring.RingComm(n_ranks, ring.DEVICE_MEMORY, BUFF, None, 20000) as comm:
        assert comm.queued() == 0
        comm.set_simple_group(True)
        for call in range(3):
            _all_reduce(comm, n_ranks, mg.F32, 0, _count(n_ranks), 5100 + 7 * call + n_ranks, _want(),
                        in_place=call == 2)


@pytest.mark.parametrize("in_place", [False, True])
def test_all_five_collectives_in_a_row(ring, oracle, in_place):
    """2-step slices (all-reduce, reduce-scatter, all-gather) and 1-step slices (reduce, broadcast) alternate."""
    n, dt, op, root = 4, mg.F32, 0, 1
    count = 4 * 5000 + 4
    per = count // n
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF, None, 20000) as comm:
        comm.set_simple_group(True)
        inputs = mg.gen_inputs(dt, n, count, 5301, special=True)
        send = _dev(inputs)
        rout = send if in_place else [torch.zeros_like(s) for s in send]
        comm.reduce(_ptrs(send), _ptrs(rout), count, dt, op, root)
        assert comm.queued() == _want()
        exp = reduce_expected(inputs, dt, op, root)
        assert mg.canon_bytes(dt, rout[root].cpu().numpy()) == mg.canon_bytes(dt, exp), "reduce"
        _all_reduce(comm, n, dt, op, count, 5300, _want(), in_place)
        send = _dev(inputs)
        bout = send if in_place else [torch.zeros_like(s) for s in send]
        comm.broadcast(_ptrs(send), _ptrs(bout), count, dt, root)
        assert comm.queued() == _want()
        exp = broadcast_expected(inputs, root)
        for r in range(n):
            assert bout[r].cpu().numpy().tobytes() == np.asarray(exp[r]).tobytes(), ("bcast", r)
        send = _dev(inputs)
        rs = [s[r * per:(r + 1) * per] for r, s in enumerate(send)] if in_place else \
            [torch.zeros(per, dtype=send[0].dtype, device="cuda") for _ in range(n)]
        comm.reduce_scatter(_ptrs(send), _ptrs(rs), per, dt, op)
        assert comm.queued() == _want()
        exp = reduce_scatter_expected(inputs, dt, op)
        for r in range(n):
            assert mg.canon_bytes(dt, rs[r].cpu().numpy()) == mg.canon_bytes(dt, exp[r]), ("rs", r)
        send = _dev(inputs)
        comm.reduce(_ptrs(send), _ptrs(rout), count, dt, op, root)       # a 1-step collective again, then 2-step
        assert comm.queued() == _want()
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


def test_four_ranks_two_channels(ring, oracle):
    with ring.RingComm(4, ring.DEVICE_MEMORY, BUFF, None, 20000, n_channels=2) as comm:
        comm.set_simple_group(True)
        for call in range(2):
            _all_reduce(comm, 4, mg.F32, 0, 2 * _count(4), 5500 + call, _want(), ch=2)


def test_bf16_sum_at_eight_ranks(ring, oracle):
    with ring.RingComm(8, ring.DEVICE_MEMORY, BUFF, None, 20000) as comm:
        comm.set_simple_group(True)
        _all_reduce(comm, 8, mg.BF16, 0, _count(8, esz=2), 5600, _want())


def test_toggling_the_option_between_collectives(ring, oracle):
    """On, off, on, off, on: host-sequenced steps and group launches keep the same step counters, and every
    group launch re-stores its tail and head words from them."""
    n = 3
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF, None, 20000) as comm:
        for call, on in enumerate((True, False, True, False, True)):
            comm.set_simple_group(on)
            _all_reduce(comm, n, mg.F32, 0, _count(n, slots=2, odd=5 + call), 5700 + call, _want(on))


def test_falls_back_when_the_grid_is_not_resident(ring, oracle, monkeypatch):
    n = 4
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF, None, 20000) as comm:
        comm.set_simple_group(True)
        for call, resident in enumerate((None, "3", "4", None)):   # 4 members: 3 do not fit even at G = 1, 4 do
            if resident is None:
                monkeypatch.delenv("NEXR_TEST_SIMPLE_GROUP_RESIDENT", raising=False)
            else:
                monkeypatch.setenv("NEXR_TEST_SIMPLE_GROUP_RESIDENT", resident)
            _all_reduce(comm, n, mg.F32, 0, _count(n, slots=2), 5900 + call, _want(resident != "3"))
