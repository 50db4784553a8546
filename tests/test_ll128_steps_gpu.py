"""nexrReduceCopyLL128StepsGroup (reduce_copy_ll128_group_kernel, nexr_ll.hip) against the sequential
interpreter of LL128 step lists (tests/ll128_steps_model.py), bit for bit: the user buffers whole with
guard bytes, every FIFO byte under the interpreter's mask of written slices (the rest must be as it was),
and the head words of every wave. Everything runs on ONE plain stream with a status word and a 2 s
timeout (20-50 ms where the timeout is the expected outcome).

fp32 / fp64 NaNs are compared by class (mg.canon_bytes' rule, as everywhere in the suite), in the user
buffers and in the FIFOs' data words; flags and everything else exactly."""
import contextlib
import time

import numpy as np
import pytest

import ll128_steps_model as model
import ll_steps_cases as cases
import make_golden as mg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

S = model.Step
TIMEOUT_US = 2_000_000
GUARD = 64
HEAD_BYTES = 4096
SLOTS = cases.SLOTS


@pytest.fixture(scope="module")
def stream():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    s = torch.cuda.Stream(device=torch.device("cuda:0"))
    yield s.cuda_stream
    torch.cuda.synchronize()


@contextlib.contextmanager
def _semantics(nexr, oracle, mode):
    prev = nexr.get_semantics()
    try:
        nexr.set_semantics(mode)
        with oracle.semantics(mode):
            yield
    finally:
        nexr.set_semantics(prev)


def _canon_fifo(dt, fifo):
    """NaNs in the data words (words 0..14 of every 16-word line) made one NaN for fp32 / fp64."""
    if dt not in (mg.F32, mg.F64):
        return fifo
    w = fifo.view(np.uint64).reshape(-1, 16).copy()
    data = np.ascontiguousarray(w[:, :15])
    v = data.view(np.float32 if dt == mg.F32 else np.float64)
    v[np.isnan(v)] = np.nan
    w[:, :15] = data
    return w.reshape(-1).view(np.uint8)


class Rig:
    """The device side of a set of members and connections, kept over several calls: user buffers with
    guards, FIFOs with their head words behind them. spec: cases.Case-like (dt, op, arg, slot_bytes,
    conn_start, prefill, members)."""

    def __init__(self, case):
        self.case = case
        self.slot = case.slot_bytes
        self.members, self.conns = model.model(case)
        self.has_receiver = {i for m in case.members for i in m.recv}
        self.d_in = [self._guarded(m.input) if m.input is not None else None for m in case.members]
        self.d_out = [self._guarded(m.output) if m.output is not None else None for m in case.members]
        self.d_conn = []
        for c in self.conns:
            host = np.zeros(self.slot * SLOTS + HEAD_BYTES, dtype=np.uint8)
            host[:self.slot * SLOTS] = c.fifo
            self.d_conn.append(torch.from_numpy(host).cuda())
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")

    @staticmethod
    def _guarded(a):
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        host = np.full(raw.size + 2 * GUARD, cases.FILL, dtype=np.uint8)
        host[GUARD:GUARD + raw.size] = raw
        return torch.from_numpy(host).cuda()

    def run(self, nexr, stream, step_lists, what, timeout_us=TIMEOUT_US, check=True):
        """One group call of step_lists (a list of Steps per member) from the connections' counters as
        they stand; the interpreter runs the same lists; then everything is compared."""
        case = self.case
        before = [c.fifo.copy() for c in self.conns]
        starts = [(c.sent, c.read) for c in self.conns]
        for mb, steps in zip(self.members, step_lists):
            mb.steps = [S(*s) for s in steps]
        model.run(self.members, case.dt, case.op, case.arg)
        for i, c in enumerate(self.conns):  # a receiver elsewhere has read everything this call will send
            if i not in self.has_receiver:
                self.d_conn[i][self.slot * SLOTS:].view(torch.int64)[:] = c.sent

        def conn_arg(i, recv):
            p = self.d_conn[i].data_ptr()
            return (p, p + self.slot * SLOTS, starts[i][1] if recv else starts[i][0])

        args = []
        for m, spec in enumerate(case.members):
            steps = [nexr.ll_step(s.src_buf, s.src_ix, s.dst_buf, s.dst_ix, s.n_elts, recv=s.recv, send=s.send,
                                  post_op=s.post_op) for s in self.members[m].steps]
            args.append((self.d_in[m].data_ptr() + GUARD if self.d_in[m] is not None else 0,
                         self.d_out[m].data_ptr() + GUARD if self.d_out[m] is not None else 0,
                         [conn_arg(i, True) for i in spec.recv], [conn_arg(i, False) for i in spec.send], steps))
        self.status.zero_()
        torch.cuda.synchronize()
        keep = nexr.reduce_copy_ll128_steps_group(args, self.slot, case.dt, case.op, case.arg, n_slots=SLOTS,
                                                  status=self.status.data_ptr(), timeout_us=timeout_us, stream=stream)
        torch.cuda.synchronize()
        del keep
        if check:
            self.check(before, what)

    def check(self, before, what):
        case, dt, slot = self.case, self.case.dt, self.slot
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
        g = min(64, -(-slot // 4096))
        for i, c in enumerate(self.conns):
            h = self.d_conn[i].cpu().numpy()
            got, exp = _canon_fifo(dt, h[:slot * SLOTS]), _canon_fifo(dt, c.fifo)
            bad = np.flatnonzero((got != exp) & c.mask)
            assert bad.size == 0, (what, "fifo", i, "(slot, slice, byte) of the first differing bytes",
                                   [(int(b) // slot, int(b) % slot // 2048, int(b) % 2048) for b in bad[:6]], bad.size)
            untouched = ~c.mask
            assert (h[:slot * SLOTS][untouched] == before[i][untouched]).all(), (what, "bytes no step sent changed", i)
            heads = h[slot * SLOTS:].view(np.uint64)
            if i in self.has_receiver:  # one word per wave at a 16-byte stride: every wave has posted every step
                assert heads[0:8 * g:2].tolist() == [c.head] * (4 * g), (what, "heads", i, heads[:8 * g:2].tolist())
                assert not heads[1::2].any() and not heads[8 * g:].any(), (what, "head words past the waves", i)
            else:
                assert (heads == c.sent).all(), (what, "the receiver's head words were written", i)


def _case(dt, op, arg, slot, conn_start, members, prefill=None):
    return cases.Case(dt, op, arg, slot, None, list(conn_start), prefill or {}, members)


def _blank(n_elts, dt):
    return np.full(n_elts * cases.esz_of(dt), cases.FILL, dtype=np.uint8).view(mg.STORE[dt])


# ---- geometry x step sizes ---------------------------------------------------------------------------------
def step_bytes(esz, cap):
    sizes = [0, esz, 8, 112, 116, 120, 124, 128, 1920 - esz, 1920, 1920 + esz, 3840, 3840 + esz, cap - esz, cap]
    return [b for b in sizes if b <= cap and b % esz == 0]


@pytest.mark.parametrize("slot", [2048, 4096, 12 << 10, 256 << 10, 512 << 10])
@pytest.mark.parametrize("dt", [mg.U8, mg.F16, mg.F32])
def test_geometry_and_step_sizes(nexr, oracle, stream, dt, slot):
    """Member 0 sends pieces of its input, member 1 reduces them with its own and sends the sum on to a
    connection whose receiver is elsewhere: G = 1 (one slice, two waves idle), one tile, G = 3, G = 64 on the cap
    and two strided tiles a workgroup; sizes round the flag lane's split chunk, a slice, a tile and the slot."""
    esz = cases.esz_of(dt)
    sizes = [b // esz for b in step_bytes(esz, model.capacity(slot))]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    total = int(offs[-1]) + 1
    xs = mg.gen_inputs(dt, 2, total, 7 + dt + slot // 2048, special=True)
    m0 = cases.MemberSpec(xs[0], None, [], [0], [])
    m1 = cases.MemberSpec(xs[1], _blank(total, dt), [0], [1], [])
    rig = Rig(_case(dt, mg.SUM, 0, slot, [3, 11], [m0, m1]))
    send = [S(0, int(o), -1, 0, n, False, True, False) for o, n in zip(offs, sizes)]
    fold = [S(0, int(o), 1, int(o) + 1, n, True, True, False) for o, n in zip(offs, sizes)]
    rig.run(nexr, stream, [send, fold], ("geometry", dt, slot))


# ---- credits -----------------------------------------------------------------------------------------------
def _pair_rig(dt, slot, conn_start, total, seed):
    xs = mg.gen_inputs(dt, 2, total, seed, special=False)
    m0 = cases.MemberSpec(xs[0], None, [], [0], [])
    m1 = cases.MemberSpec(xs[1], _blank(total, dt), [0], [], [])
    return Rig(_case(dt, mg.SUM, 0, slot, conn_start, [m0, m1]))


def _pair_lists(k0, n_steps, per):
    send = [S(0, (k0 + k) * per, -1, 0, per - (k % 3), False, True, False) for k in range(n_steps)]
    recv = [S(0, (k0 + k) * per, 1, (k0 + k) * per, per - (k % 3), True, False, False) for k in range(n_steps)]
    return [send, recv]


@pytest.mark.parametrize("n_steps", [1, 7, 8, 9, 17, 40])
def test_credits_one_to_forty_steps_over_eight_slots(nexr, oracle, stream, n_steps):
    per = 3840 // 4
    rig = _pair_rig(mg.I32, 4096, [6], n_steps * per, n_steps)
    rig.run(nexr, stream, _pair_lists(0, n_steps, per), ("credits", n_steps))


def test_counters_carried_over_three_calls_and_the_flags_high_word(nexr, oracle, stream):
    """Three calls on the same connection from where the last one stopped (11, 5 and 13 steps over 8 slots),
    starting at step 0xFFFFFFFE: the flags pass 2^32, so their high word counts."""
    per = 3840 // 4
    rig = _pair_rig(mg.I32, 4096, [0xFFFFFFFE], 29 * per, 5)
    k0 = 0
    for call, n in enumerate((11, 5, 13)):
        rig.run(nexr, stream, _pair_lists(k0, n, per), ("carried", call))
        k0 += n
    assert rig.conns[0].sent == rig.conns[0].head == 0xFFFFFFFE + 29


# ---- arithmetic ----------------------------------------------------------------------------------------------
def _alone(nexr, stream, dt, mode=0):
    for k, (name, op, arg) in enumerate(cases.ops_for(dt)):
        for j, (n_recv, n_send) in enumerate(cases.PEERS):
            case = cases.alone_case(dt, op, arg, n_recv, n_send, 1000 * dt + 10 * k + j)
            rig = Rig(case)
            rig.run(nexr, stream, [case.members[0].steps], ("alone", dt, name, n_recv, n_send, mode))


@pytest.mark.parametrize("dt", cases.DTYPES)
def test_one_member_alone_every_op_and_peer_count(nexr, oracle, stream, dt):
    """Every datatype x op with 0-3 receive and 0-3 send connections at counters that all differ, as a
    group of one (the run form): tests/ll_steps_cases.py's lists, its peers' lines pre-filled."""
    _alone(nexr, stream, dt)


@pytest.mark.parametrize("mode", ["fork", "shipped"])
@pytest.mark.parametrize("dt", [mg.F32, mg.I8])
def test_one_member_alone_under_fork_and_shipped(nexr, oracle, stream, dt, mode):
    m = int(nexr.Semantics.Fork if mode == "fork" else nexr.Semantics.Shipped)
    with _semantics(nexr, oracle, m):
        _alone(nexr, stream, dt, m)


@pytest.mark.parametrize("dt,name", [(mg.F32, "sum"), (mg.BF16, "prod"), (mg.I8, "min"), (mg.U64, "sumpostdiv")])
def test_three_leaf_star_in_one_launch(nexr, oracle, stream, dt, name):
    _n, op, arg = cases.op_named(dt, name)
    case = cases.star_case(dt, op, arg, 4096, cases.star_sizes(dt, 4096), 77 + 16 * dt + op)
    Rig(case).run(nexr, stream, [m.steps for m in case.members], ("star", dt, name))


@pytest.mark.parametrize("dt,red", [(mg.BF16, 0), (mg.F16, 0), (mg.I8, 0), (mg.F32, 4)])
def test_three_member_chain(nexr, oracle, stream, dt, red):
    """send -> recvReduceSend -> recvReduceCopy with the post-op, 12 pieces over 8 slots of 12 KiB; Sum, and the
    fp32 average as the host encodes it for three ranks."""
    op, arg = oracle.host_to_dev_red_op(red, dt, 3)
    esz = cases.esz_of(dt)
    cap = model.capacity(12 << 10) // esz
    sizes = [cap if k % 2 == 0 else cap // 3 + 1 for k in range(12)]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    total = int(offs[-1])
    xs = mg.gen_inputs(dt, 3, total, 31 + dt, special=True)
    members = [cases.MemberSpec(xs[0], None, [], [0], [S(0, int(o), -1, 0, n, False, True, False) for o, n in zip(offs, sizes)]),
               cases.MemberSpec(xs[1], None, [0], [1], [S(0, int(o), -1, 0, n, True, True, False) for o, n in zip(offs, sizes)]),
               cases.MemberSpec(xs[2], _blank(total, dt), [1], [], [S(0, int(o), 1, int(o), n, True, False, True)
                                                                    for o, n in zip(offs, sizes)])]
    case = _case(dt, op, arg, 12 << 10, [9, 2], members)
    Rig(case).run(nexr, stream, [m.steps for m in members], ("chain", dt, red))


def test_arithmetic_edge_operands_at_both_pack_parities(nexr, oracle, stream):
    """tests/arith_edges.py's pair layout (bf16) through one member: the interpreter against the independent
    reference, then the device against the interpreter."""
    import arith_edges as ae
    from test_arith_edges import first_diff, steps_cases
    dt = ae.BF16
    for name, tag, case, exp in steps_cases(dt):
        assert case.slot_bytes % 2048 == 0
        rig = Rig(case)
        rig.run(nexr, stream, [case.members[0].steps], ("edges", name, tag))
        out = rig.members[0].output.view(ae.UINT[dt])
        assert first_diff(dt, out, exp) is None, (name, tag, "interpreter vs reference", first_diff(dt, out, exp))


# ---- bounded failure ---------------------------------------------------------------------------------------
def _timed(rig, nexr, stream, lists, timeout_us, preset=0):
    case = rig.case
    args = []
    for m, spec in enumerate(case.members):
        def conn_arg(i):
            p = rig.d_conn[i].data_ptr()
            return (p, p + rig.slot * SLOTS, case.conn_start[i])
        steps = [nexr.ll_step(s.src_buf, s.src_ix, s.dst_buf, s.dst_ix, s.n_elts, recv=s.recv, send=s.send) for s in lists[m]]
        args.append((rig.d_in[m].data_ptr() + GUARD if rig.d_in[m] is not None else 0,
                     rig.d_out[m].data_ptr() + GUARD if rig.d_out[m] is not None else 0,
                     [conn_arg(i) for i in spec.recv], [conn_arg(i) for i in spec.send], steps))
    rig.status.fill_(preset)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = nexr.reduce_copy_ll128_steps_group(args, rig.slot, case.dt, case.op, case.arg, n_slots=SLOTS,
                                              status=rig.status.data_ptr(), timeout_us=timeout_us, stream=stream)
    torch.cuda.synchronize()
    dt_s = time.perf_counter() - t0
    del keep
    return dt_s


def test_a_missing_line_sets_the_status_and_ends_in_time(nexr, oracle, stream):
    """The receiver alone; its peer wrote two slices of 3840 bytes but line 5 of the second slice carries an old
    flag. Status 1 within the 30 ms timeout and a margin; the wave that owns the line (wave 3 of the tile:
    units 192-255) writes nothing, the other slice's waves have written theirs."""
    n = 3840
    x = np.arange(n, dtype=np.uint8) | 1
    conn_prefill = {0: [x]}
    case = _case(mg.U8, mg.SUM, 0, 4096, [0], [cases.MemberSpec(None, _blank(n, mg.U8), [0], [], [])], conn_prefill)
    rig = Rig(case)
    h = rig.d_conn[0].cpu().numpy()
    h.view(np.uint64).reshape(-1, 16)[16 + 5, 15] = 77
    rig.d_conn[0] = torch.from_numpy(h).cuda()
    took = _timed(rig, nexr, stream, [[S(-1, 0, 1, 0, n, True, False, False)]], 30_000)
    assert int(rig.status.item()) == 1
    assert took < 0.030 + 1.0, took
    out = rig.d_out[0].cpu().numpy()[GUARD:GUARD + n]
    assert (out[:1920] == x[:1920]).all()                       # slice 0: waves 0 and 1
    # slice 1: its lines 0-7 (the stale line 5 among them) are wave 2's, user chunks 0-59 of the slice: unwritten;
    # lines 8-15 are wave 3's, chunks 60-119: arrived and written
    assert (out[1920:1920 + 960] == cases.FILL).all(), "the stale line's wave wrote its outputs"
    assert (out[1920 + 960:] == x[1920 + 960:]).all()


def test_a_missing_credit_sets_the_status_and_ends_in_time(nexr, oracle, stream):
    """The sender alone with nine steps and head words that stay 0: the ninth has no credit. Status 1 in time,
    and slot 0 still holds step 0's lines (flag 1), not step 8's."""
    n = 1920
    x = np.arange(9 * n, dtype=np.uint32).astype(np.uint8)
    case = _case(mg.U8, mg.SUM, 0, 4096, [0], [cases.MemberSpec(x, None, [], [0], [])])
    rig = Rig(case)
    lists = [[S(0, k * n, -1, 0, n, False, True, False) for k in range(9)]]
    took = _timed(rig, nexr, stream, lists, 30_000)
    assert int(rig.status.item()) == 1
    assert took < 0.030 + 1.0, took
    flags = rig.d_conn[0].cpu().numpy()[:rig.slot * SLOTS].view(np.uint64).reshape(-1, 16)[:, 15]
    assert (flags[:16] == 1).all() and (flags[32 * 7:32 * 7 + 16] == 8).all()


def test_a_host_written_status_ends_the_polls_early(nexr, oracle, stream):
    """A receiver whose line never comes, a 2 s timeout, and a status word already 2 (an abort relayed by the
    host): the poll gives up at its next look at the word, far inside the timeout; nothing is written."""
    n = 3840
    case = _case(mg.U8, mg.SUM, 0, 4096, [0], [cases.MemberSpec(None, _blank(n, mg.U8), [0], [], [])])
    rig = Rig(case)
    took = _timed(rig, nexr, stream, [[S(-1, 0, 1, 0, n, True, False, False)]], 2_000_000, preset=2)
    assert int(rig.status.item()) == 2
    assert took < 1.0, took
    assert (rig.d_out[0].cpu().numpy() == cases.FILL).all()


# ---- consumer first: the ordered hand-off ------------------------------------------------------------------
@pytest.mark.parametrize("n_members", [2, 3])
def test_consumers_polling_before_the_first_line_is_written(nexr, oracle, stream, n_members):
    """64 steps of a full 12 KiB slot (11520 bytes: G = 3) round a ring of 2 or 3 members, random payloads (every
    16-byte unit differs from what its slot held 8 steps before). Member 0 begins with six local full-slot copies
    (no recv, no send), so every consuming wave down the ring is in its poll before the first line is written, and
    member 1 carries a local full-slot copy beside every step (uneven load). Every output word is checked, three
    times over with the counters carried on."""
    slot, n_steps, lead = 12 << 10, 64, 6
    per = model.capacity(slot)
    rng = np.random.default_rng(1234 + n_members)
    total = n_steps * per
    xs = [rng.integers(0, 256, total + per, dtype=np.uint8) for _ in range(n_members)]
    scratch = total  # the region of the local copies, in input and output alike
    specs = []
    for m in range(n_members):
        specs.append(cases.MemberSpec(xs[m], _blank(total + per, mg.U8), [m], [(m + 1) % n_members], []))
    rig = Rig(_case(mg.U8, mg.SUM, 0, slot, [5 + 9 * m for m in range(n_members)], specs))
    local = S(0, scratch, 1, scratch, per, False, False, False)
    # Two steps per piece for every member, so that a launch's cut (the same step index for all) falls between
    # pieces: member 0 sends piece k and reads piece k - lag (the ring holds that many); the others reduce the
    # piece with their input, keep it and pass it on, then copy locally (member 1) or do nothing.
    lag = n_members
    lists = [[local] * lead] + [[S()] * lead for _ in range(1, n_members)]
    for k in range(n_steps + lag):
        lists[0].append(S(0, k * per, -1, 0, per, False, True, False) if k < n_steps else S())
        lists[0].append(S(-1, 0, 1, (k - lag) * per, per, True, False, False) if k >= lag else S())
        for m in range(1, n_members):
            lists[m].append(S(0, k * per, 1, k * per, per, True, True, False) if k < n_steps else S())
            lists[m].append(local if m == 1 and k < n_steps else S())
    for rep in range(3):
        rig.run(nexr, stream, lists, ("consumer first", n_members, rep))
    acc = xs[0][:total].copy()
    for m in range(1, n_members):
        acc = acc + xs[m][:total]
    assert (rig.members[0].output[:total] == acc).all()  # the interpreter's own answer, in plain numpy
