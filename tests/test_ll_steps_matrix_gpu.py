"""The run kernel and the group kernel (nexrReduceCopyLLSteps[Rule], nexrReduceCopyLLStepsGroup; nexr_ll.hip)
against the sequential interpreter of step lists (oracle/ll_steps.py), bit for bit: every datatype x op,
one to three receive and send connections whose step counters all differ, odd sizes and offsets, sources
and destinations in either user buffer, zero-element steps, the per-connection cleanup under the test
rule, and the fork / shipped semantics. The step lists are tests/ll_steps_cases.py's.

Everything runs on ONE plain stream. A case with several members is one group call; a member that runs
alone (either entry point) never waits: its receive FIFOs hold its peers' lines before the call (written
by the interpreter's Conn.prefill from oracle.make_ll_lines, at most nSlots steps) and the head words of
its send connections already show its last send step. Every call has a status word and a 2 s timeout: a
wrong kernel ends with status 1 and a failed assertion.

User buffers are compared with mg.canon_bytes (fp32 / fp64 NaNs by class, as everywhere in the suite), the
FIFOs' data words the same way and their flag words exactly, under the interpreter's mask of defined
bytes (all but the padding of a step's partial last line)."""
import contextlib

import numpy as np
import pytest

import ll_steps_cases as cases
import make_golden as mg
from oracle import ll_steps

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TIMEOUT_US = 2_000_000
GUARD = 64
HEAD_BYTES = 4096
_EXPECTED = {}  # the interpreter's results of case A for one datatype, shared by the two entry points


@pytest.fixture(scope="module")
def stream():
    """The one plain stream of the file."""
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


def _expected(key, build, scope=None):
    """(case, the interpreter's result, its connections, every connection's FIFO as it was before the
    run). scope: remember the result for the other entry point, which runs the same case next; results
    of another scope (datatype, semantics) are dropped then, so that a session never holds many."""
    if scope is not None and _EXPECTED.get("scope") != scope:
        _EXPECTED.clear()
        _EXPECTED["scope"] = scope
    if scope is not None and key in _EXPECTED:
        return _EXPECTED[key]
    case = build()
    _members, before = cases.model(case)
    members, conns = cases.model(case)
    res = ll_steps.run(members, case.dt, case.op, case.arg)
    exp = (case, res, conns, [c.fifo for c in before])
    if scope is not None:
        _EXPECTED[key] = exp
    return exp


def _guarded(a):
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    host = np.full(raw.size + 2 * GUARD, cases.FILL, dtype=np.uint8)
    host[GUARD:GUARD + raw.size] = raw
    return torch.from_numpy(host).cuda()


def _canon_fifo(dt, fifo):
    """The FIFO's bytes with fp32 / fp64 NaNs in the data words made one NaN (canon_bytes' rule)."""
    if dt not in (mg.F32, mg.F64):
        return fifo
    w = fifo.view(np.uint32).reshape(-1, 4).copy()
    data = np.ascontiguousarray(w[:, [0, 2]])
    v = data.view(np.float32 if dt == mg.F32 else np.float64)
    v[np.isnan(v)] = np.nan
    w[:, [0, 2]] = data
    return w.reshape(-1).view(np.uint8)


def _run_and_check(nexr, stream, expected, how, what):
    case, res, conns, before = expected
    dt = case.dt
    slot = case.slot_bytes
    has_receiver = {i for m in case.members for i in m.recv}
    d_in = [_guarded(m.input) if m.input is not None else None for m in case.members]
    d_out = [_guarded(m.output) if m.output is not None else None for m in case.members]
    d_conn = []
    for i, c in enumerate(conns):
        host = np.zeros(slot * cases.SLOTS + HEAD_BYTES, dtype=np.uint8)
        host[:slot * cases.SLOTS] = before[i]
        if i not in has_receiver:  # its receiver is elsewhere and has read everything this run will send
            host[slot * cases.SLOTS:].view(np.uint64)[:] = c.sent
        d_conn.append(torch.from_numpy(host).cuda())
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def conn_arg(i):
        p = d_conn[i].data_ptr()
        return (p, p + slot * cases.SLOTS, case.conn_start[i])

    def member_args(m, spec):
        steps = [nexr.ll_step(s.src_buf, s.src_ix, s.dst_buf, s.dst_ix, s.n_elts, recv=s.recv, send=s.send,
                              post_op=s.post_op) for s in spec.steps]
        return (d_in[m].data_ptr() + GUARD if d_in[m] is not None else 0,
                d_out[m].data_ptr() + GUARD if d_out[m] is not None else 0,
                [conn_arg(i) for i in spec.recv], [conn_arg(i) for i in spec.send], steps)

    args = [member_args(m, spec) for m, spec in enumerate(case.members)]
    keep = None
    if how == "run":
        assert len(args) == 1, "several members go through the group call"
        i_ptr, o_ptr, recv, send, steps = args[0]
        nexr.reduce_copy_ll_steps(i_ptr, o_ptr, recv, send, slot, steps, dt, case.op, case.arg, n_slots=cases.SLOTS,
                                  status=status.data_ptr(), timeout_us=TIMEOUT_US, stream=stream, rule=case.rule)
    else:
        keep = nexr.reduce_copy_ll_steps_group(args, slot, dt, case.op, case.arg, n_slots=cases.SLOTS,
                                               status=status.data_ptr(), timeout_us=TIMEOUT_US, stream=stream,
                                               rule=case.rule)
    torch.cuda.synchronize()
    del keep
    assert int(status.item()) == 0, (what, "status")
    store = mg.STORE[dt]
    for m, mb in enumerate(res.members):
        for name, dev, exp in (("input", d_in[m], mb.input), ("output", d_out[m], mb.output)):
            if dev is None:
                continue
            h = dev.cpu().numpy()
            assert (h[:GUARD] == cases.FILL).all() and (h[GUARD + exp.size:] == cases.FILL).all(), (what, m, name, "guard")
            got = h[GUARD:GUARD + exp.size]
            if mg.canon_bytes(dt, got.view(store)) != mg.canon_bytes(dt, exp.view(store)):
                bad = np.flatnonzero(got != exp)
                raise AssertionError((what, m, name, "first differing bytes", bad[:8].tolist(), len(bad)))
    lines = slot // 16
    g = min(64, -(-lines // 512))
    for i, c in enumerate(conns):
        h = d_conn[i].cpu().numpy()
        got, exp = _canon_fifo(dt, h[:slot * cases.SLOTS]), _canon_fifo(dt, c.fifo)
        bad = np.flatnonzero((got != exp) & c.mask)
        assert bad.size == 0, (what, "fifo", i, "(slot, line, byte) of the first differing bytes",
                               [(int(b) // slot, int(b) % slot // 16, int(b) % 16) for b in bad[:6]], bad.size)
        heads = h[slot * cases.SLOTS:].view(np.uint64)
        if i in has_receiver:  # one word per wave at a 16-byte stride: waves [0, 4 G) have read every step
            assert heads[0:8 * g:2].tolist() == [c.read] * (4 * g), (what, "heads", i, heads[:8 * g:2].tolist())
            assert not heads[1::2].any() and not heads[8 * g:].any(), (what, "head words past the waves", i)
        else:
            assert (heads == c.sent).all(), (what, "the receiver's head words were written", i)


# ---- A ------------------------------------------------------------------------------------------------
def _alone(nexr, stream, dt, how, mode):
    for k, (name, op, arg) in enumerate(cases.ops_for(dt)):
        for j, (n_recv, n_send) in enumerate(cases.PEERS):
            key = ("alone", dt, name, n_recv, n_send, mode)
            exp = _expected(key, lambda: cases.alone_case(dt, op, arg, n_recv, n_send, 1000 * dt + 10 * k + j),
                            scope=(dt, mode))
            _run_and_check(nexr, stream, exp, how, key + (how,))


@pytest.mark.parametrize("how", list(cases.ENTRY_POINTS))
@pytest.mark.parametrize("dt", cases.DTYPES)
def test_one_member_alone_every_op_and_peer_count(nexr, oracle, stream, dt, how):
    """A: 8 steps on 0-3 receive and 0-3 send connections at counters that all differ, every op, through
    nexrReduceCopyLLSteps (how = run) and through a group of one (how = group)."""
    _alone(nexr, stream, dt, how, 0)


# ---- B ------------------------------------------------------------------------------------------------
def _star(nexr, stream, dt, name, slot_bytes, mode, tag="star"):
    _n, op, arg = cases.op_named(dt, name)
    key = (tag, dt, name, slot_bytes, mode)
    exp = _expected(key, lambda: cases.star_case(dt, op, arg, slot_bytes, cases.star_sizes(dt, slot_bytes),
                                                 77 + 16 * dt + op))
    _run_and_check(nexr, stream, exp, "group", key)


@pytest.mark.parametrize("dt,name", cases.STAR_PAIRS)
def test_star_in_one_group_launch(nexr, oracle, stream, dt, name):
    """B: three leaves and a hub that receives from and sends to all three in every step, 11 pieces over 8
    slots, six connections at six different counters, four members in one launch."""
    _star(nexr, stream, dt, name, 4096, 0)


# ---- C ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", sorted(cases.GEOMETRY_SLOTS))
@pytest.mark.parametrize("dt,name", cases.GEOMETRY_PAIRS)
def test_star_geometry(nexr, oracle, stream, dt, name, geometry):
    """C: the star at 24 KiB slots (three workgroups a member) and at 1 MiB + 8 KiB + 48 B (the
    64-workgroup cap, 4 x 64 workgroups in the launch, workgroup 0 with three tiles, a last tile of 3 lines)."""
    _star(nexr, stream, dt, name, cases.GEOMETRY_SLOTS[geometry], 0, tag="geometry")


# ---- D ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,name", cases.ROUTING_PAIRS)
def test_buffer_routing_in_one_list(nexr, oracle, stream, dt, name):
    """D: sources in the output (no pre-op on them), a destination in the input, the post-op on every second
    data step, zero-element recv, send and recv + send steps between them, and a step that ends the launch."""
    _n, op, arg = cases.op_named(dt, name)
    key = ("routing", dt, name)
    _run_and_check(nexr, stream, _expected(key, lambda: cases.routing_case(dt, op, arg, 300 + dt)), "group", key)


# ---- E ------------------------------------------------------------------------------------------------
def test_cleanup_per_connection(nexr, oracle, stream):
    """E: under {0x100, 0x78} the hub's send connections start at 0x70, 0x74 and 0x7a and clean at different
    pieces — one alone, two together, each of the three bits by itself — as do two of the leaves'; every
    output and every FIFO byte, the clean lines included, is the interpreter's."""
    _run_and_check(nexr, stream, _expected(("clean",), cases.clean_case), "group", ("clean",))


# ---- F ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fork", "shipped"])
@pytest.mark.parametrize("dt", [mg.F32, mg.BF16, mg.I8])
def test_one_member_alone_under_fork_and_shipped(nexr, oracle, stream, dt, mode):
    m = int(nexr.Semantics.Fork if mode == "fork" else nexr.Semantics.Shipped)
    with _semantics(nexr, oracle, m):
        for how in cases.ENTRY_POINTS:
            _alone(nexr, stream, dt, how, m)


@pytest.mark.parametrize("mode", ["fork", "shipped"])
@pytest.mark.parametrize("dt", [mg.F32, mg.I32])
def test_star_under_fork_and_shipped(nexr, oracle, stream, dt, mode):
    m = int(nexr.Semantics.Fork if mode == "fork" else nexr.Semantics.Shipped)
    with _semantics(nexr, oracle, m):
        for name, _op, _arg in cases.ops_for(dt):
            _star(nexr, stream, dt, name, 4096, m)
