"""The flat collectives on the MI355X: nexrRingAllReduceFlat / nexrRingReduceScatterFlat / nexrRingReduceFlat, the
plain calls routed by set_flat, and the nexrFlat* entries beneath them, on tests/flat_cases.py's order-sensitive
inputs (random bits; finite floats of mixed magnitude with NaN payloads, +-inf, +-0 and denormals).

Two yardsticks for every call, both over the WHOLE arena (every output, every guard, every input, a reduce's
untouched outputs):
  * the oracle's bytes: oracle/ring.py's chunk-loop restatement of the communicator's protocol (float32 / float64
    NaNs by class, as everywhere: tests/arith_edges.py canon);
  * the bytes of the same communicator's plain FIFO ring call with the option off, exactly.
The smallest FIFOs (ring_modes_cases.BUFF), device memory, thread ranks, timeoutMs = 20000."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import arith_edges as ae
import flat_cases as fc
import ring_modes_cases as rm
import test_flat as tf
from oracle import ring as oring

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = rm.SEED
TIMEOUT_MS = 20000
chunk_of = tf.chunk_of


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("nex-nccl_amd.ring")


def make_comm(ring, protocol, n, channels):
    return ring.RingComm(n, ring.DEVICE_MEMORY, rm.BUFF[protocol], None, TIMEOUT_MS, rm.PROTO_ID[protocol],
                         tree_ranks_per_node=rm.tree_per_node(n), n_channels=channels)


class _FlatEntries:
    """A RingComm whose three reducing collectives are the explicit *_flat entries (for rm.issue)."""

    def __init__(self, comm):
        self.all_reduce, self.reduce_scatter, self.reduce = comm.all_reduce_flat, comm.reduce_scatter_flat, comm.reduce_flat


def run_on(comm, call, base_phase=0):
    """The call on a fresh copy of its arena in device memory (the arena `base_phase` bytes past a 256-byte
    boundary); the arena afterwards."""
    dev = torch.empty(call.arena0.size + 256, dtype=torch.uint8, device="cuda")
    view = dev[base_phase:base_phase + call.arena0.size]
    view.copy_(torch.from_numpy(call.arena0))
    torch.cuda.synchronize()
    rm.issue(comm, call, view.data_ptr())
    torch.cuda.synchronize()
    return view.cpu().numpy()


def with_oracle(call, protocol, channels):
    return call.set_outputs(rm.oracle_outputs(oring, call, protocol, channels))


def check_both(comm, call, context, explicit, base_phase=0):
    """Plain with the option off, then flat (routed by set_flat, or the explicit entry with the option off): flat
    against plain exactly, flat against the oracle."""
    comm.set_flat(False)
    plain = run_on(comm, call, base_phase)
    q0 = comm.queued()
    assert q0 != 4, (context, call.spec.what())
    if explicit:
        flat = run_on(_FlatEntries(comm), call, base_phase)
        assert comm.queued() == q0, (context, call.spec.what(), "an explicit flat entry leaves the report")
    else:
        comm.set_flat(True)
        flat = run_on(comm, call, base_phase)
        assert comm.queued() == 4, (context, call.spec.what(), comm.queued())
        comm.set_flat(False)
    rm.check(call, flat, context + ("flat against the plain ring",), expected=plain)
    rm.check(call, fc.canon_outputs(call, flat), context + ("flat against the oracle",),
             expected=fc.canon_outputs(call, call.expected))


# ---- the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", rm.CHANNELS)
@pytest.mark.parametrize("n", rm.RANKS)
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_table(ring, oracle, protocol, n, channels):
    """ring_modes_cases' count table for the three collectives: PAIRS cycled, in place on odd calls, root k mod n;
    even calls routed by set_flat, odd calls through the explicit entries."""
    context = (protocol, n, channels)
    seen = set()
    with make_comm(ring, protocol, n, channels) as comm:
        for sp in rm.plan(protocol, n, chunk_of, fc.COLLECTIVES):
            call = with_oracle(fc.Call(sp, n, SEED), protocol, channels)
            check_both(comm, call, context, explicit=sp.k % 2 == 1)
            seen.add((sp.collective, sp.dt))
    assert {c for c, _ in seen} == set(fc.COLLECTIVES) and {d for _, d in seen} == set(range(10))


@pytest.mark.parametrize("n", (4, 8))
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_two_channel_counts(ring, oracle, protocol, n):
    """Several loops on each of two channels: the second part starts its own loop away from element 0."""
    with make_comm(ring, protocol, n, 2) as comm:
        for k, coll in enumerate(fc.COLLECTIVES * 2):
            e = rm.esz_of(rm.PAIRS[k % len(rm.PAIRS)][0])
            sp = rm.spec(k, coll, "large", rm.LARGE[coll](n, chunk_of(coll, protocol, e)), n)
            check_both(comm, with_oracle(fc.Call(sp, n, SEED), protocol, 2), (protocol, n, 2), explicit=k % 2 == 0)


@pytest.mark.parametrize("n", (9, 17))
def test_more_ranks_than_one_group_of_loads(ring, oracle, n):
    """9 and 17 ranks: the chain goes on beyond the kSymPeers = 8 inputs a wave loads at once."""
    e = 2
    with make_comm(ring, "simple", n, 1) as comm:
        for k, coll in enumerate(fc.COLLECTIVES):
            count = n * chunk_of(coll, "simple", e) + 1
            sp = rm.Spec(k, coll, "nC+1", count, ae.F16, rm.SUM, k % 2 == 1, (5 * k + 3) % n)
            check_both(comm, with_oracle(fc.Call(sp, n, SEED), "simple", 1), ("simple", n, 1), explicit=k == 1)


# ---- alignment --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", (ae.BF16, ae.U64), ids=["bf16", "u64"])
def test_every_phase_mod_16(ring, oracle, dt):
    """Element-aligned bases at every phase mod 16: the whole arena moved by every multiple of the element size,
    the reduce-scatter's chunks adding phases of their own (an odd count), in and out of place."""
    e, n = rm.esz_of(dt), 3
    with make_comm(ring, "simple", n, 1) as comm:
        for phase in range(0, 16, e):
            for k, coll in enumerate(fc.COLLECTIVES):
                count = 2 * (16 // e) * 64 + 2 * (16 // e) + 1 + phase // e   # above one piece, an odd tail
                sp = rm.Spec(k + phase, coll, "odd", count, dt, rm.SUM if dt == ae.BF16 else rm.PROD,
                             (k + phase // e) % 2 == 1, k % n)
                check_both(comm, with_oracle(fc.Call(sp, n, SEED), "simple", 1), ("simple", n, 1, "phase", phase),
                           explicit=True, base_phase=phase)


def test_ranks_at_different_phases(nexr, oracle):
    """The direct entry with every rank's input and output at a phase of its own."""
    n, dt, count = 4, ae.F16, 1500
    rng = np.random.default_rng([SEED, 0xA11])
    xs = fc.gen_inputs(rng, dt, n, count)
    step = tf.step_of(oracle, "ll", dt, rm.SUM, n)
    parts = tf.parts_of("ll", 1, count, 2)
    want = fc.model("all_reduce", xs, count, 0, step, parts)[0]
    slot = (count * 2 + 16 + 255) // 256 * 256
    dev = torch.full((2 * n * slot + 256,), rm.GUARD_BYTE, dtype=torch.uint8, device="cuda")
    ins = [64 + r * slot + 2 * r for r in range(n)]                               # phases 0, 2, 4, 6
    outs = [64 + (n + r) * slot + 2 * (7 - r) for r in range(n)]                  # phases 14, 12, 10, 8
    host = dev.cpu().numpy()
    for r in range(n):
        host[ins[r]:ins[r] + 2 * count] = xs[r].view(np.uint8)
    exp = host.copy()
    for r in range(n):
        exp[outs[r]:outs[r] + 2 * count] = want.view(np.uint8)
    dev.copy_(torch.from_numpy(host))
    torch.cuda.synchronize()
    base = dev.data_ptr()
    nexr.flat_all_reduce([base + o for o in ins], [base + o for o in outs], count, dt, nexr.DevRedOp.Sum, 0, False, parts)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy(), exp)


# ---- the average, NaN payloads ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_average_at_three_ranks(ring, oracle, protocol):
    """ncclAvg of every datatype at 3 ranks: PreMulSum by 1 / 3 for the floats (the pre-op on every rank's input
    and the first step's canonicalisation), SumPostDiv for the integers (the divide on the last step only)."""
    n = 3
    with make_comm(ring, protocol, n, 1) as comm:
        for dt in range(10):
            coll = fc.COLLECTIVES[dt % 3]
            count = n * chunk_of(coll, protocol, rm.esz_of(dt)) + n + 1
            sp = rm.Spec(dt, coll, "nC+n+1", count, dt, rm.AVG, dt % 2 == 1, dt % n)
            check_both(comm, with_oracle(fc.Call(sp, n, SEED), protocol, 1), (protocol, n, 1, "avg"), explicit=dt % 2 == 0)


@pytest.mark.parametrize("protocol", ("simple", "ll"))
def test_nan_payload_at_every_start_rank(ring, oracle, protocol):
    """Where a position's chain starts at rank s, rank s's input is a NaN with a payload, everything else finite:
    the first step's bit copy, then min / max keeping the first operand (which differs by protocol) and the sum's
    canonicalisation."""
    n = 4
    with make_comm(ring, protocol, n, 1) as comm:
        k = 0
        for dt in (ae.F16, ae.BF16, ae.F32):
            e = rm.esz_of(dt)
            e_bits, m_bits = ae.FMT[dt]
            count = n * chunk_of("all_reduce", protocol, e) + n + 1
            starts = fc.all_reduce_starts(n, count, e, tf.parts_of(protocol, 1, count, e))
            assert set(starts.tolist()) == set(range(n))
            for op in (rm.SUM, rm.MAX, rm.MIN):
                call = fc.Call(rm.Spec(k, "all_reduce", "nC+n+1", count, dt, op, k % 2 == 1, 0), n, SEED)
                rng = np.random.default_rng([SEED, k])
                for r in range(n):
                    x = fc._finite(rng, dt, count)
                    nan = (((1 << e_bits) - 1) << m_bits) | (0x15 + r) | (r % 2) << (e_bits + m_bits)
                    x[starts == r] = nan
                    call.inputs[r] = x
                    call.arena0[call.send_off[r]:call.send_off[r] + count * e] = x.view(np.uint8)
                check_both(comm, with_oracle(call, protocol, 1), (protocol, n, 1, "nan"), explicit=k % 2 == 0)
                k += 1


# ---- the other semantics, in a child process --------------------------------------------------------------------------
_WORKER = r"""
import importlib, sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import oracle
import flat_cases as fc, ring_modes_cases as rm
import test_flat_gpu as t
oracle.lib()
oracle.set_semantics({mode})
nexr = importlib.import_module("nex-nccl_amd")
ring = importlib.import_module("nex-nccl_amd.ring")
assert nexr.get_semantics() == {mode}
for protocol in rm.PROTO_ID:
    with t.make_comm(ring, protocol, 3, 1) as comm:
        for sp in rm.plan(protocol, 3, t.chunk_of, fc.COLLECTIVES):
            if sp.k % 2:
                continue
            call = t.with_oracle(fc.Call(sp, 3, t.SEED), protocol, 1)
            t.check_both(comm, call, (protocol, 3, 1, {name!r}), explicit=sp.k % 4 == 0)
torch.cuda.synchronize()
print("TABLE-OK")
"""


@pytest.mark.parametrize("name,mode", [("fork", 1), ("shipped", 2)])
def test_table_under_the_other_semantics(nexr, name, mode):
    """NEXR_SEMANTICS is read once per process: a child for each. Fork: signed min / max on the unsigned type;
    shipped: every reduce returns its first operand, so the result is the input of the chain's last rank (SIMPLE)
    or first rank (LL, LL128), bit for bit."""
    assert hasattr(nexr, "get_semantics")
    from conftest import GOLDEN, ROOT
    code = _WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=GOLDEN, mode=mode, name=name)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NEXR_SEMANTICS=name), capture_output=True,
                         text=True, timeout=150)
    assert out.returncode == 0 and "TABLE-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ---- mixed with everything else on one communicator -------------------------------------------------------------------
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_mixed_sequence(ring, oracle, protocol):
    """24 seeded calls of all six collectives on one communicator of 2 channels; set_flat changes every three calls
    and the group / direct options as in ring_modes_cases.mixed_state; every fourth reducing call goes through its
    explicit flat entry. Every result is exact, queued() is 4 exactly after the routed calls, and no call is
    disturbed by the ones before it (no connection, no step counter is touched by a flat call)."""
    n = 4
    with make_comm(ring, protocol, n, 2) as comm:
        for sp in rm.mixed_plan(protocol, n, chunk_of, SEED + 77):
            group, direct = rm.mixed_state(protocol, sp.k)
            if protocol == "simple":
                comm.set_simple_group(group)
                comm.set_direct(direct)
            else:
                comm.set_ll_group(group)
            flat = (sp.k // 3) % 2 == 1
            comm.set_flat(flat)
            context = (protocol, n, 2, "flat" if flat else "", "group" if group else "", "direct" if direct else "")
            reducing = sp.collective in fc.COLLECTIVES
            if reducing:
                call = with_oracle(fc.Call(sp, n, SEED), protocol, 2)
            else:
                call = rm.make_call(sp, n, SEED, oring, protocol, 2)
            explicit = reducing and sp.k % 4 == 3
            got = run_on(_FlatEntries(comm) if explicit else comm, call)
            rm.check(call, fc.canon_outputs(call, got), context, expected=fc.canon_outputs(call, call.expected))
            if reducing and flat and not explicit:
                assert comm.queued() == 4, (context, sp.what(), comm.queued())
            elif sp.collective != "tree" and not explicit:
                assert comm.queued() != 4, (context, sp.what(), comm.queued())


# ---- the entries themselves: streams, capture, many parts --------------------------------------------------------------
def _direct_case(oracle, n, dt, op, count, protocol, channels, seed):
    rng = np.random.default_rng([SEED, seed])
    e = rm.esz_of(dt)
    step = tf.step_of(oracle, protocol, dt, op, n)
    dev_op, arg = oracle.host_to_dev_red_op(op, dt, n)
    return rng, e, step, dev_op, arg


def test_entries_on_a_stream_and_under_capture(nexr, oracle):
    """nexrFlatAllReduce, nexrFlatReduceScatter and nexrFlatReduce on a non-default stream, then captured into a
    HIP graph and replayed once on new inputs: stream-ordered single launches, nothing read from the caller's
    arrays after the call."""
    n, dt, op, count, protocol = 3, ae.F32, rm.SUM, 5003, "simple"
    rng, e, step, dev_op, arg = _direct_case(oracle, n, dt, op, count, protocol, 2, 1)
    parts = tf.parts_of(protocol, 2, count, e)
    assert len(parts) == 2
    root = 1
    ins = [torch.zeros(n * count, dtype=torch.int32, device="cuda") for _ in range(n)]
    ar = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
    rs = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
    rd = torch.zeros(count, dtype=torch.int32, device="cuda")

    def load():
        xs = fc.gen_inputs(rng, dt, n, n * count)
        for t, x in zip(ins, xs):
            t.copy_(torch.from_numpy(x.view(np.int32)))
        return xs

    def launch(stream):
        ip = [t.data_ptr() for t in ins]
        pl = list(parts)   # the caller's arrays die with this call
        nexr.flat_all_reduce(ip, [t.data_ptr() for t in ar], count, dt, dev_op, arg, True, pl, stream=stream)
        nexr.flat_reduce_scatter(ip, [t.data_ptr() for t in rs], count, dt, dev_op, arg, True, stream=stream)
        nexr.flat_reduce(ip, rd.data_ptr(), root, count, dt, dev_op, arg, True, stream=stream)
        del ip, pl

    def verify(xs, what):
        head = [x[:count] for x in xs]
        want_ar = fc.model("all_reduce", head, count, 0, step, parts)[0]
        want_rs = fc.model("reduce_scatter", xs, count, 0, step)
        want_rd = fc.model("reduce", head, count, root, step)[root]
        for r in range(n):
            np.testing.assert_array_equal(ae.canon(dt, ar[r].cpu().numpy().view(np.uint32)), ae.canon(dt, want_ar), what)
            np.testing.assert_array_equal(ae.canon(dt, rs[r].cpu().numpy().view(np.uint32)), ae.canon(dt, want_rs[r]), what)
        np.testing.assert_array_equal(ae.canon(dt, rd.cpu().numpy().view(np.uint32)), ae.canon(dt, want_rd), what)

    xs = load()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        launch(s.cuda_stream)
    s.synchronize()
    verify(xs, "stream")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(torch.cuda.current_stream().cuda_stream)
    xs = load()
    for t in ar + rs + [rd]:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    verify(xs, "replay")


def test_more_parts_than_the_kernel_arguments_hold(nexr, oracle):
    """300 parts of one chunk-pair each: beyond NEXR_FLAT_INLINE_PARTS the parts travel through the call's
    stream-ordered workspace."""
    n, dt, op = 3, ae.F32, rm.SUM
    rng, e, step, dev_op, arg = _direct_case(oracle, n, dt, op, 0, "simple", 1, 2)
    parts, at = [], 0
    for k in range(300):
        cnt = 8 * (1 + k % 5)
        parts.append((at, cnt, 4 * (1 + k % 3)))
        at += cnt
    parts[-1] = (parts[-1][0], parts[-1][1] + 3, parts[-1][2])
    count = at + 3
    assert len(parts) > nexr.FLAT_INLINE_PARTS
    xs = fc.gen_inputs(rng, dt, n, count)
    want = fc.model("all_reduce", xs, count, 0, step, parts)[0]
    starts = fc.all_reduce_starts(n, count, e, parts)
    assert set(starts.tolist()) == set(range(n))
    ins = [torch.from_numpy(x.view(np.int32)).cuda() for x in xs]
    outs = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    nexr.flat_all_reduce([t.data_ptr() for t in ins], [t.data_ptr() for t in outs], count, dt, dev_op, arg, True, parts)
    torch.cuda.synchronize()
    for t in outs:
        np.testing.assert_array_equal(ae.canon(dt, t.cpu().numpy().view(np.uint32)), ae.canon(dt, want))


def test_set_flat_usage(ring, nexr):
    """On and off on an eligible communicator; one rank takes the one-rank path; count 0 succeeds."""
    with make_comm(ring, "simple", 2, 1) as comm:
        comm.set_flat(True)
        comm.all_reduce([1, 1], [1, 1], 0, ae.F32, rm.SUM)
        comm.all_reduce_flat([1, 1], [1, 1], 0, ae.F32, rm.SUM)
        comm.set_flat(False)
    with make_comm(ring, "simple", 1, 1) as comm:
        x = torch.arange(1, 9, dtype=torch.float32, device="cuda")
        y = torch.zeros_like(x)
        comm.set_flat(True)
        for fn in (comm.all_reduce, comm.all_reduce_flat):
            y.zero_()
            fn([x.data_ptr()], [y.data_ptr()], 8, ae.F32, rm.AVG)
            torch.cuda.synchronize()
            assert torch.equal(x, y)
