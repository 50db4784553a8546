"""User-created PreMulSum ops with a scalar per rank on the MI355X: device-memory communicators host-sequenced, in
LL runs and under the group options, the flat launches with a scalar per rank (nexrFlatAllReducePreMul,
nexrFlatReduceScatterPreMul, nexrFlatReducePreMul, nexrFlatTreeAllReducePreMul) beneath the ...Flat entries and
set_flat, and device-resident scalars.

Every call's WHOLE arena (every output, every guard, every input, a reduce's untouched outputs) is compared with
tests/premul_cases.py's expected bytes, and every flat call's also with the same communicator's host-sequenced call,
exactly. The smallest FIFOs (ring_modes_cases.BUFF), thread ranks, timeoutMs = 20000."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import arith_edges as ae
import premul_cases as pc
import ring_modes_cases as rm
from oracle import ring as oring

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = rm.SEED ^ 0x504D
TIMEOUT_MS = 20000


def chunk_of(coll, protocol, esz):
    return oring.chunk_count(coll, protocol, esz, rm.BUFF[protocol])


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("nex-nccl_amd.ring")


def make_comm(ring, protocol, n, channels=1):
    return ring.RingComm(n, ring.DEVICE_MEMORY, rm.BUFF[protocol], None, TIMEOUT_MS, rm.PROTO_ID[protocol],
                         tree_ranks_per_node=rm.tree_per_node(n), n_channels=channels)


class _FlatEntries:
    """A RingComm whose four reducing collectives are the explicit *_flat entries (for rm.issue)."""

    def __init__(self, comm):
        self.all_reduce, self.reduce_scatter, self.reduce = comm.all_reduce_flat, comm.reduce_scatter_flat, comm.reduce_flat
        self.tree_all_reduce = comm.tree_all_reduce_flat


class _WithOp:
    """A call as rm.issue reads it, its spec's op replaced by a handle."""

    def __init__(self, call, op):
        self.spec = call.spec._replace(op=op)
        self.send_off, self.recv_off = call.send_off, call.recv_off


def run_on(comm, call, op, base_phase=0):
    """The call under `op` on a fresh copy of its arena in device memory (`base_phase` bytes past a 256-byte
    boundary); the arena afterwards."""
    dev = torch.empty(call.arena0.size + 256, dtype=torch.uint8, device="cuda")
    view = dev[base_phase:base_phase + call.arena0.size]
    view.copy_(torch.from_numpy(call.arena0))
    torch.cuda.synchronize()
    rm.issue(comm, _WithOp(call, op), view.data_ptr())
    torch.cuda.synchronize()
    return view.cpu().numpy()


def immediate(comm, dt, bits):
    return comm.create_premul_sum(list(pc.scalar_array(dt, bits)), dt, pc.HOST_IMMEDIATE)


def all_flat(comm, on):
    comm.set_flat(on, tree=on)


def check_both(comm, call, h, context, explicit, base_phase=0):
    """Host-sequenced (every option off) against the expected bytes; then flat (routed by set_flat, or the explicit
    entry) against the host-sequenced call exactly and against the expected bytes."""
    all_flat(comm, False)
    plain = run_on(comm, call, h, base_phase)
    pc.check(call, plain, context + ("host-sequenced",))
    if explicit:
        flat = run_on(_FlatEntries(comm), call, h, base_phase)
    else:
        all_flat(comm, True)
        flat = run_on(comm, call, h, base_phase)
        assert comm.queued() == 4, (context, call.spec.what(), comm.queued())
        all_flat(comm, False)
    rm.check(call, flat, context + ("flat against host-sequenced",), expected=plain)
    pc.check(call, flat, context + ("flat",))


# ---- the FIFO paths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2, 3, 4))
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_ring_and_tree_in_device_memory(ring, oracle, protocol, n):
    """Every rank's Primitives carries its own scalar: host-sequenced SIMPLE and LL128 steps, and LL in whatever mode
    the communicator runs it (its first tree call makes a second stream per rank, after which 2 ranks' four rank
    streams no longer fit the hardware queues and LL steps are host-sequenced; the LL runs have the test below)."""
    context = (protocol, n)
    with make_comm(ring, protocol, n) as comm:
        handles = {}
        for k, coll in enumerate(pc.COLLECTIVES * 2):
            dt = pc.DTYPES[k % len(pc.DTYPES)]
            e = rm.esz_of(dt)
            c = chunk_of(coll, protocol, e)
            count = n * c + n + 1 if k < 4 else 16 // e + 1
            bits = pc.scalar_bits(dt, n)
            if dt not in handles:
                handles[dt] = immediate(comm, dt, bits)
            call = pc.make_call(oracle, oring, pc.spec(k, coll, "", count, dt, n), n, SEED, bits, protocol, 1)
            pc.check(call, run_on(comm, call, handles[dt]), context)
            if coll != "tree":
                assert comm.queued() in (0, 1, 2), context


def test_ll_runs_take_every_ranks_own_scalar(ring, oracle):
    """2 ranks, LL, ring collectives only: the steps run on the device (queued() == 2, nexrReduceCopyLLStepsRule
    per rank with that rank's redOpArg), several loops per call, every datatype of pc.DTYPES."""
    n, protocol = 2, "ll"
    with make_comm(ring, protocol, n) as comm:
        for k, coll in enumerate(("all_reduce", "reduce_scatter", "reduce") * 2):
            dt = pc.DTYPES[k % len(pc.DTYPES)]
            bits = pc.scalar_bits(dt, n)
            h = immediate(comm, dt, bits)
            count = 2 * n * chunk_of(coll, protocol, rm.esz_of(dt)) + 3
            call = pc.make_call(oracle, oring, pc.spec(k, coll, "2nC+3", count, dt, n), n, SEED, bits, protocol, 1)
            pc.check(call, run_on(comm, call, h), (protocol, n, coll))
            if torch.cuda.device_count() == 1:
                assert comm.queued() == 2, (coll, comm.queued())


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_group_options_fall_back_on_differing_scalars(ring, oracle, protocol):
    """A group launch carries one redOpArg: with differing scalars the call runs as without the option (and says
    so), with n equal scalars it runs in group launches (3) as ncclAvg's PreMulSum does. Exact either way."""
    n, dt = 4, ae.F16
    colls = ("all_reduce", "reduce_scatter", "reduce") + (("tree",) if protocol != "simple" else ())
    with make_comm(ring, protocol, n) as comm:
        differ = pc.scalar_bits(dt, n)
        equal = [differ[1]] * n
        hd, he = immediate(comm, dt, differ), immediate(comm, dt, equal)
        (comm.set_simple_group if protocol == "simple" else comm.set_ll_group)(True)
        for k, coll in enumerate(colls):
            count = n * chunk_of(coll, protocol, 2) + n + 1
            sp = pc.spec(k, coll, "nC+n+1", count, dt, n)
            call = pc.make_call(oracle, oring, sp, n, SEED, equal, protocol, 1)
            pc.check(call, run_on(comm, call, he), (protocol, coll, "equal scalars"))
            assert comm.queued() == 3, (protocol, coll, comm.queued())
            call = pc.make_call(oracle, oring, sp, n, SEED, differ, protocol, 1)
            pc.check(call, run_on(comm, call, hd), (protocol, coll, "differing scalars"))
            assert comm.queued() == 0, (protocol, coll, comm.queued())


# ---- the flat launches -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", ("simple", "ll"))
def test_flat_all_ten_datatypes(ring, oracle, protocol):
    n = 4
    with make_comm(ring, protocol, n) as comm:
        k = 0
        for dt in range(10):
            bits = pc.scalar_bits(dt, n)
            h = immediate(comm, dt, bits)
            for coll in pc.COLLECTIVES:
                if (k + dt) % 2 and coll in ("reduce_scatter", "reduce"):   # every datatype meets both all-reduces
                    k += 1
                    continue
                count = n * chunk_of(coll, protocol, rm.esz_of(dt)) + n + 1
                call = pc.make_call(oracle, oring, pc.spec(k, coll, "nC+n+1", count, dt, n), n, SEED, bits, protocol, 1)
                check_both(comm, call, h, (protocol, n, ae.NAMES[dt]), explicit=k % 4 < 2)
                k += 1
            comm.destroy_op(h)


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_flat_counts_around_packs_pieces_and_chunks(ring, oracle, protocol):
    """Around a 16-byte pack, a 2048-byte piece, a chunk boundary inside a piece (C + 1, nC + 1) and 2nC + 3, where
    every start rank occurs."""
    n, dt = 3, ae.F32 if protocol != "ll128" else ae.BF16
    e = rm.esz_of(dt)
    bits = pc.scalar_bits(dt, n)
    with make_comm(ring, protocol, n) as comm:
        h = immediate(comm, dt, bits)
        k = 0
        for coll in pc.COLLECTIVES:
            p, piece, c = 16 // e, 2048 // e, chunk_of(coll, protocol, e)
            for count in (p - 1, p, p + 1, piece - 1, piece, piece + 1, c - 1, c + 1, n * c + 1, 2 * n * c + 3):
                call = pc.make_call(oracle, oring, pc.spec(k, coll, "", count, dt, n), n, SEED, bits, protocol, 1)
                check_both(comm, call, h, (protocol, n, count), explicit=k % 2 == 0)
                k += 1


def test_flat_every_phase_mod_16(ring, oracle):
    dt, n = ae.BF16, 3
    e = rm.esz_of(dt)
    bits = pc.scalar_bits(dt, n)
    with make_comm(ring, "simple", n) as comm:
        h = immediate(comm, dt, bits)
        for phase in range(0, 16, e):
            for k, coll in enumerate(pc.COLLECTIVES):
                count = 2 * (16 // e) * 64 + 2 * (16 // e) + 1 + phase // e   # above one piece, an odd tail
                sp = pc.spec(k + phase // e, coll, "odd", count, dt, n)
                call = pc.make_call(oracle, oring, sp, n, SEED, bits, "simple", 1)
                check_both(comm, call, h, ("simple", n, "phase", phase), explicit=True, base_phase=phase)


@pytest.mark.parametrize("n", (9, 17))
def test_flat_more_ranks_than_one_group_of_loads(ring, oracle, n):
    """9 and 17 ranks: the scalars of the ranks beyond the first group of 8 loads, indexed by rank."""
    dt = ae.F16
    bits = pc.scalar_bits(dt, n)
    with make_comm(ring, "simple", n) as comm:
        h = immediate(comm, dt, bits)
        for k, coll in enumerate(pc.COLLECTIVES):
            count = n * chunk_of(coll, "simple", 2) + 1 if coll != "tree" else 3001
            sp = rm.Spec(k, coll, "nC+1", count, dt, rm.SUM, k % 2 == 1, (5 * k + 3) % n)
            call = pc.make_call(oracle, oring, sp, n, SEED, bits, "simple", 1)
            check_both(comm, call, h, ("simple", n), explicit=k % 2 == 1)


@pytest.mark.parametrize("protocol", ("simple", "ll128"))
def test_flat_two_channels(ring, oracle, protocol):
    """Several loops on each of two channels; the tree's second channel runs the other tree."""
    n = 4
    with make_comm(ring, protocol, n, 2) as comm:
        for k, coll in enumerate(pc.COLLECTIVES):
            dt = (ae.F32, ae.I32, ae.F64, ae.BF16)[k]
            bits = pc.scalar_bits(dt, n)
            h = immediate(comm, dt, bits)
            count = rm.LARGE[coll](n, chunk_of(coll, protocol, rm.esz_of(dt)))
            call = pc.make_call(oracle, oring, pc.spec(k, coll, "large", count, dt, n), n, SEED, bits, protocol, 2)
            check_both(comm, call, h, (protocol, n, 2), explicit=k % 2 == 0)


# ---- the other semantics, in a child process ---------------------------------------------------------------------------
_WORKER = r"""
import importlib, sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import oracle
from oracle import ring as oring
import arith_edges as ae, premul_cases as pc, ring_modes_cases as rm
import test_premul_gpu as t
oracle.lib()
oracle.set_semantics({mode})
nexr = importlib.import_module("nex-nccl_amd")
ring = importlib.import_module("nex-nccl_amd.ring")
assert nexr.get_semantics() == {mode}
n = 3
for protocol in ("simple", "ll"):
    with t.make_comm(ring, protocol, n) as comm:
        for k, coll in enumerate(pc.COLLECTIVES * 2):
            dt = (ae.F16, ae.I32, ae.F32, ae.I8, ae.BF16, ae.F64, ae.U8, ae.I64)[k]
            bits = pc.scalar_bits(dt, n)
            h = t.immediate(comm, dt, bits)
            count = n * t.chunk_of(coll, protocol, rm.esz_of(dt)) + n + 1
            call = pc.make_call(oracle, oring, pc.spec(k, coll, "nC+n+1", count, dt, n), n, t.SEED, bits, protocol, 1)
            t.check_both(comm, call, h, (protocol, n, {name!r}), explicit=k % 2 == 0)
            if {mode} == 2:   # shipped: a bit copy of one rank's input, whatever the scalars
                other = t.immediate(comm, dt, pc.rotate(bits))
                t.all_flat(comm, True)
                rm.check(call, t.run_on(comm, call, other), ("shipped", "other scalars"), expected=call.expected)
                t.all_flat(comm, False)
torch.cuda.synchronize()
print("PREMUL-OK")
"""


@pytest.mark.parametrize("name,mode", [("fork", 1), ("shipped", 2)])
def test_flat_under_the_other_semantics(nexr, name, mode):
    from conftest import GOLDEN, ROOT
    code = _WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=GOLDEN, mode=mode, name=name)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NEXR_SEMANTICS=name), capture_output=True,
                         text=True, timeout=150)
    assert out.returncode == 0 and "PREMUL-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ---- device-resident scalars --------------------------------------------------------------------------------------------
def _scalar_buffer(dt, n):
    """A device buffer and n element-aligned addresses in it that are not all 4-byte aligned for a 2-byte type."""
    e = rm.esz_of(dt)
    buf = torch.zeros(64 + 3 * e * n, dtype=torch.uint8, device="cuda")
    offs = [e + 3 * e * r for r in range(n)]
    return buf, offs, [buf.data_ptr() + o for o in offs]


def _fill(buf, offs, dt, bits):
    e = rm.esz_of(dt)
    host = np.zeros(buf.numel(), np.uint8)
    raw = pc.scalar_array(dt, bits).view(np.uint8)
    for r, o in enumerate(offs):
        host[o:o + e] = raw[r * e:(r + 1) * e]
    return host


@pytest.mark.parametrize("dt", (ae.BF16, ae.U8, ae.F32, ae.F64), ids=["bf16", "u8", "f32", "f64"])
def test_resident_scalars_are_read_during_every_call(ring, oracle, dt):
    """One handle, the buffer rewritten between the calls: host-sequenced and flat calls are each exact for the
    values then current."""
    n, protocol = 4, "simple"
    buf, offs, addrs = _scalar_buffer(dt, n)
    assert dt not in (ae.BF16,) or any(a % 4 for a in addrs)
    with make_comm(ring, protocol, n) as comm:
        h = comm.create_premul_sum(addrs, dt, pc.DEVICE)
        bits = pc.scalar_bits(dt, n)
        for k, coll in enumerate(pc.COLLECTIVES):
            count = n * chunk_of(coll, protocol, rm.esz_of(dt)) + n + 1
            for now in (bits, pc.rotate(bits), [bits[2]] * n):
                buf.copy_(torch.from_numpy(_fill(buf, offs, dt, now)))
                torch.cuda.synchronize()
                call = pc.make_call(oracle, oring, pc.spec(k, coll, "nC+n+1", count, dt, n), n, SEED, now, protocol, 1)
                check_both(comm, call, h, (protocol, coll, "resident", now), explicit=k % 2 == 0)


def _direct_case(oracle, dt, n, count, bits):
    e = rm.esz_of(dt)
    parts = [(off, cnt, chunk_of("all_reduce", "simple", e)) for _ch, off, cnt in oring.channel_parts(1, count, e, 2)]
    sp = pc.spec(0, "all_reduce", "direct", count, dt, n)
    return parts, sp


def test_a_copy_queued_before_the_launch_is_seen(nexr, oracle):
    """nexrFlatAllReducePreMul on a non-default stream: the scalars are copied into their buffer on that stream
    directly before the launch, nothing synchronises in between, and the kernel multiplies by them."""
    n, dt, count = 4, ae.F16, 5003
    bits = pc.scalar_bits(dt, n)
    parts, sp = _direct_case(oracle, dt, n, count, bits)
    call = pc.make_call(oracle, oring, sp, n, SEED, bits, "simple", 1)
    buf, offs, addrs = _scalar_buffer(dt, n)
    stale = torch.from_numpy(_fill(buf, offs, dt, pc.rotate(bits)))
    fresh = torch.from_numpy(_fill(buf, offs, dt, bits)).pin_memory()
    dev = torch.empty(call.arena0.size, dtype=torch.uint8, device="cuda")
    dev.copy_(torch.from_numpy(call.arena0))
    buf.copy_(stale)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        buf.copy_(fresh, non_blocking=True)
        nexr.flat_all_reduce_premul([dev.data_ptr() + o for o in call.send_off], [dev.data_ptr() + o for o in call.recv_off],
                                    count, dt, addrs, True, True, parts, stream=s.cuda_stream)
    s.synchronize()
    pc.check(call, dev.cpu().numpy(), ("stream", "copy before launch"))


def test_a_replayed_graph_reads_the_scalars_of_the_replay(nexr, oracle):
    """The four entries captured as single kernels; the scalar buffer is rewritten, the graph replayed: the bytes are
    those of the new values."""
    n, dt, count = 3, ae.F32, 4099
    bits = pc.scalar_bits(dt, n)
    later = pc.rotate(bits)
    parts, sp = _direct_case(oracle, dt, n, count, bits)
    tree = oring.tree_topology(n, rm.tree_per_node(n), 0)
    buf, offs, addrs = _scalar_buffer(dt, n)
    calls = {coll: pc.Call(pc.spec(k, coll, "graph", count, dt, n)._replace(in_place=False), n, SEED)
             for k, coll in enumerate(pc.COLLECTIVES)}
    devs = {coll: torch.empty(c.arena0.size, dtype=torch.uint8, device="cuda") for coll, c in calls.items()}

    def reset():
        for coll, c in calls.items():
            devs[coll].copy_(torch.from_numpy(c.arena0))

    def launch(stream):
        for coll, c in calls.items():
            base = devs[coll].data_ptr()
            ins, outs = [base + o for o in c.send_off], [base + o for o in c.recv_off]
            if coll == "all_reduce":
                nexr.flat_all_reduce_premul(ins, outs, count, dt, addrs, True, True, parts, stream=stream)
            elif coll == "reduce_scatter":
                nexr.flat_reduce_scatter_premul(ins, outs, count, dt, addrs, True, True, stream=stream)
            elif coll == "reduce":
                nexr.flat_reduce_premul(ins, outs[c.spec.root], c.spec.root, count, dt, addrs, True, True, stream=stream)
            else:
                nexr.flat_tree_all_reduce_premul(ins, outs, count, dt, addrs, True, True, [tree], [(0, count, 0)],
                                                 stream=stream)

    def verify(now, what):
        for coll, c in calls.items():
            c.set_outputs(pc.expected_outputs(oracle, oring, c, now, "simple", 1))
            pc.check(c, devs[coll].cpu().numpy(), (what, coll))

    reset()
    buf.copy_(torch.from_numpy(_fill(buf, offs, dt, bits)))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(torch.cuda.current_stream().cuda_stream)
    reset()
    buf.copy_(torch.from_numpy(_fill(buf, offs, dt, later)))
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    verify(later, "replay")


# ---- unchanged behaviour ------------------------------------------------------------------------------------------------
def test_built_in_ops_still_run_flat(ring, oracle):
    """set_flat with every bit and built-in ops: 4 reported and the bytes of rm's reference, as before."""
    n = 4
    with make_comm(ring, "simple", n, 2) as comm:
        comm.set_flat(True, tree=True, copies=True)
        for sp in rm.mixed_plan("simple", n, chunk_of, SEED + 5, calls=12):
            call = rm.make_call(sp, n, SEED, oring, "simple", 2)
            dev = torch.empty(call.arena0.size, dtype=torch.uint8, device="cuda")
            dev.copy_(torch.from_numpy(call.arena0))
            torch.cuda.synchronize()
            rm.issue(comm, call, dev.data_ptr())
            torch.cuda.synchronize()
            rm.check(call, dev.cpu().numpy(), ("built-in", "flat"))
            assert comm.queued() == 4, (sp.what(), comm.queued())


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_built_in_and_user_ops_alternate_with_the_options(ring, oracle, protocol):
    n = 4
    with make_comm(ring, protocol, n, 2) as comm:
        handles = {}
        for k in range(18):
            coll = pc.COLLECTIVES[k % 4]
            dt = pc.DTYPES[k % len(pc.DTYPES)]
            group, _direct = rm.mixed_state(protocol, k)
            (comm.set_simple_group if protocol == "simple" else comm.set_ll_group)(group)
            flat = (k // 2) % 2 == 1
            all_flat(comm, flat)
            count = chunk_of(coll, protocol, rm.esz_of(dt)) + k
            context = (protocol, k, coll, "flat" if flat else "", "group" if group else "")
            if k % 3 == 2:
                call = rm.make_call(rm.Spec(k, coll, "C+k", count, dt, rm.SUM, k % 2 == 1, k % n), n, SEED, oring,
                                    protocol, 2)
                got = run_on(comm, call, rm.SUM)
                rm.check(call, got, context + ("built-in",))
            else:
                bits = pc.scalar_bits(dt, n) if k % 2 else pc.rotate(pc.scalar_bits(dt, n))
                if (dt, tuple(bits)) not in handles:
                    handles[(dt, tuple(bits))] = immediate(comm, dt, bits)
                call = pc.make_call(oracle, oring, pc.spec(k, coll, "C+k", count, dt, n), n, SEED, bits, protocol, 2)
                pc.check(call, run_on(comm, call, handles[(dt, tuple(bits))]), context + ("user op",))
            if flat:
                assert comm.queued() == 4, (context, comm.queued())
            elif coll != "tree":
                assert comm.queued() != 4, (context, comm.queued())
