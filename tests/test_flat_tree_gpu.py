"""The flat tree all-reduce, broadcast and all-gather on the MI355X: nexrTreeAllReduceFlat / nexrRingBroadcastFlat /
nexrRingAllGatherFlat, the plain calls routed by set_flat's tree / copies bits, and nexrFlatTreeAllReduce /
nexrFlatBroadcast beneath them, on tests/flat_cases.py's order-sensitive inputs.

Two yardsticks for every call, both over the WHOLE arena (every output, every guard, every input):
  * the oracle's bytes: oracle/ring.py's recursive restatement of the tree for the communicator's protocol,
    channels and trees (float32 / float64 NaNs by class, as everywhere: tests/arith_edges.py canon);
  * the bytes of the same communicator's plain FIFO call with the option off, exactly.
No tolerance anywhere. The smallest FIFOs (ring_modes_cases.BUFF), device memory, thread ranks."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import arith_edges as ae
import flat_cases as fc
import flat_tree_cases as ftc
import ring_modes_cases as rm
import test_flat_tree as tt
from oracle import ring as oring

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = rm.SEED
TIMEOUT_MS = 20000


def chunk_of(coll, protocol, esz):
    return oring.chunk_count(coll, protocol, esz, rm.BUFF[protocol])


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("nex-nccl_amd.ring")


def make_comm(ring, protocol, n, channels, per_node=None, tree_index=0):
    per_node = rm.tree_per_node(n) if per_node is None else per_node
    return ring.RingComm(n, ring.DEVICE_MEMORY, rm.BUFF[protocol], None, TIMEOUT_MS, rm.PROTO_ID[protocol],
                         tree_ranks_per_node=per_node, tree_index=tree_index, n_channels=channels)


class _FlatEntries:
    """A RingComm whose tree all-reduce, broadcast and all-gather are the explicit *_flat entries (for rm.issue)."""

    def __init__(self, comm):
        self.tree_all_reduce, self.broadcast, self.all_gather = (comm.tree_all_reduce_flat, comm.broadcast_flat,
                                                                 comm.all_gather_flat)
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


def tree_call(sp, n, protocol, channels, per_node=None, tree_index=0):
    """The call with the oracle's bytes for the communicator make_comm builds from the same arguments."""
    per_node = rm.tree_per_node(n) if per_node is None else per_node
    call = fc.Call(sp, n, SEED)
    links_of = tt.links_of_channel(n, per_node, tree_index, channels)
    return call.set_outputs(oring.tree_allreduce_expected_channels(call.inputs, sp.dt, sp.op, links_of, channels,
                                                                   protocol))


def bits_of(collective):
    return {"tree": dict(tree=True), "all_gather": dict(copies=True), "broadcast": dict(copies=True)}[collective]


def check_both(comm, call, context, explicit, base_phase=0):
    """Plain with the option off, then flat (routed by set_flat's bit, or the explicit entry with the option off):
    flat against plain exactly, flat against the expected bytes."""
    comm.set_flat(False)
    plain = run_on(comm, call, base_phase)
    q0 = comm.queued()
    # (a plain tree call leaves the report as it was: it reports under set_ll_group only; an empty call runs nothing)
    if call.spec.collective != "tree" and call.spec.count:
        assert q0 != 4, (context, call.spec.what())
    if explicit:
        flat = run_on(_FlatEntries(comm), call, base_phase)
        assert comm.queued() == q0, (context, call.spec.what(), "an explicit flat entry leaves the report")
    else:
        comm.set_flat(False, **bits_of(call.spec.collective))
        flat = run_on(comm, call, base_phase)
        assert comm.queued() == 4, (context, call.spec.what(), comm.queued())
        comm.set_flat(False)
    rm.check(call, flat, context + ("flat against the plain FIFO call",), expected=plain)
    rm.check(call, fc.canon_outputs(call, flat), context + ("flat against the oracle",),
             expected=fc.canon_outputs(call, call.expected))


# ---- the table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree_index", (0, 1))
@pytest.mark.parametrize("channels", rm.CHANNELS)
@pytest.mark.parametrize("n", tt.RANKS)
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_table(ring, oracle, protocol, n, channels, tree_index):
    """test_flat_tree.py's table on device memory: every ranks-per-node of {n, 1, 2}, both tree indices, the ten
    counts; PAIRS cycled, in place on odd calls; calls routed by set_flat(tree=True) and through the explicit
    entry two by two."""
    k = 30 * tree_index
    for per_node in tt.per_nodes(n):
        with make_comm(ring, protocol, n, channels, per_node, tree_index) as comm:
            for slot in range(10):
                dt = rm.PAIRS[k % len(rm.PAIRS)][0]
                cs = tt.counts_of(protocol, rm.esz_of(dt))
                sp = rm.spec(k, "tree", "slot %d" % slot, cs[slot % len(cs)], n)
                call = tree_call(sp, n, protocol, channels, per_node, tree_index)
                check_both(comm, call, (protocol, n, channels, per_node, tree_index), explicit=(k // 2) % 2 == 1)
                k += 1


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_every_datatype_and_op(ring, oracle, protocol):
    """All ten datatypes x the five ops at 4 ranks (a rank with two children), the average of every datatype
    included: PreMulSum by 1 / 4 on every rank's own input for the floats, SumPostDiv at the root for the
    integers."""
    n = 4
    with make_comm(ring, protocol, n, 2, 1, 0) as comm:
        k = 0
        for dt in range(10):
            e = rm.esz_of(dt)
            for op in (rm.SUM, rm.PROD, rm.MAX, rm.MIN, rm.AVG):
                count = 2048 // e + 16 // e + 1
                sp = rm.Spec(k, "tree", "piece+pack+1", count, dt, op, k % 2 == 1, 0)
                check_both(comm, tree_call(sp, n, protocol, 2, 1, 0), (protocol, n, 2, ae.NAMES[dt], rm.OP_NAMES[op]),
                           explicit=k % 3 == 0)
                k += 1


def test_average_at_three_ranks(ring, oracle):
    """1 / 3 is no power of two: the pre-op's rounding on every rank's input shows."""
    n = 3
    for protocol in rm.PROTO_ID:
        with make_comm(ring, protocol, n, 1, 1, 1) as comm:
            for dt in range(10):
                sp = rm.Spec(dt, "tree", "avg", 2048 // rm.esz_of(dt) + 3, dt, rm.AVG, dt % 2 == 1, 0)
                check_both(comm, tree_call(sp, n, protocol, 1, 1, 1), (protocol, n, "avg"), explicit=dt % 2 == 0)


# ---- alignment --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", (ae.BF16, ae.U64), ids=["bf16", "u64"])
def test_every_phase_mod_16(ring, oracle, dt):
    """Element-aligned bases at every phase mod 16, in and out of place, two channels (a part boundary inside a
    piece's neighbourhood) and an odd tail."""
    e, n = rm.esz_of(dt), 4
    with make_comm(ring, "simple", n, 2, 1, 0) as comm:
        for phase in range(0, 16, e):
            count = tt.CELL["simple"] // e + 2 * (16 // e) * 64 + 1 + phase // e
            sp = rm.Spec(phase, "tree", "odd", count, dt, rm.SUM if dt == ae.BF16 else rm.PROD, (phase // e) % 2 == 1, 0)
            check_both(comm, tree_call(sp, n, "simple", 2, 1, 0), ("simple", n, 2, "phase", phase), explicit=True,
                       base_phase=phase)


def test_ranks_at_different_phases(nexr, oracle):
    """The direct entry with every rank's input and output at a phase of its own, two trees."""
    n, dt, count = 4, ae.F16, 1500
    rng = np.random.default_rng([SEED, 0xA12])
    xs = fc.gen_inputs(rng, dt, n, count)
    trees = [oring.tree_topology(n, 1, 0), oring.tree_topology(n, 1, 1)]
    parts = [(0, 1024, 0), (1024, count - 1024, 1)]
    want = ftc.model(xs, parts, trees, tt.step_of(oracle, "ll", dt, rm.SUM, n))[0]
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
    nexr.flat_tree_all_reduce([base + o for o in ins], [base + o for o in outs], count, dt, nexr.DevRedOp.Sum, 0, False,
                              trees, parts)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy(), exp)


# ---- NaN payloads -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("protocol", ("simple", "ll"))
def test_nan_payload_at_a_leaf_an_inner_rank_and_the_root(ring, oracle, protocol):
    """4 ranks, one per node: rank 0 is the root, rank 2 the inner rank with the leaves 1 and 3. A third of the
    positions holds a NaN with a payload at a leaf, a third at the inner rank, a third at the root, everything else
    finite: the leaf's bit copy, min / max keeping the first operand (which differs by protocol) and the sum's
    canonicalisation."""
    n = 4
    assert oring.tree_topology(n, 1, 0) == [(-1, [2]), (2, []), (0, [1, 3]), (2, [])]
    with make_comm(ring, protocol, n, 1, 1, 0) as comm:
        k = 0
        for dt in (ae.F16, ae.BF16, ae.F32):
            e = rm.esz_of(dt)
            e_bits, m_bits = ae.FMT[dt]
            count = 3 * (2048 // e) + 5
            holder = np.array([3, 2, 0, 1])[np.arange(count) % 4]       # leaf 3, inner 2, root 0, leaf 1
            for op in (rm.SUM, rm.MAX, rm.MIN):
                call = fc.Call(rm.Spec(k, "tree", "nan", count, dt, op, k % 2 == 1, 0), n, SEED)
                rng = np.random.default_rng([SEED, k])
                for r in range(n):
                    x = fc._finite(rng, dt, count)
                    nan = (((1 << e_bits) - 1) << m_bits) | (0x15 + r) | (r % 2) << (e_bits + m_bits)
                    x[holder == r] = nan
                    call.inputs[r] = x
                    call.arena0[call.send_off[r]:call.send_off[r] + count * e] = x.view(np.uint8)
                links_of = tt.links_of_channel(n, 1, 0, 1)
                call.set_outputs(oring.tree_allreduce_expected_channels(call.inputs, dt, op, links_of, 1, protocol))
                check_both(comm, call, (protocol, n, "nan"), explicit=k % 2 == 0)
                k += 1


# ---- many ranks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,per_node,tree_index", [(34, 2, 0), (64, 1, 1)])
def test_many_ranks(ring, oracle, n, per_node, tree_index):
    """The topology that needs the most live values (6 at 34 ranks, 2 per node, tree 0) and the most ranks a flat
    launch takes: 257 elements."""
    need = ftc.live_values(ftc.compile_tree(oring.tree_topology(n, per_node, tree_index)))
    assert need == 6 if n == 34 else need <= ftc.SLOTS
    with make_comm(ring, "simple", n, 1, per_node, tree_index) as comm:
        sp = rm.Spec(0, "tree", "257", 257, ae.F32, rm.SUM, False, 0)
        check_both(comm, tree_call(sp, n, "simple", 1, per_node, tree_index), ("simple", n, per_node, tree_index),
                   explicit=n == 64)


# ---- the other semantics, in a child process --------------------------------------------------------------------------
_WORKER = r"""
import importlib, sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import oracle
import ring_modes_cases as rm
import test_flat_tree as tt
import test_flat_tree_gpu as t
oracle.lib()
oracle.set_semantics({mode})
nexr = importlib.import_module("nex-nccl_amd")
ring = importlib.import_module("nex-nccl_amd.ring")
assert nexr.get_semantics() == {mode}
n = 4
for protocol in rm.PROTO_ID:
    for channels, tree_index in ((1, 0), (2, 1)):
        with t.make_comm(ring, protocol, n, channels, 1, tree_index) as comm:
            for k in range(10):
                dt = rm.PAIRS[k % len(rm.PAIRS)][0]
                cs = tt.counts_of(protocol, rm.esz_of(dt))
                sp = rm.spec(k, "tree", "slot", cs[k % len(cs)], n)
                call = t.tree_call(sp, n, protocol, channels, 1, tree_index)
                t.check_both(comm, call, (protocol, n, channels, {name!r}), explicit=k % 4 == 0)
torch.cuda.synchronize()
print("TABLE-OK")
"""


@pytest.mark.parametrize("name,mode", [("fork", 1), ("shipped", 2)])
def test_table_under_the_other_semantics(nexr, name, mode):
    """NEXR_SEMANTICS is read once per process: a child for each. Fork: signed min / max on the unsigned type;
    shipped: every reduce returns its first operand, so the result is one rank's input bit for bit (the root's
    for SIMPLE, the last leaf's of the last children for LL and LL128)."""
    assert hasattr(nexr, "get_semantics")
    from conftest import GOLDEN, ROOT
    code = _WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=GOLDEN, mode=mode, name=name)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NEXR_SEMANTICS=name), capture_output=True,
                         text=True, timeout=150)
    assert out.returncode == 0 and "TABLE-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ---- the entries themselves: many parts, streams, capture ----------------------------------------------------------------
def test_more_parts_than_the_kernel_arguments_hold(nexr, oracle):
    """300 parts alternating between two trees: beyond NEXR_FLAT_TREE_INLINE_PARTS the parts travel through the
    call's stream-ordered workspace."""
    n, dt, op = 4, ae.F32, rm.SUM
    dev_op, arg = oracle.host_to_dev_red_op(op, dt, n)
    trees = [oring.tree_topology(n, 1, 0), oring.tree_topology(n, 1, 1)]
    parts, at = [], 0
    for k in range(300):
        cnt = 8 * (1 + k % 5)
        parts.append((at, cnt, k % 2))
        at += cnt
    parts[-1] = (parts[-1][0], parts[-1][1] + 3, parts[-1][2])
    count = at + 3
    assert len(parts) > nexr.FLAT_TREE_INLINE_PARTS
    xs = fc.gen_inputs(np.random.default_rng([SEED, 3]), dt, n, count)
    want = ftc.model(xs, parts, trees, tt.step_of(oracle, "simple", dt, op, n))[0]
    ins = [torch.from_numpy(x.view(np.int32)).cuda() for x in xs]
    outs = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    nexr.flat_tree_all_reduce([t.data_ptr() for t in ins], [t.data_ptr() for t in outs], count, dt, dev_op, arg, True,
                              trees, parts)
    torch.cuda.synchronize()
    for t in outs:
        np.testing.assert_array_equal(ae.canon(dt, t.cpu().numpy().view(np.uint32)), ae.canon(dt, want))


def test_entries_on_a_stream_and_under_capture(nexr, oracle):
    """nexrFlatTreeAllReduce and nexrFlatBroadcast on a non-default stream, then captured into a HIP graph and
    replayed once on new inputs: stream-ordered single launches, nothing read from the caller's arrays after the
    call."""
    n, dt, op, count = 5, ae.F32, rm.SUM, 5003
    rng = np.random.default_rng([SEED, 4])
    dev_op, arg = oracle.host_to_dev_red_op(op, dt, n)
    step = tt.step_of(oracle, "simple", dt, op, n)
    trees = [oring.tree_topology(n, 1, 0), oring.tree_topology(n, 1, 1)]
    parts = [(0, 2048, 0), (2048, count - 2048, 1)]
    root = 3
    ins = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
    ar = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
    bc = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]

    def load():
        xs = fc.gen_inputs(rng, dt, n, count)
        for t, x in zip(ins, xs):
            t.copy_(torch.from_numpy(x.view(np.int32)))
        return xs

    def launch(stream):
        ip = [t.data_ptr() for t in ins]
        tl, pl = [list(t) for t in trees], list(parts)   # the caller's arrays die with this call
        nexr.flat_tree_all_reduce(ip, [t.data_ptr() for t in ar], count, dt, dev_op, arg, True, tl, pl, stream=stream)
        nexr.flat_broadcast(ip[root], [t.data_ptr() for t in bc], 4 * count - 1, stream=stream)
        del ip, tl, pl

    def verify(xs, what):
        want = ftc.model(xs, parts, trees, step)[0]
        for r in range(n):
            np.testing.assert_array_equal(ae.canon(dt, ar[r].cpu().numpy().view(np.uint32)), ae.canon(dt, want), what)
            got = bc[r].cpu().numpy().view(np.uint8)
            np.testing.assert_array_equal(got[:-1], xs[root].view(np.uint8)[:-1], what)
            assert got[-1] == 0, what   # nBytes = 4 * count - 1: the last byte is not written

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
    for t in ar + bc:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    verify(xs, "replay")


# ---- broadcast and all-gather ----------------------------------------------------------------------------------------------
BYTE_COUNTS = (1, 15, 16, 17, 2047, 2049, 0)


@pytest.mark.parametrize("n", (2, 3, 8))
def test_broadcast(ring, oracle, n):
    """Every root, in and out of place, byte counts round a pack and a piece and 0, the arena at a phase that
    changes call by call (uint8: pointers of any alignment); routed and explicit; against the FIFO broadcast's
    bytes and the expected ones."""
    with make_comm(ring, "simple", n, 1) as comm:
        k = 0
        for root in range(n):
            for nbytes in BYTE_COUNTS:
                for in_place in (False, True):
                    sp = rm.Spec(k, "broadcast", "bytes", nbytes, ae.U8, rm.SUM, in_place, root)
                    call = rm.make_call(sp, n, SEED)
                    check_both(comm, call, ("simple", n, "root", root), explicit=k % 2 == 1, base_phase=(5 * k + 1) % 16)
                    k += 1


@pytest.mark.parametrize("n", (2, 3, 8))
def test_all_gather(ring, oracle, n):
    with make_comm(ring, "simple", n, 1) as comm:
        k = 0
        for nbytes in BYTE_COUNTS:
            for in_place in (False, True):
                sp = rm.Spec(k, "all_gather", "bytes", nbytes, ae.U8, rm.SUM, in_place, 0)
                call = rm.make_call(sp, n, SEED)
                check_both(comm, call, ("simple", n), explicit=k % 2 == 1, base_phase=(5 * k + 1) % 16)
                k += 1


def test_broadcast_entry_with_every_pointer_at_its_own_phase(nexr):
    n, nbytes = 5, 4099
    rng = np.random.default_rng([SEED, 5])
    slot = 4608
    host = np.full(slot * (n + 1), rm.GUARD_BYTE, np.uint8)
    src = 64 + 7
    data = rng.integers(0, 256, nbytes, dtype=np.uint8)
    host[src:src + nbytes] = data
    outs = [slot * (r + 1) + 64 + (3 * r + 1) % 16 for r in range(n)]
    outs[2] = src                                                           # the root in place
    exp = host.copy()
    for o in outs:
        exp[o:o + nbytes] = data
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    nexr.flat_broadcast(dev.data_ptr() + src, [dev.data_ptr() + o for o in outs], nbytes)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(dev.cpu().numpy(), exp)


# ---- mixed with everything else on one communicator -------------------------------------------------------------------
SCOPES = ((0, {}), (1, dict(on=True)), (2, dict(tree=True)), (4, dict(copies=True)), (7, dict(on=True, tree=True, copies=True)),
          (3, dict(on=True, tree=True)), (5, dict(on=True, copies=True)), (6, dict(tree=True, copies=True)))
BIT = {"all_reduce": 1, "reduce_scatter": 1, "reduce": 1, "tree": 2, "all_gather": 4, "broadcast": 4}


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_mixed_sequence(ring, oracle, protocol):
    """24 seeded calls of all six collectives and the tree on one communicator of 2 channels; the scope bits change
    every three calls (all eight combinations) and the group / direct options as in ring_modes_cases.mixed_state;
    every fourth call goes through its explicit flat entry. Every result is exact, queued() is 4 exactly after the
    routed calls, an explicit entry and an unrouted tree call leave the report as it was, and no call is disturbed
    by the ones before it."""
    n = 4
    with make_comm(ring, protocol, n, 2) as comm:
        for sp in rm.mixed_plan(protocol, n, chunk_of, SEED + 78):
            group, direct = rm.mixed_state(protocol, sp.k)
            if protocol == "simple":
                comm.set_simple_group(group)
                comm.set_direct(direct)
            else:
                comm.set_ll_group(group)
            bits, kw = SCOPES[(sp.k // 3) % len(SCOPES)]
            comm.set_flat(kw.get("on", False), tree=kw.get("tree", False), copies=kw.get("copies", False))
            context = (protocol, n, 2, "bits %d" % bits, "group" if group else "", "direct" if direct else "")
            if sp.collective in fc.COLLECTIVES:
                call = fc.Call(sp, n, SEED)
                call.set_outputs(rm.oracle_outputs(oring, call, protocol, 2))
            elif sp.collective == "tree":
                call = tree_call(sp, n, protocol, 2)
            else:
                call = rm.make_call(sp, n, SEED, oring, protocol, 2)
            explicit = sp.k % 4 == 3
            q0 = comm.queued()
            got = run_on(_FlatEntries(comm) if explicit else comm, call)
            rm.check(call, fc.canon_outputs(call, got), context, expected=fc.canon_outputs(call, call.expected))
            routed = bool(bits & BIT[sp.collective]) and not explicit
            if routed:
                assert comm.queued() == 4, (context, sp.what(), comm.queued())
            elif explicit or (sp.collective == "tree" and not (group and protocol != "simple")):
                assert comm.queued() == q0, (context, sp.what(), comm.queued(), q0)   # the tree reports under set_ll_group only
            else:
                assert comm.queued() != 4, (context, sp.what(), comm.queued())


def test_set_flat_usage(ring, nexr):
    """The bits; one rank takes the one-rank path; count 0 succeeds."""
    RL = ring.ring_lib()
    with make_comm(ring, "simple", 2, 1) as comm:
        for bits in range(8):
            assert RL.nexrRingCommSetFlat(comm._h, bits) == nexr.Result.Success
        for bits in (8, 9, 16, -1, 1 << 20):
            assert RL.nexrRingCommSetFlat(comm._h, bits) == nexr.Result.InvalidArgument
        comm.set_flat(True, tree=True, copies=True)
        for fn in (comm.tree_all_reduce, comm.tree_all_reduce_flat):
            fn([1, 1], [1, 1], 0, ae.F32, rm.SUM)
        for fn in (comm.broadcast, comm.broadcast_flat):
            fn([1, 1], [1, 1], 0, ae.F32, 1)
        for fn in (comm.all_gather, comm.all_gather_flat):
            fn([1, 1], [1, 1], 0, ae.F32)
        with pytest.raises(nexr.NexrError) as e:
            comm.broadcast_flat([1, 1], [1, 1], 4, ae.F32, 2)
        assert e.value.code == nexr.Result.InvalidArgument
    with make_comm(ring, "simple", 1, 1) as comm:
        x = torch.arange(1, 9, dtype=torch.float32, device="cuda")
        y = torch.zeros_like(x)
        comm.set_flat(True, tree=True, copies=True)
        for fn in (comm.tree_all_reduce, comm.tree_all_reduce_flat):
            y.zero_()
            fn([x.data_ptr()], [y.data_ptr()], 8, ae.F32, rm.AVG)
            torch.cuda.synchronize()
            assert torch.equal(x, y)
        for fn in (comm.broadcast, comm.broadcast_flat):
            y.zero_()
            fn([x.data_ptr()], [y.data_ptr()], 8, ae.F32, 0)
            torch.cuda.synchronize()
            assert torch.equal(x, y)
