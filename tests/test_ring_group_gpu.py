"""nexrRingGroupStart / nexrRingGroupEnd on the MI355X: the collectives recorded between the two run as flat group
launches where they would run flat, and alone at their place otherwise; every arena afterwards holds the bytes of
the same call made alone (the whole arena: outputs, guards, inputs), which are the oracle's and the FIFO ring's."""
import importlib

import numpy as np
import pytest

import arith_edges as ae
import ring_modes_cases as rm
import test_flat as tf
from oracle import ring as oring

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = rm.SEED
chunk_of = tf.chunk_of
FIVE = ("all_reduce", "reduce_scatter", "reduce", "all_gather", "broadcast")


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("nex-nccl_amd.ring")


def make_comm(ring, protocol, n, channels):
    return ring.RingComm(n, ring.DEVICE_MEMORY, rm.BUFF[protocol], None, 20000, rm.PROTO_ID[protocol],
                         tree_ranks_per_node=rm.tree_per_node(n), n_channels=channels)


def on_device(calls):
    devs = []
    for call in calls:
        d = torch.empty(call.arena0.size, dtype=torch.uint8, device="cuda")
        d.copy_(torch.from_numpy(call.arena0))
        devs.append(d)
    torch.cuda.synchronize()
    return devs


def run(comm, calls, grouped):
    """The calls on fresh copies of their arenas, inside one group or one by one; the arenas afterwards."""
    devs = on_device(calls)
    if grouped:
        with comm.group():
            for call, d in zip(calls, devs):
                rm.issue(comm, call, d.data_ptr())
    else:
        for call, d in zip(calls, devs):
            rm.issue(comm, call, d.data_ptr())
    torch.cuda.synchronize()
    return [d.cpu().numpy() for d in devs]


def kinds(oracle, calls, n):
    """The launches a group of independent calls needs: one per (datatype, device op, min-or-max), one for copies."""
    ks = set()
    for call in calls:
        sp = call.spec
        if sp.collective in ("all_gather", "broadcast"):
            ks.add("copy")
        else:
            dev_op, arg = oracle.host_to_dev_red_op(sp.op, sp.dt, n)
            ks.add((sp.dt, dev_op, arg & 1 if dev_op == 2 else 0))
    return len(ks)


def mixed_calls(protocol, n, channels, how_many=8):
    """The first calls of ring_modes_cases' count table that cover the five collectives and two datatypes."""
    specs = [sp for sp in rm.plan(protocol, n, chunk_of, FIVE)]
    picked, seen = [], set()
    for sp in specs:                                  # one of each collective first
        if sp.collective not in seen:
            seen.add(sp.collective)
            picked.append(sp)
    for sp in specs[::7]:
        if len(picked) < how_many and sp not in picked:
            picked.append(sp)
    assert len(picked) >= 6 and len({sp.dt for sp in picked}) >= 2 and {sp.collective for sp in picked} == set(FIVE)
    return [rm.make_call(sp, n, SEED, oring, protocol, channels) for sp in picked]


@pytest.mark.parametrize("channels", (1, 2))
@pytest.mark.parametrize("n", (2, 4, 8))
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_mixed_group(ring, oracle, protocol, n, channels):
    context = (protocol, n, channels)
    calls = mixed_calls(protocol, n, channels)
    with make_comm(ring, protocol, n, channels) as comm:
        comm.set_flat(True, copies=True)
        single = run(comm, calls, False)
        assert comm.queued() == 4
        comm.group_stats(reset=True)
        grouped = run(comm, calls, True)
        stats = comm.group_stats()
        assert comm.queued() == 5, context
        assert stats == {"calls": len(calls), "group_launches": kinds(oracle, calls, n), "fill_launches": stats["fill_launches"],
                         "singles": 0, "cuts": 0}, (context, stats)
        for call, g, s in zip(calls, grouped, single):
            rm.check(call, g, context + ("group against the single flat calls",), expected=s)
            rm.check(call, g, context + ("group against the oracle",))
        if protocol == "simple":                      # and the FIFO ring's own bytes
            comm.set_flat(False)
            fifo = run(comm, calls, False)
            assert comm.queued() not in (4, 5)
            for call, g, f in zip(calls, grouped, fifo):
                rm.check(call, g, context + ("group against the FIFO ring",), expected=f)


def test_dependent_pair_cuts_once(ring, oracle):
    """An all-reduce whose outputs are the inputs of a reduce of the same kind: one cut, two launches, the bytes of
    the two calls in order."""
    n, count = 4, 3000
    with make_comm(ring, "simple", n, 1) as comm:
        comm.set_flat(True)
        x = [torch.arange(count, dtype=torch.int32, device="cuda") * (r + 1) for r in range(n)]
        y = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
        z = torch.zeros(count, dtype=torch.int32, device="cuda")
        other = [torch.ones(count, dtype=torch.int32, device="cuda") for _ in range(n)]
        out = [torch.zeros(count, dtype=torch.int32, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        comm.group_stats(reset=True)
        with comm.group():
            comm.all_reduce([t.data_ptr() for t in x], [t.data_ptr() for t in y], count, ae.I32, rm.SUM)
            comm.all_reduce([t.data_ptr() for t in other], [t.data_ptr() for t in out], count, ae.I32, rm.SUM)
            comm.reduce([t.data_ptr() for t in y], [z.data_ptr()] * n, count, ae.I32, rm.SUM, 2)
        torch.cuda.synchronize()
        stats = comm.group_stats()
        assert stats["cuts"] == 1 and stats["group_launches"] == 2 and stats["singles"] == 0, stats
        total = sum(r + 1 for r in range(n))
        want = np.arange(count, dtype=np.int64) * total
        for t in y:
            np.testing.assert_array_equal(t.cpu().numpy(), want.astype(np.int32))
        np.testing.assert_array_equal(z.cpu().numpy(), (want * n).astype(np.int32))
        for t in out:
            np.testing.assert_array_equal(t.cpu().numpy(), np.full(count, n, np.int32))


def test_tree_and_per_rank_ops_run_singly_at_their_place(ring, oracle):
    """A tree all-reduce and an all-reduce under a PreMulSum op with a scalar per rank inside a group: each ends the
    run of flat works and executes alone; the flat calls around them still go out as group launches."""
    n, protocol = 4, "simple"
    specs = [rm.Spec(k, coll, "x", 1000 + 37 * k, ae.F32, rm.SUM, False, k % n)
             for k, coll in enumerate(("all_reduce", "tree", "reduce_scatter", "all_reduce", "reduce"))]
    calls = [rm.make_call(sp, n, SEED, oring, protocol, 1) for sp in specs]
    with make_comm(ring, protocol, n, 1) as comm:
        comm.set_flat(True)
        user = comm.create_premul_sum([np.float32(1 + r) for r in range(n)], ae.F32)

        def issue_all(devs):
            for k, (call, d) in enumerate(zip(calls, devs)):
                if k == 3:      # the per-rank op: only the op differs from the spec
                    s = [d.data_ptr() + o for o in call.send_off]
                    r = [d.data_ptr() + o for o in call.recv_off]
                    comm.all_reduce(s, r, call.spec.count, ae.F32, user)
                else:
                    rm.issue(comm, call, d.data_ptr())

        single = on_device(calls)
        issue_all(single)
        torch.cuda.synchronize()
        grouped = on_device(calls)
        comm.group_stats(reset=True)
        with comm.group():
            issue_all(grouped)
        torch.cuda.synchronize()
        stats = comm.group_stats()
        assert stats["calls"] == 5 and stats["singles"] == 2 and stats["group_launches"] == 3, stats
        for k, (call, g, s) in enumerate(zip(calls, grouped, single)):
            rm.check(call, g.cpu().numpy(), ("singly", k), expected=s.cpu().numpy())
            if k != 3:
                rm.check(call, g.cpu().numpy(), ("singly", k, "oracle"))
        comm.destroy_op(user)


def test_set_flat_between_groups_and_calls_after_a_group(ring, oracle):
    n, protocol = 2, "ll"
    calls = mixed_calls(protocol, n, 1, 6)
    with make_comm(ring, protocol, n, 1) as comm:
        comm.group_stats(reset=True)
        off = run(comm, calls, True)                  # the option off: every call runs alone through the FIFOs
        stats = comm.group_stats(reset=True)
        assert stats["singles"] == len(calls) and stats["group_launches"] == 0 and comm.queued() != 5
        comm.set_flat(True, copies=True)
        on = run(comm, calls, True)
        stats = comm.group_stats(reset=True)
        assert stats["singles"] == 0 and stats["group_launches"] >= 2 and comm.queued() == 5
        comm.set_flat(True)                           # copies off again: they run alone, the reductions grouped
        part = run(comm, calls, True)
        stats = comm.group_stats(reset=True)
        copies = sum(c.spec.collective in ("all_gather", "broadcast") for c in calls)
        assert stats["singles"] == copies and stats["group_launches"] >= 1
        comm.set_flat(False)
        after = run(comm, calls, False)               # FIFO calls after the groups
        assert comm.queued() not in (4, 5)
        first = next(c for c in calls if c.spec.collective == "all_reduce")
        explicit = on_device([first])                 # and an explicit flat entry
        sp = first.spec
        for call, a, b, c, d in zip(calls, off, on, part, after):
            rm.check(call, a, ("off",))
            rm.check(call, b, ("on",), expected=a)
            rm.check(call, c, ("reductions only",), expected=a)
            rm.check(call, d, ("after",), expected=a)
        base = explicit[0].data_ptr()
        comm.all_reduce_flat([base + o for o in first.send_off], [base + o for o in first.recv_off], sp.count, sp.dt,
                             sp.op)
        torch.cuda.synchronize()
        rm.check(first, explicit[0].cpu().numpy(), ("explicit flat after the groups",))
