"""User-created PreMulSum ops with a scalar per rank (include/nexr_ring.h: nexrRingRedOpCreatePreMulSum,
nexrRingRedOpDestroy) without a GPU: the handle table's life cycle, every argument error (each answers before any
device call: the communicators here never touch HIP), and the ring, reduce-scatter, reduce and tree collectives
end to end on host-memory communicators whose every step is the oracle's, under SIMPLE, LL and LL128, against
tests/premul_cases.py's expected bytes."""
import ctypes
import importlib

import numpy as np
import pytest

import arith_edges as ae
import premul_cases as pc
import ring_modes_cases as rm
from oracle import ring as oring

SEED = rm.SEED ^ 0x504D
INVALID_ARGUMENT, INVALID_USAGE = 4, 5


def chunk_of(coll, protocol, esz):
    return oring.chunk_count(coll, protocol, esz, rm.BUFF[protocol])


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


@pytest.fixture(scope="module")
def fns(oracle):
    L = oracle.lib()
    cast = lambda f: ctypes.cast(f, ctypes.c_void_p).value  # noqa: E731
    return cast(L.oracle_reduce_copy_fn), cast(L.oracle_reduce_copy_ll_fn), cast(L.oracle_reduce_copy_ll128_fn)


def _comm(ring, fns, protocol, n, channels=1):
    f, fll, fll128 = fns
    return ring.RingComm(n, ring.HOST_MEMORY, rm.BUFF[protocol], f, 20000, rm.PROTO_ID[protocol], fll, fll128,
                         rm.tree_per_node(n), 0, channels)


def _op(comm, dt, bits):
    return comm.create_premul_sum(list(pc.scalar_array(dt, bits)), dt, pc.HOST_IMMEDIATE)


def _code(err):
    return err.value.code


# ---- the handle table ---------------------------------------------------------------------------------------------
def test_handles_start_at_five_are_reused_lifo_and_grow_past_four(ring, fns):
    with _comm(ring, fns, "simple", 2) as comm:
        bits = pc.scalar_bits(ae.F32, 2)
        first = [_op(comm, ae.F32, bits) for _ in range(4)]
        assert first == [5, 6, 7, 8]
        comm.destroy_op(6)
        comm.destroy_op(8)
        assert _op(comm, ae.F32, bits) == 8       # the last one destroyed comes back first
        assert _op(comm, ae.F32, bits) == 6
        more = [_op(comm, ae.F32, bits) for _ in range(5)]   # past the first capacity of 4, and past 8
        assert more == [9, 10, 11, 12, 13]
        for h in (5, 13, 9):
            comm.destroy_op(h)
        assert [_op(comm, ae.F32, bits) for _ in range(3)] == [9, 13, 5]
        assert _op(comm, ae.F32, bits) == 14


def test_create_rejects_bad_arguments(ring, fns, nexr):
    with _comm(ring, fns, "simple", 3) as comm:
        good = list(pc.scalar_array(ae.F32, pc.scalar_bits(ae.F32, 3)))
        for dt in (10, 11, 12, -1, 99):            # fp8 and unknown datatypes
            with pytest.raises(nexr.NexrError) as e:
                comm.create_premul_sum(good, dt, pc.HOST_IMMEDIATE)
            assert _code(e) == INVALID_ARGUMENT, dt
        for residence in (-1, 2):
            with pytest.raises(nexr.NexrError) as e:
                comm.create_premul_sum(good, ae.F32, residence)
            assert _code(e) == INVALID_ARGUMENT
        with pytest.raises(nexr.NexrError) as e:
            comm.create_premul_sum(None, ae.F32, pc.HOST_IMMEDIATE)
        assert _code(e) == INVALID_ARGUMENT
        for residence in (pc.HOST_IMMEDIATE, pc.DEVICE):
            for hole in range(3):
                vals = list(good) if residence == pc.HOST_IMMEDIATE else [4096] * 3   # kept, never read
                vals[hole] = None
                with pytest.raises(nexr.NexrError) as e:
                    comm.create_premul_sum(vals, ae.F32, residence)
                assert _code(e) == INVALID_ARGUMENT
        L = ring.ring_lib()
        ptrs = (ctypes.c_void_p * 3)(*[4096] * 3)
        assert L.nexrRingRedOpCreatePreMulSum(comm._h, None, ptrs, ae.F32, pc.DEVICE) == INVALID_ARGUMENT
        assert L.nexrRingRedOpCreatePreMulSum(None, ctypes.byref(ctypes.c_int()), ptrs, ae.F32, pc.DEVICE) == \
            INVALID_ARGUMENT
        assert _op(comm, ae.F32, pc.scalar_bits(ae.F32, 3)) == 5    # none of the failures took an entry


def test_destroy_rejects_built_ins_and_handles_that_are_not_live(ring, fns, nexr):
    with _comm(ring, fns, "simple", 2) as comm:
        for op in (0, 1, 2, 3, 4, -1, -1000):       # the built-ins, and garbage below them
            with pytest.raises(nexr.NexrError) as e:
                comm.destroy_op(op)
            assert _code(e) == INVALID_ARGUMENT, op
        for op in (5, 6, 1 << 20, 0x7FFFFFFF):      # never issued: the table is empty
            with pytest.raises(nexr.NexrError) as e:
                comm.destroy_op(op)
            assert _code(e) == INVALID_ARGUMENT, op
        h = _op(comm, ae.I32, pc.scalar_bits(ae.I32, 2))
        for op in (h + 1, h + 3, h + 4):             # inside the capacity but free, and past it
            with pytest.raises(nexr.NexrError) as e:
                comm.destroy_op(op)
            assert _code(e) == INVALID_ARGUMENT, op
        comm.destroy_op(h)
        with pytest.raises(nexr.NexrError) as e:     # twice
            comm.destroy_op(h)
        assert _code(e) == INVALID_ARGUMENT
        assert ring.ring_lib().nexrRingRedOpDestroy(None, 5) == INVALID_ARGUMENT


def _every_reduction(comm, s, d, count, dt, op):
    yield "all_reduce", lambda: comm.all_reduce(s, d, count, dt, op)
    yield "reduce_scatter", lambda: comm.reduce_scatter(s, d, count, dt, op)
    yield "reduce", lambda: comm.reduce(s, d, count, dt, op, 0)
    yield "tree", lambda: comm.tree_all_reduce(s, d, count, dt, op)


@pytest.mark.parametrize("n", [1, 3])
def test_collectives_reject_dead_handles_and_other_datatypes(ring, fns, nexr, n):
    """Use before create, past the capacity, after destroy, and with a datatype that is not the op's: every
    reduction entry answers InvalidArgument, writes nothing, and the communicator stays usable."""
    with _comm(ring, fns, "simple", n) as comm:
        x = [np.arange(64, dtype=np.float32) + r for r in range(n)]
        y = [np.full(64 * n, -1, np.float32) for _ in range(n)]
        s, d = [a.ctypes.data for a in x], [b.ctypes.data for b in y]

        def refused(op, dt, count=8):
            for name, call in _every_reduction(comm, s, d, count, dt, op):
                with pytest.raises(nexr.NexrError) as e:
                    call()
                assert _code(e) == INVALID_ARGUMENT, (name, op, dt)
            assert all((b == -1).all() for b in y)

        refused(5, ae.F32)                            # never issued
        h = _op(comm, ae.F32, pc.scalar_bits(ae.F32, n))
        assert h == 5
        for dt in (ae.F64, ae.I32, ae.U32, ae.F16):   # not the op's datatype
            refused(h, dt)
        for dt in (10, 11, 12):
            refused(h, dt)
        refused(h + 1, ae.F32)                        # free, inside the capacity
        refused(h + 4, ae.F32)                        # past the capacity
        refused(-3, ae.F32)
        comm.all_reduce(s, d, 8, ae.F32, h)           # the live handle works
        assert not (y[0][:8] == -1).any()
        for b in y:
            b[:] = -1
        comm.destroy_op(h)
        refused(h, ae.F32)                            # after destroy
        comm.all_reduce(s, d, 8, ae.F32, rm.SUM)
        assert np.array_equal(y[0][:8], sum(a[:8] for a in x))


def test_entries_that_take_no_user_op_still_refuse_one(ring, fns, nexr):
    """The symmetric entries are Sum only: a live handle is InvalidArgument there, as op 5 is without this."""
    with _comm(ring, fns, "simple", 2) as comm:
        h = _op(comm, ae.F32, pc.scalar_bits(ae.F32, 2))
        x = [np.zeros(16, np.float32) for _ in range(2)]
        p = [a.ctypes.data for a in x]
        for call in (lambda: comm.all_reduce_symmetric(p, p, 16, ae.F32, h),
                     lambda: comm.reduce_scatter_symmetric(p, p, 8, ae.F32, h),
                     lambda: comm.all_reduce_symmetric_ll(p, p, 16, ae.F32, h),
                     lambda: comm.reduce_scatter_symmetric_ll(p, p, 8, ae.F32, h)):
            with pytest.raises(nexr.NexrError) as e:
                call()
            assert _code(e) == INVALID_ARGUMENT


# ---- end to end on host memory ------------------------------------------------------------------------------------
def _run_plan(oracle, comm, specs, protocol, n, channels):
    context = (protocol, "host memory", n, channels)
    ops = {}
    for sp in specs:
        bits = pc.scalar_bits(sp.dt, n)
        if sp.dt not in ops:
            ops[sp.dt] = _op(comm, sp.dt, bits)
        call = pc.make_call(oracle, oring, sp, n, SEED, bits, protocol, channels)
        arena = call.arena0.copy()
        rm.issue(comm, _with_op(call, ops[sp.dt]), arena.ctypes.data)
        pc.check(call, arena, context)
    return ops


class _WithOp:
    """A call as rm.issue reads it, its spec's op replaced by a handle."""

    def __init__(self, call, op):
        self.spec = call.spec._replace(op=op)
        self.send_off, self.recv_off = call.send_off, call.recv_off


def _with_op(call, op):
    return _WithOp(call, op)


@pytest.mark.parametrize("channels", rm.CHANNELS)
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_table_on_host_memory(ring, oracle, fns, protocol, n, channels):
    """Every collective at every edge of the count table (1 element to 2nC + 3) on the smallest FIFOs, the six
    datatypes in turn, in place and out of place, every root; distinct scalars per rank."""
    specs = pc.plan(protocol, n, chunk_of)
    for coll in pc.COLLECTIVES:
        mine = [s for s in specs if s.collective == coll]
        assert {s.dt for s in mine} == set(pc.DTYPES) and {s.root for s in mine} == set(range(n)), coll
        assert {s.in_place for s in mine} == {False, True}
    with _comm(ring, fns, protocol, n, channels) as comm:
        ops = _run_plan(oracle, comm, specs, protocol, n, channels)
        assert sorted(ops.values()) == list(range(5, 5 + len(pc.DTYPES)))


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_two_channel_counts_on_host_memory(ring, oracle, fns, protocol, n):
    """The LARGE counts: several loops on each of two channels (the tree's second channel runs the other tree)."""
    specs = []
    for k, coll in enumerate(pc.COLLECTIVES * 2):
        dt = pc.DTYPES[k % len(pc.DTYPES)]
        count = rm.LARGE[coll](n, chunk_of(coll, protocol, rm.esz_of(dt)))
        specs.append(pc.spec(k, coll, "large", count, dt, n))
    with _comm(ring, fns, protocol, n, 2) as comm:
        _run_plan(oracle, comm, specs, protocol, n, 2)


@pytest.mark.parametrize("n", [2, 3, 4])
@pytest.mark.parametrize("dt", pc.DTYPES, ids=[ae.NAMES[d] for d in pc.DTYPES])
def test_rotating_the_scalars_changes_the_expected_bytes(oracle, dt, n):
    """Otherwise an indexing error (scalars by position in the chain, not by rank) could not show."""
    bits = pc.scalar_bits(dt, n)
    assert len(set(bits)) == n
    if dt in ae.FLOATS:
        for v in pc.scalar_values(dt, n):
            m = abs(v)
            while m != int(m):
                m *= 2
            assert int(m) & (int(m) - 1), v      # not a power of two
    for protocol in rm.PROTO_ID:
        for k, coll in enumerate(pc.COLLECTIVES):
            count = n * chunk_of(coll, protocol, rm.esz_of(dt)) + n + 1
            call = pc.make_call(oracle, oring, pc.spec(k, coll, "nC+n+1", count, dt, n), n, SEED, bits, protocol, 1)
            other = pc.expected_arena(oracle, oring, call, pc.rotate(bits), protocol, 1)
            assert not np.array_equal(call.expected, other), (protocol, coll)


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
@pytest.mark.parametrize("dt", ae.FLOATS, ids=[ae.NAMES[d] for d in ae.FLOATS])
def test_equal_scalars_of_one_over_n_are_ncclavg(ring, oracle, fns, dt, protocol):
    """Pinned against the existing path: a user op whose n scalars are the bits nexrHostToDevRedOp gives ncclAvg
    produces ncclAvg's bytes."""
    for n in (1, 3, 4):
        dev_op, arg = oracle.host_to_dev_red_op(rm.AVG, dt, n)
        assert dev_op == ae.PREMULSUM
        with _comm(ring, fns, protocol, n, 2) as comm:
            h = _op(comm, dt, [arg] * n)
            for k, coll in enumerate(pc.COLLECTIVES):
                count = n * chunk_of(coll, protocol, rm.esz_of(dt)) + n + 1
                call = pc.Call(pc.spec(k, coll, "nC+n+1", count, dt, n), n, SEED)
                avg, user = call.arena0.copy(), call.arena0.copy()
                rm.issue(comm, _with_op(call, rm.AVG), avg.ctypes.data)
                rm.issue(comm, _with_op(call, h), user.ctypes.data)
                assert n == 1 or not np.array_equal(avg, call.arena0)   # (times 1.0 in place changes nothing)
                rm.check(call, user, (protocol, n, coll, "user op against avg"), expected=avg)


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_a_resident_scalar_is_read_during_every_call(ring, oracle, fns, protocol):
    """Device residence on a communicator that never touches HIP: the addresses are the host's. One handle, the
    scalar buffer rewritten between two calls, each call exact for the values then current."""
    n, dt = 3, ae.BF16
    bits = pc.scalar_bits(dt, n)
    buf = pc.scalar_array(dt, bits)
    with _comm(ring, fns, protocol, n) as comm:
        h = comm.create_premul_sum([buf.ctypes.data + r * buf.itemsize for r in range(n)], dt, pc.DEVICE)
        for k, coll in enumerate(pc.COLLECTIVES):
            count = n * chunk_of(coll, protocol, rm.esz_of(dt)) + n + 1
            for now in (bits, pc.rotate(bits), bits[::-1]):
                buf[:] = pc.scalar_array(dt, now)
                call = pc.make_call(oracle, oring, pc.spec(k, coll, "nC+n+1", count, dt, n), n, SEED, now, protocol, 1)
                arena = call.arena0.copy()
                rm.issue(comm, _with_op(call, h), arena.ctypes.data)
                pc.check(call, arena, (protocol, coll, "resident", now))


def test_built_in_and_user_ops_alternate_on_one_communicator(ring, oracle, fns):
    n = 4
    with _comm(ring, fns, "simple", n, 2) as comm:
        handles = {}
        for k in range(16):
            coll = pc.COLLECTIVES[k % 4]
            dt = pc.DTYPES[k % len(pc.DTYPES)]
            count = chunk_of(coll, "simple", rm.esz_of(dt)) + k
            if k % 3 == 2:   # a built-in op of rm's order-independent inputs
                call = rm.make_call(rm.Spec(k, coll, "C+k", count, dt, rm.SUM, k % 2 == 1, k % n), n, SEED, oring,
                                    "simple", 2)
                arena = call.arena0.copy()
                rm.issue(comm, call, arena.ctypes.data)
                rm.check(call, arena, ("built-in", k))
                continue
            bits = pc.scalar_bits(dt, n) if k % 2 else pc.rotate(pc.scalar_bits(dt, n))
            if k % 4 == 0 and handles:
                comm.destroy_op(handles.pop(next(iter(handles))))
            if (dt, tuple(bits)) not in handles:
                handles[(dt, tuple(bits))] = _op(comm, dt, bits)
            call = pc.make_call(oracle, oring, pc.spec(k, coll, "C+k", count, dt, n), n, SEED, bits, "simple", 2)
            arena = call.arena0.copy()
            rm.issue(comm, _with_op(call, handles[(dt, tuple(bits))]), arena.ctypes.data)
            pc.check(call, arena, ("user op", k))


# ---- the launches with a scalar per rank: what answers without a device -------------------------------------------
def test_flat_premul_entries_reject_bad_scalars(nexr):
    """A null scalar array, and with scalarsArePtrs a null or misaligned entry: InvalidArgument from all four
    entries, before any device call (host addresses serve)."""
    x = np.zeros(64, np.float32)
    a = x.ctypes.data
    p = [a] * 2
    for scalars, ptrs in ((None, False), (None, True), ([a, 0], True), ([a, a + 2], True)):
        for call in (lambda: nexr.flat_all_reduce_premul(p, p, 16, ae.F32, scalars, ptrs, True, [(0, 16, 4)]),
                     lambda: nexr.flat_reduce_scatter_premul(p, p, 8, ae.F32, scalars, ptrs, True),
                     lambda: nexr.flat_reduce_premul(p, a, 0, 16, ae.F32, scalars, ptrs, True),
                     lambda: nexr.flat_tree_all_reduce_premul(p, p, 16, ae.F32, scalars, ptrs, True,
                                                              [[(-1, [1]), (0, [])]], [(0, 16, 0)])):
            with pytest.raises(nexr.NexrError) as e:
                call()
            assert _code(e) == INVALID_ARGUMENT, (scalars, ptrs)
    good = [0x3FC00000, 0x40100000]
    for dt in (10, 11, 12):   # the plain entries' own checks come first: fp8, an unknown datatype, one rank
        with pytest.raises(nexr.NexrError) as e:
            nexr.flat_all_reduce_premul(p, p, 16, dt, good, False, True, [(0, 16, 4)])
        assert _code(e) == INVALID_ARGUMENT
    with pytest.raises(nexr.NexrError) as e:
        nexr.flat_reduce_premul(p[:1], a, 0, 16, ae.F32, good[:1], False, True)
    assert _code(e) == INVALID_ARGUMENT
    nexr.flat_all_reduce_premul(p, p, 0, ae.F32, good, False, True, [])   # nothing to do: no launch


def test_the_per_rank_kernels_are_ten_and_ten_without_scratch():
    """One instance per datatype of flat_premul_kernel and of flat_tree_premul_kernel, each with no private segment
    and no spilled vector register; the tree's name holds "flat_tree" (tests/test_flat_tree.py's scratch check
    covers it) and not "flat_tree_kernel" (its count of 46 stands)."""
    import os

    import test_code_objects as tco
    path = os.path.join(tco.PKG, "libnexr.so")
    assert os.path.exists(path), "libnexr.so not built"
    seen = {}
    for co in tco.gfx950_code_objects(tco._read(path)):
        _tables, notes = tco.elf_tables(co)
        for k in (k for note in notes for k in note["amdhsa.kernels"]):
            if "premul_kernel" in k[".name"]:
                seen[k[".name"]] = (k[".private_segment_fixed_size"], k.get(".vgpr_spill_count", 0),
                                    k.get(".uses_dynamic_stack", False))
    ring_k = [name for name in seen if "flat_premul_kernel" in name]
    tree_k = [name for name in seen if "flat_tree_premul_kernel" in name]
    assert len(ring_k) == 10 and len(tree_k) == 10 and len(seen) == 20, sorted(seen)
    assert all("flat_tree" in name and "flat_tree_kernel" not in name for name in tree_k)
    assert all("flat_kernel" not in name for name in seen)
    assert {name: v for name, v in seen.items() if v != (0, 0, False)} == {}
