"""tests/ring_modes_cases.py without a GPU: the count tables reach the pack and chunk edges and the zero-element
chunks that tests/test_ring_modes_gpu.py exists for; its order-independent reference agrees bit for bit with
tests/arith_edges.py's folds in two orders and with oracle/ring.py's restatements of every collective; the whole
table and the mixed sequences are exact on host-memory communicators, the oracle serving every step of all three
protocols; and its checker rejects seeded errors."""
import ctypes
import importlib

import numpy as np
import pytest

import arith_edges as ae
import ring_modes_cases as rm
from oracle import ring as oring

SEED = rm.SEED


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


# ---- the tables ---------------------------------------------------------------------------------------------------
def test_chunk_counts_of_the_three_fifos():
    """oracle.ring.chunk_count at BUFF: SIMPLE 4 steps of 4 KiB a ring chunk and 1 a pipe or tree chunk, LL half
    of an 8 KiB step, LL128 15 / 16 of a 16 KiB step (a multiple of its 1,920-byte grain)."""
    for coll in rm.COLLECTIVES:
        ring_geom = coll in ("all_reduce", "reduce_scatter", "all_gather")
        for e in (1, 2, 4, 8):
            assert chunk_of(coll, "simple", e) * e == (16384 if ring_geom else 4096)
            assert chunk_of(coll, "ll", e) * e == 4096
            assert chunk_of(coll, "ll128", e) * e == 15360


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_every_table_has_the_pack_and_chunk_edges(protocol):
    for coll in rm.COLLECTIVES:
        for e in (1, 2, 4, 8):
            for n in rm.RANKS:
                p, c = 16 // e, chunk_of(coll, protocol, e)
                table = rm.count_table(n, e, c)
                assert len(set(table)) == len(table) and min(table) == 1
                want = {1, 2, n - 1, n, n + 1, p - 1, p, p + 1, n * p - 1, n * p, n * p + 1, c - 1, c, c + 1, n * c - 1,
                        n * c, n * c + 1, n * c + n + 1, 2 * n * c + 3}
                assert set(table) == {v for v in want if v >= 1}
                assert len(rm.raw_counts(n, e, c)) == 19


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
@pytest.mark.parametrize("n", rm.RANKS)
def test_every_collective_meets_every_datatype(protocol, n):
    specs = rm.plan(protocol, n, chunk_of)
    assert [s.k for s in specs] == list(range(len(specs)))
    assert {(s.dt, s.op) for s in specs} == set(rm.PAIRS)
    assert {s.op for s in specs} == {rm.SUM, rm.PROD, rm.MAX, rm.MIN, rm.AVG}
    for coll in rm.COLLECTIVES:
        mine = [s for s in specs if s.collective == coll]
        assert {s.dt for s in mine} == set(range(10)), coll
        assert {s.in_place for s in mine} == {False, True}, coll
        assert {s.root for s in mine} == set(range(n)), coll
        assert {s.edge for s in mine} >= {"1", "np-1", "np", "np+1", "C-1", "C", "C+1", "nC-1", "nC", "nC+1", "nC+n+1",
                                          "2nC+3"}, coll
        for s in mine:
            e = rm.esz_of(s.dt)
            assert s.count in rm.count_table(n, e, chunk_of(coll, protocol, e))


@pytest.mark.parametrize("n", rm.RANKS)
def test_all_reduce_tables_hold_chunks_of_zero_elements(n):
    """The zero-element-step condition: by the schedule's own formula every count up to (n - 1) p leaves at least
    one rank's chunk empty (nelem <= 0, which genericOp clamps to 0; the rank still waits, advances and posts),
    and every table and every plan holds such counts. Between (n - 1) p and n p the last chunk is short, not
    empty."""
    for e in (1, 2, 4, 8):
        p = 16 // e
        for count in range(1, n * p + 1):
            assert (rm.empty_chunks(n, e, count) > 0) == (count <= (n - 1) * p), (e, count)
        if n > 2:   # one element more than n packs: chunks of two packs, and the last rank's is empty again
            assert rm.empty_chunks(n, e, n * p + 1) > 0
        assert rm.empty_chunks(n, e, 1) == n - 1
        for protocol in rm.PROTO_ID:
            table = rm.count_table(n, e, chunk_of("all_reduce", protocol, e))
            assert sum(1 for c in table if rm.empty_chunks(n, e, c)) >= 2, (protocol, e)   # 1 and 2 at the least
    for protocol in rm.PROTO_ID:
        specs = [s for s in rm.plan(protocol, n, chunk_of) if s.collective == "all_reduce"]
        assert sum(1 for s in specs if rm.empty_chunks(n, rm.esz_of(s.dt), s.count)) >= 2, protocol


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
@pytest.mark.parametrize("n", rm.RANKS)
def test_mixed_plans_alternate_tiny_edge_and_two_channel_counts(protocol, n):
    specs = rm.mixed_plan(protocol, n, chunk_of, SEED + n)
    assert len(specs) == 24 and {s.collective for s in specs} == set(rm.COLLECTIVES)
    states = [rm.mixed_state(protocol, s.k) for s in specs]
    assert all(states[k] == states[k - k % 3] for k in range(24)) and all(states[k] != states[k - 3] for k in range(3, 24))
    assert set(states) == (set(rm.SIMPLE_STATES) if protocol == "simple" else {(False, False), (True, False)})
    for s in specs:
        e = rm.esz_of(s.dt)
        parts = oring.channel_parts(2, s.count, e, rm.TRAFFIC[s.collective](n), ll=protocol == "ll")
        c = chunk_of(s.collective, protocol, e)
        if s.k % 3 == 0:
            assert s.edge == "tiny" and 1 <= s.count < n * (16 // e) and len(parts) == 1
        elif s.k % 3 == 1:
            assert s.count in (c - 1, c, c + 1, n * c + 1)
        else:
            assert s.edge == "large" and len(parts) == 2, (s.what(), parts)
            loop = c * (n if s.collective == "all_reduce" else 1)
            assert max(cnt for _ch, _off, cnt in parts) > loop, (s.what(), parts)   # several loops (LL's split is uneven)


# ---- the reference ------------------------------------------------------------------------------------------------
def _dev_op(dt, op, n):
    """(devRedOp, arg, pre-op scalars, post-op) as hostToDevRedOp encodes the user's op, from arith_edges alone."""
    if op in (rm.SUM, rm.PROD):
        return (ae.SUM if op == rm.SUM else ae.PROD), 0, None, False
    if op in (rm.MAX, rm.MIN):
        return ae.MINMAX, ae.minmax_arg(dt, op == rm.MAX), None, False
    if dt in ae.INTS:
        return ae.SUMPOSTDIV, (n << 1) | int(dt in ae.SIGNED_INTS), None, True
    scalar = int(rm._to_bits(dt, np.array([1.0 / n]))[0])
    return ae.PREMULSUM, 0, [scalar] * n, False


@pytest.mark.parametrize("n", rm.RANKS)
def test_reduce_all_is_arith_edges_fold_in_either_order(n):
    """Source first or peer first, rank 0 first or last: the same bits, reduce_all's."""
    rng = np.random.default_rng(n)
    for dt, op in rm.PAIRS:
        xs = rm.gen_inputs(rng, dt, op, n, 48)
        red = rm.reduce_all(dt, op, xs)
        if dt in ae.FLOATS and op == rm.AVG and n == 3:
            assert red is None
            continue
        dev, arg, pre, post = _dev_op(dt, op, n)
        for order in (xs, xs[::-1], xs[1:] + xs[:1]):
            assert np.array_equal(ae.fold(dt, dev, arg, order, pre, post), red), (ae.NAMES[dt], op, "fold")
        acc = ae.fold_ll(dt, dev, arg, xs[:1], pre)                      # the LL chain: the peer's partial first
        for r in range(1, n):
            acc = ae.fold_ll(dt, dev, arg, [xs[r], acc], pre, post and r == n - 1)
        assert np.array_equal(acc, red), (ae.NAMES[dt], op, "fold_ll")


def test_copies_carry_nan_payloads():
    rng = np.random.default_rng(3)
    for dt in ae.FLOATS:
        x = rm.gen_inputs(rng, dt, None, 1, 1 << 16)[0]
        assert ae.is_nan(dt, x).any()


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
@pytest.mark.parametrize("n,channels", [(2, 1), (3, 1), (4, 2), (8, 1)])
def test_reference_agrees_with_oracle_ring(oracle, protocol, n, channels):
    """reduce_all against ring_allreduce_expected[_ll], reduce_scatter_expected, reduce_expected and the tree's
    expected function (all-gather and broadcast against theirs), over the table, bit for bit."""
    compared = 0
    for sp in rm.plan(protocol, n, chunk_of):
        call = rm.Call(sp, n, SEED)
        outs = call.outputs()
        if outs is None:
            assert n == 3 and sp.op == rm.AVG and sp.dt in ae.FLOATS
            continue
        theirs = rm.oracle_outputs(oring, call, protocol, channels)
        assert len(outs) == len(theirs) == n
        for r in range(n):
            assert (outs[r] is None) == (theirs[r] is None), (sp.what(), r)
            if outs[r] is not None:
                assert np.asarray(outs[r]).tobytes() == np.asarray(theirs[r]).tobytes(), (sp.what(), r)
        compared += 1
    assert compared >= 100


# ---- the host path ------------------------------------------------------------------------------------------------
def _host_comm(ring, fns, protocol, n, channels):
    f, fll, fll128 = fns
    return ring.RingComm(n, ring.HOST_MEMORY, rm.BUFF[protocol], f, 20000, rm.PROTO_ID[protocol], fll, fll128,
                         rm.tree_per_node(n), 0, channels)


def _run_on_host(comm, specs, protocol, n, channels, zero_counts):
    context = (protocol, "host memory", n, channels)
    seen = {}
    for sp in specs:
        call = rm.make_call(sp, n, SEED, oring, protocol, channels)
        seen[sp.collective] = seen.get(sp.collective, 0) + 1
        if zero_counts and seen[sp.collective] == 4:   # once per collective, between two calls of it
            arena = call.arena0.copy()
            rm.issue(comm, call, arena.ctypes.data, count=0)
            rm.check(call, arena, context + ("count 0",), expected=call.arena0)
        arena = call.arena0.copy()
        rm.issue(comm, call, arena.ctypes.data)
        rm.check(call, arena, context)
    assert not zero_counts or all(seen.get(c, 0) >= 4 for c in rm.COLLECTIVES)


@pytest.mark.parametrize("channels", rm.CHANNELS)
@pytest.mark.parametrize("n", rm.RANKS)
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_table_on_host_memory(ring, oracle, fns, protocol, n, channels):
    with _host_comm(ring, fns, protocol, n, channels) as comm:
        _run_on_host(comm, rm.plan(protocol, n, chunk_of), protocol, n, channels, True)


@pytest.mark.parametrize("n", rm.RANKS)
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_mixed_sizes_on_host_memory(ring, oracle, fns, protocol, n):
    with _host_comm(ring, fns, protocol, n, 2) as comm:
        _run_on_host(comm, rm.mixed_plan(protocol, n, chunk_of, SEED + n), protocol, n, 2, False)


# ---- the checker ---------------------------------------------------------------------------------------------------
def _synthetic(coll, n=4, count=None, in_place=False, root=1):
    e = 4
    c = chunk_of(coll, "simple", e)
    sp = rm.Spec(0, coll, "nC+n+1", n * c + n + 1 if count is None else count, ae.U32, rm.SUM, in_place, root)
    return rm.make_call(sp, n, SEED), c


def _rejects(call, got, *words):
    with pytest.raises(AssertionError) as err:
        rm.check(call, got, ("synthetic", call.n, 1))
    text = str(err.value)
    for w in ("synthetic", call.spec.collective, str(call.spec.count), "u32", "sum") + words:
        assert w in text, (w, text)


def test_the_checker_accepts_the_expected_bytes():
    for coll in rm.COLLECTIVES:
        for in_place in (False, True):
            call, _c = _synthetic(coll, in_place=in_place)
            rm.check(call, call.expected.copy())
            _rejects(call, call.arena0.copy())         # nothing ran


def test_the_checker_rejects_one_element_from_the_neighbouring_chunk():
    call, c = _synthetic("all_reduce")
    got = call.expected.copy()
    out = got[call.recv_off[2]:call.recv_off[2] + call.recv_elems * 4].view(np.uint32)
    assert out[c + 7] != out[7]
    out[7] = out[c + 7]
    _rejects(call, got, "rank 2", "output", "first differing element 7")


def test_the_checker_rejects_a_result_rotated_by_one_chunk():
    for coll in ("all_reduce", "tree", "all_gather"):
        call, c = _synthetic(coll)
        got = call.expected.copy()
        out = got[call.recv_off[3]:call.recv_off[3] + call.recv_elems * 4].view(np.uint32)
        out[:] = np.roll(out.copy(), c)
        _rejects(call, got, "rank 3", "output", "first differing element 0")


def test_the_checker_rejects_one_guard_byte():
    call, _c = _synthetic("reduce_scatter", count=5)
    for rank in range(call.n):
        for at, where in ((call.recv_off[rank] + 5 * 4, "guard behind"), (call.recv_off[rank] - 1, "guard before"),
                          (call.send_off[rank] - 1, "guard before"),
                          (call.send_off[rank] + call.send_elems * 4, "guard behind")):
            got = call.expected.copy()
            assert got[at] == rm.GUARD_BYTE
            got[at] ^= 1
            _rejects(call, got, "rank %d" % rank, where)
    assert call.arena0[-rm.GUARD:].tolist() == [rm.GUARD_BYTE] * rm.GUARD


def test_the_checker_rejects_a_written_non_root_reduce_output():
    call, _c = _synthetic("reduce", root=1)
    exp = call.expected[call.recv_off[1]:call.recv_off[1] + call.recv_elems * 4]
    for rank in (0, 2, 3):
        got = call.expected.copy()
        assert (got[call.recv_off[rank]:call.recv_off[rank] + call.recv_elems * 4] == rm.BLANK).all()
        got[call.recv_off[rank]:call.recv_off[rank] + call.recv_elems * 4] = exp    # the right sum at the wrong rank
        _rejects(call, got, "rank %d" % rank, "must stay untouched", "first differing element 0")
    got = call.expected.copy()
    got[call.send_off[2] + 8] ^= 0x80
    _rejects(call, got, "rank 2", "input", "first differing element 2")
