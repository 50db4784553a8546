"""tests/ring_host_cases.py without a GPU, and what of tests/test_ring_host_memory_gpu.py runs without one: the
placements keep rm's alignment and fit the mapping, split's cut is a page boundary inside the arena and, for all
but a counted few arenas, inside a user buffer; the SIMPLE table with set_direct on a host-memory communicator
(tests/test_ring_modes.py runs it with the option off only) and the one-rank cases, the oracle serving every
step, on arenas the helper placed; and the checker rejects, on such an arena, what a wrong interior-pointer
translation and a write past a buffer would leave."""
import ctypes
import importlib

import numpy as np
import pytest

import arith_edges as ae
import ring_host_cases as rh
import ring_modes_cases as rm
from oracle import ring as oring

SEED = rm.SEED
one_rank_plan, check_direct = rh.one_rank_plan, rh.check_direct


def chunk_of(coll, protocol, esz):
    return oring.chunk_count(coll, protocol, esz, rm.BUFF[protocol])


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


@pytest.fixture(scope="module")
def fn(oracle):
    return ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value


# ---- the helper ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", rm.RANKS)
def test_placements_of_every_arena_of_the_table(n):
    """Every kind: the arena starts at a multiple of 16, a page or more into the mapping, and ends inside it.
    split: the cut is a page boundary of the mapping, strictly inside the arena, everything below it registered
    from the mapping's base and nothing above. It lies strictly inside a user buffer except where the buffer at
    the arena's middle has 16 bytes or fewer (count <= p: no multiple of 16 is strictly inside it); there it is
    that buffer's first byte. Those are 34, 30, 27 and 23 of the 114 (112 at 8 ranks) arenas of the table at 2, 3,
    4 and 8 ranks, counted below."""
    calls = [rm.Call(sp, n, SEED) for sp in rm.plan("simple", n, chunk_of)]
    size = rh.mapping_bytes(rh.largest_arena(calls))
    assert size % rh.PAGE == 0 and size >= max(c.arena0.size for c in calls) + 2 * rh.PAGE
    in_guard = []
    for call in calls:
        nbytes = call.arena0.size
        for kind in rh.KINDS:
            pl = rh.place(kind, nbytes, size, call.regions)
            assert pl.offset % 16 == 0 and rh.PAGE <= pl.offset and pl.offset + nbytes <= size, (call.spec.what(), pl)
            if kind != "split":
                assert pl.offset == rh.PAGE + 48 and pl.cut is None
                assert pl.registered == (size if kind == "registered" else None)
                continue
            assert pl.cut % 16 == 0 and 0 < pl.cut < nbytes
            assert (pl.offset + pl.cut) % rh.PAGE == 0 and pl.registered == pl.offset + pl.cut
            reg = rh.cut_region(call, pl)
            if reg is None:
                in_guard.append(call.spec)
                assert any(pl.cut == off and nbytes <= 16 for _r, _k, off, nbytes in call.regions), call.spec.what()
                assert call.spec.count * call.esz <= 16, call.spec.what()
            else:
                assert reg[2] < pl.cut < reg[2] + reg[3]
    assert (len(in_guard), len(calls)) == {2: (34, 114), 3: (30, 114), 4: (27, 114), 8: (23, 112)}[n]


def test_placed_copies_registers_and_deregisters():
    call = rm.make_call(rm.spec(4, "all_reduce", "C+1", 2049, 3), 3, SEED, oring)
    m = rh.Mapping(rh.mapping_bytes(call.arena0.size))
    log = []

    def register(addr, nbytes):
        log.append(("reg", addr, nbytes))
        return 7

    for kind in ("pageable", "registered", "split"):
        del log[:]
        m.buf[:] = 0
        with m.placed(kind, call, register, lambda h: log.append(("dereg", h))) as (pl, base, view):
            assert base % 16 == 0 and base == m.base + pl.offset and view.ctypes.data == base
            assert np.array_equal(view, call.arena0) and not m.buf[:pl.offset].any()
            assert log == ([] if kind == "pageable" else [("reg", m.base, pl.registered)])
            if kind == "split":
                assert (base + pl.cut) % rh.PAGE == 0 and m.base + pl.registered == base + pl.cut
        assert log[1:] == ([] if kind == "pageable" else [("dereg", 7)])
    with pytest.raises(AssertionError):
        rh.place("pageable", m.size, m.size)


# ---- host memory, the oracle serving every step -------------------------------------------------------------------
def _run(comm, mapping, calls, kinds, context, zero_counts=False, direct=None):
    seen = {}
    for i, call in enumerate(calls):
        sp = call.spec
        seen[sp.collective] = seen.get(sp.collective, 0) + 1
        kind = kinds[i % len(kinds)]
        if zero_counts and seen[sp.collective] == 4:
            with mapping.placed(kind, call, lambda a, b: 1, lambda h: None) as (_pl, base, view):
                rm.issue(comm, call, base, count=0)
                rm.check(call, view, context + (kind, "count 0"), expected=call.arena0)
        with mapping.placed(kind, call, lambda a, b: 1, lambda h: None) as (_pl, base, view):
            rm.issue(comm, call, base)
            rm.check(call, view, context + (kind,))
        if direct:
            check_direct(comm, sp, context)


@pytest.mark.parametrize("channels", rm.CHANNELS)
@pytest.mark.parametrize("n", rm.RANKS)
def test_direct_table_on_host_memory(ring, oracle, fn, n, channels):
    """The SIMPLE table with set_direct(True), the oracle as fn: exact, and direct slices where the option
    applies. The arenas alternate between the pageable and the split placement."""
    calls = [rm.make_call(sp, n, SEED, oring, "simple", channels) for sp in rm.plan("simple", n, chunk_of)]
    mapping = rh.Mapping(rh.mapping_bytes(rh.largest_arena(calls)))
    with ring.RingComm(n, ring.HOST_MEMORY, rm.BUFF["simple"], fn, 20000, 0,
                       tree_ranks_per_node=rm.tree_per_node(n), n_channels=channels) as comm:
        comm.set_direct(True)
        _run(comm, mapping, calls, ("pageable", "split"), ("simple-direct", "host memory", n, channels), True, True)


def test_one_rank_plan_meets_every_pair_and_count():
    specs = one_rank_plan()
    assert len({s.k for s in specs}) == len(specs) == 6 * 2 * (8 * 4 + 3 * 3)   # u64, f64 and i64: p - 1 == 1
    for coll in rm.COLLECTIVES:
        mine = [s for s in specs if s.collective == coll]
        assert {(s.dt, s.op) for s in mine} == set(rm.PAIRS)
        for dt, op in rm.PAIRS:
            p = 16 // rm.esz_of(dt)
            for in_place in (False, True):
                got = {s.count for s in mine if (s.dt, s.op, s.in_place) == (dt, op, in_place)}
                assert got == {1, p - 1, p + 1, 4099}, (coll, ae.NAMES[dt], in_place)
    assert all(s.root == 0 and rm.PAIRS[s.k % len(rm.PAIRS)] == (s.dt, s.op) for s in specs)


def test_one_rank_on_host_memory(ring, oracle, fn):
    """A communicator of one rank (ncclLaunchOneRank): a float average is PreMulSum by 1 / 1, everything else a
    copy, an all-gather's and a broadcast's of any bit pattern."""
    calls = [rm.make_call(sp, 1, SEED, oring) for sp in one_rank_plan()]
    mapping = rh.Mapping(rh.mapping_bytes(rh.largest_arena(calls)))
    with ring.RingComm(1, ring.HOST_MEMORY, rm.BUFF["simple"], fn, 20000, 0, tree_ranks_per_node=1) as comm:
        _run(comm, mapping, calls, ("pageable", "split"), ("one rank", "host memory"))


def test_one_rank_expected_bytes_are_the_inputs():
    """rm.reduce_all of one buffer is that buffer, bit for bit, for every pair (a float's sum and average go
    through float64 and back, which gen_inputs' small integers survive)."""
    for sp in one_rank_plan():
        call = rm.Call(sp, 1, SEED)
        (out,) = call.outputs()
        assert np.asarray(out).tobytes() == call.inputs[0].tobytes(), sp.what()
        if sp.collective in rm.COPIES and sp.dt in ae.FLOATS and sp.count == 4099:
            assert ae.is_nan(sp.dt, call.inputs[0]).any(), sp.what()


# ---- the checker, on a placed arena --------------------------------------------------------------------------------
def _placed_expected(kind, coll, in_place):
    e = 4
    n, c = 4, chunk_of(coll, "simple", e)
    sp = rm.Spec(0, coll, "nC+n+1", n * c + n + 1, ae.U32, rm.SUM, in_place, 1)
    call = rm.make_call(sp, n, SEED)
    mapping = rh.Mapping(rh.mapping_bytes(call.arena0.size))
    return call, mapping, mapping.placed(kind, call, lambda a, b: 1, lambda h: None, content=call.expected)


def _rejects(call, got, *words):
    with pytest.raises(AssertionError) as err:
        rm.check(call, got, ("placed", call.n, 1))
    for w in ("placed", call.spec.collective) + words:
        assert w in str(err.value), (w, str(err.value))


@pytest.mark.parametrize("kind", ("pageable", "split"))
def test_the_checker_rejects_an_element_from_16_bytes_further_on(kind):
    """What a device address 16 bytes off for an interior pointer leaves: in every rank's output, at the first
    element, at the element on either side of split's cut and at the last element that has one 16 bytes on."""
    for coll in rm.COLLECTIVES:
        for in_place in (False, True):
            call, _m, cm = _placed_expected(kind, coll, in_place)
            with cm as (pl, _base, view):
                rm.check(call, view)
                hits = 0
                for rank in range(call.n):
                    if coll == "reduce" and rank != call.spec.root:
                        continue
                    off, last = call.recv_off[rank], call.recv_elems - 5
                    elems = {0, last}
                    if pl.cut is not None and off + 16 < pl.cut < off + 4 * last:
                        elems |= {(pl.cut - off) // 4 - 1, (pl.cut - off) // 4}
                    for el in sorted(elems):
                        out = view[off:off + 4 * call.recv_elems].view(np.uint32)
                        if out[el] == out[el + 4]:
                            continue
                        keep = out[el]
                        out[el] = out[el + 4]
                        _rejects(call, view, "rank %d" % rank, "first differing element %d" % el)
                        out[el] = keep
                        hits += 1
                assert hits >= 2, (coll, in_place)
                rm.check(call, view)


@pytest.mark.parametrize("kind", ("pageable", "split"))
def test_the_checker_rejects_a_written_guard_byte(kind):
    call, _m, cm = _placed_expected(kind, "reduce_scatter", False)
    with cm as (_pl, _base, view):
        for rank in range(call.n):
            for at, where in ((call.recv_off[rank] + 4 * call.recv_elems, "guard behind"),
                              (call.recv_off[rank] - 1, "guard before"), (call.send_off[rank] - 1, "guard before"),
                              (call.send_off[rank] + 4 * call.send_elems, "guard behind")):
                assert view[at] == rm.GUARD_BYTE
                view[at] ^= 1
                _rejects(call, view, "rank %d" % rank, where)
                view[at] ^= 1
        view[-1] ^= 0x80          # the arena's last byte
        _rejects(call, view, "guard behind")
        view[-1] ^= 0x80
        rm.check(call, view)
