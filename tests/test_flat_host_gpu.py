"""The flat collectives on a host-memory communicator, on the MI355X: nexrRingCommSetFlat (bits 7) routes the six
plain calls of a SIMPLE host-memory communicator with the library's own reduce-copy through the nexrFlatHost*
entries: one launch that reads and writes pinned user buffers in place over the link, pageable ones staged.

Every table case runs twice on the same communicator and the same arena, once with the option off (the
host-sequenced FIFO ring or tree) and once with it on, and the whole arena (outputs, guards, inputs, the outputs a
reduce must not touch) must be byte for byte what tests/ring_modes_cases.py expects (reduce_all where no fold order
can change the result, oracle.ring's restatement otherwise; tests/test_flat.py and test_flat_tree.py show that the
element-wise rules of flat_cases / flat_tree_cases are that restatement) and what the plain call left. The
order-sensitive inputs of flat_cases run against its element-wise model directly (test_types_and_ops).

The user buffers are of ring_host_cases.KINDS (pageable, registered, pinned by the runtime, split: registered up
to a page boundary inside one buffer) and `alloc` (inside one nexrHostMemAlloc allocation), and
nexrGetFlatHostStats is asserted for each: see expected_stats.

SIMPLE, rm.BUFF["simple"], timeoutMs = 20000. A flat launch has no credit, no poll and no residency requirement;
children get a time limit."""
import importlib
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import arith_edges as ae
import flat_cases as fc
import ring_host_cases as rh
import ring_modes_cases as rm
from oracle import ring as oring

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = rm.SEED
TIMEOUT_MS = 20000
KINDS = rh.KINDS + ("alloc",)
TABLE = [(n, ch, kind) for n in rm.RANKS for ch in rm.CHANNELS for kind in KINDS]   # the full product
ALL_BITS = 7


def chunk_of(coll, protocol, esz):
    return oring.chunk_count(coll, protocol, esz, rm.BUFF[protocol])


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    torch.cuda.init()
    return importlib.import_module("nex-nccl_amd.ring")


def nexr_mod():
    return importlib.import_module("nex-nccl_amd")


@lru_cache(maxsize=2)
def table_calls(n, channels):
    return [rm.make_call(sp, n, SEED, oring, "simple", channels) for sp in rm.plan("simple", n, chunk_of)]


_pinned, _alloc = {}, {}


def make_mapping(calls, kinds):
    """One mapping for the test; runtime-pinned memory (torch) or a nexrHostMemAlloc allocation of the same size
    beside it where `kinds` needs one (kept for the module)."""
    size = rh.mapping_bytes(rh.largest_arena(calls))
    maps = {}
    for kind in kinds:
        other = None
        if kind == "pinned":
            if size not in _pinned:
                _pinned[size] = torch.empty(size, dtype=torch.uint8).pin_memory()
            other = _pinned[size].numpy()
        elif kind == "alloc":
            if size not in _alloc:
                addr = nexr_mod().host_mem_alloc(size)
                _alloc[size] = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * size).from_address(addr))
            other = _alloc[size]
        maps[kind] = rh.Mapping(size, other)
    return maps


def placed(maps, kind, call, content=None):
    """ring_host_cases' placement; `alloc` is placed as `pinned` is, in the allocation."""
    nexr = nexr_mod()
    return maps[kind].placed("pinned" if kind == "alloc" else kind, call, nexr.host_register, nexr.host_deregister,
                             content)


def make_comm(ring, n, channels):
    return ring.RingComm(n, ring.HOST_MEMORY, rm.BUFF["simple"], None, TIMEOUT_MS, 0,
                         tree_ranks_per_node=rm.tree_per_node(n), n_channels=channels)


# ---- what a call hands to its nexrFlatHost* entry ---------------------------------------------------------------
def buffers_of(call):
    """(inputs, outputs, shared): the distinct (arena offset, bytes) the flat call reads and writes, and whether
    its pageable outputs share one staged output."""
    sp, n = call.spec, call.n
    ins = [(call.send_off[r], call.send_elems * call.esz) for r in range(n)]
    outs = [(call.recv_off[r], call.recv_elems * call.esz) for r in range(n)]
    if sp.collective == "reduce":
        outs = [outs[sp.root]]
    if sp.collective == "broadcast":
        ins = [ins[sp.root]]
        outs = [o for o in outs if o[0] != ins[0][0]]
    shared = sp.collective in ("all_reduce", "tree", "broadcast", "all_gather")
    return sorted(set(ins)), sorted(set(outs)), shared


def expected_stats(call, kind, pl):
    """nexrGetFlatHostStats after one routed call of n >= 2 ranks, by kind. Distinct buffers are distinct
    (address, bytes). registered / alloc: every buffer a cache hit, no query, nothing staged, zero-copy. pinned:
    a query per buffer, zero-copy. pageable: a query per buffer, a slot per distinct input and per distinct
    output, or ONE slot for all outputs where they share. split: a buffer wholly below the cut is a hit and read
    in place; the buffer the cut divides and every buffer above it are queried and staged."""
    ins, outs, shared = buffers_of(call)
    bufs = sorted(set(ins) | set(outs))
    if kind in ("registered", "alloc"):
        return dict(calls=1, zeroCopyCalls=1, stagedBuffers=0, registeredHits=len(bufs), pointerQueries=0, windows=1)
    if kind == "pinned":
        return dict(calls=1, zeroCopyCalls=1, stagedBuffers=0, registeredHits=0, pointerQueries=len(bufs), windows=1)

    def staged(b):
        return kind == "pageable" or b[0] + b[1] > pl.cut
    s_in = [b for b in ins if staged(b)]
    s_out = [b for b in outs if staged(b)]
    n_staged = len(s_in) + (min(1, len(s_out)) if shared else len(s_out))
    hits = len([b for b in bufs if not staged(b)])
    return dict(calls=1, zeroCopyCalls=1 if n_staged == 0 else 0, stagedBuffers=n_staged, registeredHits=hits,
                pointerQueries=len(bufs) - hits, windows=1)


def run_both(comm, maps, call, kind, context, content=None, expected=None, stats=True):
    """The call with the option off, then on, on the same arena in the same place; both arenas against the
    expected bytes, and the flat call's counters."""
    nexr = nexr_mod()
    what = (context, kind, call.spec.what())
    with placed(maps, kind, call, content) as (pl, base, view):
        comm.set_flat(False)
        before = comm.queued()
        rm.issue(comm, call, base)
        # a plain host-sequenced ring call reports 0; a plain SIMPLE tree call does not report, so queued() is
        # exactly what it was before it
        assert comm.queued() == (before if call.spec.collective == "tree" else 0), (what, before, comm.queued())
        plain = view.copy()
        view[:] = call.arena0 if content is None else content
        comm.set_flat(True, tree=True, copies=True)
        nexr.flat_host_stats(reset=True)
        rm.issue(comm, call, base)
        st = nexr.flat_host_stats()
        assert comm.queued() == 4, what
        got = view.copy()
    if expected is None:
        rm.check(call, got, context + (kind, "flat"))
        rm.check(call, plain, context + (kind, "plain"))
    else:
        rm.check(call, fc.canon_outputs(call, got), context + (kind, "flat"), expected=fc.canon_outputs(call, expected))
        plain, got = fc.canon_outputs(call, plain), fc.canon_outputs(call, got)
    assert np.array_equal(got, plain), what
    if stats:
        assert st == expected_stats(call, kind, pl), (what, st, expected_stats(call, kind, pl))
    return st


def run_empty(comm, maps, call, kind, context):
    nexr = nexr_mod()
    with placed(maps, kind, call) as (_pl, base, view):
        comm.set_flat(True, tree=True, copies=True)
        nexr.flat_host_stats(reset=True)
        rm.issue(comm, call, base, 0)
        assert nexr.flat_host_stats()["calls"] == 0
        rm.check(call, view.copy(), context + (kind, "count 0"), expected=call.arena0)


# ---- the count table ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,channels,kind", TABLE, ids=["%d-%d-%s" % t for t in TABLE])
def test_table(ring, oracle, n, channels, kind):
    calls = table_calls(n, channels)
    maps = make_mapping(calls, (kind,))
    seen, staged_calls, cut_in, cut_out = {}, 0, 0, 0
    with make_comm(ring, n, channels) as comm:
        for call in calls:
            sp = call.spec
            seen[sp.collective] = seen.get(sp.collective, 0) + 1
            if seen[sp.collective] == 4:
                run_empty(comm, maps, call, kind, ("table", n, channels))
            st = run_both(comm, maps, call, kind, ("table", n, channels))
            staged_calls += st["zeroCopyCalls"] == 0
            if kind == "split":
                pl = rh.place("split", call.arena0.size, maps[kind].size, call.regions)
                reg = rh.cut_region(call, pl)
                if reg is not None:
                    ins, outs, _ = buffers_of(call)
                    cut_in += (reg[2], reg[3]) in ins
                    cut_out += (reg[2], reg[3]) in outs
    assert all(seen[c] >= 11 for c in rm.COLLECTIVES), seen
    if kind == "split":   # a cut input and a cut output were both among the staged buffers, and nothing faulted
        assert cut_in > 0 and cut_out > 0 and staged_calls > 0, (cut_in, cut_out, staged_calls)


# ---- every datatype x op, order-sensitive inputs, against the element-wise model ------------------------------------
def step_of(oracle, dt, op, n):
    dev_op, arg = oracle.host_to_dev_red_op(op, dt, n)

    def step(x, v, post):
        return oracle.reduce_copy([x] if v is None else [x, v], 1, dt, dev_op, arg, [arg], post)[0]
    return step


def pairs_56():
    out = [(dt, op) for dt in ae.FLOATS + ae.INTS for op in (rm.SUM, rm.PROD, rm.MAX, rm.MIN, rm.AVG)]
    return out


def model_call(oracle, sp, n, channels=1):
    call = fc.Call(sp, n, SEED)
    parts = None
    if sp.collective == "all_reduce":
        chunk = chunk_of("all_reduce", "simple", call.esz)
        parts = [(off, cnt, chunk) for _ch, off, cnt in oring.channel_parts(channels, sp.count, call.esz, 2, ll=False)]
    outs = fc.model(sp.collective, call.inputs, sp.count, sp.root, step_of(oracle, sp.dt, sp.op, n), parts)
    return call.set_outputs(outs)


@pytest.mark.parametrize("kind", ["registered", "pageable"])
def test_types_and_ops(ring, oracle, kind):
    """All datatype x op pairs the ring takes at 3 ranks, at n C + n + 1 elements (a sub-pack tail for every
    element size, chunks started by every rank), on inputs whose result depends on the fold order; each pair on
    one of the three ring collectives in turn, in and out of place."""
    n = 3
    pairs = pairs_56()
    assert len(pairs) >= 50
    calls = []
    for k, (dt, op) in enumerate(pairs):
        coll = fc.COLLECTIVES[k % 3]
        count = n * chunk_of(coll, "simple", rm.esz_of(dt)) + n + 1
        calls.append(model_call(oracle, rm.Spec(k, coll, "nC+n+1", count, dt, op, k % 2 == 1, k % n), n))
    maps = make_mapping(calls, (kind,))
    with make_comm(ring, n, 1) as comm:
        for call in calls:
            run_both(comm, maps, call, kind, ("types", n), expected=call.expected)


@pytest.mark.parametrize("kind", ["registered", "pageable"])
def test_integer_pre_mul_sum(ring, oracle, kind):
    """The six pairs no ncclRedOp_t reaches (an integer PreMulSum; with test_types_and_ops' fifty, all 56 accepted
    datatype x device-op pairs): nexrFlatHostAllReduce called directly at 3 ranks, against the element-wise model
    with the oracle's reduce-copy as the step."""
    nexr = nexr_mod()
    n, arg = 3, 3
    for k, dt in enumerate(ae.INTS):
        e = rm.esz_of(dt)
        chunk = chunk_of("all_reduce", "simple", e)
        count = n * chunk + n + 1
        call = fc.Call(rm.Spec(k, "all_reduce", "nC+n+1", count, dt, rm.SUM, k % 2 == 1, 0), n, SEED)

        def step(x, v, post, dt=dt):
            return oracle.reduce_copy([x] if v is None else [x, v], 1, dt, nexr.DevRedOp.PreMulSum, arg, [arg], post)[0]
        parts = [(0, count, chunk)]
        call.set_outputs(fc.model("all_reduce", call.inputs, count, 0, step, parts))
        maps = make_mapping([call], (kind,))
        with placed(maps, kind, call) as (_pl, base, view):
            nexr.flat_host_all_reduce([base + o for o in call.send_off], [base + o for o in call.recv_off], count, dt,
                                      nexr.DevRedOp.PreMulSum, arg, True, parts)
            got = view.copy()
        rm.check(call, got, ("int PreMulSum", kind))


def test_odd_offsets_int8_fp16(ring, oracle):
    """User buffers at element-aligned odd offsets: the arena moved by one element inside the mapping (int8: an
    odd address; fp16: 2 mod 4), pinned in place and staged."""
    n = 3
    nexr = nexr_mod()
    for k, (dt, op, coll) in enumerate(((ae.I8, rm.SUM, "all_reduce"), (ae.F16, rm.SUM, "reduce_scatter"),
                                        (ae.I8, rm.MAX, "reduce"), (ae.F16, rm.PROD, "all_reduce"))):
        e = rm.esz_of(dt)
        count = n * chunk_of(coll, "simple", e) + n + 1
        call = model_call(oracle, rm.Spec(k, coll, "nC+n+1", count, dt, op, k % 2 == 1, k % n), n)
        size = rh.mapping_bytes(call.arena0.size)
        mp = rh.Mapping(size)
        with make_comm(ring, n, 1) as comm:
            for register in (True, False):
                off = rh.PAGE + 48 + e
                view = mp.buf[off:off + call.arena0.size]
                handle = nexr.host_register(mp.base, size) if register else None
                try:
                    got = []
                    for bits in (0, ALL_BITS):
                        view[:] = call.arena0
                        comm.set_flat(bool(bits & 1), tree=bool(bits & 2), copies=bool(bits & 4))
                        rm.issue(comm, call, mp.base + off)
                        got.append(fc.canon_outputs(call, view.copy()))
                finally:
                    if handle is not None:
                        nexr.host_deregister(handle)
                rm.check(call, got[1], ("odd offset", register), expected=fc.canon_outputs(call, call.expected))
                assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("sem", ["Fork", "Shipped"])
def test_semantics(ring, oracle, sem):
    """One case each under nexrSemanticsFork (signed min on the unsigned kernel) and nexrSemanticsShipped (every
    reduce returns its first operand): the flat call leaves what the plain call of the same communicator leaves."""
    nexr = nexr_mod()
    n = 3
    calls = [rm.Call(rm.Spec(k, coll, "nC+n+1", n * chunk_of(coll, "simple", 1) + n + 1, ae.I8, rm.MIN, False, 1), n,
                     SEED) for k, coll in enumerate(("all_reduce", "tree", "reduce_scatter", "reduce"))]
    maps = make_mapping(calls, ("registered", "pageable"))
    nexr.set_semantics(getattr(nexr.Semantics, sem))
    try:
        with make_comm(ring, n, 1) as comm:
            for call in calls:
                for kind in ("registered", "pageable"):
                    with placed(maps, kind, call) as (_pl, base, view):
                        got = []
                        for on in (False, True):
                            view[:] = call.arena0
                            comm.set_flat(on, tree=on, copies=on)
                            rm.issue(comm, call, base)
                            got.append(view.copy())
                        assert comm.queued() == 4
                    assert np.array_equal(got[0], got[1]), (sem, kind, call.spec.what())
                    assert not np.array_equal(got[1], call.arena0)
    finally:
        nexr.set_semantics(nexr.Semantics.Nccl)


# ---- mixed kinds in one call -----------------------------------------------------------------------------------------
def test_mixed_kinds_in_one_call(ring, oracle):
    """Two ranks, rank 0's buffers registered and rank 1's pageable: the mapping is registered up to the page
    boundary before rank 1's first buffer. Out of place and in place, all six collectives; the in-place
    reduce-scatter's output is chunk r of its input."""
    nexr = nexr_mod()
    n = 2
    specs = [rm.Spec(k, coll, "C+1", chunk_of(coll, "simple", 4) + 1, ae.F32, rm.SUM, k % 2 == 1, k % n)
             for k, coll in enumerate(rm.COLLECTIVES + rm.COLLECTIVES[1:] + rm.COLLECTIVES[:1])]
    assert {(s.collective, s.in_place) for s in specs} == {(c, p) for c in rm.COLLECTIVES for p in (False, True)}
    with make_comm(ring, n, 1) as comm:
        for sp in specs:
            call = rm.make_call(sp, n, SEED, oring, "simple", 1)
            first1 = min(off for rank, _kind, off, _b in call.regions if rank == 1)
            last0 = max(off + b for rank, _kind, off, b in call.regions if rank == 0)
            assert last0 <= first1 - rm.GUARD // 2
            size = rh.mapping_bytes(call.arena0.size) + rh.PAGE
            mp = rh.Mapping(size)
            boundary = rh.page_ceil(first1) + rh.PAGE           # a page boundary of the mapping ...
            off = boundary - (first1 - 16)                      # ... 16 bytes before rank 1's first buffer
            view = mp.buf[off:off + call.arena0.size]
            handle = nexr.host_register(mp.base, boundary)
            try:
                got = []
                for on in (False, True):
                    view[:] = call.arena0
                    comm.set_flat(on, tree=on, copies=on)
                    nexr.flat_host_stats(reset=True)
                    rm.issue(comm, call, mp.base + off)
                    got.append(view.copy())
                st = nexr.flat_host_stats()
            finally:
                nexr.host_deregister(handle)
            rm.check(call, got[1], ("mixed", sp.what()))
            assert np.array_equal(got[0], got[1])
            ins, outs, shared = buffers_of(call)
            below = [b for b in sorted(set(ins) | set(outs)) if b[0] + b[1] <= first1 - 16]
            assert st["calls"] == 1 and st["registeredHits"] == len(below), (sp.what(), st)
            assert st["zeroCopyCalls"] == 0 and st["stagedBuffers"] > 0, (sp.what(), st)


# ---- alternation -----------------------------------------------------------------------------------------------------
def test_alternation(ring, oracle):
    """Twenty-four calls on one communicator of 2 channels (rm.mixed_plan: tiny, chunk edge and several-loop
    counts, all six collectives) while set_flat toggles its bits: a call is routed exactly when its bit is on,
    queued() is 4 after it and 0 after a plain ring call (a plain SIMPLE tree call keeps the previous call's
    report, asserted exactly), and every arena is as expected whichever way it ran."""
    nexr = nexr_mod()
    n = 4
    calls = [rm.make_call(sp, n, SEED, oring, "simple", 2) for sp in rm.mixed_plan("simple", n, chunk_of, SEED + n)]
    assert len(calls) == 24
    kinds = ("pageable", "registered", "pinned", "alloc")
    maps = make_mapping(calls, kinds)
    bit_of = {"all_reduce": 1, "reduce_scatter": 1, "reduce": 1, "tree": 2, "all_gather": 4, "broadcast": 4}
    routed = stale = 0
    with make_comm(ring, n, 2) as comm:
        seq = [(call, (0, 1, 2, 4, 7, 3, 5, 6)[k % 8]) for k, call in enumerate(calls)]
        # and a plain tree call right behind a routed ring call: its report is the routed call's 4, not its own
        tree = next(c for c in calls if c.spec.collective == "tree")
        seq += [(next(c for c in calls if c.spec.collective == "reduce"), 1), (tree, 0), (calls[0], 0), (tree, 5)]
        for k, (call, bits) in enumerate(seq):
            kind = kinds[k % len(kinds)]
            comm.set_flat(bool(bits & 1), tree=bool(bits & 2), copies=bool(bits & 4))
            before = comm.queued()
            with placed(maps, kind, call) as (_pl, base, view):
                nexr.flat_host_stats(reset=True)
                rm.issue(comm, call, base)
                st = nexr.flat_host_stats()
                got = view.copy()
            rm.check(call, got, ("alternation", k, bits, kind))
            flat = bool(bits & bit_of[call.spec.collective])
            assert st["calls"] == (1 if flat else 0), (k, bits, call.spec.what(), st)
            # 4 after a routed call, 0 after a plain ring call; a plain SIMPLE tree call does not report, so the
            # report is exactly the previous call's
            want = 4 if flat else before if call.spec.collective == "tree" else 0
            assert comm.queued() == want, (k, bits, call.spec.what(), before, comm.queued())
            stale += (not flat) and want == 4
            routed += flat
    assert 4 <= routed <= 20 and stale == 1   # the plain tree call behind a routed call


# ---- process ranks -------------------------------------------------------------------------------------------------
def test_process_ranks_are_refused(ring, nexr):
    """A peer (process-rank) communicator: nexrRingCommSetFlat and all six flat entries answer nexrInvalidUsage,
    whatever the bits, and no nexrFlatHost* call is made."""
    import ctypes
    RL = ring.ring_lib()
    usage = nexr.Result.InvalidUsage
    F32 = nexr.DataType.Float32
    buf = np.zeros(64, np.float32)
    arr = (ctypes.c_void_p * 1)(buf.ctypes.data)
    name = "/nexr_flat_host_%d" % os.getpid()
    with ring.PeerRingComm(1, 0, name, device=0, buff_bytes=rm.BUFF["simple"], timeout_ms=TIMEOUT_MS) as comm:
        nexr.flat_host_stats(reset=True)
        for bits in (0, 1, 2, 4, 7):
            assert RL.nexrRingCommSetFlat(comm._h, bits) == usage, bits
        assert RL.nexrRingAllReduceFlat(comm._h, arr, arr, 4, int(F32), 0) == usage
        assert RL.nexrRingReduceScatterFlat(comm._h, arr, arr, 4, int(F32), 0) == usage
        assert RL.nexrRingReduceFlat(comm._h, arr, arr, 4, int(F32), 0, 0) == usage
        assert RL.nexrTreeAllReduceFlat(comm._h, arr, arr, 4, int(F32), 0) == usage
        assert RL.nexrRingBroadcastFlat(comm._h, arr, arr, 4, int(F32), 0) == usage
        assert RL.nexrRingAllGatherFlat(comm._h, arr, arr, 4, int(F32)) == usage
        assert nexr.flat_host_stats()["calls"] == 0
    assert not buf.any()


# ---- one rank ------------------------------------------------------------------------------------------------------
def test_one_rank(ring, oracle):
    nexr = nexr_mod()
    calls = [rm.make_call(sp, 1, SEED, oring) for sp in rh.one_rank_plan()]
    mp = rh.Mapping(rh.mapping_bytes(rh.largest_arena(calls)))
    with ring.RingComm(1, ring.HOST_MEMORY, rm.BUFF["simple"], None, TIMEOUT_MS, 0, tree_ranks_per_node=1) as comm:
        comm.set_flat(True, tree=True, copies=True)
        for call in calls:
            for kind in ("pageable", "registered"):
                with mp.placed(kind, call, nexr.host_register, nexr.host_deregister) as (_pl, base, view):
                    nexr.flat_host_stats(reset=True)
                    rm.issue(comm, call, base)
                    assert nexr.flat_host_stats()["calls"] == 0     # ncclLaunchOneRank's path, as before
                    rm.check(call, view.copy(), ("one rank", kind))


# ---- children: the window pipeline, NEXR_HOST_ZERO_COPY=0 ------------------------------------------------------------
WINDOW_CHUNK = 4096   # two pieces
CHILD_TIMEOUT_S = 60

_WORKER = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import oracle
import test_flat_host_gpu as t
oracle.lib()
torch.cuda.init()
t.{fn}()
torch.cuda.synchronize()
print("FLAT-HOST-CHILD-OK")
"""


def window_specs(n):
    """fp32 at 1023, 1024, 1025, 2049 and 3 * 1024 + 3 elements (1, 1, 2, 2 plus a tail window of 4 bytes, and 3
    plus a tail window of 12 bytes), bf16 at an odd count (4097: 2 windows plus a tail of 2 bytes); the ring
    all-reduce, the tree, the reduce and the broadcast; in and out of place."""
    out = []
    for coll in ("all_reduce", "tree", "reduce", "broadcast"):
        for dt, count in ((ae.F32, 1023), (ae.F32, 1024), (ae.F32, 1025), (ae.F32, 2049), (ae.F32, 3 * 1024 + 3),
                          (ae.BF16, 4097)):
            k = len(out)
            out.append(rm.Spec(k, coll, "window", count, dt, rm.SUM, k % 2 == 1, k % n))
    return out


def window_worker():
    """Runs with NEXR_FLAT_HOST_CHUNK_BYTES=4096 (fp32: a window is 1024 elements). 3 ranks, 2 channels: these
    counts are one short loop per channel part, whose chunks are alignUp(divUp(part, 3), 16 / esz) elements. At
    3 * 1024 + 3 elements channel 0's part of 2048 elements has chunks of 684 (boundaries at bytes 2736 and 5472:
    inside windows 0 and 1), and channel 1's part, with its own first chunk and its own tree, begins at byte
    8192, the edge of window 2; at 2049 the second part is the one-element tail window."""
    assert oring.channel_parts(2, 3 * 1024 + 3, 4, 2, ll=False) == [(0, 0, 2048), (1, 2048, 1027)]
    ring = importlib.import_module("nex-nccl_amd.ring")
    nexr = nexr_mod()
    n = 3
    calls = [rm.make_call(sp, n, SEED, oring, "simple", 2) for sp in window_specs(n)]
    maps = make_mapping(calls, ("pageable", "split", "registered"))
    with make_comm(ring, n, 2) as comm:
        for call in calls:
            region = call.spec.count * call.esz
            want = -(-region // WINDOW_CHUNK)
            for kind in ("pageable", "split", "registered"):
                st = run_both(comm, maps, call, kind, ("windows", n), stats=False)
                if kind == "registered":
                    assert st["windows"] == 1 and st["zeroCopyCalls"] == 1, (call.spec.what(), st)
                elif st["zeroCopyCalls"] == 0:
                    assert st["windows"] == want, (kind, call.spec.what(), st, want)
                if kind == "pageable":
                    assert st["zeroCopyCalls"] == 0
    seen = {-(-sp.count * rm.esz_of(sp.dt) // WINDOW_CHUNK) for sp in window_specs(n)}
    assert {1, 2, 3, 4} <= seen, seen


def zero_copy_off_worker():
    """Runs with NEXR_HOST_ZERO_COPY=0: registered and allocated buffers are staged like pageable ones, without
    a lookup or a query."""
    ring = importlib.import_module("nex-nccl_amd.ring")
    n = 3
    calls = table_calls(n, 1)[::5]
    maps = make_mapping(calls, ("registered", "alloc", "split"))
    with make_comm(ring, n, 1) as comm:
        for call in calls:
            for kind in ("registered", "alloc", "split"):
                st = run_both(comm, maps, call, kind, ("zero copy off", n), stats=False)
                assert st["zeroCopyCalls"] == 0 and st["registeredHits"] == 0 and st["pointerQueries"] == 0, st
                assert st["stagedBuffers"] > 0, st


@pytest.mark.parametrize("fn,env", [("window_worker", {"NEXR_FLAT_HOST_CHUNK_BYTES": str(WINDOW_CHUNK)}),
                                    ("zero_copy_off_worker", {"NEXR_HOST_ZERO_COPY": "0"})],
                         ids=["window-pipeline", "zero-copy-off"])
def test_children(fn, env):
    from conftest import GOLDEN, ROOT
    code = _WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=GOLDEN, fn=fn)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=CHILD_TIMEOUT_S)
    assert out.returncode == 0 and "FLAT-HOST-CHILD-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
