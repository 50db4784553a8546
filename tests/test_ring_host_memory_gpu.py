"""The ring and tree collectives on a host-memory communicator with the library's own reduce-copy underneath, on
the MI355X: every step of every rank thread is one nexrReduceCopyHost call on FIFO slots (from nexrHostMemAlloc)
and interior slices of user buffers in host memory. tests/test_ring_modes_gpu.py runs the same table on device
memory, and tests/test_ring_modes.py on host memory with the oracle as `fn`; the host paths themselves are tested a
call at a time (test_host_paths_gpu.py, test_host_register_gpu.py, test_host_zero_copy_ops_gpu.py). Here they meet:
tests/ring_modes_cases.py's count table (1 element to 2 n C + 3 and 0, all ten datatypes and five ops, in and out
of place, every root, 2 to 8 ranks, 1 and 2 channels), with and without set_direct, on user buffers that are

  pageable    every step staged through the calling thread's pinned slots;
  registered  inside one nexrHostRegister-ed mapping: every step zero-copy, classified from the cache;
  pinned      pinned by the runtime, unknown to the library (torch pin_memory): zero-copy after the pointer query
              and its range check;
  split       registered up to a page boundary inside one rank's user buffer: zero-copy and staged steps in one
              collective, and slices that straddle the registration's end

(tests/ring_host_cases.py places them), then the four kinds in turn on one mapping with direct toggled, the forced
host paths (pageable FIFOs, the chunk pipeline, the copy team with small chunks) in child processes, C1's
host_registered leg as bench.py runs it, and a communicator of one rank.

SIMPLE, rm.BUFF["simple"] (4 KiB steps), the library's own fn, timeoutMs = 20000: a stuck protocol ends with an
error. Every call's arena is compared whole with the expected bytes (rm.check): outputs, guards, inputs, and the
outputs a reduce must not touch; all comparisons are exact.

Where the issue of round 13 put split's cut, at the middle of the arena, no buffer would be divided (the middle is
in a guard for every even number of ranks); tests/ring_host_cases.py puts it at the middle of the buffer there.

Durations on an MI355X (profiles/r13a_ring_host_memory_gpu_tests.txt): the slowest table 0.36 s (8 ranks,
pageable), every other test under 0.25 s but the three children of test_forced_host_paths (2.5 to 4.2 s); all 59
in under 20 s. No cell of the table was dropped."""
import importlib
import os
import subprocess
import sys
from functools import lru_cache

import numpy as np
import pytest

import arith_edges as ae
import ring_host_cases as rh
import ring_modes_cases as rm
from oracle import ring as oring
from ring_host_cases import check_direct, one_rank_plan

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = rm.SEED


def chunk_of(coll, protocol, esz):
    return oring.chunk_count(coll, protocol, esz, rm.BUFF[protocol])


TIMEOUT_MS = 20000
FEW = ((2, 1), (3, 1), (4, 2), (8, 1))
# (n, channels, kind, direct): pageable and registered in every cell, pinned and split in FEW; ordered by cell,
# so that the calls of a cell are made once (table_calls)
TABLE = [(n, ch, kind, direct) for n in rm.RANKS for ch in rm.CHANNELS for kind in rh.KINDS for direct in (False, True)
         if kind in ("pageable", "registered") or (n, ch) in FEW]


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


@lru_cache(maxsize=4)
def mixed_calls(n):
    return [rm.make_call(sp, n, SEED, oring, "simple", 2) for sp in rm.mixed_plan("simple", n, chunk_of, SEED + n)]


_pinned = {}


def make_mapping(calls, kinds):
    """The test's one mapping, with runtime-pinned memory of the same size beside it when `kinds` needs it (kept
    for the module: the pinned allocator keeps it anyway)."""
    size = rh.mapping_bytes(rh.largest_arena(calls))
    pinned = None
    if "pinned" in kinds:
        if size not in _pinned:
            _pinned[size] = torch.empty(size, dtype=torch.uint8).pin_memory()
        pinned = _pinned[size].numpy()
    return rh.Mapping(size, pinned)


def make_comm(ring, n, channels):
    return ring.RingComm(n, ring.HOST_MEMORY, rm.BUFF["simple"], None, TIMEOUT_MS, 0,
                         tree_ranks_per_node=rm.tree_per_node(n), n_channels=channels)


def check_how_it_ran(kind, st, what, fifos_pinned=True):
    """nexrReduceCopyHost counts a call after its nElts == 0 return, so zero-element slices are not counted
    (genericOp does not even call fn for them), and classifies every buffer of a counted call: from the
    registration cache (registeredHits) or, failing that, by hipPointerGetAttributes and the range check
    (pointerQueries); zeroCopyCalls counts the calls all of whose buffers were pinned. The FIFOs come from
    nexrHostMemAlloc and are in the cache. Every step of the ring schedules and of the tree has a user buffer on
    one side at least (send, recvReduceSend, recvReduceCopy[Send], recvCopySend, recv; with set_direct a peer's
    user buffer takes the FIFO slot's place), so with pageable user buffers no counted call is zero-copy and each
    one queries; with the mapping registered every buffer of every call is a cache hit; with runtime-pinned user
    buffers every call is zero-copy after a query per user buffer. With pageable FIFOs (NEXR_RING_HOST_PINNED=0)
    only the pageable kind's expectation still holds."""
    calls, zc, q = st["calls"], st["zeroCopyCalls"], st["pointerQueries"]
    assert calls > 0, (what, st)
    if kind == "pageable":
        assert zc == 0 and q > 0, (what, st)
    elif not fifos_pinned:
        return
    elif kind == "registered":
        assert zc == calls and q == 0 and st["registeredHits"] > 0, (what, st)
    elif kind == "pinned":
        assert zc == calls and q > 0, (what, st)


def run_call(comm, mapping, call, kind, context, count=None, fifos_pinned=True):
    """The call on its arena placed as `kind` says, the whole arena read back from where it ran against the
    expected bytes (count = 0: against what it held before, and no nexrReduceCopyHost call at all). Returns the
    host-path counters of the call."""
    nexr = nexr_mod()
    what = (context, kind, call.spec.what())
    with mapping.placed(kind, call, nexr.host_register, nexr.host_deregister) as (_pl, base, view):
        nexr.host_path_stats(reset=True)
        rm.issue(comm, call, base, count)
        st = nexr.host_path_stats()
        got = view.copy()
    rm.check(call, got, context + (kind,), expected=call.arena0 if count == 0 else None)
    if count == 0:
        assert st["calls"] == 0, (what, st)
    else:
        check_how_it_ran(kind, st, what, fifos_pinned)
    return st


def run_table(comm, mapping, calls, kind, direct, context, fifos_pinned=True):
    """Every call of the table on `comm`, and count = 0 once per collective, between two calls of it. split: over
    the table some steps ran in place and some were staged."""
    comm.set_direct(direct)
    seen, total, zero_copy = {}, 0, 0
    for call in calls:
        sp = call.spec
        seen[sp.collective] = seen.get(sp.collective, 0) + 1
        if seen[sp.collective] == 4:
            run_call(comm, mapping, call, kind, context + ("count 0",), count=0)
        st = run_call(comm, mapping, call, kind, context, fifos_pinned=fifos_pinned)
        total += st["calls"]
        zero_copy += st["zeroCopyCalls"]
        if direct:
            check_direct(comm, sp, context)
    assert all(seen[c] >= 11 for c in rm.COLLECTIVES), seen
    if kind == "split" and fifos_pinned:
        assert 0 < zero_copy < total, (context, zero_copy, total)


def run_mixed(comm, mapping, calls, kinds, context, fifos_pinned=True):
    """Call k on kind k mod len(kinds), direct on when (k // 3) is odd, all on one mapping: registered before the
    call, deregistered after it."""
    for call in calls:
        k = call.spec.k
        direct = (k // 3) % 2 == 1
        comm.set_direct(direct)
        run_call(comm, mapping, call, kinds[k % len(kinds)], context + ("direct" if direct else "",),
                 fifos_pinned=fifos_pinned)
        if direct:
            check_direct(comm, call.spec, context)


@pytest.mark.parametrize("n,channels,kind,direct", TABLE,
                         ids=["%d-%d-%s%s" % (n, ch, kind, "-direct" if d else "") for n, ch, kind, d in TABLE])
def test_table(ring, oracle, n, channels, kind, direct):
    calls = table_calls(n, channels)
    mapping = make_mapping(calls, (kind,))
    with make_comm(ring, n, channels) as comm:
        run_table(comm, mapping, calls, kind, direct, ("host memory", "direct" if direct else "", n, channels))


@pytest.mark.parametrize("n", rm.RANKS)
def test_mixed_kinds_and_toggles(ring, oracle, n):
    """rm.mixed_plan's 24 calls (tiny, chunk edge, several loops over both channels) on one communicator of 2
    channels and one mapping: pageable, registered, pinned, split and again, so a pageable call runs on addresses
    that were registered one call earlier and a split call registers a prefix of a range that was registered
    whole (the pinned calls run in the runtime's memory beside it); direct changes every three calls. A stale
    cache entry, a leaked staging slot or a drifting step counter is a wrong byte, and a stale entry also a
    zero-copy step in a pageable call."""
    calls = mixed_calls(n)
    mapping = make_mapping(calls, rh.KINDS)
    with make_comm(ring, n, 2) as comm:
        run_mixed(comm, mapping, calls, rh.KINDS, ("mixed", n, 2))


# One child per knob set (the knobs are read once per process); each runs, at (3, 1) and (4, 2), the table on
# either of its two kinds without and with direct, and the mixed plan alternating between them.
FORCED = [
    # pageable FIFOs: the registered kind gives steps whose pinned side is the user buffer, staged side the FIFO
    ({"NEXR_RING_HOST_PINNED": "0"}, ("pageable", "registered")),
    # every staged step through the chunk pipeline, two chunks per 8 KiB slice
    ({"NEXR_HOST_COPY_THREADS": "0", "NEXR_HOST_CHUNK_BYTES": "4096"}, ("pageable", "split")),
    # the copy team with small chunks through its three slots
    ({"NEXR_HOST_COPY_THREADS": "3", "NEXR_HOST_MT_MIN_BYTES": "0", "NEXR_HOST_MT_CHUNK_BYTES": "4096"},
     ("pageable", "split")),
]
# In process the same eight tables and two mixed plans take 0.55 s with the default knobs (test_table[3-1-*] 0.04 s
# and [4-2-*] 0.08 s each, test_mixed_kinds_and_toggles[3] and [4] 0.03 s and 0.05 s). A child took 2.5 to 4.2 s over
# four runs, most of it importing torch and opening the GPU, which ten times the tables' own time (6 s) would not
# cover on a busy machine: the limit is ten times the slowest child.
CHILD_TIMEOUT_S = 40

_WORKER = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import oracle
import test_ring_host_memory_gpu as t
oracle.lib()
torch.cuda.init()
t.forced_worker({kinds!r}, {fifos_pinned!r}, {env!r})
torch.cuda.synchronize()
print("HOST-TABLES-OK")
"""


def forced_worker(kinds, fifos_pinned, env):
    ring = importlib.import_module("nex-nccl_amd.ring")
    for n, channels in ((3, 1), (4, 2)):
        calls = table_calls(n, channels)
        mapping = make_mapping(calls, kinds)
        with make_comm(ring, n, channels) as comm:
            for kind in kinds:
                for direct in (False, True):
                    run_table(comm, mapping, calls, kind, direct, (str(env), "direct" if direct else "", n, channels),
                              fifos_pinned)
        calls = mixed_calls(n)
        mapping = make_mapping(calls, kinds)
        with make_comm(ring, n, 2) as comm:
            run_mixed(comm, mapping, calls, kinds, (str(env), "mixed", n, 2), fifos_pinned)


@pytest.mark.parametrize("env,kinds", FORCED, ids=["pageable-fifos", "chunk-pipeline", "copy-team"])
def test_forced_host_paths(env, kinds):
    from conftest import GOLDEN, ROOT
    code = _WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=GOLDEN, kinds=kinds, env=env,
                          fifos_pinned="NEXR_RING_HOST_PINNED" not in env)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=CHILD_TIMEOUT_S)
    assert out.returncode == 0 and "HOST-TABLES-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


def test_c1_host_registered_as_the_bench_runs_it(ring, nexr):
    """bench.py's host_registered leg of C1: 2 ranks, fp32 sum, 1 << 20 elements, the default FIFOs, four
    buffers each registered on its own, neighbours sharing a page (64 bytes apart in one mapping, none
    page-aligned). Every step zero-copy from the cache; after deregistration the same call stages every step.
    Small integers: a + b is exact in fp32 whatever the order."""
    count = 1 << 20
    gap = 4 * count + 64
    mapping = rh.Mapping(rh.page_ceil(4 * gap) + 2 * rh.PAGE)
    offs = [rh.PAGE + 48 + i * gap for i in range(4)]
    assert all((offs[i] + 4 * count) // rh.PAGE == offs[i + 1] // rh.PAGE for i in range(3))
    bufs = [mapping.buf[o:o + 4 * count].view(np.float32) for o in offs]
    rng = np.random.default_rng(1)
    a, b = (rng.integers(-1000, 1000, count).astype(np.float32) for _ in range(2))
    expect = (a + b).astype(np.float32)
    ptrs = [v.ctypes.data for v in bufs]

    def run(comm):
        bufs[0][:], bufs[1][:] = a, b
        bufs[2][:] = bufs[3][:] = np.nan
        before = mapping.buf.copy()
        nexr.host_path_stats(reset=True)
        comm.all_reduce(ptrs[:2], ptrs[2:], count, 7, 0)
        st = nexr.host_path_stats()
        for out in bufs[2:]:
            assert np.array_equal(out.view(np.uint32), expect.view(np.uint32))
        for o in offs[2:]:   # nothing else in the mapping changed: the inputs, the gaps, the pages round them
            before[o:o + 4 * count] = expect.view(np.uint8)
        assert np.array_equal(mapping.buf, before)
        return st

    with ring.RingComm(2, ring.HOST_MEMORY, 0, None, protocol=ring.PROTO_SIMPLE, timeout_ms=TIMEOUT_MS) as comm:
        handles = [nexr.host_register(p, 4 * count) for p in ptrs]
        try:
            assert len(set(handles)) == 4
            st = run(comm)
            assert st["calls"] > 0 and st["zeroCopyCalls"] == st["calls"] and st["pointerQueries"] == 0, st
        finally:
            for h in handles:
                nexr.host_deregister(h)
        st = run(comm)
        assert st["calls"] > 0 and st["zeroCopyCalls"] == 0, st


@pytest.mark.parametrize("memory", ["host-pageable", "host-registered", "device"])
def test_one_rank(ring, oracle, nexr, memory):
    """A communicator of one rank (ncclLaunchOneRank): all six collectives at 1, p - 1, p + 1 and 4,099 elements,
    in and out of place, over rm.PAIRS. A float average is PreMulSum by 1 / 1 through the reduce-copy kernel (in
    host memory through nexrReduceCopyHost), an integer average and everything else a copy, an all-gather's and
    a broadcast's of any bit pattern, NaN payloads included."""
    calls = [rm.make_call(sp, 1, SEED, oring) for sp in one_rank_plan()]
    mode = ring.DEVICE_MEMORY if memory == "device" else ring.HOST_MEMORY
    mapping = rh.Mapping(rh.mapping_bytes(rh.largest_arena(calls)))
    with ring.RingComm(1, mode, rm.BUFF["simple"], None, TIMEOUT_MS, 0, tree_ranks_per_node=1) as comm:
        for call in calls:
            context = ("one rank", memory)
            if memory == "device":
                dev = torch.from_numpy(call.arena0.copy()).cuda()
                torch.cuda.synchronize()
                rm.issue(comm, call, dev.data_ptr())
                torch.cuda.synchronize()
                rm.check(call, dev.cpu().numpy(), context)
                continue
            kind = memory[5:]
            with mapping.placed(kind, call, nexr.host_register, nexr.host_deregister) as (_pl, base, view):
                nexr.host_path_stats(reset=True)
                rm.issue(comm, call, base)
                st = nexr.host_path_stats()
                rm.check(call, view, context)
            sp = call.spec
            through_kernel = sp.op == rm.AVG and sp.dt in ae.FLOATS and sp.collective not in rm.COPIES
            assert st["calls"] == (1 if through_kernel else 0), (context, sp.what(), st)
            if through_kernel:
                check_how_it_ran(kind, st, (context, sp.what()))
