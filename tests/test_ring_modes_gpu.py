"""The ring and tree collectives at small counts under every launch mode, on the MI355X: counts below and around
one pack and one chunk (tests/ring_modes_cases.py's table: ranks whose chunk is empty still wait, advance and post;
in the recorded modes that is records of zero elements at or past the end of the user buffer), all ten datatypes
and five ops, in and out of place, reduce and broadcast from every root, `count = 0`, and small and large calls
alternating on one communicator of two channels while the options are toggled (the channels' step counters, device
head / tail words and LL flags drift apart, and every group launch re-stores its words from the host counters).

The modes: SIMPLE host-sequenced, set_simple_group, set_direct and both; LL and LL128 as they run by themselves and
under set_ll_group; in worker processes LL forced host-sequenced (NEXR_LL_ASYNC=0) and queued (NEXR_LL_RUN=0). Device
memory, thread ranks, the smallest FIFOs the GPU tests of each protocol use, timeoutMs = 20000 (a stuck protocol
ends with an error).

Every call's memory is one arena compared whole with the expected bytes (rm.check): every rank's output, the guard
bytes round every user buffer, every input, and the outputs a reduce must not touch. The inputs make every result
independent of the fold order (tests/test_ring_modes.py), so all comparisons are exact."""
import importlib
import os
import subprocess
import sys

import pytest

import ring_modes_cases as rm
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


def _want(on=True):
    """Group launches need every rank on one GPU."""
    return 3 if on and torch.cuda.device_count() == 1 else 0


def make_comm(ring, protocol, n, channels):
    return ring.RingComm(n, ring.DEVICE_MEMORY, rm.BUFF[protocol], None, TIMEOUT_MS, rm.PROTO_ID[protocol],
                         tree_ranks_per_node=rm.tree_per_node(n), n_channels=channels)


def set_options(comm, protocol, group, direct):
    if protocol == "simple":
        comm.set_simple_group(group)
        comm.set_direct(direct)
    else:
        comm.set_ll_group(group)


def run_call(comm, call, context, count=None):
    """The call on a fresh copy of its arena in device memory, then the whole arena against the expected bytes
    (count = 0: against what it held before)."""
    dev = torch.from_numpy(call.arena0.copy()).cuda()
    torch.cuda.synchronize()
    rm.issue(comm, call, dev.data_ptr(), count)
    torch.cuda.synchronize()
    rm.check(call, dev.cpu().numpy(), context, expected=call.arena0 if count == 0 else None)


def check_how_it_ran(comm, sp, protocol, group, direct, context):
    """queued() == 3 after every ring collective in a group mode, and after a tree call under set_ll_group (the
    tree ignores the SIMPLE options); with set_direct, direct slices after all-gather, broadcast and out-of-place
    all-reduce and none after reduce-scatter, reduce and in-place all-reduce."""
    what = (context, sp.what())
    if sp.collective == "tree":
        if group and protocol != "simple":
            assert comm.queued() == _want(), (what, comm.queued())
        return
    if group:
        assert comm.queued() == _want(), (what, comm.queued())
    if direct and torch.cuda.device_count() == 1:
        d, f = comm.direct_slices()
        if sp.collective in ("all_gather", "broadcast") or (sp.collective == "all_reduce" and not sp.in_place):
            assert d > 0, (what, d, f)
        else:
            assert d == 0, (what, d, f)


def run_table(comm, protocol, n, channels, group, direct, context, collectives=rm.COLLECTIVES, queued_before_tree=None):
    """Every call of rm.plan on `comm`, and count = 0 once per collective, between two calls of it."""
    seen = {}
    for sp in rm.plan(protocol, n, chunk_of, collectives):
        call = rm.make_call(sp, n, SEED, oring, protocol, channels)
        seen[sp.collective] = seen.get(sp.collective, 0) + 1
        if seen[sp.collective] == 4:
            run_call(comm, call, context + ("count 0",), count=0)
        run_call(comm, call, context)
        check_how_it_ran(comm, sp, protocol, group, direct, context)
        if queued_before_tree is not None and "tree" not in seen:   # a tree call adds streams to the device
            assert comm.queued() == queued_before_tree, (context, sp.what(), comm.queued())
    assert all(seen[c] >= 11 for c in collectives), seen


@pytest.mark.parametrize("channels", rm.CHANNELS)
@pytest.mark.parametrize("n", rm.RANKS)
@pytest.mark.parametrize("mode", rm.MODES, ids=[m.id for m in rm.MODES])
def test_table(ring, oracle, mode, n, channels):
    context = (mode.id, n, channels)
    with make_comm(ring, mode.protocol, n, channels) as comm:
        set_options(comm, mode.protocol, mode.group, mode.direct)
        run_table(comm, mode.protocol, n, channels, mode.group, mode.direct, context)


@pytest.mark.parametrize("n", rm.RANKS)
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_mixed_sizes_and_toggles(ring, oracle, protocol, n):
    """24 seeded calls on one communicator of 2 channels: a tiny count (channel 0 only, empty chunks), a chunk
    edge, a count of several loops over both channels, and so on, the collectives drawn from all six; the option
    state changes every three calls (SIMPLE: none, group, direct, both; LL / LL128: group off and on)."""
    with make_comm(ring, protocol, n, 2) as comm:
        for sp in rm.mixed_plan(protocol, n, chunk_of, SEED + n):
            group, direct = rm.mixed_state(protocol, sp.k)
            set_options(comm, protocol, group, direct)
            context = (protocol, "group" if group else "", "direct" if direct else "", n, 2)
            run_call(comm, rm.make_call(sp, n, SEED, oring, protocol, 2), context)
            check_how_it_ran(comm, sp, protocol, group, direct, context)


_WORKER = r"""
import importlib, sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import oracle
import test_ring_modes_gpu as t
oracle.lib()
ring = importlib.import_module("nex-nccl_amd.ring")
want = {want} if torch.cuda.device_count() == 1 else 0
for n in (2, 3):
    with t.make_comm(ring, "ll", n, 1) as comm:
        t.run_table(comm, "ll", n, 1, False, False, ("ll", {env!r}, n, 1), queued_before_tree=want)
torch.cuda.synchronize()
print("TABLE-OK")
"""


@pytest.mark.parametrize("env,want", [({"NEXR_LL_ASYNC": "0"}, 0), ({"NEXR_LL_RUN": "0"}, 1)])
def test_ll_table_in_the_forced_modes(env, want):
    """NEXR_LL_ASYNC and NEXR_LL_RUN are read once per process: a fresh child for each, one after the other. The LL
    table at 2 and 3 ranks, host-sequenced (queued() == 0) and as queued launches of one step each (1)."""
    from conftest import GOLDEN, ROOT
    code = _WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=GOLDEN, want=want, env=env)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=150)
    assert out.returncode == 0 and "TABLE-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
