"""The tree all-reduce in group launches (nexrTreeAllReduce under nexrRingCommSetLLGroup): the
root and every other rank's reduce-up and broadcast-down halves, 2n - 1 members a channel with up to 3 + 3
connections each, in the same LL / LL128 launches on one stream, queued() == 3. Every result is compared
with oracle.ring's tree fold order for the protocol; every fall-back reports 0 and is exact too. The small
FIFOs of tests/test_collectives_gpu.py (LL 64 KiB: 4,096 data bytes a step; LL128 128 KiB: 15,360), so a
few hundred KB a rank are over a hundred steps a member."""
import ctypes
import importlib

import pytest

import make_golden as mg
from oracle.ring import (reduce_scatter_expected, ring_allreduce_expected_ll, tree_allreduce_expected,
                         tree_allreduce_expected_channels, tree_topology)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BUFF = {1: 8 * 16 * 512, 2: 8 * 2048 * 8}
PNAME = {1: "ll", 2: "ll128"}
TEST_RULE = (0x100, 0x78)  # the reference's TEST_LL_CLEANUP
TIMEOUT_MS = 20000


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("nex-nccl_amd.ring")


def _want(on=True):
    """Group launches need every rank on one GPU."""
    return 3 if on and torch.cuda.device_count() == 1 else 0


def _dev(arrs):
    out = [torch.from_numpy(a.copy()).cuda() for a in arrs]
    torch.cuda.synchronize()
    return out


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _same(dt, got, exp, what):
    for r, e in enumerate(exp):
        assert mg.canon_bytes(dt, got[r].cpu().numpy()) == mg.canon_bytes(dt, e), (what, r)


def _tree(comm, proto, n, links, dt, op, count, seed, want):
    """One tree all-reduce on fresh inputs: exact, and reported as `want` (None: not looked at)."""
    inputs = mg.gen_inputs(dt, n, count, seed, special=True)
    send = _dev(inputs)
    recv = [torch.zeros_like(s) for s in send]
    torch.cuda.synchronize()
    comm.tree_all_reduce(_ptrs(send), _ptrs(recv), count, dt, op)
    if want is not None:
        assert comm.queued() == want, (comm.queued(), want, seed)
    _same(dt, recv, tree_allreduce_expected(inputs, dt, op, links, PNAME[proto]), seed)


@pytest.mark.parametrize("proto", [1, 2])
@pytest.mark.parametrize("n,per_node,tree_index,dt,op", [(2, 0, 0, mg.F32, 0), (5, 1, 0, mg.BF16, 0),
                                                         (8, 2, 0, mg.F32, 0), (6, 1, 1, mg.I32, 3),
                                                         (4, 0, 0, mg.F16, 4)])
def test_tree_all_reduce_in_group_launches(ring, oracle, proto, n, per_node, tree_index, dt, op):
    """The shapes of test_tree_all_reduce_device with the option on: two calls, the second in place on the
    first result. LL fp32 is 118 steps a member, so two launches; (8, 2, 0) has rank 4 with three children
    (a 3 + 1 and a 1 + 3 member)."""
    count = 120_011
    inputs = mg.gen_inputs(dt, n, count, 0x2300 + n + per_node, True)
    send = _dev(inputs)
    recv = [torch.zeros_like(s) for s in send]
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF[proto], None, TIMEOUT_MS, proto, tree_ranks_per_node=per_node,
                       tree_index=tree_index) as comm:
        comm.set_ll_group(True)
        comm.tree_all_reduce(_ptrs(send), _ptrs(recv), count, dt, op)
        assert comm.queued() == _want()
        comm.tree_all_reduce(_ptrs(recv), _ptrs(recv), count, dt, op)
        assert comm.queued() == _want()
    links = tree_topology(n, per_node, tree_index)
    exp = tree_allreduce_expected(inputs, dt, op, links, PNAME[proto])
    exp = tree_allreduce_expected(exp, dt, op, links, PNAME[proto])
    _same(dt, recv, exp, "second call")


def test_a_cut_under_ll128(ring, oracle):
    """1,600,012 B at 15,360 B a step: 105 steps a member, so the 96-step cut falls inside."""
    n, count = 4, 400_003
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF[2], None, TIMEOUT_MS, 2, tree_ranks_per_node=1) as comm:
        comm.set_ll_group(True)
        _tree(comm, 2, n, tree_topology(n, 1, 0), mg.F32, 0, count, 0x5100, _want())


@pytest.mark.parametrize("proto", [1, 2])
@pytest.mark.parametrize("n,per_node", [(4, 0), (8, 2)])
def test_two_channels(ring, oracle, proto, n, per_node):
    """14 and 30 members: the upper channel runs the other tree of the double binary tree."""
    ch, count, dt = 2, 150_001, mg.BF16
    inputs = mg.gen_inputs(dt, n, count, 0x5200 + n, True)
    send = _dev(inputs)
    recv = [torch.zeros_like(s) for s in send]
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF[proto], None, TIMEOUT_MS, proto, tree_ranks_per_node=per_node,
                       n_channels=ch) as comm:
        comm.set_ll_group(True)
        comm.tree_all_reduce(_ptrs(send), _ptrs(recv), count, dt, 0)
        assert comm.queued() == _want()
    exp = tree_allreduce_expected_channels(
        inputs, dt, 0, lambda k: tree_topology(n, per_node, 1 if k >= ch // 2 else 0), ch, PNAME[proto])
    _same(dt, recv, exp, "channels")


def test_ring_and_tree_calls_mixed_and_the_option_toggled(ring, oracle):
    """One 3-rank LL communicator under TEST_LL_CLEANUP: ring and tree calls use disjoint connections, and
    group launches and host-sequenced steps keep the same counters, so every call is exact in any order.
    A tree call here is 196 steps a connection, so each crosses cleaning steps 120-127 of some 128 and the
    cleanup count grows over it, in either mode."""
    n, count, dt, buff = 3, 200_003, mg.F32, BUFF[1]
    links = tree_topology(n, 0, 0)
    with ring.RingComm(n, ring.DEVICE_MEMORY, buff, None, TIMEOUT_MS, 1) as comm:
        comm.set_ll_flag_rule(*TEST_RULE)
        cleaned = 0
        for call, (what, on) in enumerate((("ring", True), ("tree", True), ("rs", True), ("tree", False),
                                           ("tree", True), ("ring", False), ("tree", True))):
            comm.set_ll_group(on)
            seed = 0x5300 + call
            if what == "tree":
                _tree(comm, 1, n, links, dt, 0, count, seed, _want() if on else None)
                now = comm.ll_cleanup()[1]
                assert now > cleaned, (call, now, cleaned)
            else:
                inputs = mg.gen_inputs(dt, n, count, seed, special=True)
                send = _dev(inputs)
                per = count // n
                recv = [torch.zeros(per if what == "rs" else count, dtype=send[0].dtype, device="cuda") for _ in send]
                torch.cuda.synchronize()
                if what == "rs":
                    comm.reduce_scatter(_ptrs(send), _ptrs(recv), per, dt, 0)
                    exp = reduce_scatter_expected([x[:per * n] for x in inputs], dt, 0, "ll")
                else:
                    comm.all_reduce(_ptrs(send), _ptrs(recv), count, dt, 0)
                    exp = ring_allreduce_expected_ll(inputs, dt, 0, buff)
                if on:  # off: the ring's own modes, which depend on the hardware queues left to it
                    assert comm.queued() == _want(), (call, what)
                _same(dt, recv, exp, (call, what))
            cleaned = comm.ll_cleanup()[1]


@pytest.mark.parametrize("proto", [1, 2])
def test_falls_back_when_the_grid_is_not_resident(ring, oracle, monkeypatch, proto):
    """The test hook leaves room for one workgroup during the second of three calls: it runs
    host-sequenced from the counters as they were before the recording, reports 0, and the third call runs
    as group launches again on the counters it left."""
    n, count = 4, 100_003
    links = tree_topology(n, 0, 0)
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF[proto], None, TIMEOUT_MS, proto) as comm:
        comm.set_ll_group(True)
        for call, fits in enumerate((True, False, True)):
            if fits:
                monkeypatch.delenv("NEXR_TEST_LL_GROUP_RESIDENT", raising=False)
            else:
                monkeypatch.setenv("NEXR_TEST_LL_GROUP_RESIDENT", "1")
            _tree(comm, proto, n, links, mg.F32, 0, count, 0x5400 + call, _want(fits))


@pytest.mark.parametrize("proto", [1, 2])
def test_falls_back_above_thirty_two_members(ring, oracle, proto):
    """8 ranks x 3 channels are 45 members."""
    n, ch, count, dt = 8, 3, 100_003, mg.F32
    inputs = mg.gen_inputs(dt, n, count, 0x5500, True)
    send = _dev(inputs)
    recv = [torch.zeros_like(s) for s in send]
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF[proto], None, TIMEOUT_MS, proto, n_channels=ch) as comm:
        comm.set_ll_group(True)
        comm.tree_all_reduce(_ptrs(send), _ptrs(recv), count, dt, 0)
        assert comm.queued() == 0
    exp = tree_allreduce_expected_channels(
        inputs, dt, 0, lambda k: tree_topology(n, 0, 1 if k >= ch // 2 else 0), ch, PNAME[proto])
    _same(dt, recv, exp, "45 members")


@pytest.mark.parametrize("proto", [1, 2])
def test_falls_back_with_a_callers_step_function(nexr, ring, oracle, proto):
    """A caller's llFn / ll128Fn (here the library's own single step under another address than the
    default's) is driven host-sequenced."""
    n, count = 4, 60_001
    fn = ctypes.cast(getattr(nexr.lib(), "nexrReduceCopyLL" if proto == 1 else "nexrReduceCopyLL128"),
                     ctypes.c_void_p).value
    kw = dict(ll_fn_address=fn) if proto == 1 else dict(ll128_fn_address=fn)
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF[proto], None, TIMEOUT_MS, proto, **kw) as comm:
        comm.set_ll_group(True)
        _tree(comm, proto, n, tree_topology(n, 0, 0), mg.F32, 0, count, 0x5600, 0)


def test_members_with_several_send_connections_clean_every_slot(ring, oracle):
    """TEST_LL_CLEANUP on the 8-rank tree whose rank 4 has three children and whose root has two: 196 send
    steps on each of the 14 connections from step 0, so every connection runs cleaning steps 120-127 once,
    the broadcast halves with 2-3 children on every child's slot in the same launches. Two calls, exact
    (the second wraps the 256-step flag period, where a slot left uncleaned would match a stale line), and
    the count is one per connection and cleaning step."""
    n, count, dt = 8, 200_003, mg.F32
    links = tree_topology(n, 2, 0)
    assert sorted(len(kids) for _up, kids in links)[-2:] == [2, 3]
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF[1], None, TIMEOUT_MS, 1, tree_ranks_per_node=2) as comm:
        comm.set_ll_flag_rule(*TEST_RULE)
        comm.set_ll_group(True)
        steps = -(-count * 4 // (BUFF[1] // 8 // 2))
        assert steps == 196
        for call in range(2):
            _tree(comm, 1, n, links, dt, 0, count, 0x5700 + call, _want())
            sent = steps * (call + 1)
            want = 2 * (n - 1) * sum(1 for s in range(sent) if s & TEST_RULE[1] == TEST_RULE[1])
            assert comm.ll_cleanup() == (sent, want), (call, comm.ll_cleanup(), sent, want)
