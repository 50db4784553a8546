"""Every member's run of LL steps in the same launches on ONE plain stream (nexrReduceCopyLLStepsGroup,
include/nexr.h), and the ring option built on it (nexrRingCommSetLLGroup, queued() == 3):
no stream here has a hardware queue of its own, so nothing below depends on two kernels being scheduled
together. Against numpy (two-operand sums, copies: exact), the oracle's LL step for the fold order of
three, and oracle.ring's LL schedules for the ring collectives."""
import importlib

import numpy as np
import pytest

import make_golden as mg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SLOTS = 8
TEST_RULE = (0x100, 0x78)  # the reference's TEST_LL_CLEANUP


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available()
    return importlib.import_module("nex-nccl_amd.ring")


@pytest.fixture(scope="module")
def stream(dev):
    """One plain stream for every group call of the file."""
    s = torch.cuda.Stream(device=dev)
    yield s.cuda_stream
    torch.cuda.synchronize()


def _conn(slot_bytes):
    """A connection's receive FIFO with its head words behind it, zeroed (as nexr_ring.cpp makes them)."""
    buf = torch.zeros(slot_bytes * SLOTS + 4096, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr(), buf.data_ptr() + slot_bytes * SLOTS


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _heads(keep, slot_bytes):
    return keep[slot_bytes * SLOTS:].view(torch.int64).cpu().numpy()[::2]


@pytest.mark.parametrize("slot_bytes", [4096, 1 << 16, 1 << 20])
@pytest.mark.parametrize("n_steps", [1, 9, 40])
def test_two_members_send_then_recv_reduce(nexr, dev, stream, slot_bytes, n_steps):
    """Member A sends n_steps steps of its input, member B receives each and writes peer + own input:
    both in one grid on one stream. 4 KiB slots: G = 1; 64 KiB: 8; 1 MiB: the 64-workgroup cap, two tiles
    per workgroup; 40 steps wrap the 8 slots five times."""
    per = slot_bytes // 2 // 4  # fp32 elements per full step
    sizes = [per - (k % 3) * 37 for k in range(n_steps)]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offs[-1])
    rng = np.random.default_rng(slot_bytes + n_steps)
    a = rng.standard_normal(total).astype(np.float32)
    b = rng.standard_normal(total).astype(np.float32)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    out = torch.zeros(total, dtype=torch.float32, device=dev)
    keep, fifo, head = _conn(slot_bytes)
    st = _status()
    torch.cuda.synchronize()
    a_steps = [nexr.ll_step(0, int(offs[k]), -1, 0, sizes[k], send=True) for k in range(n_steps)]
    b_steps = [nexr.ll_step(0, int(offs[k]), 1, int(offs[k]), sizes[k], recv=True) for k in range(n_steps)]
    ws = nexr.reduce_copy_ll_steps_group([(db.data_ptr(), out.data_ptr(), [(fifo, head, 0)], [], b_steps),
                                          (da.data_ptr(), 0, [], [(fifo, head, 0)], a_steps)],
                                         slot_bytes, mg.F32, 0, status=st.data_ptr(), timeout_us=5_000_000,
                                         stream=stream)
    torch.cuda.synchronize()
    assert ws is not None
    assert int(st.item()) == 0
    assert np.array_equal(out.cpu().numpy().view(np.uint32), (a + b).view(np.uint32))
    # the receiver's head words (one per wave at a 16-B stride): exactly the waves in use read every step
    waves = 4 * min(64, -(-(slot_bytes // 16) // 512))
    heads = _heads(keep, slot_bytes)
    assert list(heads[:waves]) == [n_steps] * waves and not heads[waves:].any()


@pytest.mark.parametrize("dt,op", [(mg.BF16, 0), (mg.F16, 1), (mg.I8, 2), (mg.F32, 4)])
def test_three_member_chain_matches_the_oracle(nexr, oracle, dev, stream, dt, op):
    """A -> B -> C in one launch: A sends its input, B receives, folds its own input (peer first) and
    forwards, C receives, folds, applies the post-op and writes its output — a ring Reduce's chain, 30
    steps over 8 slots."""
    from oracle.ring import reduce_expected
    slot = 1 << 15
    esz = np.dtype(mg.STORE[dt]).itemsize
    per = slot // 2 // esz
    n = 30
    total = n * per - 5
    sizes = [per] * (n - 1) + [total - (n - 1) * per]
    xs = mg.gen_inputs(dt, 3, total, 11 * dt + op, special=True)
    dev_op, arg = oracle.host_to_dev_red_op(op, dt, 3)
    dx = [torch.from_numpy(x.copy()).to(dev) for x in xs]
    out = torch.zeros_like(dx[2])
    _ab, ab_fifo, ab_head = _conn(slot)
    _bc, bc_fifo, bc_head = _conn(slot)
    st = _status()
    torch.cuda.synchronize()
    offs = [k * per for k in range(n)]
    members = [
        (dx[2].data_ptr(), out.data_ptr(), [(bc_fifo, bc_head, 0)], [],
         [nexr.ll_step(0, offs[k], 1, offs[k], sizes[k], recv=True, post_op=True) for k in range(n)]),
        (dx[1].data_ptr(), 0, [(ab_fifo, ab_head, 0)], [(bc_fifo, bc_head, 0)],
         [nexr.ll_step(0, offs[k], -1, 0, sizes[k], recv=True, send=True) for k in range(n)]),
        (dx[0].data_ptr(), 0, [], [(ab_fifo, ab_head, 0)],
         [nexr.ll_step(0, offs[k], -1, 0, sizes[k], send=True) for k in range(n)]),
    ]
    _ws = nexr.reduce_copy_ll_steps_group(members, slot, dt, dev_op, arg, status=st.data_ptr(), timeout_us=5_000_000,
                                          stream=stream)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    exp = reduce_expected(xs, dt, op, 2, "ll")
    assert mg.canon_bytes(dt, out.cpu().numpy()) == mg.canon_bytes(dt, exp)


def test_cuts_apply_to_every_member_at_the_same_step(nexr, dev, stream):
    """Two members with 200 steps of one tile each (more than the 96 of a launch), and a third that only
    copies within its user buffers: its step k writes output elements that its step k + 3 reads at a
    shifted position, so nearly every step ends the launch (rangesConflict) — for all three members at
    that step index. Exact against a one-step-at-a-time numpy model."""
    slot = 8192               # 512 lines: one tile, G = 1
    per = slot // 2 // 4      # 1024 fp32
    n_pair = 200
    rng = np.random.default_rng(77)
    a = rng.integers(-1000, 1000, n_pair * per).astype(np.float32)
    b = rng.integers(-1000, 1000, n_pair * per).astype(np.float32)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    out = torch.zeros_like(db)
    keep, fifo, head = _conn(slot)
    n, off, d, n_copy = 3000, 5000, 13, 30
    x = rng.integers(-100, 100, n).astype(np.float32)
    dx = torch.from_numpy(x).to(dev)
    cout = torch.zeros(4 * off, dtype=torch.float32, device=dev)
    c_steps = [nexr.ll_step(0, 0, 1, (k % 4) * off, n) for k in range(3)] + \
              [nexr.ll_step(1, ((k - 3) % 4) * off + d, 1, (k % 4) * off, n) for k in range(3, n_copy)]
    st = _status()
    torch.cuda.synchronize()
    members = [
        (db.data_ptr(), out.data_ptr(), [(fifo, head, 0)], [],
         [nexr.ll_step(0, k * per, 1, k * per, per, recv=True) for k in range(n_pair)]),
        (da.data_ptr(), 0, [], [(fifo, head, 0)], [nexr.ll_step(0, k * per, -1, 0, per, send=True) for k in range(n_pair)]),
        (dx.data_ptr(), cout.data_ptr(), [], [], c_steps),
    ]
    _ws = nexr.reduce_copy_ll_steps_group(members, slot, mg.F32, 0, status=st.data_ptr(), timeout_us=5_000_000,
                                          stream=stream)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    assert np.array_equal(out.cpu().numpy(), a + b)
    exp = np.zeros(4 * off, np.float32)
    for k in range(n_copy):
        src = x if k < 3 else exp[((k - 3) % 4) * off + d:((k - 3) % 4) * off + d + n].copy()
        exp[(k % 4) * off:(k % 4) * off + n] = src
    assert np.array_equal(cout.cpu().numpy(), exp)
    assert list(_heads(keep, slot)[:4]) == [n_pair] * 4


def test_flag_rule_cleanup_over_three_flag_wraps(nexr, dev, stream):
    """TEST_LL_CLEANUP {0x100, 0x78}: flags repeat every 256 steps and the steps 120-127 of every 128
    clean their slots (each ends a launch). 896 steps over 4 KiB slots, a full slot alternating with 3
    lines (and swapping at every wrap of the 8 slots, so each slot sees both sizes): without the cleanup
    a 3-line step's stale lines would carry a matching flag 256 steps later. Every step's output exact."""
    slot = 4096
    full, small = slot // 2 // 4, 6  # fp32 elements: 256 lines, 3 lines
    n_steps = 896
    sizes = [full if (k + k // SLOTS) % 2 == 0 else small for k in range(n_steps)]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offs[-1])
    rng = np.random.default_rng(5)
    a = rng.integers(-1000, 1000, total).astype(np.float32)
    b = rng.integers(-1000, 1000, total).astype(np.float32)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    out = torch.zeros_like(db)
    keep, fifo, head = _conn(slot)
    st = _status()
    torch.cuda.synchronize()
    members = [
        (da.data_ptr(), 0, [], [(fifo, head, 0)],
         [nexr.ll_step(0, int(offs[k]), -1, 0, sizes[k], send=True) for k in range(n_steps)]),
        (db.data_ptr(), out.data_ptr(), [(fifo, head, 0)], [],
         [nexr.ll_step(0, int(offs[k]), 1, int(offs[k]), sizes[k], recv=True) for k in range(n_steps)]),
    ]
    _ws = nexr.reduce_copy_ll_steps_group(members, slot, mg.F32, 0, status=st.data_ptr(), timeout_us=5_000_000,
                                          stream=stream, rule=TEST_RULE)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    got, exp = out.cpu().numpy(), a + b
    bad = [k for k in range(n_steps) if not np.array_equal(got[offs[k]:offs[k + 1]], exp[offs[k]:offs[k + 1]])]
    assert not bad, bad[:10]
    # the last cleaning step before the end: its slot's lines behind the data carry {0, flag, 0, flag}
    last = max(k for k in range(n_steps - SLOTS, n_steps) if nexr.ll_cleans(k, TEST_RULE) and sizes[k] == small)
    lines = keep[:slot * SLOTS].cpu().numpy().view(np.uint32).reshape(SLOTS, -1, 4)[last % SLOTS]
    n_lines = -(-sizes[last] * 4 // 8)
    f = nexr.ll_flag(last, TEST_RULE)
    assert (lines[n_lines:] == np.array([0, f, 0, f], np.uint32)).all()


def test_counters_carry_over_between_group_and_single_member_runs(nexr, dev, stream):
    """A group call, then nexrReduceCopyLLSteps calls (each end its own call, on streams of their own: the
    sender's is queued first and its 8 steps fit the slots, so the pair completes however the streams are
    scheduled), then a group call again — the same connection throughout, the step counters carried from
    one to the next (every launch re-stores the head words from recvStep). All exact."""
    slot = 1 << 14
    per = slot // 2 // 4
    _keep, fifo, head = _conn(slot)
    st = _status()
    sa, sb = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    step = 0
    for run, (n, how) in enumerate(((21, "group"), (8, "single"), (8, "single"), (13, "group"))):
        rng = np.random.default_rng(run)
        a = rng.integers(-1000, 1000, n * per).astype(np.float32)
        b = rng.integers(-1000, 1000, n * per).astype(np.float32)
        da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
        out = torch.zeros_like(db)
        torch.cuda.synchronize()
        a_steps = [nexr.ll_step(0, k * per, -1, 0, per, send=True) for k in range(n)]
        b_steps = [nexr.ll_step(0, k * per, 1, k * per, per, recv=True) for k in range(n)]
        if how == "group":
            _ws = nexr.reduce_copy_ll_steps_group([(db.data_ptr(), out.data_ptr(), [(fifo, head, step)], [], b_steps),
                                                   (da.data_ptr(), 0, [], [(fifo, head, step)], a_steps)],
                                                  slot, mg.F32, 0, status=st.data_ptr(), timeout_us=5_000_000,
                                                  stream=stream)
        else:
            nexr.reduce_copy_ll_steps(da.data_ptr(), 0, [], [(fifo, head, step)], slot, a_steps, mg.F32, 0,
                                      status=st.data_ptr(), timeout_us=5_000_000, stream=sa.cuda_stream)
            nexr.reduce_copy_ll_steps(db.data_ptr(), out.data_ptr(), [(fifo, head, step)], [], slot, b_steps, mg.F32,
                                      0, status=st.data_ptr(), timeout_us=5_000_000, stream=sb.cuda_stream)
        torch.cuda.synchronize()
        assert int(st.item()) == 0, (run, how)
        assert np.array_equal(out.cpu().numpy(), a + b), (run, how)
        step += n


def test_a_line_that_never_comes_ends_the_group_within_its_timeout(nexr, dev, stream):
    """One member receives on a one-ended connection nobody writes (the dry run takes it as ready: its
    peer is outside the group); the other member only copies. Every poll is bounded: the stream
    completes, the shared status word is 1, and no step's output of the waiting member is written. A
    valid group call on fresh connections right after it is exact."""
    import time
    slot = 1 << 16
    per = slot // 8
    _keep, fifo, head = _conn(slot)
    x = torch.ones(20 * per, dtype=torch.float32, device=dev)
    out = torch.zeros_like(x)
    y = torch.arange(5000, dtype=torch.float32, device=dev)
    yout = torch.zeros_like(y)
    st = _status()
    torch.cuda.synchronize()
    t0 = time.time()
    _ws = nexr.reduce_copy_ll_steps_group(
        [(x.data_ptr(), out.data_ptr(), [(fifo, head, 0)], [],
          [nexr.ll_step(0, k * per, 1, k * per, per, recv=True) for k in range(20)]),
         (y.data_ptr(), yout.data_ptr(), [], [], [nexr.ll_step(0, 0, 1, 0, 5000)])],
        slot, mg.F32, 0, status=st.data_ptr(), timeout_us=50_000, stream=stream)
    torch.cuda.synchronize()
    took = time.time() - t0
    assert int(st.item()) == 1
    assert took < 5.0, took
    assert not out.any()
    assert torch.equal(yout, y)
    # fresh connections, the same stream: exact
    rng = np.random.default_rng(9)
    n = 12
    a = rng.integers(-1000, 1000, n * per).astype(np.float32)
    b = rng.integers(-1000, 1000, n * per).astype(np.float32)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    res = torch.zeros_like(db)
    _keep2, fifo2, head2 = _conn(slot)
    st2 = _status()
    torch.cuda.synchronize()
    _ws2 = nexr.reduce_copy_ll_steps_group(
        [(da.data_ptr(), 0, [], [(fifo2, head2, 0)], [nexr.ll_step(0, k * per, -1, 0, per, send=True) for k in range(n)]),
         (db.data_ptr(), res.data_ptr(), [(fifo2, head2, 0)], [],
          [nexr.ll_step(0, k * per, 1, k * per, per, recv=True) for k in range(n)])],
        slot, mg.F32, 0, status=st2.data_ptr(), timeout_us=5_000_000, stream=stream)
    torch.cuda.synchronize()
    assert int(st2.item()) == 0
    assert np.array_equal(res.cpu().numpy(), a + b)


# ---- the ring option ---------------------------------------------------------------------------------
def _want_queued(n_ranks, on=True):
    one_gpu = torch.cuda.device_count() == 1
    if not one_gpu:
        return 0
    return 3 if on else (2 if n_ranks <= 3 else 0)


def _dev(arrs):
    out = [torch.from_numpy(a.copy()).cuda() for a in arrs]
    torch.cuda.synchronize()
    return out


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


@pytest.mark.parametrize("n_ranks", [2, 3, 4, 8])
def test_ring_all_reduce_in_group_launches(ring, oracle, n_ranks):
    """LL, device memory, set_ll_group(True): three all-reduces in a row on one communicator (the step
    counters, flags and head words carry over), every rank exact against the oracle's LL fold order;
    queued() == 3 on one GPU at 4 and 8 ranks too, where the rank streams exceed the hardware queues."""
    from oracle.ring import ring_allreduce_expected_ll
    count = 600_007
    with ring.RingComm(n_ranks, ring.DEVICE_MEMORY, 0, None, 20000, ring.PROTO_LL) as comm:
        comm.set_ll_group(True)
        for call in range(3):
            inputs = mg.gen_inputs(mg.F32, n_ranks, count, 1700 + 13 * call + n_ranks, special=True)
            send = _dev(inputs)
            recv = [torch.zeros_like(s) for s in send]
            torch.cuda.synchronize()
            comm.all_reduce(_ptrs(send), _ptrs(recv), count, mg.F32, 0)
            exp = ring_allreduce_expected_ll(inputs, mg.F32, 0)
            for r in range(n_ranks):
                assert mg.canon_bytes(mg.F32, recv[r].cpu().numpy()) == mg.canon_bytes(mg.F32, exp[r]), (call, r)
            assert comm.queued() == _want_queued(n_ranks), (comm.queued(), n_ranks)


def test_ring_every_other_collective_at_four_ranks(ring, oracle):
    from oracle.ring import reduce_scatter_expected, all_gather_expected, reduce_expected, broadcast_expected
    n, dt, op, count, root = 4, mg.BF16, 4, 150_001, 1
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, 20000, ring.PROTO_LL) as comm:
        comm.set_ll_group(True)
        inputs = mg.gen_inputs(dt, n, count, 1900, special=True)
        send = _dev(inputs)
        per = count // n
        rs = [torch.zeros(per, dtype=send[0].dtype, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        comm.reduce_scatter(_ptrs(send), _ptrs(rs), per, dt, op)
        assert comm.queued() == _want_queued(n)
        exp = reduce_scatter_expected([x[:per * n] for x in inputs], dt, op, "ll")
        for r in range(n):
            assert mg.canon_bytes(dt, rs[r].cpu().numpy()) == mg.canon_bytes(dt, exp[r]), ("rs", r)
        ag = [torch.zeros(per * n, dtype=send[0].dtype, device="cuda") for _ in range(n)]
        torch.cuda.synchronize()
        comm.all_gather([s[:per].data_ptr() for s in send], _ptrs(ag), per, dt)
        exp = all_gather_expected([x[:per] for x in inputs])
        for r in range(n):
            assert ag[r].cpu().numpy().tobytes() == exp[r].tobytes(), ("ag", r)
        rout = [torch.zeros_like(s) for s in send]
        torch.cuda.synchronize()
        comm.reduce(_ptrs(send), _ptrs(rout), count, dt, op, root)
        exp = reduce_expected(inputs, dt, op, root, "ll")
        assert mg.canon_bytes(dt, rout[root].cpu().numpy()) == mg.canon_bytes(dt, exp), "reduce"
        bout = [torch.zeros_like(s) for s in send]
        torch.cuda.synchronize()
        comm.broadcast(_ptrs(send), _ptrs(bout), count, dt, root)
        exp = broadcast_expected(inputs, root)
        for r in range(n):
            assert bout[r].cpu().numpy().tobytes() == np.asarray(exp[r]).tobytes(), ("bcast", r)
        assert comm.queued() == _want_queued(n)


def test_ring_four_ranks_two_channels(ring, oracle):
    """Eight members (2 channels x 4 ranks) in one group."""
    from oracle.ring import ring_allreduce_expected_ll
    n, ch, count = 4, 2, 600_007
    inputs = mg.gen_inputs(mg.F32, n, count, 2100, special=True)
    send = _dev(inputs)
    recv = [torch.zeros_like(s) for s in send]
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, 20000, ring.PROTO_LL, n_channels=ch) as comm:
        comm.set_ll_group(True)
        comm.all_reduce(_ptrs(send), _ptrs(recv), count, mg.F32, 0)
        assert comm.queued() == _want_queued(n)
    exp = ring_allreduce_expected_ll(inputs, mg.F32, 0, n_channels=ch)
    for r in range(n):
        assert mg.canon_bytes(mg.F32, recv[r].cpu().numpy()) == mg.canon_bytes(mg.F32, exp[r]), r


def test_ring_bf16_sum_at_eight_ranks(ring, oracle):
    from oracle.ring import ring_allreduce_expected_ll
    n, count = 8, 300_001
    inputs = mg.gen_inputs(mg.BF16, n, count, 2300, special=True)
    send = _dev(inputs)
    recv = [torch.zeros_like(s) for s in send]
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, 20000, ring.PROTO_LL) as comm:
        comm.set_ll_group(True)
        comm.all_reduce(_ptrs(send), _ptrs(recv), count, mg.BF16, 0)
        assert comm.queued() == _want_queued(n)
    exp = ring_allreduce_expected_ll(inputs, mg.BF16, 0)
    for r in range(n):
        assert mg.canon_bytes(mg.BF16, recv[r].cpu().numpy()) == mg.canon_bytes(mg.BF16, exp[r]), r


def test_ring_toggling_the_option_keeps_the_counters_exact(ring, oracle):
    """One communicator under TEST_LL_CLEANUP, the option on, off, on, off, on between all-reduces: both
    modes keep the same step counters and every launch re-stores the head words from them, so every call
    is exact, and the cleaning steps keep being counted (64 KiB FIFO: about 200 send steps a call, so
    every call crosses the cleaning steps 120-127 of some 128)."""
    from oracle.ring import ring_allreduce_expected_ll
    n, count, buff = 2, 200_003, 1 << 16
    with ring.RingComm(n, ring.DEVICE_MEMORY, buff, None, 20000, ring.PROTO_LL) as comm:
        comm.set_ll_flag_rule(*TEST_RULE)
        cleaned = 0
        for call, on in enumerate((True, False, True, False, True)):
            comm.set_ll_group(on)
            inputs = mg.gen_inputs(mg.F32, n, count, 2500 + call, special=True)
            send = _dev(inputs)
            recv = [torch.zeros_like(s) for s in send]
            torch.cuda.synchronize()
            comm.all_reduce(_ptrs(send), _ptrs(recv), count, mg.F32, 0)
            assert comm.queued() == _want_queued(n, on), (call, on)
            exp = ring_allreduce_expected_ll(inputs, mg.F32, 0, buff)
            for r in range(n):
                assert mg.canon_bytes(mg.F32, recv[r].cpu().numpy()) == mg.canon_bytes(mg.F32, exp[r]), (call, r)
            lo, now = comm.ll_cleanup()
            assert now > cleaned and lo > 0, (call, now, cleaned)
            cleaned = now


def test_ring_falls_back_when_the_group_does_not_fit_the_gpu(ring, oracle, monkeypatch):
    """The group call refuses a grid that is not resident at once (here through the library's test hook:
    room for one workgroup) before anything is launched; the collective then runs the way it would have
    without the option, from the step counters as they were before the rank threads recorded their steps
    — exact, and reported as that mode. With the hook gone the next call on the same communicator runs as
    group launches again, exact: the counters carried through the fall-back."""
    from oracle.ring import ring_allreduce_expected_ll
    n, count = 4, 300_001
    with ring.RingComm(n, ring.DEVICE_MEMORY, 0, None, 20000, ring.PROTO_LL) as comm:
        comm.set_ll_group(True)
        for call, fits in enumerate((True, False, True)):
            if fits:
                monkeypatch.delenv("NEXR_TEST_LL_GROUP_RESIDENT", raising=False)
            else:
                monkeypatch.setenv("NEXR_TEST_LL_GROUP_RESIDENT", "1")
            inputs = mg.gen_inputs(mg.F32, n, count, 2700 + call, special=True)
            send = _dev(inputs)
            recv = [torch.zeros_like(s) for s in send]
            torch.cuda.synchronize()
            comm.all_reduce(_ptrs(send), _ptrs(recv), count, mg.F32, 0)
            assert comm.queued() == _want_queued(n, fits), (call, fits)
            exp = ring_allreduce_expected_ll(inputs, mg.F32, 0)
            for r in range(n):
                assert mg.canon_bytes(mg.F32, recv[r].cpu().numpy()) == mg.canon_bytes(mg.F32, exp[r]), (call, r)
