"""The kernels against tests/arith_edges.py's independent reference, bit for bit (fp32 / fp64 NaNs by class,
fp16 / bf16 including the canonical 0x7fff), on the operand sets of tests/test_arith_edges.py: every entry
point that folds — nexrReduceCopy, nexrReduceCopyBatch, nexrReduceCopyLL, nexrReduceCopyLL128,
nexrReduceCopyLLSteps[Rule], nexrReduceCopyLLStepsGroup and the 2-rank ring all-reduce. On a disagreement the
oracle's value is reported beside the kernel's and the reference's, so that a three-way difference reads at
once. Every destination has guard bytes. No case moves more than about 66 K elements per buffer."""
import importlib

import numpy as np
import pytest

import arith_edges as ae
from test_arith_edges import (_ref_cache, first_diff, ll_cases, ll_ops, premul_cases, reference, steps_cases,
                              STEPS_TYPES)
from test_reduce_copy_gpu import run_gpu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

RC_TYPES = (ae.F16, ae.BF16, ae.F32, ae.F64, ae.I8, ae.U8)
GUARD = 64
FILL = 0x5A


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def three_way(dt, got, exp, srcs, oracle_out):
    """None, or the first disagreement with the oracle's value at the same element."""
    d = first_diff(dt, got, exp, srcs)
    if d:
        d["oracle"] = hex(int(ae.canon(dt, oracle_out())[d["at"]]))
    return d


def check_reduce_copy(nexr, oracle, bad, ctx, dt, op, arg, srcs, exp, pre=None, post=False, semantics=ae.NCCL):
    """Both parities, M = 1 and M = 2."""
    for tag, ss in ae.both_parities(srcs):
        e = exp if tag == "even" else ae.pad_front(dt, op, arg, srcs, exp, pre, post, semantics=semantics)
        for m in (1, 2):
            for got in run_gpu(nexr, ss, m, dt, op, arg, pre, post):
                d = three_way(dt, got, e, ss, lambda: oracle.reduce_copy(ss, 1, dt, op, arg, pre, post)[0])
                if d:
                    bad.append((ctx, tag, m, d))


# ---- nexrReduceCopy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", RC_TYPES)
def test_reduce_copy_four_ops_every_layout(nexr, oracle, dev, dt):
    """K = 2 pairs, K = 3 triples and the K = 8 fold (and every fp16 pattern against seven rotations)."""
    bad = []
    for lname, srcs in ae.layouts(dt):
        for name, op, is_max in ae.FOUR_OPS:
            arg = ae.op_arg(dt, op, is_max)
            exp = reference(dt, lname, srcs, name, op, arg)
            check_reduce_copy(nexr, oracle, bad, (lname, name), dt, op, arg, srcs, exp)
    assert not bad, (len(bad), bad[:4])


@pytest.mark.parametrize("dt", RC_TYPES)
def test_reduce_copy_premulsum_scalar_sweep(nexr, oracle, dev, dt):
    """x * s and x0 * s0 + x1 * s1 for every scalar of the sweep (all 256 for the 8-bit types); for fp32 / fp64
    the operands whose unfused sum is exactly 0 and whose fused multiply-add is not."""
    bad = []
    for cname, srcs, pre in premul_cases(dt):
        exp = ae.fold(dt, ae.PREMULSUM, 0, srcs, pre, True)
        check_reduce_copy(nexr, oracle, bad, cname, dt, ae.PREMULSUM, 0, srcs, exp, pre, True)
    assert not bad, (len(bad), bad[:4])


@pytest.mark.parametrize("dt", ae.INTS)
def test_reduce_copy_sumpostdiv_divisor_sweep(nexr, oracle, dev, dt):
    """Every divisor x sign flag on every integer type; the combinations left out are refused before a launch."""
    valid, excluded = ae.postdiv_cases(dt)
    x = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for d, flag in excluded:
        with pytest.raises(nexr.NexrError):
            nexr.reduce_copy_ptrs([x.data_ptr()], [x.data_ptr()], 4, dt, ae.SUMPOSTDIV, (d << 1) | flag, None, True)
    bad = []
    for d, flag in valid:
        arg = (d << 1) | flag
        for k in (1, 2):
            srcs = ae.postdiv_sources(dt, d, k)
            exp = ae.fold(dt, ae.SUMPOSTDIV, arg, srcs, None, True)
            check_reduce_copy(nexr, oracle, bad, (hex(d), flag, k), dt, ae.SUMPOSTDIV, arg, srcs, exp, None, True)
    assert not bad, (len(bad), bad[:4])


def test_reduce_copy_int8_minmax_fork_semantics_compare_unsigned(nexr, oracle, dev):
    srcs = ae.byte_pairs()
    prev = nexr.get_semantics()
    bad = []
    try:
        nexr.set_semantics(int(nexr.Semantics.Fork))
        with oracle.semantics(ae.FORK):
            for is_max in (0, 1):
                arg = ae.minmax_arg(ae.I8, is_max)
                exp = ae.fold(ae.I8, ae.MINMAX, arg, srcs, semantics=ae.FORK)
                check_reduce_copy(nexr, oracle, bad, is_max, ae.I8, ae.MINMAX, arg, srcs, exp, semantics=ae.FORK)
    finally:
        nexr.set_semantics(prev)
    assert not bad, (len(bad), bad[:4])


# ---- nexrReduceCopyBatch -----------------------------------------------------------------------------------
def _dev_bytes(a, extra=GUARD):
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.zeros(raw.size + extra, dtype=torch.uint8, device="cuda")
    t[:raw.size] = torch.from_numpy(raw.copy()).cuda()
    return t


def _guarded_dst(n_bytes):
    return torch.full((n_bytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")


def _read_guarded(t, n_bytes, what):
    h = t.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[GUARD + n_bytes:] == FILL).all(), (what, "write outside the destination")
    return h[GUARD:GUARD + n_bytes].copy()


@pytest.mark.parametrize("dt", [ae.F16, ae.BF16, ae.I8])
def test_batch_three_works_in_one_call(nexr, oracle, dev, dt):
    """K = 2, 3 and 8 as three works of one nexrReduceCopyBatch (the batch kernels are compiled separately)."""
    lay = ae.layouts(dt)[:3]
    assert [len(s) for _n, s in lay] == [2, 3, 8]
    bad = []
    for name, op, is_max in ae.FOUR_OPS:
        arg = ae.op_arg(dt, op, is_max)
        for parity in (0, 1):
            works, keep, want = [], [], []
            for lname, srcs in lay:
                exp = reference(dt, lname, srcs, name, op, arg)
                tag, ss = ae.both_parities(srcs)[parity]
                if parity:
                    exp = ae.pad_front(dt, op, arg, srcs, exp)
                d_src = [_dev_bytes(s) for s in ss]
                d_dst = _guarded_dst(exp.nbytes)
                keep.append((d_src, d_dst))
                want.append((lname, ss, exp, d_dst))
                works.append(nexr.make_work([t.data_ptr() for t in d_src], [d_dst.data_ptr() + GUARD], exp.size, arg))
            torch.cuda.synchronize()
            nexr.reduce_copy_batch(works, dt, op, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            for lname, ss, exp, d_dst in want:
                got = _read_guarded(d_dst, exp.nbytes, (name, lname)).view(ae.UINT[dt])
                d = three_way(dt, got, exp, ss, lambda: oracle.reduce_copy(ss, 1, dt, op, arg)[0])
                if d:
                    bad.append((name, lname, parity, d))
    assert not bad, (len(bad), bad[:4])


# ---- nexrReduceCopyLL, nexrReduceCopyLL128 -------------------------------------------------------------------
def _ll_step_on_device(nexr, proto, dt, ss, recv, rflags, op, arg, post, sflag):
    n = ss[0].size
    nb = n * ss[0].itemsize
    d_src = _dev_bytes(ss[0])
    d_recv = [_dev_bytes(w) for w in recv]
    d_dst = _guarded_dst(nb)
    wire_bytes = ((nb + 7) // 8) * 16 if proto == "ll" else -(-nb // 1920) * 2048
    d_send = torch.zeros(wire_bytes + GUARD, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    call = nexr.reduce_copy_ll if proto == "ll" else nexr.reduce_copy_ll128
    call(d_src.data_ptr(), [t.data_ptr() for t in d_recv], rflags, d_dst.data_ptr() + GUARD, [d_send.data_ptr()],
         [sflag], n, dt, op, arg, True, post, status=status.data_ptr(), timeout_us=2_000_000,
         stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    wire = d_send.cpu().numpy()
    assert not wire[wire_bytes:].any(), "write behind the send wire"
    return _read_guarded(d_dst, nb, "ll dst").view(ae.UINT[dt]), wire[:wire_bytes].copy()


@pytest.mark.parametrize("proto", ["ll", "ll128"])
@pytest.mark.parametrize("dt", RC_TYPES)
def test_ll_and_ll128_steps(nexr, oracle, dev, dt, proto):
    """recvReduceCopySend on the pairs (peer, src) and twoPeers on the triples: the peer is the first operand.
    The user output, and the send wire's valid data bytes and flags."""
    from test_arith_edges import run_oracle_ll
    sflag = 77
    bad = []
    for lname, srcs in ll_cases(dt):
        for name, op, arg, post in ll_ops(dt):
            pre = [arg] if op == ae.PREMULSUM else None
            key = (dt, "ll_" + lname, name)
            if key not in _ref_cache:
                _ref_cache[key] = ae.fold_ll(dt, op, arg, srcs, pre, post)
            exp = _ref_cache[key]
            for tag, ss in ae.both_parities(srcs):
                e = exp if tag == "even" else ae.pad_front(dt, op, arg, srcs, exp, pre, post, ll=True)
                odst, osends, recv, rflags = run_oracle_ll(oracle, proto, dt, ss, op, arg, post, (sflag,))
                got, wire = _ll_step_on_device(nexr, proto, dt, ss, recv, rflags, op, arg, post, sflag)
                d = three_way(dt, got, e, ss, lambda: odst)
                if d:
                    bad.append((lname, name, tag, "dst", d))
                if proto == "ll":
                    data, flags = ae.ll_decode(wire, e.nbytes)
                    assert (flags == sflag).all(), (lname, name, tag, "flags")
                else:
                    w = wire.view(np.uint64).reshape(-1, 16)
                    assert (w[:, 15] == sflag).all(), (lname, name, tag, "flags")
                    rc, data, _ = oracle.reduce_copy_ll128(None, False, [wire], [sflag], True, 0, [], e.size, dt,
                                                           ae.SUM, 0, False)
                    assert rc == 0
                d = three_way(dt, data.view(ae.UINT[dt]), e, ss, lambda: odst)
                if d:
                    bad.append((lname, name, tag, "wire", d))
    assert not bad, (len(bad), bad[:4])


# ---- nexrReduceCopyLLStepsRule, nexrReduceCopyLLStepsGroup ------------------------------------------------------
@pytest.fixture(scope="module")
def stream(dev):
    s = torch.cuda.Stream(device=dev)
    yield s.cuda_stream
    torch.cuda.synchronize()


@pytest.mark.parametrize("how", ["run", "group"])
@pytest.mark.parametrize("dt", STEPS_TYPES)
def test_ll_steps_run_and_group_of_one(nexr, oracle, stream, dt, how):
    """One member, a receive connection pre-filled with the peer operand and a send connection, the pair
    layout in steps that fit the slot: the device against the interpreter (user buffers, every defined FIFO
    byte, flags and head words), and the interpreter's output against the reference."""
    import ll_steps_cases as cases
    from oracle import ll_steps
    from test_ll_steps_matrix_gpu import _run_and_check
    for name, tag, case, exp in steps_cases(dt):
        _members, before = cases.model(case)
        members, conns = cases.model(case)
        res = ll_steps.run(members, case.dt, case.op, case.arg)
        out = res.members[0].output.view(ae.UINT[dt])
        assert first_diff(dt, out, exp) is None, (name, tag, "interpreter vs reference", first_diff(dt, out, exp))
        _run_and_check(nexr, stream, (case, res, conns, [c.fifo for c in before]), how, (ae.NAMES[dt], name, tag, how))


# ---- the ring all-reduce, 2 ranks, device memory ------------------------------------------------------------------
RING_BUFF = {"simple": 1 << 16, "ll": 8 * 16 * 512, "ll128": 8 * 2048 * 8, "resident": 1 << 16}
SUM_OP, MIN_OP = 0, 3  # ncclRedOp_t


def _ring_module(which):
    if which == "resident":
        from conftest import extras_ring
        return extras_ring()  # skipped when the opt-in library is not built
    return importlib.import_module("nex-nccl_amd.ring")


@pytest.mark.parametrize("which", ["simple", "ll", "ll128", "resident"])
@pytest.mark.parametrize("dt", [ae.F16, ae.I8])
def test_ring_all_reduce_two_ranks(nexr, oracle, dev, dt, which):
    """The two ranks' inputs are the two operand vectors of the pair layout; a FIFO small enough for several
    chunks. oracle/ring.py fixes which rank is the first operand of a chunk (its arithmetic is the oracle's,
    pinned by tests/test_arith_edges.py); whichever it is, every element is one of the reference's two
    orders."""
    from oracle.ring import ring_allreduce_expected, ring_allreduce_expected_ll
    ring = _ring_module(which)
    buff = RING_BUFF[which]
    proto = {"simple": ring.PROTO_SIMPLE, "ll": ring.PROTO_LL, "ll128": ring.PROTO_LL128,
             "resident": ring.PROTO_SIMPLE}[which]
    a, b = dict(ae.layouts(dt))["pairs"]
    with ring.RingComm(2, ring.DEVICE_MEMORY, buff, None, 20000, proto) as comm:
        for rop, dev_op, is_max in ((SUM_OP, ae.SUM, 0), (MIN_OP, ae.MINMAX, 0)):
            arg = ae.op_arg(dt, dev_op, is_max)
            for tag, inputs in ae.both_parities([a, b]):
                count = inputs[0].size
                send = [_dev_bytes(x) for x in inputs]
                recv = [_guarded_dst(x.nbytes) for x in inputs]
                torch.cuda.synchronize()
                call = comm.all_reduce_resident if which == "resident" else comm.all_reduce
                call([s.data_ptr() for s in send], [r.data_ptr() + GUARD for r in recv], count, dt, rop)
                torch.cuda.synchronize()
                if which in ("simple", "resident"):
                    exp = ring_allreduce_expected(inputs, dt, rop, buff)
                else:
                    exp = ring_allreduce_expected_ll(inputs, dt, rop, buff, proto=which)
                ab = ae.canon(dt, ae.fold(dt, dev_op, arg, inputs))
                ba = ae.canon(dt, ae.fold(dt, dev_op, arg, inputs[::-1]))
                for r in range(2):
                    got = _read_guarded(recv[r], inputs[0].nbytes, (which, rop, tag, r)).view(ae.UINT[dt])
                    d = first_diff(dt, got, exp[r].view(ae.UINT[dt]), inputs)
                    assert d is None, (which, rop, tag, r, d)
                    g = ae.canon(dt, got)
                    assert ((g == ab) | (g == ba)).all(), (which, rop, tag, r, "neither order of the reference")
