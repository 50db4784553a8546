"""The flat collectives without a GPU. include/nexr.h states the ring all-reduce, reduce-scatter and reduce element
by element (a start rank per position, then one reduce-copy step per rank); tests/flat_cases.py restates that
rule, and here it must give, with the oracle's three step functions, exactly what oracle/ring.py's chunk-loop
restatements of the three protocols give: over 2 / 3 / 4 / 8 ranks, 1 / 2 channels, the count table of
tests/ring_modes_cases.py (1 element to 2nC + 3) and the two-channel LARGE counts, on inputs whose result depends
on the fold order (asserted: moving every start rank by one changes the result). Then the argument checks of the
nexrFlat* entries and of nexrRingCommSetFlat, which answer before any device call."""
import ctypes
import importlib

import numpy as np
import pytest

import arith_edges as ae
import flat_cases as fc
import ring_modes_cases as rm
from oracle import ring as oring

SEED = rm.SEED


def chunk_of(coll, protocol, esz):
    return oring.chunk_count(coll, protocol, esz, rm.BUFF[protocol])


def parts_of(protocol, channels, count, esz):
    """The all-reduce's channel parts as nexrFlatAllReduce takes them: (offset, count, chunkCount) in elements."""
    chunk = chunk_of("all_reduce", protocol, esz)
    return [(off, cnt, chunk) for _ch, off, cnt in oring.channel_parts(channels, count, esz, 2, ll=protocol == "ll")]


def step_of(oracle, protocol, dt, op, n):
    """The step function of flat_cases' rule from the oracle's reduce-copy of `protocol`."""
    dev_op, arg = oracle.host_to_dev_red_op(op, dt, n)
    if protocol == "simple":
        def step(x, v, post):
            return oracle.reduce_copy([x] if v is None else [x, v], 1, dt, dev_op, arg, [arg], post)[0]
        return step
    fn = oracle.reduce_copy_ll if protocol == "ll" else oracle.reduce_copy_ll128

    def step(x, v, post):
        recv = [] if v is None else [v]
        rc, dst, sends = fn(x, True, recv, [1] * len(recv), post, 1, [1], x.size, dt, dev_op, arg, post)
        assert rc == 0
        return dst.view(x.dtype) if post else sends[0]
    return step


def model_outputs(oracle, call, protocol, channels, shift=0):
    sp, n = call.spec, call.n
    parts = parts_of(protocol, channels, sp.count, call.esz) if sp.collective == "all_reduce" else None
    return fc.model(sp.collective, call.inputs, sp.count, sp.root, step_of(oracle, protocol, sp.dt, sp.op, n), parts,
                    shift)


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            np.testing.assert_array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


# ---- the element-wise rule against the chunk-loop oracle ---------------------------------------------------------
@pytest.mark.parametrize("channels", rm.CHANNELS)
@pytest.mark.parametrize("n", rm.RANKS)
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_rule_is_the_oracles_ring(oracle, protocol, n, channels):
    seen = set()
    for sp in rm.plan(protocol, n, chunk_of, fc.COLLECTIVES):
        call = fc.Call(sp, n, SEED)
        same(model_outputs(oracle, call, protocol, channels), rm.oracle_outputs(oring, call, protocol, channels))
        seen.add(sp.collective)
    assert seen == set(fc.COLLECTIVES)


@pytest.mark.parametrize("n", rm.RANKS)
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_rule_on_two_channel_counts(oracle, protocol, n):
    """The LARGE counts: several loops on each of two channels, the second part's offset not at 0."""
    for k, coll in enumerate(fc.COLLECTIVES * 4):
        dt = rm.PAIRS[k % len(rm.PAIRS)][0]
        e = rm.esz_of(dt)
        count = rm.LARGE[coll](n, chunk_of(coll, protocol, e))
        sp = rm.spec(k, coll, "large", count, n)
        if coll == "all_reduce":
            assert len(parts_of(protocol, 2, count, e)) == 2
        call = fc.Call(sp, n, SEED)
        same(model_outputs(oracle, call, protocol, 2), rm.oracle_outputs(oring, call, protocol, 2))


def test_start_ranks_follow_the_chunks():
    """A known answer of the formula: 3 ranks, fp32, a part of 2 * 3 * 8 + 13 elements in chunks of 8: two full
    loops, then a last loop of 13 in chunks of alignUp(divUp(13, 3), 4) = 8, whose third chunk is empty."""
    s = fc.all_reduce_starts(3, 61, 4, [(0, 61, 8)])
    want = [1] * 8 + [2] * 8 + [0] * 8 + [1] * 8 + [2] * 8 + [0] * 8 + [1] * 8 + [2] * 5
    assert s.tolist() == want
    two = fc.all_reduce_starts(2, 24, 2, [(0, 16, 8), (16, 8, 8)])   # the second part starts its own loop
    assert two.tolist() == [1] * 8 + [0] * 8 + [1] * 8


# ---- the inputs ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [n for n in rm.RANKS if n >= 3])
@pytest.mark.parametrize("op", [rm.SUM, rm.PROD], ids=["sum", "prod"])
@pytest.mark.parametrize("dt", ae.FLOATS, ids=[ae.NAMES[d] for d in ae.FLOATS])
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_inputs_depend_on_the_start_rank(oracle, protocol, dt, op, n):
    """With every start rank moved by one, at least one expected element changes, for each of the three
    collectives: a wrong map cannot pass on these inputs."""
    e = rm.esz_of(dt)
    for k, coll in enumerate(fc.COLLECTIVES):
        count = n * chunk_of(coll, protocol, e) + n + 1
        call = fc.Call(rm.Spec(k, coll, "nC+n+1", count, dt, op, False, k % n), n, SEED)
        right = model_outputs(oracle, call, protocol, 1)
        wrong = model_outputs(oracle, call, protocol, 1, shift=1)
        for a, b in zip(right, wrong):
            if a is not None:
                assert not np.array_equal(ae.canon(dt, a), ae.canon(dt, b)), (coll, ae.NAMES[dt])


def test_inputs_hold_the_edge_classes():
    rng = np.random.default_rng(SEED)
    for dt in ae.FLOATS:
        xs = fc.gen_inputs(rng, dt, 4, 4096)
        allx = np.concatenate(xs)
        e_bits, m_bits = ae.FMT[dt]
        expo = (allx.astype(np.uint64) >> np.uint64(m_bits)) & np.uint64((1 << e_bits) - 1)
        mant = allx.astype(np.uint64) & np.uint64((1 << m_bits) - 1)
        assert ae.is_nan(dt, allx).any()
        assert ((expo == (1 << e_bits) - 1) & (mant == 0)).any()      # an infinity
        assert ((expo == 0) & (mant == 0)).any() and ((expo == 0) & (mant != 0)).any()   # a zero, a denormal
        if dt in (ae.F32, ae.F64):
            assert np.stack([ae.is_nan(dt, x) for x in xs]).sum(axis=0).max() == 1


# ---- argument checks, before any device call -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def L(nexr):
    return nexr.lib()


def _arr(vals):
    a = (ctypes.c_void_p * max(1, len(vals)))()
    for i, v in enumerate(vals):
        a[i] = v
    return a


def _parts(nexr, parts):
    return (nexr.FlatPart * max(1, len(parts)))(*[nexr.FlatPart(*p) for p in parts])


def test_flat_argument_checks(nexr, L):
    bad, ok = nexr.Result.InvalidArgument, nexr.Result.Success
    F32, SUM, DIV = nexr.DataType.Float32, nexr.DevRedOp.Sum, nexr.DevRedOp.SumPostDiv
    a = _arr([0x1000, 0x2000, 0x3000])
    one = _parts(nexr, [(0, 64, 16)])

    def ar(n=3, ins=a, outs=a, elts=64, dt=F32, op=SUM, arg=0, parts=one, nparts=1):
        return L.nexrFlatAllReduce(n, ins, outs, elts, int(dt), int(op), arg, 1, parts, nparts, None)

    def rs(n=3, ins=a, outs=a, elts=64, dt=F32, op=SUM, arg=0):
        return L.nexrFlatReduceScatter(n, ins, outs, elts, int(dt), int(op), arg, 1, None)

    def rd(n=3, ins=a, out=0x1000, root=0, elts=64, dt=F32, op=SUM, arg=0):
        return L.nexrFlatReduce(n, ins, out, root, elts, int(dt), int(op), arg, 0, None)

    # an empty call succeeds without a launch
    assert ar(elts=0, parts=None, nparts=0) == ok and rs(elts=0) == ok and rd(elts=0) == ok
    for call in (ar, rs):
        assert call(ins=None) == bad and call(outs=None) == bad
        assert call(ins=_arr([0x1000, None, 0x3000])) == bad and call(outs=_arr([0x1000, 0x2000, None])) == bad
        assert call(outs=_arr([0x1000, 0x2002, 0x3000])) == bad            # not aligned to 4
    assert rd(ins=None) == bad and rd(out=None) == bad and rd(ins=_arr([None, 0x2000, 0x3000])) == bad
    assert rd(out=0x1002) == bad and rd(root=-1) == bad and rd(root=3) == bad
    big = _arr([0x1000] * 65)
    for call in (ar, rs, rd):
        assert call(n=1) == bad and call(n=65, ins=big) == bad
        assert call(dt=nexr.DataType.Float8e4m3) == bad and call(dt=nexr.DataType.Float8e5m2) == bad
        assert call(dt=12) == bad and call(dt=-1) == bad and call(op=5) == bad and call(op=-1) == bad
        assert call(op=DIV) == bad                                           # floats have no SumPostDiv
        assert call(dt=nexr.DataType.Int8, op=DIV, arg=(256 << 1) | 1) == bad   # (int8_t)256 == 0
        assert call(ins=_arr([0x1000, 0x2001, 0x3000])) == bad              # not aligned to 4
    assert rs(elts=(1 << 62)) == bad and ar(elts=(1 << 62), parts=_parts(nexr, [(0, 1 << 62, 16)])) == bad
    assert rd(elts=(1 << 62)) == bad
    # the parts: null, gaps, overlaps, descending, short, long, empty, unaligned, zero chunk, n * chunkCount overflow
    assert ar(parts=None) == bad and ar(nparts=-1) == bad and ar(nparts=0) == bad
    for parts in ([(0, 32, 16)], [(0, 65, 16)], [(0, 32, 16), (48, 16, 16)], [(0, 48, 16), (32, 32, 16)],
                  [(32, 32, 16), (0, 32, 16)], [(0, 32, 16), (32, 0, 16), (32, 32, 16)], [(0, 30, 16), (30, 34, 16)],
                  [(0, 64, 0)], [(0, 64, 6)], [(0, 64, 1 << 63)], [(4, 60, 16)]):
        assert ar(parts=_parts(nexr, parts), nparts=len(parts)) == bad, parts
    u8 = nexr.DataType.Uint8
    assert ar(dt=u8, parts=_parts(nexr, [(0, 64, 8)])) == bad                # 16 / esz = 16 elements


def test_set_flat_argument_checks(nexr, oracle):
    ring = importlib.import_module("nex-nccl_amd.ring")
    RL = ring.ring_lib()
    assert RL.nexrRingCommSetFlat(None, 1) == nexr.Result.InvalidArgument
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value
    with ring.RingComm(2, ring.HOST_MEMORY, 8 * 1024, fn) as comm:      # host memory: never eligible
        with pytest.raises(nexr.NexrError) as e:
            comm.set_flat(True)
        assert e.value.code == nexr.Result.InvalidUsage
        with pytest.raises(nexr.NexrError) as e:
            comm.all_reduce_flat([1, 1], [1, 1], 4, nexr.DataType.Float32, 0)
        assert e.value.code == nexr.Result.InvalidUsage
        assert comm.queued() == 0
    for name in ("nexrRingAllReduceFlat", "nexrRingReduceScatterFlat"):
        assert getattr(RL, name)(None, None, None, 0, 7, 0) == nexr.Result.InvalidArgument
    assert RL.nexrRingReduceFlat(None, None, None, 0, 7, 0, 0) == nexr.Result.InvalidArgument
