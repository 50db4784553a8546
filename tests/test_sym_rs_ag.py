"""The symmetric reduce-scatter and all-gather (nexrSymReduceScatter, nexrSymAllGather and their ring entries)
without a GPU: the model the GPU test compares with (tests/sym_rs_ag_cases.py) is pinned by an exact-arithmetic
fold, the case table is shown to tell the rank-r-first fold from a rank-0-first one and the fp32 accumulator
from a rounding per step, and every rejection of the four calls is shown to come before any device call (this
machine has no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import sym_cases as sc
import sym_rs_ag_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [sc.NAMES[d] for d in sc.DTYPES]


@pytest.fixture(scope="module")
def ring(nexr):
    import importlib
    return importlib.import_module("nex-nccl_amd.ring")


# ---- the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("n", rc.RANKS)
def test_model_is_pinned_by_exact_sums_with_one_rounding_per_step(n, dt):
    """rs_expected (numpy float32 adds from rank r on, one conversion back) == fractions.Fraction sums rounded
    to float32 after every add and to T once at the end, on every finite element of every chunk."""
    count = 16 // sc.ESZ[dt] * 9 + 1  # packs and a tail; the special columns up to element 3 + 7 * 4
    ins = rc.rs_inputs(dt, n, count, [n, dt, 1])
    exp = rc.rs_expected(dt, ins, count)
    inf = sc._INF[dt]
    pinned = 0
    for r in range(n):
        for e in range(count):
            vals = [int(x[r * count + e]) for x in ins]
            if any(v & inf == inf for v in vals):
                continue
            try:
                want = sc.fold_fraction(dt, vals, r)
            except OverflowError:
                continue
            assert int(exp[r][e]) == want, (r, e, [hex(v) for v in vals])
            pinned += 1
    assert pinned > n * count * 3 // 4


def test_regions_are_what_the_counts_promise():
    for esz in (2, 4):
        p, g, P = 16 // esz, 1024 // esz, 2048 // esz
        regs = lambda c: set(np.unique(rc.chunk_regions(esz, c)).tolist())
        assert regs(1) == regs(p - 1) == {rc.TAIL}
        assert regs(p) == {rc.PACKS} and regs(p + 1) == {rc.PACKS, rc.TAIL}
        assert regs(g - 1) == regs(g + 1) == regs(P - 1) == {rc.PACKS, rc.TAIL}
        assert regs(P) == {rc.PIECES} and regs(P + 1) == {rc.PIECES, rc.TAIL}
        assert regs(3 * P + g + p + 1) == {rc.PIECES, rc.PACKS, rc.TAIL}
        for n in rc.RANKS:
            assert regs(2 * n * P + 37) == {rc.PIECES, rc.PACKS, rc.TAIL}
            assert len(rc.rs_counts(esz, n)) == 11 and rc.rs_counts(esz, n)[-2] == 3 * P + g + p + 1
            ins, outs = rc.rs_offsets(esz, n)
            assert all(o % esz == 0 and o < 16 for o in ins + outs)
            assert all(ins[r] != ins[r + 1] and outs[r] != outs[r + 1] for r in range(n - 1))
    for n in rc.AG_RANKS + (64,):
        for parity in (0, 1):
            ins, outs = rc.ag_offsets(n, parity)
            assert all(o % 2 == parity and o < 16 for o in ins + outs)
            assert all(ins[r] != ins[r + 1] and outs[r] != outs[r + 1] for r in range(n - 1))


@pytest.mark.parametrize("dt", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("n", rc.RANKS)
def test_table_tells_the_rank_r_first_fold_from_a_rank0_first_one(n, dt):
    """For every count of the table and every chunk r >= 1 the expectation differs from a rank-0-first fold at
    a witness of every non-empty region. With two ranks the two orders are the same sum (a + b == b + a in
    IEEE arithmetic), so there the outputs must be equal; chunk 0 is rank-0-first by the rule."""
    esz = sc.ESZ[dt]
    for count in rc.rs_counts(esz, n):
        ins = rc.rs_inputs(dt, n, count, [n, dt, count])
        if dt == sc.F32:  # the float32 inputs stay inside what the rule pins (sym_cases docstring)
            w = np.stack([sc.widen(dt, x) for x in ins])
            assert (np.isnan(w).sum(axis=0) <= 1).all()
            assert not ((w == np.inf).any(axis=0) & (w == -np.inf).any(axis=0)).any()
        exp, r0 = rc.rs_expected(dt, ins, count), rc.rs_rank0_first(dt, ins, count)
        assert np.array_equal(exp[0], r0[0])
        wit = rc.witness_positions(esz, count)
        assert set(wit) == set(np.unique(rc.chunk_regions(esz, count)).tolist())
        for r in range(1, n):
            if n == 2:
                assert np.array_equal(exp[r], r0[r])
                continue
            for reg, positions in wit.items():
                assert positions and all(exp[r][pos] != r0[r][pos] for pos in positions), (count, r, reg)


def test_accumulating_in_float32_differs_from_rounding_every_step():
    for dt in (sc.F16, sc.BF16):
        for n, lo in ((3, 0.1), (5, 0.2), (8, 0.3)):
            count = 2500
            rng = np.random.default_rng([n, dt, 2])
            ins = [sc.random_values(dt, rng, n * count) for _ in range(n)]
            a, b = np.concatenate(rc.rs_expected(dt, ins, count)), np.concatenate(rc.rs_per_step_rounding(dt, ins, count))
            frac = float((a != b).mean())
            assert frac > lo, (dt, n, frac)


def test_all_gather_model_is_the_inputs_in_rank_order():
    ins = rc.ag_inputs(3, 17, [3, 17])
    exp = rc.ag_expected(ins)
    assert exp.size == 51 and all(np.array_equal(exp[17 * r:17 * r + 17], ins[r]) for r in range(3))
    assert len({x.tobytes() for x in ins}) == 3


# ---- rejections, before any device call -------------------------------------------------------------------------
def _arr(v):
    return (ctypes.c_void_p * max(1, len(v)))(*v) if v is not None else None


def _rs(nexr, n, ins, outs, count, dt, op=0):
    return nexr.lib().nexrSymReduceScatter(n, _arr(ins), _arr(outs), count, dt, op, 0, None)


def _ag(nexr, n, ins, outs, n_bytes):
    return nexr.lib().nexrSymAllGather(n, _arr(ins), _arr(outs), n_bytes, None)


def test_sym_reduce_scatter_rejects_bad_arguments_before_any_device_call(nexr):
    ok, bad = int(nexr.Result.Success), int(nexr.Result.InvalidArgument)
    p = [0x10000 + 64 * i for i in range(130)]  # never dereferenced: every call below returns before a launch
    assert _rs(nexr, 2, None, p[:2], 8, sc.F32) == bad
    assert _rs(nexr, 2, p[:2], None, 8, sc.F32) == bad
    assert _rs(nexr, 2, [p[0], None], p[2:4], 8, sc.F32) == bad
    assert _rs(nexr, 2, p[:2], [None, p[3]], 8, sc.F32) == bad
    for n in (-1, 0, 1, 65):
        assert _rs(nexr, n, p[:65], p[65:130], 8, sc.F32) == bad
    for dt in (0, 1, 2, 3, 4, 5, 8, 10, 11, 12, -1):
        assert _rs(nexr, 2, p[:2], p[2:4], 8, dt) == bad
    for op in (1, 2, 3, 4, 5, -1):
        assert _rs(nexr, 2, p[:2], p[2:4], 8, sc.F32, op=op) == bad
    assert _rs(nexr, 2, [p[0], p[1] + 2], p[2:4], 8, sc.F32) == bad
    assert _rs(nexr, 2, p[:2], [p[2] + 2, p[3]], 8, sc.F32) == bad
    for dt in (sc.F16, sc.BF16):
        assert _rs(nexr, 3, [p[0], p[1], p[2] + 1], p[3:6], 8, dt) == bad
        assert _rs(nexr, 3, p[:3], [p[3] + 3, p[4], p[5]], 8, dt) == bad
    # nRanks * nElts * esz must fit size_t: the largest count that fits is refused one element further on
    top = (1 << 64) - 1
    for dt in sc.DTYPES:
        for n in (2, 3, 64):
            assert _rs(nexr, n, p[:64], p[64:128], top // sc.ESZ[dt] // n + 1, dt) == bad
    assert _rs(nexr, 2, p[:2], p[2:4], top, sc.F32) == bad
    # valid arguments and nothing to do: success, and no launch (there is no device to launch on here)
    for dt in sc.DTYPES:
        assert _rs(nexr, 2, [p[0] + 2 * sc.ESZ[dt], p[1]], p[2:4], 0, dt) == ok
        assert _rs(nexr, 64, p[:64], p[64:128], 0, dt) == ok
    with pytest.raises(nexr.NexrError) as e:
        nexr.sym_reduce_scatter(p[:1], p[1:2], 8, sc.F32)
    assert e.value.code == bad
    with pytest.raises(nexr.NexrError):
        nexr.sym_reduce_scatter(p[:2], p[2:5], 8, sc.F32)
    nexr.sym_reduce_scatter(p[:2], p[2:4], 0, sc.F32)


def test_sym_all_gather_rejects_bad_arguments_before_any_device_call(nexr):
    ok, bad = int(nexr.Result.Success), int(nexr.Result.InvalidArgument)
    p = [0x10001 + 67 * i for i in range(130)]  # any byte alignment is valid
    assert _ag(nexr, 2, None, p[:2], 8) == bad
    assert _ag(nexr, 2, p[:2], None, 8) == bad
    assert _ag(nexr, 2, [p[0], None], p[2:4], 8) == bad
    assert _ag(nexr, 2, p[:2], [None, p[3]], 8) == bad
    for n in (-1, 0, 1, 65):
        assert _ag(nexr, n, p[:65], p[65:130], 8) == bad
    top = (1 << 64) - 1
    for n in (2, 3, 64):
        assert _ag(nexr, n, p[:64], p[64:128], top // n + 1) == bad
    assert _ag(nexr, 2, p[:2], p[2:4], 0) == ok
    assert _ag(nexr, 64, p[:64], p[64:128], 0) == ok
    with pytest.raises(nexr.NexrError) as e:
        nexr.sym_all_gather(p[:1], p[1:2], 8)
    assert e.value.code == bad
    with pytest.raises(nexr.NexrError):
        nexr.sym_all_gather(p[:2], p[2:5], 8)
    nexr.sym_all_gather(p[:2], p[2:4], 0)


def test_ring_symmetric_rejections_on_a_host_memory_communicator(nexr, ring, oracle):
    """Arguments first (InvalidArgument), then the communicator's kind (InvalidUsage): host memory is not
    device memory. Nothing here reaches a device."""
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value
    bad, usage = int(nexr.Result.InvalidArgument), int(nexr.Result.InvalidUsage)
    send = [np.zeros(128, dtype=np.float32) for _ in range(2)]
    recv = [np.zeros(128, dtype=np.float32) for _ in range(2)]
    sp, rp = [b.ctypes.data for b in send], [b.ctypes.data for b in recv]
    L = ring.ring_lib()
    arr = lambda v: (ctypes.c_void_p * len(v))(*v)
    assert L.nexrRingReduceScatterSymmetric(None, arr(sp), arr(rp), 8, sc.F32, 0) == bad
    assert L.nexrRingAllGatherSymmetric(None, arr(sp), arr(rp), 8, sc.F32) == bad
    with ring.RingComm(2, ring.HOST_MEMORY, 1 << 14, fn, timeout_ms=20000) as comm:
        def code(call, *a):
            with pytest.raises(nexr.NexrError) as e:
                call(*a)
            return e.value.code
        for op in (1, 2, 3, 4):
            assert code(comm.reduce_scatter_symmetric, sp, rp, 8, sc.F32, op) == bad
        for dt in (0, 2, 4, 8, 10):
            assert code(comm.reduce_scatter_symmetric, sp, rp, 8, dt, 0) == bad
        for dt in (10, 11, 12, -1):
            assert code(comm.all_gather_symmetric, sp, rp, 8, dt) == bad
        assert code(comm.reduce_scatter_symmetric, [sp[0], 0], rp, 8, sc.F32, 0) == bad
        assert code(comm.all_gather_symmetric, sp, [0, rp[1]], 8, sc.F32) == bad
        assert L.nexrRingReduceScatterSymmetric(comm._h, None, arr(rp), 8, sc.F32, 0) == bad
        assert L.nexrRingAllGatherSymmetric(comm._h, arr(sp), None, 8, sc.F32) == bad
        for dt in sc.DTYPES:
            for count in (8, 0):
                assert code(comm.reduce_scatter_symmetric, sp, rp, count, dt, 0) == usage
                assert code(comm.all_gather_symmetric, sp, rp, count, dt) == usage
        assert code(comm.all_gather_symmetric, sp, rp, 8, 1) == usage  # uint8: every datatype of the ring's
        assert comm.queued() == 0
        assert all((b == 0).all() for b in send + recv)
        # the communicator still works
        for b in send:
            b[:] = 1.0
        comm.reduce_scatter(sp, rp, 64, sc.F32, 0)
        assert (recv[0][:64] == 2.0).all() and (recv[1][:64] == 2.0).all()
    with ring.RingComm(1, ring.HOST_MEMORY, 1 << 14, fn) as one:
        for call, a in ((one.reduce_scatter_symmetric, (sp[:1], rp[:1], 8, sc.F32, 0)),
                        (one.all_gather_symmetric, (sp[:1], rp[:1], 8, sc.F32))):
            with pytest.raises(nexr.NexrError) as e:
                call(*a)
            assert e.value.code == usage


# ---- the public surface ------------------------------------------------------------------------------------------
def test_headers_carry_the_rules_and_the_symbols(nexr, ring):
    with open(os.path.join(ROOT, "include", "nexr.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "include", "nexr_ring.h")) as f:
        rhdr = f.read()
    for name in ("nexrSymReduceScatter", "nexrSymAllGather"):
        assert re.search(r"NEXR_API\s+nexrResult_t\s+%s\s*\(" % name, hdr)
        assert name in nexr.ABI_SYMBOLS and hasattr(nexr.lib(), name)
    text = " ".join(hdr.split()).replace(" * ", " ")
    for sentence in ("symmetric/reduce_scatter.hh:6-241", "symmetric/all_gather.hh:5-177",
                     "acc = inputs[r][r nElts + e]", "acc = acc + inputs[(r + j) mod n][r nElts + e]",
                     "reduceDeep :23-89", "reduceEnds :118-157", "input + prim.rank*args->nElts, :237",
                     "ncclSymAccumType", "every NaN to 0x7fff", "reduce_scatter.hh:160-220",
                     "no output byte depends on alignment or on nBlocks", "the entry takes no nBlocks",
                     "reduce_scatter.hh:234-240", "outputs[r] may be chunk r of any rank's input",
                     "NCCL's in-place form is s = r", "Under nexrSemanticsShipped every add returns its first operand",
                     "nElts == 0 succeeds without a launch", "nRanks nElts esz overflowing",
                     "outputs[s][r nBytes + b] = inputs[r][b]", "the reference runs it on char, :173",
                     "inputs[r] == outputs[r] + r nBytes", "(:105, :33, :81), decided per rank",
                     "nBytes == 0 succeeds without a launch",
                     "multicast forms (…MC) of the symmetric ReduceScatter_LD / AllGather_ST are not built"):
        assert sentence in text, sentence
    for name in ("nexrRingReduceScatterSymmetric", "nexrRingAllGatherSymmetric"):
        assert re.search(r"NEXR_API\s+nexrResult_t\s+%s\s*\(" % name, rhdr)
        assert name in ring.RING_ABI_SYMBOLS and hasattr(ring.ring_lib(), name)
    rtext = " ".join(rhdr.split()).replace(" * ", " ")
    for sentence in ("symmetric/reduce_scatter.hh:6-241", "symmetric/all_gather.hh:5-177", "Never chosen automatically",
                     "sym_rs_ag_probe"):
        assert sentence in rtext, sentence
    assert rtext.count("it leaves nexrRingCommGetQueued as it was") == 3
    assert "ReduceScatter_LD and AllGather_ST are not built" not in rtext
    assert nexr.version() == 300  # additions only


def test_the_kernels_live_in_the_ll_object():
    from test_code_objects import PKG, _read, elf_tables, gfx950_code_objects
    path = os.path.join(PKG, "libnexr.so")
    if not os.path.exists(path):
        pytest.fail("libnexr.so not built")
    cos = gfx950_code_objects(_read(path))
    assert len(cos) == 11
    homes = []
    for co in cos:
        _t, notes = elf_tables(co)
        names = [k[".name"] for nn in notes for k in nn["amdhsa.kernels"]]
        rs = [x for x in names if "sym_reduce_scatter_kernel" in x]
        ag = [x for x in names if "sym_all_gather_kernel" in x]
        if rs or ag:
            homes.append((rs, ag, any("reduce_copy_ll_kernel" in x for x in names)))
    assert len(homes) == 1
    rs, ag, with_ll = homes[0]
    assert len(rs) == 3 and len(ag) == 1 and with_ll
