"""The symmetric LL collectives (nexrSymLLAllReduce, nexrSymLLReduceScatter, nexrSymLLAllGather and their ring
entries) without a GPU: the model the GPU test compares with (tests/sym_ll_cases.py) is pinned by an
exact-arithmetic fold, the case table is shown to tell the rank-0-first fold from the rank-r-first and
owner-first folds of the siblings and the fp32 accumulator from a rounding per step, the flag sequence is
checked across the wrap, and every rejection of the six entries is shown to come before any device call (this
machine has no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import sym_cases as sc
import sym_ll_cases as lc
import sym_rs_ag_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [sc.NAMES[d] for d in sc.DTYPES]


@pytest.fixture(scope="module")
def ring(nexr):
    import importlib
    return importlib.import_module("nex-nccl_amd.ring")


# ---- the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("n", lc.RANKS + (9,))
def test_model_is_pinned_by_exact_sums_with_one_rounding_per_step(n, dt):
    """rs_expected / ar_expected (numpy float32 adds from rank 0 on, one conversion back) == fractions.Fraction
    sums rounded to float32 after every add and to T once at the end, on every finite element."""
    count = 8 // sc.ESZ[dt] * 18 + 1
    ins = lc.rs_inputs(dt, n, count, [n, dt, 1])
    exp = np.concatenate(lc.rs_expected(dt, ins, count))
    assert np.array_equal(exp, lc.ar_expected(dt, ins))  # the all-reduce of the same vectors: the same fold
    inf = sc._INF[dt]
    pinned = 0
    for e in range(n * count):
        vals = [int(x[e]) for x in ins]
        if any(v & inf == inf for v in vals):
            continue
        try:
            want = sc.fold_fraction(dt, vals, 0)
        except OverflowError:
            continue
        assert int(exp[e]) == want, (e, [hex(v) for v in vals])
        pinned += 1
    assert pinned > n * count * 3 // 4


@pytest.mark.parametrize("dt", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("n", lc.RANKS + (9, 17))
def test_table_tells_the_rank0_first_fold_from_rank_r_first_and_owner_first(n, dt, nexr):
    """For n >= 3 and every chunk r >= 1 the expectation differs at a witness from the rank-r-first fold of
    nexrSymReduceScatter (sym_rs_ag_cases.rs_expected) and, for the all-reduce, from the owner-first fold of
    nexrSymAllReduce (sym_cases.expected) for every owner >= 1. With two ranks every order is the same IEEE sum,
    so there the outputs must be equal."""
    esz, R = sc.ESZ[dt], nexr.SYM_LL_ROUND_PACKS
    for P in (R - 1, R + 1):
        count = 8 * P // esz
        ins = lc.rs_inputs(dt, n, count, [n, dt, P])
        if dt == sc.F32:  # the float32 inputs stay inside what the rule pins (sym_cases docstring)
            w = np.stack([sc.widen(dt, x) for x in ins])
            assert (np.isnan(w).sum(axis=0) <= 1).all()
            assert not ((w == np.inf).any(axis=0) & (w == -np.inf).any(axis=0)).any()
        exp, rfirst = lc.rs_expected(dt, ins, count), rc.rs_expected(dt, ins, count)
        assert np.array_equal(exp[0], rfirst[0])
        wit = sorted(p for v in lc.witness_positions(count).values() for p in v)
        for r in range(1, n):
            if n == 2:
                assert np.array_equal(exp[r], rfirst[r])
            else:
                assert any(exp[r][p] != rfirst[r][p] for p in wit), (P, r)
        # the all-reduce of one chunk against the owner-first fold, owner by owner
        one = lc.chunks_of(ins, count, n - 1)
        mine = lc.ar_expected(dt, one)
        for o in range(1, n):
            theirs = sc.expected(dt, one, np.full(count, o, dtype=np.int32))
            if n == 2:
                assert np.array_equal(mine, theirs)
            else:
                assert any(mine[p] != theirs[p] for p in wit), (P, o)
        # and against the map a real call of nexrSymAllReduce would use
        owner, _region = sc.owner_map(n, 1, esz, count, 0, 0)
        theirs = sc.expected(dt, one, owner)
        for o in range(1, min(n, int(owner.max()) + 1)):
            sel = np.flatnonzero(owner == o)
            if n >= 3 and sel.size >= 14:
                assert (mine[sel] != theirs[sel]).any(), (P, o)


def test_witness_a_alone_cannot_tell_three_ranks_chunk_two():
    """Why witness B exists: with three ranks the orders (0, 1, 2) and (2, 0, 1) of witness A are both 0."""
    for dt in sc.DTYPES:
        v = [np.array([x], dtype=sc.UINT[dt]) for x in lc.witness_values(dt, 3, "A")]
        assert sc.fold_from(dt, v, 0)[0] == sc.fold_from(dt, v, 2)[0]
        assert sc.fold_from(dt, v, 0)[0] != sc.fold_from(dt, v, 1)[0]
        v = [np.array([x], dtype=sc.UINT[dt]) for x in lc.witness_values(dt, 3, "B")]
        assert sc.fold_from(dt, v, 0)[0] != sc.fold_from(dt, v, 2)[0]


def test_accumulating_in_float32_differs_from_rounding_every_step():
    for dt in (sc.F16, sc.BF16):
        for n, lo in ((3, 0.1), (5, 0.2), (8, 0.3)):
            count = 2500
            rng = np.random.default_rng([n, dt, 2])
            ins = [sc.random_values(dt, rng, n * count) for _ in range(n)]
            a = np.concatenate(lc.rs_expected(dt, ins, count))
            b = np.concatenate(lc.rs_per_step_rounding(dt, ins, count))
            frac = float((a != b).mean())
            assert frac > lo, (dt, n, frac)


def test_shipped_is_rank_zero_through_the_casts():
    for dt in sc.DTYPES:
        ins = lc.rs_inputs(dt, 3, 40, [dt, 3])
        want = sc.narrow(dt, sc.widen(dt, ins[0]))
        assert np.array_equal(np.concatenate(lc.rs_expected_shipped(dt, ins, 40)), want)
        assert np.array_equal(lc.ar_expected_shipped(dt, ins), want)
        if dt != sc.F32:
            assert (want == 0x7FFF).any()  # a NaN of rank 0 is canonical afterwards


def test_all_gather_model_is_the_inputs_in_rank_order():
    ins = lc.ag_inputs(3, 17, [3, 17])
    exp = lc.ag_expected(ins)
    assert exp.size == 51 and all(np.array_equal(exp[17 * r:17 * r + 17], ins[r]) for r in range(3))


# ---- the flags ---------------------------------------------------------------------------------------------------
def test_flag_sequence_across_the_wrap():
    got, stored = lc.flags(0xFFFFFFFA, 8)
    assert got == [0xFFFFFFFC, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF, 2, 3, 4, 5]
    assert stored == 4
    assert lc.flags(0, 3) == ([2, 3, 4], 3)
    assert lc.flags(0xFFFFFFFD, 1) == ([0xFFFFFFFF], 0)
    assert lc.flags(7, 0) == ([], 7)
    # consecutive flags alternate in parity, across the wrap too: two buffers are enough
    assert all((a ^ b) & 1 for a, b in zip(got, got[1:]))


def test_split_and_rounds(nexr):
    R = nexr.SYM_LL_ROUND_PACKS
    for P in (0, 1, 2, R, 3 * R + 1, 12345):
        for B in (1, 2, 3, 16, 64):
            s = [lc.share(P, B, b) for b in range(B)]
            assert sum(s) == P and max(s) - min(s) <= 1 and s == sorted(s, reverse=True)
    assert [lc.rounds(3 * R + 1, 3, b, R) for b in range(3)] == [2, 1, 1]
    assert [lc.rounds(2, 3, b, R) for b in range(3)] == [1, 1, 0]
    assert lc.rounds(2 * R + 3, 1, 0, R) == 3
    words = lc.advance([0xFFFFFFFA] * 64, 3 * R + 1, 3, R)
    assert words[:4] == [0xFFFFFFFC, 0xFFFFFFFB, 0xFFFFFFFB, 0xFFFFFFFA]
    for esz in (2, 4):
        assert lc.byte_counts(5, esz, False) == [40, 32 + esz]
    assert lc.byte_counts(5, 1, True) == [40, 33, 35, 39]
    assert all(lc.packs(b) == 5 for b in lc.byte_counts(5, 2, False) + lc.byte_counts(5, 1, True))
    for esz in (1, 2, 4):
        for aligned in (True, False):
            i, o = lc.offsets(esz, 8, aligned)
            assert all(x % esz == 0 and 0 <= x < 16 for x in i + o)
            assert all((x % 8 == 0) == aligned for x in i + o)


# ---- nexrSymLLWindowBytes ----------------------------------------------------------------------------------------
def _wb(nexr, n, blocks):
    out = ctypes.c_size_t(0)
    rc_ = nexr.lib().nexrSymLLWindowBytes(n, blocks, ctypes.byref(out))
    return rc_, out.value


def test_window_bytes_is_monotone_and_rejects_out_of_range(nexr):
    ok, bad = int(nexr.Result.Success), int(nexr.Result.InvalidArgument)
    R, H = nexr.SYM_LL_ROUND_PACKS, nexr.SYM_LL_HEADER_BYTES
    assert H >= 64 * 4 and H % 16 == 0
    prev_n = 0
    for n in range(2, nexr.SYM_MAX_RANKS + 1):
        prev_b = 0
        for blocks in range(1, nexr.SYM_LL_MAX_BLOCKS + 1):
            code, v = _wb(nexr, n, blocks)
            assert code == ok and v == H + blocks * 2 * n * R * 16
            assert v > prev_b and v % 16 == 0
            prev_b = v
        assert _wb(nexr, n, 1)[1] > prev_n
        prev_n = _wb(nexr, n, 1)[1]
    for n in (-1, 0, 1, 65):
        assert _wb(nexr, n, 1)[0] == bad
    for blocks in (-1, 0, 65):
        assert _wb(nexr, 2, blocks)[0] == bad
    assert nexr.lib().nexrSymLLWindowBytes(2, 1, None) == bad
    assert nexr.sym_ll_window_bytes(8, 16) == H + 16 * 2 * 8 * R * 16
    with pytest.raises(nexr.NexrError):
        nexr.sym_ll_window_bytes(1, 1)


# ---- rejections, before any device call -------------------------------------------------------------------------
def _arr(v):
    return (ctypes.c_void_p * max(1, len(v)))(*v) if v is not None else None


def _call(nexr, coll, n, ins, outs, count, dt=sc.F32, op=0, wins=None, wbytes=None, blocks=1):
    L = nexr.lib()
    if wbytes is None:
        wbytes = 1 << 40
    tail = (_arr(wins), wbytes, blocks, None, 0, None)
    if coll == "ag":
        return L.nexrSymLLAllGather(n, _arr(ins), _arr(outs), count, *tail)
    fn = L.nexrSymLLAllReduce if coll == "ar" else L.nexrSymLLReduceScatter
    return fn(n, _arr(ins), _arr(outs), count, dt, op, 0, *tail)


@pytest.mark.parametrize("coll", ["ar", "rs", "ag"])
def test_sym_ll_rejects_bad_arguments_before_any_device_call(nexr, coll):
    ok, bad = int(nexr.Result.Success), int(nexr.Result.InvalidArgument)
    p = [0x10000 + 64 * i for i in range(200)]  # never dereferenced: every call below returns before a launch
    i2, o2, w2 = p[:2], p[2:4], p[4:6]
    assert _call(nexr, coll, 2, None, o2, 8, wins=w2) == bad
    assert _call(nexr, coll, 2, i2, None, 8, wins=w2) == bad
    assert _call(nexr, coll, 2, i2, o2, 8, wins=None) == bad
    assert _call(nexr, coll, 2, [p[0], None], o2, 8, wins=w2) == bad
    assert _call(nexr, coll, 2, i2, [None, p[3]], 8, wins=w2) == bad
    assert _call(nexr, coll, 2, i2, o2, 8, wins=[p[4], None]) == bad
    for n in (-1, 0, 1, 65):
        assert _call(nexr, coll, n, p[:65], p[65:130], 8, wins=p[130:195]) == bad
    for blocks in (-1, 65, 1000):
        assert _call(nexr, coll, 2, i2, o2, 8, wins=w2, blocks=blocks) == bad
    # windows: 16-byte aligned, and large enough for (n, B)
    for off in (1, 2, 4, 8):
        assert _call(nexr, coll, 2, i2, o2, 8, wins=[p[4], p[5] + off]) == bad
    for n, blocks in ((2, 1), (2, 0), (3, 16), (64, 64)):
        need = nexr.sym_ll_window_bytes(n, max(1, blocks))
        args = (nexr, coll, n, p[:64], p[64:128], 0)
        assert _call(*args, wins=p[128:192], wbytes=need - 1, blocks=blocks) == bad
        assert _call(*args, wins=p[128:192], wbytes=need, blocks=blocks) == ok
    if coll != "ag":
        for dt in (0, 1, 2, 3, 4, 5, 8, 10, 11, 12, -1):
            assert _call(nexr, coll, 2, i2, o2, 8, dt=dt, wins=w2) == bad
        for op in (1, 2, 3, 4, 5, -1):
            assert _call(nexr, coll, 2, i2, o2, 8, op=op, wins=w2) == bad
        assert _call(nexr, coll, 2, [p[0], p[1] + 2], o2, 8, wins=w2) == bad
        assert _call(nexr, coll, 2, i2, [p[2] + 2, p[3]], 8, wins=w2) == bad
        for dt in (sc.F16, sc.BF16):
            assert _call(nexr, coll, 3, [p[0], p[1], p[2] + 1], p[3:6], 8, dt=dt, wins=p[6:9]) == bad
    # a buffer (the reduce-scatter's whole input) stays below 2^31 bytes; products do not overflow
    top = (1 << 64) - 1
    for dt in sc.DTYPES if coll != "ag" else (sc.F32,):
        esz = 1 if coll == "ag" else sc.ESZ[dt]
        for n in (2, 3, 64):
            limit = (1 << 31) // esz // (n if coll == "rs" else 1)
            args = (nexr, coll, n, p[:64], p[64:128])
            assert _call(*args, limit, dt=dt, wins=p[128:192]) == bad
            assert _call(*args, min(top, top // esz + 1), dt=dt, wins=p[128:192]) == bad
            assert _call(*args, top, dt=dt, wins=p[128:192]) == bad
    # valid arguments and nothing to do: success, and no launch (there is no device to launch on here)
    assert _call(nexr, coll, 2, i2, o2, 0, wins=w2) == ok
    assert _call(nexr, coll, 64, p[:64], p[64:128], 0, wins=p[128:192], blocks=64) == ok
    if coll == "ag":
        assert _call(nexr, coll, 2, [p[0] + 1, p[1] + 3], [p[2] + 5, p[3] + 7], 0, wins=w2) == ok


def test_python_wrappers_check_the_lists(nexr):
    p = [0x10000 + 64 * i for i in range(8)]
    bad = int(nexr.Result.InvalidArgument)
    for call, a in ((nexr.sym_ll_all_reduce, (p[:2], p[2:4], 8, sc.F32, p[4:7], 1 << 30)),
                    (nexr.sym_ll_reduce_scatter, (p[:2], p[2:5], 8, sc.F32, p[5:7], 1 << 30)),
                    (nexr.sym_ll_all_gather, (p[:3], p[3:5], 8, p[5:7], 1 << 30)),
                    (nexr.sym_ll_all_reduce, (p[:1], p[1:2], 8, sc.F32, p[2:3], 1 << 30))):
        with pytest.raises(nexr.NexrError) as e:
            call(*a)
        assert e.value.code == bad
    nexr.sym_ll_all_reduce(p[:2], p[2:4], 0, sc.F32, p[4:6], 1 << 30)
    nexr.sym_ll_reduce_scatter(p[:2], p[2:4], 0, sc.BF16, p[4:6], 1 << 30, n_blocks=3)
    nexr.sym_ll_all_gather(p[:2], p[2:4], 0, p[4:6], 1 << 30)


def test_ring_symmetric_ll_rejections_on_a_host_memory_communicator(nexr, ring, oracle):
    """Arguments first (InvalidArgument), then the communicator's kind (InvalidUsage): host memory is not
    device memory. Nothing here reaches a device."""
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value
    bad, usage = int(nexr.Result.InvalidArgument), int(nexr.Result.InvalidUsage)
    send = [np.zeros(128, dtype=np.float32) for _ in range(2)]
    recv = [np.zeros(128, dtype=np.float32) for _ in range(2)]
    sp, rp = [b.ctypes.data for b in send], [b.ctypes.data for b in recv]
    L = ring.ring_lib()
    arr = lambda v: (ctypes.c_void_p * len(v))(*v)
    assert L.nexrRingAllReduceSymmetricLL(None, arr(sp), arr(rp), 8, sc.F32, 0, 0) == bad
    assert L.nexrRingReduceScatterSymmetricLL(None, arr(sp), arr(rp), 8, sc.F32, 0, 0) == bad
    assert L.nexrRingAllGatherSymmetricLL(None, arr(sp), arr(rp), 8, sc.F32, 0) == bad
    with ring.RingComm(2, ring.HOST_MEMORY, 1 << 14, fn, timeout_ms=20000) as comm:
        def code(call, *a):
            with pytest.raises(nexr.NexrError) as e:
                call(*a)
            return e.value.code
        for call in (comm.all_reduce_symmetric_ll, comm.reduce_scatter_symmetric_ll):
            for op in (1, 2, 3, 4):
                assert code(call, sp, rp, 8, sc.F32, op) == bad
            for dt in (0, 2, 4, 8, 10):
                assert code(call, sp, rp, 8, dt, 0) == bad
            for blocks in (-1, 17, 64):
                assert code(call, sp, rp, 8, sc.F32, 0, blocks) == bad
            assert code(call, [sp[0], 0], rp, 8, sc.F32, 0) == bad
        for dt in (10, 11, 12, -1):
            assert code(comm.all_gather_symmetric_ll, sp, rp, 8, dt) == bad
        for blocks in (-1, 17):
            assert code(comm.all_gather_symmetric_ll, sp, rp, 8, sc.F32, blocks) == bad
        assert code(comm.all_gather_symmetric_ll, sp, [0, rp[1]], 8, sc.F32) == bad
        assert L.nexrRingAllReduceSymmetricLL(comm._h, None, arr(rp), 8, sc.F32, 0, 0) == bad
        assert L.nexrRingAllGatherSymmetricLL(comm._h, arr(sp), None, 8, sc.F32, 0) == bad
        for dt in sc.DTYPES:
            for count in (8, 0):
                for blocks in (0, 16):
                    assert code(comm.all_reduce_symmetric_ll, sp, rp, count, dt, 0, blocks) == usage
                    assert code(comm.reduce_scatter_symmetric_ll, sp, rp, count, dt, 0, blocks) == usage
                    assert code(comm.all_gather_symmetric_ll, sp, rp, count, dt, blocks) == usage
        assert code(comm.all_gather_symmetric_ll, sp, rp, 8, 1) == usage  # uint8: every datatype of the ring's
        assert comm.queued() == 0
        assert all((b == 0).all() for b in send + recv)
        for b in send:  # the communicator still works
            b[:] = 1.0
        comm.reduce_scatter(sp, rp, 64, sc.F32, 0)
        assert (recv[0][:64] == 2.0).all() and (recv[1][:64] == 2.0).all()
    with ring.RingComm(1, ring.HOST_MEMORY, 1 << 14, fn) as one:
        with pytest.raises(nexr.NexrError) as e:
            one.all_reduce_symmetric_ll(sp[:1], rp[:1], 8, sc.F32, 0)
        assert e.value.code == usage


# ---- the public surface ------------------------------------------------------------------------------------------
def test_headers_carry_the_rules_and_the_symbols(nexr, ring):
    with open(os.path.join(ROOT, "include", "nexr.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "include", "nexr_ring.h")) as f:
        rhdr = f.read()
    for name in ("nexrSymLLWindowBytes", "nexrSymLLAllReduce", "nexrSymLLReduceScatter", "nexrSymLLAllGather"):
        assert re.search(r"NEXR_API\s+nexrResult_t\s+%s\s*\(" % name, hdr)
        assert name in nexr.ABI_SYMBOLS and hasattr(nexr.lib(), name)
    for macro, value in (("NEXR_SYM_LL_HEADER_BYTES", nexr.SYM_LL_HEADER_BYTES),
                         ("NEXR_SYM_LL_ROUND_PACKS", nexr.SYM_LL_ROUND_PACKS),
                         ("NEXR_SYM_LL_MAX_BLOCKS", nexr.SYM_LL_MAX_BLOCKS)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr)
    text = " ".join(hdr.split()).replace(" * ", " ")
    for sentence in ("all_reduce.hh:356-428", "reduce_scatter.hh:320-388", "all_gather.hh:256-363",
                     "primitives.hh:212-377", "acc = inputs[0][e], then acc = acc + inputs[j][e] for j = 1..n-1",
                     "every NaN to 0x7fff", "no byte depends on alignment, on nBlocks or on the 8-byte pack",
                     "rank-0-first fp32 fold of inputs[j][r nElts + e]", "outputs[s][r nBytes + b] = inputs[r][b]",
                     "uint32_t llEpoch[64]", "flags 0 and 1 never occur", "after 0xffffffff the next flag is 2",
                     "flag is >= 0xfffffffe", "every wave drains before the barrier",
                     "the caller zeroes ALL windows before the next call",
                     "A count of 0 succeeds without a launch and leaves the epoch words alone",
                     "not resident as a whole"):
        assert sentence in text, sentence
    assert "LL variants (AGxLL_R)" not in text
    for name in ("nexrRingAllReduceSymmetricLL", "nexrRingReduceScatterSymmetricLL", "nexrRingAllGatherSymmetricLL"):
        assert re.search(r"NEXR_API\s+nexrResult_t\s+%s\s*\(" % name, rhdr)
        assert name in ring.RING_ABI_SYMBOLS and hasattr(ring.ring_lib(), name)
    rtext = " ".join(rhdr.split()).replace(" * ", " ")
    assert "LL symmetric kernels are not built" not in rtext and "sym_ll_probe" in rtext
    assert nexr.version() == 300  # additions only


def test_the_kernels_live_in_the_ll_object_and_use_no_scratch():
    from test_code_objects import PKG, _read, elf_tables, gfx950_code_objects
    path = os.path.join(PKG, "libnexr.so")
    if not os.path.exists(path):
        pytest.fail("libnexr.so not built")
    cos = gfx950_code_objects(_read(path))
    assert len(cos) == 11
    homes = []
    for co in cos:
        _t, notes = elf_tables(co)
        kernels = [k for nn in notes for k in nn["amdhsa.kernels"]]
        mine = [k for k in kernels if "sym_ll_" in k[".name"]]
        if mine:
            homes.append((mine, any("reduce_copy_ll_kernel" in k[".name"] for k in kernels)))
    assert len(homes) == 1
    mine, with_ll = homes[0]
    assert with_ll
    names = [k[".name"] for k in mine]
    assert sum("sym_ll_all_reduce_kernel" in x for x in names) == 3
    assert sum("sym_ll_reduce_scatter_kernel" in x for x in names) == 3
    assert sum("sym_ll_all_gather_kernel" in x for x in names) == 1
    for k in mine:
        assert k[".private_segment_fixed_size"] == 0, k[".name"]
