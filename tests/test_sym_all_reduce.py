"""The symmetric all-reduce (nexrSymAllReduce, nexrRingAllReduceSymmetric) without a GPU: the model the GPU
test compares with (tests/sym_cases.py) is checked against a second derivation of the ownership map and an
exact-arithmetic fold, the case table is shown to tell the owner-first fold from a rank-0-first one, and
every rejection of the two calls is shown to come before any device call (this machine has no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import sym_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ring(nexr):
    import importlib
    return importlib.import_module("nex-nccl_amd.ring")


# ---- the ownership map ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", sc.BLOCKS)
@pytest.mark.parametrize("n", sc.RANKS)
def test_owner_map_equals_the_walk_of_warps_and_threads(n, B):
    """Closed form == the walk over (rank, block, warp) numbers, for every geometry of the table, at 64
    threads per block and, from the first non-empty pass 1 on, at 512 too: the map does not depend on it."""
    seen = set()
    for dt in (sc.F32, sc.F16):
        esz = sc.ESZ[dt]
        for count, A, D, _ in sc.all_table_cases(n, B, dt):
            if (esz, count, A, D) in seen:
                continue
            seen.add((esz, count, A, D))
            owner, region = sc.owner_map(n, B, esz, count, A, D)
            dims = (64, 512) if count >= n * B * 8192 // esz - 1 else (64,)
            for block_dim in dims:
                o2, r2 = sc.owner_map_walk(n, B, esz, count, A, D, block_dim)
                assert np.array_equal(owner, o2) and np.array_equal(region, r2), (esz, count, A, D, block_dim)
    assert len(seen) > 100


def test_owner_map_regions_are_what_the_counts_promise():
    """The counts of the table bracket the passes: one element short of n*B*8192 bytes has no pass 1, that size
    has one (aligned, D = 0), D = 4 moves it all to pass 2, D = 2 (16-bit) leaves only ends, and the largest
    count has all three regions (the one before it, 2*n*B*8192/esz + 3*512/esz + 37, has pass 1 and ends)."""
    for dt in (sc.F32, sc.F16):
        esz = sc.ESZ[dt]
        for n in sc.RANKS:
            for B in sc.BLOCKS:
                full = n * B * 8192 // esz
                regs = lambda count, A, D: set(np.unique(sc.owner_map(n, B, esz, count, A, D)[1]).tolist())
                assert sc.PASS1 not in regs(full - 1, 0, 0)
                assert regs(full, 0, 0) == {sc.PASS1}
                assert regs(full, 0, 4) == {sc.PASS2}
                assert regs(n * B * 2048 // esz, 0, 4) == {sc.PASS2}
                assert regs(n * B * 2048 // esz - 1, 0, 4) == {sc.ENDS}
                assert regs(n * B * 512 // esz + 1, 0, 0) == {sc.ENDS}
                assert regs(sc.counts(n, B, esz)[-2], 0, 0) == {sc.PASS1, sc.ENDS}
                assert regs(sc.counts(n, B, esz)[-2], 0, 4) == {sc.PASS2, sc.ENDS}
                assert regs(sc.counts(n, B, esz)[-1], 0, 0) == {sc.PASS1, sc.PASS2, sc.ENDS}
                assert regs(sc.counts(n, B, esz)[-1], 4, 0) == {sc.PASS1, sc.PASS2, sc.ENDS}
                if esz == 2:
                    assert regs(sc.counts(n, B, esz)[-1], 0, 2) == {sc.ENDS}
                p = sc.plan(n, B, esz, sc.counts(n, B, esz)[-1], 4, 0)
                assert p["pre"] == 12 and p["p1_bytes"] % (n * B * 8192) == 0 and p["p2_bytes"] % (n * B * 2048) == 0


# ---- the fold ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sc.DTYPES, ids=[sc.NAMES[d] for d in sc.DTYPES])
@pytest.mark.parametrize("n", sc.RANKS)
def test_fold_is_pinned_by_exact_sums_with_one_rounding_per_step(n, dt):
    """expected() (numpy float32 adds, one conversion back) == fractions.Fraction sums rounded to float32 after
    every add and to T once at the end, for every owner: random values and the finite special columns."""
    rng = np.random.default_rng([n, dt])
    count = 96
    ins = [sc.random_values(dt, rng, count) for _ in range(n)]
    k = 0
    for col in sc.special_columns(dt, n):
        vals = [v for v in col if v is not None]
        finite = all((v & (sc._INF[dt] | 0)) != sc._INF[dt] for v in vals)
        if finite and k < count:
            for r, v in enumerate(col):
                if v is not None:
                    ins[r][k] = v
            k += 1
    assert k >= 6
    for o in range(n):
        owner = np.full(count, o, dtype=np.int32)
        got = sc.expected(dt, ins, owner)
        for i in range(count):
            vals = [int(x[i]) for x in ins]
            try:
                want = sc.fold_fraction(dt, vals, o)
            except OverflowError:
                continue
            assert int(got[i]) == want, (o, i, [hex(v) for v in vals], hex(int(got[i])), hex(want))


def test_round_fraction_agrees_with_numpy_on_every_float16():
    from fractions import Fraction
    for u in list(range(0, 0x7C00, 37)) + [1, 0x3FF, 0x400, 0x7BFF]:
        x = Fraction(float(np.uint16(u).view(np.float16)))
        assert sc.round_fraction(sc.F16, x) == u
        assert sc.to_fraction(sc.F16, u) == x
    # ties and overflow
    assert sc.round_fraction(sc.F16, Fraction(1) + Fraction(1, 2048)) == 0x3C00
    assert sc.round_fraction(sc.F16, Fraction(1) + Fraction(3, 2048)) == 0x3C02
    assert sc.round_fraction(sc.F16, Fraction(65520)) == 0x7C00 and sc.round_fraction(sc.F16, Fraction(65519)) == 0x7BFF
    assert sc.round_fraction(sc.F16, Fraction(1, 1 << 25)) == 0 and sc.round_fraction(sc.F16, Fraction(3, 1 << 25)) == 2


@pytest.mark.parametrize("dt", sc.DTYPES, ids=[sc.NAMES[d] for d in sc.DTYPES])
@pytest.mark.parametrize("B", sc.BLOCKS)
@pytest.mark.parametrize("n", sc.RANKS)
def test_table_tells_the_owner_first_fold_from_a_rank0_first_one(n, B, dt):
    """For n >= 3 the expected bytes of every table case differ from the rank-0-first fold in every region
    that has an element a rank other than 0 owns; for n = 2 the order is invisible."""
    esz = sc.ESZ[dt]
    for count, A, D, in_place in sc.all_table_cases(n, B, dt):
        owner, region = sc.owner_map(n, B, esz, count, A, D)
        ins = sc.make_inputs(dt, n, count, sc.case_seed(n, B, dt, count, A, D, in_place), owner, region)
        if dt == sc.F32:  # the float32 inputs stay inside what the rule pins (sym_cases docstring)
            w = np.stack([sc.widen(dt, x) for x in ins])
            assert (np.isnan(w).sum(axis=0) <= 1).all()
            assert not ((w == np.inf).any(axis=0) & (w == -np.inf).any(axis=0)).any()
        exp, r0 = sc.expected(dt, ins, owner), sc.rank0_first(dt, ins)
        if n == 2:
            assert np.array_equal(exp, r0)
            continue
        for reg in (sc.PASS1, sc.PASS2, sc.ENDS):
            m = region == reg
            if (m & (owner != 0)).any():
                assert (exp[m] != r0[m]).any(), (count, A, D, reg)
            elif m.any():
                assert np.array_equal(exp[m], r0[m])


def test_accumulating_in_float32_differs_from_rounding_every_step():
    for dt in (sc.F16, sc.BF16):
        for n, lo in ((3, 0.1), (5, 0.2), (8, 0.3)):
            owner, region = sc.owner_map(n, 1, 2, 20000, 0, 0)
            ins = [sc.random_values(dt, np.random.default_rng([n, dt, r]), 20000) for r in range(n)]
            frac = float((sc.expected(dt, ins, owner) != sc.per_step_rounding(dt, ins, owner)).mean())
            assert frac > lo, (dt, n, frac)


def test_rank_offsets_realise_a_and_d_and_differ_from_rank0():
    for esz in (2, 4):
        for A in sc.offsets_a(esz):
            for D in sc.offsets_d(esz):
                ins, outs = sc.rank_offsets(esz, 8, A, D, False)
                assert ins[0] == A and (ins[0] - outs[0]) % 16 == D
                assert all(o % esz == 0 for o in ins + outs)
                assert all(i != ins[0] for i in ins[1:]) and all(o != outs[0] for o in outs[1:])
            ins, outs = sc.rank_offsets(esz, 8, A, 0, True)
            assert ins == outs


# ---- rejections, before any device call -------------------------------------------------------------------------
def _call(nexr, n, ins, outs, count, dt, op=0, blocks=0):
    L = nexr.lib()
    a = (ctypes.c_void_p * max(1, len(ins)))(*ins) if ins is not None else None
    b = (ctypes.c_void_p * max(1, len(outs)))(*outs) if outs is not None else None
    return L.nexrSymAllReduce(n, a, b, count, dt, op, 0, blocks, None)


def test_sym_all_reduce_rejects_bad_arguments_before_any_device_call(nexr):
    ok, bad = int(nexr.Result.Success), int(nexr.Result.InvalidArgument)
    p = [0x10000 + 64 * i for i in range(130)]  # never dereferenced: every call below returns before a launch
    assert _call(nexr, 2, None, p[:2], 8, sc.F32) == bad
    assert _call(nexr, 2, p[:2], None, 8, sc.F32) == bad
    assert _call(nexr, 2, [p[0], None], p[2:4], 8, sc.F32) == bad
    assert _call(nexr, 2, p[:2], [None, p[3]], 8, sc.F32) == bad
    for n in (-1, 0, 1, 65):
        assert _call(nexr, n, p[:65], p[65:130], 8, sc.F32) == bad
    for blocks in (-1, 65, 1 << 20):
        assert _call(nexr, 2, p[:2], p[2:4], 8, sc.F32, blocks=blocks) == bad
    for dt in (0, 1, 2, 3, 4, 5, 8, 10, 11, 12, -1):
        assert _call(nexr, 2, p[:2], p[2:4], 8, dt) == bad
    for op in (1, 2, 3, 4, 5, -1):
        assert _call(nexr, 2, p[:2], p[2:4], 8, sc.F32, op=op) == bad
    assert _call(nexr, 2, [p[0], p[1] + 2], p[2:4], 8, sc.F32) == bad
    assert _call(nexr, 2, p[:2], [p[2] + 2, p[3]], 8, sc.F32) == bad
    for dt in (sc.F16, sc.BF16):
        assert _call(nexr, 3, [p[0], p[1], p[2] + 1], p[3:6], 8, dt) == bad
        assert _call(nexr, 3, p[:3], [p[3] + 3, p[4], p[5]], 8, dt) == bad
    # valid arguments and nothing to do: success, and no launch (there is no device to launch on here)
    for dt in sc.DTYPES:
        assert _call(nexr, 2, [p[0] + 2 * sc.ESZ[dt], p[1]], p[2:4], 0, dt) == ok
        assert _call(nexr, 64, p[:64], p[64:128], 0, dt, blocks=64) == ok
    with pytest.raises(nexr.NexrError) as e:
        nexr.sym_all_reduce(p[:1], p[1:2], 8, sc.F32)
    assert e.value.code == bad
    with pytest.raises(nexr.NexrError):
        nexr.sym_all_reduce(p[:2], p[2:5], 8, sc.F32)
    nexr.sym_all_reduce(p[:2], p[2:4], 0, sc.F32, n_blocks=3)


def test_ring_symmetric_rejections_on_a_host_memory_communicator(nexr, ring, oracle):
    """Arguments first (InvalidArgument), then the communicator's kind (InvalidUsage): host memory is not
    device memory. Nothing here reaches a device."""
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value
    bad, usage = int(nexr.Result.InvalidArgument), int(nexr.Result.InvalidUsage)
    bufs = [np.zeros(64, dtype=np.float32) for _ in range(4)]
    ptrs = [b.ctypes.data for b in bufs]
    L = ring.ring_lib()
    arr = lambda v: (ctypes.c_void_p * len(v))(*v)
    assert L.nexrRingAllReduceSymmetric(None, arr(ptrs[:2]), arr(ptrs[2:]), 8, sc.F32, 0, 0) == bad
    with ring.RingComm(2, ring.HOST_MEMORY, 1 << 14, fn, timeout_ms=20000) as comm:
        def code(send, recv, count, dt, op, blocks=0):
            with pytest.raises(nexr.NexrError) as e:
                comm.all_reduce_symmetric(send, recv, count, dt, op, blocks)
            return e.value.code
        for op in (1, 2, 3, 4):
            assert code(ptrs[:2], ptrs[2:], 8, sc.F32, op) == bad
        for dt in (0, 2, 4, 8, 10):
            assert code(ptrs[:2], ptrs[2:], 8, dt, 0) == bad
        for blocks in (-1, 65):
            assert code(ptrs[:2], ptrs[2:], 8, sc.F32, 0, blocks) == bad
        assert code([ptrs[0], 0], ptrs[2:], 8, sc.F32, 0) == bad
        assert L.nexrRingAllReduceSymmetric(comm._h, None, arr(ptrs[2:]), 8, sc.F32, 0, 0) == bad
        for dt in sc.DTYPES:
            assert code(ptrs[:2], ptrs[2:], 8, dt, 0) == usage
            assert code(ptrs[:2], ptrs[2:], 0, dt, 0) == usage
        assert comm.queued() == 0
        assert all((b == 0).all() for b in bufs)
        # the communicator still works
        for b in bufs[:2]:
            b[:] = 1.0
        comm.all_reduce(ptrs[:2], ptrs[2:], 64, sc.F32, 0)
        assert (bufs[2] == 2.0).all() and (bufs[3] == 2.0).all()
    with ring.RingComm(1, ring.HOST_MEMORY, 1 << 14, fn) as one:
        with pytest.raises(nexr.NexrError) as e:
            one.all_reduce_symmetric(ptrs[:1], ptrs[2:3], 8, sc.F32, 0)
        assert e.value.code == usage


# ---- the public surface ------------------------------------------------------------------------------------------
def test_headers_carry_the_rule_and_the_symbols(nexr, ring):
    with open(os.path.join(ROOT, "include", "nexr.h")) as f:
        hdr = f.read()
    with open(os.path.join(ROOT, "include", "nexr_ring.h")) as f:
        rhdr = f.read()
    assert re.search(r"NEXR_API\s+nexrResult_t\s+nexrSymAllReduce\s*\(", hdr)
    assert re.search(r"#define\s+NEXR_SYM_MAX_RANKS\s+64\b", hdr)
    assert "nexrSymAllReduce" in nexr.ABI_SYMBOLS and hasattr(nexr.lib(), "nexrSymAllReduce")
    assert nexr.SYM_MAX_RANKS == 64
    text = " ".join(hdr.split()).replace(" * ", " ")
    for sentence in ("symmetric/all_reduce.hh:6-276", "piece i owned by rank i mod n",
                     "element e is owned by rank floor(e / 32) mod n", "B fixes only the pass boundaries",
                     "all_reduce.hh:269-275", "both are the stream's order", "ncclSymAccumType",
                     "every NaN to 0x7fff", "A = inputs[0] mod 16", "D = (inputs[0] - outputs[0]) mod 16",
                     "c1 -= c1 mod (n B)", "c2 -= c2 mod (n B)", "ReduceScatter_LD / AllGather_ST are not built",
                     "nElts == 0 succeeds without a launch"):
        assert sentence in text, sentence
    assert re.search(r"NEXR_API\s+nexrResult_t\s+nexrRingAllReduceSymmetric\s*\(", rhdr)
    assert "nexrRingAllReduceSymmetric" in ring.RING_ABI_SYMBOLS
    assert hasattr(ring.ring_lib(), "nexrRingAllReduceSymmetric")
    rtext = " ".join(rhdr.split()).replace(" * ", " ")
    for sentence in ("it leaves nexrRingCommGetQueued as it was", "touches no connection and no step counter",
                     "anything else is nexrInvalidUsage", "sym_all_reduce_probe"):
        assert sentence in rtext, sentence
    assert nexr.version() == 300  # additions only


def test_the_kernel_lives_in_the_ll_object_and_the_makefile_knows_it():
    with open(os.path.join(ROOT, "nex-nccl_amd", "csrc", "Makefile")) as f:
        mk = f.read()
    rule = [l for l in mk.splitlines() if l.startswith("$(BUILD)/nexr_ll.o:")]
    assert rule and "nexr_sym.hip" in rule[0] and "nexr_simple.hip" in rule[0]
    with open(os.path.join(ROOT, "nex-nccl_amd", "csrc", "nexr_ll.hip")) as f:
        assert '#include "nexr_sym.hip"' in f.read()
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
        sym = [x for x in names if "sym_all_reduce_kernel" in x]
        if sym:
            homes.append((sym, any("reduce_copy_ll_kernel" in x for x in names)))
    assert len(homes) == 1 and len(homes[0][0]) == 3 and homes[0][1]
