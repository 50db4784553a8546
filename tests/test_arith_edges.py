"""The oracle against tests/arith_edges.py's independent reference, bit for bit, on operand sets that reach
every arithmetic edge class: the 230-pattern edge set of each float format (all ordered pairs, triples and a
K = 8 fold), every float16 pattern against seven rotations, every ordered pair of bytes, the PreMulSum scalar
sweep and the SumPostDiv divisor x sign-flag sweep on all six integer types. Every layout runs at both pack
parities. This pins oracle/nexr_oracle.c from a second side."""
import numpy as np
import pytest

import arith_edges as ae

ALL_TYPES = sorted(ae.NAMES)


def first_diff(dt, got, exp, srcs=None):
    g, e = ae.canon(dt, got), ae.canon(dt, exp)
    assert g.shape == e.shape, (g.shape, e.shape)
    bad = np.nonzero(g != e)[0]
    if not bad.size:
        return None
    i = int(bad[0])
    ops = [hex(int(np.asarray(s).view(ae.UINT[dt])[i])) for s in srcs] if srcs is not None else None
    return dict(n_bad=int(bad.size), at=i, operands=ops, got=hex(int(g[i])), expected=hex(int(e[i])))


_ref_cache = {}


def reference(dt, lname, srcs, name, op, arg, ll=False):
    """The reference of one (layout, op), computed once per process."""
    key = (dt, lname, name, ll)
    if key not in _ref_cache:
        _ref_cache[key] = (ae.fold_ll if ll else ae.fold)(dt, op, arg, srcs)
    return _ref_cache[key]


def test_the_sets_are_what_the_module_says():
    for dt in ae.FLOATS:
        s = ae.edge_set(dt)
        assert s.size == 230 and np.unique(s).size == 230
        assert int(ae.is_nan(dt, s).sum()) == 8
        assert ae.pairs(s)[0].size == 52900 and ae.triples(s[::6])[0].size == 59319
        assert len(ae.fold8(s)) == 8
        assert len(ae.float_scalars(dt)) == 14 and len(set(ae.float_scalars(dt))) == 14
    a, b = ae.byte_pairs()
    assert np.unique(a.astype(np.uint32) << 8 | b).size == 65536
    # the value nearest 1/3, from numpy's own conversions
    assert ae.float_scalars(ae.F16)[5] == int(np.array([1 / 3]).astype(np.float16).view(np.uint16)[0])
    assert ae.float_scalars(ae.F32)[5] == int(np.array([1 / 3]).astype(np.float32).view(np.uint32)[0])
    assert ae.float_scalars(ae.F64)[5] == int(np.array([1 / 3]).view(np.uint64)[0])
    assert ae.float_scalars(ae.BF16)[5] == 0x3EAB
    # the parity rule: the same tuples, one element later
    ev, od = ae.both_parities([a, b])
    assert od[1][0].size == a.size + 1 and np.array_equal(od[1][0][1:], a) and np.array_equal(od[1][1][1:], b)


def test_reference_spot_values():
    """Hand-checked results of the reference itself."""
    def one(dt, op, is_max, c, v):
        u = ae.UINT[dt]
        return int(ae.step(dt, op, is_max, np.array([c], dtype=u), np.array([v], dtype=u))[0])
    assert one(ae.F16, ae.SUM, 0, 0x7BFF, 0x7BFF) == 0x7C00                  # overflow by rounding
    assert one(ae.F16, ae.SUM, 0, 0x7BFF, 0x4BFF) == 0x7BFF                  # 65504 + 15.99: below the tie
    assert one(ae.F16, ae.SUM, 0, 0x7BFF, 0x4C00) == 0x7C00                  # 65504 + 16: the tie goes to even = inf
    assert one(ae.F16, ae.PROD, 0, 0x0001, 0x3800) == 0x0000                 # 2^-24 / 2: tie to even 0
    assert one(ae.F16, ae.PROD, 0, 0x0003, 0x3800) == 0x0002                 # 1.5 ulp: tie to even 2
    assert one(ae.F16, ae.SUM, 0, 0x7C00, 0xFC00) == 0x7FFF                  # inf - inf
    assert one(ae.F16, ae.MINMAX, 0, 0x7E01, 0x3C00) == 0x7FFF               # a NaN accumulator stays, canonical
    assert one(ae.F16, ae.MINMAX, 0, 0x3C00, 0x7E01) == 0x3C00               # a NaN operand is dropped
    assert one(ae.F16, ae.MINMAX, 0, 0x0000, 0x8000) == 0x0000               # -0 < +0 is false: keeps c
    assert one(ae.F16, ae.MINMAX, 1, 0x8000, 0x0000) == 0x8000
    assert one(ae.BF16, ae.SUM, 0, 0x3F80, 0x3B80) == 0x3F80                 # 1 + 2^-8: tie to even
    assert one(ae.BF16, ae.SUM, 0, 0x3F81, 0x3B80) == 0x3F82                 # odd: tie goes up
    assert one(ae.BF16, ae.SUM, 0, 0x7F7F, 0x7F7F) == 0x7F80
    assert one(ae.F64, ae.SUM, 0, 0x7FEFFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF) == 0x7FF0000000000000
    assert one(ae.F64, ae.SUM, 0, 0xFFEFFFFFFFFFFFFF, 0xFC90000000000000) == 0xFFF0000000000000  # -max - ulp/2: tie to inf
    assert one(ae.F64, ae.SUM, 0, 0xFFEFFFFFFFFFFFFF, 0xFC8FFFFFFFFFFFFF) == 0xFFEFFFFFFFFFFFFF
    assert one(ae.F64, ae.PROD, 0, 0x0000000000000001, 0x3FE0000000000000) == 0   # smallest subnormal / 2: tie to 0
    assert one(ae.F64, ae.PROD, 0, 0x8000000000000003, 0x3FE0000000000000) == 0x8000000000000002
    assert one(ae.F64, ae.SUM, 0, 0x3FF0000000000000, 0xBFF0000000000000) == 0    # x - x = +0
    assert one(ae.F64, ae.SUM, 0, 0x8000000000000000, 0x8000000000000000) == 0x8000000000000000
    assert one(ae.I8, ae.MINMAX, 0, 0x80, 0x7F) == 0x80 and one(ae.U8, ae.MINMAX, 0, 0x80, 0x7F) == 0x7F
    assert one(ae.I8, ae.PROD, 0, 0x80, 0xFF) == 0x80 and one(ae.U8, ae.SUM, 0, 0xFF, 0x02) == 0x01
    assert ae.postdiv(8, 0x80, (255 << 1) | 1) == 0x80                       # -128 / -1 wraps
    assert ae.postdiv(8, 0xF9, (2 << 1) | 1) == 0xFD                         # -7 / 2 = -3, toward zero
    assert ae.postdiv(8, 0xF9, (2 << 1) | 0) == 0x7C                         # 249 / 2
    assert ae.postdiv(8, 0xF9, (256 << 1) | 0) == 0                          # unsigned by 256
    assert ae.postdiv(32, 0x80000000, (0xFFFFFFFF << 1) | 1) == 0x80000000   # MIN / -1 wraps
    assert ae.postdiv(64, (1 << 64) - 9, (0xFFFFFFFF << 1) | 1) == 0         # -9 / 4294967295 (not -1 at 64 bits)
    assert ae.postdiv(32, 7, 0) == 7                                         # divisor 0 means 1


@pytest.mark.parametrize("dt", ALL_TYPES)
def test_oracle_reduce_copy_matches_reference(oracle, dt):
    """Sum, Prod, Min, Max on every layout at both parities."""
    bad = []
    for lname, srcs in ae.layouts(dt):
        for name, op, is_max in ae.FOUR_OPS:
            arg = ae.op_arg(dt, op, is_max)
            exp = reference(dt, lname, srcs, name, op, arg)
            for tag, ss in ae.both_parities(srcs):
                e = exp if tag == "even" else ae.pad_front(dt, op, arg, srcs, exp)
                got = oracle.reduce_copy(ss, 1, dt, op, arg)[0]
                d = first_diff(dt, got, e, ss)
                if d:
                    bad.append((lname, name, tag, d))
    assert not bad, bad[:4]


def test_oracle_int8_minmax_under_fork_semantics_is_unsigned(oracle):
    srcs = ae.byte_pairs()
    with oracle.semantics(ae.FORK):
        for is_max in (0, 1):
            arg = ae.minmax_arg(ae.I8, is_max)
            exp = ae.fold(ae.I8, ae.MINMAX, arg, srcs, semantics=ae.FORK)
            assert np.array_equal(exp, ae.fold(ae.U8, ae.MINMAX, is_max, srcs))
            for tag, ss in ae.both_parities(srcs):
                e = exp if tag == "even" else ae.pad_front(ae.I8, ae.MINMAX, arg, srcs, exp, semantics=ae.FORK)
                assert first_diff(ae.I8, oracle.reduce_copy(ss, 1, ae.I8, ae.MINMAX, arg)[0], e, ss) is None


def premul_float_cases(dt):
    """(name, sources, pre): K = 1 (x * s) and K = 2 (x0 * s0 + x1 * s1) over S(T) for every scalar; the K = 2
    partner scalar walks the list at another stride, and float32 / float64 carry the fused-multiply-add
    witness in front."""
    s = ae.edge_set(dt)
    scal = ae.float_scalars(dt)
    x1 = np.roll(s, 29)
    for i, sc in enumerate(scal):
        yield f"k1_s{sc:#x}", [s], [sc]
        yield f"k2_s{sc:#x}", [s, x1], [sc, scal[(i * 5 + 3) % len(scal)]]
        yield f"k2_one_pre_s{sc:#x}", [s, x1], [sc]
    if dt in (ae.F32, ae.F64):
        x0, s0, w1, s1 = ae.fma_witness(dt)
        u = ae.UINT[dt]
        yield "fma_witness", [np.full(5, x0, dtype=u), np.full(5, w1, dtype=u)], [s0, s1]
        # ... and with the inexact product first, whichever product a contraction would fuse
        yield "fma_witness_swapped", [np.full(5, w1, dtype=u), np.full(5, x0, dtype=u)], [s1, s0]


def premul_int_cases(dt):
    if ae.BITS[dt] == 8:
        x = np.arange(256, dtype=np.uint16).astype(np.uint8)
        for sc in range(256):
            yield f"k1_s{sc}", [x], [sc]
        for sc in ae.int_scalars(dt):
            yield f"k2_s{sc}", ae.byte_pairs(), [sc, (sc * 7 + 3) & 0xFF]
    else:
        x = ae.int_edge_set(dt)
        for sc in ae.int_scalars(dt):
            yield f"k1_s{sc:#x}", [x], [sc]
            yield f"k2_s{sc:#x}", ae.pairs(x), [sc, 3]


def premul_cases(dt):
    return premul_int_cases(dt) if dt in ae.INTS else premul_float_cases(dt)


@pytest.mark.parametrize("dt", ALL_TYPES)
def test_oracle_premulsum_scalar_sweep(oracle, dt):
    bad = []
    for cname, srcs, pre in premul_cases(dt):
        exp = ae.fold(dt, ae.PREMULSUM, 0, srcs, pre, True)
        if cname.startswith("fma_witness"):
            assert not exp.any(), "the unfused sum is exactly +0"
        for tag, ss in ae.both_parities(srcs):
            e = exp if tag == "even" else ae.pad_front(dt, ae.PREMULSUM, 0, srcs, exp, pre, True)
            d = first_diff(dt, oracle.reduce_copy(ss, 1, dt, ae.PREMULSUM, 0, pre, True)[0], e, ss)
            if d:
                bad.append((cname, tag, d))
    assert not bad, bad[:4]


@pytest.mark.parametrize("dt", ae.INTS)
def test_oracle_sumpostdiv_divisor_sweep(oracle, dt):
    """Every divisor x sign flag, whatever the datatype's signedness. Left out: exactly what the API refuses."""
    valid, excluded = ae.postdiv_cases(dt)
    assert len(valid) + len(excluded) == 2 * len(ae.DIVISORS)
    want_excluded = [(d, 1) for d in ae.DIVISORS if (d or 1) & 0xFF == 0] if ae.BITS[dt] == 8 else []
    assert excluded == want_excluded
    assert (excluded == [(256, 1), (0x80000000, 1)]) if ae.BITS[dt] == 8 else not excluded
    x = np.zeros(4, dtype=ae.UINT[dt])
    for d, flag in excluded:
        with pytest.raises(ValueError):
            oracle.reduce_copy([x], 1, dt, ae.SUMPOSTDIV, (d << 1) | flag, post_op=True)
    bad = []
    for d, flag in valid:
        arg = (d << 1) | flag
        for k in (1, 2):
            srcs = ae.postdiv_sources(dt, d, k)
            exp = ae.fold(dt, ae.SUMPOSTDIV, arg, srcs, None, True)
            for tag, ss in ae.both_parities(srcs):
                e = exp if tag == "even" else ae.pad_front(dt, ae.SUMPOSTDIV, arg, srcs, exp, None, True)
                got = oracle.reduce_copy(ss, 1, dt, ae.SUMPOSTDIV, arg, None, True)[0]
                diff = first_diff(dt, got, e, ss)
                if diff:
                    bad.append((d, flag, k, tag, diff))
    assert not bad, bad[:4]


def test_sumpostdiv_validation_follows_the_sign_flag(oracle):
    """The signed quotient is chosen by bit 0 of redOpArg, not by the datatype: uint8 with the flag and divisor
    256 would divide by (int8)0 and is refused; int8 without it divides by 256 and is 0 everywhere."""
    x = np.arange(256, dtype=np.uint16).astype(np.uint8)
    with pytest.raises(ValueError):
        oracle.reduce_copy([x], 1, ae.U8, ae.SUMPOSTDIV, (256 << 1) | 1, post_op=True)
    got = oracle.reduce_copy([x], 1, ae.I8, ae.SUMPOSTDIV, (256 << 1) | 0, post_op=True)[0]
    exp = ae.fold(ae.I8, ae.SUMPOSTDIV, (256 << 1) | 0, [x], None, True)
    assert not exp.any() and np.array_equal(got.view(np.uint8), exp)
    for proto in ("ll", "ll128"):
        step = oracle.reduce_copy_ll if proto == "ll" else oracle.reduce_copy_ll128
        assert step(x, True, [], [], True, 0, [], 256, ae.U8, ae.SUMPOSTDIV, (256 << 1) | 1, True)[0] == 4
        rc, dst, _ = step(x, True, [], [], True, 0, [], 256, ae.I8, ae.SUMPOSTDIV, (256 << 1) | 0, True)
        assert rc == 0 and not dst.any()


# ---- the LL and LL128 steps: the peer is the first operand ----------------------------------------------
def ll_cases(dt):
    """(name, [user source, peers...]): recvReduceCopySend on the pair layout (peer, src) and twoPeers on the
    triples."""
    lay = dict(ae.layouts(dt))
    a, b = lay["pairs"]
    yield "pairs", [b, a]
    if "triples" in lay:
        t = lay["triples"]
        yield "triples", [t[2], t[0], t[1]]
    else:
        t = lay["fold3"]
        yield "fold3", [t[2], t[0], t[1]]
    if dt == ae.F16:
        for r in ae.F16_ROTATIONS:
            a, b = ae.f16_all_pairs(r)
            yield f"all_rot{r:#x}", [b, a]


def ll_ops(dt):
    for name, op, is_max in ae.FOUR_OPS:
        yield name, op, ae.op_arg(dt, op, is_max), False
    sc = ae.float_scalars(dt)[5] if dt in ae.FLOATS else 3
    yield "premulsum", ae.PREMULSUM, sc, False
    if dt in ae.INTS:
        yield "sumpostdiv_u", ae.SUMPOSTDIV, (3 << 1) | 0, True
        yield "sumpostdiv_s", ae.SUMPOSTDIV, (0xFFFFFFFE << 1) | 1, True


def run_oracle_ll(oracle, proto, dt, srcs, op, arg, post, flags=(77,)):
    """One step on the oracle: srcs[0] the user input, srcs[1:] the peers' wires; returns (dst, sends)."""
    n = srcs[0].size
    nrecv = len(srcs) - 1
    if proto == "ll":
        rflags = [300 + i for i in range(nrecv)]
        recv = [ae.ll_encode(srcs[1 + i], rflags[i]) for i in range(nrecv)]
        rc, dst, sends = oracle.reduce_copy_ll(srcs[0], True, recv, rflags, True, len(flags), list(flags), n, dt, op,
                                               arg, post)
    else:
        rflags = [500 + i for i in range(nrecv)]
        recv = [oracle.make_ll128_wire(srcs[1 + i], rflags[i], dt) for i in range(nrecv)]
        rc, dst, sends = oracle.reduce_copy_ll128(srcs[0], True, recv, rflags, True, len(flags), list(flags), n, dt,
                                                  op, arg, post)
    assert rc == 0
    return dst.view(ae.UINT[dt]), sends, recv, rflags


@pytest.mark.parametrize("proto", ["ll", "ll128"])
@pytest.mark.parametrize("dt", ALL_TYPES)
def test_oracle_ll_steps_match_reference(oracle, dt, proto):
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
                dst, sends, _, _ = run_oracle_ll(oracle, proto, dt, ss, op, arg, post)
                d = first_diff(dt, dst, e, ss)
                if d:
                    bad.append((lname, name, tag, "dst", d))
                nb = e.size * e.itemsize
                if proto == "ll":
                    data, flags = ae.ll_decode(sends[0], nb)
                    assert (flags == 77).all()
                else:  # the wire, read back by a receive-only step
                    rc, back, _ = oracle.reduce_copy_ll128(None, False, [sends[0]], [77], True, 0, [], e.size, dt,
                                                           ae.SUM, 0, False)
                    assert rc == 0
                    data = back
                d = first_diff(dt, data.view(ae.UINT[dt]), e, ss)
                if d:
                    bad.append((lname, name, tag, "wire", d))
    assert not bad, bad[:4]


# ---- a run of LL steps (oracle/ll_steps.py's interpreter) ------------------------------------------------
STEPS_TYPES = (ae.F16, ae.BF16, ae.F32, ae.I8)


def steps_slot_bytes(dt):
    """Slots that take the pair layout in at most 8 steps: 7 for the floats (8192 elements a step), 4 or 5 for int8."""
    return (1 << 16) if ae.BITS[dt] == 32 else (1 << 15)


def steps_cases(dt):
    """(name, tag, case, the reference's output): the pair layout (peer, src) at both parities, four ops."""
    import ll_steps_cases as cases
    a, b = dict(ae.layouts(dt))["pairs"]
    for name, op, is_max in ae.FOUR_OPS:
        arg = ae.op_arg(dt, op, is_max)
        key = (dt, "ll_pairs", name)
        if key not in _ref_cache:
            _ref_cache[key] = ae.fold_ll(dt, op, arg, [b, a])
        exp = _ref_cache[key]
        for tag, (src, peer) in ae.both_parities([b, a]):
            e = exp if tag == "even" else ae.pad_front(dt, op, arg, [b, a], exp, ll=True)
            yield name, tag, cases.edge_pairs_case(dt, op, arg, peer, src, steps_slot_bytes(dt)), e


@pytest.mark.parametrize("dt", STEPS_TYPES)
def test_ll_steps_interpreter_matches_reference(oracle, dt):
    import ll_steps_cases as cases
    from oracle import ll_steps
    for name, tag, case, exp in steps_cases(dt):
        assert 4 <= len(case.members[0].steps) <= cases.SLOTS
        members, conns = cases.model(case)
        res = ll_steps.run(members, case.dt, case.op, case.arg)
        out = res.members[0].output.view(ae.UINT[dt])
        assert first_diff(dt, out, exp) is None, (name, tag, first_diff(dt, out, exp))
        # the send connection's lines, step by step
        send, e = conns[1], exp.view(np.uint8)
        off = 0
        for k, st in enumerate(case.members[0].steps):
            nb = st.n_elts * exp.itemsize
            data, flags = ae.ll_decode(send.slot(send.start + k), nb)
            assert (flags == ll_steps.ll_flag(send.start + k)).all(), (name, tag, k)
            assert first_diff(dt, data.view(ae.UINT[dt]), e[off:off + nb].view(ae.UINT[dt])) is None, (name, tag, k)
            off += nb
        assert off == e.size


def test_the_builds_keep_floating_point_contraction_off():
    """The fused-multiply-add witness (premul_float_cases) fails only where the compiler does fuse. With the
    kernels as they are it fuses nothing with or without the flag (the pre-op's `s < nPreOp` select stands
    between the multiply and the add), so the flag and the pragma are pinned here as text too: both the
    kernels' and the oracle's build must round every multiply and add on its own."""
    import os
    import re
    from conftest import ROOT
    csrc = os.path.join(ROOT, "nex-nccl_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    common = re.search(r"^COMMON\s*=(.*)$", mk, re.M).group(1)
    assert "-ffp-contract=off" in common.split() and "$(COMMON)" in re.search(r"^KFLAGS\s*=(.*)$", mk, re.M).group(1)
    assert "-ffast-math" not in mk and "-Ofast" not in mk
    assert re.search(r"^#pragma clang fp contract\(off\)$", open(os.path.join(csrc, "nexr_types.hpp")).read(), re.M)
    omk = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    assert "-ffp-contract=off" in omk.split() and "-ffast-math" not in omk.split()
