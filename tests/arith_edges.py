"""TEST INFRASTRUCTURE (a helper, not a test module): operand sets that reach every arithmetic edge class
of the ten datatypes, and an independent reference of the reduction arithmetic to compare the oracle
(tests/test_arith_edges.py) and the kernels (tests/test_arith_edges_gpu.py) with.

numpy and the standard library only; it never imports the library under test or the oracle. Every buffer
is carried as the unsigned integer of the element's width (the bits are what count).

The reference computes one step op(c, v) in higher precision and rounds once:
  * float16, float32: widen to float64, apply the op, numpy's direct float64 -> T conversion (the float64
    sum / product of two halves is exact; for float32 it is innocuous double rounding, 53 >= 2*24 + 2);
  * bfloat16: the float32 result as above, then round-to-nearest-even in integer arithmetic on the f32 bits,
    (u + 0x7fff + ((u >> 16) & 1)) >> 16 (__float2bfloat16_rn, reduce_kernel.h:352-367);
  * float64: fractions.Fraction for finite non-zero results (overflow given its sign explicitly), IEEE
    rules for zero / inf / NaN operands;
  * min / max: v < c ? v : c and v > c ? v : c on the widened values, c the accumulator (a NaN on either
    side keeps c), reduce_kernel.h:455-478;
  * NaN results: 0x7fff for float16 / bfloat16 after every step (:329-367); float32 / float64 NaNs are
    compared by class (canon());
  * integers: Python ints wrapping at the type's width; min / max at the signedness asked for; SumPostDiv
    truncating toward zero with reduce_kernel.h:83-97's casts. The 8-bit types go through 256 x 256 tables
    filled by the same Python-int functions.
Folds: acc = pre(src0); acc = op(acc, pre(src_s)); post (common_kernel.h:141-237). The LL / LL128 steps
fold with the peer first: d = pre(src); d = op(peer_i, d) (prims_ll.h:251-258).
"""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np

I8, U8, I32, U32, I64, U64, F16, F32, F64, BF16 = range(10)
NAMES = {I8: "i8", U8: "u8", I32: "i32", U32: "u32", I64: "i64", U64: "u64", F16: "f16", F32: "f32", F64: "f64",
         BF16: "bf16"}
INTS = (I8, U8, I32, U32, I64, U64)
FLOATS = (F16, BF16, F32, F64)
SIGNED_INTS = (I8, I32, I64)
BITS = {I8: 8, U8: 8, I32: 32, U32: 32, I64: 64, U64: 64, F16: 16, F32: 32, F64: 64, BF16: 16}
UINT = {dt: np.dtype(f"u{b // 8}") for dt, b in BITS.items()}
FMT = {F16: (5, 10), BF16: (8, 7), F32: (8, 23), F64: (11, 52)}  # exponent bits, mantissa bits
SUM, PROD, MINMAX, PREMULSUM, SUMPOSTDIV = range(5)
NCCL, FORK = 0, 1  # semantics: min / max of a signed integer compare as signed (nccl) or unsigned (fork)

FOUR_OPS = (("sum", SUM, 0), ("prod", PROD, 0), ("min", MINMAX, 0), ("max", MINMAX, 1))


def minmax_arg(dt: int, is_max: bool) -> int:
    """hostToDevRedOp's xormask (enqueue.cc:2207-2216); only bit 0 (0 = min, 1 = max) reaches the arithmetic."""
    allb = (1 << BITS[dt]) - 1
    sign = allb ^ (allb >> 1)
    return (sign if dt in SIGNED_INTS else 0) ^ (allb if is_max else 0)


def op_arg(dt: int, op: int, is_max: int) -> int:
    return minmax_arg(dt, bool(is_max)) if op == MINMAX else 0


# ---- operand sets ---------------------------------------------------------------------------------------
def float_fields(dt: int):
    e_bits, m_bits = FMT[dt]
    emax, mmax = (1 << e_bits) - 1, (1 << m_bits) - 1
    b, h = emax // 2, mmax // 2
    exps = [0, 1, 2, b - m_bits - 1, b - 1, b, b + 1, b + m_bits, b + m_bits + 1, emax - 2, emax - 1]
    alt = int("01" * 32, 2) & mmax
    mants = [0, 1, 2, 3, h, h + 1, h + 2, mmax - 1, mmax, alt]
    nans = [1, h + 1, h + 2, mmax]
    return e_bits, m_bits, exps, mants, nans


def edge_set(dt: int) -> np.ndarray:
    """S(T): 2 signs x 11 exponent fields x 10 mantissas, +-inf, 4 NaN payloads under both signs = 230."""
    e_bits, m_bits, exps, mants, nans = float_fields(dt)
    emax = (1 << e_bits) - 1
    out = []
    for sign in (0, 1):
        s = sign << (e_bits + m_bits)
        out += [s | (e << m_bits) | m for e in exps for m in mants]
        out.append(s | (emax << m_bits))
        out += [s | (emax << m_bits) | m for m in nans]
    assert len(set(out)) == 230
    return np.array(out, dtype=np.uint64).astype(UINT[dt])


def int_edge_set(dt: int) -> np.ndarray:
    """32- and 64-bit integers: the values around 0, MIN, MAX and the type's top, and a few random ones."""
    bits = BITS[dt]
    mask, top = (1 << bits) - 1, 1 << (bits - 1)
    rnd = np.random.default_rng(bits).integers(0, 1 << 63, size=5, dtype=np.uint64)
    vals = [0, 1, 2, 3, mask, mask - 1, top, top + 1, top - 1, top - 2, 0x10001, 0xFFFF] + [int(r) & mask for r in rnd]
    return np.array(vals, dtype=np.uint64).astype(UINT[dt])


def pairs(s: np.ndarray) -> list:
    """All ordered pairs: (s[i], s[j]) at element i * len(s) + j."""
    return [np.repeat(s, s.size), np.tile(s, s.size)]


def triples(s: np.ndarray) -> list:
    n = s.size
    return [np.repeat(s, n * n), np.tile(np.repeat(s, n), n), np.tile(s, n * n)]


def fold8(s: np.ndarray) -> list:
    return [np.roll(s, (k * 29) % s.size).copy() for k in range(8)]


F16_ALL = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
F16_ROTATIONS = (1, 128, 255, 4099, 0x7C00, 0x8000, 0xFC01)


def f16_all_pairs(rot: int) -> list:
    return [F16_ALL.copy(), np.roll(F16_ALL, rot).copy()]


def byte_pairs() -> list:
    """All 65,536 ordered pairs of bytes."""
    return pairs(np.arange(256, dtype=np.uint16).astype(np.uint8))


def byte_fold(k: int) -> list:
    """K sources for the 8-bit types: the two vectors of byte_pairs(), then rotations of them."""
    a, b = byte_pairs()
    return [a, b] + [np.roll(b if s % 2 else a, 257 * s + 37).copy() for s in range(2, k)]


def float_layouts(dt: int) -> list:
    """(name, sources) of every layout of a float type, before the parity rule."""
    s = edge_set(dt)
    out = [("pairs", pairs(s)), ("triples", triples(s[::6])), ("fold8", fold8(s))]
    if dt == F16:
        out += [(f"all_rot{r:#x}", f16_all_pairs(r)) for r in F16_ROTATIONS]
    return out


def int_layouts(dt: int) -> list:
    if BITS[dt] == 8:
        return [("pairs", byte_pairs()), ("fold3", byte_fold(3)), ("fold8", byte_fold(8))]
    s = int_edge_set(dt)
    return [("pairs", pairs(s)), ("triples", triples(s[::2])), ("fold8", fold8(s))]


def layouts(dt: int) -> list:
    return int_layouts(dt) if dt in INTS else float_layouts(dt)


def both_parities(srcs: list) -> list:
    """The parity rule: (tag, sources) as they are and with one padding element in front, so that every
    operand tuple sits at an even and at an odd element position of a 16-byte pack."""
    return [("even", [np.ascontiguousarray(s) for s in srcs]),
            ("odd", [np.concatenate([s[-1:], s]) for s in srcs])]


def pad_front(dt: int, op: int, arg: int, srcs: list, exp: np.ndarray, pre=None, post=False, ll=False,
              semantics=NCCL) -> np.ndarray:
    """The expected output of the odd-parity layout from the even one's (the element in front is folded
    alone; everything after it is unchanged)."""
    head = (fold_ll if ll else fold)(dt, op, arg, [s[-1:] for s in srcs], pre, post, semantics=semantics)
    return np.concatenate([head, exp])


# ---- float arithmetic --------------------------------------------------------------------------------------
def is_nan(dt: int, bits: np.ndarray) -> np.ndarray:
    e_bits, m_bits = FMT[dt]
    inf = ((1 << e_bits) - 1) << m_bits
    return (bits.astype(np.uint64) & np.uint64((1 << (e_bits + m_bits)) - 1)) > np.uint64(inf)


def canon(dt: int, bits: np.ndarray) -> np.ndarray:
    """Bits for comparison: float32 / float64 NaNs by class, everything else exact."""
    bits = np.asarray(bits).view(UINT[dt])
    if dt in (F32, F64):
        e_bits, m_bits = FMT[dt]
        bits = bits.copy()
        bits[is_nan(dt, bits)] = (((1 << e_bits) - 1) << m_bits) | (1 << (m_bits - 1))
    return bits


def widen(dt: int, bits: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):  # widening a signalling NaN
        if dt == F16:
            return bits.view(np.float16).astype(np.float64)
        if dt == BF16:
            return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
        if dt == F32:
            return bits.view(np.float32).astype(np.float64)
        return bits.view(np.float64)


def narrow(dt: int, x: np.ndarray) -> np.ndarray:
    """float64 -> T with one rounding (two for bfloat16, as the reference), NaN -> 0x7fff for 16-bit types."""
    with np.errstate(all="ignore"):
        if dt == F16:
            r = x.astype(np.float16).view(np.uint16).copy()
            r[np.isnan(x)] = 0x7FFF
            return r
        f = x.astype(np.float32)
        if dt == F32:
            return f.view(np.uint32).copy()
        u = f.view(np.uint32).astype(np.uint64)
        r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
        r[np.isnan(x)] = 0x7FFF
        return r


_F64_SIGN, _F64_INF, _F64_NAN = 1 << 63, 0x7FF << 52, (0x7FF << 52) | (1 << 51)
_F64_OVER = Fraction(2 ** 1024 - 2 ** 970)  # the tie between the largest finite and 2^1024 rounds away
_f64_value_cache: dict = {}


def _f64_value(u: int) -> Fraction:
    v = _f64_value_cache.get(u)
    if v is None:
        e, m = (u >> 52) & 0x7FF, u & ((1 << 52) - 1)
        mag = Fraction(m) * Fraction(2) ** -1074 if e == 0 else Fraction(m | (1 << 52)) * Fraction(2) ** (e - 1075)
        v = _f64_value_cache[u] = -mag if u >> 63 else mag
    return v


def _f64_round(r: Fraction) -> int:
    sign = _F64_SIGN if r < 0 else 0
    mag = -r if r < 0 else r
    if mag >= _F64_OVER:
        return sign | _F64_INF
    try:
        f = float(mag)  # int / int true division: correctly rounded, subnormals included
    except OverflowError:
        return sign | _F64_INF
    return sign | struct.unpack("<Q", struct.pack("<d", f))[0]


def f64_arith(op: int, a: int, b: int) -> int:
    """a + b or a * b on float64 bit patterns, exactly rounded."""
    mag_a, mag_b = a & ~_F64_SIGN, b & ~_F64_SIGN
    if mag_a > _F64_INF or mag_b > _F64_INF:
        return _F64_NAN
    sa, sb = a >> 63, b >> 63
    if op == PROD:
        sign = (sa ^ sb) << 63
        if mag_a == _F64_INF or mag_b == _F64_INF:
            return _F64_NAN if (mag_a == 0 or mag_b == 0) else sign | _F64_INF
        if mag_a == 0 or mag_b == 0:
            return sign
        r = _f64_value(a) * _f64_value(b)
        bits = _f64_round(r)
        return bits
    if mag_a == _F64_INF or mag_b == _F64_INF:
        if mag_a == _F64_INF and mag_b == _F64_INF:
            return a if sa == sb else _F64_NAN
        return a if mag_a == _F64_INF else b
    if mag_a == 0 and mag_b == 0:
        return a if sa == sb else 0
    if mag_a == 0:
        return b
    if mag_b == 0:
        return a
    r = _f64_value(a) + _f64_value(b)
    return 0 if r == 0 else _f64_round(r)


def _f64_vec(op: int, c: np.ndarray, v: np.ndarray) -> np.ndarray:
    memo: dict = {}
    out = np.empty(c.size, dtype=np.uint64)
    for i, key in enumerate(zip(c.tolist(), v.tolist())):
        r = memo.get(key)
        if r is None:
            r = memo[key] = f64_arith(op, key[0], key[1])
        out[i] = r
    return out


def float_step(dt: int, op: int, is_max: bool, c: np.ndarray, v: np.ndarray) -> np.ndarray:
    """op(c, v), c the accumulator."""
    if op == MINMAX:
        wc, wv = widen(dt, c), widen(dt, v)
        with np.errstate(invalid="ignore"):
            r = np.where(wv > wc if is_max else wv < wc, v, c)
        if dt in (F16, BF16):  # ncclFromFloat of the chosen value: exact, except NaN -> 0x7fff
            r = r.copy()
            r[is_nan(dt, r)] = 0x7FFF
        return r
    if dt == F64:
        return _f64_vec(PROD if op == PROD else SUM, c, v)
    with np.errstate(all="ignore"):
        wc, wv = widen(dt, c), widen(dt, v)
        return narrow(dt, wc * wv if op == PROD else wc + wv)


# ---- integer arithmetic ------------------------------------------------------------------------------------
def to_signed(x: int, bits: int) -> int:
    return x - (1 << bits) if x >> (bits - 1) else x


def int_op(bits: int, op: int, is_max: bool, signed: bool, c: int, v: int) -> int:
    mask = (1 << bits) - 1
    if op == PROD:
        return (c * v) & mask
    if op == MINMAX:
        kc, kv = (to_signed(c, bits), to_signed(v, bits)) if signed else (c, v)
        return v if (kv > kc if is_max else kv < kc) else c
    return (c + v) & mask


def postdiv(bits: int, x: int, arg: int) -> int:
    """FuncSumPostDiv::divide (reduce_kernel.h:79-97): divisor = arg >> 1 as uint32 (0 -> 1), bit 0 selects the
    signed quotient, which divides by the divisor cast to the signed T and truncates toward zero."""
    mask = (1 << bits) - 1
    d = ((arg >> 1) & 0xFFFFFFFF) or 1
    if not arg & 1:
        return (x // d) & mask
    s, ds = to_signed(x, bits), to_signed(d & mask, bits)
    q = abs(s) // abs(ds)  # ds == 0 is postdiv_invalid()
    return (-q if (s < 0) != (ds < 0) else q) & mask


def postdiv_invalid(dt: int, divisor: int, signed_flag: int) -> bool:
    """The one class of SumPostDiv arguments the API refuses: the signed quotient of a 1-byte type by a
    divisor whose low byte is 0."""
    return BITS[dt] == 8 and signed_flag == 1 and ((divisor & 0xFFFFFFFF) or 1) & 0xFF == 0


_tables: dict = {}


def _table8(op: int, is_max: bool, signed: bool) -> np.ndarray:
    key = (op, is_max, signed)
    if key not in _tables:
        _tables[key] = np.array([[int_op(8, op, is_max, signed, c, v) for v in range(256)] for c in range(256)],
                                dtype=np.uint8)
    return _tables[key]


def _py_map(dt: int, fn, *arrs) -> np.ndarray:
    return np.array([fn(*t) for t in zip(*[a.tolist() for a in arrs])], dtype=np.uint64).astype(UINT[dt])


def int_step(dt: int, op: int, is_max: bool, c: np.ndarray, v: np.ndarray, semantics: int = NCCL) -> np.ndarray:
    signed = dt in SIGNED_INTS and semantics == NCCL
    op = op if op in (PROD, MINMAX) else SUM
    if BITS[dt] == 8:
        return _table8(op, bool(is_max), signed)[c, v]
    return _py_map(dt, lambda a, b: int_op(BITS[dt], op, is_max, signed, a, b), c, v)


# ---- folds -------------------------------------------------------------------------------------------------
def step(dt, op, is_max, c, v, semantics=NCCL):
    if dt in INTS:
        return int_step(dt, op, is_max, c, v, semantics)
    return float_step(dt, op, is_max, c, v)


def premul(dt: int, x: np.ndarray, raw: int) -> np.ndarray:
    """x * ncclDecodeScalar<T>(raw) (reduce_kernel.h:498-518)."""
    s = np.full(x.shape, raw & ((1 << BITS[dt]) - 1), dtype=np.uint64).astype(UINT[dt])
    return step(dt, PROD, False, x, s)


def _post(dt, acc, arg):
    if BITS[dt] == 8:
        return np.array([postdiv(8, x, arg) for x in range(256)], dtype=np.uint8)[acc]
    return _py_map(dt, lambda x: postdiv(BITS[dt], x, arg), acc)


def fold(dt: int, op: int, arg: int, srcs: list, pre=None, post: bool = False, semantics: int = NCCL) -> np.ndarray:
    """reduceCopy: acc = pre0(src0); acc = op(acc, pre_s(src_s)); post (common_kernel.h:141-237). A K = 1 copy
    keeps its bits."""
    pre = list(pre or [])
    is_max = bool(arg & 1)
    srcs = [np.ascontiguousarray(s).view(UINT[dt]) for s in srcs]
    acc = srcs[0].copy()
    if op == PREMULSUM and pre:
        acc = premul(dt, acc, pre[0])
    for s in range(1, len(srcs)):
        v = srcs[s]
        if op == PREMULSUM and s < len(pre):
            v = premul(dt, v, pre[s])
        acc = step(dt, op, is_max, acc, v, semantics)
    if op == SUMPOSTDIV and post:
        acc = _post(dt, acc, arg)
    return np.ascontiguousarray(acc)


def fold_ll(dt: int, op: int, arg: int, srcs: list, pre=None, post: bool = False, semantics: int = NCCL) -> np.ndarray:
    """One LL / LL128 step: srcs[0] is the user source, srcs[1:] the peers in connection order;
    d = pre(src); d = op(peer_i, d) (prims_ll.h:251-258). `pre` is [scalar] when the source is the user input
    of a PreMulSum."""
    is_max = bool(arg & 1)
    srcs = [np.ascontiguousarray(s).view(UINT[dt]) for s in srcs]
    d = srcs[0].copy()
    if op == PREMULSUM and pre:
        d = premul(dt, d, pre[0])
    for peer in srcs[1:]:
        d = step(dt, op, is_max, peer, d, semantics)
    if op == SUMPOSTDIV and post:
        d = _post(dt, d, arg)
    return np.ascontiguousarray(d)


# ---- LL lines (union ncclLLFifoLine: {data1, flag1, data2, flag2}) ------------------------------------------
def ll_encode(data: np.ndarray, flag: int) -> np.ndarray:
    raw = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    n_lines = (raw.size + 7) // 8
    padded = np.zeros(n_lines * 8, dtype=np.uint8)
    padded[:raw.size] = raw
    lines = np.full((n_lines, 4), flag, dtype=np.uint32)
    lines[:, 0::2] = padded.view(np.uint32).reshape(n_lines, 2)
    return lines.reshape(-1).view(np.uint8)


def ll_decode(lines: np.ndarray, n_bytes: int):
    """(the first n_bytes data bytes, the flags of the lines that carry them)."""
    n_lines = (n_bytes + 7) // 8
    w = np.ascontiguousarray(lines).view(np.uint8)[:n_lines * 16].view(np.uint32).reshape(n_lines, 4)
    return np.ascontiguousarray(w[:, 0::2]).reshape(-1).view(np.uint8)[:n_bytes].copy(), w[:, 1::2].copy()


# ---- scalar and divisor sweeps -----------------------------------------------------------------------------
def float_scalars(dt: int) -> list:
    """PreMulSum scalars (raw bits): +-0, +-1, 0.5, nearest 1/3, 1 + ulp, smallest / largest subnormal,
    smallest normal, largest finite, +-inf, a NaN."""
    e_bits, m_bits = FMT[dt]
    emax, mmax, b = (1 << e_bits) - 1, (1 << m_bits) - 1, ((1 << e_bits) - 1) // 2
    sign = 1 << (e_bits + m_bits)
    one = b << m_bits
    # 1/3 = 1.0101..b * 2^-2: an even mantissa width ends ..01 with a 0 next (round down), an odd one ends
    # ..10 with 101.. next (round up)
    third = ((b - 2) << m_bits) | ((int("01" * 32, 2) & mmax) if m_bits % 2 == 0 else (int("10" * 32, 2) & mmax) + 1)
    return [0, sign, one, sign | one, (b - 1) << m_bits, third, one + 1, 1, mmax, 1 << m_bits,
            ((emax - 1) << m_bits) | mmax, emax << m_bits, sign | (emax << m_bits), (emax << m_bits) | (mmax // 2 + 2)]


def int_scalars(dt: int) -> list:
    bits = BITS[dt]
    mask = (1 << bits) - 1
    return [0, 1, mask, 1 << (bits - 1), (1 << (bits - 1)) - 1, 3]


def fma_witness(dt: int):
    """(x0, s0, x1, s1) bit patterns, float32 / float64: x1 * s1 is inexact and x0 * s0 = -round(x1 * s1), so
    the unfused x0*s0 + x1*s1 is exactly 0 and a fused multiply-add returns the product's rounding error."""
    _, m_bits = FMT[dt]
    one = (((1 << FMT[dt][0]) - 1) // 2) << m_bits
    x1 = s1 = one + 1  # (1 + ulp)^2 = 1 + 2 ulp + ulp^2: the last term is lost
    p = int(float_step(dt, PROD, False, np.array([x1], dtype=UINT[dt]), np.array([s1], dtype=UINT[dt]))[0])
    assert p == one + 2
    return p | (1 << (BITS[dt] - 1)), one, x1, s1


DIVISORS = (0, 1, 2, 3, 7, 10, 127, 128, 129, 255, 256, 257, 0x7FFF, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE,
            0xFFFFFFFF)


def postdiv_inputs(dt: int, divisor: int) -> np.ndarray:
    bits = BITS[dt]
    if bits == 8:
        return np.arange(256, dtype=np.uint16).astype(np.uint8)
    mask, top, d = (1 << bits) - 1, 1 << (bits - 1), divisor
    rnd = np.random.default_rng(divisor & 0xFFFF).integers(0, 1 << 63, size=4, dtype=np.uint64)
    vals = [0, 1, -1, top, top + 1, top - 1, d, -d, d + 1, d - 1, -d + 1, -d - 1] + [int(r) * 2 + 1 for r in rnd]
    return np.array([v & mask for v in vals], dtype=np.uint64).astype(UINT[dt])


def postdiv_cases(dt: int):
    """(valid, excluded): every (divisor, signed flag) of the sweep for `dt`; `excluded` holds exactly the
    combinations postdiv_invalid() names."""
    valid, excluded = [], []
    for d in DIVISORS:
        for flag in (0, 1):
            (excluded if postdiv_invalid(dt, d, flag) else valid).append((d, flag))
    return valid, excluded


def postdiv_sources(dt: int, divisor: int, k: int) -> list:
    """K = 1: the inputs. K = 2: all ordered pairs of them, so that sums wrap before the divide."""
    x = postdiv_inputs(dt, divisor)
    return [x] if k == 1 else pairs(x)
