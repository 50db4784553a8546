"""TEST INFRASTRUCTURE (a helper, not a test module): an independent numpy restatement of the symmetric
all-reduce RSxLD_AGxST (include/nexr.h, nexrSymAllReduce; reference src/device/symmetric/all_reduce.hh:6-276)
and the case table its CPU and GPU tests share.

numpy and the standard library only; it never imports the library under test. Buffers are carried as the
unsigned integer of the element's width.

  * owner_map: which rank owns which element, in closed form from (n, B, esz, nElts, A, D);
  * owner_map_walk: the same map derived a second way, by walking the reference's global warp and thread
    numbers (warps ordered by rank, then block, then warp within the block; strides of the total warp and
    thread count), for any block size;
  * expected: acc = in[o]; acc = acc + in[(o + j) % n] in float32 (numpy float32 adds), one conversion back:
    astype(float16) for fp16, the integer round-to-nearest-even of tests/arith_edges.py for bf16, every NaN
    of a 16-bit type 0x7fff;
  * fold_fraction: the same fold with fractions.Fraction sums and one exact rounding per step;
  * make_inputs / table_cases: the inputs (random values with exponents spread over +-6, special values,
    fold-order witnesses) and the (count, A, D, in place) list of every (n, B, datatype) of the table.

float32 NaNs. The rule gives a float32 NaN no bits of its own (only fp16 / bf16 results are canonicalised), so
the float32 inputs carry at most ONE NaN per element and no infinities of opposite sign: the result is then
that NaN with its quiet bit set, payload kept, on every IEEE implementation (add32 writes exactly that, whatever
the host's adder does), while inf - inf would have an implementation-chosen sign. The 16-bit types carry both.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

F16, F32, BF16 = 6, 7, 9  # nexrFloat16, nexrFloat32, nexrBfloat16
DTYPES = (F32, F16, BF16)
NAMES = {F16: "f16", F32: "f32", BF16: "bf16"}
ESZ = {F16: 2, F32: 4, BF16: 2}
UINT = {F16: np.dtype(np.uint16), F32: np.dtype(np.uint32), BF16: np.dtype(np.uint16)}
FMT = {F16: (5, 10), F32: (8, 23), BF16: (8, 7)}  # exponent bits, mantissa bits
RANKS = (2, 3, 5, 8)
BLOCKS = (1, 2, 3)
PASS1, PASS2, ENDS = 1, 2, 3


# ---- geometry ------------------------------------------------------------------------------------------------
def plan(n: int, B: int, esz: int, n_elts: int, A: int, D: int) -> dict:
    """The pass boundaries in bytes (all_reduce.hh:203-251). A = inputs[0] mod 16, D = (inputs[0] - outputs[0])
    mod 16."""
    n_bytes = n_elts * esz
    pre = min((16 - A) % 16, n_bytes)
    cursor = pre
    c1 = 0
    if D % 16 == 0:
        c1 = (n_bytes - cursor) // 8192
        c1 -= c1 % (n * B)
    p1_off, p1_bytes = cursor, c1 * 8192
    cursor += p1_bytes
    c2 = 0
    if esz == 4 or D % 4 == 0:
        c2 = (n_bytes - cursor) // 2048
        c2 -= c2 % (n * B)
    p2_off, p2_bytes = cursor, c2 * 2048
    cursor += p2_bytes
    return dict(pre=pre, p1_off=p1_off, p1_bytes=p1_bytes, p2_off=p2_off, p2_bytes=p2_bytes, suf_off=cursor,
                pre_elts=pre // esz, n_ends=pre // esz + (n_bytes - cursor) // esz)


def owner_map(n: int, B: int, esz: int, n_elts: int, A: int, D: int):
    """(owner, region) per element, closed form: 2048-byte pieces of pass 1 and 512-byte pieces of pass 2 go
    round the ranks, end element e belongs to rank (e // 32) % n."""
    p = plan(n, B, esz, n_elts, A, D)
    idx = np.arange(n_elts, dtype=np.int64)
    byte = idx * esz
    in1 = (byte >= p["p1_off"]) & (byte < p["p1_off"] + p["p1_bytes"])
    in2 = (byte >= p["p2_off"]) & (byte < p["p2_off"] + p["p2_bytes"])
    e = np.where(byte < p["pre"], idx, p["pre_elts"] + (byte - p["suf_off"]) // esz)
    owner = np.where(in1, (byte - p["p1_off"]) // 2048 % n, np.where(in2, (byte - p["p2_off"]) // 512 % n, e // 32 % n))
    region = np.where(in1, PASS1, np.where(in2, PASS2, ENDS))
    return owner.astype(np.int32), region.astype(np.int8)


def owner_map_walk(n: int, B: int, esz: int, n_elts: int, A: int, D: int, block_dim: int):
    """The second derivation. Every rank runs B blocks of block_dim threads, warps of 32. Global warp number:
    rank fastest, then block, then warp within the block (all_reduce.hh:262-267); wn warps and tn threads in
    all. In a pass a warp's iteration is 4 packs x 32 lanes of 16 (pass 1) or 4 (pass 2) bytes, warp g runs
    iterations g, g + wn, ... of the chunks * 4 there are (:15-25, :106-109), a chunk being 4 iterations
    whatever block_dim is (:211-216). In the ends thread t takes elements t, t + tn, ... (:134-135). Returns
    (owner, region) per element; every byte must be taken exactly once."""
    assert block_dim % 32 == 0
    wpb = block_dim // 32
    wn = n * B * wpb
    tn = wn * 32
    n_bytes = n_elts * esz
    owner_b = np.full(n_bytes, -1, dtype=np.int32)
    region_b = np.zeros(n_bytes, dtype=np.int8)
    taken = np.zeros(n_bytes, dtype=np.int32)
    pre = min((16 - A) % 16, n_bytes)
    cursor = pre
    lanes = np.arange(32, dtype=np.int64)
    passes = []
    if D % 16 == 0:
        passes.append((PASS1, 16))
    if esz == 4 or D % 4 == 0:
        passes.append((PASS2, 4))
    for tag, pack in passes:
        chunk = 4 * 4 * 32 * pack  # MinWarpPerBlock x UnrollPacks x WARP_SIZE x BytePerPack
        chunks = (n_bytes - cursor) // chunk
        chunks -= chunks % (n * B)
        iters = chunks * 4
        for rank in range(n):
            for block in range(B):
                for w in range(wpb):
                    g = rank + n * (block + B * w)
                    for it in range(g, iters, wn):
                        for u in range(4):  # lane l's pack: bytes [lo + l * pack, lo + (l + 1) * pack)
                            lo = cursor + it * (4 * 32 * pack) + u * 32 * pack
                            owner_b[lo:lo + 32 * pack] = rank
                            region_b[lo:lo + 32 * pack] = tag
                            taken[lo:lo + 32 * pack] += 1
        cursor += chunks * chunk
    n_pre, n_suf = pre // esz, (n_bytes - cursor) // esz
    for rank in range(n):
        for block in range(B):
            for w in range(wpb):
                g = rank + n * (block + B * w)
                i = (np.arange(32 * g, n_pre + n_suf, tn, dtype=np.int64)[:, None] + lanes[None, :]).reshape(-1)
                i = i[i < n_pre + n_suf]
                elt = np.where(i < n_pre, i, n_elts - n_suf - n_pre + i)
                for b in range(esz):
                    owner_b[elt * esz + b] = rank
                    region_b[elt * esz + b] = ENDS
                    taken[elt * esz + b] += 1
    assert n_bytes == 0 or (taken.min() == 1 and taken.max() == 1), "a byte is taken once, by one rank"
    ob, rb = owner_b.reshape(n_elts, esz), region_b.reshape(n_elts, esz)
    assert (ob == ob[:, :1]).all() and (rb == rb[:, :1]).all()
    return ob[:, 0].copy(), rb[:, 0].copy()


# ---- arithmetic ----------------------------------------------------------------------------------------------
def widen(dt: int, bits: np.ndarray) -> np.ndarray:
    bits = np.ascontiguousarray(bits).view(UINT[dt])
    with np.errstate(invalid="ignore"):
        if dt == F16:
            return bits.view(np.float16).astype(np.float32)
        if dt == BF16:
            return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
        return bits.view(np.float32).copy()


def add32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a + b in float32, a the accumulator. A NaN operand comes out quiet with its payload (a's before b's)."""
    with np.errstate(all="ignore"):
        r = (a + b).astype(np.float32)
    ru, au, bu = r.view(np.uint32), a.view(np.uint32), b.view(np.uint32)
    nb, na = np.isnan(b), np.isnan(a)
    ru[nb] = bu[nb] | np.uint32(0x00400000)
    ru[na] = au[na] | np.uint32(0x00400000)
    return r


def narrow(dt: int, f: np.ndarray) -> np.ndarray:
    """float32 -> T, one round-to-nearest-even; NaN -> 0x7fff for the 16-bit types."""
    f = np.ascontiguousarray(f, dtype=np.float32)
    if dt == F32:
        return f.view(np.uint32).copy()
    with np.errstate(all="ignore"):
        if dt == F16:
            r = f.astype(np.float16).view(np.uint16).copy()
        else:
            u = f.view(np.uint32).astype(np.uint64)
            r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    r[np.isnan(f)] = 0x7FFF
    return r


def fold_from(dt: int, inputs: list, start: int) -> np.ndarray:
    """acc = in[start]; acc = acc + in[(start + j) % n], j = 1..n-1, in float32; one conversion back."""
    n = len(inputs)
    acc = widen(dt, inputs[start])
    for j in range(1, n):
        acc = add32(acc, widen(dt, inputs[(start + j) % n]))
    return narrow(dt, acc)


def expected(dt: int, inputs: list, owner: np.ndarray) -> np.ndarray:
    """Every element folded from its owner on: operand j of element i is input (owner[i] + j) % n."""
    n = len(inputs)
    x = np.stack([np.ascontiguousarray(v).view(UINT[dt]) for v in inputs])
    cols = np.arange(owner.size)
    acc = widen(dt, x[owner, cols])
    for j in range(1, n):
        acc = add32(acc, widen(dt, x[(owner + j) % n, cols]))
    return narrow(dt, acc)


def expected_shipped(dt: int, inputs: list, owner: np.ndarray) -> np.ndarray:
    """Every add returns its first operand: the owner's input through the two casts."""
    out = np.empty(owner.size, dtype=UINT[dt])
    for o in range(len(inputs)):
        m = owner == o
        out[m] = narrow(dt, widen(dt, np.ascontiguousarray(inputs[o]).view(UINT[dt])[m]))
    return out


def rank0_first(dt: int, inputs: list) -> np.ndarray:
    """The fold the ring-style entry points would give with fp32 accumulation: rank 0 first for every element."""
    return fold_from(dt, [np.ascontiguousarray(x).view(UINT[dt]) for x in inputs], 0)


def per_step_rounding(dt: int, inputs: list, owner: np.ndarray) -> np.ndarray:
    """Owner first, but rounded to T after every add (what a fold in T would give)."""
    out = np.empty(owner.size, dtype=UINT[dt])
    n = len(inputs)
    for o in range(n):
        m = owner == o
        acc = np.ascontiguousarray(inputs[o]).view(UINT[dt])[m]
        for j in range(1, n):
            acc = narrow(dt, add32(widen(dt, acc), widen(dt, np.ascontiguousarray(inputs[(o + j) % n]).view(UINT[dt])[m])))
        out[m] = acc
    return out


# ---- exact arithmetic (fold pinning) ----------------------------------------------------------------------------
def to_fraction(dt: int, u: int) -> Fraction:
    e_bits, m_bits = FMT[dt]
    bias = (1 << (e_bits - 1)) - 1
    sign = -1 if u >> (e_bits + m_bits) else 1
    e, m = (u >> m_bits) & ((1 << e_bits) - 1), u & ((1 << m_bits) - 1)
    assert e != (1 << e_bits) - 1, "finite values only"
    mag = Fraction(m, 1 << m_bits) * Fraction(2) ** (1 - bias) if e == 0 else \
        (1 + Fraction(m, 1 << m_bits)) * Fraction(2) ** (e - bias)
    return sign * mag


def round_fraction(dt: int, x: Fraction, neg_zero: bool = False) -> int:
    """The bits of x rounded to nearest, ties to even, in dt's format (subnormals, overflow to infinity)."""
    e_bits, m_bits = FMT[dt]
    bias = (1 << (e_bits - 1)) - 1
    sign = (1 << (e_bits + m_bits)) if (x < 0 or (x == 0 and neg_zero)) else 0
    mag = -x if x < 0 else x
    if mag == 0:
        return sign
    e = mag.numerator.bit_length() - mag.denominator.bit_length()
    if Fraction(2) ** e > mag:
        e -= 1
    e = max(e, 1 - bias)  # the exponent of the spacing: subnormals share the smallest one
    q = mag / Fraction(2) ** (e - m_bits)  # in units of the last place
    k, rem = divmod(q.numerator, q.denominator)
    if 2 * rem > q.denominator or (2 * rem == q.denominator and k & 1):
        k += 1
    # k in [0, 2^(m_bits + 1)]: k == 2^(m_bits+1) carries into the next exponent, which the sum below does too
    bits = ((e + bias - 1) << m_bits) + k if k >= (1 << m_bits) or e > 1 - bias else k
    inf = ((1 << e_bits) - 1) << m_bits
    return sign | min(bits, inf)


def fold_fraction(dt: int, values: list, start: int) -> int:
    """One element: the owner-first fold with exact sums, one rounding to float32 per add, one to T at the end.
    Finite inputs; a zero sum takes IEEE's sign (+0 unless both operands are -0)."""
    n = len(values)
    acc_bits = round_fraction(F32, to_fraction(dt, values[start]), neg_zero=bool(values[start] >> (8 * ESZ[dt] - 1)))
    for j in range(1, n):
        v = values[(start + j) % n]
        v_neg = bool(v >> (8 * ESZ[dt] - 1))
        s = to_fraction(F32, acc_bits) + to_fraction(dt, v)
        acc_bits = round_fraction(F32, s, neg_zero=bool(acc_bits >> 31) and v_neg)
        if acc_bits & 0x7FFFFFFF == 0x7F800000:
            raise OverflowError("the pinned fold stays finite")
    return round_fraction(dt, to_fraction(F32, acc_bits), neg_zero=bool(acc_bits >> 31))


# ---- inputs ----------------------------------------------------------------------------------------------------
def from_float(dt: int, x: float) -> int:
    """Bits of a value that dt represents exactly."""
    f = np.float32(x)
    assert float(f) == x
    if dt == F32:
        return int(f.view(np.uint32))
    if dt == F16:
        h = np.float16(x)
        assert float(h) == x
        return int(h.view(np.uint16))
    u = int(f.view(np.uint32))
    assert u & 0xFFFF == 0
    return u >> 16


def random_values(dt: int, rng, size: int) -> np.ndarray:
    """Finite values, random sign and mantissa, exponents spread over +-6 around 1."""
    e_bits, m_bits = FMT[dt]
    bias = (1 << (e_bits - 1)) - 1
    sign = rng.integers(0, 2, size=size, dtype=np.uint64) << np.uint64(e_bits + m_bits)
    exp = rng.integers(bias - 6, bias + 7, size=size, dtype=np.uint64) << np.uint64(m_bits)
    man = rng.integers(0, 1 << m_bits, size=size, dtype=np.uint64)
    return (sign | exp | man).astype(UINT[dt])


_QNAN = {F32: 0x7FC12345, F16: 0x7E55, BF16: 0x7FD5}
_SNAN = {F32: 0xFF812345, F16: 0xFD55, BF16: 0xFF95}
_INF = {F32: 0x7F800000, F16: 0x7C00, BF16: 0x7F80}
_MAXF = {F32: 0x7F7FFFFF, F16: 0x7BFF, BF16: 0x7F7F}
_HALF_ULP = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}  # half a unit in the last place of 1.0
# fold-order witness: big at the owner, -big at the next rank, small elsewhere; small vanishes beside big in fp32
_WITNESS = {F32: (2.0 ** 30, 1.0), F16: (2.0 ** 15, 2.0 ** -14), BF16: (2.0 ** 30, 1.0)}


def special_columns(dt: int, n: int) -> list:
    """Per-rank values of special elements; None keeps the rank's random value."""
    sign = 1 << (8 * ESZ[dt] - 1)
    one, hu = from_float(dt, 1.0), from_float(dt, _HALF_ULP[dt])
    cols = []
    for k in range(n):
        cols.append([_QNAN[dt] if r == k else None for r in range(n)])  # one NaN with a payload, at every rank
    cols.append([_SNAN[dt] if r == n - 1 else None for r in range(n)])
    cols.append([_INF[dt] if r == 0 else None for r in range(n)])
    if dt == F32:  # same-sign infinities only (module docstring)
        cols.append([_INF[dt] | sign if r < 2 else None for r in range(n)])
    else:
        cols.append([_INF[dt] if r == 1 else (_INF[dt] | sign if r == 0 else None) for r in range(n)])
        cols.append([_QNAN[dt] if r % 2 else _SNAN[dt] for r in range(n)])
    cols.append([sign] * n)                                   # -0 everywhere: the sum is -0
    cols.append([0 if r == 0 else sign for r in range(n)])    # a +0 among them: +0
    cols.append([one if r == 0 else hu if r == 1 else 0 for r in range(n)])          # tie, rounds down to even
    cols.append([one + 1 if r == 0 else hu if r == 1 else sign for r in range(n)])   # tie, rounds up to even
    cols.append([hu if r == 0 else one if r == n - 1 else 0 for r in range(n)])
    cols.append([_MAXF[dt] if r < 2 else (_MAXF[dt] | sign if r == 2 else 0) for r in range(n)])  # beyond T's range
    if dt == F32:  # denormals are kept
        cols.append([1 if r == 0 else 3 if r == 1 else sign | 1 for r in range(n)])
        cols.append([0x00800000 if r == 0 else sign | 0x007FFFFF if r == 1 else 0 for r in range(n)])
    else:          # sums that are subnormal in T, and float32 sums T cannot hold exactly
        cols.append([1 if r == 0 else 3 if r == 1 else sign | 1 for r in range(n)])
        cols.append([one if r == 0 else from_float(dt, _HALF_ULP[dt] / 2) if r in (1, 2) else 0 for r in range(n)])
    return cols


def make_inputs(dt: int, n: int, n_elts: int, seed, owner: np.ndarray, region: np.ndarray) -> list:
    """n input vectors: random values, the special columns at elements 3, 10, 17, ... (as far as they fit),
    and fold-order witnesses at up to three elements of every region that a rank other than 0 owns."""
    rng = np.random.default_rng(seed)
    ins = [random_values(dt, rng, n_elts) for _ in range(n)]
    for k, col in enumerate(special_columns(dt, n)):
        pos = 3 + 7 * k
        if pos >= n_elts:
            break
        for r, v in enumerate(col):
            if v is not None:
                ins[r][pos] = v
    big, small = (from_float(dt, x) for x in _WITNESS[dt])
    sign = 1 << (8 * ESZ[dt] - 1)
    for reg in (PASS1, PASS2, ENDS):
        cand = np.flatnonzero((region == reg) & (owner != 0))
        for pos in sorted({int(cand[i]) for i in (0, cand.size // 2, cand.size - 1)} if cand.size else ()):
            o = int(owner[pos])
            for r in range(n):
                ins[r][pos] = big if r == o else (big | sign) if r == (o + 1) % n else small
    return ins


# ---- the case table ----------------------------------------------------------------------------------------------
def counts(n: int, B: int, esz: int) -> list:
    c = [1, 31, 32, 33, 32 * n - 1, 32 * n + 1,
         n * B * 512 // esz - 1, n * B * 512 // esz + 1,
         # pass 2 takes whole 2048-byte chunks, n * B of them at least: its first non-empty size
         n * B * 2048 // esz - 1, n * B * 2048 // esz, n * B * 2048 // esz + 1,
         n * B * 8192 // esz - 1, n * B * 8192 // esz, n * B * 8192 // esz + 1,
         2 * n * B * 8192 // esz + 3 * 512 // esz + 37,
         # all three regions at D = 0: pass 2 needs n * B whole 2048-byte chunks behind pass 1 (the count above
         # leaves it 3 * 512 bytes and 37 elements: pass 1 and ends, or pass 2 and ends when D is 4 or 8)
         2 * n * B * 8192 // esz + 3 * n * B * 2048 // esz + 37]
    return sorted(set(c))


def offsets_a(esz: int) -> list:
    return [0, 4, 8, 12] + ([2] if esz == 2 else [])


def offsets_d(esz: int) -> list:
    return [0, 4, 8] + ([2] if esz == 2 else [])


GROUPS = ("small", "passes", "cross")


def table_cases(n: int, B: int, dt: int, group: str) -> list:
    """(count, A, D, in_place) of one (n, B, datatype), in three groups that together are the table: every
    count under every D out of place and once in place, A going round its values ("small": the counts below
    the first non-empty pass 1, "passes": from there on), and the count with all three regions under every
    (A, D) ("cross")."""
    esz = ESZ[dt]
    a_s, d_s = offsets_a(esz), offsets_d(esz)
    cs = counts(n, B, esz)
    if group == "cross":
        return [(cs[-1], a, d, False) for a in a_s for d in d_s]
    cases, k = [], 0
    for count in cs:
        for d in d_s + [None]:  # None: in place (D = 0)
            if (count >= n * B * 8192 // esz - 1) == (group == "passes"):
                cases.append((count, a_s[k % len(a_s)], d or 0, d is None))
            k += 1
    return cases


def all_table_cases(n: int, B: int, dt: int) -> list:
    return [c for g in GROUPS for c in table_cases(n, B, dt, g)]


def case_seed(n: int, B: int, dt: int, count: int, A: int, D: int, in_place: bool) -> list:
    return [n, B, dt, count, A, D, int(in_place)]


def rank_offsets(esz: int, n: int, A: int, D: int, in_place: bool):
    """Byte offsets (mod 16) of every rank's input and output from a 16-byte boundary: rank 0's realise A and
    D, the others differ from rank 0's."""
    k = 16 // esz - 1
    ins = [A] + [(A + esz * (1 + (r - 1) % k)) % 16 for r in range(1, n)]
    if in_place:
        return ins, list(ins)
    out0 = (A - D) % 16
    outs = [out0] + [(out0 + esz * (1 + r % k)) % 16 for r in range(1, n)]
    return ins, outs
