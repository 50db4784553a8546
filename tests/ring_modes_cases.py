"""TEST INFRASTRUCTURE (a helper, not a test module): the ring and tree collectives at small counts under every
launch mode (tests/test_ring_modes.py on the CPU, tests/test_ring_modes_gpu.py on the MI355X), as data: the
modes, the count table, the (datatype, op) pairs, inputs whose reduction no fold order can change, the expected
bytes of every rank, and the checker.

numpy and tests/arith_edges.py only; it never imports the library under test or the oracle. What needs the
oracle's restatements (the chunk count of a collective, the fold-order-dependent float average at 3 ranks) is
handed in by the caller: `chunk_of` is oracle.ring.chunk_count behind BUFF, `oring` is the module oracle.ring.

Every buffer is carried as the unsigned integer of the element's width (the bits are what count). All ranks'
buffers of one call live in ONE byte arena, each user buffer with GUARD bytes of GUARD_BYTE before and behind it
and every output pre-filled with BLANK, so that one comparison of the whole arena checks every output whole, every
guard, every input, and every output the collective must not write (a reduce's non-root outputs)."""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional

import numpy as np

import arith_edges as ae

COLLECTIVES = ("all_reduce", "reduce_scatter", "all_gather", "reduce", "broadcast", "tree")
COPIES = ("all_gather", "broadcast")
PROTO_ID = {"simple": 0, "ll": 1, "ll128": 2}
# the smallest FIFOs the GPU tests of each protocol already use
BUFF = {"simple": 8 * 4096, "ll": 8 * 16 * 512, "ll128": 8 * 2048 * 8}
RANKS = (2, 3, 4, 8)
CHANNELS = (1, 2)
SUM, PROD, MAX, MIN, AVG = range(5)  # ncclRedOp_t
OP_NAMES = {SUM: "sum", PROD: "prod", MAX: "max", MIN: "min", AVG: "avg"}
GUARD, GUARD_BYTE, BLANK = 64, 0x5A, 0xC3
SEED = 0x52494E47  # of both test modules: what runs on the GPU has run on the host path


class Mode(NamedTuple):
    protocol: str
    group: bool   # set_simple_group (SIMPLE) or set_ll_group (LL, LL128)
    direct: bool  # set_direct (SIMPLE only)

    @property
    def id(self):
        return self.protocol + ("-group" if self.group else "") + ("-direct" if self.direct else "")


MODES = [Mode("simple", False, False), Mode("simple", True, False), Mode("simple", False, True),
         Mode("simple", True, True), Mode("ll", False, False), Mode("ll", True, False), Mode("ll128", False, False),
         Mode("ll128", True, False)]
# call k of a test uses pair k mod 11: all ten datatypes, all five ops
PAIRS = [(ae.F32, SUM), (ae.I8, MIN), (ae.BF16, SUM), (ae.U64, PROD), (ae.F16, AVG), (ae.I32, AVG), (ae.F64, MAX),
         (ae.U8, MAX), (ae.U32, SUM), (ae.I64, MIN), (ae.BF16, PROD)]


def esz_of(dt: int) -> int:
    return ae.BITS[dt] // 8


def tree_per_node(n: int) -> int:
    """treeRanksPerNode of the communicators: binary trees over single ranks (odd n) or over chains of two."""
    return 1 if n % 2 else 2


# ---- the count table -----------------------------------------------------------------------------------------
# n ranks, p = 16 / e elements a pack, C the chunk element count of the collective's geometry
EDGES = (("1", lambda n, p, c: 1), ("2", lambda n, p, c: 2), ("n-1", lambda n, p, c: n - 1), ("n", lambda n, p, c: n),
         ("n+1", lambda n, p, c: n + 1), ("p-1", lambda n, p, c: p - 1), ("p", lambda n, p, c: p),
         ("p+1", lambda n, p, c: p + 1), ("np-1", lambda n, p, c: n * p - 1), ("np", lambda n, p, c: n * p),
         ("np+1", lambda n, p, c: n * p + 1), ("C-1", lambda n, p, c: c - 1), ("C", lambda n, p, c: c),
         ("C+1", lambda n, p, c: c + 1), ("nC-1", lambda n, p, c: n * c - 1), ("nC", lambda n, p, c: n * c),
         ("nC+1", lambda n, p, c: n * c + 1), ("nC+n+1", lambda n, p, c: n * c + n + 1),
         ("2nC+3", lambda n, p, c: 2 * n * c + 3))


def raw_counts(n: int, esz: int, chunk: int) -> list:
    """[(edge name, count)] in EDGES' order, duplicates and all."""
    return [(name, f(n, 16 // esz, chunk)) for name, f in EDGES]


def count_table(n: int, esz: int, chunk: int) -> list:
    """The counts of one (collective, protocol, element size, n): EDGES without duplicates and values below 1.
    The per-rank count for reduce-scatter and all-gather."""
    out = []
    for _name, c in raw_counts(n, esz, chunk):
        if c >= 1 and c not in out:
            out.append(c)
    return out


def empty_chunks(n: int, esz: int, count: int) -> int:
    """How many ranks' chunks of a ring all-reduce's last loop of `count` elements are empty, by the schedule's
    formula (all_reduce.h:31-44: chunkCount = alignUp(divUp(count, n), 16 / e), nelem = min(chunkCount,
    count - chunk * chunkCount))."""
    p = 16 // esz
    per_rank = (count + n - 1) // n
    chunk = (per_rank + p - 1) // p * p
    return sum(1 for c in range(n) if min(chunk, count - c * chunk) <= 0)


class Spec(NamedTuple):
    k: int            # the call's index in its test
    collective: str
    edge: str
    count: int        # per rank for reduce_scatter and all_gather
    dt: int
    op: int
    in_place: bool
    root: int

    def what(self):
        return (self.collective, self.edge, self.count, ae.NAMES[self.dt], OP_NAMES[self.op],
                "in place" if self.in_place else "out of place", "root %d" % self.root)


def spec(k: int, collective: str, edge: str, count: int, n: int) -> Spec:
    dt, op = PAIRS[k % len(PAIRS)]
    return Spec(k, collective, edge, count, dt, op, k % 2 == 1, k % n)


def plan(protocol: str, n: int, chunk_of: Callable, collectives=COLLECTIVES) -> List[Spec]:
    """The calls of the table test on one communicator: for every collective every edge of EDGES, evaluated at
    the element size of the call's own pair; call k takes pair k mod 11, is in place when k is odd, and has
    root k mod n. A (collective, count, datatype) that has occurred is not repeated."""
    out, seen = [], set()
    for coll in collectives:
        for name, f in EDGES:
            k = len(out)
            dt = PAIRS[k % len(PAIRS)][0]
            e = esz_of(dt)
            count = f(n, 16 // e, chunk_of(coll, protocol, e))
            if count < 1 or (coll, count, dt) in seen:
                continue
            seen.add((coll, count, dt))
            out.append(spec(k, coll, name, count, n))
    return out


# trafficPerByte of the planner's channel split (enqueue.cc:74-81) and, per collective, a count of several loops
# whose traffic is at least four channels' minimum of 16 KiB, so that it spreads over two channels
TRAFFIC = {"all_reduce": lambda n: 2, "tree": lambda n: 2, "reduce_scatter": lambda n: n, "all_gather": lambda n: n,
           "reduce": lambda n: 1, "broadcast": lambda n: 1}
LARGE = {"all_reduce": lambda n, c: 4 * n * c + 5, "tree": lambda n, c: 4 * n * c + 5,
         "reduce_scatter": lambda n, c: 8 * c + 5, "all_gather": lambda n, c: 8 * c + 5,
         "reduce": lambda n, c: 16 * c + 5, "broadcast": lambda n, c: 16 * c + 5}
SIMPLE_STATES = ((False, False), (True, False), (False, True), (True, True))   # (group, direct)


def mixed_plan(protocol: str, n: int, chunk_of: Callable, seed: int, calls: int = 24) -> List[Spec]:
    """Seeded calls for one communicator with 2 channels: the counts alternate between a tiny one (< n p, which
    stays on channel 0 with empty chunks), a chunk edge and a LARGE one; the collectives come from shuffled
    decks of all six."""
    rng = np.random.default_rng(seed)
    out = []
    deck = []
    for k in range(calls):
        if not deck:
            deck = [COLLECTIVES[i] for i in rng.permutation(len(COLLECTIVES))]
        coll = deck.pop()
        e = esz_of(PAIRS[k % len(PAIRS)][0])
        p, c = 16 // e, chunk_of(coll, protocol, e)
        if k % 3 == 0:
            edge, count = "tiny", int(rng.integers(1, n * p))
        elif k % 3 == 1:
            edge, count = [("C-1", c - 1), ("C", c), ("C+1", c + 1), ("nC+1", n * c + 1)][int(rng.integers(4))]
        else:
            edge, count = "large", LARGE[coll](n, c)
        out.append(spec(k, coll, edge, count, n))
    return out


def mixed_state(protocol: str, k: int) -> tuple:
    """(group, direct) of call k: the option state changes every three calls."""
    if protocol == "simple":
        return SIMPLE_STATES[(k // 3) % 4]
    return ((k // 3) % 2 == 1, False)


# ---- inputs and the order-independent reference ----------------------------------------------------------------
def _to_bits(dt: int, x: np.ndarray) -> np.ndarray:
    """float64 values that the type holds exactly, as its bits."""
    if dt == ae.F64:
        return x.view(np.uint64).copy()
    if dt == ae.F16:
        r = x.astype(np.float16)
        assert np.array_equal(r.astype(np.float64), x)
        return r.view(np.uint16).copy()
    f = x.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), x)
    u = f.view(np.uint32)
    if dt == ae.F32:
        return u.copy()
    assert not (u & np.uint32(0xFFFF)).any()
    return (u >> np.uint32(16)).astype(np.uint16)


def _random_bits(rng, dt: int, size: int) -> np.ndarray:
    return rng.integers(0, 256, size * esz_of(dt), dtype=np.uint8).view(ae.UINT[dt])


def gen_inputs(rng, dt: int, op: Optional[int], n: int, size: int) -> list:
    """n buffers of `size` elements. op None (a copy): any bit pattern, NaN payloads included. Integers:
    uniformly random bits. Floats: sum and avg integers in [-8, 8] (|sum| <= 64 at 8 ranks: exact in bf16's 8
    significant bits), prod +-0.5 / +-1 / +-2, min and max normal numbers (finite, non-zero, no NaN)."""
    if op is None or dt in ae.INTS:
        return [_random_bits(rng, dt, size) for _ in range(n)]
    if op in (SUM, AVG):
        return [_to_bits(dt, rng.integers(-8, 9, size).astype(np.float64)) for _ in range(n)]
    if op == PROD:
        vals = np.array([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])
        return [_to_bits(dt, vals[rng.integers(0, 6, size)]) for _ in range(n)]
    e_bits, m_bits = ae.FMT[dt]
    out = []
    for _ in range(n):
        sign = rng.integers(0, 2, size, dtype=np.uint64) << np.uint64(e_bits + m_bits)
        expo = rng.integers(1, (1 << e_bits) - 1, size, dtype=np.uint64) << np.uint64(m_bits)
        mant = rng.integers(0, 1 << m_bits, size, dtype=np.uint64)
        out.append((sign | expo | mant).astype(ae.UINT[dt]))
    return out


def reduce_all(dt: int, op: int, xs: list) -> Optional[np.ndarray]:
    """op over xs element by element, exact whatever the fold order (for gen_inputs' values). None for the one
    case that has no such answer: a float average whose 1 / n is not a power of two."""
    n = len(xs)
    if dt in ae.INTS:
        u = ae.UINT[dt]
        signed = np.dtype("i%d" % esz_of(dt))
        if op in (SUM, AVG, PROD):
            acc = xs[0].astype(u, copy=True)
            for x in xs[1:]:                       # unsigned array arithmetic wraps modulo 2^bits
                acc = acc * x if op == PROD else acc + x
            if op != AVG:
                return acc
            if dt not in ae.SIGNED_INTS:
                return acc // u.type(n)
            s = acc.view(signed)                   # FuncSumPostDiv: the signed quotient truncates toward zero
            q = s // signed.type(n)
            q = q + ((s % signed.type(n) != 0) & (s < 0)).astype(signed)
            return q.view(u)
        v = [x.view(signed) if dt in ae.SIGNED_INTS else x for x in xs]
        r = (np.maximum if op == MAX else np.minimum).reduce(np.stack(v), axis=0)
        return np.ascontiguousarray(r).view(u)
    if op in (MAX, MIN):
        wide = np.stack([ae.widen(dt, x) for x in xs])
        pick = (np.argmax if op == MAX else np.argmin)(wide, axis=0)
        return np.stack(xs)[pick, np.arange(xs[0].size)]
    wide = [ae.widen(dt, x) for x in xs]
    acc = wide[0].copy()
    for w in wide[1:]:
        acc = acc * w if op == PROD else acc + w
    if op == AVG:
        if n & (n - 1):
            return None
        acc = acc / n
    return _to_bits(dt, acc)


# ---- one call: layout, expected bytes, pointers -----------------------------------------------------------------
class Call:
    """One collective on n ranks: `arena0` is what the memory holds before it, `expected` after it (None until
    set_outputs); send_off / recv_off are every rank's user pointers as byte offsets into the arena."""

    def __init__(self, sp: Spec, n: int, seed: int):
        self.spec, self.n = sp, n
        coll, count, dt = sp.collective, sp.count, sp.dt
        e = self.esz = esz_of(dt)
        rng = np.random.default_rng([seed, sp.k, count])
        if coll == "reduce_scatter":
            send_n, recv_n = n * count, count
        elif coll == "all_gather":
            send_n, recv_n = count, n * count
        else:
            send_n = recv_n = count
        self.send_elems, self.recv_elems = send_n, recv_n
        self.inputs = gen_inputs(rng, dt, None if coll in COPIES else sp.op, n, send_n)
        self.send_off, self.recv_off, self.regions = [], [], []   # regions: (rank, kind, offset, bytes)
        parts, at = [], 0

        def put(raw):
            nonlocal at
            parts.append(np.full(GUARD + (-at) % 16, GUARD_BYTE, np.uint8))   # user buffers start 16-byte aligned
            at += parts[-1].size
            off = at
            parts.append(np.ascontiguousarray(raw).view(np.uint8))
            at += parts[-1].size
            return off

        for r in range(n):
            if not sp.in_place:
                junk = coll == "broadcast" and r != sp.root   # never read
                s = put(_random_bits(rng, dt, send_n) if junk else self.inputs[r])
                d = put(np.full(recv_n * e, BLANK, np.uint8))
            elif coll == "reduce_scatter":
                s = put(self.inputs[r])
                d = s + r * count * e
            elif coll == "all_gather":
                buf = np.full(recv_n * e, BLANK, np.uint8)
                buf[r * count * e:(r + 1) * count * e] = self.inputs[r].view(np.uint8)
                d = put(buf)
                s = d + r * count * e
            elif coll == "broadcast" and r != sp.root:
                s = d = put(np.full(recv_n * e, BLANK, np.uint8))
            else:
                s = d = put(self.inputs[r])
            self.send_off.append(s)
            self.recv_off.append(d)
            self.regions.append((r, "input", s, send_n * e))
            self.regions.append((r, "output", d, recv_n * e))
        parts.append(np.full(GUARD, GUARD_BYTE, np.uint8))
        self.arena0 = np.concatenate(parts)
        self.expected = None

    def outputs(self) -> Optional[list]:
        """Every rank's expected output (None: the collective leaves it as it was), from reduce_all; None
        altogether where reduce_all has no answer (then the caller asks oracle_outputs)."""
        sp, n = self.spec, self.n
        if sp.collective == "all_gather":
            whole = np.concatenate(self.inputs)
            return [whole] * n
        if sp.collective == "broadcast":
            return [self.inputs[sp.root]] * n
        red = reduce_all(sp.dt, sp.op, self.inputs)
        if red is None:
            return None
        if sp.collective == "reduce_scatter":
            return [red[r * sp.count:(r + 1) * sp.count] for r in range(n)]
        if sp.collective == "reduce":
            return [red if r == sp.root else None for r in range(n)]
        return [red] * n

    def set_outputs(self, outs: list) -> "Call":
        exp = self.arena0.copy()
        for r, o in enumerate(outs):
            if o is None:
                continue
            raw = np.ascontiguousarray(o).view(np.uint8).reshape(-1)
            assert raw.size == self.recv_elems * self.esz, (self.spec.what(), r, raw.size)
            exp[self.recv_off[r]:self.recv_off[r] + raw.size] = raw
        self.expected = exp
        return self


def oracle_outputs(oring, call: Call, protocol: str, channels: int) -> list:
    """Every rank's expected output from oracle.ring's restatements (`oring`), which follow the protocol's fold
    order and the channel split: for what reduce_all cannot answer, and to compare reduce_all with."""
    sp, n, xs = call.spec, call.n, call.inputs
    buff = BUFF[protocol]
    if sp.collective == "all_gather":
        return oring.all_gather_expected(xs)
    if sp.collective == "broadcast":
        return oring.broadcast_expected(xs, sp.root)
    if sp.collective == "all_reduce":
        if protocol == "simple":
            return oring.ring_allreduce_expected(xs, sp.dt, sp.op, buff, channels)
        return oring.ring_allreduce_expected_ll(xs, sp.dt, sp.op, buff, protocol, channels)
    if sp.collective == "reduce_scatter":
        return oring.reduce_scatter_expected(xs, sp.dt, sp.op, protocol)
    if sp.collective == "reduce":
        red = oring.reduce_expected(xs, sp.dt, sp.op, sp.root, protocol)
        return [red if r == sp.root else None for r in range(n)]

    def links_of(ch):
        return oring.tree_topology(n, tree_per_node(n), 1 if (channels >= 2 and ch >= channels // 2) else 0)
    return oring.tree_allreduce_expected_channels(xs, sp.dt, sp.op, links_of, channels, protocol)


def make_call(sp: Spec, n: int, seed: int, oring=None, protocol: str = "simple", channels: int = 1) -> Call:
    """The call with its expected bytes: reduce_all's where it has an answer, else oracle.ring's (`oring`)."""
    call = Call(sp, n, seed)
    outs = call.outputs()
    if outs is None:
        outs = oracle_outputs(oring, call, protocol, channels)
    return call.set_outputs(outs)


def issue(comm, call: Call, base: int, count: Optional[int] = None) -> None:
    """The collective on `comm` (a RingComm or anything with its methods), the arena at address `base`."""
    sp = call.spec
    count = sp.count if count is None else count
    s = [base + o for o in call.send_off]
    d = [base + o for o in call.recv_off]
    if sp.collective == "all_reduce":
        comm.all_reduce(s, d, count, sp.dt, sp.op)
    elif sp.collective == "tree":
        comm.tree_all_reduce(s, d, count, sp.dt, sp.op)
    elif sp.collective == "reduce_scatter":
        comm.reduce_scatter(s, d, count, sp.dt, sp.op)
    elif sp.collective == "all_gather":
        comm.all_gather(s, d, count, sp.dt)
    elif sp.collective == "reduce":
        comm.reduce(s, d, count, sp.dt, sp.op, sp.root)
    else:
        comm.broadcast(s, d, count, sp.dt, sp.root)


# ---- the checker --------------------------------------------------------------------------------------------------
def check(call: Call, got: np.ndarray, context=(), expected: Optional[np.ndarray] = None) -> None:
    """The whole arena after the call against the expected bytes: every output whole, every guard, every input,
    every output that must stay as it was. The failure names the context (mode, n, channels), the call, the rank,
    what was hit and the first differing element."""
    exp = call.expected if expected is None else expected
    got = np.ascontiguousarray(got).view(np.uint8).reshape(-1)
    assert got.size == exp.size, (context, call.spec.what(), "arena size", got.size, exp.size)
    if np.array_equal(got, exp):
        return
    bad = np.flatnonzero(got != exp)
    b = int(bad[0])
    e = call.esz
    hit = None
    for rank, kind, off, nbytes in call.regions:
        if off <= b < off + nbytes and (hit is None or kind == "output"):
            hit = (rank, kind, (b - off) // e, off + (b - off) // e * e)
    if hit is None:  # a guard: name the nearest user buffer
        rank, kind, off, nbytes = min(call.regions, key=lambda g: min(abs(b - g[2]), abs(b - (g[2] + g[3]))))
        where = "guard before" if b < off else "guard behind"
        raise AssertionError((context, call.spec.what(), "rank %d" % rank, "%s the %s" % (where, kind),
                              "arena byte %d" % b, "0x%02x" % got[b], "%d bytes differ" % bad.size))
    rank, kind, elem, at = hit
    untouched = kind == "output" and call.spec.collective == "reduce" and rank != call.spec.root
    raise AssertionError((context, call.spec.what(), "rank %d" % rank,
                          "%s%s" % (kind, " that must stay untouched" if untouched else ""), "first differing element %d" % elem,
                          "got 0x" + got[at:at + e][::-1].tobytes().hex(), "expected 0x" + exp[at:at + e][::-1].tobytes().hex(),
                          "%d bytes differ" % bad.size))
