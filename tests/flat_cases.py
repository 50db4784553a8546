"""TEST INFRASTRUCTURE (a helper, not a test module): the ring all-reduce, reduce-scatter and reduce stated element
by element, as include/nexr.h states them for nexrFlatAllReduce / nexrFlatReduceScatter / nexrFlatReduce, and
inputs on which a wrong start rank or a wrong operand order shows (tests/test_flat.py on the CPU,
tests/test_flat_gpu.py on the MI355X).

numpy, tests/arith_edges.py and tests/ring_modes_cases.py only (its arena, guards, BUFF, RANKS, CHANNELS, PAIRS and
count table); it never imports the library under test or the oracle. The caller hands in what needs them: the
channel parts of an all-reduce and the step function of the chain.

The rule. An element has a start rank s. v = in[s] through the first step; for j = 1..n-1, r = (s + j) mod n:
v = one reduce-copy step of {in[r], v}, the last one with the post-op. A step function is
    step(x, v, post) -> v'
with x the rank's input elements (an array of the element's unsigned integer), v the partial as the last step
returned it (None for the chain's first rank: the K = 1 step) and post the last step's flag; what the last step
returns is the result's elements. What travels between two steps is the step function's own business (the LL
oracles hand their wire lines on)."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np

import arith_edges as ae
import ring_modes_cases as rm

COLLECTIVES = ("all_reduce", "reduce_scatter", "reduce")


def _div_up(a: int, b: int) -> int:
    return -(-a // b)


# ---- the start rank of every position ------------------------------------------------------------------------
def all_reduce_starts(n: int, count: int, esz: int, parts: Sequence[tuple]) -> np.ndarray:
    """s of every element of an all-reduce of `count` elements: `parts` are (offset, count, chunkCount) in
    elements and tile [0, count). For element i of a part: j = i - offset, loop = n * chunkCount, L = j // loop,
    rem = count - L * loop, cc = alignUp(divUp(rem, n), 16 / esz) if rem < loop else chunkCount,
    c = (j - L * loop) // cc, s = (c + 1) mod n."""
    s = np.full(count, -1, np.int64)
    at = 0
    for offset, cnt, chunk in parts:
        assert offset == at and cnt > 0 and chunk > 0, (parts, at)
        j = np.arange(cnt, dtype=np.int64)
        loop = n * chunk
        L = j // loop
        rem = cnt - L * loop
        last = _div_up(_div_up(cnt % loop if cnt % loop else loop, n), 16 // esz) * (16 // esz)
        cc = np.where(rem < loop, last, chunk)
        c = (j - L * loop) // cc
        assert c.max() < n
        s[offset:offset + cnt] = (c + 1) % n
        at += cnt
    assert at == count and s.min() >= 0
    return s


def starts_of(collective: str, n: int, count: int, esz: int, root: int = 0, parts: Optional[Sequence[tuple]] = None):
    """Per INPUT position: the all-reduce's and the reduce's `count` elements, the reduce-scatter's n * count
    (position d * count + e belongs to chunk d)."""
    if collective == "all_reduce":
        return all_reduce_starts(n, count, esz, parts)
    if collective == "reduce":
        return np.full(count, (root + 1) % n, np.int64)
    assert collective == "reduce_scatter"
    return np.repeat((np.arange(n, dtype=np.int64) + 1) % n, count)


# ---- the model ----------------------------------------------------------------------------------------------------
def fold_positions(inputs: List[np.ndarray], starts: np.ndarray, step: Callable) -> np.ndarray:
    """The rule on every position of the inputs: the chain per distinct start rank over the positions that have
    it."""
    n = len(inputs)
    out = np.empty_like(inputs[0])
    assert starts.size == out.size
    for s in np.unique(starts):
        idx = np.flatnonzero(starts == s)
        v = None
        for j in range(n):
            x = np.ascontiguousarray(inputs[(int(s) + j) % n][idx])
            v = step(x, v, j == n - 1)
        out[idx] = np.asarray(v).view(out.dtype).reshape(-1)
    return out


def model(collective: str, inputs: List[np.ndarray], count: int, root: int, step: Callable,
          parts: Optional[Sequence[tuple]] = None, shift: int = 0) -> list:
    """Every rank's expected output (None: not written) by the rule. `shift` moves every start rank (the
    order-sensitivity check of the inputs)."""
    n, esz = len(inputs), inputs[0].itemsize
    starts = (starts_of(collective, n, count, esz, root, parts) + shift) % n
    red = fold_positions(inputs, starts, step)
    if collective == "all_reduce":
        return [red] * n
    if collective == "reduce":
        return [red if r == root else None for r in range(n)]
    return [red[r * count:(r + 1) * count] for r in range(n)]


# ---- order-sensitive inputs -----------------------------------------------------------------------------------------
def _finite(rng, dt: int, size: int) -> np.ndarray:
    """Random finite normal numbers of mixed magnitude: exponents within m_bits + 3 of the bias, so that sums
    round differently in every order and products of eight stay away from nothing."""
    e_bits, m_bits = ae.FMT[dt]
    bias = (1 << (e_bits - 1)) - 1
    span = min(m_bits + 3, bias - 2)
    sign = rng.integers(0, 2, size, dtype=np.uint64) << np.uint64(e_bits + m_bits)
    expo = rng.integers(bias - span, bias + span + 1, size, dtype=np.uint64) << np.uint64(m_bits)
    mant = rng.integers(0, 1 << m_bits, size, dtype=np.uint64)
    return (sign | expo | mant).astype(ae.UINT[dt])


def gen_inputs(rng, dt: int, n: int, size: int) -> list:
    """n buffers of `size` elements. Integers: random bits. Floats: random finite values of mixed magnitude
    with, at about one position in eight per rank, a value of arith_edges.edge_set (NaN payloads, +-inf, +-0,
    denormals, the largest and smallest normals). float32 / float64 keep a NaN's payload through an add or a
    multiply, and IEEE 754 leaves open which payload survives two NaN operands: there a position holds at most
    one NaN, and then plain finite values on the other ranks (none that could make a second NaN)."""
    if dt in ae.INTS:
        return [rm._random_bits(rng, dt, size) for _ in range(n)]
    edges = ae.edge_set(dt)
    xs = []
    for _ in range(n):
        x = _finite(rng, dt, size)
        hit = rng.integers(0, 8, size) == 0
        x[hit] = edges[rng.integers(0, edges.size, int(hit.sum()))]
        xs.append(x)
    if dt in (ae.F32, ae.F64):
        plain = [_finite(rng, dt, size) for _ in range(n)]
        nan = np.stack([ae.is_nan(dt, x) for x in xs])
        holder = np.argmax(nan, axis=0)   # the first rank with a NaN keeps it
        any_nan = nan.any(axis=0)
        for r in range(n):
            swap = any_nan & (holder != r)
            xs[r][swap] = plain[r][swap]
    return xs


class Call(rm.Call):
    """rm.Call (layout, guards, in place or not, regions) over gen_inputs' order-sensitive inputs: the arena is
    rm.Call's with every input region rewritten."""

    def __init__(self, sp: rm.Spec, n: int, seed: int):
        super().__init__(sp, n, seed)
        rng = np.random.default_rng([seed, sp.k, sp.count, 0xF1A7])
        self.inputs = gen_inputs(rng, sp.dt, n, self.send_elems)
        for r in range(n):
            raw = self.inputs[r].view(np.uint8)
            self.arena0[self.send_off[r]:self.send_off[r] + raw.size] = raw


def canon_outputs(call: rm.Call, arena: np.ndarray) -> np.ndarray:
    """The arena with every float32 / float64 NaN of an output region replaced by one NaN (arith_edges.canon:
    those two types are compared by class, their payloads and the sign of a generated NaN being the adder's
    choice); every other byte, and every other datatype, as it is."""
    dt = call.spec.dt
    if dt not in (ae.F32, ae.F64):
        return arena
    out = np.ascontiguousarray(arena).view(np.uint8).reshape(-1).copy()
    for _rank, kind, off, nbytes in call.regions:
        if kind == "output" and nbytes:
            out[off:off + nbytes] = ae.canon(dt, out[off:off + nbytes].view(ae.UINT[dt])).view(np.uint8)
    return out
