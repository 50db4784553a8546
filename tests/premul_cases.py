"""TEST INFRASTRUCTURE (a helper, not a test module): collectives under a user-created PreMulSum op with a scalar
per rank (include/nexr_ring.h: nexrRingRedOpCreatePreMulSum), as data: the scalars, the calls and their expected
bytes (tests/test_premul.py on the CPU, tests/test_premul_gpu.py on the MI355X).

The expected bytes, with the oracle unchanged. Rank r's input goes through oracle.reduce_copy as a K = 1
PreMulSum step with scalars[r] (the product rounded to the datatype); then oracle/ring.py's ncclSum expectation
of the collective and protocol runs on those products. That is the per-rank rule for every datatype: the library
rounds the product to T before the add too, and a 16-bit NaN is canonical after the next step either way. float32
and float64 inputs hold no NaN (which payload survives is the adder's choice there); float16 and bfloat16 ones do.

numpy, tests/arith_edges.py, tests/flat_cases.py and tests/ring_modes_cases.py only; the oracle and oracle.ring are
handed in by the caller."""
from __future__ import annotations

from types import SimpleNamespace
from typing import List

import numpy as np

import arith_edges as ae
import flat_cases as fc
import ring_modes_cases as rm

COLLECTIVES = ("all_reduce", "reduce_scatter", "reduce", "tree")
DTYPES = (ae.F32, ae.F16, ae.BF16, ae.F64, ae.I32, ae.U8)   # of the CPU end-to-end tests
HOST_IMMEDIATE, DEVICE = 1, 0                                # nexrScalarResidence_t


def scalar_values(dt: int, n: int) -> list:
    """n distinct scalars. Floats: +-(2k + 3) / 4, an odd numerator of at most 8 bits over 4, so never a power of
    two and exact in bfloat16. Integers: odd numbers from 3 on, every other one negative for a signed type."""
    if dt in ae.FLOATS:
        assert 2 * n + 3 < 256
        return [(-1.0 if k % 2 else 1.0) * (2 * k + 3) / 4.0 for k in range(n)]
    vals = [(2 * k + 3) % 251 for k in range(n)]
    if dt in ae.SIGNED_INTS:
        vals = [-v if k % 2 else v for k, v in enumerate(vals)]
    return vals


def scalar_bits(dt: int, n: int) -> List[int]:
    """scalar_values as the raw bits of one element each."""
    vals = scalar_values(dt, n)
    if dt in ae.FLOATS:
        return [int(b) for b in rm._to_bits(dt, np.array(vals, np.float64))]
    mask = (1 << ae.BITS[dt]) - 1
    return [int(v) & mask for v in vals]


def scalar_array(dt: int, bits: List[int]) -> np.ndarray:
    """The scalars as elements of the datatype (carried, like every buffer, as the unsigned integer of its width)."""
    return np.array(bits, dtype=ae.UINT[dt])


def rotate(bits: List[int]) -> List[int]:
    return list(bits[1:]) + list(bits[:1])


class Call(fc.Call):
    """fc.Call (layout, guards, order-sensitive inputs) with the NaNs of float32 / float64 inputs replaced by
    finite values; the op of the spec is not used (the call runs under a user op)."""

    def __init__(self, sp: rm.Spec, n: int, seed: int):
        super().__init__(sp, n, seed)
        if sp.dt in (ae.F32, ae.F64):
            rng = np.random.default_rng([seed, sp.k, sp.count, 0x9E3])
            for r in range(n):
                nan = ae.is_nan(sp.dt, self.inputs[r])
                if nan.any():
                    self.inputs[r][nan] = fc._finite(rng, sp.dt, int(nan.sum()))
                raw = self.inputs[r].view(np.uint8)
                self.arena0[self.send_off[r]:self.send_off[r] + raw.size] = raw


def spec(k: int, collective: str, edge: str, count: int, dt: int, n: int) -> rm.Spec:
    """Call k: in place when k is odd, root k mod n (over a test's calls every root occurs)."""
    return rm.Spec(k, collective, edge, count, dt, rm.SUM, k % 2 == 1, k % n)


def premultiplied(oracle, call, bits: List[int]) -> list:
    """Every rank's input through the K = 1 PreMulSum step with its own scalar."""
    dt = call.spec.dt
    return [oracle.reduce_copy([np.ascontiguousarray(x)], 1, dt, ae.PREMULSUM, s, [s], False)[0]
            for x, s in zip(call.inputs, bits)]


def expected_outputs(oracle, oring, call, bits: List[int], protocol: str, channels: int) -> list:
    """Every rank's expected output (None: not written): oracle.ring's ncclSum expectation on the products."""
    assert len(bits) == call.n
    shadow = SimpleNamespace(spec=call.spec._replace(op=rm.SUM), n=call.n, inputs=premultiplied(oracle, call, bits))
    return rm.oracle_outputs(oring, shadow, protocol, channels)


def make_call(oracle, oring, sp: rm.Spec, n: int, seed: int, bits: List[int], protocol: str, channels: int) -> Call:
    call = Call(sp, n, seed)
    return call.set_outputs(expected_outputs(oracle, oring, call, bits, protocol, channels))


def expected_arena(oracle, oring, call, bits: List[int], protocol: str, channels: int) -> np.ndarray:
    """The expected bytes of the same call under other scalars (call.expected stays as it is)."""
    keep = call.expected
    arena = call.set_outputs(expected_outputs(oracle, oring, call, bits, protocol, channels)).expected
    call.expected = keep
    return arena


def plan(protocol: str, n: int, chunk_of, dtypes=DTYPES, collectives=COLLECTIVES) -> List[rm.Spec]:
    """For every collective every edge of rm.EDGES (1 element to 2nC + 3), call k with datatype k mod len(dtypes);
    a (collective, count, datatype) that has occurred is not repeated."""
    out, seen = [], set()
    for coll in collectives:
        for name, f in rm.EDGES:
            k = len(out)
            dt = dtypes[k % len(dtypes)]
            e = rm.esz_of(dt)
            count = f(n, 16 // e, chunk_of(coll, protocol, e))
            if count < 1 or (coll, count, dt) in seen:
                continue
            seen.add((coll, count, dt))
            out.append(spec(k, coll, name, count, dt, n))
    return out


def check(call, got: np.ndarray, context=(), expected=None) -> None:
    """rm.check on the whole arena, float32 / float64 NaNs of the outputs compared by class (fc.canon_outputs: an
    infinity minus an infinity makes one, whose sign is the adder's choice)."""
    exp = call.expected if expected is None else expected
    rm.check(call, fc.canon_outputs(call, got), context, expected=fc.canon_outputs(call, exp))
