"""TEST INFRASTRUCTURE (a helper, not a test module): the numpy model of the symmetric LL collectives
(include/nexr.h, nexrSymLLAllReduce / nexrSymLLReduceScatter / nexrSymLLAllGather; reference
src/device/symmetric/all_reduce.hh:356-428, reduce_scatter.hh:320-388, all_gather.hh:256-363) and the case
tables their CPU and GPU tests share. numpy and tests/sym_cases.py only; it never imports the library under
test, so the round size R (NEXR_SYM_LL_ROUND_PACKS) is an argument.

AllReduce: every output is sc.fold_from(dt, inputs, 0): rank 0 first, float32 adds, one conversion back.
ReduceScatter: output r is that fold of chunk r of every input. AllGather: the inputs in rank order.

The protocol part of the model is the flag sequence: block b of a call over P packs with B blocks runs
ceil(share(P, B, b) / R) rounds, round k with flag stored + 2 + k where 2 follows 0xffffffff, and stores the
next flag minus 2.

Witnesses. At elements 0 and 1 mod 7 of every chunk (the special columns of sym_cases sit at 3 mod 7):
  A  big at rank 1, -big at rank 2, a value that vanishes beside big elsewhere (with two ranks: big at rank 1);
  B  big at rank 0, -big at rank 1, the vanishing value elsewhere.
A alone tells a rank-0-first fold from a fold that starts at rank r for every r >= 1 but one: with three ranks
the orders (0, 1, 2) and (2, 0, 1) both give s + big - big = -big + s + big = 0. B tells those two apart.
"""
from __future__ import annotations

import numpy as np

import sym_cases as sc

RANKS = (2, 3, 8)
BLOCKS = (1, 3)


# ---- the split and the flags -------------------------------------------------------------------------------------
def packs(n_bytes: int) -> int:
    return (n_bytes + 7) // 8


def share(P: int, B: int, b: int) -> int:
    return P // B + (1 if b < P % B else 0)


def rounds(P: int, B: int, b: int, R: int) -> int:
    return -(-share(P, B, b) // R)


def next_flag(f: int) -> int:
    return 2 if f == 0xFFFFFFFF else f + 1


def flags(stored: int, k: int):
    """The flags of k rounds from a stored word, and the word stored afterwards."""
    f, out = (stored + 2) & 0xFFFFFFFF, []
    assert f >= 2
    for _ in range(k):
        out.append(f)
        f = next_flag(f)
    return out, f - 2


def advance(words: list, P: int, B: int, R: int) -> list:
    """The 64 epoch words after one call of P packs with B blocks."""
    out = list(words)
    for b in range(B):
        out[b] = flags(words[b], rounds(P, B, b, R))[1]
    return out


def pack_counts(R: int, B: int) -> list:
    """Packs per call: one, two (with three blocks one team is empty), around one round, 3R + 1 (with three
    blocks team 0 runs two rounds and the others one), and 2R + 3 with one block."""
    return [1, 2, R - 1, R, R + 1, 3 * R + 1] + ([2 * R + 3] if B == 1 else [])


def byte_counts(P: int, esz: int, all_gather: bool) -> list:
    """Bytes of P packs: a multiple of 8, and with a last pack of esz bytes (the all-gather: 1, 3 and 7)."""
    tails = (1, 3, 7) if all_gather else (esz,)
    return [8 * P] + [8 * (P - 1) + t for t in tails]


# ---- inputs ----------------------------------------------------------------------------------------------------
def witness_values(dt: int, n: int, kind: str) -> list:
    big, small = (sc.from_float(dt, x) for x in sc._WITNESS[dt])
    sign = 1 << (8 * sc.ESZ[dt] - 1)
    first = 1 if kind == "A" else 0
    return [big if s == first else (big | sign) if s == first + 1 else small for s in range(n)]


def witness_positions(count: int) -> dict:
    return {"A": list(range(0, count, 7)), "B": list(range(1, count, 7))}


def chunk_inputs(dt: int, n: int, count: int, n_chunks: int, seed) -> list:
    """n inputs of n_chunks * count elements: random finite values, in every chunk the special columns of
    sym_cases at elements 3, 10, 17, ... (as far as they fit: at most one float32 NaN per element, no opposite
    infinities) and the witnesses."""
    rng = np.random.default_rng(seed)
    ins = [sc.random_values(dt, rng, n_chunks * count) for _ in range(n)]
    cols = sc.special_columns(dt, n)
    wit = witness_positions(count)
    for c in range(n_chunks):
        for k, col in enumerate(cols):
            pos = 3 + 7 * k
            if pos >= count:
                break
            for s, v in enumerate(col):
                if v is not None:
                    ins[s][c * count + pos] = v
        for kind, positions in wit.items():
            vals = witness_values(dt, n, kind)
            for pos in positions:
                for s in range(n):
                    ins[s][c * count + pos] = vals[s]
    return ins


def ar_inputs(dt: int, n: int, count: int, seed) -> list:
    return chunk_inputs(dt, n, count, 1, seed)


def rs_inputs(dt: int, n: int, count: int, seed) -> list:
    return chunk_inputs(dt, n, count, n, seed)


def ag_inputs(n: int, n_bytes: int, seed) -> list:
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=n_bytes, dtype=np.uint8) for _ in range(n)]


def chunks_of(ins: list, count: int, r: int) -> list:
    return [np.ascontiguousarray(x[r * count:(r + 1) * count]) for x in ins]


# ---- expectations ------------------------------------------------------------------------------------------------
def ar_expected(dt: int, ins: list) -> np.ndarray:
    return sc.fold_from(dt, ins, 0)


def ar_expected_shipped(dt: int, ins: list) -> np.ndarray:
    """Every add returns its first operand: rank 0's input through the two casts."""
    return sc.narrow(dt, sc.widen(dt, ins[0]))


def rs_expected(dt: int, ins: list, count: int) -> list:
    return [sc.fold_from(dt, chunks_of(ins, count, r), 0) for r in range(len(ins))]


def rs_expected_shipped(dt: int, ins: list, count: int) -> list:
    return [sc.narrow(dt, sc.widen(dt, chunks_of(ins, count, r)[0])) for r in range(len(ins))]


def rs_per_step_rounding(dt: int, ins: list, count: int) -> list:
    """Rank 0 first, but rounded to T after every add."""
    return [sc.per_step_rounding(dt, chunks_of(ins, count, r), np.zeros(count, dtype=np.int32))
            for r in range(len(ins))]


def ag_expected(ins: list) -> np.ndarray:
    return np.concatenate([np.ascontiguousarray(x).view(np.uint8).reshape(-1) for x in ins])


# ---- placement ---------------------------------------------------------------------------------------------------
def offsets(esz: int, n: int, aligned: bool):
    """Byte offsets (mod 16) of every rank's input and output slot. aligned: all 0 or 8. Else the inputs are off
    by esz from an 8-byte boundary and the outputs by another element-aligned offset: the element-wise path."""
    if aligned:
        return [8 * (r % 2) for r in range(n)], [8 * ((r + 1) % 2) for r in range(n)]
    return [esz + 8 * (r % 2) for r in range(n)], [16 - esz - 8 * (r % 2) for r in range(n)]
