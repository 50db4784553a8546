"""TEST INFRASTRUCTURE (a helper, not a test module): the numpy model of the symmetric reduce-scatter and
all-gather (include/nexr.h, nexrSymReduceScatter / nexrSymAllGather; reference
src/device/symmetric/reduce_scatter.hh:6-241, all_gather.hh:5-177) and the case tables their CPU and GPU tests
share. numpy and tests/sym_cases.py only; it never imports the library under test.

ReduceScatter: rank s's input is n chunks of `count` elements; output r is chunk r folded from rank r's own
input on (sc.fold_from(dt, chunks_r, start=r)): float32 adds, one conversion back. There is no ownership map:
no output byte depends on alignment. The three regions of a chunk (whole 2048-byte pieces, 16-byte packs,
the last elements below 16 bytes) are the device's layout, restated here only to place witnesses in each.

AllGather: output s is the n inputs in rank order, a bit copy.
"""
from __future__ import annotations

import numpy as np

import sym_cases as sc

RANKS = (2, 3, 5, 8)
PIECES, PACKS, TAIL = 1, 2, 3
REGIONS = (PIECES, PACKS, TAIL)
MODES = ("out_of_place", "in_place", "on_next_rank")  # where outputs[r] lies (rs_case_layout)


# ---- reduce-scatter ----------------------------------------------------------------------------------------------
def rs_counts(esz: int, n: int) -> list:
    """Elements per rank: p = one 16-byte pack, g = half a piece, P = one 2048-byte piece."""
    p, g, P = 16 // esz, 1024 // esz, 2048 // esz
    out = []
    for c in (1, p - 1, p, p + 1, g - 1, g + 1, P - 1, P, P + 1, 3 * P + g + p + 1, 2 * n * P + 37):
        if c not in out:
            out.append(c)
    return out


def chunk_regions(esz: int, count: int) -> np.ndarray:
    """The region of every element of a chunk, cut from the chunk's byte 0."""
    n_bytes = count * esz
    pieces_end = n_bytes // 2048 * 2048
    packs_end = pieces_end + (n_bytes - pieces_end) // 16 * 16
    byte = np.arange(count, dtype=np.int64) * esz
    return np.where(byte < pieces_end, PIECES, np.where(byte < packs_end, PACKS, TAIL)).astype(np.int8)


def witness_positions(esz: int, count: int) -> dict:
    """Up to three elements (first, middle, last) of each non-empty region of a chunk."""
    region = chunk_regions(esz, count)
    out = {}
    for reg in REGIONS:
        cand = np.flatnonzero(region == reg)
        if cand.size:
            out[reg] = sorted({int(cand[i]) for i in (0, cand.size // 2, cand.size - 1)})
    return out


def rs_inputs(dt: int, n: int, count: int, seed) -> list:
    """n inputs of n * count elements: random finite values; in every chunk the special columns of sym_cases at
    elements 3, 10, 17, ... (as far as they fit: at most one float32 NaN per element, no infinities of opposite
    sign); and, in every chunk r >= 1, fold-order witnesses at up to three elements of each region: big at
    rank r, -big at rank r + 1, a value that vanishes beside big elsewhere."""
    rng = np.random.default_rng(seed)
    ins = [sc.random_values(dt, rng, n * count) for _ in range(n)]
    cols = sc.special_columns(dt, n)
    big, small = (sc.from_float(dt, x) for x in sc._WITNESS[dt])
    sign = 1 << (8 * sc.ESZ[dt] - 1)
    wit = witness_positions(sc.ESZ[dt], count)
    for r in range(n):
        for k, col in enumerate(cols):
            pos = 3 + 7 * k
            if pos >= count:
                break
            for s, v in enumerate(col):
                if v is not None:
                    ins[s][r * count + pos] = v
        if r >= 1:
            for positions in wit.values():
                for pos in positions:
                    for s in range(n):
                        ins[s][r * count + pos] = big if s == r else (big | sign) if s == (r + 1) % n else small
    return ins


def chunks_of(ins: list, count: int, r: int) -> list:
    return [np.ascontiguousarray(x[r * count:(r + 1) * count]) for x in ins]


def rs_expected(dt: int, ins: list, count: int) -> list:
    """Output r = chunk r folded from rank r on."""
    return [sc.fold_from(dt, chunks_of(ins, count, r), r) for r in range(len(ins))]


def rs_expected_shipped(dt: int, ins: list, count: int) -> list:
    """Every add returns its first operand: rank r's own chunk through the two casts."""
    return [sc.narrow(dt, sc.widen(dt, chunks_of(ins, count, r)[r])) for r in range(len(ins))]


def rs_rank0_first(dt: int, ins: list, count: int) -> list:
    return [sc.fold_from(dt, chunks_of(ins, count, r), 0) for r in range(len(ins))]


def rs_per_step_rounding(dt: int, ins: list, count: int) -> list:
    """Rank r first, but rounded to T after every add."""
    return [sc.per_step_rounding(dt, chunks_of(ins, count, r), np.full(count, r, dtype=np.int32))
            for r in range(len(ins))]


def rs_offsets(esz: int, n: int):
    """Byte offsets (mod 16) of every rank's input and output slot: element-aligned, neighbours differ."""
    k = 16 // esz
    return [esz * (r % k) for r in range(n)], [esz * ((3 * r + 1) % k) for r in range(n)]


# ---- all-gather ------------------------------------------------------------------------------------------------
AG_RANKS = (2, 3, 5, 8, 13)
AG_BYTES = (1, 15, 16, 17, 1023, 1025, 2047, 2048, 2049, 3 * 2048 + 1024 + 16 + 5)
AG_MODES = ("out_of_place", "in_place", "even_in_place")


def ag_inputs(n: int, n_bytes: int, seed) -> list:
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=n_bytes, dtype=np.uint8) for _ in range(n)]


def ag_expected(ins: list) -> np.ndarray:
    return np.concatenate([np.ascontiguousarray(x).view(np.uint8).reshape(-1) for x in ins])


def ag_offsets(n: int, parity: int):
    """Byte offsets of the input and output slots: all odd (parity 1) or all even (0), neighbours differ mod 16."""
    return [(2 * ((5 * r + 1) % 8) + parity) % 16 for r in range(n)], [(2 * ((3 * s + 2) % 8) + parity) % 16 for s in range(n)]
