"""The step lists of the SIMPLE group tests (tests/test_simple_group_gpu.py), as data: for every case the
members, connections and nexrLLStep records (one slice each) — once, so that the interpreter
(tests/simple_steps_model.py) and the device calls are given the same thing, and so that a CPU test
(tests/test_simple_steps_model.py) runs every list through the interpreter without a GPU. The Case and
MemberSpec types, the datatype / op tables and the guard fill are tests/ll_steps_cases.py's. Nothing here
touches the GPU or the library under test."""
from typing import List, NamedTuple

import numpy as np

import ll_steps_cases as cases
import make_golden as mg
from oracle import ll_steps

S = ll_steps.Step
SLOTS = cases.SLOTS
TILE = 4096


class SimpleCase(NamedTuple):
    case: cases.Case      # rule unused
    step_per_slice: int
    what: str


def _blank(n_elts, dt):
    return np.full(n_elts * cases.esz_of(dt), cases.FILL, dtype=np.uint8).view(mg.STORE[dt])


def _case(dt, op, arg, slot, conn_start, members, sps, what, prefill=None):
    return SimpleCase(cases.Case(dt, op, arg, slot, None, list(conn_start), prefill or {}, members), sps, what)


# ---- 1: two members, send -> recv-reduce-copy, 40 slices over 8 slots ------------------------------------
def pair_slot(sps):
    """One tile + 1 element must fit a slice: 4 KiB slots for 2-step slices, 4 KiB + 256 B for 1-step ones."""
    return 4096 if sps == 2 else 4096 + 256


def pair_sizes(dt, slot, sps, n_slices=40):
    """Elements per slice, cycled: a full slice, 3 elements, 0, one tile + 1 element."""
    e = cases.esz_of(dt)
    cyc = [slot * sps // e, 3, 0, TILE // e + 1]
    return [cyc[k % 4] for k in range(n_slices)]


def pair_case(sps, dt=mg.F32, n_slices=40, start=None, seed=3) -> SimpleCase:
    """Member 0 sends a fresh piece of its input per slice; member 1 reduces it with its own input into its
    output. 40 slices over 8 slots: 5 wraps at 1-step slices, 10 at 2-step ones."""
    slot = pair_slot(sps)
    sizes = pair_sizes(dt, slot, sps, n_slices)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offs[-1]) + 1
    xs = mg.gen_inputs(dt, 2, total, seed + sps, special=False)
    send = [S(0, int(o), -1, 0, n, False, True, False) for o, n in zip(offs, sizes)]
    fold = [S(0, int(o), 1, int(o), n, True, False, False) for o, n in zip(offs, sizes)]
    m0 = cases.MemberSpec(xs[0], None, [], [0], send)
    m1 = cases.MemberSpec(xs[1], _blank(total, dt), [0], [], fold)
    return _case(dt, mg.SUM, 0, slot, [start if start is not None else 6 * sps], [m0, m1], sps, f"pair sps={sps}")


# ---- 2: a three-member chain ---------------------------------------------------------------------------
CHAIN_PAIRS = [(mg.F32, "sum"), (mg.BF16, "sum"), (mg.F16, "premulsum"), (mg.I32, "sumpostdiv"), (mg.I8, "min"),
               (mg.U64, "prod"), (mg.F64, "max")]


def chain_case(dt, name, sps=1, slot=1024, n_slices=20, seed=11) -> SimpleCase:
    """send (the pre-op on the input), recv-reduce-send (the pre-op again), recv-reduce-copy with the post-op:
    20 slices over 8 slots of 1 KiB, sizes a full slice, 1 element, a third, 0."""
    _n, op, arg = cases.op_named(dt, name)
    e = cases.esz_of(dt)
    cap = slot * sps // e
    cyc = [cap, 1, cap // 3, 0, cap - 1]
    sizes = [cyc[k % 5] for k in range(n_slices)]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offs[-1]) + 1
    xs = mg.gen_inputs(dt, 3, total, seed + dt, special=True)
    a = [S(0, int(o), -1, 0, n, False, True, False) for o, n in zip(offs, sizes)]
    b = [S(0, int(o), -1, 0, n, True, True, False) for o, n in zip(offs, sizes)]
    c = [S(0, int(o), 1, int(o), n, True, False, True) for o, n in zip(offs, sizes)]
    members = [cases.MemberSpec(xs[0], None, [], [0], a), cases.MemberSpec(xs[1], None, [0], [1], b),
               cases.MemberSpec(xs[2], _blank(total, dt), [1], [], c)]
    return _case(dt, op, arg, slot, [5 * sps, 14 * sps], members, sps, f"chain {mg.DT_NAMES[dt]} {name}")


# ---- 3: the fan: user src + 3 recv -> user dst + 3 send (K = 4, M = 4) ------------------------------------
def fan_case(dt, name, seed=23) -> SimpleCase:
    """One member, its three senders' slices pre-filled and its three receivers elsewhere: 3 slices of 300, 1
    and 257 elements at 4 KiB slots, the post-op on every second slice, every connection at a counter of
    its own."""
    _n, op, arg = cases.op_named(dt, name)
    sizes = [300, 1, 257]
    offs = [0, 300, 301]
    total = 558 + 2
    xs = mg.gen_inputs(dt, 5, total, seed + 7 * dt, special=True)
    steps = [S(0, o, 1, o + 1, n, True, True, k % 2 == 0) for k, (o, n) in enumerate(zip(offs, sizes))]
    prefill = {i: [xs[2 + i][o:o + n] for o, n in zip(offs, sizes)] for i in range(3)}
    member = cases.MemberSpec(xs[0], _blank(total, dt), [0, 1, 2], [3, 4, 5], steps)
    return _case(dt, op, arg, 4096, list(cases.RECV_START) + list(cases.SEND_START), [member], 1,
                 f"fan {mg.DT_NAMES[dt]} {name}", prefill)


# ---- 4: user pointers offset by one element, byte counts that are no multiple of 16 -------------------------
def offset_case(dt, sps=1, seed=31) -> SimpleCase:
    """int8 / fp16: every user offset odd (source and destination on different 16-byte phases), slices of
    1, 7, 33, 1000 and 2049 elements, K = 2 and M = 2 (member 1 writes its output and sends on)."""
    sizes = [1, 7, 33, 1000, 2049 if cases.esz_of(dt) == 1 else 1023, 15]
    region = 2052
    total = region * len(sizes) + 8
    xs = mg.gen_inputs(dt, 2, total, seed + dt, special=True)
    send = [S(0, k * region + 1, -1, 0, n, False, True, False) for k, n in enumerate(sizes)]
    fold = [S(0, k * region + 3, 1, k * region + 1 + 2 * (k & 1), n, True, True, False) for k, n in enumerate(sizes)]
    m0 = cases.MemberSpec(xs[0], None, [], [0], send)
    m1 = cases.MemberSpec(xs[1], _blank(total, dt), [0], [1], fold)
    return _case(dt, mg.SUM, 0, 4096, [3 * sps, 9 * sps], [m0, m1], sps, f"offset {mg.DT_NAMES[dt]}")


# ---- 5: one-ended connections -----------------------------------------------------------------------------
def one_ended_case(sps=2, seed=37) -> SimpleCase:
    """One member alone (the "run" form): recv-reduce-copy-send of 4 slices whose sender wrote them before
    (FIFO and tail words from the host) and whose receiver is elsewhere. 2-step slices of 2 KiB slots: a
    full slice is one tile, so with workgroupsPerMember = 2 workgroup 1 owns no tile at all."""
    dt = mg.I32
    sizes = [1024, 5, 0, 1000]
    offs = [0, 1024, 1029, 1029]
    total = 2030
    xs = mg.gen_inputs(dt, 2, total, seed, special=False)
    steps = [S(0, o, 1, o, n, True, True, False) for o, n in zip(offs, sizes)]
    member = cases.MemberSpec(xs[0], _blank(total, dt), [0], [1], steps)
    return _case(dt, mg.SUM, 0, 2048, [4 * sps, 10 * sps], [member], sps, "one-ended",
                 {0: [xs[1][o:o + n] for o, n in zip(offs, sizes)]})


# ---- 6: launch cuts ----------------------------------------------------------------------------------------
def cut_case(seed=41) -> SimpleCase:
    """100 slices (a cut at 96), and member 1 works IN PLACE on ranges that overlap earlier ones at other
    offsets (a cut at every such slice): slice k reads and writes [k * 40, k * 40 + 64) of its output."""
    dt = mg.U32
    n, stride, n_slices = 64, 40, 100
    total = stride * n_slices + n
    xs = mg.gen_inputs(dt, 2, total, seed, special=False)
    send = [S(0, k * stride, -1, 0, n, False, True, False) for k in range(n_slices)]
    fold = [S(1, k * stride, 1, k * stride, n, True, False, False) for k in range(n_slices)]
    m0 = cases.MemberSpec(xs[0], None, [], [0], send)
    m1 = cases.MemberSpec(None, xs[1], [0], [], fold)
    return _case(dt, mg.SUM, 0, 512, [8], [m0, m1], 1, "cuts")


def long_case(seed=43) -> SimpleCase:
    """130 slices with no conflict: one cut, at the 97th."""
    dt = mg.F32
    n, n_slices = 100, 130
    xs = mg.gen_inputs(dt, 2, n * n_slices, seed, special=False)
    send = [S(0, k * n, -1, 0, n, False, True, False) for k in range(n_slices)]
    fold = [S(0, k * n, 1, k * n, n, True, False, False) for k in range(n_slices)]
    m0 = cases.MemberSpec(xs[0], None, [], [0], send)
    m1 = cases.MemberSpec(xs[1], _blank(n * n_slices, dt), [0], [], fold)
    return _case(dt, mg.SUM, 0, 512, [16], [m0, m1], 1, "long")


# ---- 7: several workgroups a member ----------------------------------------------------------------------
def grid_case(seed=47) -> SimpleCase:
    """16 KiB slots, 2-step slices: 8 tiles a slice, so G = 8 by default; sizes leave workgroups without a
    tile (3 elements), give one workgroup two tiles under G = 2, and end inside a tile."""
    dt, sps, slot = mg.F16, 2, 16 << 10
    e = 2
    sizes = [slot * sps // e, 3, (5 * TILE + 18) // e, 0, TILE // e, slot * sps // e - 1] * 3
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offs[-1]) + 1
    xs = mg.gen_inputs(dt, 2, total, seed, special=True)
    send = [S(0, int(o), -1, 0, n, False, True, False) for o, n in zip(offs, sizes)]
    fold = [S(0, int(o), 1, int(o) + 1, n, True, False, False) for o, n in zip(offs, sizes)]
    m0 = cases.MemberSpec(xs[0], None, [], [0], send)
    m1 = cases.MemberSpec(xs[1], _blank(total, dt), [0], [], fold)
    return _case(dt, mg.SUM, 0, slot, [2], [m0, m1], sps, "grid")


# ---- 8: fork and shipped semantics ------------------------------------------------------------------------
def semantics_cases() -> List[SimpleCase]:
    """Signed min / max (what fork changes), PreMulSum and SumPostDiv (what shipped drops), and the fan
    (shipped: source 0 wins among four)."""
    return [chain_case(mg.I8, "min", n_slices=6), chain_case(mg.I32, "max", n_slices=6),
            chain_case(mg.F16, "premulsum", n_slices=6), chain_case(mg.I32, "sumpostdiv", n_slices=6),
            fan_case(mg.F32, "sum"), fan_case(mg.I64, "min")]


def all_cases() -> List[SimpleCase]:
    """Every step list the GPU file uses."""
    out = [pair_case(1), pair_case(2)]
    out += [chain_case(dt, name) for dt, name in CHAIN_PAIRS]
    out += [fan_case(dt, name) for dt, name in cases.STAR_PAIRS]
    out += [offset_case(mg.I8), offset_case(mg.F16)]
    out += [one_ended_case(), cut_case(), long_case(), grid_case()]
    return out
