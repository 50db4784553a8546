"""The step lists of the LL step matrix (tests/test_ll_steps_matrix_gpu.py), as data: which datatypes and ops
it covers, and for every case the members, connections and nexrLLStep records — once, so that the
interpreter (oracle/ll_steps.py) and the device calls are given the same thing, and so that a CPU test
(tests/test_ll_steps_model.py) can run every list through the interpreter and count the parametrisation
without a GPU. Nothing here touches the GPU or the library under test."""
from typing import List, NamedTuple, Optional

import numpy as np

import make_golden as mg
from oracle import ll_steps

SLOTS = 8
TEST_RULE = (0x100, 0x78)
FILL = 0x5A  # guard bytes round the user buffers

DTYPES = sorted(mg.DT_NAMES)
# (nRecv, nSend) of case A
PEERS = [(0, 1), (1, 0), (1, 1), (2, 1), (1, 2), (3, 0), (0, 3), (3, 3)]
ENTRY_POINTS = ("run", "group")
# every connection starts at a counter of its own: no two of a member's share a slot index or a flag
RECV_START = (5, 14, 23)
SEND_START = (3, 9, 16)


def ops_for(dt):
    """(name, devRedOp, redOpArg) — the op set of test_ll_gpu.py::test_ll_all_ops_and_shapes: SumPostDiv for
    the integers only (the API refuses it for floats), its steps with the post-op."""
    ops = [("sum", mg.SUM, 0), ("prod", mg.PROD, 0), ("min", mg.MINMAX, mg.minmax_arg(dt, False)),
           ("max", mg.MINMAX, mg.minmax_arg(dt, True)),
           ("premulsum", mg.PREMULSUM, mg.float_scalar_bits(dt, 0.5 if dt not in mg.INTS else 3))]
    if dt in mg.INTS:
        ops.append(("sumpostdiv", mg.SUMPOSTDIV, (3 << 1) | int(dt in (mg.I8, mg.I32, mg.I64))))
    return ops


OP_NAMES = ("sum", "prod", "min", "max", "premulsum", "sumpostdiv")
# (datatype, op name) of case B: every pair the API accepts (56)
STAR_PAIRS = [(dt, name) for dt in DTYPES for name, _op, _arg in ops_for(dt)]


def op_named(dt, name):
    return next(o for o in ops_for(dt) if o[0] == name)


class MemberSpec(NamedTuple):
    input: Optional[np.ndarray]    # initial user bytes (storage dtype), None: the member has no such buffer
    output: Optional[np.ndarray]
    recv: List[int]                # indices into Case.conn_start
    send: List[int]
    steps: List[ll_steps.Step]


class Case(NamedTuple):
    dt: int
    op: int
    arg: int
    slot_bytes: int
    rule: Optional[tuple]
    conn_start: List[int]          # a connection's step counter at the start
    prefill: dict                  # connection index -> the data of the steps a sender outside has written
    members: List[MemberSpec]


def esz_of(dt):
    return np.dtype(mg.STORE[dt]).itemsize


def model(case: Case):
    """The case as interpreter objects: (members, conns), receive FIFOs pre-filled."""
    conns = [ll_steps.Conn(case.slot_bytes, SLOTS, s, case.rule) for s in case.conn_start]
    for i, datas in case.prefill.items():
        conns[i].prefill(datas)
    members = [ll_steps.Member(m.input, m.output, [conns[i] for i in m.recv], [conns[i] for i in m.send], m.steps)
               for m in case.members]
    return members, conns


# ---- A: one member alone, its peers pre-filled ---------------------------------------------------------
def alone_sizes(dt):
    """Step sizes in bytes: one element; a partial last line (types under 8 bytes); one element short of 64
    lines, 64 lines (lanes j and j + 64 of a wave), 65; 128 lines and an element (a second wave); the full
    2048 data bytes of a 4 KiB slot. Cycled over the 8 steps."""
    e = esz_of(dt)
    return [e, 24 + e if e < 8 else 24, 64 * 8 - e, 64 * 8, 65 * 8, 128 * 8 + e, 2048]


def alone_case(dt, op, arg, n_recv, n_send, seed) -> Case:
    """8 steps of one member with n_recv + n_send connections at 4 KiB slots, every step on all of them.
    The source cycles through input, nothing (where there is a peer) and output (no pre-op), the
    destination through output, nothing (where it sends) and input; the post-op is set on every second
    step; srcIx and dstIx are odd on every other step (on different ones)."""
    e = esz_of(dt)
    sizes = alone_sizes(dt)
    region = 2048 // e + 2  # even: a step's elements and room for the odd offsets
    total = 8 * region
    bufs = mg.gen_inputs(dt, 2 + n_recv, total, seed, special=True)
    src_cycle = [0, -1, 0, 1, 0, -1, 1, 0] if n_recv else [0, 0, 1, 0, 0, 1, 0, 0]
    dst_cycle = [1, -1, 0, 1, -1, 1, 0, 1] if n_send else [1, 1, 0, 1, 1, 1, 0, 1]
    steps, peer_data = [], [[] for _ in range(n_recv)]
    for k in range(8):
        n = sizes[k % len(sizes)] // e
        src_buf, dst_buf = src_cycle[k], dst_cycle[k]
        src_ix = k * region + (k & 1)
        dst_ix = src_ix if src_buf == dst_buf else k * region + ((k >> 1) & 1)
        steps.append(ll_steps.Step(src_buf, src_ix, dst_buf, dst_ix, n, n_recv > 0, n_send > 0, k % 2 == 0))
        for i in range(n_recv):
            peer_data[i].append(bufs[2 + i][k * region:k * region + n])
    conn_start = list(RECV_START[:n_recv]) + list(SEND_START[:n_send])
    member = MemberSpec(bufs[0], bufs[1], list(range(n_recv)), list(range(n_recv, n_recv + n_send)), steps)
    return Case(dt, op, arg, 4096, None, conn_start, {i: peer_data[i] for i in range(n_recv)}, [member])


# ---- B, C, E: a star -----------------------------------------------------------------------------------
def star_case(dt, op, arg, slot_bytes, sizes, seed, n_leaves=3, rule=None, conn_start=None, lockstep=False) -> Case:
    """n_leaves leaves send a piece of their input to the hub; the hub does recvReduceCopySend on all its
    connections (its own input the last operand, the post-op set) and every leaf copies the result to its
    output: per piece, a leaf's steps are send k, recv k. sizes: elements per piece. Connections 0 ..
    n_leaves - 1 are leaf -> hub, the rest hub -> leaf. lockstep: the hub takes a step that does nothing
    beside every leaf's send, so that hub and leaves reach piece k at the same step index (a group call
    ends a launch at the same index for every member)."""
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offs[-1])
    xs = mg.gen_inputs(dt, 1 + n_leaves, total, seed, special=True)
    fill = mg.STORE[dt]
    hub_steps, leaf_steps = [], []
    for k, n in enumerate(sizes):
        o = int(offs[k])
        if lockstep:
            hub_steps.append(ll_steps.Step())
        hub_steps.append(ll_steps.Step(0, o, 1, o, n, True, True, True))
        leaf_steps.append(ll_steps.Step(0, o, -1, 0, n, False, True, False))
        leaf_steps.append(ll_steps.Step(-1, 0, 1, o, n, True, False, False))
    if conn_start is None:
        conn_start = [(RECV_START + (30, 39))[i] for i in range(n_leaves)] + \
                     [(SEND_START + (28, 33))[i] for i in range(n_leaves)]
    blank = np.full(total * esz_of(dt), FILL, dtype=np.uint8).view(fill)
    members = [MemberSpec(xs[0], blank.copy(), list(range(n_leaves)), list(range(n_leaves, 2 * n_leaves)), hub_steps)]
    for i in range(n_leaves):
        members.append(MemberSpec(xs[1 + i], blank.copy(), [n_leaves + i], [i], list(leaf_steps)))
    return Case(dt, op, arg, slot_bytes, rule, list(conn_start), {}, members)


def star_sizes(dt, slot_bytes, n_steps=11):
    """A full slot alternating with a third of one (a partial last line for the 2-byte types at 4 KiB)."""
    e = esz_of(dt)
    data = slot_bytes // 2
    return [data // e if k % 2 == 0 else data // 3 // e for k in range(n_steps)]


GEOMETRY_SLOTS = {"g3": 24 << 10,                         # three tiles of 512 lines: G = 3
                  "cap": (1 << 20) + (8 << 10) + 48}      # 130 tiles on the 64-workgroup cap: workgroup 0 takes
#                                                           three of them, the last tile has 3 lines
GEOMETRY_PAIRS = [(mg.BF16, "sum"), (mg.I8, "min")]

CLEAN_HUB_START = (0x70, 0x74, 0x7a)   # hub -> leaf: clean at the hub's pieces 8-15, 4-11 and 0-5
CLEAN_LEAF_START = (0x10, 0x7c, 0x75)  # leaf -> hub: never, at pieces 0-3, at pieces 3-10


def clean_case(seed=41) -> Case:
    """E: the star under {0x100, 0x78}, fp32 Sum, 24 pieces of a full 4 KiB slot or 3 lines (swapped at every
    wrap of the 8 slots, so that every slot holds both in turn and a cleaning 3-line step has a full
    step's stale lines behind it)."""
    full, small = 4096 // 2 // 4, 6
    sizes = [full if (k + k // SLOTS) % 2 == 0 else small for k in range(24)]
    return star_case(mg.F32, mg.SUM, 0, 4096, sizes, seed, rule=TEST_RULE,
                     conn_start=CLEAN_LEAF_START + CLEAN_HUB_START, lockstep=True)


# ---- D: buffer routing in one list ---------------------------------------------------------------------
ROUTING_PAIRS = [(mg.F16, "premulsum"), (mg.I32, "sumpostdiv")]


def routing_case(dt, op, arg, seed) -> Case:
    """A hub and two leaves at 4 KiB slots, in lockstep (leaf: send, recv; hub: a step beside the leaves'
    send, then its recv + send), six rounds:
      0  data: everything from the input to the output, no post-op;
      1  zero elements: leaf send / recv, hub recv + send in one step;
      2  the source is the OUTPUT (round 0's results: no pre-op on them) and the destination the INPUT,
         the post-op set;
      3  zero elements: the hub's recv and send as two steps;
      4  data from the inputs round 2 wrote, to the output at another offset (it overlaps round 0's: the
         library must end the launch there), no post-op;
      5  the leaves send their output and the hub has no source (the two peers' lines reduced without a
         local operand), the post-op set."""
    e = esz_of(dt)
    n = 2048 // e - 23
    total = 2 * n + 64
    xs = mg.gen_inputs(dt, 6, total, seed, special=True)
    S = ll_steps.Step
    a, b = 1, 2 * (n // 3) + 1  # two odd element offsets, the ranges [a, a + n) and [b, b + n) overlapping
    hub = [S(), S(0, a, 1, a, n, True, True, False),
           S(), S(-1, 0, -1, 0, 0, True, True, False),
           S(), S(1, a, 0, a, n, True, True, True),
           S(-1, 0, -1, 0, 0, True, False, False), S(-1, 0, -1, 0, 0, False, True, False),
           S(), S(0, a, 1, b, n, True, True, False),
           S(), S(-1, 0, 1, a, n, True, True, True)]
    leaf = [S(0, a, -1, 0, n, False, True), S(-1, 0, 1, a, n, True, False),
            S(-1, 0, -1, 0, 0, False, True), S(-1, 0, -1, 0, 0, True, False),
            S(1, a, -1, 0, n, False, True), S(-1, 0, 0, a, n, True, False),
            S(-1, 0, -1, 0, 0, False, True), S(-1, 0, -1, 0, 0, True, False),
            S(0, a, -1, 0, n, False, True), S(-1, 0, 1, b, n, True, False),
            S(1, b, -1, 0, n, False, True), S(-1, 0, 1, a, n, True, False)]
    members = [MemberSpec(xs[0], xs[3], [0, 1], [2, 3], hub),
               MemberSpec(xs[1], xs[4], [2], [0], list(leaf)),
               MemberSpec(xs[2], xs[5], [3], [1], list(leaf))]
    return Case(dt, op, arg, 4096, None, [5, 14, 3, 9], {}, members)


# ---- G: the arithmetic edge pairs through one member's run ------------------------------------------------
def edge_pairs_case(dt, op, arg, peer, src, slot_bytes) -> Case:
    """One member, one receive connection pre-filled with `peer` and one send connection: recvReduceCopySend
    of `src` (the user input, to the output at the same offsets) in full-slot steps and a last step with
    what is left, at most SLOTS of them (nobody frees a pre-filled slot). For tests/test_arith_edges*.py:
    `peer` and `src` are the two operand vectors of tests/arith_edges.py's pair layout, any integer dtype of
    the element's width."""
    e = esz_of(dt)
    n = int(src.size)
    assert peer.size == n and peer.itemsize == e and src.itemsize == e
    per = slot_bytes // 2 // e
    steps, pieces = [], []
    for o in range(0, n, per):
        m = min(per, n - o)
        steps.append(ll_steps.Step(0, o, 1, o, m, True, True, False))
        pieces.append(peer[o:o + m])
    assert len(steps) <= SLOTS
    blank = np.full(n * e, FILL, dtype=np.uint8).view(src.dtype)
    member = MemberSpec(src, blank, [0], [1], steps)
    return Case(dt, op, arg, slot_bytes, None, [RECV_START[0], SEND_START[0]], {0: pieces}, [member])
