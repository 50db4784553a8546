"""TEST INFRASTRUCTURE ONLY — a sequential interpreter of LL128 step lists.

What nexrReduceCopyLL128StepsGroup (include/nexr.h) must leave behind, worked out one step at a time in
plain Python: members (one Primitives each: user input and output, receive and send connections, a list of
nexrLLStep records) take turns; a member's next step runs once its lines are there and its credits are free
(reference src/device/prims_ll128.h:58-75 waitSend / postRecv) as ONE ``oracle.reduce_copy_ll128`` call
(the C oracle's literal restatement of :86-331) with the 64-bit flags step + 1 of the connections' own
counters. Nothing of nex-nccl_amd and no GPU is used: the arithmetic and the wire are the C oracle's, the
rest is bookkeeping. The step, member and error types are oracle/ll_steps.py's (the LL interpreter), so the
step lists of tests/ll_steps_cases.py run here unchanged.

Per connection it keeps the FIFO bytes, a mask of the bytes WRITTEN (every whole 2 KiB slice a send step
or a prefill put there: an LL128 step writes whole slices, padding included), the step counters `sent` and
`read`, and `head`, the step count the receiver has posted (what every head word of a wave that owns a
tile of the slot must hold in the end). There is no flag rule and no cleanup for LL128.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence

import numpy as np

import oracle
from oracle import ll_steps

Step, Member, StuckError = ll_steps.Step, ll_steps.Member, ll_steps.StuckError
SLICE, SLICE_DATA = 2048, 1920


def capacity(slot_bytes: int) -> int:
    """Data bytes a step may fill in a slot."""
    return slot_bytes // SLICE * SLICE_DATA


def slices_of(n_bytes: int) -> int:
    return -(-int(n_bytes) // SLICE_DATA)


class Conn:
    def __init__(self, slot_bytes: int, n_slots: int = 8, step: int = 0):
        assert slot_bytes > 0 and slot_bytes % SLICE == 0 and n_slots > 0
        self.slot_bytes, self.n_slots = int(slot_bytes), int(n_slots)
        self.start = self.sent = self.read = self.head = int(step)
        self.fifo = np.zeros(self.slot_bytes * self.n_slots, dtype=np.uint8)
        self.mask = np.zeros(self.fifo.size, dtype=bool)

    def slot(self, step: int) -> np.ndarray:
        s = (int(step) % self.n_slots) * self.slot_bytes
        return self.fifo[s:s + self.slot_bytes]

    def write(self, wire: np.ndarray) -> None:
        """Send step `sent`: whole slices with their flags in place go into slot sent % nSlots; sent += 1."""
        assert wire.size % SLICE == 0 and wire.size <= self.slot_bytes, "step larger than a slot"
        s = (self.sent % self.n_slots) * self.slot_bytes
        self.fifo[s:s + wire.size] = wire
        self.mask[s:s + wire.size] = True
        self.sent += 1

    def prefill(self, datas: Sequence[np.ndarray], datatype: int) -> None:
        """The steps a sender outside the run has written: one send step per entry (elements of `datatype`)."""
        for d in datas:
            assert self.sent + 1 <= self.read + self.n_slots, "more steps than slots: nobody frees one"
            d = np.ascontiguousarray(d)
            self.write(oracle.make_ll128_wire(d, self.sent + 1, datatype) if d.size
                       else np.zeros(0, dtype=np.uint8))


class Result(NamedTuple):
    members: List[Member]
    conns: List[Conn]
    trace: List[tuple]  # (member, step index)


def _run_step(mb: Member, st: Step, esz: int, datatype: int, dev_red_op: int, red_op_arg: int) -> None:
    n_bytes = st.n_elts * esz
    wire_bytes = slices_of(n_bytes) * SLICE
    recv = mb.recv if st.recv else []
    send = mb.send if st.send else []
    if st.n_elts:
        src = None
        if st.src_buf >= 0:
            b = mb.buf(st.src_buf)
            assert b is not None and st.src_ix >= 0 and st.src_ix * esz + n_bytes <= b.size, "source out of range"
            src = b[st.src_ix * esz:st.src_ix * esz + n_bytes].copy()
        for c in recv + send:
            assert wire_bytes <= c.slot_bytes, "step larger than a slot"
        rc, dst, sends = oracle.reduce_copy_ll128(src, st.src_buf == 0, [c.slot(c.read)[:wire_bytes].copy() for c in recv],
                                                  [c.read + 1 for c in recv], st.dst_buf >= 0, len(send),
                                                  [c.sent + 1 for c in send], st.n_elts, datatype, dev_red_op,
                                                  red_op_arg, bool(st.post_op))
        if rc != 0:
            raise ValueError(f"the oracle's LL128 step failed (rc={rc}: 3 is a line without its flag)")
        if st.dst_buf >= 0:
            b = mb.buf(st.dst_buf)
            assert b is not None and st.dst_ix >= 0 and st.dst_ix * esz + n_bytes <= b.size, "destination out of range"
            b[st.dst_ix * esz:st.dst_ix * esz + n_bytes] = dst
    else:
        sends = [np.zeros(0, dtype=np.uint8) for _ in send]
    for c, wire in zip(send, sends):
        c.write(wire)
    for c in recv:
        c.read += 1
        c.head = c.read


def run(members: Sequence[Member], datatype: int, dev_red_op: int, red_op_arg: int = 0) -> Result:
    """Run every member's steps to the end, round-robin, one step at a time. Raises StuckError when a step
    would wait for ever. The members and their connections are changed in place."""
    esz = oracle.lib().oracle_type_size(int(datatype))
    if esz == 0:
        raise ValueError("bad datatype")
    conns: List[Conn] = []
    for mb in members:
        for c in mb.recv + mb.send:
            if not any(c is x for x in conns):
                conns.append(c)
    has_receiver = {id(c) for mb in members for c in mb.recv}

    def ready(mb: Member, st: Step) -> bool:
        if st.recv and any(c.sent <= c.read for c in mb.recv):
            return False
        if st.send and any(id(c) in has_receiver and c.sent + 1 > c.read + c.n_slots for c in mb.send):
            return False
        return True

    trace = []
    for mb in members:
        mb.pos = 0
    while any(mb.pos < len(mb.steps) for mb in members):
        progress = False
        for m, mb in enumerate(members):
            if mb.pos >= len(mb.steps) or not ready(mb, mb.steps[mb.pos]):
                continue
            st = mb.steps[mb.pos]
            assert not (st.recv and not mb.recv) and not (st.send and not mb.send), "step without connections"
            _run_step(mb, st, esz, datatype, dev_red_op, red_op_arg)
            trace.append((m, mb.pos))
            mb.pos += 1
            progress = True
        if not progress:
            left = {m: mb.pos for m, mb in enumerate(members) if mb.pos < len(mb.steps)}
            raise StuckError(f"no member can take its next step (member: step index) {left}")
    return Result(list(members), conns, trace)


def model(case):
    """A tests/ll_steps_cases.py Case as LL128 interpreter objects: (members, conns), receive FIFOs pre-filled.
    The case's rule is ignored (LL128 has none)."""
    import ll_steps_cases as cases
    conns = [Conn(case.slot_bytes, cases.SLOTS, s) for s in case.conn_start]
    for i, datas in case.prefill.items():
        conns[i].prefill(datas, case.dt)
    members = [Member(m.input, m.output, [conns[i] for i in m.recv], [conns[i] for i in m.send], m.steps)
               for m in case.members]
    return members, conns


def ring_chunk(buff_bytes: int, esz: int) -> int:
    """Elements per LL128 ring chunk (src/enqueue.cc:1997-1999: stepBytes / 16 * 15 on the 1920-byte grain)."""
    return (buff_bytes // 8) // 16 * 15 // SLICE_DATA * SLICE_DATA // esz


def ring_allreduce_steps(n: int, rank: int, count: int, chunk: int, esz: int) -> List[Step]:
    """Rank `rank`'s step list of the one-channel ring all-reduce (runRing, all_reduce.h:17-79), one FIFO step
    per primitive: send, recvReduceSend x (n - 2), recvReduceCopySend (post-op), recvCopySend x (n - 2), recv."""
    steps = []
    loop = n * chunk
    for elem_off in range(0, count, loop):
        rem = count - elem_off
        if rem < loop:
            chunk = -(-(-(-rem // n)) // (16 // esz)) * (16 // esz)

        def at(c):
            return elem_off + c * chunk, max(0, min(chunk, rem - c * chunk))

        o, m = at((rank + n - 1) % n)
        steps.append(Step(0, o, -1, 0, m, False, True, False))
        for j in range(2, n):
            o, m = at((rank + n - j) % n)
            steps.append(Step(0, o, -1, 0, m, True, True, False))
        o, m = at(rank)
        steps.append(Step(0, o, 1, o, m, True, True, True))
        for j in range(1, n - 1):
            o, m = at((rank + n - j) % n)
            steps.append(Step(-1, 0, 1, o, m, True, True, False))
        o, m = at((rank + 1) % n)
        steps.append(Step(-1, 0, 1, o, m, True, False, False))
    return steps
