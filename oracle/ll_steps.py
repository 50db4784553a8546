"""TEST INFRASTRUCTURE ONLY — a sequential interpreter of LL step lists.

What nexrReduceCopyLLSteps[Rule] and nexrReduceCopyLLStepsGroup (include/nexr.h) must leave behind, worked
out one step at a time in plain Python: members (one Primitives each: user input and output, receive and
send connections, a list of nexrLLStep records) take turns, a member's next step runs once its lines are
there and its credits are free (reference src/device/prims_ll.h:55-83 waitSend / postRecv), as one
``oracle.reduce_copy_ll`` call (the C oracle's LLGenericOp, :218-283) with the flags of the connections'
own step counters, and a cleaning send step rewrites the rest of its slot (incSend, :85-93). No GPU and
nothing of nex-nccl_amd is used here: the arithmetic is the C oracle's, the rest is bookkeeping.

A connection both ends of which are members of the run is walked with its data and its credits. One that
only some member sends into has its receiver elsewhere: its credits are taken as free. One that a member
only receives from has its sender elsewhere: what that sender wrote is put there with ``Conn.prefill``
before the run (at most nSlots steps: nobody frees a slot), and a step that finds nothing is stuck.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import lib, make_ll_lines, reduce_copy_ll

PRODUCTION_RULE = (0, 0x7FFFFFF8)  # NCCL_LL_CLEAN_MASK with 32-bit flags (src/include/device.h:726-727)
TEST_RULE = (0x100, 0x78)          # TEST_LL_CLEANUP (:720-723)
LINE = 16                          # bytes of an LL line: {data, flag, data, flag}


def ll_flag(step: int, rule=None) -> int:
    """NCCL_LL_FLAG(step + 1) under the rule (flag_max, clean_mask): what the lines of step `step` carry."""
    flag_max = (rule or PRODUCTION_RULE)[0]
    a = int(step) + 1
    return a % flag_max if flag_max else a & 0xFFFFFFFF


def ll_cleans(step: int, rule=None) -> bool:
    """Whether send step `step` cleans its slot: (step & cleanMask) == cleanMask."""
    clean_mask = (rule or PRODUCTION_RULE)[1]
    return (int(step) & 0xFFFFFFFF & clean_mask) == clean_mask


class StuckError(RuntimeError):
    """The step lists cannot finish: every member with steps left waits for a line or a credit."""


class Step(NamedTuple):
    """The fields of nexrLLStep (buffers: 0 input, 1 output, -1 none; offsets in elements)."""
    src_buf: int = -1
    src_ix: int = 0
    dst_buf: int = -1
    dst_ix: int = 0
    n_elts: int = 0
    recv: bool = False
    send: bool = False
    post_op: bool = False


class Conn:
    """One connection: nSlots x slotBytes bytes of FIFO, `sent` and `read` (both start at the connection's
    step counter) and a flag rule. `mask` marks the FIFO bytes whose value is defined: what the FIFO was
    made with (zeros), the valid data bytes and all flag words of written lines, clean lines — not the
    padding data bytes of a step's partial last line."""

    def __init__(self, slot_bytes: int, n_slots: int = 8, step: int = 0, rule=None):
        assert slot_bytes > 0 and slot_bytes % LINE == 0 and n_slots > 0
        self.slot_bytes, self.n_slots, self.rule = int(slot_bytes), int(n_slots), rule or PRODUCTION_RULE
        self.start = self.sent = self.read = int(step)
        self.fifo = np.zeros(self.slot_bytes * self.n_slots, dtype=np.uint8)
        self.mask = np.ones(self.fifo.size, dtype=bool)
        self.cleaned: List[int] = []  # the send steps that cleaned

    def slot(self, step: int) -> np.ndarray:
        s = (int(step) % self.n_slots) * self.slot_bytes
        return self.fifo[s:s + self.slot_bytes]

    def _slot_mask(self, step: int) -> np.ndarray:
        s = (int(step) % self.n_slots) * self.slot_bytes
        return self.mask[s:s + self.slot_bytes]

    def write(self, lines: np.ndarray, n_bytes: int) -> None:
        """Send step `sent`: `lines` (16 B each, flags in place) carrying n_bytes data bytes go into slot
        sent % nSlots; a cleaning step makes the slot's other lines {0, f, 0, f}. Then sent += 1."""
        n_lines = (n_bytes + 7) // 8
        assert lines.size == n_lines * LINE <= self.slot_bytes
        slot, mask = self.slot(self.sent), self._slot_mask(self.sent)
        slot[:lines.size] = lines
        if n_lines:
            m = mask[:lines.size].reshape(n_lines, 4, 4)
            m[:, 1, :] = m[:, 3, :] = True                  # both flag words
            valid = np.arange(n_lines * 8) < n_bytes        # data bytes in line order: word 0, then word 2
            m[:, 0, :] = valid.reshape(n_lines, 2, 4)[:, 0, :]
            m[:, 2, :] = valid.reshape(n_lines, 2, 4)[:, 1, :]
        if ll_cleans(self.sent, self.rule):
            f = ll_flag(self.sent, self.rule)
            rest = slot[lines.size:].view(np.uint32).reshape(-1, 4)
            rest[:] = np.array([0, f, 0, f], dtype=np.uint32)
            mask[lines.size:] = True
            self.cleaned.append(self.sent)
        self.sent += 1

    def prefill(self, datas: Sequence[np.ndarray]) -> None:
        """The steps a sender outside the run has written: one send step per entry (raw data bytes, any
        dtype), encoded by make_ll_lines at this connection's flags."""
        for d in datas:
            raw = np.ascontiguousarray(d).view(np.uint8).reshape(-1)
            assert self.sent + 1 <= self.read + self.n_slots, "more steps than slots: nobody frees one"
            self.write(make_ll_lines(raw, ll_flag(self.sent, self.rule)), raw.size)


class Member:
    """One Primitives: input and output bytes (copied; None where it has none), its connections and steps."""

    def __init__(self, input, output, recv: Sequence[Conn], send: Sequence[Conn], steps: Sequence[Step]):
        def as_bytes(a):
            return None if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
        self.input, self.output = as_bytes(input), as_bytes(output)
        self.recv, self.send, self.steps = list(recv), list(send), [Step(*s) for s in steps]
        self.pos = 0

    def buf(self, which: int) -> Optional[np.ndarray]:
        return self.input if which == 0 else self.output if which == 1 else None


class Result(NamedTuple):
    members: List[Member]   # .input / .output: the final user bytes
    conns: List[Conn]       # every connection once, in order of first use: .fifo, .mask, .sent, .read, .cleaned
    trace: List[tuple]      # (member, step index, recv (slot, flag) per connection, send (slot, flag) per connection)


def _run_step(mb: Member, st: Step, esz: int, datatype: int, dev_red_op: int, red_op_arg: int) -> tuple:
    n_bytes = st.n_elts * esz
    n_lines = (n_bytes + 7) // 8
    recv = mb.recv if st.recv else []
    send = mb.send if st.send else []
    rinfo = [(c.read % c.n_slots, ll_flag(c.read, c.rule)) for c in recv]
    sinfo = [(c.sent % c.n_slots, ll_flag(c.sent, c.rule)) for c in send]
    if st.n_elts:
        src = None
        if st.src_buf >= 0:
            b = mb.buf(st.src_buf)
            assert b is not None and st.src_ix >= 0 and (st.src_ix * esz + n_bytes) <= b.size, "source out of range"
            src = b[st.src_ix * esz:st.src_ix * esz + n_bytes].copy()
        for c in recv + send:
            assert n_lines * LINE <= c.slot_bytes, "step larger than a slot"
        rc, dst, sends = reduce_copy_ll(src, st.src_buf == 0, [c.slot(c.read)[:n_lines * LINE] for c in recv],
                                        [f for _s, f in rinfo], st.dst_buf >= 0, len(send), [f for _s, f in sinfo],
                                        st.n_elts, datatype, dev_red_op, red_op_arg, bool(st.post_op))
        if rc != 0:
            raise ValueError(f"the oracle's LL step failed (rc={rc}: 3 is a line without its flag)")
        if st.dst_buf >= 0:
            b = mb.buf(st.dst_buf)
            assert b is not None and st.dst_ix >= 0 and (st.dst_ix * esz + n_bytes) <= b.size, "destination out of range"
            b[st.dst_ix * esz:st.dst_ix * esz + n_bytes] = dst
    else:
        sends = [np.zeros(0, dtype=np.uint8) for _ in send]
    for c, lines in zip(send, sends):
        c.write(lines, n_bytes)
    for c in recv:
        c.read += 1
    return rinfo, sinfo


def run(members: Sequence[Member], datatype: int, dev_red_op: int, red_op_arg: int = 0) -> Result:
    """Run every member's steps to the end, round-robin, one step at a time. Raises StuckError when no
    member can take its next step. The members and their connections are changed in place."""
    esz = lib().oracle_type_size(int(datatype))
    if esz == 0:
        raise ValueError("bad datatype")
    conns: List[Conn] = []
    for mb in members:
        for c in mb.recv + mb.send:
            if not any(c is x for x in conns):
                conns.append(c)
    has_receiver = {id(c) for mb in members for c in mb.recv}
    trace = []

    def ready(mb: Member, st: Step) -> bool:
        if st.recv and any(c.sent <= c.read for c in mb.recv):
            return False
        if st.send and any(id(c) in has_receiver and c.sent + 1 > c.read + c.n_slots for c in mb.send):
            return False
        return True

    for mb in members:
        mb.pos = 0
    while any(mb.pos < len(mb.steps) for mb in members):
        progress = False
        for m, mb in enumerate(members):
            if mb.pos >= len(mb.steps) or not ready(mb, mb.steps[mb.pos]):
                continue
            st = mb.steps[mb.pos]
            assert not (st.recv and not mb.recv) and not (st.send and not mb.send), "step without connections"
            rinfo, sinfo = _run_step(mb, st, esz, datatype, dev_red_op, red_op_arg)
            trace.append((m, mb.pos, rinfo, sinfo))
            mb.pos += 1
            progress = True
        if not progress:
            left = {m: mb.pos for m, mb in enumerate(members) if mb.pos < len(mb.steps)}
            raise StuckError(f"no member can take its next step (member: step index) {left}")
    return Result(list(members), conns, trace)
