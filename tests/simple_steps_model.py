"""TEST INFRASTRUCTURE ONLY — a sequential interpreter of SIMPLE step lists.

What nexrReduceCopySimpleStepsGroup (include/nexr.h) must leave behind, worked out one slice at a time in
plain Python: members (one Primitives each: user input and output, receive and send connections, a list of
nexrLLStep records, each ONE SLICE of genericOp) take turns; a member's next slice runs once its tails are
there and its credits are free (reference src/device/prims_simple.h:111-188 waitPeer / postPeer) as ONE
``oracle.reduce_copy`` call (the C oracle's reduceCopy) with srcs = [user src, the receive slots...] and as
many destinations as the slice has, the pre-op on source 0 when it is the user input. Nothing of
nex-nccl_amd and no GPU is used: the arithmetic is the C oracle's, the rest is bookkeeping. The step, member
and error types are oracle/ll_steps.py's (the LL interpreter).

Per connection it keeps the FIFO bytes, a mask of the bytes WRITTEN (SIMPLE data has no flags and no
padding: a slice writes its nElts * size bytes and nothing else), the step counters `sent` and `read`, and
`head`, the step count the receiver has posted. A recv or send slice advances the counters by
step_per_slice and may fill that many consecutive slots; a slice of zero elements only advances.
"""
from __future__ import annotations

from typing import List, NamedTuple, Sequence

import numpy as np

import oracle
from oracle import ll_steps

Step, Member, StuckError = ll_steps.Step, ll_steps.Member, ll_steps.StuckError
TILE = 4096          # tile t of a slice belongs to workgroup t % G
MAX_GRID = 256       # NEXR_SIMPLE_GROUP_MAX_GRID
CREDIT_BYTES = 4096  # NEXR_SIMPLE_CREDIT_BYTES
CREDIT_STRIDE = 16   # one 8-byte word per workgroup


def default_grid(slot_bytes: int, step_per_slice: int) -> int:
    """G for workgroupsPerMember = 0."""
    return min(MAX_GRID, -(-(slot_bytes * step_per_slice) // TILE))


class Conn:
    def __init__(self, slot_bytes: int, n_slots: int = 8, step: int = 0, step_per_slice: int = 1):
        assert slot_bytes > 0 and slot_bytes % 16 == 0 and n_slots > 0
        assert step_per_slice >= 1 and n_slots % step_per_slice == 0 and step % step_per_slice == 0
        self.slot_bytes, self.n_slots, self.sps = int(slot_bytes), int(n_slots), int(step_per_slice)
        self.start = self.sent = self.read = self.head = int(step)
        self.fifo = np.zeros(self.slot_bytes * self.n_slots, dtype=np.uint8)
        self.mask = np.zeros(self.fifo.size, dtype=bool)

    def slice_at(self, step: int, n_bytes: int) -> np.ndarray:
        assert n_bytes <= self.slot_bytes * self.sps, "slice larger than its slots"
        s = (int(step) % self.n_slots) * self.slot_bytes
        assert s + n_bytes <= self.fifo.size, "a slice wraps the FIFO"
        return self.fifo[s:s + n_bytes]

    def write(self, data: np.ndarray) -> None:
        """Send slice `sent`: its bytes go to slot sent % nSlots onwards; sent += step_per_slice."""
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self.slice_at(self.sent, data.size)[:] = data
        s = (self.sent % self.n_slots) * self.slot_bytes
        self.mask[s:s + data.size] = True
        self.sent += self.sps

    def prefill(self, datas: Sequence[np.ndarray]) -> None:
        """The slices a sender outside the run has written: one send slice per entry."""
        for d in datas:
            assert self.sent + self.sps <= self.read + self.n_slots, "more slices than slots: nobody frees one"
            self.write(d)


class Result(NamedTuple):
    members: List[Member]
    conns: List[Conn]
    trace: List[tuple]  # (member, step index)


def _run_step(mb: Member, st: Step, esz: int, datatype: int, dev_red_op: int, red_op_arg: int) -> None:
    n_bytes = st.n_elts * esz
    recv = mb.recv if st.recv else []
    send = mb.send if st.send else []
    if st.n_elts:
        srcs = []
        if st.src_buf >= 0:
            b = mb.buf(st.src_buf)
            assert b is not None and st.src_ix >= 0 and st.src_ix * esz + n_bytes <= b.size, "source out of range"
            srcs.append(b[st.src_ix * esz:st.src_ix * esz + n_bytes].copy())
        srcs += [c.slice_at(c.read, n_bytes).copy() for c in recv]
        assert srcs and (st.dst_buf >= 0 or send), "a slice needs a source and a destination"
        pre = [red_op_arg] if st.src_buf == 0 else None   # PreOpSrcs = SrcBuf != Input ? 0 : 1
        (out,) = oracle.reduce_copy(srcs, 1, datatype, dev_red_op, red_op_arg, pre, bool(st.post_op))
        out = np.ascontiguousarray(out).view(np.uint8).reshape(-1)
        if st.dst_buf >= 0:
            b = mb.buf(st.dst_buf)
            assert b is not None and st.dst_ix >= 0 and st.dst_ix * esz + n_bytes <= b.size, "destination out of range"
            b[st.dst_ix * esz:st.dst_ix * esz + n_bytes] = out
    else:
        out = np.zeros(0, dtype=np.uint8)
    for c in send:
        c.write(out)
    for c in recv:
        c.read += c.sps
        c.head = c.read


def run(members: Sequence[Member], datatype: int, dev_red_op: int, red_op_arg: int = 0) -> Result:
    """Run every member's slices to the end, round-robin, one at a time. Raises StuckError when a slice
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
        if st.recv and any(c.sent < c.read + c.sps for c in mb.recv):           # tail >= step + StepPerSlice
            return False
        if st.send and any(id(c) in has_receiver and c.sent + c.sps > c.read + c.n_slots for c in mb.send):
            return False                                                       # head + NCCL_STEPS >= step + StepPerSlice
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


def model(case, step_per_slice: int = 1):
    """A tests/ll_steps_cases.py Case as SIMPLE interpreter objects: (members, conns), receive FIFOs
    pre-filled. The case's rule is ignored (SIMPLE has none)."""
    import ll_steps_cases as cases
    conns = [Conn(case.slot_bytes, cases.SLOTS, s, step_per_slice) for s in case.conn_start]
    for i, datas in case.prefill.items():
        conns[i].prefill(datas)
    members = [Member(m.input, m.output, [conns[i] for i in m.recv], [conns[i] for i in m.send], m.steps)
               for m in case.members]
    return members, conns
