"""TEST INFRASTRUCTURE ONLY — the sequential interpreter of SIMPLE step lists (tests/simple_steps_model.py,
imported, not edited) with DirectWrite connections, and the three direct ring schedules as step lists.

What nexrReduceCopySimpleStepsGroupDirect (include/nexr.h) must leave behind. A record carries `direct`
(nexrLLStep.pad[0]: bit 0 DirectRecv, bit 1 DirectSend); a member carries, per send connection, the member
whose OUTPUT a direct send writes into (None: the FIFO), and whether its one receive connection is direct.
An end is direct when both the record's bit and the connection say so (reference
src/device/prims_simple.h:148-164):
  - a direct send stores the slice at the receiver's output + dst_ix instead of the slot;
  - a direct receive reads the member's own output + dst_ix instead of the slot;
  - a direct receive with src_buf == -1 and dst_buf == 1 has source and destination at the same bytes
    (:258-269): nothing is stored to the output; a sending record copies the source to its send destinations
    bit for bit, any other moves no data.
Everything else is simple_steps_model's: the arithmetic is ``oracle.reduce_copy``, the counters advance by
step_per_slice per recv / send record whatever the slice's path, and every connection keeps its FIFO bytes
and the mask of the bytes WRITTEN, so that "a direct slice writes no FIFO byte" can be checked.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import numpy as np

import oracle
import simple_steps_model as model

Conn, StuckError, Result = model.Conn, model.StuckError, model.Result
DIRECT_RECV, DIRECT_SEND = 1, 2


class DStep(NamedTuple):
    """nexrLLStep with its direct bits (pad[0])."""
    src_buf: int = -1
    src_ix: int = 0
    dst_buf: int = -1
    dst_ix: int = 0
    n_elts: int = 0
    recv: bool = False
    send: bool = False
    post_op: bool = False
    direct: int = 0


class DMember:
    """One Primitives: simple_steps_model's Member plus its direct ends. send_direct[j]: the DMember whose
    output send connection j writes into (None: its FIFO); recv_direct: the receive connection is direct."""

    def __init__(self, input, output, recv: Sequence[Conn], send: Sequence[Conn], steps: Sequence[tuple],
                 send_direct: Optional[Sequence[Optional["DMember"]]] = None, recv_direct: bool = False):
        def as_bytes(a):
            return None if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
        self.output = as_bytes(output)
        self.input = self.output if input is output else as_bytes(input)   # the same object: in place
        self.recv, self.send = list(recv), list(send)
        self.steps = [DStep(*s) for s in steps]
        self.send_direct = list(send_direct) if send_direct is not None else [None] * len(self.send)
        self.recv_direct = bool(recv_direct)
        assert not self.recv_direct or (len(self.recv) == 1 and self.output is not None), "one direct receive"
        self.pos = 0

    def buf(self, which: int) -> Optional[np.ndarray]:
        return self.input if which == 0 else self.output if which == 1 else None


def _run_step(mb: DMember, st: DStep, esz: int, datatype: int, dev_red_op: int, red_op_arg: int) -> None:
    n_bytes = st.n_elts * esz
    recv = mb.recv if st.recv else []
    send = mb.send if st.send else []
    d_recv = bool(recv) and bool(st.direct & DIRECT_RECV) and mb.recv_direct
    targets = [mb.send_direct[j] if st.direct & DIRECT_SEND else None for j in range(len(send))]
    lo = st.dst_ix * esz
    out = np.zeros(0, dtype=np.uint8)
    if st.n_elts:
        srcs = []
        if st.src_buf >= 0:
            b = mb.buf(st.src_buf)
            assert b is not None and st.src_ix >= 0 and st.src_ix * esz + n_bytes <= b.size, "source out of range"
            srcs.append(b[st.src_ix * esz:st.src_ix * esz + n_bytes].copy())
        for i, c in enumerate(recv):
            if d_recv and i == 0:
                assert lo >= 0 and lo + n_bytes <= mb.output.size, "direct source out of range"
                srcs.append(mb.output[lo:lo + n_bytes].copy())
            else:
                srcs.append(c.slice_at(c.read, n_bytes).copy())
        assert srcs and (st.dst_buf >= 0 or send), "a slice needs a source and a destination"
        if d_recv and st.src_buf < 0 and st.dst_buf == 1:
            out = srcs[0]                                    # the skipped copy: bits, and nothing to the output
        else:
            pre = [red_op_arg] if st.src_buf == 0 else None
            (out,) = oracle.reduce_copy(srcs, 1, datatype, dev_red_op, red_op_arg, pre, bool(st.post_op))
            out = np.ascontiguousarray(out).view(np.uint8).reshape(-1)
            if st.dst_buf >= 0:
                b = mb.buf(st.dst_buf)
                assert b is not None and lo >= 0 and lo + n_bytes <= b.size, "destination out of range"
                b[lo:lo + n_bytes] = out
    for c, t in zip(send, targets):
        if t is None:
            c.write(out)
        else:
            if st.n_elts:
                assert lo >= 0 and lo + n_bytes <= t.output.size, "direct destination out of range"
                t.output[lo:lo + n_bytes] = out
            c.sent += c.sps
    for c in recv:
        c.read += c.sps
        c.head = c.read


def run(members: Sequence[DMember], datatype: int, dev_red_op: int, red_op_arg: int = 0) -> Result:
    """simple_steps_model.run with the direct rules: every member's slices to the end, round-robin."""
    esz = oracle.lib().oracle_type_size(int(datatype))
    if esz == 0:
        raise ValueError("bad datatype")
    conns: List[Conn] = []
    for mb in members:
        for c in mb.recv + mb.send:
            if not any(c is x for x in conns):
                conns.append(c)
    has_receiver = {id(c) for mb in members for c in mb.recv}

    def ready(mb, st) -> bool:
        if st.recv and any(c.sent < c.read + c.sps for c in mb.recv):
            return False
        if st.send and any(id(c) in has_receiver and c.sent + c.sps > c.read + c.n_slots for c in mb.send):
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
            _run_step(mb, mb.steps[mb.pos], esz, datatype, dev_red_op, red_op_arg)
            trace.append((m, mb.pos))
            mb.pos += 1
            progress = True
        if not progress:
            left = {m: mb.pos for m, mb in enumerate(members) if mb.pos < len(mb.steps)}
            raise StuckError(f"no member can take its next step (member: step index) {left}")
    return Result(list(members), conns, trace)


# ---- the direct ring schedules as step lists ------------------------------------------------------------------
def _div_up(a, b):
    return -(-a // b)


def slices(nelem: int, step_elts: int, sps: int, spc: int) -> List[int]:
    """genericOp's slices of one primitive call (prims_simple.h:199-201, :236): spc sizes, zeros included."""
    nelem = max(0, nelem)
    size = max(_div_up(nelem, 16 * spc) * 16, step_elts * sps // 32)
    out, off = [], 0
    for _ in range(spc):
        size = max(0, min(size, nelem - off))
        out.append(size)
        off += size
    return out


class Lists:
    """One rank's records, primitive by primitive, split into slices."""

    def __init__(self, step_elts, sps, spc, direct=True):
        self.step_elts, self.sps, self.spc, self.on = step_elts, sps, spc, direct
        self.steps: List[DStep] = []
        self.direct_recv_only = 0   # slices of directRecv calls (they move no data when direct)

    def op(self, recv, send, src_buf, dst_buf, src_ix, dst_ix, n, post=False, bits=0):
        off = 0
        for sz in slices(n, self.step_elts, self.sps, self.spc):
            self.steps.append(DStep(src_buf, src_ix + off if src_buf >= 0 else 0, dst_buf,
                                    dst_ix + off if (dst_buf >= 0 or (self.on and bits)) else 0, sz, recv, send, post,
                                    bits if self.on else 0))
            if recv and not send and src_buf < 0 and sz:
                self.direct_recv_only += 1
            off += sz

    # the reference's names (prims_simple.h:897-972)
    def direct_send(self, inp, out, n):
        self.op(False, True, 0, -1, inp, out, n, bits=DIRECT_SEND)

    def direct_copy_send(self, inp, out, n):
        self.op(False, True, 0, 1, inp, out, n, bits=DIRECT_SEND)

    def direct_recv_reduce_direct_send(self, inp, out, n):
        self.op(True, True, 0, -1, inp, out, n, bits=DIRECT_RECV | DIRECT_SEND)

    def direct_recv_reduce_copy_direct_send(self, inp, out, n, post):
        self.op(True, True, 0, 1, inp, out, n, post, bits=DIRECT_RECV | DIRECT_SEND)

    def direct_recv_copy_direct_send(self, out, n):
        self.op(True, True, -1, 1, 0, out, n, bits=DIRECT_RECV | DIRECT_SEND)

    def direct_recv(self, out, n):
        self.op(True, False, -1, 1, 0, out, n, bits=DIRECT_RECV)


def all_reduce_lists(n, count, esz, step_elts, sps=2, spc=2, direct=True) -> List[Lists]:
    """runRing of ncclAllReduce (all_reduce.h:12-84) on the direct* primitives, one channel."""
    ranks = [Lists(step_elts, sps, spc, direct) for _ in range(n)]
    chunk0 = step_elts * sps * spc
    for r, L in enumerate(ranks):
        chunk = chunk0
        for elem in range(0, count, n * chunk0):
            rem = count - elem
            if rem < n * chunk0:
                chunk = _div_up(_div_up(rem, n), 16 // esz) * (16 // esz)

            def at(c):
                return elem + c * chunk, min(chunk, rem - c * chunk)
            off, ne = at((r + n - 1) % n)
            L.direct_send(off, off, ne)
            for j in range(2, n):
                off, ne = at((r + n - j) % n)
                L.direct_recv_reduce_direct_send(off, off, ne)
            off, ne = at(r)
            L.direct_recv_reduce_copy_direct_send(off, off, ne, True)
            for j in range(1, n - 1):
                off, ne = at((r + n - j) % n)
                L.direct_recv_copy_direct_send(off, ne)
            off, ne = at((r + 1) % n)
            L.direct_recv(off, ne)
    return ranks


def all_gather_lists(n, per, step_elts, in_place, sps=2, spc=2, direct=True) -> List[Lists]:
    """runRing of ncclAllGather (all_gather.h:12-72): `per` elements a rank."""
    ranks = [Lists(step_elts, sps, spc, direct) for _ in range(n)]
    chunk = step_elts * sps * spc
    for r, L in enumerate(ranks):
        for elem in range(0, per, chunk):
            ne = min(chunk, per - elem)
            off = elem + r * per
            if in_place:
                L.direct_send(off, off, ne)       # the member's input IS its output: the same element offset
            else:
                L.direct_copy_send(elem, off, ne)
            for j in range(1, n - 1):
                L.direct_recv_copy_direct_send(elem + ((r + n - j) % n) * per, ne)
            L.direct_recv(elem + ((r + 1) % n) * per, ne)
    return ranks


def broadcast_lists(n, count, step_elts, root, in_place, direct=True) -> List[Lists]:
    """runRing of ncclBroadcast (broadcast.h:12-58): 1-step slices, one slice a chunk."""
    ranks = [Lists(step_elts, 1, 1, direct) for _ in range(n)]
    for r, L in enumerate(ranks):
        for off in range(0, count, step_elts):
            ne = min(step_elts, count - off)
            if r == root:
                (L.direct_send if in_place else L.direct_copy_send)(off, off, ne)
            elif (r + 1) % n == root:
                L.direct_recv(off, ne)
            else:
                L.direct_recv_copy_direct_send(off, ne)
    return ranks


def ring_members(lists: Sequence[Lists], inputs, outputs, slot_bytes, sps, start=0, direct=True, n_slots=8,
                 skip_conn_into=None):
    """The ranks of a ring as DMembers: conns[r] is the connection INTO rank r from rank r - 1, every one
    starting at `start`. direct: every connection direct. skip_conn_into: a rank whose incoming connection no
    record uses (the broadcast's root)."""
    n = len(lists)
    conns = [Conn(slot_bytes, n_slots, start, sps) for _ in range(n)]
    members = [DMember(inputs[r], outputs[r], [conns[r]], [conns[(r + 1) % n]], lists[r].steps, recv_direct=direct)
               for r in range(n)]
    if direct:
        for r, mb in enumerate(members):
            mb.send_direct = [members[(r + 1) % n]]
    return members, conns
