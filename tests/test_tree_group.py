"""CPU tests for the tree all-reduce in group launches (nexrTreeAllReduce under nexrRingCommSetLLGroup,
include/nexr_ring.h): the member set the tree builds, 2n - 1 Primitives a channel with up to 3 + 3
connections each, goes through the host side of both group calls (nexrReduceCopyLLStepsGroup,
nexrReduceCopyLL128StepsGroup) with made-up addresses. Every return code here comes before any device call:
the dry run's refusal (5, nexrInvalidUsage), the workspace check right behind the dry run (4,
nexrInvalidArgument) and, behind that, the residency refusal through the library's test hook (5)."""
import ctypes
import os

import pytest

from conftest import ROOT
from oracle.ring import tree_topology

F32 = 7
N_RANKS, N_STEPS = 8, 100
SLOT = 1 << 16
PER = {"ll": SLOT // 2 // 4, "ll128": SLOT // 2048 * 1920 // 4}   # fp32 elements of a full step
G = {"ll": 8, "ll128": 16}                                        # workgroups a member at 64 KiB slots
WS = 0x800000
# made-up device addresses: nothing here reaches the device
UP, DOWN, INPUT, OUTPUT = 0x10000000, 0x20000000, 0x100000000, 0x200000000


def _conn(base, rank):
    fifo = base + rank * 0x100000
    return (fifo, fifo + 8 * SLOT, 0)


def _tree_members(nexr, proto, n_steps=N_STEPS):
    """(rank, role, input, output, recv, send, steps) per member, with the connections and in the order
    nexrTreeAllReduce builds its Primitives: per rank the root once (receive from and send to every child),
    every other rank its reduce-up half (children -> parent) and then its broadcast-down half."""
    links = tree_topology(N_RANKS, 2, 0)
    per = PER[proto]
    out = []
    for r, (up, kids) in enumerate(links):
        leaf = not kids
        inp, outp = INPUT + r * 0x1000000, OUTPUT + r * 0x1000000
        offs = [k * per for k in range(n_steps)]
        if up == -1:
            steps = [nexr.ll_step(0, o, 1, o, per, recv=True, send=True, post_op=True) for o in offs]
            out.append((r, "root", inp, outp, [_conn(UP, c) for c in kids], [_conn(DOWN, c) for c in kids], steps))
            continue
        steps = [nexr.ll_step(0, o, -1, 0, per, recv=not leaf, send=True) for o in offs]
        out.append((r, "up", inp, outp, [_conn(UP, c) for c in kids], [_conn(UP, r)], steps))
        steps = [nexr.ll_step(-1, 0, 1, o, per, recv=True, send=not leaf) for o in offs]
        out.append((r, "down", inp, outp, [_conn(DOWN, r)], [_conn(DOWN, c) for c in kids], steps))
    return links, out


def _call(nexr, proto, members, ws_bytes):
    L = nexr.lib()
    n = len(members)
    cs = (nexr.LLConnSet * n)(*[nexr.ll_conn_set(i, o, r, s, SLOT, 8) for _k, _w, i, o, r, s, _st in members])
    arrs = [(nexr.LLStep * len(m[6]))(*m[6]) for m in members]
    ptrs = (ctypes.POINTER(nexr.LLStep) * n)(*[ctypes.cast(a, ctypes.POINTER(nexr.LLStep)) for a in arrs])
    counts = (ctypes.c_int * n)(*[len(m[6]) for m in members])
    if proto == "ll128":
        return L.nexrReduceCopyLL128StepsGroup(n, cs, ptrs, counts, F32, 0, 0, None, 0, ctypes.c_void_p(WS), ws_bytes,
                                               None)
    return L.nexrReduceCopyLLStepsGroup(n, cs, ptrs, counts, F32, 0, 0, None, None, 0, ctypes.c_void_p(WS), ws_bytes,
                                        None)


def test_the_member_set_is_the_trees(nexr):
    """tree_topology(8, 2, 0): 15 members, rank 4 with three children, so its reduce-up half receives on
    three connections and its broadcast-down half sends on three."""
    links, members = _tree_members(nexr, "ll", 1)
    assert len(members) == 2 * N_RANKS - 1
    assert len(links[4][1]) == 3 and links[4][0] != -1
    fans = {(r, role): (len(recv), len(send)) for r, role, _i, _o, recv, send, _s in members}
    assert fans[(4, "up")] == (3, 1) and fans[(4, "down")] == (1, 3)
    root = next(r for r, (up, _k) in enumerate(links) if up == -1)
    assert fans[(root, "root")] == (len(links[root][1]),) * 2
    # every connection has exactly one sender and one receiver among the members
    sends = sorted(c[0] for m in members for c in m[5])
    recvs = sorted(c[0] for m in members for c in m[4])
    assert sends == recvs and len(set(sends)) == len(sends) == 2 * (N_RANKS - 1)


@pytest.mark.parametrize("proto", ["ll", "ll128"])
def test_the_dry_run_accepts_a_tree_with_a_cut_inside(nexr, proto, monkeypatch):
    """100 steps a member are two launches (96 steps each at the most). With a workspace one region short
    the call returns nexrInvalidArgument: that check stands right behind the dry run, so the dry run took
    the set. With both regions the workspace passes too, and the next refusal is the residency check's
    (15 x G workgroups against room for one fewer, through the test hook): nexrInvalidUsage."""
    _links, members = _tree_members(nexr, proto)
    region = nexr.ll_group_workspace_bytes(len(members), 1)
    assert _call(nexr, proto, members, region) == 4
    assert _call(nexr, proto, members, 2 * region - 8) == 4
    monkeypatch.setenv("NEXR_TEST_LL_GROUP_RESIDENT", str(len(members) * G[proto] - 1))
    assert _call(nexr, proto, members, 2 * region) == 5
    assert _call(nexr, proto, members, region) == 4      # the workspace is looked at first


@pytest.mark.parametrize("proto", ["ll", "ll128"])
def test_the_dry_run_refuses_a_tree_whose_child_stops_reading(nexr, proto):
    """The same set, but the broadcast-down half of a leaf among rank 4's three children has 80 steps
    only: its parent's first launch sends 96, and the 89th needs the 81st read, which no step of that launch
    (or of any) gives. nexrInvalidUsage, whatever the workspace."""
    links, members = _tree_members(nexr, proto)
    child = next(c for c in links[4][1] if not links[c][1])
    short = [(r, role, i, o, rv, sd, st[:80] if (r, role) == (child, "down") else st)
             for r, role, i, o, rv, sd, st in members]
    assert sum(len(m[6]) for m in short) == 15 * N_STEPS - 20
    region = nexr.ll_group_workspace_bytes(len(short), 1)
    assert _call(nexr, proto, short, 2 * region) == 5
    assert _call(nexr, proto, short, 8) == 5
    # 92 reads are the fewest that let the parent send all 100: accepted again (the workspace's 4)
    ok = [(r, role, i, o, rv, sd, st[:92] if (r, role) == (child, "down") else st)
          for r, role, i, o, rv, sd, st in members]
    assert _call(nexr, proto, ok, 8) == 4


def test_the_header_describes_the_tree_option():
    hdr = open(os.path.join(ROOT, "include", "nexr_ring.h")).read()
    assert "The tree all-reduce is not affected" not in hdr
    text = " ".join(hdr.replace("*", " ").split())
    assert "2n - 1 members per channel" in text
    assert "nexrTreeAllReduce takes the option too" in text
