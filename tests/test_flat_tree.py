"""The flat tree all-reduce and broadcast without a GPU. include/nexr.h states the tree all-reduce as a program over
the channel's tree (LEAF / JOIN / PUSH / MERGE); tests/flat_tree_cases.py restates the compiler and interprets the
program with the oracle's three step functions, and here that must give exactly what oracle/ring.py's recursive
restatement (tree_allreduce_expected_channels, one K-source step per rank) gives: three protocols, 2 / 3 / 4 / 5 /
8 / 9 ranks, every ranks-per-node of {n, 1, 2}, both trees of the double binary tree, 1 / 2 channels, counts round
a pack, a 2048-byte piece and a channel cell, on inputs whose result depends on the fold order (asserted). Then the
live-value count of every topology up to 64 ranks, the argument checks of nexrFlatTreeAllReduce /
nexrFlatBroadcast and of the ring library's entries, the symbols, and the code-object metadata: no flat tree kernel
may use scratch."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

import arith_edges as ae
import flat_cases as fc
import flat_tree_cases as ftc
import ring_modes_cases as rm
import test_code_objects as tco
from oracle import ring as oring

SEED = rm.SEED
RANKS = (2, 3, 4, 5, 8, 9)
CELL = {"simple": 8192, "ll": 2048, "ll128": 8192}   # bytes of a channel cell (16 KiB of traffic at 2 or 8 a byte)


def per_nodes(n):
    return [p for p in (n, 1, 2) if n % p == 0 and (p != 2 or n > 2)]


def counts_of(protocol, esz):
    """1, 3, a pack +- 1, a 2048-byte piece +- 1 element, one cell +- 1, two cells + 3, and 0."""
    p, piece, cell = 16 // esz, 2048 // esz, CELL[protocol] // esz
    out = []
    for c in (1, 3, p - 1, p + 1, piece - 1, piece + 1, cell - 1, cell + 1, 2 * cell + 3, 0):
        if c >= 0 and c not in out:
            out.append(c)
    return out


def links_of_channel(n, per_node, tree_index, channels):
    """The channel's tree as nexrRingCommCreate gives it: the upper half of 2+ channels runs the other tree."""
    def links_of(ch):
        return oring.tree_topology(n, per_node, (tree_index + (1 if channels >= 2 and ch >= channels // 2 else 0)) % 2)
    return links_of


def tree_parts(protocol, channels, count, esz, links_of):
    """(trees, parts) as nexrFlatTreeAllReduce takes them: the distinct trees of the parts' channels and
    (offset, count, tree) in elements."""
    trees, parts = [], []
    for ch, off, cnt in oring.channel_parts(channels, count, esz, 2, ll=protocol == "ll"):
        links = links_of(ch)
        if links not in trees:
            trees.append(links)
        parts.append((off, cnt, trees.index(links)))
    return trees, parts


def step_of(oracle, protocol, dt, op, n):
    """flat_tree_cases' step function from the oracle's reduce-copy of `protocol`: SIMPLE folds left from the
    first source (the user input with its pre-op where the step has one); LL / LL128 take the wire lines of
    `vals` as peers, every peer the first operand."""
    dev_op, arg = oracle.host_to_dev_red_op(op, dt, n)
    if protocol == "simple":
        def step(x, vals, post):
            srcs = ([x] if x is not None else []) + list(vals)
            return oracle.reduce_copy(srcs, 1, dt, dev_op, arg, [arg] if x is not None else [], post)[0]
        return step
    fn = oracle.reduce_copy_ll if protocol == "ll" else oracle.reduce_copy_ll128

    def step(x, vals, post):
        size = x.size if x is not None else vals[0][1]
        rc, dst, sends = fn(x, x is not None, [v for v, _ in vals], [1] * len(vals), post, 1, [1], size, dt, dev_op,
                            arg, post)
        assert rc == 0
        return dst.view(ae.UINT[dt]) if post else (sends[0], size)
    return step


def model_outputs(oracle, inputs, protocol, channels, dt, op, links_of):
    n, count = len(inputs), inputs[0].size
    if count == 0:
        return [x.copy() for x in inputs]
    trees, parts = tree_parts(protocol, channels, count, inputs[0].itemsize, links_of)
    return ftc.model(inputs, parts, trees, step_of(oracle, protocol, dt, op, n))


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))


# ---- the program against the recursive oracle ------------------------------------------------------------------
@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_program_is_the_oracles_tree(oracle, protocol, n):
    k = 0
    arities = set()
    for per_node in per_nodes(n):
        for tree_index in (0, 1):
            for channels in (1, 2):
                links_of = links_of_channel(n, per_node, tree_index, channels)
                arities |= {len(d) for _u, d in links_of(0)}
                for slot in range(10):
                    dt, op = rm.PAIRS[k % len(rm.PAIRS)]
                    cs = counts_of(protocol, rm.esz_of(dt))
                    count = cs[slot % len(cs)]
                    rng = np.random.default_rng([SEED, k, count])
                    xs = fc.gen_inputs(rng, dt, n, count)
                    want = oring.tree_allreduce_expected_channels(xs, dt, op, links_of, channels, protocol)
                    same(model_outputs(oracle, xs, protocol, channels, dt, op, links_of), want)
                    k += 1
    if n == 8:
        assert 3 in arities   # 2 per node: a node head with its chain successor and two tree children


def test_second_channel_holds_one_element():
    for protocol in rm.PROTO_ID:
        parts = oring.channel_parts(2, CELL[protocol] // 4 + 1, 4, 2, ll=protocol == "ll")
        assert [c for _ch, _o, c in parts] == [CELL[protocol] // 4, 1]


def test_known_programs():
    L, J, P, M = ftc.LEAF, ftc.JOIN, ftc.PUSH, ftc.MERGE
    chain = oring.tree_topology(3)                      # 0 <- 1 <- 2
    assert ftc.compile_tree(chain) == [(L, 2), (J, 1), (J, 0)]
    assert ftc.encode(ftc.compile_tree(chain)) == bytes([2, 0x41, 0x40])
    four = oring.tree_topology(4, 1, 0)                 # 0 <- 2 <- {1, 3}
    assert four == [(-1, [2]), (2, []), (0, [1, 3]), (2, [])]
    assert ftc.compile_tree(four) == [(L, 1), (J, 2), (P, 0), (L, 3), (M, 0), (J, 0)]
    assert ftc.live_values(ftc.compile_tree(four)) == 2 and ftc.live_values(ftc.compile_tree(chain)) == 1


# ---- the inputs -----------------------------------------------------------------------------------------------------
def _expected(xs, dt, op, links, protocol):
    return ae.canon(dt, oring.tree_allreduce_expected(xs, dt, op, links, protocol)[0])


@pytest.mark.parametrize("n", [n for n in RANKS if n >= 4])
@pytest.mark.parametrize("op", [rm.SUM, rm.PROD], ids=["sum", "prod"])
@pytest.mark.parametrize("dt", ae.FLOATS, ids=[ae.NAMES[d] for d in ae.FLOATS])
@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
def test_inputs_depend_on_the_child_order(oracle, protocol, dt, op, n):
    """With two children of one rank swapped, at least one expected element changes: a program that folds the
    children in another order cannot pass on these inputs."""
    links = oring.tree_topology(n, 1, 0)
    r = next(r for r, (_u, d) in enumerate(links) if len(d) >= 2)
    swapped = list(links)
    swapped[r] = (links[r][0], [links[r][1][1], links[r][1][0]] + links[r][1][2:])
    xs = fc.gen_inputs(np.random.default_rng([SEED, n, dt, op]), dt, n, 512)
    assert not np.array_equal(_expected(xs, dt, op, links, protocol), _expected(xs, dt, op, swapped, protocol))


@pytest.mark.parametrize("n", [n for n in RANKS if n >= 4])
@pytest.mark.parametrize("dt", ae.FLOATS, ids=[ae.NAMES[d] for d in ae.FLOATS])
def test_inputs_depend_on_the_operand_order(oracle, dt, n):
    """The operand order (SIMPLE: the accumulator first; LL: the peer first) changes the expected bytes. It does so
    through Min / Max, which keep their first operand against a NaN; an IEEE add or multiply of two operands is
    commutative bit for bit (and the 16-bit types' NaNs are canonicalised), so under Sum / Prod the two orders
    give the same bytes by construction and only the child order above can show."""
    links = oring.tree_topology(n, 1, 0)
    xs = fc.gen_inputs(np.random.default_rng([SEED, n, dt]), dt, n, 512)
    assert any(not np.array_equal(_expected(xs, dt, op, links, "simple"), _expected(xs, dt, op, links, "ll"))
               for op in (rm.MAX, rm.MIN))
    for op in (rm.SUM, rm.PROD):
        np.testing.assert_array_equal(_expected(xs, dt, op, links, "simple"), _expected(xs, dt, op, links, "ll"))


# ---- live values ------------------------------------------------------------------------------------------------------
def test_live_values_of_every_topology():
    """Every topology the ring library builds at 2..64 ranks, every ranks-per-node that divides n, both trees: at
    most 6 values alive at once, 6 at (34 ranks, 2 per node, tree 0); the kernel holds NEXR_FLAT_TREE_SLOTS = 8."""
    worst = {}
    for n in range(2, 65):
        for per_node in (p for p in range(1, n + 1) if n % p == 0):
            for t in (0, 1):
                code = ftc.compile_tree(oring.tree_topology(n, per_node, t))
                assert len(code) <= 3 * n - 2 and len(ftc.encode(code)) == len(code)
                worst[(n, per_node, t)] = ftc.live_values(code)
    assert max(worst.values()) == 6 <= ftc.SLOTS
    assert worst[(34, 2, 0)] == 6


# ---- argument checks, before any device call ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L(nexr):
    return nexr.lib()


def _arr(vals):
    a = (ctypes.c_void_p * max(1, len(vals)))()
    for i, v in enumerate(vals):
        a[i] = v
    return a


def _parts(nexr, parts):
    return (nexr.FlatTreePart * max(1, len(parts)))(*[nexr.FlatTreePart(o, c, t, 0) for o, c, t in parts])


def _deep(levels):
    """A tree that needs levels + 1 live values: rank 2i has the children [2i + 1 (a leaf), 2i + 2]."""
    n = 2 * levels + 1
    links = []
    for r in range(n):
        if r == n - 1:
            links.append((r - 2 if n > 1 else -1, []))
        elif r % 2 == 0:
            links.append((r - 2 if r else -1, [r + 1, r + 2]))
        else:
            links.append((r - 1, []))
    return links


def test_flat_tree_argument_checks(nexr, L):
    bad, ok = nexr.Result.InvalidArgument, nexr.Result.Success
    F32, SUM, DIV = nexr.DataType.Float32, nexr.DevRedOp.Sum, nexr.DevRedOp.SumPostDiv
    a = _arr([0x1000, 0x2000, 0x3000])
    chain = oring.tree_topology(3)
    keep = []

    def trees_of(*links):
        arr, rows = nexr.flat_tree_links(links)
        keep.append(rows)
        return arr

    one = _parts(nexr, [(0, 64, 0)])
    T1 = trees_of(chain)

    def ar(n=3, ins=a, outs=a, elts=64, dt=F32, op=SUM, arg=0, trees=T1, ntrees=1, parts=one, nparts=1):
        return L.nexrFlatTreeAllReduce(n, ins, outs, elts, int(dt), int(op), arg, 1, trees, ntrees, parts, nparts, None)

    def empty(**kw):   # a valid empty call succeeds without a launch, so what it refuses is the argument
        return ar(elts=0, parts=None, nparts=0, **kw)

    assert empty() == ok
    # everything nexrFlatAllReduce refuses
    assert ar(ins=None) == bad and ar(outs=None) == bad
    assert ar(ins=_arr([0x1000, None, 0x3000])) == bad and ar(outs=_arr([0x1000, 0x2000, None])) == bad
    assert ar(outs=_arr([0x1000, 0x2002, 0x3000])) == bad and ar(ins=_arr([0x1000, 0x2001, 0x3000])) == bad
    assert ar(n=1) == bad and ar(n=65, ins=_arr([0x1000] * 65)) == bad
    assert ar(dt=nexr.DataType.Float8e4m3) == bad and ar(dt=nexr.DataType.Float8e5m2) == bad
    assert ar(dt=12) == bad and ar(dt=-1) == bad and ar(op=5) == bad and ar(op=-1) == bad and ar(op=DIV) == bad
    assert ar(dt=nexr.DataType.Int8, op=DIV, arg=(256 << 1) | 1) == bad
    assert ar(elts=(1 << 62), parts=_parts(nexr, [(0, 1 << 62, 0)])) == bad
    # the trees
    assert empty(ntrees=0) == bad and empty(ntrees=3) == bad and empty(trees=None) == bad
    null_tree = (ctypes.POINTER(nexr.FlatTreeLinks) * 2)()
    null_tree[0] = T1[0]
    assert empty(trees=null_tree, ntrees=2) == bad
    assert empty(trees=trees_of(chain, oring.tree_topology(3, 1, 1)), ntrees=2) == ok
    for links in ([(-1, [1]), (0, []), (-1, [])],                 # two roots
                  [(1, [1]), (0, [0]), (0, [])],                   # no root
                  [(-1, [1]), (0, [2]), (0, [])],                  # an up that its parent's down does not match
                  [(-1, [1, 2]), (0, []), (1, [])],                # a down whose child names another parent
                  [(-1, []), (2, [2]), (1, [1])],                  # a cycle beside the root
                  [(-1, [1, 1]), (0, []), (0, [])],                # a child twice
                  [(-1, [-1, 1, 2]), (0, []), (0, [])],            # children not packed first
                  [(-1, [1]), (0, [3]), (1, [])],                  # a rank out of range
                  [(-1, [1]), (0, [2]), (5, [])],
                  [(0, [1]), (0, [2]), (1, [])]):                  # a rank its own parent
        assert empty(trees=trees_of(links)) == bad, links
    n15, n17 = _deep(7), _deep(8)
    assert ftc.live_values(ftc.compile_tree(n15)) == 8 and ftc.live_values(ftc.compile_tree(n17)) == 9
    assert empty(n=15, ins=_arr([0x1000] * 15), outs=_arr([0x1000] * 15), trees=trees_of(n15)) == ok
    assert empty(n=17, ins=_arr([0x1000] * 17), outs=_arr([0x1000] * 17), trees=trees_of(n17)) == bad
    # the parts: null, a missing tree, gaps, overlaps, descending, short, long, empty, off a pack
    assert ar(parts=None) == bad and ar(nparts=-1) == bad and ar(nparts=0) == bad
    for parts in ([(0, 64, 1)], [(0, 32, 0)], [(0, 65, 0)], [(0, 32, 0), (48, 16, 0)], [(0, 48, 0), (32, 32, 0)],
                  [(32, 32, 0), (0, 32, 0)], [(0, 32, 0), (32, 0, 0), (32, 32, 0)], [(0, 30, 0), (30, 34, 0)],
                  [(4, 60, 0)], [(0, 32, 0), (32, 32, 2)]):
        assert ar(parts=_parts(nexr, parts), nparts=len(parts)) == bad, parts


def test_flat_broadcast_argument_checks(nexr, L):
    bad, ok = nexr.Result.InvalidArgument, nexr.Result.Success
    a = _arr([0x1000, 0x2000, 0x3000])
    assert L.nexrFlatBroadcast(3, 0x1000, a, 0, None) == ok
    assert L.nexrFlatBroadcast(3, 0x1001, _arr([0x1001] * 3), 5, None) == ok   # nothing to write: no launch
    assert L.nexrFlatBroadcast(3, None, a, 0, None) == bad and L.nexrFlatBroadcast(3, 0x1000, None, 0, None) == bad
    assert L.nexrFlatBroadcast(3, 0x1000, _arr([0x1000, None, 0x3000]), 0, None) == bad
    assert L.nexrFlatBroadcast(1, 0x1000, a, 0, None) == bad
    assert L.nexrFlatBroadcast(65, 0x1000, _arr([0x1000] * 65), 0, None) == bad


def test_ring_entries_on_a_host_memory_communicator(nexr, oracle):
    ring = importlib.import_module("nex-nccl_amd.ring")
    RL = ring.ring_lib()
    F32 = nexr.DataType.Float32
    for bits in (1, 2, 4, 7, 8):
        assert RL.nexrRingCommSetFlat(None, bits) == nexr.Result.InvalidArgument
    fn = ctypes.cast(oracle.lib().oracle_reduce_copy_fn, ctypes.c_void_p).value
    with ring.RingComm(2, ring.HOST_MEMORY, 8 * 1024, fn) as comm:      # host memory: never eligible
        for kw in ({"tree": True}, {"copies": True}, {"tree": True, "copies": True}):
            with pytest.raises(nexr.NexrError) as e:
                comm.set_flat(False, **kw)
            assert e.value.code == nexr.Result.InvalidUsage
        for call in (lambda: comm.tree_all_reduce_flat([1, 1], [1, 1], 4, F32, 0),
                     lambda: comm.broadcast_flat([1, 1], [1, 1], 4, F32, 0),
                     lambda: comm.all_gather_flat([1, 1], [1, 1], 4, F32)):
            with pytest.raises(nexr.NexrError) as e:
                call()
            assert e.value.code == nexr.Result.InvalidUsage
        with pytest.raises(nexr.NexrError) as e:
            comm.broadcast_flat([1, 1], [1, 1], 4, F32, 2)               # the root
        assert e.value.code == nexr.Result.InvalidArgument
        assert comm.queued() == 0
    for name in ("nexrTreeAllReduceFlat", "nexrRingBroadcastFlat"):
        assert getattr(RL, name)(None, None, None, 0, 7, 0) == nexr.Result.InvalidArgument
    assert RL.nexrRingAllGatherFlat(None, None, None, 0, 7) == nexr.Result.InvalidArgument
    assert (ring.FLAT_RING, ring.FLAT_TREE, ring.FLAT_COPIES) == (1, 2, 4)


# ---- the symbols, the code objects ------------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_listed(nexr):
    from conftest import ROOT
    ring = importlib.import_module("nex-nccl_amd.ring")
    core = open(os.path.join(ROOT, "include", "nexr.h")).read()
    rng = open(os.path.join(ROOT, "include", "nexr_ring.h")).read()
    for name in ("nexrFlatTreeAllReduce", "nexrFlatBroadcast"):
        assert re.search(r"NEXR_API nexrResult_t %s\(" % name, core)
        assert name in nexr.ABI_SYMBOLS and hasattr(nexr.lib(), name)
    for name in ("nexrTreeAllReduceFlat", "nexrRingBroadcastFlat", "nexrRingAllGatherFlat"):
        assert re.search(r"NEXR_API nexrResult_t %s\(" % name, rng)
        assert name in ring.RING_ABI_SYMBOLS and hasattr(ring.ring_lib(), name)
    for macro, value in (("NEXR_FLAT_RING", 1), ("NEXR_FLAT_TREE", 2), ("NEXR_FLAT_COPIES", 4)):
        assert re.search(r"#define %s %d\b" % (macro, value), rng)
    assert re.search(r"#define NEXR_FLAT_TREE_SLOTS %d\b" % nexr.FLAT_TREE_SLOTS, core) and nexr.FLAT_TREE_SLOTS == ftc.SLOTS
    assert re.search(r"#define NEXR_FLAT_TREE_INLINE_PARTS %d\b" % nexr.FLAT_TREE_INLINE_PARTS, core)
    assert ctypes.sizeof(nexr.FlatTreeLinks) == 16 and ctypes.sizeof(nexr.FlatTreePart) == 24


def test_no_flat_tree_kernel_uses_scratch():
    """The saved accumulators live in registers behind wave-uniform compares: the metadata of every flat tree
    kernel (46 datatype x op instances, the parts fill) and of the broadcast must show no private segment."""
    path = os.path.join(tco.PKG, "libnexr.so")
    assert os.path.exists(path), "libnexr.so not built"
    seen = {}
    for co in tco.gfx950_code_objects(tco._read(path)):
        _tables, notes = tco.elf_tables(co)
        for k in (k for note in notes for k in note["amdhsa.kernels"]):
            if "flat_tree" in k[".name"] or "flat_bcast" in k[".name"]:
                seen[k[".name"]] = (k[".private_segment_fixed_size"], k.get(".vgpr_spill_count", 0),
                                    k.get(".uses_dynamic_stack", False))
    tree = [name for name in seen if "flat_tree_kernel" in name]
    assert len(tree) == 46, len(tree)
    assert any("flat_bcast_kernel" in name for name in seen) and any("flat_tree_parts_kernel" in name for name in seen)
    assert {name: v for name, v in seen.items() if v != (0, 0, False)} == {}
