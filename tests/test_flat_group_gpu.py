"""nexrFlatGroup on the MI355X: several flat collectives as group launches.

Every call is checked two ways over its WHOLE arena, guard bytes included:
  * against tests/flat_cases.py's element-by-element model with the oracle's step function, applied work by work in
    array order to a host copy of the arena (float32 / float64 NaNs by class, as everywhere: arith_edges.canon);
  * against the same works issued one by one through nexrFlatAllReduce / nexrFlatReduceScatter / nexrFlatReduce /
    nexrFlatBroadcast on a twin arena of the same layout, byte for byte.
The inputs are flat_cases' order-sensitive ones, so a wave that ran another work's record, another piece or another
start rank cannot pass. Shapes are the smallest that can go wrong: around one 2048-byte piece, a few pieces, sizes
that differ inside one 4-wave workgroup."""
import os
import subprocess
import sys
from typing import NamedTuple, Optional

import numpy as np
import pytest

import arith_edges as ae
import flat_cases as fc
import ring_modes_cases as rm
import test_flat as tf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = rm.SEED
GUARD = 64
AR, RS, RD, CP = "all_reduce", "reduce_scatter", "reduce", "copy"
COLL_ID = {AR: 0, RS: 1, RD: 2, CP: 3}
PRE_MUL = 3  # nexrDevPreMulSum


class W(NamedTuple):
    """One work. Reducing: `count` elements of `dt` under the host op `op` (encoded for `op_n` ranks: an average's
    factor or divisor; default the call's n), or under the device op `dev` = (devRedOp, redOpArg). A copy: `count`
    bytes to `n_out` destinations. `parts`: the all-reduce's, default one part in chunks of 16 / esz * 4 elements."""
    coll: str
    count: int
    dt: int = ae.F32
    op: int = rm.SUM
    root: int = 0
    parts: Optional[list] = None
    inplace: bool = False
    phase: int = 0
    op_n: Optional[int] = None
    dev: Optional[tuple] = None
    n_out: int = 2
    chain: bool = False   # the inputs are the previous work's outputs (same shape)


def _simple_step(oracle, dt, dev_op, arg):
    def step(x, v, post):
        return oracle.reduce_copy([x] if v is None else [x, v], 1, dt, dev_op, arg, [arg], post)[0]
    return step


class Case:
    """The works laid out in one arena: every buffer at a 256-byte boundary plus its phase, GUARD bytes apart."""

    def __init__(self, oracle, n, works, user_first=True, seed=0):
        self.oracle, self.n, self.works, self.user_first = oracle, n, list(works), user_first
        self.protocol = "simple" if user_first else "ll"
        self.seed = seed
        at = 0
        self.ins, self.outs, self.meta = [], [], []

        def place(nbytes, phase):
            nonlocal at
            start = (at + GUARD + 255) // 256 * 256 + phase
            at = start + nbytes
            return start

        for k, w in enumerate(self.works):
            if w.coll == CP:
                src = place(w.count, w.phase) if not w.chain else self.outs[k - 1][0]
                dsts = [src if (w.inplace and j == 0) else place(w.count, (w.phase + 3 * j + 1) % 16) for j in range(w.n_out)]
                self.ins.append([src])
                self.outs.append(dsts)
                self.meta.append(None)
                continue
            e = rm.esz_of(w.dt)
            assert w.phase % e == 0
            in_elems = w.count * (n if w.coll == RS else 1)
            if w.chain:
                ins = list(self.outs[k - 1])
                assert len(ins) == n and all(ins) and in_elems == self.works[k - 1].count
            else:
                ins = [place(in_elems * e, w.phase) for _ in range(n)]
            if w.inplace:
                outs = [ins[r] + (r * w.count * e if w.coll == RS else 0) for r in range(n)]
            else:
                outs = [place(w.count * e, (w.phase + e * (r + 1)) % 16) for r in range(n)]
            if w.coll == RD:
                outs = [o if r == w.root else 0 for r, o in enumerate(outs)]
            parts = w.parts
            if w.coll == AR and parts is None:
                parts = [(0, w.count, 4 * (16 // e))] if w.count else []
            if w.dev is not None:
                assert user_first
                dev_op, arg = w.dev
                step = _simple_step(oracle, w.dt, dev_op, arg)
            else:
                dev_op, arg = oracle.host_to_dev_red_op(w.op, w.dt, w.op_n or n)
                step = tf.step_of(oracle, self.protocol, w.dt, w.op, w.op_n or n)
            self.ins.append(ins)
            self.outs.append(outs)
            self.meta.append((e, in_elems, parts, dev_op, arg, step))
        self.size = at + GUARD

    def fresh(self, round_=0):
        """The arena before the call: guard bytes, and every input that is not a chained one."""
        rng = np.random.default_rng([SEED, self.seed, round_])
        a = np.full(self.size, rm.GUARD_BYTE, np.uint8)
        for k, w in enumerate(self.works):
            if w.chain:
                continue
            if w.coll == CP:
                a[self.ins[k][0]:self.ins[k][0] + w.count] = rng.integers(0, 256, w.count, dtype=np.uint8)
                continue
            e, in_elems = self.meta[k][:2]
            for r, x in enumerate(fc.gen_inputs(rng, w.dt, self.n, in_elems)):
                a[self.ins[k][r]:self.ins[k][r] + in_elems * e] = x.view(np.uint8)
        return a

    def expected(self, arena):
        """The model, work by work in array order on a copy of the arena."""
        a = arena.copy()
        for k, w in enumerate(self.works):
            if w.coll == CP:
                src = a[self.ins[k][0]:self.ins[k][0] + w.count].copy()
                for d in self.outs[k]:
                    a[d:d + w.count] = src
                continue
            e, in_elems, parts, _dev_op, _arg, step = self.meta[k]
            if w.count == 0:
                continue
            xs = [a[o:o + in_elems * e].copy().view(ae.UINT[w.dt]) for o in self.ins[k]]
            outs = fc.model(w.coll, xs, w.count, w.root, step, parts)
            for r, o in enumerate(self.outs[k]):
                if outs[r] is not None and o:
                    a[o:o + w.count * e] = np.ascontiguousarray(outs[r]).view(np.uint8)
        return a

    def dicts(self, base):
        """The works as nexr.flat_group takes them, over the arena at device address `base`."""
        ds = []
        for k, w in enumerate(self.works):
            ins = [base + o for o in self.ins[k]]
            outs = [base + o if o else 0 for o in self.outs[k]]
            if w.coll == CP:
                ds.append({"coll": 3, "inputs": ins, "outputs": outs, "n_elts": w.count})
                continue
            _e, _ie, parts, dev_op, arg, _step = self.meta[k]
            ds.append({"coll": COLL_ID[w.coll], "inputs": ins, "outputs": outs, "n_elts": w.count, "datatype": w.dt,
                       "dev_red_op": dev_op, "red_op_arg": arg, "root": w.root, "parts": parts if w.coll == AR else None})
        return ds

    def singles(self, nexr, base, stream=0):
        """The same works one by one through the single entries."""
        for d in self.dicts(base):
            if d["coll"] == 3:
                outs = d["outputs"] if len(d["outputs"]) > 1 else d["outputs"] * 2
                nexr.flat_broadcast(d["inputs"][0], outs, d["n_elts"], stream=stream)
            elif d["coll"] == 0:
                nexr.flat_all_reduce(d["inputs"], d["outputs"], d["n_elts"], d["datatype"], d["dev_red_op"],
                                     d["red_op_arg"], self.user_first, d["parts"] or [], stream=stream)
            elif d["coll"] == 1:
                nexr.flat_reduce_scatter(d["inputs"], d["outputs"], d["n_elts"], d["datatype"], d["dev_red_op"],
                                         d["red_op_arg"], self.user_first, stream=stream)
            else:
                nexr.flat_reduce(d["inputs"], d["outputs"][d["root"]], d["root"], d["n_elts"], d["datatype"],
                                 d["dev_red_op"], d["red_op_arg"], self.user_first, stream=stream)

    def canon(self, arena):
        """float32 / float64 output regions with every NaN made one NaN."""
        a = arena.copy()
        for k, w in enumerate(self.works):
            if w.coll != CP and w.dt in (ae.F32, ae.F64):
                e = self.meta[k][0]
                for o in self.outs[k]:
                    if o:
                        a[o:o + w.count * e] = ae.canon(w.dt, a[o:o + w.count * e].copy().view(ae.UINT[w.dt])).view(np.uint8)
        return a

    def verify(self, got, twin, before, what=""):
        bad = np.flatnonzero(got != twin)
        assert bad.size == 0, (what, "group against the single calls", bad[:8].tolist(), self.where(bad[0]))
        want = self.canon(self.expected(before))
        bad = np.flatnonzero(self.canon(got) != want)
        assert bad.size == 0, (what, "group against the model", bad[:8].tolist(), self.where(bad[0]))

    def where(self, off):
        for k in range(len(self.works)):
            for kind, lst in (("in", self.ins[k]), ("out", self.outs[k])):
                for r, o in enumerate(lst):
                    if o and o - GUARD <= off < o + self.size_of(k, kind) + GUARD:
                        return (k, self.works[k].coll, kind, r, int(off) - o)
        return None

    def size_of(self, k, kind):
        w = self.works[k]
        if w.coll == CP:
            return w.count
        e, in_elems = self.meta[k][:2]
        return (in_elems if kind == "in" else w.count) * e


def device_arena(case, arena):
    dev = torch.empty(case.size + 256, dtype=torch.uint8, device="cuda")
    view = dev[:case.size]
    assert view.data_ptr() % 256 == 0
    view.copy_(torch.from_numpy(arena))
    return view


def run(nexr, oracle, n, works, user_first=True, max_workgroups=0, seed=0, what=""):
    """The group on one arena, the single calls on its twin; both checks. Returns (launch_of, info)."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    case = Case(oracle, n, works, user_first, seed)
    before = case.fresh()
    g, t = device_arena(case, before), device_arena(case, before)
    torch.cuda.synchronize()
    launch_of, info = nexr.flat_group(n, case.dicts(g.data_ptr()), user_first, max_workgroups)
    case.singles(nexr, t.data_ptr())
    torch.cuda.synchronize()
    case.verify(g.cpu().numpy(), t.cpu().numpy(), before, what)
    return launch_of, info


def piece_counts(e):
    """Element counts around one 2048-byte piece, then 3 and 5 pieces with odd ends."""
    p = 2048 // e
    return [1, p - 1, p, p + 1, 3 * p - 5, 4 * p + 3]


# ---- works of different size inside one workgroup ------------------------------------------------------------------
@pytest.mark.parametrize("user_first", (True, False), ids=["simple", "ll"])
@pytest.mark.parametrize("dt", (ae.I8, ae.F16, ae.F32, ae.F64), ids=["i8", "f16", "f32", "f64"])
def test_small_works(nexr, oracle, dt, user_first):
    """1 element, 2048 / esz - 1, 2048 / esz, 2048 / esz + 1, 3 and 5 pieces, the three reductions in turn: works
    of different size meet inside one 4-wave workgroup, and a wrong work lookup shows."""
    e = rm.esz_of(dt)
    colls = (AR, RS, RD)
    works = [W(colls[k % 3], c, dt, rm.SUM, root=k % 3, inplace=k % 4 == 3) for k, c in enumerate(piece_counts(e))]
    works += [W(colls[(k + 1) % 3], c, dt, rm.SUM, root=(k + 1) % 3) for k, c in enumerate(piece_counts(e)[:4])]
    launch_of, info = run(nexr, oracle, 3, works, user_first, seed=dt)
    assert launch_of == [0] * len(works) and info["launches"] == 1 and info["fill_launches"] == 0


def test_one_element_beside_a_large_work(nexr, oracle):
    works = [W(AR, 1), W(AR, 100003, parts=[(0, 50000, 64), (50000, 50003, 64)]), W(RD, 1, root=1), W(RS, 1)]
    launch_of, info = run(nexr, oracle, 4, works, seed=1)
    assert launch_of == [0, 0, 0, 0] and info["workgroups"] == (1 + 196 + 1 + 4 + 3) // 4


def test_chunk_boundary_inside_a_piece(nexr, oracle):
    """Two parts whose chunks (16 and 40 elements) end inside 2048-byte pieces; the second part starts inside one."""
    works = [W(AR, 1000, parts=[(0, 300, 16), (300, 700, 40)]), W(AR, 600, ae.BF16, parts=[(0, 40, 8), (40, 560, 24)]),
             W(AR, 1000, parts=[(0, 520, 128), (520, 480, 4)])]
    launch_of, _ = run(nexr, oracle, 3, works, seed=2)
    assert launch_of == [0, 1, 0]
    for w in works:   # the premise: a start rank changes inside a piece
        s = fc.all_reduce_starts(3, w.count, rm.esz_of(w.dt), w.parts)
        piece = 2048 // rm.esz_of(w.dt)
        assert any(len(set(s[i:i + piece].tolist())) > 1 for i in range(0, w.count, piece))


def test_all_kinds_in_one_call(nexr, oracle):
    """The three reductions and copies, four kinds, in place and out of place: one launch per kind."""
    works = [W(AR, 700), W(CP, 3001, n_out=3), W(RS, 513, ae.I32, rm.MIN), W(RD, 2049, root=2), W(AR, 5, ae.BF16),
             W(RS, 100, inplace=True), W(CP, 17, n_out=1), W(RD, 64, ae.I32, rm.MIN, root=1, inplace=True),
             W(AR, 1025, ae.BF16, inplace=True), W(CP, 2048, n_out=4, inplace=True), W(RD, 3, ae.I32, rm.MAX)]
    launch_of, info = run(nexr, oracle, 4, works, seed=3)
    assert launch_of == [0, 1, 2, 0, 3, 0, 1, 2, 3, 1, 4]
    assert info["launches"] == 5 and info["works"] == 11 and info["fill_launches"] == 0


@pytest.mark.parametrize("n", (2, 3, 8, 9))
def test_rank_counts(nexr, oracle, n):
    """9 ranks: the chain goes on beyond the kSymPeers = 8 inputs a wave loads at once."""
    works = [W(AR, 1030, ae.F16, root=0), W(RS, 515, ae.F16), W(RD, 1500, ae.F16, root=n - 1), W(CP, 777, n_out=n),
             W(AR, 9, ae.F16, inplace=True)]
    launch_of, _ = run(nexr, oracle, n, works, seed=10 + n)
    assert launch_of == [0, 0, 0, 1, 0]


@pytest.mark.parametrize("dt", (ae.BF16, ae.U64), ids=["bf16", "u64"])
def test_every_phase_mod_16(nexr, oracle, dt):
    """One group whose works sit at every element-aligned phase mod 16 (outputs at further phases), odd tails."""
    e = rm.esz_of(dt)
    op = rm.SUM if dt == ae.BF16 else rm.PROD
    works = []
    for phase in range(0, 16, e):
        k = phase // e
        works.append(W((AR, RS, RD)[k % 3], 2 * (2048 // e) + 16 // e + 1 + k, dt, op, root=k % 3, phase=phase,
                       inplace=k % 5 == 4))
    works += [W(CP, 2048 + 31 + p, phase=p, n_out=2) for p in range(16)]
    run(nexr, oracle, 3, works, seed=20 + dt)


# ---- the table: inline, workspace, many fill launches ----------------------------------------------------------------
def test_table_sizes(nexr, oracle):
    """W = 1, the largest table that rides in the kernel arguments, one work more, and 200 works (several fill
    launches), at 2 ranks with one part per all-reduce."""
    n = 2
    most = nexr.FLAT_GROUP_INLINE_BYTES // (40 + 16 * n + 24)
    for count, fills in ((1, 0), (most, 0), (most + 1, 2), (200, 5)):
        works = [W(AR, 1 + (37 * k) % 600, ae.I32, rm.SUM, inplace=k % 7 == 0) for k in range(count)]
        launch_of, info = run(nexr, oracle, n, works, seed=30, what=count)
        assert launch_of == [0] * count and info["launches"] == 1
        assert info["fill_launches"] == fills, (count, info)
    copies = [W(CP, 1 + 29 * k, n_out=1 + k % 3, phase=k % 16) for k in range(120)]
    launch_of, info = run(nexr, oracle, n, copies, seed=31)
    assert info["launches"] == 1 and info["fill_launches"] == 2      # 120 records of 24 + 8 * 3 bytes


@pytest.mark.parametrize("cap", (1, 2))
def test_capped_grid_strides_across_works(nexr, oracle, cap):
    works = [W((AR, RS, RD)[k % 3], c, ae.F32, rm.SUM, root=k % 2) for k, c in enumerate([700, 1, 513, 2000, 3, 1025, 512])]
    works.append(W(CP, 9000, n_out=2))
    launch_of, info = run(nexr, oracle, 3, works, max_workgroups=cap, seed=40 + cap)
    assert info["launches"] == 2 and info["workgroups"] == 2 * cap


# ---- every instance ---------------------------------------------------------------------------------------------------
def test_every_instance(nexr, oracle):
    """All 46 (datatype, device op) instances and the copy kernel, three works each, in ONE call: Sum, Prod, MinMax
    (a launch for min and one for max), PreMulSum on every datatype, SumPostDiv on the integers."""
    n = 3
    works = []
    for dt in range(10):
        e = rm.esz_of(dt)
        devs = [oracle.host_to_dev_red_op(op, dt, n) for op in (rm.SUM, rm.PROD, rm.MIN, rm.MAX)]
        devs.append(oracle.host_to_dev_red_op(rm.AVG, dt, n) if dt in ae.FLOATS else (PRE_MUL, 3))
        if dt in ae.INTS:
            devs.append(oracle.host_to_dev_red_op(rm.AVG, dt, n))
        for j, dev in enumerate(devs):
            for k, coll in enumerate((AR, RS, RD)):
                works.append(W(coll, 2048 // e + 16 // e + 1 + k + j, dt, dev=dev, root=(j + k) % n, inplace=(j + k) % 4 == 0))
    works += [W(CP, 5000, n_out=3), W(CP, 1), W(CP, 2047, n_out=1)]
    assert {(w.dt, w.dev[0]) for w in works if w.coll != CP} == {(dt, op) for dt in range(10) for op in range(5)
                                                                 if op != 4 or dt in ae.INTS}
    launch_of, info = run(nexr, oracle, n, works, seed=50)
    assert info["launches"] == 10 * 5 + 6 + 1 and info["works"] == len(works)
    assert len(set(launch_of)) == info["launches"]


@pytest.mark.parametrize("user_first", (True, False), ids=["simple", "ll"])
def test_average_with_an_argument_per_work(nexr, oracle, user_first):
    """PreMulSum by 1 / 2, 1 / 3, 1 / 5, 1 / 7 and SumPostDiv by 2, 3, 5, 7 in one launch each: redOpArg is the
    work's, not the launch's."""
    works = []
    for k, m in enumerate((2, 3, 5, 7)):
        works.append(W((AR, RS, RD)[k % 3], 1100 + k, ae.F16, rm.AVG, root=k % 3, op_n=m))
        works.append(W((RD, AR, RS)[k % 3], 530 + k, ae.I32, rm.AVG, root=k % 3, op_n=m))
        works.append(W((RS, RD, AR)[k % 3], 300 + k, ae.F32, rm.AVG, root=k % 3, op_n=m))
    launch_of, info = run(nexr, oracle, 3, works, user_first, seed=60)
    assert launch_of == [0, 1, 2] * 4


def test_dependent_works_cut(nexr, oracle):
    """A chain: the second work reduces what the first wrote, the third copies the second's result."""
    works = [W(AR, 1500, ae.I32), W(AR, 1500, ae.I32, chain=True), W(RD, 40, ae.I32),
             W(AR, 1500, ae.I32, rm.MAX, chain=False)]
    works.insert(2, W(CP, 1500 * 4, n_out=2, chain=True))
    launch_of, info = run(nexr, oracle, 3, works, seed=70)
    assert launch_of == [0, 1, 2, 3, 4] and info["launches"] == 5
    # the reduce after the cuts found no open launch of its kind: each cut closes them all


# ---- the other semantics, in child processes ----------------------------------------------------------------------------
_WORKER = r"""
import importlib, sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
import oracle
import arith_edges as ae, ring_modes_cases as rm
import test_flat_group_gpu as t
oracle.lib()
oracle.set_semantics({mode})
nexr = importlib.import_module("nex-nccl_amd")
assert nexr.get_semantics() == {mode}
for user_first in (True, False):
    works = []
    for k, (dt, op) in enumerate([(ae.I8, rm.MIN), (ae.I32, rm.MAX), (ae.F16, rm.AVG), (ae.I64, rm.AVG), (ae.F32, rm.SUM)]):
        for j, coll in enumerate((t.AR, t.RS, t.RD)):
            works.append(t.W(coll, 2048 // rm.esz_of(dt) + 5 + j + k, dt, op, root=(j + k) % 3, inplace=(j + k) % 3 == 0))
    works.append(t.W(t.CP, 4099, n_out=3))
    launch_of, info = t.run(nexr, oracle, 3, works, user_first, seed=80)
    assert info["launches"] == 6, info
torch.cuda.synchronize()
print("GROUP-OK")
"""


@pytest.mark.parametrize("name,mode", [("fork", 1), ("shipped", 2)])
def test_under_the_other_semantics(nexr, name, mode):
    """NEXR_SEMANTICS is read once per process: a child for each. Fork: signed min / max on the unsigned type;
    shipped: every reduce returns its first operand."""
    from conftest import GOLDEN, ROOT
    code = _WORKER.format(root=ROOT, tests=os.path.join(ROOT, "tests"), golden=GOLDEN, mode=mode)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, NEXR_SEMANTICS=name), capture_output=True,
                         text=True, timeout=150)
    assert out.returncode == 0 and "GROUP-OK" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


# ---- streams and graph capture ------------------------------------------------------------------------------------------
def test_on_a_stream_and_under_capture(nexr, oracle):
    """A non-default stream, then one linear graph capture (a table in the arguments and one in the workspace)
    replayed on new inputs: nothing of the caller's arrays is read after the call."""
    n = 2
    works = [W((AR, RS, RD)[k % 3], 1 + (53 * k) % 900, ae.F16, rm.SUM, root=k % 2) for k in range(60)]
    works += [W(CP, 100 + k, n_out=2) for k in range(3)]
    case = Case(oracle, n, works, True, seed=90)
    before = case.fresh()
    g, t = device_arena(case, before), device_arena(case, before)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        _, info = nexr.flat_group(n, case.dicts(g.data_ptr()), True, stream=s.cuda_stream)
        case.singles(nexr, t.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert info["launches"] == 2 and info["fill_launches"] == 2
    case.verify(g.cpu().numpy(), t.cpu().numpy(), before, "stream")

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ds = case.dicts(g.data_ptr())
        nexr.flat_group(n, ds, True, stream=torch.cuda.current_stream().cuda_stream)
        del ds
    again = case.fresh(round_=1)
    assert not np.array_equal(again, before)
    g.copy_(torch.from_numpy(again))
    t.copy_(torch.from_numpy(again))
    torch.cuda.synchronize()
    graph.replay()
    case.singles(nexr, t.data_ptr())
    torch.cuda.synchronize()
    case.verify(g.cpu().numpy(), t.cpu().numpy(), again, "replay")
