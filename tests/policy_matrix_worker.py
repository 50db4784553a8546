"""Child process of tests/test_policy_matrix.py and tests/test_policy_matrix_gpu.py: every compiled
reduce-copy kernel under the cache policy forced by NEXR_POLICY (0 plain, 1 non-temporal loads, 3
non-temporal loads and stores; read once by the library, hence a child per setting), at sizes of one to
five trips of the workgroup shape that policy selects (shape_for, nexr_internal.h), against the oracle
bit for bit.

    policy_matrix_worker.py [--plan] [--mode matrix|grid|bare] DATATYPE...   (names of mg.DT_NAMES, or "all")

The plan is pure Python and deterministic. For every datatype x {sum, prod, min, max, premulsum, sumpostdiv
(integers)} x K = 1..8, with T = B * U * E elements the trip of the shape the call runs (E = 16 / esz):
  A  n = T, every pointer 128-B aligned, M = 1: exactly one full trip;
  B  n = 2T + 37E + max(1, E - 1), every pointer at 128 - 3 esz within its line (a head of 3), M = 2;
  C  n = T - E + 1 (no full trip), pointer i at ((3 i) mod E) esz (mixed 16-B phases), M = 3;
  D  n = T + 5, pointer i at the odd byte 2 i + 1, M = 8 when K <= 2, else 1;
  one nexrReduceCopyBatch of A, B and C with M = 1, each work also run alone and compared byte for byte;
  B once more in place (dst == src0, M = 1).
fp16, bf16 and int8 add tests/arith_edges.py's pair layout (K = 2) and K = 8 fold at both pack parities
against its independent reference; fp32, fp16, bf16 and fp64 add the one-rank launcher with the scalar in
device memory (n = T + 5). `--mode grid` (run with NEXR_GRID=2) is layout E alone: n = 5T + 11E + 1 with
B's phases, M = 2, sum and max at K = 2, 4, 5, 8, so both workgroups stride over full trips.

Before every call nexrQueryLaunch must report the forced policy and the (block, packsPerLane) this
file's restatement of shape_for gives for the routed (datatype, K). `--plan` stops there, on fabricated
addresses: no device allocation, no launch. Exit status 1 and a FAIL line at the first mismatch or library
error; on success one JSON line: the policy, the calls made, the routed (dt, op, K, isMin) keys launched
as single and as batch kernels, and the shapes seen. `--mode bare` imports torch, loads the library, touches
the device and exits: the start-up floor of every item."""
import argparse
import importlib
import json
import os
import sys
from types import SimpleNamespace

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE, os.path.join(HERE, "golden")]

import numpy as np  # noqa: E402

import make_golden as mg  # noqa: E402

OPS = [("sum", mg.SUM), ("prod", mg.PROD), ("min", mg.MINMAX), ("max", mg.MINMAX), ("premulsum", mg.PREMULSUM),
       ("sumpostdiv", mg.SUMPOSTDIV)]
GRID_OPS = ("sum", "max")
GRID_KS = (2, 4, 5, 8)
ARITH_TYPES = (mg.F16, mg.BF16, mg.I8)
ONE_RANK_TYPES = (mg.F32, mg.F16, mg.BF16, mg.F64)
SIGNED = (mg.I8, mg.I32, mg.I64)
GUARD = 64
SRC_FILL, DST_FILL = 0xA5, 0x5A
LINE = 128


def ops_for(dt):
    return [(name, op) for name, op in OPS if name != "sumpostdiv" or dt in mg.INTS]


def esz_of(dt):
    return np.dtype(mg.STORE[dt]).itemsize


# ---- restatements of nexr_internal.h (shape_for) and nexr_api.cpp (routeKernel) -----------------------------
def shape_for(dt, k, pol):
    """(B lanes, U packs per lane) of the kernel for (routed datatype, K, policy)."""
    half = dt in (mg.F16, mg.BF16)
    four = dt in (mg.I32, mg.U32, mg.F32)
    if pol == 3 and k >= 6:
        return (512, 1)
    if half and k >= 8:
        return (1024, 1)
    if k == 4 and pol == 1 and not four:
        return (512, 2)
    if k in (4, 5) and pol == 3 and dt == mg.BF16:
        return (512, 1)
    if k in (4, 5) and pol == 3 and dt != mg.F16:
        return (1024, 1)
    return (256, 4)


def route(dt, op, k, n_pre, post, arg):
    """The (dt, op, K, isMin) of the kernel a call launches: PreMulSum without pre-op sources and SumPostDiv
    without the divide are Sum; K = 1 without arithmetic is the uint8 copy; signed Sum / Prod / PreMulSum /
    SumPostDiv run the unsigned type."""
    if op == mg.PREMULSUM and n_pre == 0:
        op = mg.SUM
    if op == mg.SUMPOSTDIV and not post:
        op = mg.SUM
    if k == 1 and op not in (mg.PREMULSUM, mg.SUMPOSTDIV):
        return (mg.U8, mg.SUM, 1, 0)
    if op != mg.MINMAX and dt in SIGNED:
        dt = {mg.I8: mg.U8, mg.I32: mg.U32, mg.I64: mg.U64}[dt]
    return (dt, op, k, int(op == mg.MINMAX and (arg & 1) == 0))


# ---- the plan ---------------------------------------------------------------------------------------------
def case_args(dt, name, k, rng):
    """As test_reduce_copy_gpu._case_args, except that SumPostDiv's divisor is always > 1 (PreMulSum there
    already has a pre-op source and the post-op), so that neither routes onto Sum."""
    arg, pre, post = 0, None, False
    if name in ("min", "max"):
        arg = mg.minmax_arg(dt, name == "max")
    if name == "premulsum":
        vals = [0.5, -1.25, 3.0, 0.125, 1.0, -0.75, 2.0, 0.3333333]
        npre = int(rng.integers(1, k + 1))
        pre = [mg.float_scalar_bits(dt, vals[s] if dt not in mg.INTS else s * 5 + 3) for s in range(npre)]
        post = True
    if name == "sumpostdiv":
        arg = (int(rng.integers(2, 9)) << 1) | int(dt in SIGNED)
        post = True
    return arg, pre, post


def layout(letter, dt, k, m, trip):
    """(n, source byte offsets, destination byte offsets) within each pointer's 128-B line."""
    esz = esz_of(dt)
    e = 16 // esz
    if letter == "A":
        return trip, [0] * k, [0] * m
    if letter in ("B", "E"):
        n = 2 * trip + 37 * e + max(1, e - 1) if letter == "B" else 5 * trip + 11 * e + 1
        return n, [LINE - 3 * esz] * k, [LINE - 3 * esz] * m
    if letter == "C":
        offs = [((3 * i) % e) * esz for i in range(k + m)]
        assert e == 1 or len({o % 16 for o in offs}) >= 2
        return trip - e + 1, offs[:k], offs[k:]
    assert letter == "D"
    offs = [2 * i + 1 for i in range(k + m)]
    return trip + 5, offs[:k], offs[k:]


LETTERS = "ABCDE"
MATRIX_LAYOUTS = (("A", 1), ("B", 2), ("C", 3), ("D", None))  # (letter, M); D: M = 8 when K <= 2, else 1


def make_call(pol, check, dt, name, op, k, args, m, letter, in_place=False):
    arg, pre, post = args
    key = route(dt, op, k, len(pre or []), post, arg)
    shape = shape_for(key[0], key[2], pol)
    trip = shape[0] * shape[1] * (16 // esz_of(dt))
    n, so, do = layout(letter, dt, k, m, trip)
    if in_place:
        do = so[:1]
    return SimpleNamespace(kind="single", check=check, dt=dt, name=name, op=op, k=k, m=m, n=n, arg=arg, pre=pre,
                           post=post, src_off=so, dst_off=do, key=key, shape=shape, letter=letter,
                           seed=7000 + 100 * dt + 10 * k + LETTERS.index(letter), in_place=in_place)


def build_plan(pol, dts, mode):
    """The list of calls; a batch is one entry (its three works under .works) followed by those works alone."""
    plan = []
    for dt in dts:
        for k in (GRID_KS if mode == "grid" else range(1, 9)):  # K outermost: the ops share its sources
            for oi, (name, op) in enumerate(ops_for(dt)):
                if mode == "grid" and name not in GRID_OPS:
                    continue
                case = (pol, dt, name, op, k, case_args(dt, name, k, np.random.default_rng([dt, oi, k])))
                if mode == "grid":
                    plan.append(make_call(pol, "layout E", *case[1:], 2, "E"))
                    continue
                for letter, m in MATRIX_LAYOUTS:
                    plan.append(make_call(pol, "layout " + letter, *case[1:], m or (8 if k <= 2 else 1), letter))
                works = [make_call(pol, "batch work %s alone" % letter, *case[1:], 1, letter) for letter in "ABC"]
                plan.append(SimpleNamespace(kind="batch", check="batch", dt=dt, name=name, op=op, k=k, works=works))
                plan.extend(works)
                plan.append(make_call(pol, "in place", *case[1:], 1, "B", in_place=True))
        if mode == "grid":
            continue
        if dt in ARITH_TYPES:
            plan.extend(arith_calls(pol, dt))
        if dt in ONE_RANK_TYPES:
            key = (dt, mg.PREMULSUM, 1, 0)
            shape = shape_for(dt, 1, pol)
            plan.append(SimpleNamespace(kind="onerank", check="one-rank pointer scalar", dt=dt, name="premulsum",
                                        op=mg.PREMULSUM, k=1, m=1, n=shape[0] * shape[1] * (16 // esz_of(dt)) + 5,
                                        arg=0, pre=None, post=True, src_off=[0], dst_off=[0], key=key, shape=shape,
                                        seed=7900 + dt, in_place=False))
    return plan


def arith_calls(pol, dt):
    """arith_edges' pair layout (K = 2) and K = 8 fold, the four ops, both pack parities, M = 1."""
    import arith_edges as ae
    lay = dict(ae.layouts(dt))
    out = []
    for lname in ("pairs", "fold8"):
        srcs = lay[lname]
        k = len(srcs)
        assert k == (2 if lname == "pairs" else 8)
        for name, op, is_max in ae.FOUR_OPS:
            arg = ae.op_arg(dt, op, is_max)
            key = route(dt, op, k, 0, False, arg)
            for parity, tag in enumerate(("even", "odd")):
                out.append(SimpleNamespace(kind="arith", check="arith_edges %s %s" % (lname, tag), dt=dt,
                                           name=name, op=op, k=k, m=1,
                                           n=srcs[0].size + parity, arg=arg, pre=None, post=False, src_off=[0] * k,
                                           dst_off=[0], key=key, shape=shape_for(key[0], k, pol), lname=lname,
                                           parity=parity, in_place=False))
    return out


def planned_calls(dts, mode):
    """The number of library calls of a plan, from its parameters alone (the tests' own count)."""
    if mode == "grid":
        return len(dts) * len(GRID_OPS) * len(GRID_KS)
    per_case = len(MATRIX_LAYOUTS) + 1 + 3 + 1  # layouts, the batch, its works alone, in place
    return sum(len(ops_for(dt)) * 8 * per_case + (2 * 4 * 2 if dt in ARITH_TYPES else 0) + (dt in ONE_RANK_TYPES)
               for dt in dts)


# ---- running it -------------------------------------------------------------------------------------------
class Failure(Exception):
    pass


class Runner:
    def __init__(self, nexr, pol, grid, plan_only):
        self.nexr, self.pol, self.grid, self.plan_only = nexr, pol, grid, plan_only
        self.calls = 0
        self.single_keys, self.batch_keys, self.shapes = set(), set(), set()
        self.host_srcs, self.dev_srcs, self.expected = {}, {}, {}
        self.fake = 0x7F00_0000_0000
        if not plan_only:
            import torch
            import oracle
            self.torch, self.oracle = torch, oracle
            oracle.lib()
            assert torch.cuda.is_available(), "needs an MI355X"
            self.stream = torch.cuda.current_stream().cuda_stream

    def fail(self, c, what, srcs=None, dsts=None):
        raise Failure("FAIL policy=%d grid=%d dt=%s op=%s K=%d M=%s n=%s src_off=%s dst_off=%s ptrs=%s check=%r: %s" % (
            self.pol, self.grid, mg.DT_NAMES[c.dt], c.name, c.k, getattr(c, "m", "-"), getattr(c, "n", "-"),
            getattr(c, "src_off", "-"), getattr(c, "dst_off", "-"),
            [hex(p) for p in (srcs or []) + (dsts or [])], c.check, what))

    # -- buffers: data at `off` past a 128-B boundary, at least 128 bytes of fill before it and 64 behind
    def fake_ptr(self, off):
        self.fake += 1 << 24
        return self.fake + off

    def alloc(self, nbytes, off, fill, data=None):
        t = self.torch.empty(nbytes + 3 * LINE + GUARD + off, dtype=self.torch.uint8, device="cuda")
        lead = (-t.data_ptr()) % LINE + LINE + off
        host = np.full(t.numel(), fill, dtype=np.uint8)
        if data is not None:
            host[lead:lead + nbytes] = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        t.copy_(self.torch.from_numpy(host))
        return SimpleNamespace(t=t, lead=lead, nbytes=nbytes, ptr=t.data_ptr() + lead, fill=fill)

    def read(self, c, buf, what):
        host = buf.t.cpu().numpy()
        if not ((host[:buf.lead] == buf.fill).all() and (host[buf.lead + buf.nbytes:] == buf.fill).all()):
            self.fail(c, what + ": write outside the destination")
        return host[buf.lead:buf.lead + buf.nbytes].copy()

    def sources(self, c):
        key = (c.dt, c.k, c.n, c.seed)
        if key not in self.host_srcs:
            self.host_srcs[key] = mg.gen_inputs(c.dt, c.k, c.n, c.seed, special=True)
        return self.host_srcs[key]

    def device_sources(self, c, srcs, tag):
        key = (tag, tuple(c.src_off))
        if key not in self.dev_srcs:
            self.dev_srcs[key] = [self.alloc(s.nbytes, o, SRC_FILL, s) for s, o in zip(srcs, c.src_off)]
        return self.dev_srcs[key]

    def expect(self, c, srcs):
        key = (c.dt, c.name, c.k, c.n, c.seed)
        if key not in self.expected:
            exp = self.oracle.reduce_copy(srcs, 1, c.dt, c.op, c.arg, c.pre, c.post)[0]
            self.expected[key] = mg.canon_bytes(c.dt, exp)
        return self.expected[key]

    def geometry(self, c, srcs, dsts):
        info = self.nexr.query_launch(srcs, dsts, c.n, c.dt)
        got = (info.policy, info.block, info.packsPerLane)
        if got != (self.pol,) + c.shape:
            self.fail(c, "nexrQueryLaunch reports (policy, block, packsPerLane) %s, expected %s" % (
                got, (self.pol,) + c.shape), srcs, dsts)
        if self.grid and info.grid != self.grid:
            self.fail(c, "nexrQueryLaunch reports grid %d under NEXR_GRID=%d" % (info.grid, self.grid), srcs, dsts)
        self.shapes.add(c.shape)

    def compare(self, c, got_bytes, exp_canon, what, srcs, dsts):
        got = mg.canon_bytes(c.dt, got_bytes.view(mg.STORE[c.dt]))
        if got != exp_canon:
            g, e = np.frombuffer(got, np.uint8), np.frombuffer(exp_canon, np.uint8)
            bad = np.nonzero(g != e)[0]
            self.fail(c, "%s: %d bytes differ from the oracle, first at byte %d (element %d)" % (
                what, bad.size, int(bad[0]), int(bad[0]) // esz_of(c.dt)), srcs, dsts)

    # -- one nexrReduceCopy with every check; returns the destinations' raw bytes
    def single(self, c, srcs_host=None, count_key=True):
        if self.plan_only:
            sp = [self.fake_ptr(o) for o in c.src_off]
            dp = sp[:1] if c.in_place else [self.fake_ptr(o) for o in c.dst_off]
            self.geometry(c, sp, dp)
            self.calls += 1
            self.single_keys.add(c.key)
            return None
        host = srcs_host if srcs_host is not None else self.sources(c)
        dev = self.device_sources(c, host, (c.kind, c.dt, c.k, c.n, getattr(c, "seed", c.check)))
        if c.in_place:  # a private copy of src0: the call overwrites it
            dev = [self.alloc(host[0].nbytes, c.src_off[0], SRC_FILL, host[0])] + dev[1:]
            dst = dev[:1]
        else:
            dst = [self.alloc(c.n * esz_of(c.dt), o, DST_FILL) for o in c.dst_off]
        sp, dp = [b.ptr for b in dev], [b.ptr for b in dst]
        self.geometry(c, sp, dp)
        try:
            self.nexr.reduce_copy_ptrs(sp, dp, c.n, c.dt, c.op, c.arg, c.pre, c.post, self.stream)
        except self.nexr.NexrError as e:
            self.fail(c, "nexrReduceCopy: %s" % e, sp, dp)
        self.calls += 1
        self.single_keys.add(c.key)
        return [self.read(c, b, "dst %d" % i) for i, b in enumerate(dst)], sp, dp

    def run_single(self, c):
        if self.plan_only:
            return self.single(c)
        host = self.sources(c)
        exp = self.expect(c, host)
        outs, sp, dp = self.single(c)
        for i, o in enumerate(outs):
            self.compare(c, o, exp, "dst %d" % i, sp, dp)
        return outs

    def run_batch(self, c, solo_outs):
        keyset = self.batch_keys if self.pol < 2 else self.single_keys  # nt stores: the host runs single launches
        if self.plan_only:
            for w in c.works:
                self.geometry(w, [self.fake_ptr(o) for o in w.src_off], [self.fake_ptr(o) for o in w.dst_off])
                keyset.add(w.key)
            self.calls += 1
            return
        works, dsts = [], []
        for w in c.works:
            host = self.sources(w)
            dev = self.device_sources(w, host, (w.kind, w.dt, w.k, w.n, w.seed))
            d = self.alloc(w.n * esz_of(w.dt), w.dst_off[0], DST_FILL)
            self.geometry(w, [b.ptr for b in dev], [d.ptr])
            works.append(self.nexr.make_work([b.ptr for b in dev], [d.ptr], w.n, w.arg, w.pre, w.post))
            dsts.append(d)
        try:
            self.nexr.reduce_copy_batch(works, c.dt, c.op, self.stream)
        except self.nexr.NexrError as e:
            self.fail(c, "nexrReduceCopyBatch: %s" % e)
        self.calls += 1
        for w, d, solo in zip(c.works, dsts, solo_outs):
            w = SimpleNamespace(**dict(vars(w), check="batch work " + w.letter))
            got = self.read(w, d, "batch dst")
            self.compare(w, got, self.expect(w, self.sources(w)), "in the batch", [], [d.ptr])
            if got.tobytes() != solo[0].tobytes():
                self.fail(w, "the batch's bytes differ from the same work run alone", [], [d.ptr])
            keyset.add(w.key)

    def run_arith(self, c):
        if self.plan_only:
            return self.single(c)
        import arith_edges as ae
        from test_arith_edges import first_diff, reference
        srcs = dict(ae.layouts(c.dt))[c.lname]
        exp = reference(c.dt, c.lname, srcs, c.name, c.op, c.arg)
        tag, ss = ae.both_parities(srcs)[c.parity]
        if c.parity:
            exp = ae.pad_front(c.dt, c.op, c.arg, srcs, exp)
        outs, sp, dp = self.single(c, srcs_host=ss)
        d = first_diff(c.dt, outs[0].view(ae.UINT[c.dt]), exp, ss)
        if d:
            self.fail(c, "differs from arith_edges' reference: %s" % d, sp, dp)

    def run_one_rank(self, c):
        nexr = self.nexr
        red = nexr.host_to_dev_red_op(nexr.RedOp.Avg, c.dt, 4)
        if red.op != nexr.DevRedOp.PreMulSum:
            self.fail(c, "Avg of a float type is not PreMulSum")
        if self.plan_only:
            self.geometry(c, [self.fake_ptr(0)], [self.fake_ptr(0)])
            self.calls += 1
            self.single_keys.add(c.key)
            return
        src = self.sources(c)[0]
        exp = mg.canon_bytes(c.dt, self.oracle.reduce_copy([src], 1, c.dt, mg.PREMULSUM, red.scalarArg,
                                                           [red.scalarArg], True)[0])
        s = self.alloc(src.nbytes, 0, SRC_FILL, src)
        d = self.alloc(src.nbytes, 0, DST_FILL)
        self.geometry(c, [s.ptr], [d.ptr])
        scalar = self.torch.tensor([red.scalarArg], dtype=self.torch.int64).cuda()
        red2 = nexr.DevRedOpFull(red.op, red.proxyOp, 1, scalar.data_ptr())
        try:
            nexr.launch_one_rank(d.ptr, s.ptr, c.n, red2, c.dt, self.stream)
        except nexr.NexrError as e:
            self.fail(c, "nexrLaunchOneRank: %s" % e, [s.ptr], [d.ptr])
        self.calls += 1
        self.single_keys.add(c.key)
        self.compare(c, self.read(c, d, "dst"), exp, "scalarArgIsPtr", [s.ptr], [d.ptr])

    def run(self, plan):
        i = 0
        group = None
        while i < len(plan):
            c = plan[i]
            if (c.dt, c.k, c.kind == "arith") != group:  # device and host buffers live for one (datatype, K)
                group = (c.dt, c.k, c.kind == "arith")
                self.host_srcs, self.dev_srcs, self.expected = {}, {}, {}
            if c.kind == "batch":  # its works alone first (the next three entries), then the batch
                solos = [self.run_single(w) for w in plan[i + 1:i + 4]]
                self.run_batch(c, solos)
                i += 4
                continue
            {"single": self.run_single, "arith": self.run_arith, "onerank": self.run_one_rank}[c.kind](c)
            i += 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", action="store_true")
    ap.add_argument("--mode", choices=("matrix", "grid", "bare"), default="matrix")
    ap.add_argument("datatypes", nargs="*")
    a = ap.parse_args()
    if a.mode == "bare":
        import torch
        importlib.import_module("nex-nccl_amd").lib()
        torch.zeros(1, device="cuda").cpu()
        print("bare ok", flush=True)
        return 0
    if os.environ.get("NEXR_POLICY") not in ("0", "1", "3"):
        print("NEXR_POLICY must be set to 0, 1 or 3 in the environment", flush=True)
        return 2
    pol = int(os.environ["NEXR_POLICY"])
    grid = int(os.environ.get("NEXR_GRID", "0") or 0)
    names = {v: k for k, v in mg.DT_NAMES.items()}
    dts = sorted(mg.DT_NAMES) if a.datatypes in ([], ["all"]) else [names[d] for d in a.datatypes]
    nexr = importlib.import_module("nex-nccl_amd")
    runner = Runner(nexr, pol, grid, a.plan)
    try:
        runner.run(build_plan(pol, dts, a.mode))
    except Failure as f:
        print(f, flush=True)
        return 1
    if not a.plan:
        runner.torch.cuda.synchronize()
    print(json.dumps({"policy": pol, "grid": grid, "mode": a.mode, "plan": a.plan,
                      "datatypes": [mg.DT_NAMES[d] for d in dts], "calls": runner.calls,
                      "single": sorted(runner.single_keys), "batch": sorted(runner.batch_keys),
                      "shapes": sorted(runner.shapes)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
