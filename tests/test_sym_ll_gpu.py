"""nexrSymLLAllReduce / nexrSymLLReduceScatter / nexrSymLLAllGather (sym_ll_*_kernel, nexr_sym.hip) and their
ring entries on the GPU against the numpy model (tests/sym_ll_cases.py), bit for bit.

Every call runs in one arena of device memory (test_sym_rs_ag_gpu.Arena): each buffer in a slot of its own with
guard bytes on both sides. After a call the whole arena is compared: every output must equal the model and
every other byte (guards, the inputs of an out-of-place call, the other chunks of an in-place one) must be as
it was; the status word must be 0. The windows of a group live in one allocation with guards between them;
their epoch words are compared with the model's round counts. No test forces a timeout or launches a grid that
is not resident."""
import importlib

import numpy as np
import pytest

import make_golden as mg
import sym_cases as sc
import sym_ll_cases as lc
from oracle.ring import ring_allreduce_expected_ll, tree_allreduce_expected, tree_topology
from test_sym_rs_ag_gpu import Arena

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

IDS = [sc.NAMES[d] for d in sc.DTYPES]
WGUARD = 256
FILL = 0xA5
COLLS = ("ar", "rs", "ag")


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("nex-nccl_amd.ring")


class Windows:
    """The n windows of a group, zeroed, 256-byte aligned with guards between them, a status word, and the
    model's epoch words."""

    def __init__(self, nexr, n, blocks):
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        self.n, self.R, self.H = n, nexr.SYM_LL_ROUND_PACKS, nexr.SYM_LL_HEADER_BYTES
        self.bytes = nexr.sym_ll_window_bytes(n, blocks)
        self.stride = (self.bytes + 2 * WGUARD + 255) // 256 * 256
        raw = torch.full((n * self.stride + 256,), FILL, dtype=torch.uint8, device="cuda")
        pad = (-raw.data_ptr()) % 256
        self.dev = raw[pad:pad + n * self.stride]
        for r in range(n):
            self.win(r).zero_()
        self.ptrs = [self.dev.data_ptr() + r * self.stride + WGUARD for r in range(n)]
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.words = [0] * 64
        torch.cuda.synchronize()

    def win(self, r):
        return self.dev[r * self.stride + WGUARD:r * self.stride + WGUARD + self.bytes]

    def preset(self, word, stale_flag):
        """Plain copies: every epoch word, and every line as a previous cycle would have left it."""
        host = np.empty(self.bytes // 4, dtype=np.uint32)
        host[:self.H // 4] = 0
        host[:64] = word
        host[self.H // 4:] = np.tile(np.array([0xDEADBEEF, stale_flag, 0xDEADBEEF, stale_flag], dtype=np.uint32),
                                     (self.bytes - self.H) // 16)
        for r in range(self.n):
            self.win(r).copy_(torch.from_numpy(host.view(np.uint8)))
        self.words = [word] * 64
        torch.cuda.synchronize()

    def advance(self, n_bytes, B):
        self.words = lc.advance(self.words, lc.packs(n_bytes), B, self.R)

    def snapshot(self):
        torch.cuda.synchronize()
        return self.dev.cpu().numpy().copy()

    def check(self, what):
        """status 0, every window's words the model's, the header's padding zero, the guards untouched."""
        got = self.snapshot()
        assert int(self.status.item()) == 0, what
        for r in range(self.n):
            at = r * self.stride
            assert (got[at:at + WGUARD] == FILL).all() and (got[at + WGUARD + self.bytes:at + self.stride] == FILL).all(), what
            hdr = got[at + WGUARD:at + WGUARD + self.H].view(np.uint32)
            assert hdr[:64].tolist() == self.words, (what, r, hdr[:64].tolist()[:4], self.words[:4])
            assert not hdr[64:].any(), what


def _seed(*a):
    return [int(x) for x in a]


def prepare(coll, dt, n, n_bytes, aligned, in_place=False):
    """(arena, input addresses, output addresses, count argument, [(arena byte, expected)])."""
    esz = 1 if coll == "ag" else sc.ESZ[dt]
    assert n_bytes % esz == 0
    count = n_bytes // esz
    in_off, out_off = lc.offsets(esz, n, aligned)
    if coll == "ar":
        ins = lc.ar_inputs(dt, n, count, _seed(1, dt, n, n_bytes))
        arena = Arena([n_bytes] * n + [n_bytes] * n, in_off + out_off)
        in_at, out_at = arena.at[:n], arena.at[n:]
        if in_place:
            out_at = in_at
        exp = [lc.ar_expected(dt, ins)] * n
    elif coll == "rs":
        ins = lc.rs_inputs(dt, n, count, _seed(2, dt, n, n_bytes))
        arena = Arena([n * n_bytes] * n + [n_bytes] * n, in_off + out_off)
        in_at, out_at = arena.at[:n], arena.at[n:]
        if in_place:
            out_at = [in_at[r] + r * n_bytes for r in range(n)]
        exp = lc.rs_expected(dt, ins, count)
    else:
        ins = lc.ag_inputs(n, n_bytes, _seed(3, n, n_bytes))
        arena = Arena([n_bytes] * n + [n * n_bytes] * n, in_off + out_off)
        in_at, out_at = arena.at[:n], arena.at[n:]
        if in_place:
            in_at = [out_at[r] + r * n_bytes for r in range(n)]
        exp = [lc.ag_expected(ins)] * n
    for r in range(n):
        arena.put(in_at[r], ins[r])
    arena.upload()
    if not aligned:
        assert all((arena.base + a) % 8 for a in in_at + out_at) or in_place
    return arena, in_at, out_at, count, ins, exp


def launch(nexr, W, coll, dt, arena, in_at, out_at, count, B, stream=0):
    i, o = [arena.base + a for a in in_at], [arena.base + a for a in out_at]
    tail = dict(n_blocks=B, status=W.status.data_ptr(), timeout_us=5_000_000, stream=stream)
    if coll == "ar":
        nexr.sym_ll_all_reduce(i, o, count, dt, W.ptrs, W.bytes, **tail)
    elif coll == "rs":
        nexr.sym_ll_reduce_scatter(i, o, count, dt, W.ptrs, W.bytes, **tail)
    else:
        nexr.sym_ll_all_gather(i, o, count, W.ptrs, W.bytes, **tail)


def run(nexr, W, coll, dt, n, n_bytes, B, aligned=True, in_place=False, expect=None):
    arena, in_at, out_at, count, ins, exp = prepare(coll, dt, n, n_bytes, aligned, in_place)
    if expect is not None:
        exp = expect(ins, count)
    launch(nexr, W, coll, dt, arena, in_at, out_at, count, B)
    W.advance(n_bytes, B)
    arena.check(list(zip(out_at, exp)), (coll, sc.NAMES[dt], n, n_bytes, B, aligned, in_place))
    assert int(W.status.item()) == 0


# ---- 1. the table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", lc.BLOCKS)
@pytest.mark.parametrize("dt", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("n", lc.RANKS)
def test_table(nexr, n, dt, B):
    """n x datatype x B, the three collectives on one group of windows: every pack count of pack_counts(), as
    whole packs and with a short last pack, at 8-byte aligned pointers and on the element-wise path."""
    W = Windows(nexr, n, B)
    for P in lc.pack_counts(W.R, B):
        for coll in COLLS:
            for n_bytes in lc.byte_counts(P, sc.ESZ[dt], coll == "ag"):
                for aligned in (True, False):
                    run(nexr, W, coll, dt, n, n_bytes, B, aligned)
    W.check((n, sc.NAMES[dt], B))


# ---- 2. many ranks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dt", [(9, sc.BF16), (17, sc.F32), (9, sc.F16)])
def test_many_ranks_fold_in_groups_of_eight(nexr, n, dt):
    W = Windows(nexr, n, 1)
    for coll in COLLS:
        run(nexr, W, coll, dt, n, 8 * W.R + sc.ESZ[dt], 1, aligned=False)
    W.check((n, sc.NAMES[dt]))


# ---- 3. in place -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sc.DTYPES, ids=IDS)
def test_in_place(nexr, dt):
    """outputs[r] == inputs[r] (all-reduce), outputs[r] == chunk r of inputs[r] (reduce-scatter), inputs[r] at
    its place in outputs[r] (all-gather), at three ranks, with a short last pack."""
    W = Windows(nexr, 3, 2)
    for coll in COLLS:
        for n_bytes in (8 * (W.R + 5), 8 * (2 * W.R + 1) + sc.ESZ[dt]):
            for aligned in (True, False):
                run(nexr, W, coll, dt, 3, n_bytes, 2, aligned, in_place=True)
    W.check(sc.NAMES[dt])


# ---- 4. a sequence without a host wait ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", sc.DTYPES, ids=IDS)
def test_six_calls_on_one_stream_without_a_wait(nexr, dt):
    """Six calls rotate the collectives with B = 2, 3, 1, alternating a full round per team and three lines per
    team, so stale lines of earlier rounds lie in both buffers under later ones; the blocks end with different
    epoch words."""
    n = 3
    W = Windows(nexr, n, 3)
    calls = []
    for k in range(6):
        coll, B = COLLS[k % 3], (2, 3, 1)[k % 3]
        n_bytes = 8 * B * (W.R if k % 2 == 0 else 3)
        calls.append((coll, B, n_bytes) + prepare(coll, dt, n, n_bytes, k % 2 == 0))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        for coll, B, n_bytes, arena, in_at, out_at, count, _ins, _exp in calls:
            launch(nexr, W, coll, dt, arena, in_at, out_at, count, B, stream=stream.cuda_stream)
            W.advance(n_bytes, B)
    stream.synchronize()
    for k, (coll, B, n_bytes, arena, _in_at, out_at, _count, _ins, exp) in enumerate(calls):
        arena.check(list(zip(out_at, exp)), ("sequence", k, coll, B))
    assert W.words[:4] == [6, 4, 2, 0]
    W.check(("sequence", sc.NAMES[dt]))


# ---- 5. the wrap -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stale", [2, 3])
def test_wrap_cleans_the_lines_of_the_cycle_that_ends(nexr, stale):
    """Words at 0xfffffffa and every line {0xdeadbeef, stale, 0xdeadbeef, stale}, as the previous cycle would
    have left them. Four calls of three lines per team use flags 0xfffffffc .. 0xffffffff; four calls of a full
    round then use flags 2 .. 5. Without the cleanup at 0xfffffffe / 0xffffffff the stale lines satisfy the polls
    of flag 2 / 3 and the outputs are 0xdeadbeef: a wrong answer, never a hang."""
    n, B, dt = 3, 2, sc.F32
    W = Windows(nexr, n, B)
    W.preset(0xFFFFFFFA, stale)
    for k in range(8):
        n_bytes = 8 * B * (3 if k < 4 else W.R)
        run(nexr, W, COLLS[k % 3], dt, n, n_bytes, B)
        assert W.words[:3] == [lc.flags(0xFFFFFFFA, k + 1)[1]] * 2 + [0xFFFFFFFA]
    assert W.words[:2] == [4, 4]
    W.check(("wrap", stale))


# ---- 6. semantics ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["shipped", "fork"])
def test_semantics_modes(nexr, mode):
    """shipped: every add returns its first operand, so the result is rank 0's input through the two casts (a
    NaN of a 16-bit type still becomes 0x7fff); fork is nccl."""
    before = nexr.get_semantics()
    try:
        nexr.set_semantics(nexr.Semantics.Shipped if mode == "shipped" else nexr.Semantics.Fork)
        W = Windows(nexr, 3, 2)
        for dt in sc.DTYPES:
            n_bytes = 8 * (W.R + 3) + sc.ESZ[dt]
            if mode == "shipped":
                run(nexr, W, "ar", dt, 3, n_bytes, 2, expect=lambda ins, c: [lc.ar_expected_shipped(dt, ins)] * 3)
                run(nexr, W, "rs", dt, 3, n_bytes, 2, expect=lambda ins, c: lc.rs_expected_shipped(dt, ins, c))
            else:
                run(nexr, W, "ar", dt, 3, n_bytes, 2)
                run(nexr, W, "rs", dt, 3, n_bytes, 2)
            run(nexr, W, "ag", dt, 3, n_bytes, 2)
        W.check(mode)
    finally:
        nexr.set_semantics(before)


# ---- 7. residency ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coll", COLLS)
def test_a_grid_that_is_not_resident_is_invalid_usage_and_launches_nothing(nexr, coll, monkeypatch):
    n, B, dt = 2, 2, sc.F32
    W = Windows(nexr, n, B)
    n_bytes = 8 * 3 * B
    arena, in_at, out_at, count, _ins, exp = prepare(coll, dt, n, n_bytes, True)
    before = W.snapshot()
    monkeypatch.setenv("NEXR_TEST_SYM_LL_RESIDENT", "3")
    with pytest.raises(nexr.NexrError) as e:
        launch(nexr, W, coll, dt, arena, in_at, out_at, count, B)
    assert e.value.code == nexr.Result.InvalidUsage
    arena.check([], ("rejected", coll))
    assert np.array_equal(W.snapshot(), before)
    monkeypatch.setenv("NEXR_TEST_SYM_LL_RESIDENT", "4")
    launch(nexr, W, coll, dt, arena, in_at, out_at, count, B)
    arena.check(list(zip(out_at, exp)), ("hook at 4", coll))
    monkeypatch.delenv("NEXR_TEST_SYM_LL_RESIDENT")
    launch(nexr, W, coll, dt, arena, in_at, out_at, count, B)
    arena.check(list(zip(out_at, exp)), ("no hook", coll))
    W.advance(n_bytes, B)
    W.advance(n_bytes, B)
    W.check(("residency", coll))


# ---- 8. the ring library -----------------------------------------------------------------------------------------
BUFF = 8 * 16 * 512


def _dev(arrs):
    out = [torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() for a in arrs]
    torch.cuda.synchronize()
    return out


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _same(dt, got, exp, what):
    for r, e in enumerate(exp):
        assert mg.canon_bytes(dt, got[r].cpu().numpy()) == mg.canon_bytes(dt, e), (what, r)


@pytest.mark.parametrize("n", [2, 4])
def test_ring_entries_interleaved_with_a_ring_ll_all_reduce_and_a_tree_call(nexr, ring, oracle, n):
    """all_reduce_symmetric_ll, reduce_scatter_symmetric_ll into chunk r of every rank's buffer and
    all_gather_symmetric_ll in place on it, between a ring LL all-reduce in group launches and a tree call of
    one device communicator. Ring and tree stay exact against oracle.ring, the symmetric calls against the
    model, and queued() is left as it was."""
    dt, count = mg.F32, 50_021
    links = tree_topology(n, 0, 0)
    sdt, sesz = sc.BF16, 2
    c = (8 * (2 * nexr.SYM_LL_ROUND_PACKS + 3) + sesz) // sesz
    ins = lc.rs_inputs(sdt, n, c, [0x7400 + n])
    exp_ar = lc.ar_expected(sdt, ins)
    exp_rs = np.concatenate(lc.rs_expected(sdt, ins, c))
    assert np.array_equal(exp_ar, exp_rs)  # the same fold: the all-reduce is the gathered reduce-scatter
    send = _dev(ins)
    recv = [torch.full_like(s, 0x55) for s in send]
    chunk = [recv[r].data_ptr() + r * c * sesz for r in range(n)]
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF, None, 20000, ring.PROTO_LL) as comm:
        comm.set_ll_group(True)
        for call, what in enumerate(("ring", "sym_ar", "tree", "sym_rs", "sym_ag", "ring", "sym_ar")):
            if what.startswith("sym"):
                q = comm.queued()
                if what == "sym_ar":
                    out = [torch.full_like(s, 0x33) for s in send]
                    comm.all_reduce_symmetric_ll(_ptrs(send), _ptrs(out), n * c, sdt, 0, n_blocks=(call % 4) + 1)
                    for r in range(n):
                        assert np.array_equal(out[r].cpu().numpy().view(np.uint16), exp_ar), (n, r)
                elif what == "sym_rs":
                    comm.reduce_scatter_symmetric_ll(_ptrs(send), chunk, c, sdt, 0, n_blocks=3)
                    for r in range(n):
                        got = recv[r].cpu().numpy().view(np.uint16)
                        assert np.array_equal(got[r * c:(r + 1) * c], exp_rs[r * c:(r + 1) * c]), (n, r)
                        assert (np.delete(got, np.s_[r * c:(r + 1) * c]) == 0x55).all()
                else:
                    comm.all_gather_symmetric_ll(chunk, _ptrs(recv), c, sdt, n_blocks=16)
                    for r in range(n):
                        assert np.array_equal(recv[r].cpu().numpy().view(np.uint16), exp_rs), (n, r)
                for r in range(n):
                    assert np.array_equal(send[r].cpu().numpy().view(np.uint16), ins[r])
                assert comm.queued() == q
                continue
            inputs = mg.gen_inputs(dt, n, count, 0x7500 + 16 * n + call, special=True)
            rs = _dev(inputs)
            rr = [torch.zeros_like(s) for s in rs]
            torch.cuda.synchronize()
            if what == "ring":
                comm.all_reduce(_ptrs(rs), _ptrs(rr), count, dt, 0)
                want = ring_allreduce_expected_ll(inputs, dt, 0, BUFF)
                if torch.cuda.device_count() == 1:
                    assert comm.queued() == 3
            else:
                comm.tree_all_reduce(_ptrs(rs), _ptrs(rr), count, dt, 0)
                want = tree_allreduce_expected(inputs, dt, 0, links, "ll")
            _same(dt, rr, want, (n, call, what))


def test_ring_entries_one_rank_and_zero_count(nexr, ring):
    x = torch.arange(1000, dtype=torch.float32, device="cuda")
    y, z, w = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    with ring.RingComm(1, ring.DEVICE_MEMORY, 1 << 18, None, 20000) as comm:
        comm.all_reduce_symmetric_ll([x.data_ptr()], [y.data_ptr()], 1000, sc.F32, 0)
        comm.reduce_scatter_symmetric_ll([x.data_ptr()], [z.data_ptr()], 1000, sc.F32, 0)
        comm.all_gather_symmetric_ll([x.data_ptr()], [w.data_ptr()], 1000, sc.F32)
        torch.cuda.synchronize()
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x, w)
    with ring.RingComm(2, ring.DEVICE_MEMORY, 1 << 18, None, 20000) as comm:
        p = [x.data_ptr(), y.data_ptr()]
        comm.all_reduce_symmetric_ll(p, p, 0, sc.F32, 0)
        comm.reduce_scatter_symmetric_ll(p, p, 0, sc.F32, 0)
        comm.all_gather_symmetric_ll(p, p, 0, sc.F32)
        torch.cuda.synchronize()
        assert torch.equal(x, y) and torch.equal(x, z)
        for bad in (lambda: comm.all_reduce_symmetric_ll(p, p, 8, sc.F32, 1),
                    lambda: comm.all_reduce_symmetric_ll(p, p, 8, sc.F32, 0, n_blocks=17),
                    lambda: comm.all_gather_symmetric_ll(p, p, 1 << 31, 1)):
            with pytest.raises(nexr.NexrError) as e:
                bad()
            assert e.value.code == nexr.Result.InvalidArgument
        assert comm.queued() == 0
        # a SIMPLE communicator has no status word until its first symmetric LL call makes one
        a = torch.ones(64, dtype=torch.float32, device="cuda")
        b = torch.full((64,), 2.0, dtype=torch.float32, device="cuda")
        comm.all_reduce_symmetric_ll([a.data_ptr(), b.data_ptr()], [a.data_ptr(), b.data_ptr()], 64, sc.F32, 0)
        torch.cuda.synchronize()
        assert (a == 3.0).all() and (b == 3.0).all()


def test_ring_entries_are_invalid_usage_on_a_host_memory_communicator(nexr, ring):
    """The library's own host-memory communicator (its steps run on the GPU, its buffers are host memory)."""
    bufs = [np.ones(128, dtype=np.float32) for _ in range(4)]
    p = [b.ctypes.data for b in bufs]
    with ring.RingComm(2, ring.HOST_MEMORY, 1 << 18, None, 20000) as comm:
        for count in (0, 64):
            for call in (lambda: comm.all_reduce_symmetric_ll(p[:2], p[2:], count, sc.F32, 0),
                         lambda: comm.reduce_scatter_symmetric_ll(p[:2], p[2:], count, sc.F32, 0),
                         lambda: comm.all_gather_symmetric_ll(p[:2], p[2:], count, sc.F32)):
                with pytest.raises(nexr.NexrError) as e:
                    call()
                assert e.value.code == nexr.Result.InvalidUsage
        comm.all_gather(p[:2], p[2:], 64, sc.F32)
        assert all((b == 1.0).all() for b in bufs)
