"""nexrSymReduceScatter / nexrSymAllGather (sym_reduce_scatter_kernel, sym_all_gather_kernel, nexr_sym.hip) and
their ring entries on the GPU against the numpy model (tests/sym_rs_ag_cases.py), bit for bit.

Every call runs in one arena of device memory: each buffer in a slot of its own with guard bytes on both
sides, the ranks' slots at offsets that differ mod 16. After a call the whole arena is compared: every output
must equal the model and every other byte (guards, the inputs of an out-of-place call, the other chunks of an
in-place one) must be as it was."""
import importlib

import numpy as np
import pytest

import make_golden as mg
import sym_cases as sc
import sym_rs_ag_cases as rc
from oracle.ring import ring_allreduce_expected, ring_allreduce_expected_ll, tree_allreduce_expected, tree_topology

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 64
FILL = 0xA5
IDS = [sc.NAMES[d] for d in sc.DTYPES]


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("nex-nccl_amd.ring")


class Arena:
    """One slot per (size, offset) in one device allocation, 256-byte aligned; slot i's buffer starts at
    at[i]."""

    def __init__(self, sizes, offs):
        self.at, top = [], 0
        for size, off in zip(sizes, offs):
            self.at.append(top + GUARD + off)
            top += (size + 16 + 2 * GUARD + 255) // 256 * 256
        self.host = np.full(top, FILL, dtype=np.uint8)
        self.dev = None

    def put(self, at, x):
        raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        self.host[at:at + raw.size] = raw

    def upload(self):
        assert torch.cuda.is_available(), "GPU tests need an MI355X"
        raw = torch.empty(self.host.size + 256, dtype=torch.uint8, device="cuda")
        pad = (-raw.data_ptr()) % 256
        self.dev = raw[pad:pad + self.host.size]
        self.dev.copy_(torch.from_numpy(self.host))
        self.base = self.dev.data_ptr()
        assert self.base % 256 == 0
        torch.cuda.synchronize()

    def check(self, outs, what):
        """outs: (arena byte, expected array) per output. Outputs == expected; everything else untouched."""
        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        want = self.host.copy()
        for at, exp in outs:
            eb = np.ascontiguousarray(exp).view(np.uint8).reshape(-1)
            want[at:at + eb.size] = eb
        if not np.array_equal(got, want):
            for k, (at, exp) in enumerate(outs):
                eb = np.ascontiguousarray(exp).view(np.uint8).reshape(-1)
                bad = np.flatnonzero(got[at:at + eb.size] != eb)
                if bad.size:
                    i = int(bad[0])
                    raise AssertionError(f"{what}: output {k}: {bad.size} of {eb.size} bytes differ, first at byte {i}: "
                                         f"got {int(got[at + i]):#x}, expected {int(eb[i]):#x}")
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{what}: {bad.size} bytes outside the outputs changed, first at arena byte {int(bad[0])}")
        self.host = want


# ---- reduce-scatter ----------------------------------------------------------------------------------------------
def rs_arena(dt, n, count, ins, mode):
    """n input slots of n * count elements, n output slots of count elements; (arena, in_at, out_at). mode:
    out_of_place: outputs in their own slots; in_place: outputs[r] = chunk r of inputs[r] (NCCL's form);
    on_next_rank: outputs[r] = chunk r of inputs[r + 1]."""
    esz = sc.ESZ[dt]
    in_off, out_off = rc.rs_offsets(esz, n)
    arena = Arena([n * count * esz] * n + [count * esz] * n, in_off + out_off)
    in_at, out_at = arena.at[:n], arena.at[n:]
    if mode == "in_place":
        out_at = [in_at[r] + r * count * esz for r in range(n)]
    elif mode == "on_next_rank":
        out_at = [in_at[(r + 1) % n] + r * count * esz for r in range(n)]
    for r in range(n):
        arena.put(in_at[r], ins[r])
    arena.upload()
    assert len({(arena.base + a) % 16 for a in in_at[:2]}) == 2
    return arena, in_at, out_at


def run_rs(nexr, dt, n, count, mode, ins, exp):
    arena, in_at, out_at = rs_arena(dt, n, count, ins, mode)
    nexr.sym_reduce_scatter([arena.base + a for a in in_at], [arena.base + a for a in out_at], count, dt)
    arena.check(list(zip(out_at, exp)), (sc.NAMES[dt], n, count, mode))
    return arena, in_at, out_at


@pytest.mark.parametrize("dt", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("n", rc.RANKS)
def test_reduce_scatter_table(nexr, n, dt):
    """n x datatype: every count of rs_counts() out of place, in NCCL's in-place form and with outputs[r] on
    chunk r of rank r + 1's input; one expectation per count, shared by the three."""
    for count in rc.rs_counts(sc.ESZ[dt], n):
        ins = rc.rs_inputs(dt, n, count, [n, dt, count])
        exp = rc.rs_expected(dt, ins, count)
        for mode in rc.MODES:
            run_rs(nexr, dt, n, count, mode, ins, exp)


@pytest.mark.parametrize("n,dt", [(13, sc.BF16), (64, sc.F32)])
def test_reduce_scatter_many_ranks_fold_in_groups_of_peers(nexr, n, dt):
    """Beyond 8 ranks the fold goes on in groups of 8 peers (13: one whole group, then 4 and 1; 64: eight)."""
    count = 2 * 2048 // sc.ESZ[dt] + 37
    ins = rc.rs_inputs(dt, n, count, [n, dt, count])
    run_rs(nexr, dt, n, count, "out_of_place", ins, rc.rs_expected(dt, ins, count))


def test_reduce_scatter_eight_ranks_of_1_mib_chunks(nexr):
    """8 ranks of fp32 with 1 MiB chunks (8 MiB per input), compared whole."""
    n, count = 8, (1 << 20) // 4
    ins = rc.rs_inputs(sc.F32, n, count, [n, count])
    run_rs(nexr, sc.F32, n, count, "out_of_place", ins, rc.rs_expected(sc.F32, ins, count))


@pytest.mark.parametrize("mode", ["shipped", "fork"])
def test_reduce_scatter_semantics_modes(nexr, mode):
    """shipped: every add returns its first operand, so output r is rank r's own chunk through the two casts (a
    NaN of a 16-bit type still becomes 0x7fff); fork is nccl."""
    before = nexr.get_semantics()
    try:
        nexr.set_semantics(nexr.Semantics.Shipped if mode == "shipped" else nexr.Semantics.Fork)
        for dt in sc.DTYPES:
            count = rc.rs_counts(sc.ESZ[dt], 3)[-2]
            ins = rc.rs_inputs(dt, 3, count, [3, dt, 0x5E])
            exp = rc.rs_expected_shipped(dt, ins, count) if mode == "shipped" else rc.rs_expected(dt, ins, count)
            run_rs(nexr, dt, 3, count, "out_of_place", ins, exp)
    finally:
        nexr.set_semantics(before)


@pytest.mark.parametrize("dt", sc.DTYPES, ids=IDS)
def test_reduce_scatter_two_calls_back_to_back_the_second_in_place(nexr, dt):
    """Both queued on one stream with no wait between them. The first scatters chunks of n * c elements out of
    place; the second takes those outputs as its inputs (n chunks of c elements) in NCCL's in-place form, so it
    reads what the first wrote."""
    n, esz = 5, sc.ESZ[dt]
    c = rc.rs_counts(esz, n)[-2]
    ins = rc.rs_inputs(dt, n, n * c, [0x5B, dt])
    arena, in_at, out_at = rs_arena(dt, n, n * c, ins, "out_of_place")
    mid = [arena.base + a for a in out_at]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        nexr.sym_reduce_scatter([arena.base + a for a in in_at], mid, n * c, dt, stream=stream.cuda_stream)
        nexr.sym_reduce_scatter(mid, [mid[r] + r * c * esz for r in range(n)], c, dt, stream=stream.cuda_stream)
    stream.synchronize()
    exp1 = rc.rs_expected(dt, ins, n * c)
    exp2 = rc.rs_expected(dt, exp1, c)
    final = [e.copy() for e in exp1]
    for r in range(n):
        final[r][r * c:(r + 1) * c] = exp2[r]
    arena.check(list(zip(out_at, final)), ("back to back", sc.NAMES[dt]))


# ---- all-gather ------------------------------------------------------------------------------------------------
def run_ag(nexr, n, n_bytes, parity, mode):
    """out_of_place: n input slots and n output slots; in_place: inputs[r] is chunk r of outputs[r];
    even_in_place: that for the even ranks only."""
    ins = rc.ag_inputs(n, n_bytes, [n, n_bytes, parity])
    in_off, out_off = rc.ag_offsets(n, parity)
    arena = Arena([n_bytes] * n + [n * n_bytes] * n, in_off + out_off)
    out_at = arena.at[n:]
    placed = [mode == "in_place" or (mode == "even_in_place" and r % 2 == 0) for r in range(n)]
    in_at = [out_at[r] + r * n_bytes if placed[r] else arena.at[r] for r in range(n)]
    for r in range(n):
        arena.put(in_at[r], ins[r])
    arena.upload()
    nexr.sym_all_gather([arena.base + a for a in in_at], [arena.base + a for a in out_at], n_bytes)
    exp = rc.ag_expected(ins)
    arena.check([(a, exp) for a in out_at], ("all-gather", n, n_bytes, parity, mode))


@pytest.mark.parametrize("mode", rc.AG_MODES)
@pytest.mark.parametrize("n", rc.AG_RANKS)
def test_all_gather_table(nexr, n, mode):
    """n x placement: every size of AG_BYTES at odd and at even byte offsets, random bytes."""
    for n_bytes in rc.AG_BYTES:
        for parity in (0, 1):
            run_ag(nexr, n, n_bytes, parity, mode)


@pytest.mark.parametrize("mode", rc.AG_MODES)
def test_all_gather_64_ranks(nexr, mode):
    run_ag(nexr, 64, 2049, 1, mode)


# ---- the ring library ----------------------------------------------------------------------------------------------
BUFF = {"simple": 1 << 18, "ll_group": 8 * 16 * 512, "simple_group": 8 * 4096}


def _dev(arrs):
    out = [torch.from_numpy(np.ascontiguousarray(a).copy()).cuda() for a in arrs]
    torch.cuda.synchronize()
    return out


def _ptrs(ts):
    return [t.data_ptr() for t in ts]


def _same(dt, got, exp, what):
    for r, e in enumerate(exp):
        assert mg.canon_bytes(dt, got[r].cpu().numpy()) == mg.canon_bytes(dt, e), (what, r)


@pytest.mark.parametrize("mode", ["simple", "ll_group", "simple_group"])
@pytest.mark.parametrize("n", [2, 4, 8])
def test_ring_symmetric_pair_interleaved_with_ring_and_tree_calls(nexr, ring, oracle, n, mode):
    """reduce_scatter_symmetric into chunk r of every rank's receive buffer, then all_gather_symmetric in place
    on that buffer, between ring and tree all-reduces of one device communicator: host-sequenced SIMPLE, LL in
    group launches, SIMPLE in group launches. Every ring and tree call stays exact against oracle.ring, the
    gathered result is every chunk folded from its own rank, and queued() is left as it was."""
    dt, count = mg.F32, 50_021
    proto = ring.PROTO_LL if mode == "ll_group" else ring.PROTO_SIMPLE
    pname = "ll" if mode == "ll_group" else "simple"
    links = tree_topology(n, 0, 0)
    sdt, sesz = sc.BF16, 2
    c = rc.rs_counts(sesz, n)[-1]
    ins = rc.rs_inputs(sdt, n, c, [0x7200 + n])
    exp = np.concatenate(rc.rs_expected(sdt, ins, c))
    send = _dev(ins)
    recv = [torch.full_like(s, 0x55) for s in send]
    chunk = [recv[r].data_ptr() + r * c * sesz for r in range(n)]
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF[mode], None, 20000, proto) as comm:
        if mode == "ll_group":
            comm.set_ll_group(True)
        if mode == "simple_group":
            comm.set_simple_group(True)
        for call, what in enumerate(("ring", "sym_rs", "tree", "sym_ag", "ring")):
            if what.startswith("sym"):
                q = comm.queued()
                if what == "sym_rs":
                    comm.reduce_scatter_symmetric(_ptrs(send), chunk, c, sdt, 0)
                    for r in range(n):
                        got = recv[r].cpu().numpy().view(np.uint16)
                        assert np.array_equal(got[r * c:(r + 1) * c], exp[r * c:(r + 1) * c]), (mode, n, r)
                        assert (np.delete(got, np.s_[r * c:(r + 1) * c]) == 0x55).all()
                        assert np.array_equal(send[r].cpu().numpy().view(np.uint16), ins[r])
                else:
                    comm.all_gather_symmetric(chunk, _ptrs(recv), c, sdt)
                    for r in range(n):
                        assert np.array_equal(recv[r].cpu().numpy().view(np.uint16), exp), (mode, n, r)
                assert comm.queued() == q
                continue
            inputs = mg.gen_inputs(dt, n, count, 0x7300 + 16 * n + call, special=True)
            rs = _dev(inputs)
            rr = [torch.zeros_like(s) for s in rs]
            torch.cuda.synchronize()
            if what == "ring":
                comm.all_reduce(_ptrs(rs), _ptrs(rr), count, dt, 0)
                want = (ring_allreduce_expected_ll(inputs, dt, 0, BUFF[mode]) if mode == "ll_group"
                        else ring_allreduce_expected(inputs, dt, 0, buff_bytes=BUFF[mode]))
                if mode != "simple" and torch.cuda.device_count() == 1:
                    assert comm.queued() == 3
            else:
                comm.tree_all_reduce(_ptrs(rs), _ptrs(rr), count, dt, 0)
                want = tree_allreduce_expected(inputs, dt, 0, links, pname)
            _same(dt, rr, want, (mode, n, call, what))


def test_ring_symmetric_one_rank_and_zero_count(nexr, ring):
    x = torch.arange(1000, dtype=torch.float32, device="cuda")
    y = torch.zeros_like(x)
    z = torch.zeros_like(x)
    with ring.RingComm(1, ring.DEVICE_MEMORY, 1 << 18, None, 20000) as comm:
        comm.reduce_scatter_symmetric([x.data_ptr()], [y.data_ptr()], 1000, sc.F32, 0)
        comm.all_gather_symmetric([x.data_ptr()], [z.data_ptr()], 1000, sc.F32)
        torch.cuda.synchronize()
        assert torch.equal(x, y) and torch.equal(x, z)
    with ring.RingComm(2, ring.DEVICE_MEMORY, 1 << 18, None, 20000) as comm:
        p = [x.data_ptr(), y.data_ptr()]
        comm.reduce_scatter_symmetric(p, p, 0, sc.F32, 0)
        comm.all_gather_symmetric(p, p, 0, sc.F32)
        torch.cuda.synchronize()
        assert torch.equal(x, y) and torch.equal(x, z)
        with pytest.raises(nexr.NexrError) as e:
            comm.reduce_scatter_symmetric(p, p, 8, sc.F32, 1)
        assert e.value.code == nexr.Result.InvalidArgument
        assert comm.queued() == 0


def test_ring_symmetric_is_invalid_usage_on_a_host_memory_communicator(nexr, ring):
    """The library's own host-memory communicator (its steps run on the GPU, its buffers are host memory)."""
    bufs = [np.ones(128, dtype=np.float32) for _ in range(4)]
    p = [b.ctypes.data for b in bufs]
    with ring.RingComm(2, ring.HOST_MEMORY, 1 << 18, None, 20000) as comm:
        for count in (0, 64):
            with pytest.raises(nexr.NexrError) as e:
                comm.reduce_scatter_symmetric(p[:2], p[2:], count, sc.F32, 0)
            assert e.value.code == nexr.Result.InvalidUsage
            with pytest.raises(nexr.NexrError) as e:
                comm.all_gather_symmetric(p[:2], p[2:], count, sc.F32)
            assert e.value.code == nexr.Result.InvalidUsage
        comm.all_gather(p[:2], p[2:], 64, sc.F32)
        assert all((b == 1.0).all() for b in bufs)
