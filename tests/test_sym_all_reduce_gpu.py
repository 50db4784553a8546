"""nexrSymAllReduce (sym_all_reduce_kernel, nexr_sym.hip) and nexrRingAllReduceSymmetric on the GPU against
the numpy restatement of the rule (tests/sym_cases.py), bit for bit.

Every call runs in one arena of device memory: each buffer in a slot of its own with guard bytes on both
sides, rank 0's buffers at the offsets that realise the case's A and D, the other ranks' at offsets that
differ from rank 0's. After a call every output must equal the expectation and every other byte of the arena
(guards, and the inputs of an out-of-place call) must be as it was."""
import importlib

import numpy as np
import pytest

import make_golden as mg
import sym_cases as sc
from oracle.ring import ring_allreduce_expected, ring_allreduce_expected_ll, tree_allreduce_expected, tree_topology

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def ring(nexr):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return importlib.import_module("nex-nccl_amd.ring")


class Arena:
    """2n slots (inputs, then outputs) in one device allocation, 256-byte aligned."""

    def __init__(self, n, n_bytes, in_off, out_off, in_place):
        self.n, self.n_bytes, self.in_place = n, n_bytes, in_place
        self.slot = (n_bytes + 16 + 2 * GUARD + 255) // 256 * 256
        self.host = np.full(2 * n * self.slot, FILL, dtype=np.uint8)
        self.in_at = [r * self.slot + GUARD + in_off[r] for r in range(n)]
        self.out_at = list(self.in_at) if in_place else [(n + r) * self.slot + GUARD + out_off[r] for r in range(n)]
        self.dev = None

    def upload(self, inputs):
        for r, x in enumerate(inputs):
            raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
            assert raw.size == self.n_bytes
            self.host[self.in_at[r]:self.in_at[r] + raw.size] = raw
        raw = torch.empty(self.host.size + 256, dtype=torch.uint8, device="cuda")
        pad = (-raw.data_ptr()) % 256
        self.dev = raw[pad:pad + self.host.size]
        self.dev.copy_(torch.from_numpy(self.host))
        self.base = self.dev.data_ptr()
        assert self.base % 256 == 0
        torch.cuda.synchronize()

    def in_ptrs(self):
        return [self.base + a for a in self.in_at]

    def out_ptrs(self):
        return [self.base + a for a in self.out_at]

    def check(self, dt, exp, what):
        """Outputs == exp for every rank; everything else untouched."""
        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        want = self.host.copy()
        eb = np.ascontiguousarray(exp).view(np.uint8).reshape(-1)
        for r in range(self.n):
            want[self.out_at[r]:self.out_at[r] + self.n_bytes] = eb
        if not np.array_equal(got, want):
            for r in range(self.n):
                g = got[self.out_at[r]:self.out_at[r] + self.n_bytes].view(sc.UINT[dt])
                bad = np.flatnonzero(g != np.ascontiguousarray(exp).view(sc.UINT[dt]))
                if bad.size:
                    i = int(bad[0])
                    raise AssertionError(f"{what}: rank {r}: {bad.size} of {g.size} elements differ, first at {i}: "
                                         f"got {int(g[i]):#x}, expected {int(exp[i]):#x}")
            bad = np.flatnonzero(got != want)
            raise AssertionError(f"{what}: {bad.size} bytes outside the outputs changed, first at arena byte {int(bad[0])}")
        self.host = want


def run_case(nexr, dt, n, B, count, A, D, in_place, seed=None, semantics=None):
    esz = sc.ESZ[dt]
    in_off, out_off = sc.rank_offsets(esz, n, A, D, in_place)
    owner, region = sc.owner_map(n, B, esz, count, A, D)
    ins = sc.make_inputs(dt, n, count, seed if seed is not None else sc.case_seed(n, B, dt, count, A, D, in_place),
                         owner, region)
    arena = Arena(n, count * esz, in_off, out_off, in_place)
    arena.upload(ins)
    assert arena.in_ptrs()[0] % 16 == A and (arena.in_ptrs()[0] - arena.out_ptrs()[0]) % 16 == D
    nexr.sym_all_reduce(arena.in_ptrs(), arena.out_ptrs(), count, dt, n_blocks=B)
    exp = sc.expected_shipped(dt, ins, owner) if semantics == "shipped" else sc.expected(dt, ins, owner)
    arena.check(dt, exp, (sc.NAMES[dt], n, B, count, A, D, in_place))
    return arena, exp, ins


@pytest.mark.parametrize("group", sc.GROUPS)
@pytest.mark.parametrize("dt", sc.DTYPES, ids=[sc.NAMES[d] for d in sc.DTYPES])
@pytest.mark.parametrize("B", sc.BLOCKS)
@pytest.mark.parametrize("n", sc.RANKS)
def test_table(nexr, n, B, dt, group):
    """n x B x datatype: every count of sym_cases.counts() under every D and in place, A going round its
    values; the count with all three regions under every (A, D)."""
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    cases = sc.table_cases(n, B, dt, group)
    assert cases
    for count, A, D, in_place in cases:
        run_case(nexr, dt, n, B, count, A, D, in_place)


@pytest.mark.parametrize("n,B,dt", [(13, 2, sc.BF16), (64, 1, sc.F32), (64, 64, sc.F16)])
def test_many_ranks_fold_in_groups_of_peers(nexr, n, B, dt):
    """Beyond 8 ranks the fold goes on in groups of 8 peers (13: one whole group and a part; 64: eight)."""
    esz = sc.ESZ[dt]
    count = n * B * 8192 // esz + n * B * 2048 // esz + 37 if B < 64 else n * 2048 // esz * 3 + 333
    run_case(nexr, dt, n, B, count, 4, 0, False)


def test_full_size_eight_ranks_of_4_mib(nexr):
    """8 ranks x 4 MiB of fp32, compared whole."""
    run_case(nexr, sc.F32, 8, 1, 1 << 20, 0, 0, False)


@pytest.mark.parametrize("mode", ["shipped", "fork"])
def test_semantics_modes(nexr, mode):
    """shipped: every add returns its first operand, so an element is its owner's input through the two casts
    (a NaN of a 16-bit type still becomes 0x7fff); fork is nccl."""
    before = nexr.get_semantics()
    try:
        nexr.set_semantics(nexr.Semantics.Shipped if mode == "shipped" else nexr.Semantics.Fork)
        for dt in sc.DTYPES:
            esz = sc.ESZ[dt]
            run_case(nexr, dt, 3, 1, 2 * 3 * 8192 // esz + 3 * 3 * 2048 // esz + 37, 4, 0, False, semantics=mode)
    finally:
        nexr.set_semantics(before)


@pytest.mark.parametrize("dt", sc.DTYPES, ids=[sc.NAMES[d] for d in sc.DTYPES])
def test_two_calls_back_to_back_the_second_in_place(nexr, dt):
    """Both queued on one stream with no wait between them: the second reads what the first wrote."""
    n, B, esz = 5, 2, sc.ESZ[dt]
    count = sc.counts(n, B, esz)[-1]
    A, D = 8, 0
    in_off, out_off = sc.rank_offsets(esz, n, A, D, False)
    owner, region = sc.owner_map(n, B, esz, count, A, D)
    ins = sc.make_inputs(dt, n, count, [0x5B, dt], owner, region)
    arena = Arena(n, count * esz, in_off, out_off, False)
    arena.upload(ins)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        nexr.sym_all_reduce(arena.in_ptrs(), arena.out_ptrs(), count, dt, n_blocks=B, stream=stream.cuda_stream)
        nexr.sym_all_reduce(arena.out_ptrs(), arena.out_ptrs(), count, dt, n_blocks=B, stream=stream.cuda_stream)
    stream.synchronize()
    exp1 = sc.expected(dt, ins, owner)
    owner2, _ = sc.owner_map(n, B, esz, count, out_off[0], 0)
    exp2 = sc.expected(dt, [exp1] * n, owner2)
    arena.check(dt, exp2, ("back to back", sc.NAMES[dt]))


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


def _sym(comm, n, dt, count, B, seed, in_place):
    """One all_reduce_symmetric on tensors of its own (torch allocations: A = 0, D = 0), exact; queued() is
    what it was."""
    esz = sc.ESZ[dt]
    owner, region = sc.owner_map(n, B, esz, count, 0, 0)
    ins = sc.make_inputs(dt, n, count, seed, owner, region)
    send = _dev(ins)
    recv = send if in_place else [torch.full_like(s, 0x55) for s in send]
    assert all(p % 16 == 0 for p in _ptrs(send) + _ptrs(recv))
    torch.cuda.synchronize()
    q = comm.queued()
    comm.all_reduce_symmetric(_ptrs(send), _ptrs(recv), count, dt, 0, B)
    assert comm.queued() == q
    exp = sc.expected(dt, ins, owner)
    for r in range(n):
        got = recv[r].cpu().numpy().view(sc.UINT[dt])
        assert np.array_equal(got, exp), (seed, r, int((got != exp).sum()))
        if not in_place:
            assert np.array_equal(send[r].cpu().numpy().view(sc.UINT[dt]), ins[r])


@pytest.mark.parametrize("mode", ["simple", "ll_group", "simple_group"])
@pytest.mark.parametrize("n", [2, 4, 8])
def test_ring_symmetric_interleaved_with_ring_and_tree_calls(nexr, ring, oracle, n, mode):
    """all_reduce_symmetric between ring and tree all-reduces of one device communicator: host-sequenced SIMPLE,
    LL in group launches, SIMPLE in group launches. Every ring and tree call stays exact against oracle.ring
    (fp32 NaNs by class, the suite's rule for them), every symmetric call against sym_cases, and queued() is
    left as it was."""
    dt, count = mg.F32, 50_021
    proto = ring.PROTO_LL if mode == "ll_group" else ring.PROTO_SIMPLE
    pname = "ll" if mode == "ll_group" else "simple"
    links = tree_topology(n, 0, 0)
    sym_count = 2 * n * 8192 // 4 + 3 * n * 2048 // 4 + 37
    with ring.RingComm(n, ring.DEVICE_MEMORY, BUFF[mode], None, 20000, proto) as comm:
        if mode == "ll_group":
            comm.set_ll_group(True)
        if mode == "simple_group":
            comm.set_simple_group(True)
        for call, what in enumerate(("sym", "ring", "sym", "tree", "sym_in_place", "ring", "sym16")):
            seed = 0x7100 + 16 * n + call
            if what.startswith("sym"):
                sdt = sc.BF16 if what == "sym16" else sc.F32
                _sym(comm, n, sdt, sym_count * (2 if what == "sym16" else 1), 1 + call % 3, [seed], what == "sym_in_place")
                continue
            inputs = mg.gen_inputs(dt, n, count, seed, special=True)
            send = _dev(inputs)
            recv = [torch.zeros_like(s) for s in send]
            torch.cuda.synchronize()
            if what == "ring":
                comm.all_reduce(_ptrs(send), _ptrs(recv), count, dt, 0)
                exp = (ring_allreduce_expected_ll(inputs, dt, 0, BUFF[mode]) if mode == "ll_group"
                       else ring_allreduce_expected(inputs, dt, 0, buff_bytes=BUFF[mode]))
                if mode != "simple" and torch.cuda.device_count() == 1:
                    assert comm.queued() == 3
            else:
                comm.tree_all_reduce(_ptrs(send), _ptrs(recv), count, dt, 0)
                exp = tree_allreduce_expected(inputs, dt, 0, links, pname)
            _same(dt, recv, exp, (mode, n, call, what))


def test_ring_symmetric_one_rank_and_zero_count(nexr, ring):
    x = torch.arange(1000, dtype=torch.float32, device="cuda")
    y = torch.zeros_like(x)
    with ring.RingComm(1, ring.DEVICE_MEMORY, 1 << 18, None, 20000) as comm:
        comm.all_reduce_symmetric([x.data_ptr()], [y.data_ptr()], 1000, sc.F32, 0)
        torch.cuda.synchronize()
        assert torch.equal(x, y)
    with ring.RingComm(2, ring.DEVICE_MEMORY, 1 << 18, None, 20000) as comm:
        comm.all_reduce_symmetric([x.data_ptr(), y.data_ptr()], [x.data_ptr(), y.data_ptr()], 0, sc.F32, 0)
        with pytest.raises(nexr.NexrError) as e:
            comm.all_reduce_symmetric([x.data_ptr(), y.data_ptr()], [x.data_ptr(), y.data_ptr()], 8, sc.F32, 1)
        assert e.value.code == nexr.Result.InvalidArgument


def test_ring_symmetric_is_invalid_usage_on_a_host_memory_communicator(nexr, ring):
    """The library's own host-memory communicator (its steps run on the GPU, its buffers are host memory)."""
    bufs = [np.ones(64, dtype=np.float32) for _ in range(4)]
    p = [b.ctypes.data for b in bufs]
    with ring.RingComm(2, ring.HOST_MEMORY, 1 << 18, None, 20000) as comm:
        for count in (0, 64):
            with pytest.raises(nexr.NexrError) as e:
                comm.all_reduce_symmetric(p[:2], p[2:], count, sc.F32, 0)
            assert e.value.code == nexr.Result.InvalidUsage
        comm.all_reduce(p[:2], p[2:], 64, sc.F32, 0)
        assert (bufs[2] == 2.0).all() and (bufs[3] == 2.0).all()
