"""nexrFlatAllToAllv and nexrRingAllToAllv on the MI355X, byte for byte against the packed rule
out[d][recvOff(d,s) + i] = in[s][sendOff(s,d) + i] in numpy on uint8 views, under host counts and under counts the
kernel reads from device memory. Seeded bytes; every output sits in an arena of BLANK bytes (64 guard bytes, the
capacity, 64 guard bytes) of which everything but the row total must survive."""
import importlib

import numpy as np
import pytest

import arith_edges as ae
import ring_modes_cases as rm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, BLANK = 64, 0xC3
HOST, DEVICE = 1, 0  # nexrScalarResidence_t
BOTH = pytest.mark.parametrize("residence", [HOST, DEVICE], ids=["host-counts", "device-counts"])


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


def random_counts(n, hi, seed=0):
    return np.random.default_rng(rm.SEED + 1000 * n + hi + seed).integers(0, hi + 1, (n, n)).astype(np.uint64)


class Exchange:
    """Seeded inputs and BLANK output arenas on the device, capacities `slack` elements above the sums of `counts`."""

    def __init__(self, counts, esz, slack=3, in_phase=0, out_phase=0):
        self.n, self.esz, self.in_phase, self.at = len(counts), esz, in_phase, GUARD + out_phase
        self.in_elts = [int(r) + slack for r in np.asarray(counts).sum(axis=1)]
        self.out_elts = [int(c) + slack for c in np.asarray(counts).sum(axis=0)]
        gen = torch.Generator().manual_seed(rm.SEED + int(np.asarray(counts).sum() % 9973))
        self.ins = [torch.randint(0, 256, (in_phase + e * esz,), dtype=torch.uint8, generator=gen).cuda()
                    for e in self.in_elts]
        self.arenas = [torch.full((self.at + e * esz + GUARD,), BLANK, dtype=torch.uint8).cuda() for e in self.out_elts]
        self.dev_counts = torch.zeros(self.n * self.n, dtype=torch.int64).cuda()
        self.status = torch.full((1,), 7, dtype=torch.int32).cuda()

    def pointers(self):
        return [t.data_ptr() + self.in_phase for t in self.ins], [a.data_ptr() + self.at for a in self.arenas]

    def counts_arg(self, counts, residence):
        flat = np.asarray(counts, np.uint64).reshape(-1)
        if residence == HOST:
            return [int(c) for c in flat]
        self.dev_counts.copy_(torch.from_numpy(flat.view(np.int64)).pin_memory(), non_blocking=True)
        return self.dev_counts.data_ptr()

    def call(self, nexr, counts, residence, max_workgroups=0, out_elts=None):
        ins, outs = self.pointers()
        nexr.flat_all_to_all_v(ins, outs, self.counts_arg(counts, residence), self.esz, self.in_elts,
                               out_elts or self.out_elts, self.status.data_ptr(), max_workgroups)

    def check(self, counts, arenas=None, status=0):
        counts = np.asarray(counts, np.uint64).astype(np.int64) * self.esz
        send_off = np.concatenate([np.zeros((self.n, 1), np.int64), np.cumsum(counts, axis=1)], axis=1)
        src = [t.cpu().numpy()[self.in_phase:] for t in self.ins]
        for d, arena in enumerate(arenas or self.arenas):
            want = np.full(arena.numel(), BLANK, np.uint8)
            row = [src[s][send_off[s, d]:send_off[s, d] + counts[s, d]] for s in range(self.n)]
            want[self.at:self.at + int(counts[:, d].sum())] = np.concatenate(row)
            np.testing.assert_array_equal(arena.cpu().numpy(), want, err_msg="arena of output %d" % d)
        if status is not None:
            assert int(self.status.item()) == status


def run(nexr, counts, esz, residence, max_workgroups=0, **layout):
    x = Exchange(counts, esz, **layout)
    x.call(nexr, counts, residence, max_workgroups)
    torch.cuda.synchronize()
    x.check(counts, status=0 if residence == DEVICE or np.asarray(counts).any() else None)  # no launch, no report


@BOTH
@pytest.mark.parametrize("n", [2, 3, 8, 64])
@pytest.mark.parametrize("esz, hi", [(1, 40), (2, 40), (4, 700), (8, 700)])
def test_seeded_random_counts(nexr, n, esz, hi, residence):
    """Straddling packs and blocks under 16 bytes at 1 and 2 bytes; 64 ranks pass the inline limit of host counts."""
    run(nexr, random_counts(n, hi), esz, residence)


SHAPES = {  # esz, counts, and what differs from Exchange's layout or the default grid
    "zero rows and zero columns": (4, [[3, 0, 9, 1], [0, 0, 0, 0], [7, 0, 2, 30], [5, 0, 0, 4]], {}),
    "runs of consecutive empty blocks": (1, [[0, 0, 0, 5, 0], [0, 0, 0, 0, 0], [21, 0, 0, 0, 0], [0, 0, 0, 0, 0],
                                             [0, 0, 0, 0, 17]], {}),
    "a whole empty output": (2, [[0, 19, 4], [0, 1, 33], [0, 8, 8]], {}),
    "all-zero counts": (4, [[0, 0, 0], [0, 0, 0], [0, 0, 0]], {}),
    "one long block beside empty ones": (1, [[0, 0, 0], [0, 5120 + 16, 0], [0, 0, 0]], {}),
    "row totals exactly at capacity": (1, [[17, 2048 - 17, 1], [2031, 16, 0], [0, 1, 15]], dict(slack=0)),
    "a row total of one byte": (1, [[0, 0], [1, 0]], {}),
    "bases off alignment, 1 byte": (1, random_counts(3, 40, seed=1), dict(in_phase=1, out_phase=3)),
    "bases off alignment, 8 bytes": (8, random_counts(3, 700, seed=1), dict(in_phase=1, out_phase=3)),
    "one workgroup strides": (4, random_counts(4, 200, seed=2) + np.uint64(200), dict(max_workgroups=1)),
}


@BOTH
@pytest.mark.parametrize("case", list(SHAPES))
def test_hand_made_shapes(nexr, case, residence):
    esz, counts, how = SHAPES[case]
    run(nexr, np.array(counts, np.uint64), esz, residence, **how)


def test_device_counts_rewritten_between_two_calls(nexr):
    """The same pointers twice, the matrix rewritten on the stream in between, no host synchronisation in between."""
    first, second = random_counts(5, 300, seed=3), random_counts(5, 300, seed=4)
    x = Exchange(np.maximum(first, second), 2)
    x.call(nexr, first, DEVICE)
    kept = [a.clone() for a in x.arenas]  # stream-ordered copies, then the arenas blank again
    for a in x.arenas:
        a.fill_(BLANK)
    x.call(nexr, second, DEVICE)
    torch.cuda.synchronize()
    x.check(first, kept, status=None)
    x.check(second)


@pytest.mark.parametrize("what", ["a column sum one element above outElts", "a single count of 2**63"])
def test_violations_with_device_counts_write_nothing(nexr, what):
    counts = random_counts(3, 300, seed=5) + np.uint64(1)
    x = Exchange(counts, 4, slack=0)
    if what.startswith("a column"):
        x.call(nexr, counts, DEVICE, out_elts=[x.out_elts[0], x.out_elts[1] - 1, x.out_elts[2]])
    else:
        wrong = counts.copy()
        wrong[0, 1] = 2 ** 63
        x.call(nexr, wrong, DEVICE)
    torch.cuda.synchronize()
    x.check(np.zeros((3, 3), np.uint64), status=1)  # every arena wholly BLANK
    x.call(nexr, counts, DEVICE)
    torch.cuda.synchronize()
    x.check(counts, status=0)


@BOTH
def test_process_ranks_are_refused(ring, nexr, residence):
    """InvalidUsage ahead of every other check, alone and behind a group start (which such a communicator refuses)."""
    import ctypes
    import os
    L, buf, counts = ring.ring_lib(), np.zeros(64, np.float32), np.array([4], np.uint64)
    arr, cap = (ctypes.c_void_p * 1)(buf.ctypes.data), (ctypes.c_size_t * 1)(8)
    status = np.full(1, 7, np.uint32)
    with ring.PeerRingComm(1, 0, "/nexr_alltoallv_%d_%d" % (residence, os.getpid()), device=0,
                           buff_bytes=rm.BUFF["simple"], timeout_ms=20000) as comm:
        for start in (False, True):
            if start:
                assert L.nexrRingGroupStart(comm._h) == nexr.Result.InvalidUsage
            assert L.nexrRingAllToAllv(comm._h, arr, arr, counts.ctypes.data, residence, ae.F32, cap, cap,
                                       status.ctypes.data) == nexr.Result.InvalidUsage
    assert not buf.any() and status[0] == 7


@BOTH
@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("dt, esz", [(ae.F16, 2), (ae.I64, 8)], ids=["fp16", "int64"])
def test_ring_all_to_all_v_on_device_memory(ring, nexr, n, dt, esz, residence):
    """Alone and inside a group: queued() as it was, `singles` counted, a ring all-reduce before and after exact."""
    counts = random_counts(n, 60, seed=dt)
    x = Exchange(counts, esz)
    a = [torch.full((32,), r + 1, dtype=torch.int32).cuda() for r in range(n)]
    b = [torch.zeros(32, dtype=torch.int32).cuda() for _ in range(n)]
    with ring.RingComm(n, ring.DEVICE_MEMORY, rm.BUFF["simple"], None, 20000, rm.PROTO_ID["simple"],
                       tree_ranks_per_node=rm.tree_per_node(n), n_channels=1) as comm:
        def all_reduce():
            for t in b:
                t.zero_()
            torch.cuda.synchronize()
            comm.all_reduce([t.data_ptr() for t in a], [t.data_ptr() for t in b], 32, ae.I32, rm.SUM)
            torch.cuda.synchronize()
            assert all((t.cpu().numpy() == sum(range(1, n + 1))).all() for t in b)

        def exchange():
            arg = x.counts_arg(counts, residence)
            torch.cuda.synchronize()  # the communicator's stream is not torch's
            comm.all_to_all_v(*x.pointers(), arg, dt, x.in_elts, x.out_elts, x.status.data_ptr())

        all_reduce()
        queued = comm.queued()
        exchange()
        assert comm.queued() == queued
        x.check(counts)
        for t in x.arenas:
            t.fill_(BLANK)
        comm.group_stats(reset=True)
        with comm.group():
            exchange()
        assert comm.group_stats()["singles"] == 1 and comm.queued() == queued
        x.check(counts)
        all_reduce()
