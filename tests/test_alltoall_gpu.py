"""nexrFlatAllToAll and nexrRingAllToAll on the MI355X, byte for byte against the index rule
out[d][s*B + i] = in[s][d*B + i] in numpy on uint8 views. Every byte comes from a seeded generator, every output sits
in a larger arena between 64 guard bytes that must survive, and the shapes are the smallest at which the kernel can
go wrong: a row shorter than a piece, block boundaries inside a piece and between a lane's two packs, a boundary off
the piece grid with a partial last piece, all 64 pointers, both sides of the 2048-byte switch of the pack path, the
byte path around one pack and one piece, bases off every alignment, and a grid that strides."""
import importlib

import numpy as np
import pytest

import arith_edges as ae
import ring_modes_cases as rm

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, BLANK = 64, 0xC3


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


def buffers(n, row, in_phase=0, out_phase=0, seed=0):
    """n inputs of `row` seeded bytes and n output arenas (guard, row, guard) filled with BLANK, on the device."""
    gen = torch.Generator().manual_seed(rm.SEED + seed)
    ins = [torch.randint(0, 256, (row + in_phase,), dtype=torch.uint8, generator=gen).cuda() for _ in range(n)]
    arenas = [torch.full((GUARD + out_phase + row + GUARD,), BLANK, dtype=torch.uint8).cuda() for _ in range(n)]
    return ins, arenas


def check(ins, arenas, n, in_phase=0, out_phase=0):
    blocks = [t.cpu().numpy()[in_phase:].reshape(n, -1) for t in ins]
    for d, arena in enumerate(arenas):
        got = arena.cpu().numpy()
        want = np.concatenate([blocks[s][d] for s in range(n)])
        at = GUARD + out_phase
        np.testing.assert_array_equal(got[at:at + want.size], want, err_msg="output %d" % d)
        assert (got[:at] == BLANK).all() and (got[at + want.size:] == BLANK).all(), "guards of output %d" % d


def run_flat(nexr, n, B, in_phase=0, out_phase=0, max_workgroups=0):
    ins, arenas = buffers(n, n * B, in_phase, out_phase, seed=n * 8192 + B)
    nexr.flat_all_to_all([t.data_ptr() + in_phase for t in ins], [a.data_ptr() + GUARD + out_phase for a in arenas], B,
                         max_workgroups)
    torch.cuda.synchronize()
    check(ins, arenas, n, in_phase, out_phase)


@pytest.mark.parametrize("n", [2, 3, 8, 64])
@pytest.mark.parametrize("B", [16, 48, 2080, 5120])
def test_pack_path(nexr, n, B):
    run_flat(nexr, n, B)


@pytest.mark.parametrize("n", [2, 5])
@pytest.mark.parametrize("B", [1, 15, 17, 2049])
def test_byte_path(nexr, n, B):
    run_flat(nexr, n, B)


@pytest.mark.parametrize("n, B", [(3, 2080), (3, 48), (5, 2049)], ids=["packs-wide", "packs-narrow", "bytes"])
def test_misaligned_bases(nexr, n, B):
    run_flat(nexr, n, B, in_phase=1, out_phase=3)


def test_one_workgroup_strides_over_the_items(nexr):
    run_flat(nexr, 8, 5120, max_workgroups=1)


def test_an_output_may_begin_where_an_input_ends(nexr):
    """Half-open ranges: output 0 directly behind input 0 in one allocation is accepted and exact; one byte earlier
    is refused before any device call."""
    n, B = 2, 48
    row = n * B
    gen = torch.Generator().manual_seed(rm.SEED)
    both = torch.randint(0, 256, (2 * row,), dtype=torch.uint8, generator=gen).cuda()
    other = torch.randint(0, 256, (row,), dtype=torch.uint8, generator=gen).cuda()
    out1 = torch.zeros(row, dtype=torch.uint8).cuda()
    want = np.concatenate([both.cpu().numpy()[:B], other.cpu().numpy()[:B]])
    with pytest.raises(nexr.NexrError) as e:
        nexr.flat_all_to_all([both.data_ptr(), other.data_ptr()], [both.data_ptr() + row - 1, out1.data_ptr()], B)
    assert e.value.code == nexr.Result.InvalidArgument
    nexr.flat_all_to_all([both.data_ptr(), other.data_ptr()], [both.data_ptr() + row, out1.data_ptr()], B)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(both.cpu().numpy()[row:], want)


def test_process_ranks_are_refused(ring, nexr):
    import ctypes
    import os
    buf = np.zeros(64, np.float32)
    arr = (ctypes.c_void_p * 1)(buf.ctypes.data)
    with ring.PeerRingComm(1, 0, "/nexr_alltoall_%d" % os.getpid(), device=0, buff_bytes=rm.BUFF["simple"],
                           timeout_ms=20000) as comm:
        assert ring.ring_lib().nexrRingAllToAll(comm._h, arr, arr, 4, ae.F32) == nexr.Result.InvalidUsage
    assert not buf.any()


@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("dt, esz, count", [(ae.F16, 2, 24), (ae.I64, 8, 5)], ids=["fp16x24", "int64x5"])
def test_ring_all_to_all_on_device_memory(ring, nexr, n, dt, esz, count):
    """One launch through the communicator: the rule's bytes, queued() as it was, and a ring all-reduce before and
    after it with its own bytes: no protocol state is touched."""
    ins, arenas = buffers(n, n * count * esz, seed=n + dt)
    x = [torch.full((32,), r + 1, dtype=torch.int32).cuda() for r in range(n)]
    y = [torch.zeros(32, dtype=torch.int32).cuda() for _ in range(n)]
    total = sum(range(1, n + 1))
    with ring.RingComm(n, ring.DEVICE_MEMORY, rm.BUFF["simple"], None, 20000, rm.PROTO_ID["simple"],
                       tree_ranks_per_node=rm.tree_per_node(n), n_channels=1) as comm:
        def all_reduce():
            for t in y:
                t.zero_()
            torch.cuda.synchronize()
            comm.all_reduce([t.data_ptr() for t in x], [t.data_ptr() for t in y], 32, ae.I32, rm.SUM)
            torch.cuda.synchronize()
            assert all((t.cpu().numpy() == total).all() for t in y)

        all_reduce()
        queued = comm.queued()
        comm.all_to_all([t.data_ptr() for t in ins], [a.data_ptr() + GUARD for a in arenas], count, dt)
        torch.cuda.synchronize()
        assert comm.queued() == queued
        check(ins, arenas, n)
        all_reduce()
