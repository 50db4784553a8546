"""nexrFlatAllToAll2D / nexrFlatAllGather2D and their ring entries on the MI355X, byte for byte against the rule of
tests/test_pitched.py (numpy on uint8 views). Every byte is seeded and every output sits between 64 guard bytes that
must survive. The shapes are the smallest at which the index derivation can go wrong."""
import importlib

import numpy as np
import pytest

import arith_edges as ae
import ring_modes_cases as rm
from test_pitched import MODES, rule

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GUARD, BLANK = 64, 0xC3
modes = pytest.mark.parametrize("mode", list(MODES))


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


def run(nexr, mode, n, R, B, in_phase=0, out_phase=0, max_workgroups=0, call=None):
    """Seeded inputs, blank output arenas (guard, n * R * B bytes, guard), the call, outputs and guards checked."""
    gather = MODES[mode] is None
    gen = torch.Generator().manual_seed(rm.SEED + n * 8192 + R * 131 + B)
    size = (1 if gather else n) * R * B
    ins = [torch.randint(0, 256, (in_phase + size,), dtype=torch.uint8, generator=gen).cuda() for _ in range(n)]
    arenas = [torch.full((GUARD + out_phase + n * R * B + GUARD,), BLANK, dtype=torch.uint8).cuda() for _ in range(n)]
    xs, ys = [t.data_ptr() + in_phase for t in ins], [a.data_ptr() + GUARD + out_phase for a in arenas]
    if call:
        call(xs, ys)
    elif gather:
        nexr.flat_all_gather_2d(xs, ys, R, B, max_workgroups)
    else:
        nexr.flat_all_to_all_2d(xs, ys, R, B, *MODES[mode], max_workgroups)
    torch.cuda.synchronize()
    want = rule([t.cpu().numpy()[in_phase:] for t in ins], n, R, MODES[mode])
    at = GUARD + out_phase
    for d, arena in enumerate(arenas):
        got = arena.cpu().numpy()
        np.testing.assert_array_equal(got[at:at + want[d].size], want[d], err_msg="output %d" % d)
        assert (got[:at] == BLANK).all() and (got[at + want[d].size:] == BLANK).all(), "guards of output %d" % d


SHAPES = ([(n, R, B) for R, B in [(3, 16), (5, 48), (2, 256)] for n in (2, 3, 8)] + [(64, 3, 16)] +  # W = 16, narrow
          [(n, R, B) for R, B in [(2, 2048), (3, 2080), (2, 5120)] for n in (2, 3)] +               # W = 16, wide
          [(3, R, B) for R, B in [(7, 4), (3, 20), (2, 516)]] +                                     # W = 4
          [(n, R, B) for R, B in [(3, 1), (2, 17), (2, 129)] for n in (2, 5)])                      # W = 1


@modes
@pytest.mark.parametrize("n, R, B", SHAPES)
def test_every_width_and_path(nexr, mode, n, R, B):
    run(nexr, mode, n, R, B)


@modes
@pytest.mark.parametrize("R, B", [(5, 48), (3, 2080), (3, 20), (2, 17)], ids=["w16-narrow", "w16-wide", "w4", "w1"])
def test_misaligned_bases(nexr, mode, R, B):
    run(nexr, mode, 3, R, B, in_phase=1, out_phase=3)


@modes
def test_one_workgroup_strides_over_the_items(nexr, mode):
    run(nexr, mode, 8, 3, 2080, max_workgroups=1)


@modes
def test_an_output_may_begin_where_an_input_ends(nexr, mode):
    """Output 0 directly behind input 0 in one allocation is accepted and exact; one byte earlier is refused."""
    n, R, B = 2, 3, 48
    gather = MODES[mode] is None
    size, out = (1 if gather else n) * R * B, n * R * B
    gen = torch.Generator().manual_seed(rm.SEED)
    both = torch.randint(0, 256, (size + out,), dtype=torch.uint8, generator=gen).cuda()
    other = torch.randint(0, 256, (size,), dtype=torch.uint8, generator=gen).cuda()
    out1 = torch.zeros(out, dtype=torch.uint8).cuda()
    want = rule([both.cpu().numpy()[:size], other.cpu().numpy()], n, R, MODES[mode])

    def call(first_out):
        xs, ys = [both.data_ptr(), other.data_ptr()], [first_out, out1.data_ptr()]
        if gather:
            nexr.flat_all_gather_2d(xs, ys, R, B)
        else:
            nexr.flat_all_to_all_2d(xs, ys, R, B, *MODES[mode])

    with pytest.raises(nexr.NexrError) as e:
        call(both.data_ptr() + size - 1)
    assert e.value.code == nexr.Result.InvalidArgument
    call(both.data_ptr() + size)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(both.cpu().numpy()[size:], want[0])
    np.testing.assert_array_equal(out1.cpu().numpy(), want[1])


@modes
@pytest.mark.parametrize("n", [2, 8])
@pytest.mark.parametrize("dt, esz, count", [(ae.F16, 2, 24), (ae.I64, 8, 5)], ids=["fp16x24", "int64x5"])
def test_ring_entries_on_device_memory(ring, nexr, mode, n, dt, esz, count):
    """The rule's bytes, queued() as it was, and a ring all-reduce before and after it with its own bytes."""
    R = 3
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

        def call(xs, ys):
            queued = comm.queued()
            if MODES[mode] is None:
                comm.all_gather_2d(xs, ys, R, count, dt)
            else:
                comm.all_to_all_2d(xs, ys, R, count, dt, *MODES[mode])
            assert comm.queued() == queued

        all_reduce()
        run(nexr, mode, n, R, count * esz, call=call)
        all_reduce()
