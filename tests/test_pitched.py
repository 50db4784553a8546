"""nexrFlatAllToAll2D / nexrFlatAllGather2D and nexrRingAllToAll2D / nexrRingAllGather2D without a GPU: every refusal
answers before a device call (made-up addresses), and a host-memory communicator with the oracle's step functions
gives the rule, alone and inside a group. The reference is numpy on uint8 views: reshape and transpose."""
import ctypes
import importlib

import numpy as np
import pytest

import ring_modes_cases as rm

F32, I8 = 7, 0  # nexrFloat32, nexrInt8
BLOCKS, ROWS = 0, 1
MODES = {"rows-blocks": (ROWS, BLOCKS), "blocks-rows": (BLOCKS, ROWS), "rows-rows": (ROWS, ROWS),
         "gather": None}  # (inLayout, outLayout) of the exchange; None: the gather


def rule(ins, n, R, mode):
    """The outputs as uint8 arrays. x[s][k][r] is block row (k, r) of input s, y[d][s][r] = x[s][d][r]."""
    if mode is None:
        x = [np.asarray(a).view(np.uint8).reshape(R, -1) for a in ins]
        return [np.stack(x, axis=1).reshape(-1) for _ in range(n)]  # [R][n][B]
    lay_in, lay_out = mode
    x = [np.asarray(a).view(np.uint8).reshape((n, R, -1) if lay_in == BLOCKS else (R, n, -1)) for a in ins]
    x = [a if lay_in == BLOCKS else a.transpose(1, 0, 2) for a in x]
    y = [np.stack([x[s][d] for s in range(n)]) for d in range(n)]
    return [(a if lay_out == BLOCKS else a.transpose(1, 0, 2)).reshape(-1) for a in y]


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


@pytest.fixture(scope="module")
def comm3(ring, oracle):
    L = oracle.lib()
    f, fll, fll128 = (ctypes.cast(g, ctypes.c_void_p).value
                      for g in (L.oracle_reduce_copy_fn, L.oracle_reduce_copy_ll_fn, L.oracle_reduce_copy_ll128_fn))
    comms = {n: ring.RingComm(n, ring.HOST_MEMORY, rm.BUFF["simple"], f, 20000, rm.PROTO_ID["simple"], fll, fll128,
                              rm.tree_per_node(n), 0, 1) for n in (2, 3)}
    yield comms
    for c in comms.values():
        c.close()


def _flat(nexr, gather, ins, outs, rows=3, n_bytes=0x100, lay=(ROWS, BLOCKS), n=None, max_wgs=0):
    arr = lambda ps: (ctypes.c_void_p * len(ps))(*[p or None for p in ps]) if ps else None  # noqa: E731
    n = len(ins) if n is None else n
    if gather:
        return nexr.lib().nexrFlatAllGather2D(n, arr(ins), arr(outs), rows, n_bytes, max_wgs, None)
    return nexr.lib().nexrFlatAllToAll2D(n, arr(ins), arr(outs), rows, n_bytes, lay[0], lay[1], max_wgs, None)


A, Z = 0x10000000, 0x20000000  # where the made-up inputs and outputs begin; a buffer is 2 * 3 * 0x100 = 0x600 bytes
FLAT_REFUSALS = {
    "one rank": dict(ins=[A], outs=[Z]),
    "65 ranks": dict(ins=[A + r * 0x100000 for r in range(65)], outs=[Z + r * 0x100000 for r in range(65)]),
    "null inputs": dict(ins=None, outs=[Z, Z + 0x1000], n=2),
    "null outputs": dict(ins=[A, A + 0x1000], outs=None, n=2),
    "a null input": dict(ins=[A, 0], outs=[Z, Z + 0x1000]),
    "a null output": dict(ins=[A, A + 0x1000], outs=[Z, 0]),
    "layout 2 in": dict(ins=[A, A + 0x1000], outs=[Z, Z + 0x1000], lay=(2, BLOCKS)),
    "layout -1 out": dict(ins=[A, A + 0x1000], outs=[Z, Z + 0x1000], lay=(ROWS, -1)),
    "maxWorkgroups < 0": dict(ins=[A, A + 0x1000], outs=[Z, Z + 0x1000], max_wgs=-1),
    "2^31 rows": dict(ins=[A, A + 0x1000], outs=[Z, Z + 0x1000], rows=2 ** 31, n_bytes=1),
    "n * R * B beyond size_t": dict(ins=[A, A + 0x1000], outs=[Z, Z + 0x1000], n_bytes=2 ** 62),
    "an input is an output": dict(ins=[A, Z + 0x1000], outs=[Z, Z + 0x1000]),
    "one byte of an output in an input": dict(ins=[A, A + 0x1000], outs=[Z, A - 0x600 + 1]),
    "two outputs meet": dict(ins=[A, A + 0x1000], outs=[Z, Z + 0x600 - 1]),
}


@pytest.mark.parametrize("why, gather", [(w, g) for w in FLAT_REFUSALS for g in (False, True)
                                         if not (g and "layout" in w)])  # the gather has no layout argument
def test_flat_refusals_answer_before_any_device_call(nexr, why, gather):
    assert _flat(nexr, gather, **FLAT_REFUSALS[why]) == int(nexr.Result.InvalidArgument), why


def test_flat_input_ranges_are_a_whole_buffer_or_the_gathers_rows(nexr):
    # the last byte of input 1 in output 0: the exchange's input is n * R * B = 0x600 bytes, the gather's R * B
    bad, ok = int(nexr.Result.InvalidArgument), int(nexr.Result.Success)
    assert (nexr.LAYOUT_BLOCKS, nexr.LAYOUT_ROWS) == (BLOCKS, ROWS)
    assert _flat(nexr, False, [A, Z - 0x600 + 1], [Z, Z + 0x1000]) == bad
    assert _flat(nexr, True, [A, Z - 0x300 + 1], [Z, Z + 0x1000]) == bad
    # no rows or no bytes meet nothing, even at equal addresses: success without a launch
    for gather in (False, True):
        assert _flat(nexr, gather, [A, A], [A, A], rows=0) == ok
        assert _flat(nexr, gather, [A, A], [A, A], n_bytes=0) == ok


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("R, count, dt, np_dt", [(3, 5, F32, np.float32), (2, 33, I8, np.int8)])
def test_ring_entries_on_host_memory(ring, nexr, comm3, n, mode, R, count, dt, np_dt):
    """Alone, then inside a group: nothing is written before the End, and the call counts as one of `singles`."""
    comm, gather = comm3[n], MODES[mode] is None
    rng = np.random.default_rng(rm.SEED + n * 100 + count)
    size = (1 if gather else n) * R * count * np.dtype(np_dt).itemsize
    ins = [rng.integers(0, 256, size, dtype=np.uint8).view(np_dt) for _ in range(n)]
    want = rule(ins, n, R, MODES[mode])

    def call(outs):
        xs, ys = [a.ctypes.data for a in ins], [a.ctypes.data for a in outs]
        if gather:
            comm.all_gather_2d(xs, ys, R, count, dt)
        else:
            comm.all_to_all_2d(xs, ys, R, count, dt, *MODES[mode])

    for grouped in (False, True):
        outs = [np.zeros(n * R * count, np_dt) for _ in range(n)]
        comm.group_stats(reset=True)
        if grouped:
            with comm.group():
                call(outs)
                assert not any(o.view(np.uint8).any() for o in outs)
        else:
            call(outs)
        for d in range(n):
            np.testing.assert_array_equal(outs[d].view(np.uint8), want[d])
        assert comm.group_stats()["singles"] == int(grouped)


def test_blocks_to_blocks_is_the_all_to_all_of_whole_blocks(comm3):
    n, R, count = 3, 4, 7
    rng = np.random.default_rng(rm.SEED)
    ins = [rng.integers(0, 256, n * R * count * 4, dtype=np.uint8).view(np.float32) for _ in range(n)]
    a, b = ([np.zeros(n * R * count, np.float32) for _ in range(n)] for _ in range(2))
    xs = [t.ctypes.data for t in ins]
    comm3[n].all_to_all_2d(xs, [t.ctypes.data for t in a], R, count, F32, BLOCKS, BLOCKS)
    comm3[n].all_to_all(xs, [t.ctypes.data for t in b], R * count, F32)
    for d in range(n):
        assert b[d].view(np.uint8).any()
        np.testing.assert_array_equal(a[d].view(np.uint8), b[d].view(np.uint8))


def test_ring_refusals(ring, nexr, comm3):
    bad, n, R, count = nexr.Result.InvalidArgument, 3, 2, 4
    comm, L = comm3[n], ring.ring_lib()
    x = [np.arange(n * R * count, dtype=np.float32) + r for r in range(n)]
    y = [np.zeros(n * R * count, np.float32) for _ in range(n)]
    xs, ys = [a.ctypes.data for a in x], [a.ctypes.data for a in y]
    size = n * R * count * 4
    for h in (None, comm._h):  # no communicator, null arrays
        assert L.nexrRingAllToAll2D(h, None, None, 1, 1, F32, ROWS, BLOCKS) == bad
        assert L.nexrRingAllGather2D(h, None, None, 1, 1, F32) == bad
    cases = {"a null buffer": lambda: comm.all_to_all_2d([xs[0], 0, xs[2]], ys, R, count, F32, ROWS, BLOCKS),
             "fp8": lambda: comm.all_to_all_2d(xs, ys, R, count, 10, ROWS, BLOCKS),
             "no such datatype": lambda: comm.all_gather_2d(xs, ys, R, count, 99),
             "layout 2": lambda: comm.all_to_all_2d(xs, ys, R, count, F32, ROWS, 2),
             "2^31 rows": lambda: comm.all_to_all_2d(xs, ys, 2 ** 31, 1, I8, ROWS, BLOCKS),
             "beyond size_t": lambda: comm.all_gather_2d(xs, ys, R, 2 ** 61, F32),
             "in place": lambda: comm.all_to_all_2d(xs, xs, R, count, F32, BLOCKS, ROWS),
             "in place, gather": lambda: comm.all_gather_2d(xs, xs, R, count, F32),
             "one byte shared": lambda: comm.all_to_all_2d(xs, [ys[0], ys[1], xs[0] + size - 1], R, count, F32,
                                                           ROWS, ROWS),
             "two outputs meet": lambda: comm.all_gather_2d(xs, [ys[0], ys[1], ys[0] + size - 1], R, count, F32)}
    for why, call in cases.items():
        with pytest.raises(nexr.NexrError) as e:
            call()
        assert e.value.code == bad, why
    comm.group_stats(reset=True)
    with comm.group():  # refused at once, not recorded
        with pytest.raises(nexr.NexrError) as e:
            comm.all_to_all_2d(xs, xs, R, count, F32, ROWS, BLOCKS)
        assert e.value.code == bad and comm.group_stats(reset=True)["calls"] == 0
    comm.all_to_all_2d([0] * n, [0] * n, 0, count, F32, ROWS, BLOCKS)  # no rows: success, buffers unread
    comm.all_gather_2d([0] * n, [0] * n, R, 0, F32)
    assert not any(a.any() for a in y)
