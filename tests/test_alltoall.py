"""The all-to-all without a GPU: nexrFlatAllToAll (include/nexr.h) and nexrRingAllToAll (include/nexr_ring.h). The
headers, the exports and the ctypes lists agree; every refusal answers before a device call (made-up addresses); a
host-memory communicator with the oracle's step functions gives the index rule
out[d][s*B + i] = in[s][d*B + i], alone and inside a group; and the shipped code object holds exactly the two
instances, without scratch."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import ring_modes_cases as rm
from conftest import ROOT

F32, I8 = 7, 0  # nexrFloat32, nexrInt8


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


@pytest.fixture(scope="module")
def fns(oracle):
    L = oracle.lib()
    cast = lambda f: ctypes.cast(f, ctypes.c_void_p).value  # noqa: E731
    return cast(L.oracle_reduce_copy_fn), cast(L.oracle_reduce_copy_ll_fn), cast(L.oracle_reduce_copy_ll128_fn)


def host_comm(ring, fns, protocol, n):
    f, fll, fll128 = fns
    return ring.RingComm(n, ring.HOST_MEMORY, rm.BUFF[protocol], f, 20000, rm.PROTO_ID[protocol], fll, fll128,
                         rm.tree_per_node(n), 0, 1)


def exchange(ins, n):
    """The rule on uint8 views: block d of input s becomes block s of output d."""
    blocks = [np.frombuffer(a.tobytes(), np.uint8).reshape(n, -1) for a in ins]
    return [np.concatenate([blocks[s][d] for s in range(n)]) for d in range(n)]


@pytest.mark.parametrize("header, name, lib_of", [("nexr.h", "nexrFlatAllToAll", "nexr"),
                                                  ("nexr_ring.h", "nexrRingAllToAll", "ring")])
def test_symbols_are_declared_exported_and_listed(nexr, ring, header, name, lib_of):
    text = open(os.path.join(ROOT, "include", header)).read()
    assert re.search(r"NEXR_API\s+nexrResult_t\s+%s\s*\(" % name, text)
    listed, path = ((nexr.ABI_SYMBOLS, nexr.LIB_PATH) if lib_of == "nexr" else (ring.RING_ABI_SYMBOLS, ring.RING_LIB_PATH))
    assert name in listed
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert name in {line.split()[-1] for line in out.splitlines() if " T " in line}


def _flat(nexr, ins, outs, n_bytes, n=None, max_wgs=0):
    arr = lambda ps: (ctypes.c_void_p * len(ps))(*[p or None for p in ps])  # noqa: E731
    return nexr.lib().nexrFlatAllToAll(len(ins) if n is None else n, arr(ins) if ins else None,
                                       arr(outs) if outs else None, n_bytes, max_wgs, None)


B, A, Z = 0x100, 0x10000000, 0x20000000  # bytes per pair, where the made-up inputs and outputs begin
FLAT_REFUSALS = {
    "one rank": dict(ins=[A], outs=[Z]),
    "65 ranks": dict(ins=[A + r * 0x100000 for r in range(65)], outs=[Z + r * 0x100000 for r in range(65)]),
    "null inputs": dict(ins=None, outs=[Z, Z + 0x1000], n=2),
    "null outputs": dict(ins=[A, A + 0x1000], outs=None, n=2),
    "a null input": dict(ins=[A, 0], outs=[Z, Z + 0x1000]),
    "a null output": dict(ins=[A, A + 0x1000], outs=[Z, 0]),
    "maxWorkgroups < 0": dict(ins=[A, A + 0x1000], outs=[Z, Z + 0x1000], max_wgs=-1),
    "n * B beyond size_t": dict(ins=[A, A + 0x1000], outs=[Z, Z + 0x1000], n_bytes=2 ** 63),
    "an input is an output": dict(ins=[A, Z + 0x1000], outs=[Z, Z + 0x1000]),
    "one byte of an input in an output": dict(ins=[A, Z + 2 * B - 1], outs=[Z, Z + 0x1000]),
    "one byte of an output in an input": dict(ins=[A, A + 0x1000], outs=[Z, A - 2 * B + 1]),
    "two outputs meet": dict(ins=[A, A + 0x1000], outs=[Z, Z + 2 * B - 1]),
}


@pytest.mark.parametrize("why", list(FLAT_REFUSALS))
def test_flat_refusals_answer_before_any_device_call(nexr, why):
    kw = dict(n_bytes=B)
    kw.update(FLAT_REFUSALS[why])
    assert _flat(nexr, **kw) == int(nexr.Result.InvalidArgument), why


def test_flat_empty_call_succeeds_without_a_launch(nexr):
    """No bytes meet nothing, even at equal addresses. (Touching ranges with bytes to copy are a launch: they are
    shown on real memory, in test_ring_refusals here and in tests/test_alltoall_gpu.py.)"""
    ok = int(nexr.Result.Success)
    assert _flat(nexr, [A, A + 0x1000], [Z, Z + 0x1000], 0) == ok
    assert _flat(nexr, [A, A], [A, A], 0) == ok


@pytest.mark.parametrize("protocol", list(rm.PROTO_ID))
@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("dt, np_dt", [(F32, np.float32), (I8, np.int8)])
@pytest.mark.parametrize("count", [1, 33])
def test_ring_all_to_all_on_host_memory(ring, nexr, oracle, fns, protocol, n, dt, np_dt, count):
    """Alone, then inside a group: nothing is written before the End, and the call counts as one of `singles`."""
    rng = np.random.default_rng(rm.SEED + n * 100 + count)
    ins = [rng.integers(0, 256, n * count * np.dtype(np_dt).itemsize, dtype=np.uint8).view(np_dt) for _ in range(n)]
    want = exchange(ins, n)
    with host_comm(ring, fns, protocol, n) as comm:
        outs = [np.zeros(n * count, np_dt) for _ in range(n)]
        comm.all_to_all([a.ctypes.data for a in ins], [a.ctypes.data for a in outs], count, dt)
        for d in range(n):
            np.testing.assert_array_equal(outs[d].view(np.uint8), want[d])
        outs = [np.zeros(n * count, np_dt) for _ in range(n)]
        comm.group_stats(reset=True)
        with comm.group():
            comm.all_to_all([a.ctypes.data for a in ins], [a.ctypes.data for a in outs], count, dt)
            assert not any(o.view(np.uint8).any() for o in outs)
        for d in range(n):
            np.testing.assert_array_equal(outs[d].view(np.uint8), want[d])
        assert comm.group_stats()["singles"] == 1


def test_ring_refusals(ring, nexr, oracle, fns):
    bad = nexr.Result.InvalidArgument
    n, count = 3, 4
    x = [np.arange(n * count, dtype=np.float32) + r for r in range(n)]
    y = [np.zeros(n * count, np.float32) for _ in range(n)]
    xs, ys = [a.ctypes.data for a in x], [a.ctypes.data for a in y]
    L = ring.ring_lib()
    assert L.nexrRingAllToAll(None, None, None, 1, F32) == bad
    with host_comm(ring, fns, "simple", n) as comm:
        assert L.nexrRingAllToAll(comm._h, None, None, 1, F32) == bad                # null arrays
        row = n * count * 4
        cases = {"a null buffer": lambda: comm.all_to_all([xs[0], 0, xs[2]], ys, count, F32),
                 "fp8": lambda: comm.all_to_all(xs, ys, count, 10),
                 "no such datatype": lambda: comm.all_to_all(xs, ys, count, 99),
                 "in place": lambda: comm.all_to_all(xs, xs, count, F32),
                 "one byte shared": lambda: comm.all_to_all(xs, [ys[0], ys[1], xs[0] + row - 1], count, F32)}
        for why, call in cases.items():
            with pytest.raises(nexr.NexrError) as e:
                call()
            assert e.value.code == bad, why
        with comm.group():                                                           # refused at once, not recorded
            with pytest.raises(nexr.NexrError) as e:
                comm.all_to_all(xs, xs, count, F32)
            assert e.value.code == bad and comm.group_stats(reset=True)["calls"] == 0
        comm.all_to_all([0] * n, [0] * n, 0, F32)                                     # count 0: success, buffers unread
        # a receive range that begins exactly where a send range ends is accepted
        both = np.zeros(2 * n * count, np.float32)
        both[:n * count] = x[0]
        comm.all_to_all([both.ctypes.data, xs[1], xs[2]], [both.ctypes.data + row, ys[1], ys[2]], count, F32)
        np.testing.assert_array_equal(both[n * count:].view(np.uint8), exchange(x, n)[0])


def test_the_alltoall_kernels_are_the_two_instances_without_scratch():
    """flat_alltoall_kernel<false> (packs) and <true> (bytes) in the LL code object, which stays one of 11: no
    private segment, no spilled vector register, no dynamic stack (read out of the shipped library)."""
    import test_code_objects as tco
    path = os.path.join(tco.PKG, "libnexr.so")
    assert os.path.exists(path), "libnexr.so not built"
    objects = tco.gfx950_code_objects(tco._read(path))
    seen = {}
    for co in objects:
        _tables, notes = tco.elf_tables(co)
        for k in (k for note in notes for k in note["amdhsa.kernels"]):
            if "alltoall" in k[".name"]:
                seen[k[".name"]] = (k[".private_segment_fixed_size"], k.get(".vgpr_spill_count", 0),
                                    k.get(".uses_dynamic_stack", False))
    assert len(objects) == 11
    assert len(seen) == 2 and all("flat_alltoall_kernel" in name for name in seen), sorted(seen)
    assert {name: v for name, v in seen.items() if v != (0, 0, False)} == {}
