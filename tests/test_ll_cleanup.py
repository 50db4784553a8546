"""CPU tests of the LL flag rule and the flag-wrap slot cleanup (nexrLLFlagRule, include/nexr.h; reference
src/device/prims_ll.h:85-93 incSend and the TEST_LL_CLEANUP mode of src/include/device.h:719-728) — no GPU
calls: the emulated ring in host memory with the oracle's LL step under the test rule {0x100, 0x78}, past
four flag periods and eight cleaning windows; the rule's validation in nexrReduceCopyLLStepsRule and
nexrRingCommSetLLFlagRule; nexrLLCleanSlot's argument checks; and the ctypes mirrors against the header.
"""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import make_golden as mg

TEST_RULE = (0x100, 0x78)
SLOTS = 8


@pytest.fixture(scope="module")
def ring(nexr):
    return importlib.import_module("nex-nccl_amd.ring")


@pytest.fixture(scope="module")
def oracle_ll_fn(oracle):
    return ctypes.cast(oracle.lib().oracle_reduce_copy_ll_fn, ctypes.c_void_p).value


def cleaning_steps_below(step, clean_mask):
    """How many send steps s < step clean: (s & mask) == mask."""
    period = 1 << clean_mask.bit_length()
    in_period = [s for s in range(period) if (s & clean_mask) == clean_mask]
    return len(in_period) * (step // period) + sum(1 for s in in_period if s < step % period)


@pytest.mark.parametrize("n_ranks", [2, 4])
def test_host_ring_cleans_under_the_test_rule(ring, oracle, oracle_ll_fn, n_ranks):
    """All-reduces on one communicator, alternating a count that fills the 4 KiB slots for many loops with
    one of a few lines, until every connection has sent 1024 steps (flags step % 256: four flag periods;
    mask 0x78: eight cleaning windows of eight steps). Every call is exact against the oracle's ring, and
    the communicator reports exactly the cleaning steps its counters imply."""
    from oracle.ring import ring_allreduce_expected_ll
    buff = 32 << 10
    big, small = n_ranks * 512 * 16 + 5, 9
    with ring.RingComm(n_ranks, ring.HOST_MEMORY, buff, None, 20000, ring.PROTO_LL, oracle_ll_fn) as comm:
        assert comm.ll_cleanup() == (0, 0)
        comm.set_ll_flag_rule(*TEST_RULE)
        lo, it = 0, 0
        while lo < 1024:
            count = big if it % 2 == 0 else small
            inputs = mg.gen_inputs(mg.F32, n_ranks, count, 0xC1EA + it, False)
            recv = [np.zeros_like(x) for x in inputs]
            comm.all_reduce([a.ctypes.data for a in inputs], [b.ctypes.data for b in recv], count, mg.F32, 0)
            exp = ring_allreduce_expected_ll(inputs, mg.F32, 0, buff)
            for r in range(n_ranks):
                assert mg.canon_bytes(mg.F32, recv[r]) == mg.canon_bytes(mg.F32, exp[r]), (it, r)
            lo, cleaned = comm.ll_cleanup()
            it += 1
            assert it < 200
        assert cleaned > 0 and cleaned >= n_ranks * 8 * (lo // 128)
        # a ring all-reduce advances every connection alike, so the count is exact
        assert cleaned == n_ranks * cleaning_steps_below(lo, TEST_RULE[1])
        assert comm.queued() == 0


def test_host_ring_production_rule_is_the_default(ring, oracle, oracle_ll_fn):
    """Without a rule (and with the production rule set explicitly, or NULL) nothing cleans in the first
    steps, and the results are those of the ring as it was."""
    from oracle.ring import ring_allreduce_expected_ll
    buff = 32 << 10
    for how in ("default", "explicit", "null"):
        with ring.RingComm(3, ring.HOST_MEMORY, buff, None, 20000, ring.PROTO_LL, oracle_ll_fn) as comm:
            if how == "explicit":
                comm.set_ll_flag_rule(0, 0x7FFFFFF8)
            elif how == "null":
                assert comm._L.nexrRingCommSetLLFlagRule(comm._h, None) == 0
            inputs = mg.gen_inputs(mg.I32, 3, 20_003, 77, True)
            recv = [np.zeros_like(x) for x in inputs]
            comm.all_reduce([a.ctypes.data for a in inputs], [b.ctypes.data for b in recv], 20_003, mg.I32, 0)
            exp = ring_allreduce_expected_ll(inputs, mg.I32, 0, buff)
            for r in range(3):
                assert np.array_equal(recv[r], exp[r])
            lo, cleaned = comm.ll_cleanup()
            assert lo > 0 and cleaned == 0


def test_set_rule_only_before_the_first_collective(ring, nexr, oracle_ll_fn):
    with ring.RingComm(2, ring.HOST_MEMORY, 32 << 10, None, 20000, ring.PROTO_LL, oracle_ll_fn) as comm:
        for bad in ((0x30, 0x78), (0, 0), (0x100, 0x7C), (0x40, 0x78)):
            with pytest.raises(nexr.NexrError) as e:
                comm.set_ll_flag_rule(*bad)
            assert e.value.code == nexr.Result.InvalidArgument, bad
        comm.set_ll_flag_rule(*TEST_RULE)
        comm.set_ll_flag_rule(0, 0x7FFFFFF8)  # still before the first collective
        x = [np.ones(64, np.float32) for _ in range(2)]
        y = [np.zeros(64, np.float32) for _ in range(2)]
        comm.all_reduce([a.ctypes.data for a in x], [b.ctypes.data for b in y], 64, mg.F32, 0)
        with pytest.raises(nexr.NexrError) as e:
            comm.set_ll_flag_rule(*TEST_RULE)
        assert e.value.code == nexr.Result.InvalidUsage
        L = comm._L
        lo = ctypes.c_uint64()
        assert L.nexrRingCommGetLLCleanup(comm._h, None, ctypes.byref(lo)) == nexr.Result.InvalidArgument
        assert L.nexrRingCommGetLLCleanup(None, ctypes.byref(lo), ctypes.byref(lo)) == nexr.Result.InvalidArgument
        assert L.nexrRingCommSetLLFlagRule(None, None) == nexr.Result.InvalidArgument


def _conns(nexr, n_slots=SLOTS):
    c = nexr.LLConnSet()
    c.input, c.output, c.nRecv, c.nSend = 0x10000, 0x20000, 1, 1
    c.recvFifo[0], c.recvHead[0] = 0x100000, 0x200000
    c.sendFifo[0], c.sendHead[0] = 0x300000, 0x400000
    c.slotBytes, c.nSlots = 1 << 16, n_slots
    return c


def test_steps_rule_is_validated_before_the_device(nexr):
    """nexrReduceCopyLLStepsRule rejects an invalid rule before anything is launched (the pointers here
    are not memory at all), and accepts NULL, the production rule and the test rule."""
    L = nexr.lib()
    step = nexr.ll_step(0, 0, 1, 0, 100, recv=True, send=True)
    arr = (nexr.LLStep * 1)(step)

    def call(rule, n_steps=1, n_slots=SLOTS):
        r = ctypes.byref(nexr.LLFlagRule(*rule)) if rule is not None else None
        return L.nexrReduceCopyLLStepsRule(ctypes.byref(_conns(nexr, n_slots)), arr, n_steps, 7, 0, 0, r, None, 0, None)

    assert call((0x30, 0x78)) == 4          # flagMax not a power of two
    assert call((0x100, 0)) == 4            # cleanMask = 0
    assert call((0x100, 0x7C)) == 4         # cleanMask % nSlots != 0
    assert call((0, 0x7FFFFFFC)) == 4       # the same for the 32-bit flags
    assert call((0x40, 0x78)) == 4          # cleaning period 128 above the flag period 64
    assert call((1, 0x78)) == 4             # one flag value only
    assert call((0x100, 0x78), n_slots=16) == 4   # 0x78 % 16 != 0: valid for 8 slots only
    assert call((0x100, 0x70), n_steps=0, n_slots=16) == 0
    assert call((0x80, 0x78), n_steps=0) == 0     # cleaning period == flag period
    for ok in (None, (0, 0x7FFFFFF8), TEST_RULE, (0, 0x80000000), (0, 0xFFFFFFF8)):
        assert call(ok, n_steps=0) == 0, ok
    # nSlots above INT_MAX would turn negative in the kernels (they keep it as an int): refused, though the
    # rule itself is valid for that many slots (0x80000000 % 0x80000000 == 0); INT_MAX slots themselves pass
    assert call((0, 0x80000000), n_steps=0, n_slots=0x80000000) == 4
    assert call((0, 0x80000000), n_steps=1, n_slots=0x80000000) == 4
    assert call((0, 0xFFFFFFFF), n_steps=0, n_slots=0xFFFFFFFF) == 4
    assert call((0, 0x7FFFFFFF), n_steps=0, n_slots=0x7FFFFFFF) == 0
    with pytest.raises(nexr.NexrError) as e:
        nexr.reduce_copy_ll_steps(0x10000, 0x20000, [(0x100000, 0x200000, 0)], [], 1 << 16, [step], 7, 0,
                                  rule=(0x30, 0x78))
    assert e.value.code == nexr.Result.InvalidArgument


def test_clean_slot_validates_before_the_device(nexr):
    L = nexr.lib()
    u32 = ctypes.c_uint32

    def call(ptrs, first, lines, n=None, flags=True):
        arr = (ctypes.c_void_p * 9)(*ptrs) if ptrs is not None else None
        fl = (u32 * 9)(*([5] * 9)) if flags else None
        return L.nexrLLCleanSlot(len(ptrs) if n is None else n, arr, fl, first, lines, None)

    assert call([0x1008], 0, 256) == 4                   # not 16-B aligned
    assert call([0x1000, 0], 0, 256) == 4                # NULL slot
    assert call(None, 0, 256, n=1) == 4                  # no slot array
    assert call([0x1000], 0, 256, flags=False) == 4      # no flags
    assert call([0x1000] * 9, 0, 256) == 4               # > NEXR_MAX_DSTS
    assert call([0x1000], 0, 256, n=-1) == 4
    assert call([0x1008], 256, 256) == 4                 # validated even when there is nothing to write
    assert call([0x1000], 256, 256) == 0                 # firstLine == slotLines: no-op, nothing launched
    assert call([0x1000, 0x2000], 300, 256) == 0
    assert call([], 0, 256) == 0
    with pytest.raises(nexr.NexrError):
        nexr.ll_clean_slot([0x1004], [1], 0, 16)
    nexr.ll_clean_slot([0x1000], [1], 16, 16)


def test_flag_helpers_follow_the_reference_macros(nexr):
    """ll_flag(step) is NCCL_LL_FLAG(step + 1); ll_cleans(step) is (step & NCCL_LL_CLEAN_MASK) ==
    NCCL_LL_CLEAN_MASK — production (device.h:726-727) and TEST_LL_CLEANUP (:720-723)."""
    assert nexr.ll_flag(0) == 1 and nexr.ll_flag(0xFFFFFFFE) == 0xFFFFFFFF and nexr.ll_flag(0xFFFFFFFF) == 0
    assert nexr.ll_flag((1 << 32) + 6) == 7
    assert [s for s in range(0x7FFFFFF0, 0x80000004) if nexr.ll_cleans(s)] == list(range(0x7FFFFFF8, 0x80000000))
    assert not nexr.ll_cleans(0) and nexr.ll_cleans(0xFFFFFFFF) and nexr.ll_cleans((1 << 32) + 0x7FFFFFF8)
    assert nexr.ll_flag(254, TEST_RULE) == 255 and nexr.ll_flag(255, TEST_RULE) == 0
    assert nexr.ll_flag(256, nexr.LLFlagRule(*TEST_RULE)) == 1
    assert [s for s in range(300) if nexr.ll_cleans(s, TEST_RULE)] == list(range(120, 128)) + list(range(248, 256))
    assert nexr.LL_TEST_RULE == TEST_RULE and nexr.LL_PRODUCTION_RULE == (0, 0x7FFFFFF8)


_RULE_LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "nexr_ring.h"
int main(void) {
  nexrResult_t (*steps)(const nexrLLConnSet*, const nexrLLStep*, int, int, int, uint64_t, const nexrLLFlagRule*,
                        uint32_t*, uint32_t, nexrStream_t) = nexrReduceCopyLLStepsRule;
  nexrResult_t (*clean)(int, void* const*, const uint32_t*, size_t, size_t, nexrStream_t) = nexrLLCleanSlot;
  nexrResult_t (*set)(nexrRingComm_t, const nexrLLFlagRule*) = nexrRingCommSetLLFlagRule;
  nexrResult_t (*get)(nexrRingComm_t, uint64_t*, uint64_t*) = nexrRingCommGetLLCleanup;
  printf("%zu %zu %zu %d\n", sizeof(nexrLLFlagRule), offsetof(nexrLLFlagRule, flagMax),
         offsetof(nexrLLFlagRule, cleanMask), steps && clean && set && get);
  return 0;
}
"""


def test_mirrors_and_symbols_match_the_headers(nexr, ring, tmp_path):
    """nexrLLFlagRule's C layout and the ctypes mirror agree; the new entry points have the documented C
    signatures (plain C11), are exported, and are listed in ABI_SYMBOLS / RING_ABI_SYMBOLS."""
    src = tmp_path / "rule_layout.c"
    src.write_text(_RULE_LAYOUT)
    exe = tmp_path / "rule_layout"
    lib = os.path.join(ROOT, "nex-nccl_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                    "-L" + lib, "-lnexr_ring", "-lnexr", "-Wl,-rpath," + lib, "-o", str(exe)], check=True,
                   capture_output=True, text=True, timeout=120)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    R = nexr.LLFlagRule
    assert out == [str(v) for v in (ctypes.sizeof(R), R.flagMax.offset, R.cleanMask.offset, 1)]
    assert ctypes.sizeof(R) == 8
    decl = r"NEXR_API\s+[\w\s\*]+?\b(nexr\w+)\s*\("
    core = set(re.findall(decl, open(os.path.join(ROOT, "include", "nexr.h")).read()))
    rng = set(re.findall(decl, open(os.path.join(ROOT, "include", "nexr_ring.h")).read()))
    assert {"nexrReduceCopyLLStepsRule", "nexrLLCleanSlot"} <= core and core == set(nexr.ABI_SYMBOLS)
    assert {"nexrRingCommSetLLFlagRule", "nexrRingCommGetLLCleanup"} <= rng and rng == set(ring.RING_ABI_SYMBOLS)
    for name in ("nexrReduceCopyLLStepsRule", "nexrLLCleanSlot"):
        assert hasattr(nexr.lib(), name)
    for name in ("nexrRingCommSetLLFlagRule", "nexrRingCommGetLLCleanup"):
        assert hasattr(ring.ring_lib(), name)
    assert nexr.version() == 300
