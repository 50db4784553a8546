"""The LL flag-wrap slot cleanup on the GPU (nexrLLFlagRule, nexrReduceCopyLLStepsRule, nexrLLCleanSlot,
nexrRingCommSetLLFlagRule; reference src/device/prims_ll.h:85-93 incSend, src/include/device.h:719-728).

The shared expectation is a numpy model of the wire: send step k writes slot k % 8; its lines [0, nLines)
carry the step's flag, and on a cleaning step the lines [nLines, slotLines) are {0, flag, 0, flag}. After
the streams are synchronised the FIFO is read back and every line's two flag words are compared with the
model, and the data words of cleaned (and untouched) lines with 0 — which does not depend on who polled
first. Outputs are compared exactly as well."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import make_golden as mg

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = 8
TEST_RULE = (0x100, 0x78)


def _tile_lines():
    """kLLTileLines as the kernels are built (nex-nccl_amd/csrc/nexr_internal.h): kLLU * 2 * kBlock."""
    text = open(os.path.join(ROOT, "nex-nccl_amd", "csrc", "nexr_internal.h")).read()
    block = int(re.search(r"constexpr int kBlock = (\d+);", text).group(1))
    unroll = int(re.search(r"#define NEXR_LL_U (\d+)", text).group(1))
    assert re.search(r"constexpr int kLLSubLines = 2 \* kBlock;", text)
    assert re.search(r"constexpr int kLLTileLines = kLLU \* kLLSubLines;", text)
    return unroll * 2 * block


TILE = _tile_lines()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class _OwnQueueStreams:
    """Streams with a hardware queue of their own (hipExtStreamCreateWithCUMask, every CU in the mask):
    a run waits for its peer's, so the two must not share one of HIP's GPU_MAX_HW_QUEUES queues, on
    which kernels run one after the other (the ring library makes its rank streams the same way)."""

    def __init__(self, nexr):
        self.hip = nexr.hip_runtime()
        self.hip.hipExtStreamCreateWithCUMask.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32,
                                                          ctypes.POINTER(ctypes.c_uint32)]
        self.hip.hipExtStreamCreateWithCUMask.restype = ctypes.c_int
        self.hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        words = [0xFFFFFFFF] * ((cus + 31) // 32)
        if cus % 32:
            words[-1] = (1 << (cus % 32)) - 1
        self.mask = (ctypes.c_uint32 * len(words))(*words)
        self.made = []

    def __call__(self, n):
        out = []
        for _ in range(n):
            h = ctypes.c_void_p()
            assert self.hip.hipExtStreamCreateWithCUMask(ctypes.byref(h), len(self.mask), self.mask) == 0
            self.made.append(h.value)
            out.append(h.value)
        return out

    def close(self):
        torch.cuda.synchronize()
        for h in self.made:
            self.hip.hipStreamDestroy(h)


@pytest.fixture(scope="module")
def streams(nexr):
    s = _OwnQueueStreams(nexr)
    yield s
    s.close()


def _conn(slot_bytes):
    """A connection's receive FIFO with its head words behind it, zeroed (as nexr_ring.cpp makes them)."""
    buf = torch.zeros(slot_bytes * SLOTS + 4096, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr(), buf.data_ptr() + slot_bytes * SLOTS


def _status():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def _flag(step, rule):
    """NCCL_LL_FLAG(step + 1) under the rule (None: production), restated here for the model."""
    flag_max = rule[0] if rule else 0
    return (step + 1) % flag_max if flag_max else (step + 1) & 0xFFFFFFFF


def _cleans(step, rule):
    mask = rule[1] if rule else 0x7FFFFFF8
    return (step & mask) == mask


class Wire:
    """The model: per slot and line the flag both flag words must hold, and whether the data words must be 0
    (cleaned lines, and the lines of the zero-filled FIFO nobody has written)."""

    def __init__(self, nexr, slot_lines, rule):
        self.nexr, self.rule, self.slot_lines = nexr, rule, slot_lines
        self.flag = np.zeros((SLOTS, slot_lines), np.uint32)
        self.zero = np.ones((SLOTS, slot_lines), bool)

    def send(self, step, n_lines):
        s, f = step % SLOTS, _flag(step, self.rule)
        self.flag[s, :n_lines] = f
        self.zero[s, :n_lines] = False
        if _cleans(step, self.rule):
            self.flag[s, n_lines:] = f
            self.zero[s, n_lines:] = True

    def check(self, fifo_tensor):
        lines = fifo_tensor[:SLOTS * self.slot_lines * 16].cpu().numpy().view(np.uint32).reshape(SLOTS, -1, 4)
        for word in (1, 3):
            bad = np.argwhere(lines[:, :, word] != self.flag)
            assert not len(bad), (word, bad[:4].tolist(), [hex(lines[s, l, word]) for s, l in bad[:4]],
                                  [hex(self.flag[s, l]) for s, l in bad[:4]])
        assert not lines[:, :, 0][self.zero].any() and not lines[:, :, 2][self.zero].any()


def _pair_run(nexr, dev, streams, slot_bytes, step0, line_counts, rule, dt=mg.F32, odd_bytes=False):
    """A sender run and a receiver run (receive + reduce into the output) on one connection, both counters
    starting at step0, step k moving line_counts[k] lines (odd_bytes: 3 bytes short of them, int8). The
    receiver's run is queued first. Returns nothing: asserts the outputs, the status words and the wire."""
    np_t = np.dtype(mg.STORE[dt])
    esz = np_t.itemsize
    sizes = [(8 * n - 3 if odd_bytes and n else 8 * n) // esz for n in line_counts]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offs[-1])
    rng = np.random.default_rng(slot_bytes + step0 + len(line_counts))
    a = rng.integers(-50, 50, total).astype(np_t)
    b = rng.integers(-50, 50, total).astype(np_t)
    da, db = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    out = torch.zeros(total, dtype=da.dtype, device=dev)
    keep, fifo, head = _conn(slot_bytes)
    sa, sb = streams(2)
    st_a, st_b = _status(), _status()
    torch.cuda.synchronize()
    n = len(sizes)
    b_steps = [nexr.ll_step(0, int(offs[k]), 1, int(offs[k]), sizes[k], recv=True) for k in range(n)]
    a_steps = [nexr.ll_step(0, int(offs[k]), -1, 0, sizes[k], send=True) for k in range(n)]
    kw = {"rule": rule} if rule is not None else {}  # no rule: the plain nexrReduceCopyLLSteps
    nexr.reduce_copy_ll_steps(db.data_ptr(), out.data_ptr(), [(fifo, head, step0)], [], slot_bytes, b_steps, dt, 0,
                              status=st_b.data_ptr(), timeout_us=5_000_000, stream=sb, **kw)
    nexr.reduce_copy_ll_steps(da.data_ptr(), 0, [], [(fifo, head, step0)], slot_bytes, a_steps, dt, 0,
                              status=st_a.data_ptr(), timeout_us=5_000_000, stream=sa, **kw)
    torch.cuda.synchronize()
    assert int(st_a.item()) == 0 and int(st_b.item()) == 0
    assert np.array_equal(out.cpu().numpy(), a + b)
    wire = Wire(nexr, slot_bytes // 16, rule)
    for k in range(n):
        wire.send(step0 + k, line_counts[k])
    wire.check(keep)
    return wire


@pytest.mark.parametrize("slot_bytes", [4096, 1 << 16])
def test_production_rule_cleans_at_the_flag_wrap(nexr, dev, streams, slot_bytes):
    """The plain nexrReduceCopyLLSteps (rule = NULL) across send steps 0x7ffffff8-0x7fffffff: 16 steps from
    0x7ffffff4, a full slot and 3 lines in turn. Output exact, status words 0, and the FIFO equal to the
    model: all eight slots fully flagged 0x7ffffff9 .. 0x80000000 by the eight cleaning steps, then the
    data lines of the four steps after them."""
    slot_lines = slot_bytes // 16
    counts = [slot_lines if k % 2 == 0 else 3 for k in range(16)]
    wire = _pair_run(nexr, dev, streams, slot_bytes, 0x7FFFFFF4, counts, None)
    assert wire.flag.min() >= 0x7FFFFFF9 and wire.flag.max() == 0x80000004  # the model itself: no line left behind
    # slot s was cleaned by step 0x7ffffff8 + s (flag 0x7ffffff9 + s); slots 0 and 2 were then filled again
    # by the full steps 0x80000000 and 0x80000002, slots 1 and 3 got 3 lines only and keep the clean flag
    assert [int(wire.flag[s, -1]) for s in range(SLOTS)] == [0x80000001, 0x7FFFFFFA, 0x80000003, 0x7FFFFFFC,
                                                             0x7FFFFFFD, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000]


def _candidates(slot_lines):
    """Line counts at which the cleanup takes another path: none, one, the wave's two half-rows (64) and
    its 128 lines, the tile, a full slot — those that fit the slot."""
    c = [0, 1, 63, 64, 65, 128, 129, TILE - 1, TILE, TILE + 1, slot_lines]
    return [v for i, v in enumerate(c) if v <= slot_lines and v not in c[:i]]


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("slot_bytes", [4096, 1 << 16, 1 << 20])
def test_test_rule_every_line_count(nexr, dev, streams, slot_bytes, shift):
    """Rule {0x100, 0x78}, counters from 0x70, 24 steps (the cleaning steps are 0x78-0x7f): one workgroup
    (4 KiB slots), eight (64 KiB) and the 64-workgroup cap with two strided tiles each (1 MiB). The two
    shifts put every candidate line count on a cleaning step."""
    cand = _candidates(slot_bytes // 16)
    counts = [cand[(k + shift) % len(cand)] for k in range(24)]
    cleaning = {counts[k] for k in range(8, 16)}
    assert 0 in cleaning or shift  # the empty step cleans a whole slot (shift 0)
    _pair_run(nexr, dev, streams, slot_bytes, 0x70, counts, TEST_RULE)


def test_test_rule_partial_last_data_line(nexr, dev, streams):
    """int8 with an odd byte count: the last data line is partial (its flags still the step's, as storeLL
    writes whole lines), and the clean lines start right behind it."""
    cand = _candidates((1 << 16) // 16)
    counts = [cand[(k + 2) % len(cand)] for k in range(24)]
    _pair_run(nexr, dev, streams, 1 << 16, 0x70, counts, TEST_RULE, dt=mg.I8, odd_bytes=True)


def _wrap_sizes(n_steps, slot_lines):
    return [slot_lines if k % 9 == 0 else 2 + k % 4 for k in range(n_steps)]


def test_receiver_across_wraps_two_ranks(nexr, dev, streams):
    """600 steps on one connection under the test rule, 4 KiB slots: more than two flag periods and four
    cleaning windows; every ninth step a full slot, the rest 2-5 lines; the receiver queued first."""
    counts = _wrap_sizes(600, 256)
    _pair_run(nexr, dev, streams, 4096, 0, counts, TEST_RULE)


def test_receiver_across_wraps_three_connections(nexr, oracle, dev, streams):
    """A -> B -> C over the same 600 steps (B a receiver and a sender in every step), bf16 sum, against the
    oracle's LL step for the fold order; both FIFOs equal to the model."""
    from oracle.ring import reduce_expected
    dt, op, slot = mg.BF16, 0, 4096
    counts = _wrap_sizes(600, slot // 16)
    sizes = [4 * c for c in counts]
    offs = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)])]
    total, n = offs[-1], len(sizes)
    xs = mg.gen_inputs(dt, 3, total, 0xC1EA, special=True)
    dev_op, arg = oracle.host_to_dev_red_op(op, dt, 3)
    dx = [torch.from_numpy(x.copy()).to(dev) for x in xs]
    out = torch.zeros_like(dx[2])
    ab, ab_fifo, ab_head = _conn(slot)
    bc, bc_fifo, bc_head = _conn(slot)
    ss = streams(3)
    st = _status()
    torch.cuda.synchronize()
    common = dict(status=st.data_ptr(), timeout_us=5_000_000, rule=TEST_RULE)
    nexr.reduce_copy_ll_steps(dx[2].data_ptr(), out.data_ptr(), [(bc_fifo, bc_head, 0)], [], slot,
                              [nexr.ll_step(0, offs[k], 1, offs[k], sizes[k], recv=True, post_op=True)
                               for k in range(n)], dt, dev_op, arg, stream=ss[2], **common)
    nexr.reduce_copy_ll_steps(dx[1].data_ptr(), 0, [(ab_fifo, ab_head, 0)], [(bc_fifo, bc_head, 0)], slot,
                              [nexr.ll_step(0, offs[k], -1, 0, sizes[k], recv=True, send=True) for k in range(n)],
                              dt, dev_op, arg, stream=ss[1], **common)
    nexr.reduce_copy_ll_steps(dx[0].data_ptr(), 0, [], [(ab_fifo, ab_head, 0)], slot,
                              [nexr.ll_step(0, offs[k], -1, 0, sizes[k], send=True) for k in range(n)],
                              dt, dev_op, arg, stream=ss[0], **common)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    exp = reduce_expected(xs, dt, op, 2, "ll")
    assert mg.canon_bytes(dt, out.cpu().numpy()) == mg.canon_bytes(dt, exp)
    wire = Wire(nexr, slot // 16, TEST_RULE)
    for k in range(n):
        wire.send(k, counts[k])
    wire.check(ab)
    wire.check(bc)


def test_clean_slot_after_single_steps(nexr, dev):
    """The single-step contract: a full slot written by nexrReduceCopyLL at step 0 (flag F = 1), then the 31
    later steps that reuse that slot before F recurs under the test rule (steps 8, 16, .. 248), each a
    3-line nexrReduceCopyLL followed by nexrLLCleanSlot when the step cleans (120 and 248), all on one
    stream. No line of the slot carries F any more, and the slot equals the model."""
    slot_lines = 256
    keep, fifo, _head = _conn(slot_lines * 16)
    x = torch.arange(2 * slot_lines, dtype=torch.float32, device=dev)
    wire = Wire(nexr, slot_lines, TEST_RULE)
    s = torch.cuda.current_stream().cuda_stream
    cleaned = []
    for step in range(0, 256, SLOTS):
        n_lines = slot_lines if step == 0 else 3
        flag = nexr.ll_flag(step, TEST_RULE)
        nexr.reduce_copy_ll(x.data_ptr(), [], [], 0, [fifo], [flag], 2 * n_lines, mg.F32, 0, stream=s)
        if nexr.ll_cleans(step, TEST_RULE):
            nexr.ll_clean_slot([fifo], [flag], n_lines, slot_lines, stream=s)
            cleaned.append(step)
        wire.send(step, n_lines)
    torch.cuda.synchronize()
    assert cleaned == [120, 248]
    lines = keep[:slot_lines * 16].cpu().numpy().view(np.uint32).reshape(-1, 4)
    f0 = nexr.ll_flag(0, TEST_RULE)
    assert nexr.ll_flag(256, TEST_RULE) == f0 and not (lines[:, 1] == f0).any() and not (lines[:, 3] == f0).any()
    wire.check(keep)
    assert np.array_equal(lines[:3, 0].view(np.float32), [0, 2, 4]) and np.array_equal(lines[:3, 2].view(np.float32),
                                                                                       [1, 3, 5])


def test_clean_slot_ranges_and_arguments(nexr, dev):
    """firstLine = 0, firstLine inside a tile of a slot that is no multiple of the tile, firstLine ==
    slotLines (nothing written), two slots in one call; nothing before firstLine or behind the slot is
    touched; a misaligned or NULL slot is nexrInvalidArgument."""
    slot_lines = 2 * TILE + 476
    first = TILE + 188

    def fresh():
        return torch.full(((slot_lines + 64) * 4,), 0xABABABAB - (1 << 32), dtype=torch.int32, device=dev)

    def view(t):
        return t.cpu().numpy().view(np.uint32).reshape(-1, 4)

    a, b, c, d = fresh(), fresh(), fresh(), fresh()
    torch.cuda.synchronize()
    nexr.ll_clean_slot([a.data_ptr()], [7], 0, slot_lines)
    nexr.ll_clean_slot([b.data_ptr(), c.data_ptr()], [0x11, 0x80000022], first, slot_lines)
    nexr.ll_clean_slot([d.data_ptr()], [9], slot_lines, slot_lines)
    torch.cuda.synchronize()
    va, vb, vc, vd = view(a), view(b), view(c), view(d)
    assert (va[:slot_lines] == [0, 7, 0, 7]).all() and (va[slot_lines:] == 0xABABABAB).all()
    for v, f in ((vb, 0x11), (vc, 0x80000022)):
        assert (v[:first] == 0xABABABAB).all() and (v[first:slot_lines] == [0, f, 0, f]).all()
        assert (v[slot_lines:] == 0xABABABAB).all()
    assert (vd == 0xABABABAB).all()
    for bad in ([a.data_ptr() + 8], [a.data_ptr(), 0]):
        with pytest.raises(nexr.NexrError) as e:
            nexr.ll_clean_slot(bad, [1] * len(bad), 0, 16)
        assert e.value.code == nexr.Result.InvalidArgument
    torch.cuda.synchronize()
    assert (view(a)[:slot_lines] == [0, 7, 0, 7]).all()


def _cleaning_steps_below(step, clean_mask):
    period = 1 << clean_mask.bit_length()
    in_period = [s for s in range(period) if (s & clean_mask) == clean_mask]
    return len(in_period) * (step // period) + sum(1 for s in in_period if s < step % period)


def ring_until(n_ranks, target=1024):
    """All-reduces on one device-memory LL communicator with 4 KiB slots under the test rule, a count that
    fills the slots for many loops and one of a few lines in turn, until every connection has sent
    `target` steps; every call exact against the oracle's ring. Returns (queued, min_send_step, cleaned)."""
    import importlib
    from oracle.ring import ring_allreduce_expected_ll
    ring = importlib.import_module("nex-nccl_amd.ring")
    buff = 32 << 10
    big, small = n_ranks * 512 * 64 + 5, 9
    with ring.RingComm(n_ranks, ring.DEVICE_MEMORY, buff, None, 20000, ring.PROTO_LL) as comm:
        comm.set_ll_flag_rule(*TEST_RULE)
        lo, it = 0, 0
        while lo < target:
            count = big if it % 2 == 0 else small
            inputs = mg.gen_inputs(mg.F32, n_ranks, count, 0xD0 + it, False)
            send = [torch.from_numpy(x.copy()).cuda() for x in inputs]
            recv = [torch.zeros_like(s) for s in send]
            torch.cuda.synchronize()
            comm.all_reduce([s.data_ptr() for s in send], [d.data_ptr() for d in recv], count, mg.F32, 0)
            exp = ring_allreduce_expected_ll(inputs, mg.F32, 0, buff)
            for r in range(n_ranks):
                assert mg.canon_bytes(mg.F32, recv[r].cpu().numpy()) == mg.canon_bytes(mg.F32, exp[r]), (it, r)
            lo, cleaned = comm.ll_cleanup()
            it += 1
            assert it < 100
        return comm.queued(), lo, cleaned


def _check_ring(n_ranks, queued, lo, cleaned, want_queued):
    assert lo >= 1024
    assert cleaned > 0 and cleaned >= n_ranks * 8 * (lo // 128)
    assert cleaned == n_ranks * _cleaning_steps_below(lo, TEST_RULE[1])  # every connection advances alike
    assert queued == (want_queued if torch.cuda.device_count() == 1 else 0)


@pytest.mark.parametrize("n_ranks", [2, 3])
def test_ring_cleans_in_device_runs(oracle, dev, n_ranks):
    """The default mode: runs on the device (queued() == 2 as before), the rule passed by flushRun."""
    _check_ring(n_ranks, *ring_until(n_ranks), want_queued=2)


@pytest.mark.parametrize("env,want", [({"NEXR_LL_RUN": "0"}, 1), ({"NEXR_LL_ASYNC": "0"}, 0)])
def test_ring_cleans_in_queued_and_host_sequenced_steps(env, want):
    """NEXR_LL_RUN=0 (queued launches) and NEXR_LL_ASYNC=0 (host-sequenced), each read once per process, so
    in a fresh child: nexrLLCleanSlot on the rank's stream behind the cleaning step's kernel."""
    code = ("import sys, json; sys.path[:0] = [%r, %r, %r]; import test_ll_cleanup_gpu as t; "
            "print(json.dumps([t.ring_until(n) for n in (2, 3)]))"
            % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True,
                         timeout=150)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("[")][-1])
    for n_ranks, (queued, lo, cleaned) in zip((2, 3), res):
        _check_ring(n_ranks, queued, lo, cleaned, want_queued=want)
