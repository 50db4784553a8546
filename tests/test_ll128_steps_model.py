"""CPU tests that pin the LL128 step-list interpreter (tests/ll128_steps_model.py) before the GPU tests lean on
it: plain numpy for copy and integer-sum lists (user bytes, counters, heads and the mask of written slices),
the error for a list that would wait for ever, and the ring's own step lists for 2 and 3 ranks against the
oracle's independent restatement of the LL128 ring (oracle.ring.ring_allreduce_expected_ll)."""
import numpy as np
import pytest

import ll128_steps_model as model
import ll_steps_cases as cases
import make_golden as mg
from oracle.ring import ring_allreduce_expected_ll

S = model.Step


def _pair(dt, store, sizes, reduce, seed, slot=4096, start=(0, 0)):
    """Member 0 sends pieces of its input, member 1 receives them (reduced with its own input or not) into
    its output."""
    rng = np.random.default_rng(seed)
    total = int(sum(sizes)) + 3
    a = rng.integers(0, 256, total * np.dtype(store).itemsize, dtype=np.uint8).view(store)
    b = rng.integers(0, 256, total * np.dtype(store).itemsize, dtype=np.uint8).view(store)
    out = np.zeros_like(b)
    conn = model.Conn(slot, 8, start[0])
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    send = [S(0, int(o), -1, 0, int(n), False, True, False) for o, n in zip(offs, sizes)]
    recv = [S(0 if reduce else -1, int(o) if reduce else 0, 1, int(o) + 3, int(n), True, False, False)
            for o, n in zip(offs, sizes)]
    members = [model.Member(a, None, [], [conn], send), model.Member(b, out, [conn], [], recv)]
    return a, b, conn, members


@pytest.mark.parametrize("n_steps", [1, 8, 9, 40])
def test_copy_lists_are_numpy_copies(oracle, n_steps):
    sizes = [(1 + 37 * k) % 3841 for k in range(n_steps)]  # 0 < bytes <= 3840, the capacity of a 4 KiB slot
    a, _b, conn, members = _pair(mg.U8, np.uint8, sizes, False, n_steps, start=(5, 5))
    res = model.run(members, mg.U8, mg.SUM)
    total = sum(sizes)
    assert (res.members[1].output[3:3 + total] == a[:total]).all() and not res.members[1].output[:3].any()
    assert conn.sent == conn.read == conn.head == 5 + n_steps
    # the mask is the whole slices of what each slot was last... every slice any step wrote
    written = np.zeros(conn.fifo.size, dtype=bool)
    for k, n in enumerate(sizes):
        s = ((5 + k) % 8) * 4096
        written[s:s + model.slices_of(n) * 2048] = True
    assert (conn.mask == written).all()
    # every written line carries the flag of the last step that wrote it in word 15
    flags = conn.fifo.view(np.uint64).reshape(-1, 16)[:, 15]
    k_last = {(5 + k) % 8: k for k in range(n_steps)}
    for slot, k in k_last.items():
        lines = model.slices_of(sizes[k]) * 16
        assert (flags[slot * 32:slot * 32 + lines] == 5 + k + 1).all()


def test_integer_sum_lists_are_numpy_sums(oracle):
    sizes = [1, 480, 481, 960, 7, 959, 960, 3, 100, 960, 960, 5]  # int32 elements, <= 3840 bytes
    a, b, conn, members = _pair(mg.I32, np.int32, sizes, True, 3)
    res = model.run(members, mg.I32, mg.SUM)
    total = sum(sizes)
    got = res.members[1].output.view(np.int32)[3:3 + total]
    assert (got == (a[:total].astype(np.int64) + b[:total]).astype(np.int32)).all()
    assert conn.sent == conn.read == conn.head == len(sizes)


def test_a_list_that_would_wait_for_ever_raises(oracle):
    x, y = model.Conn(4096), model.Conn(4096)
    buf = np.zeros(64, dtype=np.uint8)
    recv_then_send = [S(-1, 0, 1, 0, 16, True, False, False), S(0, 0, -1, 0, 16, False, True, False)]
    members = [model.Member(buf, buf.copy(), [x], [y], recv_then_send),
               model.Member(buf, buf.copy(), [y], [x], recv_then_send)]
    with pytest.raises(model.StuckError):
        model.run(members, mg.U8, mg.SUM)
    # nine sends into eight slots with a receiver that never reads
    c = model.Conn(4096)
    members = [model.Member(buf, None, [], [c], [S(0, 0, -1, 0, 16, False, True, False)] * 9),
               model.Member(None, buf.copy(), [c], [], [])]
    with pytest.raises(model.StuckError):
        model.run(members, mg.U8, mg.SUM)
    # a step larger than its slot is the caller's error
    with pytest.raises(AssertionError):
        model.run([model.Member(np.zeros(4000, np.uint8), None, [], [model.Conn(4096)],
                                [S(0, 0, -1, 0, 3841, False, True, False)])], mg.U8, mg.SUM)


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("dt,op", [(mg.F32, 0), (mg.BF16, 0), (mg.I32, 3), (mg.F32, 4)])
def test_the_rings_own_step_lists_match_the_ring_oracle(oracle, n, dt, op):
    """Sum, Min and Avg over the ring's LL128 step lists at 8 slots of 4 KiB (several loops, a short last one)."""
    buff = 8 * 4096
    store = mg.STORE[dt]
    esz = np.dtype(store).itemsize
    count = 3 * n * model.ring_chunk(buff, esz) + 1234 // esz + 1
    inputs = mg.gen_inputs(dt, n, count, 11 * n + dt, special=False)
    exp = ring_allreduce_expected_ll(inputs, dt, op, buff, proto="ll128")
    dev_op, arg = oracle.host_to_dev_red_op(op, dt, n)
    conns = [model.Conn(4096, 8, 3 * r) for r in range(n)]  # conns[r]: into rank r
    members = [model.Member(inputs[r], np.zeros_like(inputs[r]), [conns[r]], [conns[(r + 1) % n]],
                            model.ring_allreduce_steps(n, r, count, model.ring_chunk(buff, esz), esz))
               for r in range(n)]
    res = model.run(members, dt, dev_op, arg)
    for r in range(n):
        assert mg.canon_bytes(dt, res.members[r].output.view(store)) == mg.canon_bytes(dt, exp[r]), r


def test_the_step_matrix_cases_run_as_ll128(oracle):
    """tests/ll_steps_cases.py's one-member lists fit an LL128 slot of the same size and run here unchanged."""
    for dt, name in [(mg.F16, "sum"), (mg.I8, "sumpostdiv")]:
        _n, op, arg = cases.op_named(dt, name)
        members, conns = model.model(cases.alone_case(dt, op, arg, 3, 3, 5))
        res = model.run(members, dt, op, arg)
        assert all(c.read == c.start + 8 for c in conns[:3]) and all(c.sent == c.start + 8 for c in conns[3:])
        assert len(res.trace) == 8
