"""The direct interpreter (tests/simple_direct_model.py) on the three direct ring schedules, without a GPU and
without the library under test: for 2, 3 and 5 members, with 1- and 2-step slices, every rank's output equals
oracle/ring.py's expected arrays, no FIFO byte is written, and the step counters equal those of the same
schedules run through FIFOs (where the outputs are the same too)."""
import numpy as np
import pytest

import ll_steps_cases as cases
import make_golden as mg
import simple_direct_cases as dc
import simple_direct_model as dm
from oracle.ring import all_gather_expected, broadcast_expected, ring_allreduce_expected

SLOT = 512          # bytes per FIFO step
DT, ESZ = mg.F32, 4
STEP = SLOT // ESZ  # elements per step


def _counters(conns):
    return [(c.sent, c.read, c.head) for c in conns]


def _run_both(make_lists, inputs, outputs, sps, dt=DT, op=mg.SUM, arg=0, in_place=False):
    """The direct run and the FIFO run of the same schedule: (direct members, direct conns, fifo members, fifo conns)."""
    res = []
    for direct in (True, False):
        lists = make_lists(direct)
        outs = [o.copy() for o in outputs]
        ins = outs if in_place else inputs
        members, conns = dm.ring_members(lists, ins, outs, SLOT, sps, start=2 * sps, direct=direct)
        dm.run(members, dt, op, arg)
        res += [members, conns]
    return res


@pytest.mark.parametrize("sps,spc", [(2, 2), (1, 1)])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_all_reduce(oracle, n, sps, spc):
    chunk = STEP * sps * spc
    count = 2 * n * chunk + n * 40 + 5   # two full loops and a last one of odd size
    inputs = mg.gen_inputs(DT, n, count, 900 + n, special=True)
    blank = [np.zeros(count, dtype=np.float32) for _ in range(n)]
    d, dc, f, fc = _run_both(lambda on: dm.all_reduce_lists(n, count, ESZ, STEP, sps, spc, on), inputs, blank, sps)
    exp = ring_allreduce_expected(inputs, DT, 0, buff_bytes=SLOT * 8 * sps * spc // 4)
    for r in range(n):
        assert mg.canon_bytes(DT, d[r].output.view(np.float32)) == mg.canon_bytes(DT, exp[r]), r
        assert d[r].output.tobytes() == f[r].output.tobytes(), r
        assert d[r].input.tobytes() == np.asarray(inputs[r]).tobytes(), r
    assert not any(c.mask.any() for c in dc)
    assert all(c.mask.any() for c in fc)
    assert _counters(dc) == _counters(fc)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("sps,spc", [(2, 2), (1, 1)])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_all_gather(oracle, n, sps, spc, in_place):
    per = 2 * STEP * sps * spc + 37
    xs = mg.gen_inputs(DT, n, per, 950 + n, special=False)
    outs = [np.zeros(per * n, dtype=np.float32) for _ in range(n)]
    if in_place:
        for r in range(n):
            outs[r][r * per:(r + 1) * per] = xs[r]
    d, dc, f, fc = _run_both(lambda on: dm.all_gather_lists(n, per, STEP, in_place, sps, spc, on), xs, outs, sps,
                             in_place=in_place)
    exp = all_gather_expected(xs)
    for r in range(n):
        assert d[r].output.tobytes() == exp[r].tobytes(), r
        assert f[r].output.tobytes() == exp[r].tobytes(), r
    assert not any(c.mask.any() for c in dc)
    assert _counters(dc) == _counters(fc)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_broadcast_from_every_root(oracle, n, in_place):
    count = 5 * STEP + 3
    xs = mg.gen_inputs(DT, n, count, 980 + n, special=False)
    for root in range(n):
        outs = [xs[r].copy() if (in_place and r == root) else np.zeros(count, dtype=np.float32) for r in range(n)]
        res = []
        for direct in (True, False):
            lists = dm.broadcast_lists(n, count, STEP, root, in_place, direct)
            o = [x.copy() for x in outs]
            ins = [o[r] if in_place else (xs[r] if r == root else None) for r in range(n)]
            members, conns = dm.ring_members(lists, ins, o, SLOT, 1, start=3, direct=direct)
            dm.run(members, DT, mg.SUM, 0)
            res += [members, conns]
        d, dc, f, fc = res
        exp = broadcast_expected(xs, root)
        for r in range(n):
            assert d[r].output.tobytes() == np.asarray(exp[r]).tobytes(), (root, r)
            assert f[r].output.tobytes() == np.asarray(exp[r]).tobytes(), (root, r)
        assert not any(c.mask.any() for c in dc)
        assert _counters(dc) == _counters(fc)


def _ring_fold(xs, dt, op, arg, chunk0):
    """The all-reduce of a SIMPLE ring by tests/golden/make_golden.py's numpy fold alone: chunk c starts at rank
    c + 1 with the pre-op, every following rank folds its own pre-op'd input first, rank c ends with the post-op."""
    n, count, esz = len(xs), xs[0].size, xs[0].itemsize
    out = np.empty_like(xs[0])
    chunk = chunk0
    for elem in range(0, count, n * chunk0):
        rem = count - elem
        if rem < n * chunk0:
            pack = 16 // esz
            chunk = ((rem + n - 1) // n + pack - 1) // pack * pack
        for c in range(n):
            sl = slice(elem + c * chunk, elem + min(c * chunk + chunk, rem))
            if sl.stop <= sl.start:
                continue
            acc = mg.reference_reduce(dt, op, arg, [xs[(c + 1) % n][sl]], [arg], False)
            for k in range(2, n + 1):
                acc = mg.reference_reduce(dt, op, arg, [xs[(c + k) % n][sl], acc], [arg], k == n)
            out[sl] = acc
    return out


@pytest.mark.parametrize("dt,name", cases.STAR_PAIRS)
def test_all_reduce_types_and_ops(oracle, dt, name):
    """The lists of tests/test_simple_direct_gpu.py::test_all_reduce_types_and_ops, all 56 accepted pairs, without
    a GPU: direct, every rank's output is the numpy fold of the ring order and the output of the same schedule run
    through FIFOs, no FIFO byte is written, and the step counters agree."""
    d = dc.types_and_ops_case(dt, name)
    f = dc.types_and_ops_case(dt, name, direct=False)
    xs = [m.input.copy() for m in d.members]
    dm.run(d.members, d.dt, d.op, d.arg)
    dm.run(f.members, f.dt, f.op, f.arg)
    store = mg.STORE[dt]
    exp = _ring_fold([x.view(store) for x in xs], dt, d.op, d.arg, d.slot // cases.esz_of(dt))
    for r, (a, b) in enumerate(zip(d.members, f.members)):
        assert mg.canon_bytes(dt, a.output.view(store)) == mg.canon_bytes(dt, exp), r
        assert a.output.tobytes() == b.output.tobytes(), r
        assert a.input.tobytes() == xs[r].tobytes(), r
    assert not any(c.mask.any() for c in d.conns) and all((c.fifo == dc.PATTERN).all() for c in d.conns)
    assert all(c.mask.any() for c in f.conns)
    assert _counters(d.conns) == _counters(f.conns)


def test_the_types_and_ops_cover_every_pair_the_api_accepts():
    assert len(cases.STAR_PAIRS) == len(set(cases.STAR_PAIRS)) == 56


def test_a_direct_receive_that_does_not_send_moves_no_data(oracle):
    """directRecv: the output keeps what the sender wrote there; with the record's bit clear the same record
    copies from the slot."""
    conn = dm.Conn(SLOT, 8, 0, 1)
    x = np.arange(64, dtype=np.float32)
    recv = dm.DMember(None, np.zeros(64, dtype=np.float32), [conn], [], [dm.DStep(-1, 0, 1, 0, 64, True, False, False, 1)],
                      recv_direct=True)
    send = dm.DMember(x, None, [], [conn], [dm.DStep(0, 0, -1, 0, 64, False, True, False, 2)], send_direct=[recv])
    dm.run([send, recv], DT, mg.SUM, 0)
    assert recv.output.tobytes() == x.tobytes() and not conn.mask.any()
    assert (conn.sent, conn.read, conn.head) == (1, 1, 1)
