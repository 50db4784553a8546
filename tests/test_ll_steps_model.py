"""CPU tests of the sequential interpreter of LL step lists (oracle/ll_steps.py), the reference of
tests/test_ll_steps_matrix_gpu.py, against things that do not come from the library under test: numpy's
own arithmetic, the flag and cleaning rules as the header states them, and a list that cannot finish. Also
here: every step list of the matrix runs to its end in the interpreter, and the matrix's parametrisation
covers every (datatype, op) pair the API accepts."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

import ll_steps_cases as cases
import make_golden as mg
from oracle import ll_steps

S = ll_steps.Step


def _run(case):
    members, conns = cases.model(case)
    return ll_steps.run(members, case.dt, case.op, case.arg), conns


@pytest.mark.parametrize("dt", list(mg.INTS))
def test_integer_sum_through_a_star_is_numpys_wrapping_sum(oracle, dt):
    case = cases.star_case(dt, mg.SUM, 0, 4096, cases.star_sizes(dt, 4096), 100 + dt)
    res, conns = _run(case)
    with np.errstate(over="ignore"):
        want = case.members[0].input.copy()
        for m in case.members[1:]:
            want = want + m.input
    assert want.dtype == mg.STORE[dt]
    for m, mb in enumerate(res.members):
        assert mb.output.tobytes() == want.tobytes(), m
        assert mb.input.tobytes() == case.members[m].input.tobytes(), m
    # 11 pieces on every connection, from its own counter
    assert [(c.sent, c.read) for c in conns] == [(s + 11, s + 11) for s in case.conn_start]


def test_fp32_sum_of_two_is_numpys(oracle):
    rng = np.random.default_rng(1)
    n, per = 5 * 300 - 7, 300
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    sizes = [per] * 4 + [n - 4 * per]
    conn = ll_steps.Conn(4096, 8, 6)
    send = [S(0, k * per, -1, 0, sizes[k], False, True) for k in range(5)]
    recv = [S(0, k * per, 1, k * per, sizes[k], True, False) for k in range(5)]
    res = ll_steps.run([ll_steps.Member(b, np.zeros(n, np.float32), [conn], [], recv),
                        ll_steps.Member(a, None, [], [conn], send)], mg.F32, mg.SUM)
    assert res.members[0].output.view(np.uint32).tolist() == (a + b).view(np.uint32).tolist()
    # the receiver was asked first in every round and had to wait for the sender
    assert [t[0] for t in res.trace[:4]] == [1, 0, 1, 0]


def test_a_crossed_pair_is_stuck(oracle):
    x, y = ll_steps.Conn(4096), ll_steps.Conn(4096)
    data = np.arange(64, dtype=np.float32)
    recv, send = S(-1, 0, 1, 0, 64, True, False), S(0, 0, -1, 0, 64, False, True)
    with pytest.raises(ll_steps.StuckError):
        ll_steps.run([ll_steps.Member(data, data, [x], [y], [recv, send]),
                      ll_steps.Member(data, data, [y], [x], [recv, send])], mg.F32, mg.SUM)
    # either member sending first, the same pair finishes
    x, y = ll_steps.Conn(4096), ll_steps.Conn(4096)
    res = ll_steps.run([ll_steps.Member(data, data, [x], [y], [send, recv]),
                        ll_steps.Member(data, data, [y], [x], [recv, send])], mg.F32, mg.SUM)
    assert all(mb.pos == 2 for mb in res.members)
    # a ninth send into eight slots nobody reads is stuck as well; into a FIFO whose receiver is elsewhere it is not
    z = ll_steps.Conn(4096)
    with pytest.raises(ll_steps.StuckError):
        ll_steps.run([ll_steps.Member(data, None, [], [z], [send] * 9),
                      ll_steps.Member(None, data, [z], [], [])], mg.F32, mg.SUM)
    assert ll_steps.run([ll_steps.Member(data, None, [], [ll_steps.Conn(4096)], [send] * 9)], mg.F32, mg.SUM)
    # and so is a receive from a FIFO nobody has written
    with pytest.raises(ll_steps.StuckError):
        ll_steps.run([ll_steps.Member(None, data, [ll_steps.Conn(4096)], [], [recv])], mg.F32, mg.SUM)


def test_connections_at_different_counters_carry_different_flags(oracle):
    """One step on three receive and three send connections that start at 5, 14, 23 and 3, 9, 16: each
    line is looked for and written in its connection's own slot with its connection's own flag."""
    case = cases.alone_case(mg.I32, mg.SUM, 0, 3, 3, 7)
    res, conns = _run(case)
    _m, _k, rinfo, sinfo = res.trace[0]
    assert rinfo == [(5, 6), (6, 15), (7, 24)] and sinfo == [(3, 4), (1, 10), (0, 17)]
    for c, (slot, flag) in zip(conns[3:], sinfo):
        words = c.fifo.view(np.uint32).reshape(8, -1, 4)
        assert words[slot, 0, 1] == flag and words[slot, 0, 3] == flag
    assert [(c.sent, c.read) for c in conns[:3]] == [(13, 13), (22, 22), (31, 31)]
    assert [c.sent for c in conns[3:]] == [11, 17, 24]
    # a line at the wrong flag is not taken: the same list with one FIFO written at another counter fails
    members, conns = cases.model(case)
    other = ll_steps.Conn(4096, 8, 13)
    other.prefill(case.prefill[1])
    conns[1].fifo[:] = other.fifo
    with pytest.raises(ValueError):
        ll_steps.run(members, case.dt, case.op, case.arg)


def test_the_test_rule_cleans_steps_0x78_to_0x7f_of_every_0x80(oracle):
    conn = ll_steps.Conn(4096, 8, 0, cases.TEST_RULE)
    data = np.arange(6, dtype=np.float32)  # 3 lines
    n_steps = 0x200
    res = ll_steps.run([ll_steps.Member(data, None, [], [conn], [S(0, 0, -1, 0, 6, False, True)] * n_steps)],
                       mg.F32, mg.SUM)
    want = [s for base in range(0, n_steps, 0x80) for s in range(base + 0x78, base + 0x80)]
    assert res.conns[0].cleaned == want
    assert want == [s for s in range(n_steps) if ll_steps.ll_cleans(s, cases.TEST_RULE)]
    # the last eight steps cleaned one slot each: 3 data lines at the step's flag, then {0, f, 0, f}
    lines = conn.fifo.view(np.uint32).reshape(8, -1, 4)
    for s in range(n_steps - 8, n_steps):
        f = (s + 1) % 0x100
        assert ll_steps.ll_flag(s, cases.TEST_RULE) == f
        assert (lines[s % 8, :, 1] == f).all() and (lines[s % 8, :, 3] == f).all()
        assert not lines[s % 8, 3:, 0].any() and not lines[s % 8, 3:, 2].any()
        assert lines[s % 8, :3, 0].view(np.float32).tolist() == [0.0, 2.0, 4.0]
    assert conn.mask.all()
    # the production rule: flags are the 32-bit step + 1, steps 0x7ffffff8 .. 0x7fffffff of every 2^31 clean
    assert ll_steps.ll_flag(0xFFFFFFFF) == 0 and ll_steps.ll_flag((1 << 32) + 6) == 7
    assert [s for s in range(0x7FFFFFF0, 0x80000004) if ll_steps.ll_cleans(s)] == list(range(0x7FFFFFF8, 0x80000000))


def test_the_mask_leaves_out_only_the_padding_of_a_partial_last_line(oracle):
    conn = ll_steps.Conn(4096, 8, 2)
    data = np.arange(11, dtype=np.uint8) + 1  # one line and 3 bytes
    ll_steps.run([ll_steps.Member(data, None, [], [conn], [S(0, 0, -1, 0, 11, False, True)])], mg.U8, mg.SUM)
    undefined = np.flatnonzero(~conn.mask) - 2 * 4096
    assert undefined.tolist() == [16 + 3, 16 + 8, 16 + 9, 16 + 10, 16 + 11]  # byte 3 of word 0 and word 2 of line 1
    slot = conn.fifo[2 * 4096:3 * 4096]
    assert slot[:4].tolist() == [1, 2, 3, 4] and slot[8:12].tolist() == [5, 6, 7, 8] and slot[16:19].tolist() == [9, 10, 11]


def test_every_list_of_the_matrix_finishes(oracle):
    """A, B (at 4 KiB), D and E: the interpreter reaches the end of every list, every connection ends
    with sent == read where both ends are members, and E's hub connections clean at different pieces."""
    for dt in cases.DTYPES:
        for name, op, arg in cases.ops_for(dt):
            for n_recv, n_send in cases.PEERS:
                res, conns = _run(cases.alone_case(dt, op, arg, n_recv, n_send, 3))
                assert [c.read - c.start for c in conns[:n_recv]] == [8] * n_recv
                assert [c.sent - c.start for c in conns[n_recv:]] == [8] * n_send
            res, conns = _run(cases.star_case(dt, op, arg, 4096, cases.star_sizes(dt, 4096), 5))
            assert all(c.sent == c.read == c.start + 11 for c in conns)
    for dt, name in cases.ROUTING_PAIRS:
        _n, op, arg = cases.op_named(dt, name)
        case = cases.routing_case(dt, op, arg, 9)
        res, conns = _run(case)
        assert all(c.sent == c.read == c.start + 6 for c in conns)
        assert res.members[0].input.tobytes() != case.members[0].input.tobytes()  # round 2 wrote the input
    res, conns = _run(cases.clean_case())
    assert [[s - c.start for s in c.cleaned] for c in conns[3:]] == [list(range(8, 16)), list(range(4, 12)),
                                                                     list(range(0, 6))]
    assert [[s - c.start for s in c.cleaned] for c in conns[:3]] == [[], list(range(0, 4)), list(range(3, 11))]


def test_the_matrix_covers_every_pair_the_api_accepts(nexr):
    """Every (datatype, op) pair nexrReduceCopyLLSteps accepts — every datatype of the golden set times Sum,
    Prod, Min, Max, PreMulSum, and SumPostDiv for the integers (the argument checks refuse it for floats,
    asserted here without a GPU) — is in case A (by datatype, the ops inside, both entry points) and in
    case B (by pair), as the GPU file is parametrised."""
    import ctypes
    want = {(dt, name) for dt in mg.DT_NAMES for name in cases.OP_NAMES if name != "sumpostdiv" or dt in mg.INTS}
    assert len(want) == 56
    cs = nexr.ll_conn_set(0x10000, 0x20000, [], [], 4096)
    for dt in mg.DT_NAMES:
        for dev_op in range(5):
            rc = nexr.lib().nexrReduceCopyLLSteps(ctypes.byref(cs), None, 0, dt, dev_op, 2, None, 0, None)
            assert (rc == 0) == (dev_op != mg.SUMPOSTDIV or dt in mg.INTS), (dt, dev_op)
    names = {"sum": mg.SUM, "prod": mg.PROD, "min": mg.MINMAX, "max": mg.MINMAX, "premulsum": mg.PREMULSUM,
             "sumpostdiv": mg.SUMPOSTDIV}
    for dt in mg.DT_NAMES:
        for name, op, arg in cases.ops_for(dt):
            assert names[name] == op
            if name in ("min", "max"):
                assert arg == mg.minmax_arg(dt, name == "max")
    pytest.importorskip("torch")
    import test_ll_steps_matrix_gpu as matrix

    def params(fn, arg):
        marks = [m for m in getattr(fn, "pytestmark", []) if m.name == "parametrize" and m.args[0] == arg]
        assert len(marks) == 1, (fn.__name__, arg)
        return list(marks[0].args[1])

    a_dts = params(matrix.test_one_member_alone_every_op_and_peer_count, "dt")
    assert {(dt, name) for dt in a_dts for name, _o, _a in cases.ops_for(dt)} == want
    assert sorted(params(matrix.test_one_member_alone_every_op_and_peer_count, "how")) == ["group", "run"]
    assert {tuple(p) for p in params(matrix.test_star_in_one_group_launch, "dt,name")} == want
    assert set(cases.PEERS) == {(0, 1), (1, 0), (1, 1), (2, 1), (1, 2), (3, 0), (0, 3), (3, 3)}


def test_the_matrix_file_keeps_to_one_plain_stream_and_two_seconds():
    src = open(os.path.join(ROOT, "tests", "test_ll_steps_matrix_gpu.py")).read()
    assert "CUMask" not in src and "hipStreamCreate" not in src
    assert len(re.findall(r"torch\.cuda\.Stream\(", src)) == 1  # the module's one plain stream
    timeouts = [int(t.replace("_", "")) for t in re.findall(r"timeout_us\s*=\s*([0-9_]+)", src)]
    named = [int(t.replace("_", "")) for t in re.findall(r"^TIMEOUT_US\s*=\s*([0-9_]+)", src, re.M)]
    assert named and all(t <= 2_000_000 for t in timeouts + named)
    assert not re.findall(r"timeout_us\s*=\s*(?!TIMEOUT_US\b)[A-Za-z_]", src)  # nothing but the constant or a literal
