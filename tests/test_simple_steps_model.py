"""CPU tests of the SIMPLE step-list interpreter (tests/simple_steps_model.py): hand-worked cases, and every
step list tests/test_simple_group_gpu.py gives the device runs through it to the end."""
import numpy as np
import pytest

import make_golden as mg
import simple_steps_cases as sc
import simple_steps_model as model

S = model.Step


def _i32(*v):
    return np.array(v, dtype=np.int32)


def test_send_then_recv_reduce_copy_by_hand(oracle):
    c = model.Conn(64, 8, 0)
    m0 = model.Member(_i32(1, 2, 3, 4), None, [], [c], [S(0, 1, -1, 0, 3, False, True, False)])
    m1 = model.Member(_i32(10, 20, 30, 40), np.zeros(4, np.int32), [c], [], [S(0, 0, 1, 1, 3, True, False, False)])
    model.run([m0, m1], mg.I32, mg.SUM)
    assert m1.output.view(np.int32).tolist() == [0, 12, 23, 34]
    assert c.fifo[:12].view(np.int32).tolist() == [2, 3, 4] and c.mask[:12].all() and not c.mask[12:].any()
    assert (c.sent, c.read, c.head) == (1, 1, 1)


def test_the_user_source_is_the_first_operand_and_takes_the_pre_op(oracle):
    """PreMulSum by 3 on the INPUT only: 3 * 5 + 7 from the input, 5 + 7 from the output."""
    for src_buf, want in ((0, 22), (1, 12)):
        c = model.Conn(64, 8, 0)
        c.prefill([_i32(7)])
        mb = model.Member(_i32(5), _i32(5), [c], [], [S(src_buf, 0, 1, 0, 1, True, False, False)])
        model.run([mb], mg.I32, mg.PREMULSUM, 3)
        assert mb.output.view(np.int32).tolist() == [want]
    # min with the user source first: the result does not depend on the order, the shipped semantics do
    c = model.Conn(64, 8, 0)
    c.prefill([_i32(7)])
    mb = model.Member(_i32(5), _i32(0), [c], [], [S(0, 0, 1, 0, 1, True, False, False)])
    with oracle.semantics(2):
        model.run([mb], mg.I32, mg.SUM)
    assert mb.output.view(np.int32).tolist() == [5]   # source 0 is the user's, not the peer's


def test_two_step_slices_fill_two_slots_and_count_by_two(oracle):
    c = model.Conn(16, 8, 6, 2)
    data = np.arange(8, dtype=np.int32)
    m0 = model.Member(data, None, [], [c], [S(0, 0, -1, 0, 8, False, True, False), S(0, 0, -1, 0, 0, False, True, False)])
    m1 = model.Member(None, np.zeros(8, np.int32), [c], [], [S(-1, 0, 1, 0, 8, True, False, False),
                                                               S(-1, 0, -1, 0, 0, True, False, False)])
    model.run([m0, m1], mg.I32, mg.SUM)
    assert c.fifo[6 * 16:8 * 16].view(np.int32).tolist() == list(range(8))   # slots 6 and 7
    assert int(c.mask.sum()) == 32 and (c.sent, c.read, c.head) == (10, 10, 10)
    assert m1.output.view(np.int32).tolist() == list(range(8))
    with pytest.raises(AssertionError):
        model.Conn(16, 8, 7, 2)            # a 2-step slice at step 7 would wrap
    with pytest.raises(AssertionError):
        model.Conn(16, 6, 0, 4)            # nSlots % stepPerSlice


def test_credits_and_deadlock(oracle):
    x = np.zeros(4, np.int32)
    c = model.Conn(16, 8, 0, 2)
    sends = [S(0, 0, -1, 0, 4, False, True, False)] * 5      # the fifth 2-step slice has no credit
    with pytest.raises(model.StuckError):
        model.run([model.Member(x, None, [], [c], sends), model.Member(None, x.copy(), [c], [], [])], mg.I32, mg.SUM)
    c = model.Conn(16, 8, 0, 2)
    model.run([model.Member(x, None, [], [c], sends)], mg.I32, mg.SUM)   # one-ended: the receiver is elsewhere
    assert c.sent == 10
    c = model.Conn(16, 8, 0)
    with pytest.raises(model.StuckError):   # a tail that never comes
        model.run([model.Member(None, x.copy(), [c], [], [S(-1, 0, 1, 0, 4, True, False, False)])], mg.I32, mg.SUM)
    with pytest.raises(AssertionError):
        c.prefill([x] * 9)


@pytest.mark.parametrize("ix", range(len(sc.all_cases())))
def test_every_gpu_step_list_runs_to_the_end(oracle, ix):
    case = sc.all_cases()[ix]
    members, conns = model.model(case.case, case.step_per_slice)
    res = model.run(members, case.case.dt, case.case.op, case.case.arg)
    assert len(res.trace) == sum(len(m.steps) for m in case.case.members)
    for c in conns:
        assert c.sent % case.step_per_slice == 0 and c.read <= c.sent
    for i, c in enumerate(conns):   # internal connections are drained
        if any(i in m.recv for m in case.case.members):
            assert c.read == c.sent == c.head, case.what


def test_the_case_list_covers_every_pair_the_api_accepts():
    import ll_steps_cases as cases
    assert len(cases.STAR_PAIRS) == 56
    whats = [c.what for c in sc.all_cases()]
    assert len(whats) == len(set(whats))
    assert sum(w.startswith("fan ") for w in whats) == 56
    for sps in (1, 2):
        case = sc.pair_case(sps)
        sizes = [s.n_elts for s in case.case.members[0].steps]
        assert len(sizes) == 40 and 40 * sps // 8 >= 3                       # at least three wraps
        assert sorted(set(sizes)) == sorted({case.case.slot_bytes * sps // 4, 3, 0, 1025})
