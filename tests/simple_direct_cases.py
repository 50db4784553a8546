"""TEST INFRASTRUCTURE (a helper, not a test module): the direct all-reduce cases of
tests/test_simple_direct_gpu.py as data, so that tests/test_simple_direct_model.py can run every list through the
direct interpreter (tests/simple_direct_model.py) without a GPU. Nothing here touches the GPU or the library
under test."""
import numpy as np

import ll_steps_cases as cases
import make_golden as mg
import simple_direct_model as dm

PATTERN = 0xA5  # what every FIFO byte holds before the call


class DCase:
    """Members (dm.DMember, made by `build`, fresh for every run), their connections, and how to run them."""

    def __init__(self, what, dt, op, arg, slot, sps, build, misalign=0):
        self.what, self.dt, self.op, self.arg, self.slot, self.sps, self.misalign = what, dt, op, arg, slot, sps, misalign
        self.members, self.conns = build()
        for c in self.conns:
            c.fifo[:] = PATTERN


def blank(n, dt):
    return np.full(n * cases.esz_of(dt), cases.FILL, dtype=np.uint8).view(mg.STORE[dt])


def all_reduce_case(dt=mg.F32, name="sum", slot=4096, sps=1, spc=1, loops=20, tail=None, misalign=0, n=2, seed=61,
                    direct=True):
    """The n-member direct all-reduce: `loops` full loops (2 send slices a connection and loop at n = 2) and a
    last loop of `tail` elements. direct=False: the same schedule through the FIFOs."""
    _n, op, arg = cases.op_named(dt, name)
    esz = cases.esz_of(dt)
    step = slot // esz
    tail = (16 * 1024 + 5 + esz - 1) // esz + 3 if tail is None else tail
    count = loops * n * step * sps * spc + tail
    xs = mg.gen_inputs(dt, n, count, seed + dt, special=True)

    def build():
        lists = dm.all_reduce_lists(n, count, esz, step, sps, spc, direct)
        return dm.ring_members(lists, xs, [blank(count, dt) for _ in range(n)], slot, sps, start=6 * sps, direct=direct)
    return DCase(f"all-reduce {mg.DT_NAMES[dt]} {name} slot={slot} sps={sps}", dt, op, arg, slot, sps, build, misalign)


def types_and_ops_case(dt, name, direct=True):
    """test_all_reduce_types_and_ops' case of one (datatype, op name) of ll_steps_cases.STAR_PAIRS."""
    return all_reduce_case(dt, name, loops=3, n=3, direct=direct)
