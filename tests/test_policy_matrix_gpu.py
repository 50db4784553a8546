"""Every compiled reduce-copy kernel under each cache policy, on the GPU: one child process of
tests/policy_matrix_worker.py per (policy, datatype), NEXR_POLICY forcing the policy at sizes of one to five
trips (8-80 KiB per buffer) where the size alone would pick policy 0. Policies 1 (non-temporal loads) and 3
(non-temporal loads and stores) are the kernels the full-size configurations and the benchmark run; policy 0
is the control: the same worker against kernels the rest of the suite already covers, so a failure there is
the worker's. Every item is bit-exact against the oracle with guard bytes around every destination, and
launches exactly the kernels and as many calls as the worker's plan holds (tests/test_policy_matrix.py pins
that plan to all 319 single kernels per policy and all 319 batch kernels of policies 0 and 1). One further
item per nt policy runs every datatype with NEXR_GRID=2, so that each workgroup strides over two or three
full trips of every shape, from a misaligned start.

A child that ends on a signal or at its time limit may have faulted the device: every later item then fails
at once without starting another child."""
import json
import os
import subprocess
import sys

import pytest

import make_golden as mg
from test_policy_matrix import WORKER, run_plan

pytestmark = pytest.mark.gpu

_lost = []  # the item whose child was lost, if any


def run_child(policy, datatypes, mode="matrix", grid=None):
    if _lost:
        pytest.fail("not started: the child of %s was lost earlier in this module" % _lost[0])
    what = "policy %s %s %s" % (policy, mode, " ".join(datatypes))
    env = dict(os.environ, NEXR_POLICY=str(policy))
    env.pop("NEXR_GRID", None)
    if grid:
        env["NEXR_GRID"] = str(grid)
    try:
        p = subprocess.run([sys.executable, WORKER, "--mode", mode, *datatypes], capture_output=True, text=True,
                           timeout=120, env=env)
    except subprocess.TimeoutExpired as e:
        _lost.append(what)
        out, err = (x.decode(errors="replace") if isinstance(x, bytes) else (x or "") for x in (e.stdout, e.stderr))
        print(out[-2000:], err[-2000:])
        pytest.fail("the child of %s did not end within 120 s" % what)
    if p.returncode < 0:
        _lost.append(what)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0, (what, p.returncode, p.stdout[-2000:] + p.stderr[-2000:])
    report = json.loads(p.stdout.strip().splitlines()[-1])
    want = run_plan(policy, datatypes, mode, grid)
    assert report["plan"] is False and report["policy"] == policy
    for field in ("calls", "single", "batch", "shapes", "datatypes", "grid"):
        assert report[field] == want[field], (what, field)
    return report


@pytest.mark.parametrize("dt", sorted(mg.DT_NAMES), ids=lambda dt: mg.DT_NAMES[dt])
@pytest.mark.parametrize("policy", [0, 1, 3])
def test_every_kernel_of_the_datatype_under_the_policy(policy, dt):
    r = run_child(policy, [mg.DT_NAMES[dt]])
    assert r["calls"] > 0 and r["single"]


@pytest.mark.parametrize("policy", [1, 3])
def test_strided_trips_of_every_shape_from_a_misaligned_start(policy):
    r = run_child(policy, ["all"], mode="grid", grid=2)
    assert r["calls"] == 80
