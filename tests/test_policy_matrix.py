"""The plan of tests/policy_matrix_worker.py, without a GPU: under each cache policy (NEXR_POLICY is read
once per process, hence a child per policy) the worker's `--plan` mode builds every call it would make and
asks nexrQueryLaunch (no device call) for each one's policy and workgroup shape. The plan must launch every
compiled single kernel of that policy, every batch kernel of policies 0 and 1, and every workgroup shape
the policy selects; and it must hold as many calls as its parameters say. These are conditions on the
inputs of tests/test_policy_matrix_gpu.py, not measurements."""
import json
import os
import subprocess
import sys

import pytest

import make_golden as mg
import policy_matrix_worker as worker
from test_code_objects import expected_kernels

HERE = os.path.dirname(os.path.abspath(__file__))
WORKER = os.path.join(HERE, "policy_matrix_worker.py")

SHAPES = {0: {(256, 4), (1024, 1)},
          1: {(256, 4), (512, 2), (1024, 1)},
          3: {(256, 4), (1024, 1), (512, 1)}}


def run_plan(policy, datatypes=("all",), mode="matrix", grid=None):
    """The report of `--plan` for these datatypes under this policy (a CPU-only child)."""
    env = dict(os.environ, NEXR_POLICY=str(policy))
    env.pop("NEXR_GRID", None)
    if grid:
        env["NEXR_GRID"] = str(grid)
    p = subprocess.run([sys.executable, WORKER, "--plan", "--mode", mode, *datatypes], capture_output=True, text=True,
                       timeout=120, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def keys(report, which):
    return {tuple(k) for k in report[which]}


@pytest.mark.parametrize("policy", [0, 1, 3])
def test_the_plan_launches_every_compiled_kernel_of_the_policy(policy):
    r = run_plan(policy)
    assert r["policy"] == policy and r["plan"] is True
    want_single = {(dt, op, k, is_min) for (batch, dt, op, k, pol, is_min) in expected_kernels()
                   if batch == 0 and pol == policy}
    assert len(want_single) == 319
    got = keys(r, "single")
    assert got == want_single, (sorted(got - want_single)[:5], sorted(want_single - got)[:5])
    if policy in (0, 1):
        want_batch = {(dt, op, k, is_min) for (batch, dt, op, k, pol, is_min) in expected_kernels()
                      if batch == 1 and pol == policy}
        assert len(want_batch) == 319
        got = keys(r, "batch")
        assert got == want_batch, (sorted(got - want_batch)[:5], sorted(want_batch - got)[:5])
    else:  # no batch kernels under nt stores: the host runs the works as single launches
        assert r["batch"] == []
    assert {tuple(s) for s in r["shapes"]} == SHAPES[policy]
    # datatypes x ops x K x (four layouts + the batch + its three works alone + in place) + the legs
    n_ops = {dt: 6 if dt in mg.INTS else 5 for dt in mg.DT_NAMES}
    count = sum(n_ops[dt] * 8 * (4 + 1 + 3 + 1) for dt in mg.DT_NAMES)
    count += 3 * (2 * 4 * 2)  # fp16, bf16, int8: pairs and fold8 x four ops x two parities
    count += 4                # fp32, fp16, bf16, fp64: the one-rank pointer scalar
    assert r["calls"] == count == worker.planned_calls(sorted(mg.DT_NAMES), "matrix")


@pytest.mark.parametrize("policy", [1, 3])
def test_the_strided_plan_covers_every_shape_of_the_policy(policy):
    r = run_plan(policy, mode="grid", grid=2)
    assert r["grid"] == 2 and r["calls"] == 10 * 2 * 4 == worker.planned_calls(sorted(mg.DT_NAMES), "grid")
    assert {tuple(s) for s in r["shapes"]} == SHAPES[policy]
    assert r["batch"] == []
    # sum and max at K = 2, 4, 5, 8: Sum on the seven unsigned and float types, Max on all ten
    assert len(keys(r, "single")) == (7 + 10) * 4
