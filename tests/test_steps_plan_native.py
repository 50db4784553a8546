"""The pure half of the step-list planner (nex-nccl_amd/csrc/nexr_steps_plan.h: the launch cuts and the dry run)
under AddressSanitizer + UndefinedBehaviorSanitizer on the CPU: tests/native/steps_plan.cpp includes the header,
which calls nothing from HIP, so no HIP library is linked. It walks the cut rules (96 and 97 steps, unequal
members, user-range conflicts, cleaning steps under the test rule, a SIMPLE direct receive), rings of two and
eight members, groups the dry run refuses, and the most members with three peers each."""
import os
import subprocess

from conftest import ROOT

HIP_INC = "/opt/rocm/include"


def test_steps_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "steps_plan"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-D__HIP_PLATFORM_AMD__", f"-I{HIP_INC}", os.path.join(ROOT, "tests", "native", "steps_plan.cpp"),
           "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "steps_plan failures=0" in p.stdout
