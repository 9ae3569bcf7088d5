"""The round calls' launch planner (freddie_amd/csrc/clu_plan.h) without a GPU: tools/plan_host_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a child process, plans hand-built orders -- an empty one, a problem smaller than a workgroup, one
across several launches, the launch counts the GPU tests assert, budgets that end the taking on the first, a middle and no problem, a unit
cost of 1 against the enumeration's running-total test, budgets and unit costs near 2^62 -- and checks every plan itself."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_planner_under_sanitizers(tmp_path):
    exe = str(tmp_path / "plan_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "freddie_amd", "csrc"), os.path.join(ROOT, "tools", "plan_host_check.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout[-2000:], res.stderr[-4000:])
    checks, failed = (int(w) for w in res.stdout.splitlines()[-1].split() if w.isdigit())
    assert failed == 0 and checks > 4000
