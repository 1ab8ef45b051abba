"""The host-only batch planning of coral_segment_coverage_host (coral_amd/csrc/coral_query_plan.h), without a device:
tests/native/query_plan_host.cpp compiled as a plain program and run."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_query_plan_host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH: the planning header cannot be checked")
    exe = str(tmp_path / "query_plan_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "query_plan_host.cpp"), "-o", exe],
                   check=True, cwd=ROOT)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "query plan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
