"""The SSSP threshold step (csrc/sssp_threshold.hpp) as a host program: compiled with
the host compiler alone and run on the CPU (tests/c/sssp_threshold_test.cpp sweeps
fp32 and fp64 values, the absorbed-delta cases among them)."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "c", "sssp_threshold_test.cpp")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_threshold_always_advances(tmp_path):
    out = tmp_path / "sssp_threshold_test"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I",
                        os.path.join(PKG, "csrc"), "-o", str(out), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS threshold" in r.stdout
