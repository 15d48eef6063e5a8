"""The sorted-row intersection (csrc/intersect.hpp) as a host program: the thread merge,
one lane's probe and sim_seg_len compiled with the host compiler alone, against csrc/
only, and run on the CPU (tests/c/intersect_test.cpp: sorted rows with repeated ids,
int32 and int64, lengths around the wave cut and the LDS stage, cuts inside runs)."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "c", "intersect_test.cpp")


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_merge_probe_and_segments_agree(tmp_path):
    out = tmp_path / "intersect_test"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        "-o", str(out), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS intersect" in r.stdout
