"""The position-reporting forms of the sorted-row intersection (csrc/intersect.hpp isect_merge_at,
isect_probe_at) as a host program: compiled with the host compiler alone, against csrc/ only, and run
on the CPU (tests/c/intersect_at_test.cpp: a brute-force model, sorted rows with repeated ids, int32
and int64, lengths around the wave cut, the split segment and the LDS stage, cuts inside runs).  The
second build runs the same program under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "c", "intersect_at_test.cpp")


def build_and_run(tmp_path, name, extra):
    out = tmp_path / name
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I",
                        os.path.join(PKG, "csrc"), "-o", str(out), SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS intersect_at" in r.stdout


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_positions_agree_with_the_model(tmp_path):
    build_and_run(tmp_path, "intersect_at_test", [])


@pytest.mark.skipif(not shutil.which("g++"), reason="no g++")
def test_positions_agree_with_the_model_under_sanitizers(tmp_path):
    build_and_run(tmp_path, "intersect_at_test_san",
                  ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
