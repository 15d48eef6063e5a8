"""The plain-C client of the core number / k-core entry points (tests/c/core_test.c): compiled
with gcc against include/cugraph_c/*.h and linked to libcugraph_c.so, then run on the GPU.  It
re-authors the reference's cpp/tests/c_api/core_number_test.c and the disabled branch of
k_core_test.c."""
import os
import subprocess

import pytest

from conftest import PKG, ROOT

SRC = os.path.join(ROOT, "tests", "c", "core_test.c")
BIN = os.path.join(ROOT, "tests", "c", "core_test")
LIBDIR = os.path.join(PKG, "lib")


def test_c_client_compiles_and_links(tmp_path):
    out = tmp_path / "core_test"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(out), SRC, "-L", LIBDIR, "-lcugraph_c", f"-Wl,-rpath,{LIBDIR}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_c_client_runs():
    assert os.path.exists(BIN), "tests/c/core_test not built (make -C cugraph-forked_amd)"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("core_number", "k_core", "core_errors"):
        assert f"PASS {name}" in r.stdout
