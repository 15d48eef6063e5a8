"""The plain-C client of the sampling entry points (tests/c/sampling_test.c): compiled with gcc against
include/cugraph_c/*.h and linked to libcugraph_c.so (tests/test_sampling_api.py checks that without a
GPU), then run on the GPU.  It runs the two cases of the reference's
cpp/tests/c_api/uniform_neighbor_sample_test.c and one uniform random walk."""
import os
import subprocess

import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "tests", "c", "sampling_test")


@pytest.mark.gpu
def test_c_client_runs():
    assert os.path.exists(BIN), "tests/c/sampling_test not built (make -C cugraph-forked_amd)"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("sample", "sample_all_neighbors", "uniform_walk"):
        assert f"PASS {name}" in r.stdout
