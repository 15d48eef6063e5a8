"""The plain-C client of the vertex pair, similarity and two-hop entry points
(tests/c/similarity_test.c): compiled with gcc against include/cugraph_c/*.h and linked to
libcugraph_c.so (tests/test_similarity_api.py checks that without a GPU), then run on the GPU.
It re-authors the reference's cpp/tests/c_api/similarity_test.c with the expected values that
file leaves as TODO."""
import os
import subprocess

import pytest

from conftest import ROOT

BIN = os.path.join(ROOT, "tests", "c", "similarity_test")


@pytest.mark.gpu
def test_c_client_runs():
    assert os.path.exists(BIN), "tests/c/similarity_test not built (make -C cugraph-forked_amd)"
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    for name in ("jaccard", "sorensen", "overlap", "two_hop", "similarity_errors"):
        assert f"PASS {name}" in r.stdout
