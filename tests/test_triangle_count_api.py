"""Triangle counting, the parts that need no GPU: the declarations in
community_algorithms.h, the library's exports, the Python names and the argument
errors of community/triangle_count.py:61-73, which fire before any GPU call."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT

LIB = os.path.join(PKG, "lib", "libcugraph_c.so")
HEADER = os.path.join(ROOT, "include", "cugraph_c", "community_algorithms.h")
FUNCS = ["cugraph_triangle_count", "cugraph_triangle_count_result_get_vertices",
         "cugraph_triangle_count_result_get_counts", "cugraph_triangle_count_result_free"]


def test_header_declares_the_five_names():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*cugraph_triangle_count_result_t\s*;", text)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, text), f


def test_library_exports_the_functions():
    lib = ctypes.CDLL(LIB)
    assert [f for f in FUNCS if not hasattr(lib, f)] == []


def test_python_names():
    import cugraph
    import pylibcugraph
    assert callable(pylibcugraph.triangle_count) and "triangle_count" in pylibcugraph.__all__
    assert callable(cugraph.triangle_count) and "triangle_count" in cugraph.__all__


def test_directed_graph_is_refused():
    import cugraph
    with pytest.raises(ValueError, match="input graph must be undirected"):
        cugraph.triangle_count(cugraph.Graph(directed=True))
    with pytest.raises(ValueError, match="input graph must be undirected"):
        cugraph.triangle_count(cugraph.DiGraph(), [0])


@pytest.mark.parametrize("start", [np.array([0, 1]), (0, 1), "0", 1.5, {0: 1}])
def test_bad_start_list_type(start):
    import cugraph
    G = cugraph.Graph()  # no edge list: the check must fire before anything touches it
    with pytest.raises(TypeError, match="'start_list' must be either a list or a cudf.Series"):
        cugraph.triangle_count(G, start)


def test_golden_vectors_are_consistent():
    with open(os.path.join(GOLDEN, "triangle_count_vectors.json")) as f:
        v = json.load(f)
    small = v["small"]
    assert len(small["src"]) == len(small["dst"]) == small["num_edges"]
    assert sorted(zip(small["src"], small["dst"])) == sorted(zip(small["dst"], small["src"]))  # symmetric
    assert [small["all_counts"][i] for i in small["start"]] == small["result"]
    edges = np.loadtxt(os.path.join(GOLDEN, v["dolphins"]["edges"]), usecols=(0, 1), dtype=np.int64)
    assert len(edges) == v["dolphins"]["num_edges"] and edges.max() + 1 == v["dolphins"]["num_vertices"]
