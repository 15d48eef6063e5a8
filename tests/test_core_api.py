"""Core number / k-core, the parts that need no GPU: the declarations in core_algorithms.h,
the library's exports, the Python names, the directed-graph errors of cores/core_number.py:74
and cores/k_core.py:87 (which fire before any GPU call) and the golden file's consistency."""
import ctypes
import json
import os
import re

import pytest

from conftest import GOLDEN, PKG, ROOT

LIB = os.path.join(PKG, "lib", "libcugraph_c.so")
HEADER = os.path.join(ROOT, "include", "cugraph_c", "core_algorithms.h")
FUNCS = ["cugraph_core_result_create", "cugraph_core_result_get_vertices", "cugraph_core_result_get_core_numbers",
         "cugraph_core_result_free", "cugraph_k_core_result_get_src_vertices",
         "cugraph_k_core_result_get_dst_vertices", "cugraph_k_core_result_get_weights",
         "cugraph_k_core_result_free", "cugraph_core_number", "cugraph_k_core"]


def header_text(name=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(name).read(), flags=re.S)


def test_header_declares_the_types_and_functions():
    text = header_text()
    for t in ("cugraph_core_result_t", "cugraph_k_core_result_t"):
        assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*%s\s*;" % t, text), t
    m = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*cugraph_k_core_degree_type_t\s*;", text)
    assert m
    values = dict(re.findall(r"(K_CORE_DEGREE_TYPE_\w+)\s*=\s*(\d+)", m.group(1)))
    assert values == {"K_CORE_DEGREE_TYPE_IN": "0", "K_CORE_DEGREE_TYPE_OUT": "1", "K_CORE_DEGREE_TYPE_INOUT": "2"}
    assert len(FUNCS) == 10
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, text), f


def test_umbrella_header_includes_it():
    assert "<cugraph_c/core_algorithms.h>" in open(os.path.join(ROOT, "include", "cugraph_c", "algorithms.h")).read()


def test_library_exports_the_functions():
    lib = ctypes.CDLL(LIB)
    assert [f for f in FUNCS if not hasattr(lib, f)] == []


def test_python_names():
    import cugraph
    import pylibcugraph
    for name in ("core_number", "k_core"):
        assert callable(getattr(pylibcugraph, name)) and name in pylibcugraph.__all__
        assert callable(getattr(cugraph, name)) and name in cugraph.__all__


def test_core_scan_is_documented():
    assert "core_scan" in open(os.path.join(ROOT, "include", "cugraph_amd", "ext.h")).read()


def test_directed_graph_is_refused():
    import cugraph
    with pytest.raises(ValueError, match="input graph must be undirected"):
        cugraph.core_number(cugraph.Graph(directed=True))
    with pytest.raises(ValueError, match="input graph must be undirected"):
        cugraph.core_number(cugraph.DiGraph())
    with pytest.raises(ValueError, match="G must be an undirected Graph instance"):
        cugraph.k_core(cugraph.Graph(directed=True))
    with pytest.raises(ValueError, match="G must be an undirected Graph instance"):
        cugraph.k_core(cugraph.DiGraph(), k=2)


def test_golden_vectors_are_consistent():
    with open(os.path.join(GOLDEN, "core_vectors.json")) as f:
        v = json.load(f)
    small = v["small"]
    n = small["num_vertices"]
    assert len(small["src"]) == len(small["dst"]) == len(small["weights"]) == small["num_edges"] == 22
    pairs = sorted(zip(small["src"], small["dst"]))
    assert pairs == sorted(zip(small["dst"], small["src"]))  # symmetric
    assert len(set(pairs)) == len(pairs) and all(a != b for a, b in pairs)
    assert len(small["core_numbers"]) == n and max(max(small["src"]), max(small["dst"])) == n - 1
    core, k = small["core_numbers"], small["k"]
    want = sorted((a, b) for a, b in pairs if core[a] >= k and core[b] >= k)
    assert sorted(zip(small["k_core_src"], small["k_core_dst"])) == want and len(want) == 12
    # the core numbers themselves, by the definition: peel the smallest remaining degree
    adj = {i: {b for a, b in pairs if a == i} for i in range(n)}
    left, level, got = set(range(n)), 0, {}
    while left:
        u = min(left, key=lambda x: len(adj[x] & left))
        level = max(level, len(adj[u] & left))
        got[u] = level
        left.remove(u)
    assert [got[i] for i in range(n)] == core
    for name, facts in v["datasets"].items():
        if name != "comment":
            assert os.path.exists(os.path.join(GOLDEN, name)), name
            assert set(facts) == {"vertices", "largest_core", "in_largest_core", "sum"}
