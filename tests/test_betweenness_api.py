"""Betweenness / edge betweenness centrality, the parts that need no GPU: the declarations in
centrality_algorithms.h, the library's exports, the Python names with the reference's parameters and
defaults, the checks that fire before any GPU call, the documented options and the twin on closed forms."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT

LIB = os.path.join(PKG, "lib", "libcugraph_c.so")
HEADER = os.path.join(ROOT, "include", "cugraph_c", "centrality_algorithms.h")
FUNCS = ["cugraph_betweenness_centrality", "cugraph_edge_betweenness_centrality",
         "cugraph_edge_centrality_result_get_src_vertices", "cugraph_edge_centrality_result_get_dst_vertices",
         "cugraph_edge_centrality_result_get_values", "cugraph_edge_centrality_result_free"]


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def arguments(text, name):
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, text)
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_header_declares_the_six_functions():
    text = header_text()
    assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*cugraph_edge_centrality_result_t\s*;", text)
    assert arguments(text, "cugraph_betweenness_centrality") == [
        "const cugraph_resource_handle_t* handle", "cugraph_graph_t* graph",
        "const cugraph_type_erased_device_array_view_t* vertex_list", "bool_t normalized",
        "bool_t include_endpoints", "bool_t do_expensive_check", "cugraph_centrality_result_t** result",
        "cugraph_error_t** error"]
    assert arguments(text, "cugraph_edge_betweenness_centrality") == [
        "const cugraph_resource_handle_t* handle", "cugraph_graph_t* graph",
        "const cugraph_type_erased_device_array_view_t* vertex_list", "bool_t normalized",
        "bool_t do_expensive_check", "cugraph_edge_centrality_result_t** result", "cugraph_error_t** error"]
    for f in FUNCS[2:]:
        assert arguments(text, f) == ["cugraph_edge_centrality_result_t* result"], f
    assert len(FUNCS) == 6


def test_header_documents_the_value_type_and_the_origin_of_the_names():
    raw = open(HEADER).read()
    assert "FLOAT64" in raw and "later cuGraph releases" in raw


def test_library_exports_the_functions():
    lib = ctypes.CDLL(LIB)
    assert [f for f in FUNCS if not hasattr(lib, f)] == []


def test_python_names_parameters_and_defaults():
    import cugraph
    import pylibcugraph
    for name in ("betweenness_centrality", "edge_betweenness_centrality"):
        assert callable(getattr(pylibcugraph, name)) and name in pylibcugraph.__all__
        assert callable(getattr(cugraph, name)) and name in cugraph.__all__
    assert list(inspect.signature(pylibcugraph.betweenness_centrality).parameters) == [
        "resource_handle", "graph", "k", "random_state", "normalized", "include_endpoints", "do_expensive_check"]
    assert list(inspect.signature(pylibcugraph.edge_betweenness_centrality).parameters) == [
        "resource_handle", "graph", "k", "random_state", "normalized", "do_expensive_check"]

    def defaults(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    E = inspect.Parameter.empty
    assert defaults(cugraph.betweenness_centrality) == [
        ("G", E), ("k", None), ("normalized", True), ("weight", None), ("endpoints", False), ("seed", None),
        ("result_dtype", np.float64)]
    assert defaults(cugraph.edge_betweenness_centrality) == [
        ("G", E), ("k", None), ("normalized", True), ("weight", None), ("seed", None), ("result_dtype", np.float64)]


def test_weight_and_result_dtype_are_checked_before_anything_else():
    import cugraph
    G = cugraph.Graph()  # no edges: the checks come first
    for f in (cugraph.betweenness_centrality, cugraph.edge_betweenness_centrality):
        with pytest.raises(NotImplementedError, match="not currently supported"):
            f(G, weight="w")
        with pytest.raises(TypeError, match="np.float32 or np.float64"):
            f(G, result_dtype=np.int32)
        with pytest.raises(TypeError, match="np.float32 or np.float64"):
            f(G, result_dtype=np.float16)


def test_options_are_documented():
    for name in (os.path.join(ROOT, "include", "cugraph_amd", "ext.h"), os.path.join(ROOT, "README.md")):
        text = open(name).read()
        assert "bc_batch" in text and "bc_row_split" in text, name


# ------------------------------------------------------------------ the twin on closed forms
def test_twin_path():
    """A path of n vertices: vertex i lies between i vertices and n - 1 - i vertices."""
    import betweenness_ref as ref
    n = 9
    p = np.arange(n - 1)
    s, d = np.r_[p, p + 1], np.r_[p + 1, p]
    i = np.arange(n, dtype=np.float64)
    assert np.array_equal(ref.betweenness(n, s, d, None, True, normalized=False), i * (n - 1 - i))
    # edge (i, i + 1) carries the (i + 1)(n - 1 - i) pairs it separates, half of it per direction and per /2
    row, col, x = ref.edge_betweenness(n, s, d, None, True, normalized=False)
    lo = np.minimum(row, col).astype(np.float64)
    assert np.array_equal(x, (lo + 1) * (n - 1 - lo) / 2)
    # with endpoints every vertex also ends the n - 1 paths to the others, counted from both ends and halved
    assert np.array_equal(ref.betweenness(n, s, d, None, True, normalized=False, endpoints=True),
                          i * (n - 1 - i) + (n - 1))


def test_twin_star_sources_and_scaling():
    import betweenness_ref as ref
    leaves = 7
    n = leaves + 1
    s, d = np.r_[np.zeros(leaves, np.int64), 1 + np.arange(leaves)], np.r_[1 + np.arange(leaves), np.zeros(leaves, np.int64)]
    full = ref.betweenness(n, s, d, None, True, normalized=True)
    assert full[0] == 1.0 and (full[1:] == 0).all()  # the hub is on every shortest path
    # from k leaf sources: each contributes (leaves - 1) to the hub; scaled by n / k
    for k in (1, 3):
        got = ref.betweenness(n, s, d, list(range(1, k + 1)), True, normalized=False)
        assert got[0] == pytest.approx(k * (leaves - 1) / 2 * n / k, rel=1e-15) and (got[1:] == 0).all()
    assert (ref.betweenness(n, s, d, [], True) == 0).all()
    # a repeated source counts again, the factor n / k follows
    assert np.allclose(ref.betweenness(n, s, d, [1, 1], True), ref.betweenness(n, s, d, [1], True), rtol=1e-15)
    # directed, not normalized: no factor at all
    assert ref.betweenness(n, s, d, [1], False, normalized=False)[0] == leaves - 1


def test_twin_parallel_edges_and_self_loops():
    import betweenness_ref as ref
    # 0 => 1 twice, 1 -> 2, loops on 1: two paths from 0 to 2, both through 1
    s, d = np.array([0, 0, 1, 1]), np.array([1, 1, 2, 1])
    assert ref.betweenness(3, s, d, None, False, normalized=False).tolist() == [0.0, 1.0, 0.0]
    row, col, x = ref.edge_betweenness(3, s, d, None, False, normalized=False)
    assert list(zip(row.tolist(), col.tolist(), x.tolist())) == [(0, 1, 1.0), (0, 1, 1.0), (1, 1, 0.0), (1, 2, 2.0)]


def test_email_golden_matches_its_dataset():
    z = np.load(os.path.join(GOLDEN, "betweenness_email_nx.npz"))
    e = np.loadtxt(os.path.join(GOLDEN, "email-Eu-core.csv"), usecols=(0, 1), dtype=np.int64)
    pairs = np.unique(e, axis=0)
    n = len(np.unique(pairs))
    for normalized in (0, 1):
        assert z[f"ebc_n{normalized}"].shape == (len(pairs),)
        for endpoints in (0, 1):
            assert z[f"bc_n{normalized}_e{endpoints}"].shape == (n,)
    # the recorded variants differ by NetworkX's own factors only
    assert np.allclose(z["bc_n1_e0"] * (n - 1) * (n - 2), z["bc_n0_e0"], rtol=1e-12)
    assert np.allclose(z["ebc_n1"] * n * (n - 1), z["ebc_n0"], rtol=1e-12)
