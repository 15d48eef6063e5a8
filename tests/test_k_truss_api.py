"""k-truss, the parts that need no GPU: the declarations in community_algorithms.h and
graph_functions.h, the library's exports, the Python names, the errors that fire before any GPU call,
and the CPU twin (tests/k_truss_ref.py) against networkx.k_truss and the recorded facts of
tests/golden/k_truss_vectors.json (scripts/make_k_truss_golden.py)."""
import ctypes
import functools
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT, dataset_path
from k_truss_ref import k_truss, simple_edges

LIB = os.path.join(PKG, "lib", "libcugraph_c.so")
HEADERS = [os.path.join(ROOT, "include", "cugraph_c", n) for n in ("community_algorithms.h", "graph_functions.h")]
FUNCS = ["cugraph_induced_subgraph_get_sources", "cugraph_induced_subgraph_get_destinations",
         "cugraph_induced_subgraph_get_edge_weights", "cugraph_induced_subgraph_get_subgraph_offsets",
         "cugraph_induced_subgraph_result_free", "cugraph_k_truss_subgraph"]
DATASETS = ["karate.csv", "dolphins.csv", "polbooks.csv", "netscience.csv", "email-Eu-core.csv"]


def header_text():
    return "\n".join(re.sub(r"/\*.*?\*/", "", open(name).read(), flags=re.S) for name in HEADERS)


def test_header_declares_the_type_and_functions():
    text = header_text()
    assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*cugraph_induced_subgraph_result_t\s*;", text)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, text), f
    m = re.search(r"cugraph_k_truss_subgraph\s*\(([^)]*)\)", text)
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const cugraph_resource_handle_t* handle", "cugraph_graph_t* graph", "size_t k",
                    "bool_t do_expensive_check", "cugraph_induced_subgraph_result_t** result",
                    "cugraph_error_t** error"]


def test_library_exports_the_functions():
    lib = ctypes.CDLL(LIB)
    assert [f for f in FUNCS if not hasattr(lib, f)] == []


def test_python_names():
    import cugraph
    import pylibcugraph
    assert callable(pylibcugraph.k_truss_subgraph) and "k_truss_subgraph" in pylibcugraph.__all__
    for name in ("ktruss_subgraph", "k_truss"):
        assert callable(getattr(cugraph, name)) and name in cugraph.__all__


def test_kt_path_is_documented():
    assert "kt_path" in open(os.path.join(ROOT, "include", "cugraph_amd", "ext.h")).read()


def test_directed_graph_and_bad_k_are_refused():
    import cugraph
    import networkx as nx
    for G in (cugraph.Graph(directed=True), cugraph.DiGraph(), nx.DiGraph([(0, 1)])):
        with pytest.raises(ValueError, match="input graph must be undirected"):
            cugraph.k_truss(G, 3)
    for G in (cugraph.Graph(directed=True), cugraph.DiGraph()):
        with pytest.raises(ValueError, match="input graph must be undirected"):
            cugraph.ktruss_subgraph(G, 3)
    # an undirected graph without edges: k is checked before the graph is touched
    for k in (-1, 2.5, "3", None, True):
        with pytest.raises(ValueError, match="non-negative integer"):
            cugraph.ktruss_subgraph(cugraph.Graph(), k)
        with pytest.raises(ValueError, match="non-negative integer"):
            cugraph.k_truss(cugraph.Graph(), k)
        with pytest.raises(ValueError, match="non-negative integer"):
            cugraph.k_truss(nx.Graph([(0, 1)]), k)


# ------------------------------------------------------------------ the twin
@functools.lru_cache(maxsize=None)
def dataset(name):
    data = np.loadtxt(dataset_path(name), dtype=np.float64, ndmin=2)
    return data[:, 0].astype(np.int64), data[:, 1].astype(np.int64)


def nx_truss(s, d, k):
    import networkx as nx
    G = nx.Graph()
    G.add_edges_from((a, b) for a, b in zip(s.tolist(), d.tolist()) if a != b)
    return sorted((min(u, v), max(u, v)) for u, v in nx.k_truss(G, k).edges())


@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(GOLDEN, "k_truss_vectors.json")) as f:
        return json.load(f)["datasets"]


@pytest.mark.parametrize("name", DATASETS)
def test_twin_equals_networkx(name):
    s, d = dataset(name)
    for k in range(3, 9):
        edges, _ = k_truss(s, d, k)
        assert [tuple(e) for e in edges.tolist()] == nx_truss(s, d, k), k


def test_twin_equals_networkx_on_a_long_cascade():
    import networkx as nx
    G = nx.gnp_random_graph(300, 0.08, seed=1)
    s, d = np.array(G.edges(), np.int64).T
    edges, rounds = k_truss(s, d, 4)
    assert [tuple(e) for e in edges.tolist()] == nx_truss(s, d, 4)
    assert rounds >= 10


@pytest.mark.parametrize("name", DATASETS)
def test_twin_reproduces_the_recorded_facts(name):
    s, d = dataset(name)
    facts = vectors()[name]
    assert sorted(facts) == ["3", "4", "5", "6", "8"]
    for k, want in facts.items():
        edges, rounds = k_truss(s, d, int(k))
        assert (len(edges), rounds) == (want["edges"], want["rounds"]), k
        if "edge_list" in want:
            assert edges.tolist() == want["edge_list"]


def test_recorded_facts_hold_the_published_numbers():
    v = vectors()
    assert [v["karate.csv"][k]["edges"] for k in "3456"] == [67, 25, 14, 0]
    assert len(v["karate.csv"]["4"]["edge_list"]) == 25 and len(v["karate.csv"]["5"]["edge_list"]) == 14
    assert (v["polbooks.csv"]["5"], v["polbooks.csv"]["6"]) == ({"edges": 233, "rounds": 5}, {"edges": 72, "rounds": 5})
    assert v["email-Eu-core.csv"]["5"] == {"edges": 14771, "rounds": 8}
    assert v["email-Eu-core.csv"]["8"] == {"edges": 12712, "rounds": 12}


def test_twin_on_closed_forms():
    # the diamond: the four outer edges go first, the spine after them
    s, d = np.array([0, 0, 0, 1, 1]), np.array([1, 2, 3, 2, 3])
    assert k_truss(s, d, 3)[0].tolist() == simple_edges(s, d).tolist() and k_truss(s, d, 3)[1] == 0
    edges, rounds = k_truss(s, d, 4)
    assert len(edges) == 0 and rounds == 2
    # K5: whole at k = 5, gone in one round at k = 6; loops and repeats do not count
    s, d = np.array([(a, b) for a in range(5) for b in range(5)]).T
    assert len(simple_edges(s, d)) == 10
    assert len(k_truss(s, d, 5)[0]) == 10 and k_truss(s, d, 6) [1] == 1 and len(k_truss(s, d, 6)[0]) == 0
