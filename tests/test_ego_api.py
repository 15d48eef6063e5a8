"""Induced subgraphs and ego nets, the parts that need no GPU: the declarations in graph_functions.h and
community_algorithms.h, the library's exports, the Python names, the options' documentation, the errors
that fire before any GPU call, the host arithmetic of the packed keys (tests/c/ego_keys_test.cpp over
csrc/subgraph_keys.hpp), and the CPU twin (tests/ego_ref.py) against networkx.ego_graph / G.subgraph and
the recorded facts of tests/golden/ego_vectors.json (scripts/make_ego_golden.py)."""
import ctypes
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT, dataset_path
from ego_ref import Rows, batched, batched_ego, ego_graph, ego_vertices, induced_subgraph, sorted_edges

LIB = os.path.join(PKG, "lib", "libcugraph_c.so")
INCLUDE = os.path.join(ROOT, "include", "cugraph_c")
DATASETS = {"karate.csv": False, "dolphins.csv": False, "polbooks.csv": False, "netscience.csv": False,
            "email-Eu-core.csv": False, "karate-asymmetric.csv": True}


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def arguments(text, func):
    m = re.search(r"\b%s\s*\(([^)]*)\)" % func, text)
    assert m, func
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_headers_declare_the_functions():
    assert arguments(header_text("graph_functions.h"), "cugraph_extract_induced_subgraph") == [
        "const cugraph_resource_handle_t* handle", "cugraph_graph_t* graph",
        "const cugraph_type_erased_device_array_view_t* subgraph_offsets",
        "const cugraph_type_erased_device_array_view_t* subgraph_vertices", "bool_t do_expensive_check",
        "cugraph_induced_subgraph_result_t** result", "cugraph_error_t** error"]
    assert arguments(header_text("community_algorithms.h"), "cugraph_extract_ego") == [
        "const cugraph_resource_handle_t* handle", "cugraph_graph_t* graph",
        "const cugraph_type_erased_device_array_view_t* source_vertices", "size_t radius",
        "bool_t do_expensive_check", "cugraph_induced_subgraph_result_t** result", "cugraph_error_t** error"]
    for text, func in ((header_text("graph_functions.h"), "cugraph_extract_induced_subgraph"),
                       (header_text("community_algorithms.h"), "cugraph_extract_ego")):
        assert re.search(r"cugraph_error_code_t\s+%s\s*\(" % func, text)


def test_library_exports_the_functions():
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "cugraph_extract_induced_subgraph") and hasattr(lib, "cugraph_extract_ego")


def test_python_names():
    import cugraph
    import pylibcugraph
    for name in ("induced_subgraph", "ego_graph"):
        assert callable(getattr(pylibcugraph, name)) and name in pylibcugraph.__all__
    for name in ("subgraph", "ego_graph", "batched_ego_graphs"):
        assert callable(getattr(cugraph, name)) and name in cugraph.__all__


def test_python_signatures():
    import inspect
    import cugraph
    import pylibcugraph
    assert list(inspect.signature(pylibcugraph.induced_subgraph).parameters) == [
        "resource_handle", "graph", "subgraph_vertices", "subgraph_offsets", "do_expensive_check"]
    assert list(inspect.signature(pylibcugraph.ego_graph).parameters) == [
        "resource_handle", "graph", "source_vertices", "radius", "do_expensive_check"]
    assert str(inspect.signature(cugraph.subgraph)) == "(G, vertices)"
    assert str(inspect.signature(cugraph.ego_graph)) == \
        "(G, n, radius=1, center=True, undirected=False, distance=None)"
    assert str(inspect.signature(cugraph.batched_ego_graphs)) == \
        "(G, seeds, radius=1, center=True, undirected=False, distance=None)"


def test_options_are_documented():
    ext = open(os.path.join(ROOT, "include", "cugraph_amd", "ext.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    for name in ("sg_path", "sg_split_min", "ego_budget"):
        assert name in ext and name in readme, name


def test_argument_errors_fire_before_any_gpu_call():
    import cugraph
    import networkx as nx
    import pylibcugraph
    # graphs without a device graph behind them: any GPU call would fail differently
    graphs = (cugraph.Graph(), cugraph.Graph(directed=True), nx.path_graph(3))
    for G in graphs:
        for radius in (-1, 2.5, "1", None, True, False):
            with pytest.raises(ValueError, match="non-negative integer"):
                cugraph.ego_graph(G, 0, radius=radius)
            with pytest.raises(ValueError, match="non-negative integer"):
                cugraph.batched_ego_graphs(G, [0], radius=radius)
        for kw in ({"center": False}, {"undirected": True}, {"distance": "weight"}):
            with pytest.raises(NotImplementedError, match="not supported"):
                cugraph.ego_graph(G, 0, **kw)
            with pytest.raises(NotImplementedError, match="not supported"):
                cugraph.batched_ego_graphs(G, [0], **kw)
    for radius in (-1, 2.5, True):
        with pytest.raises(ValueError, match="non-negative integer"):
            pylibcugraph.ego_graph(None, None, None, radius, False)
    # a graph without edges: empty lists are allowed, a vertex is unknown
    E = cugraph.Graph()
    assert cugraph.subgraph(E, []).edgelist is None
    df, off = cugraph.batched_ego_graphs(E, [], radius=2)
    assert len(df) == 0 and list(df.columns) == ["src", "dst"] and off.tolist() == [0]
    with pytest.raises(ValueError, match="not valid"):
        cugraph.subgraph(E, [3])
    with pytest.raises(ValueError, match="not valid"):
        cugraph.ego_graph(E, 3)
    with pytest.raises(ValueError, match="integer vertex ids"):
        cugraph.subgraph(E, [1.5])


def test_distributed_graph_is_refused():
    import cugraph
    G = cugraph.Graph()
    G._distributed = True
    for call in (lambda: cugraph.subgraph(G, [0]), lambda: cugraph.ego_graph(G, 0),
                 lambda: cugraph.batched_ego_graphs(G, [0])):
        with pytest.raises(NotImplementedError, match="distributed graph"):
            call()


def test_key_arithmetic_on_the_host(tmp_path):
    """slots x vertices at the edge of 64 bits, the sort bits, the thread tier's search and merge."""
    out = tmp_path / "ego_keys_test"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG, "csrc"),
                        "-o", str(out), os.path.join(ROOT, "tests", "c", "ego_keys_test.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(out)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS ego_keys" in r.stdout


# ------------------------------------------------------------------ the twin
@functools.lru_cache(maxsize=None)
def dataset(name):
    """(networkx graph, stored src, stored dst): an undirected file's edges both ways, a loop once."""
    import networkx as nx
    data = np.loadtxt(dataset_path(name), dtype=np.float64, ndmin=2)
    G = nx.DiGraph() if DATASETS[name] else nx.Graph()
    G.add_edges_from((int(a), int(b)) for a, b in data[:, :2])
    e = np.asarray(list(G.edges()), np.int64).reshape(-1, 2)
    if not DATASETS[name]:
        back = e[e[:, 0] != e[:, 1]][:, ::-1]
        e = np.concatenate([e, back])
    return G, e[:, 0].copy(), e[:, 1].copy()


def nx_edges(H):
    """The stored edges of a networkx graph, sorted: both ways when undirected, a loop once."""
    out = []
    for u, v in H.edges():
        out.append((u, v))
        if not H.is_directed() and u != v:
            out.append((v, u))
    return sorted(out)


def seeds_of(G):
    nodes = sorted(G.nodes())
    deg = G.out_degree if G.is_directed() else G.degree
    hub = max(nodes, key=lambda n: (deg(n), -n))
    return sorted({nodes[0], nodes[len(nodes) // 3], nodes[-1], hub})


@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(GOLDEN, "ego_vectors.json")) as f:
        return json.load(f)["datasets"]


@pytest.mark.parametrize("name", sorted(DATASETS))
def test_twin_equals_networkx_ego_graph(name):
    import networkx as nx
    G, s, d = dataset(name)
    rows = Rows(s, d)
    for seed in seeds_of(G):
        for r in range(4):
            H = nx.ego_graph(G, seed, radius=r)
            assert ego_vertices(rows, seed, r).tolist() == sorted(H.nodes()), (seed, r)
            es, ed, _ = ego_graph(s, d, None, seed, r, rows)
            assert sorted_edges(es, ed) == nx_edges(H), (seed, r)


@pytest.mark.parametrize("name", sorted(DATASETS))
def test_twin_equals_networkx_subgraph(name):
    G, s, d = dataset(name)
    nodes = np.asarray(sorted(G.nodes()), np.int64)
    rng = np.random.default_rng(len(nodes))
    sets = [rng.choice(nodes, size=k, replace=False) for k in (0, 1, 2, len(nodes) // 4, len(nodes) // 2, len(nodes))]
    bs, bd, _, off = batched(s, d, None, sets)
    assert off[0] == 0 and off[-1] == len(bs) and len(off) == len(sets) + 1
    for i, S in enumerate(sets):
        es, ed, _ = induced_subgraph(s, d, None, S)
        assert sorted_edges(es, ed) == nx_edges(G.subgraph(S.tolist())), i
        assert sorted_edges(bs[off[i]:off[i + 1]], bd[off[i]:off[i + 1]]) == sorted_edges(es, ed)


def test_twin_keeps_loops_repeats_and_weights():
    s = np.array([0, 0, 0, 1, 2, 2, 3])
    d = np.array([1, 1, 0, 2, 2, 0, 3])
    w = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], np.float32)
    es, ed, ew = induced_subgraph(s, d, w, [1, 0])
    assert sorted_edges(es, ed, ew) == sorted_edges([0, 0, 0], [1, 1, 0], np.array([1, 2, 3], np.float32))
    assert ego_vertices(Rows(s, d), 0, 1).tolist() == [0, 1] and ego_vertices(Rows(s, d), 0, 9).tolist() == [0, 1, 2]
    assert ego_vertices(Rows(s, d), 3, 5).tolist() == [3] and ego_vertices(Rows(s, d), 1, 0).tolist() == [1]
    es, ed, ew, off = batched_ego(s, d, w, [3, 3, 1], 0)
    assert off.tolist() == [0, 1, 2, 2] and es.tolist() == [3, 3] and ew.tolist() == [7.0, 7.0]


@pytest.mark.parametrize("name", sorted(DATASETS))
def test_twin_reproduces_the_recorded_facts(name):
    G, s, d = dataset(name)
    rows = Rows(s, d)
    facts = vectors()[name]
    assert sorted(facts) == sorted("%d/%d" % (seed, r) for seed in seeds_of(G) for r in range(4))
    for key, want in facts.items():
        seed, r = (int(x) for x in key.split("/"))
        es, ed, _ = ego_graph(s, d, None, seed, r, rows)
        pairs = set(zip(es.tolist(), ed.tolist())) if DATASETS[name] else \
            {(min(a, b), max(a, b)) for a, b in zip(es.tolist(), ed.tolist())}
        assert (len(ego_vertices(rows, seed, r)), len(pairs)) == (want["vertices"], want["edges"]), key
        if "edge_list" in want:
            assert sorted([a, b] for a, b in pairs) == want["edge_list"]


def test_recorded_facts_hold_the_known_numbers():
    v = vectors()
    k = v["karate.csv"]
    assert k["0/0"] == {"vertices": 1, "edges": 0} and k["0/3"] == {"vertices": 34, "edges": 78}
    assert (k["0/1"]["vertices"], k["0/1"]["edges"], len(k["0/1"]["edge_list"])) == (17, 34, 34)
    assert (k["33/1"]["vertices"], k["33/1"]["edges"], len(k["33/1"]["edge_list"])) == (18, 32, 32)
    a = v["karate-asymmetric.csv"]
    assert a["34/3"] == {"vertices": 1, "edges": 0} and len(a["1/1"]["edge_list"]) == a["1/1"]["edges"]
    assert v["email-Eu-core.csv"]["0/0"] == {"vertices": 1, "edges": 1}  # vertex 0 has a self-loop
    assert os.path.getsize(os.path.join(GOLDEN, "ego_vectors.json")) < 16384
