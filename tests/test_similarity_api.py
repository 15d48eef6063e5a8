"""Similarity / two-hop, the parts that need no GPU: the declarations in similarity_algorithms.h and
graph_functions.h, the library's exports, the Python names, the two ValueErrors of
link_prediction/jaccard.py (which fire before any GPU call), the plain-C client's build and the
golden file's consistency."""
import ctypes
import json
import os
import re
import subprocess
from fractions import Fraction

import pytest

from conftest import GOLDEN, PKG, ROOT

LIB = os.path.join(PKG, "lib", "libcugraph_c.so")
LIBDIR = os.path.join(PKG, "lib")
INCLUDE = os.path.join(ROOT, "include", "cugraph_c")
# the reference's two headers declare these and no others
FUNCS = {"graph_functions.h": ["cugraph_create_vertex_pairs", "cugraph_vertex_pairs_get_first",
                               "cugraph_vertex_pairs_get_second", "cugraph_vertex_pairs_free",
                               "cugraph_two_hop_neighbors"],
         "similarity_algorithms.h": ["cugraph_similarity_result_get_similarity", "cugraph_similarity_result_free",
                                     "cugraph_jaccard_coefficients", "cugraph_sorensen_coefficients",
                                     "cugraph_overlap_coefficients"]}
MEASURES = ("jaccard", "sorensen", "overlap")


def header_text(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, name)).read(), flags=re.S)


def test_headers_declare_the_types_and_functions():
    for header, funcs in FUNCS.items():
        text = header_text(header)
        for f in funcs:
            assert re.search(r"\b%s\s*\(" % f, text), f
    assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*cugraph_vertex_pairs_t\s*;", header_text("graph_functions.h"))
    assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*cugraph_similarity_result_t\s*;",
                     header_text("similarity_algorithms.h"))
    # argument order of the reference: (handle, graph, vertex_pairs, use_weight, do_expensive_check, result, error)
    for m in MEASURES:
        args = re.search(r"cugraph_%s_coefficients\s*\(([^)]*)\)" % m, header_text("similarity_algorithms.h")).group(1)
        names = [a.split()[-1].lstrip("*") for a in args.split(",")]
        assert names == ["handle", "graph", "vertex_pairs", "use_weight", "do_expensive_check", "result", "error"]


def test_umbrella_header_includes_them():
    text = open(os.path.join(INCLUDE, "algorithms.h")).read()
    assert "<cugraph_c/similarity_algorithms.h>" in text and "<cugraph_c/graph_functions.h>" in text


def test_library_exports_the_functions():
    lib = ctypes.CDLL(LIB)
    assert [f for fs in FUNCS.values() for f in fs if not hasattr(lib, f)] == []


def test_python_names():
    import cugraph
    import pylibcugraph
    for name in [m + "_coefficients" for m in MEASURES] + ["get_two_hop_neighbors"]:
        assert callable(getattr(pylibcugraph, name)) and name in pylibcugraph.__all__
    for name in list(MEASURES) + [m + "_coefficient" for m in MEASURES]:
        assert callable(getattr(cugraph, name)) and name in cugraph.__all__
    assert callable(cugraph.Graph.get_two_hop_neighbors)


def test_options_are_documented():
    text = open(os.path.join(ROOT, "include", "cugraph_amd", "ext.h")).read()
    for name in ("sim_path", "sim_split_min", "two_hop_budget"):
        assert name in text


@pytest.mark.parametrize("measure", MEASURES)
def test_bad_arguments_are_refused_without_a_gpu(measure):
    import cugraph
    f, fc = getattr(cugraph, measure), getattr(cugraph, measure + "_coefficient")
    for G in (cugraph.Graph(directed=True), cugraph.DiGraph()):
        with pytest.raises(ValueError, match="Input must be an undirected Graph."):
            f(G)
        with pytest.raises(ValueError, match="Input must be an undirected Graph."):
            fc(G)
    for bad in ([(0, 1)], {"first": [0], "second": [1]}, 3):
        with pytest.raises(ValueError, match="vertex_pair must be a cudf dataframe"):
            f(cugraph.Graph(), vertex_pair=bad)


def test_c_client_compiles_and_links(tmp_path):
    out = tmp_path / "similarity_test"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(out), os.path.join(ROOT, "tests", "c", "similarity_test.c"), "-L", LIBDIR,
                        "-lcugraph_c", f"-Wl,-rpath,{LIBDIR}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_golden_vectors_are_consistent():
    with open(os.path.join(GOLDEN, "similarity_vectors.json")) as f:
        v = json.load(f)
    n = v["num_vertices"]
    edges = sorted(zip(v["src"], v["dst"]))
    assert len(edges) == 16 and edges == sorted(zip(v["dst"], v["src"])) and len(set(edges)) == 16
    nb = {u: {b for a, b in edges if a == u} for u in range(n)}
    assert len(v["first"]) == len(v["second"]) == 10
    for i, (a, b) in enumerate(zip(v["first"], v["second"])):
        c, da, db = len(nb[a] & nb[b]), len(nb[a]), len(nb[b])
        assert (c, da, db) == (v["counts"][i], v["degree_first"][i], v["degree_second"][i])
        assert Fraction(*v["jaccard"][i]) == Fraction(c, da + db - c)
        assert Fraction(*v["sorensen"][i]) == Fraction(2 * c, da + db)
        assert Fraction(*v["overlap"][i]) == Fraction(c, min(da, db))
    want = sorted([a, b] for a in range(n) for b in range(n) if a != b and any(b in nb[w] for w in nb[a]))
    assert v["two_hop"] == want and len(want) == 22
