"""Neighbour sampling / random walks, the parts that need no GPU: the declarations of
sampling_algorithms.h, the library's exports, the Python names, the documented options, the two TypeErrors
of the cugraph layer (which fire before any GPU call), the plain-C client's build, and the sanity of the
numpy twin (tests/sampling_ref.py) that the GPU tests compare against."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.stats import chi2

import sampling_ref as ref
from conftest import GOLDEN, PKG, ROOT

LIB = os.path.join(PKG, "lib", "libcugraph_c.so")
LIBDIR = os.path.join(PKG, "lib")
INCLUDE = os.path.join(ROOT, "include", "cugraph_c")
# every function of the reference's header, with its argument names in order
WALK_ARGS = ["handle", "graph", "start_vertices", "max_length", "result", "error"]
FUNCS = {
    "cugraph_uniform_random_walks": WALK_ARGS,
    "cugraph_biased_random_walks": WALK_ARGS,
    "cugraph_node2vec_random_walks": ["handle", "graph", "start_vertices", "max_length", "p", "q", "result", "error"],
    "cugraph_node2vec": ["handle", "graph", "sources", "max_depth", "compress_result", "p", "q", "result", "error"],
    "cugraph_random_walk_result_get_max_path_length": ["result"],
    "cugraph_random_walk_result_get_paths": ["result"],
    "cugraph_random_walk_result_get_weights": ["result"],
    "cugraph_random_walk_result_get_path_sizes": ["result"],
    "cugraph_random_walk_result_free": ["result"],
    "cugraph_uniform_neighbor_sample": ["handle", "graph", "start", "fan_out", "with_replacement",
                                        "do_expensive_check", "result", "error"],
    "cugraph_sample_result_get_sources": ["result"],
    "cugraph_sample_result_get_destinations": ["result"],
    "cugraph_sample_result_get_start_labels": ["result"],
    "cugraph_sample_result_get_index": ["result"],
    "cugraph_sample_result_get_counts": ["result"],
    "cugraph_sample_result_free": ["result"],
    "cugraph_test_sample_result_create": ["handle", "srcs", "dsts", "weights", "counts", "result", "error"],
}


def header_text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_header_declares_the_types_and_functions():
    text = header_text(os.path.join(INCLUDE, "sampling_algorithms.h"))
    for t in ("cugraph_random_walk_result_t", "cugraph_sample_result_t"):
        assert re.search(r"typedef\s+struct\s*\{[^}]*\}\s*%s\s*;" % t, text), t
    for f, want in FUNCS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % f, text)
        assert m, f
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == want, f


def test_umbrella_header_includes_it():
    assert "<cugraph_c/sampling_algorithms.h>" in open(os.path.join(INCLUDE, "algorithms.h")).read()


def test_library_exports_the_functions():
    lib = ctypes.CDLL(LIB)
    assert [f for f in list(FUNCS) + ["cugraph_amd_sample_result_get_counts"] if not hasattr(lib, f)] == []


def test_python_names():
    import cugraph
    import pylibcugraph
    for name in ("uniform_neighbor_sample", "uniform_random_walks", "biased_random_walks", "node2vec"):
        assert callable(getattr(pylibcugraph, name)) and name in pylibcugraph.__all__
    for name in ("uniform_neighbor_sample", "random_walks"):
        assert callable(getattr(cugraph, name)) and name in cugraph.__all__


def test_options_are_documented():
    text = open(os.path.join(ROOT, "include", "cugraph_amd", "ext.h")).read()
    for name in ("sample_seed", "sample_path", "cugraph_amd_sample_result_get_counts"):
        assert name in text


def test_bad_arguments_are_refused_without_a_gpu():
    import cugraph
    G = cugraph.Graph()
    with pytest.raises(TypeError, match="must specify a 'max_depth'"):
        cugraph.random_walks(G, [0])
    with pytest.raises(TypeError, match="fanout_vals must be a list"):
        cugraph.uniform_neighbor_sample(G, [0], (1, 2))


def test_c_client_compiles_and_links(tmp_path):
    out = tmp_path / "sampling_test"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        "-o", str(out), os.path.join(ROOT, "tests", "c", "sampling_test.c"), "-L", LIBDIR,
                        "-lcugraph_c", f"-Wl,-rpath,{LIBDIR}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_golden_cases_are_consistent():
    with open(os.path.join(GOLDEN, "sampling_vectors.json")) as f:
        v = json.load(f)
    assert v["num_vertices"] == 6 and len(v["cases"]) == 2
    for c in v["cases"]:
        assert len(c["src"]) == len(c["dst"]) == len(c["edge_ids"]) == 8
        assert len(set(zip(c["src"], c["dst"]))) == 8 and len(set(c["edge_ids"])) == 8
        assert all(0 <= x < 6 for x in c["src"] + c["dst"] + c["start"])


# ---------------------------------------------------------------- the twin
def test_twin_draw_matches_a_plain_integer_restatement():
    def sm(x):
        z = (x + 0x9E3779B97F4A7C15) % 2**64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2**64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2**64
        return z ^ (z >> 31)
    for seed, stream, i, j in [(0, 0, 0, 0), (7, 2, 12345, 9), (2**53 - 1, 79, 2**40, 64), (12345, 1, 3, 2**33)]:
        want = sm(sm(sm(((seed * 0x9E3779B97F4A7C15) % 2**64) ^ stream) ^ i) ^ j)
        assert int(ref.draw(seed, stream, i, j)) == want
        for n in (1, 2, 65, 70000, 2**32 - 1):
            assert int(ref.index(want, n)) == (want * n) >> 64
        assert float(ref.unit(want)) == (want >> 11) / 2.0**53


@pytest.mark.parametrize("d, k", [(11, 10), (65, 64), (66, 65), (130, 65), (200, 10), (20, 3)])
def test_twin_floyd_gives_k_distinct_positions(d, k):
    for seed, hop, i in [(0, 0, 0), (7, 1, 5), (12345, 2, 999)]:
        p = ref.floyd(seed, hop, i, d, k)
        assert len(p) == k == len(set(p.tolist())) and p.min() >= 0 and p.max() < d


@pytest.mark.parametrize("d", [2, 3, 5, 63, 64, 65, 200, 4097])
def test_twin_index_of_draw_is_uniform(d):
    """Pearson chi-square of index(draw(seed, hop, i, j), d) over i < max(2000, 40 d) rounded down to a
    multiple of 10 and j < 10, against the 1 - 1e-6 quantile with d - 1 degrees of freedom."""
    n = max(2000, 40 * d) // 10 * 10
    i, j = np.repeat(np.arange(n), 10), np.tile(np.arange(10), n)
    bound = chi2.ppf(1 - 1e-6, d - 1)
    for seed in (0, 1, 2, 12345):
        for hop in (0, 1, 2):
            got = np.bincount(ref.index(ref.draw(seed, hop, i, j), d), minlength=d)
            assert len(got) == d
            e = len(i) / d
            stat = float(((got - e) ** 2 / e).sum())
            print(f"d={d} seed={seed} hop={hop}: chi2 {stat:.1f}, bound {bound:.1f}")
            assert stat < bound
