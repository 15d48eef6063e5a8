"""Connected components, the parts that need no GPU: the labeling header, the
library's exports, the Python names and the argument errors of
components/connectivity.py:26-64 and :367-375, which fire before any GPU call."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import PKG, ROOT

LIB = os.path.join(PKG, "lib", "libcugraph_c.so")
HEADER = os.path.join(ROOT, "include", "cugraph_c", "labeling_algorithms.h")
FUNCS = ["cugraph_labeling_result_get_vertices", "cugraph_labeling_result_get_labels",
         "cugraph_labeling_result_free", "cugraph_weakly_connected_components",
         "cugraph_strongly_connected_components"]


def test_header_declares_the_labeling_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert "cugraph_labeling_result_t" in text
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, text), f
    umbrella = open(os.path.join(ROOT, "include", "cugraph_c", "algorithms.h")).read()
    assert "#include <cugraph_c/labeling_algorithms.h>" in umbrella


def test_library_exports_the_labeling_functions():
    lib = ctypes.CDLL(LIB)
    assert [f for f in FUNCS if not hasattr(lib, f)] == []


def test_python_names():
    import cugraph
    import pylibcugraph
    for n in ["weakly_connected_components", "strongly_connected_components"]:
        assert callable(getattr(pylibcugraph, n)) and n in pylibcugraph.__all__
    for n in ["weakly_connected_components", "strongly_connected_components", "connected_components"]:
        assert callable(getattr(cugraph, n)) and n in cugraph.__all__


def test_graph_input_rejects_matrix_only_arguments():
    import cugraph
    G = cugraph.Graph()  # no edge list: the checks must fire before anything touches it
    for api in (cugraph.weakly_connected_components, cugraph.strongly_connected_components,
                cugraph.connected_components):
        with pytest.raises(TypeError, match="directed"):
            api(G, directed=True)
        with pytest.raises(TypeError, match="return_labels"):
            api(G, return_labels=False)


def test_connection_argument():
    import cugraph
    M = np.zeros((3, 3))
    with pytest.raises(TypeError, match="must be 'weak'"):
        cugraph.weakly_connected_components(M, connection="strong")
    with pytest.raises(TypeError, match="must be 'strong'"):
        cugraph.strongly_connected_components(M, connection="weak")
    with pytest.raises(ValueError, match="invalid connection type"):
        cugraph.connected_components(M, connection="sideways")
    with pytest.raises(TypeError, match="not a supported type"):
        cugraph.weakly_connected_components([[0, 1], [1, 0]])


def test_matrix_without_entries_needs_no_gpu():
    import cugraph
    n, labels = cugraph.connected_components(np.zeros((4, 4)), directed=False)
    assert n == 4 and labels.tolist() == [0, 1, 2, 3]
    assert cugraph.weakly_connected_components(np.zeros((4, 4)), return_labels=False) == 4
