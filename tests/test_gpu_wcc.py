"""Weakly connected components on the GPU (csrc/wcc.hip through the C ABI and the
Python layers) against scipy.sparse.csgraph.connected_components on the same edges.

Unless a test says otherwise it asserts, through check(): the CPU truth's partition,
every label in [0, V), the label of a vertex equal to the smallest internal id of its
component (internal id = position in the result's ``vertices``), and ``vertices`` a
permutation of the graph's ids."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, dataset_path
from gpu_util import host, make_graph, plc

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ CPU truth
def symmetrize(s, d):
    """Both directions of every edge, duplicates dropped."""
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    if len(s) == 0:
        return s, d
    lo = int(min(s.min(), d.min()))
    span = int(max(s.max(), d.max())) - lo + 1
    assert span < 1 << 31
    key = np.unique(np.r_[(s - lo) * span + (d - lo), (d - lo) * span + (s - lo)])
    return key // span + lo, key % span + lo


def truth(s, d, ids):
    """Component number of every id of ``ids`` (sorted, unique) under the edges (s, d)."""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    n = len(ids)
    a, b = np.searchsorted(ids, s), np.searchsorted(ids, d)
    A = sp.coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(n, n)).tocsr()
    return connected_components(A, directed=False)[1]


class Case:
    """A symmetrised edge list, the ids the graph must report and their CPU components."""

    def __init__(self, s, d, renumber, vdtype=np.int32):
        self.s, self.d = symmetrize(s, d)
        self.renumber, self.vdtype = renumber, vdtype
        self.ids = np.unique(np.r_[self.s, self.d]) if renumber else np.arange(int(self.s.max()) + 1)
        self.comp = truth(self.s, self.d, self.ids)
        self.sizes = np.bincount(self.comp)

    def graph(self, transposed=False, options=None):
        return make_graph(self.s, self.d, None, transposed=transposed, renumber=self.renumber, symmetric=True,
                          vdtype=self.vdtype, options=options)


def check(case, vertices, labels):
    v, lab = host(vertices), host(labels)
    V = len(case.ids)
    assert v.dtype == np.dtype(case.vdtype) and lab.dtype == v.dtype
    assert len(v) == V and len(lab) == V
    assert np.array_equal(np.sort(v), case.ids), "vertices is not a permutation of the graph's ids"
    if not case.renumber:
        assert np.array_equal(v, case.ids)
    assert lab.min() >= 0 and lab.max() < V
    comp = case.comp[np.searchsorted(case.ids, v)]  # CPU component of the vertex at every position
    smallest = np.full(len(case.sizes), V, np.int64)
    np.minimum.at(smallest, comp, np.arange(V))
    # equal labels <=> equal CPU component, and the label is the component's smallest internal id
    assert np.array_equal(lab, smallest[comp])
    return v, lab


def run(case, transposed=False, options=None):
    h, g = case.graph(transposed, options)
    vertices, labels = plc().weakly_connected_components(h, g, False)
    return check(case, vertices, labels)


# ------------------------------------------------------------------ the graphs (built once)
@functools.lru_cache(maxsize=None)
def golden_edges():
    with open(os.path.join(GOLDEN, "wcc_vectors.json")) as f:
        return json.load(f)


def path_edges(order):
    n = 4097
    ids = {"in_order": np.arange(n), "reversed": np.arange(n)[::-1],
           "scrambled": np.random.default_rng(5).permutation(n)}[order]
    return ids[:-1], ids[1:]


@functools.lru_cache(maxsize=None)
def star_cycle():
    """A 70,000-leaf star whose hub gets internal id 0 and is the guessed giant, a
    100,000-vertex cycle that is the largest component, and 1,000 disjoint edges."""
    L, C, P = 70000, 100000, 1000
    hub = 0
    leaves = np.arange(1, L + 1)
    cyc = np.arange(L + 1, L + 1 + C)
    pairs = np.arange(L + 1 + C, L + 1 + C + 2 * P)
    s = np.r_[np.full(L, hub), cyc, pairs[0::2]]
    d = np.r_[leaves, np.roll(cyc, -1), pairs[1::2]]
    return Case(s, d, renumber=True)


def small_component_edges():
    """300 components of 1..2000 vertices: a random tree plus 10 % more edges, some
    self-loops, all ids permuted among 5,000 more ids than are used; the highest id is unused."""
    rng = np.random.default_rng(17)
    sizes = rng.integers(1, 2001, 300)
    total = int(sizes.sum())
    ss, dd, base = [], [], 0
    for n in sizes:
        n = int(n)
        if n > 1:
            child = np.arange(1, n)
            ss.append(base + child)
            dd.append(base + (rng.random(n - 1) * child).astype(np.int64))  # a parent below the child
            extra = max(1, n // 10)
            ss.append(base + rng.integers(0, n, extra))
            dd.append(base + rng.integers(0, n, extra))
        base += n
    loops = rng.integers(0, total, 500)  # self-loops, also on some one-vertex components
    s, d = np.r_[tuple(ss) + (loops,)], np.r_[tuple(dd) + (loops,)]
    N = total + 5000
    new_id = rng.permutation(N - 1)[:total]  # id N-1 is never used
    return new_id[s], new_id[d], N


@functools.lru_cache(maxsize=None)
def small_components():
    s, d, _ = small_component_edges()
    return Case(s, d, renumber=False)


@functools.lru_cache(maxsize=None)
def small_components_int64():
    s, d, _ = small_component_edges()
    return Case((1 << 33) + 3 * s, (1 << 33) + 3 * d, renumber=True, vdtype=np.int64)


@functools.lru_cache(maxsize=None)
def rmat_case(scale, edges, seed, renumber):
    from oracle.rmat import rmat
    s, d = rmat(scale, edges, seed=seed)
    return Case(s, d, renumber=renumber)


# ------------------------------------------------------------------ 1. the reference's C test graph
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("renumber", [False, True])
def test_golden_graph(renumber, transposed):
    gold = golden_edges()
    case = Case(gold["src"], gold["dst"], renumber)
    assert len(case.s) == gold["num_edges"] and len(case.ids) == gold["num_vertices"]
    assert np.array_equal(case.comp, gold["result"])
    v, lab = run(case, transposed)
    if not renumber:
        assert lab.tolist() == [0] * 6 + [6] * 6


# ------------------------------------------------------------------ 2. the deepest pointer chains
@pytest.mark.parametrize("renumber", [False, True])
@pytest.mark.parametrize("order", ["in_order", "reversed", "scrambled"])
def test_path(order, renumber):
    case = Case(*path_edges(order), renumber)
    assert len(case.sizes) == 1 and len(case.ids) == 4097
    v, lab = run(case)
    assert not lab.any()


# ------------------------------------------------------------------ 3. the giant guess is wrong
@pytest.mark.parametrize("sample", [None, 0])
def test_star_and_cycle(sample):
    case = star_cycle()
    assert len(case.sizes) == 1002 and sorted(case.sizes)[-2:] == [70001, 100000]
    v, lab = run(case, options=None if sample is None else {"wcc_sample": sample})
    assert v[0] == 0 and lab[0] == 0  # the hub has internal id 0: it is the guess, and not the largest set
    assert np.bincount(lab).max() == 100000


# ------------------------------------------------------------------ 4. many small components, isolated ids
def test_small_components():
    case = small_components()
    _, _, N = small_component_edges()
    assert len(case.ids) < N  # the highest id is unused
    assert (case.sizes == 1).sum() > 4000 and (case.sizes > 1).sum() > 250
    run(case)


# ------------------------------------------------------------------ 5. RMAT
@pytest.mark.parametrize("renumber", [False, True])
def test_rmat18(renumber):
    case = rmat_case(18, 2 << 18, 11, renumber)
    if not renumber:
        assert case.sizes.max() == 96013 and (case.sizes > 1).sum() == 513
        assert (case.sizes == 1).sum() + (1 << 18) - len(case.ids) == 165095
    else:
        assert case.sizes.max() == 96013 and len(case.sizes) == 513
    run(case)


def test_rmat16_dense():
    case = rmat_case(16, 16 << 16, 7, True)
    assert case.sizes.max() == 46674 and np.bincount(case.s).max() == 9710
    run(case)


# ------------------------------------------------------------------ 6. 64-bit ids
def test_int64_ids_above_2_33():
    case = small_components_int64()
    assert case.ids.min() >= 1 << 33
    run(case)


# ------------------------------------------------------------------ 7. options and determinism
@pytest.mark.parametrize("name", ["star_cycle", "small_components", "rmat18", "rmat18_renumbered", "rmat16"])
def test_same_bits_under_every_option(name):
    import torch
    case = {"star_cycle": star_cycle, "small_components": small_components,
            "rmat18": lambda: rmat_case(18, 2 << 18, 11, False),
            "rmat18_renumbered": lambda: rmat_case(18, 2 << 18, 11, True),
            "rmat16": lambda: rmat_case(16, 16 << 16, 7, True)}[name]()
    h, g = case.graph()
    p = plc()
    v0, first = p.weakly_connected_components(h, g, False)
    check(case, v0, first)
    _, again = p.weakly_connected_components(h, g, False)
    assert torch.equal(first, again)
    for k in (0, 1, 2, 4):
        h.set_option("wcc_sample", k)
        v, lab = p.weakly_connected_components(h, g, False)
        assert torch.equal(v, v0) and torch.equal(lab, first), f"wcc_sample={k}"


# ------------------------------------------------------------------ 8. errors
def test_asymmetric_graph_is_refused():
    h, g = make_graph([0, 1], [1, 2], None, symmetric=False)
    with pytest.raises(ValueError, match="symmetric"):
        plc().weakly_connected_components(h, g, False)


def test_strongly_connected_components_is_not_implemented():
    import cugraph
    import pandas as pd
    h, g = make_graph([0, 1], [1, 0], None, symmetric=True)
    with pytest.raises(NotImplementedError, match="SCC"):
        plc().strongly_connected_components(h, g, False)
    G = cugraph.Graph(directed=True)
    G.from_pandas_edgelist(pd.DataFrame({"s": [0, 1], "d": [1, 2]}), "s", "d")
    with pytest.raises(NotImplementedError):
        cugraph.strongly_connected_components(G)
    with pytest.raises(NotImplementedError):
        cugraph.connected_components(G, connection="strong")


def test_graph_without_edges():
    h, g = make_graph([], [], None, symmetric=True)
    v, lab = plc().weakly_connected_components(h, g, False)
    assert v.numel() == 0 and lab.numel() == 0


# ------------------------------------------------------------------ 9. the Python layers
def _csv_case(name):
    from oracle import graph as og
    s, d, _ = og.read_csv(dataset_path(name))
    return Case(s, d, renumber=True)


def _check_frame(case, df):
    assert list(df.columns) == ["labels", "vertex"]
    return check(case, np_tensor(df["vertex"].to_numpy().astype(np.int32)), np_tensor(df["labels"].to_numpy()))


def np_tensor(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a))


def test_cugraph_karate_and_netscience():
    import cugraph
    import pandas as pd
    for name in ("karate.csv", "netscience.csv"):
        case = _csv_case(name)
        G = cugraph.Graph()
        G.from_pandas_edgelist(pd.DataFrame({"s": case.s, "d": case.d}), "s", "d")
        v, lab = _check_frame(case, cugraph.weakly_connected_components(G))
        if name == "karate.csv":
            assert len(case.sizes) == 1 and not lab.any()
        else:
            assert len(case.sizes) > 1
        # a directed Graph over one direction of the edges: the same partition
        D = cugraph.Graph(directed=True)
        one = case.s < case.d
        D.from_pandas_edgelist(pd.DataFrame({"s": case.s[one], "d": case.d[one]}), "s", "d")
        _check_frame(case, cugraph.connected_components(D))


def test_cugraph_networkx_input():
    import cugraph
    import networkx as nx
    G = nx.Graph([("a", "b"), ("b", "c"), ("x", "y")])
    G.add_edge("p", "q")
    out = cugraph.weakly_connected_components(G)
    assert set(out) == set("abcxypq")
    groups = {}
    for node, label in out.items():
        groups.setdefault(int(label), set()).add(node)
    assert sorted(map(sorted, groups.values())) == [["a", "b", "c"], ["p", "q"], ["x", "y"]]


@pytest.mark.parametrize("directed", [False, True])
def test_scipy_matrix_with_empty_rows(directed):
    import cugraph
    import scipy.sparse as sp
    n = 9  # edges 0-2, 2-5, 3-4 (one direction only); rows 1, 6, 7, 8 are empty
    M = sp.csr_matrix((np.ones(3), ([0, 2, 3], [2, 5, 4])), shape=(n, n))
    count, labels = cugraph.connected_components(M, directed=directed)
    assert count == 6 and labels.tolist() == [0, 1, 0, 3, 3, 0, 6, 7, 8]
    assert cugraph.weakly_connected_components(M.toarray(), directed=directed, return_labels=False) == 6


def test_pylibcugraph_legacy_csr_form():
    import scipy.sparse as sp
    import torch
    n = 10  # ids 8 and 9 have no edges and lie past the graph's last vertex
    s, d = symmetrize([0, 1, 4, 6], [1, 2, 5, 7])
    A = sp.csr_matrix((np.ones(len(s)), (s, d)), shape=(n, n))
    labels = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    plc().weakly_connected_components(torch.as_tensor(A.indptr), torch.as_tensor(A.indices), None, n, len(s),
                                      labels)
    assert labels.tolist() == [0, 0, 0, 3, 4, 4, 6, 6, 8, 9]
    on_host = np.full(n, -1, np.int32)
    plc().weakly_connected_components(A.indptr, A.indices, None, n, len(s), on_host)
    assert on_host.tolist() == labels.tolist()
