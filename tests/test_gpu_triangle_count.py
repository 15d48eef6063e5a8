"""Triangle counting on the GPU (csrc/triangle_count.hip through the C ABI and the
Python layers) against an exact scipy count of the same edges.

Every comparison is integer equality for every vertex.  check() also asserts that
``vertices`` is a permutation of the graph's ids, that ``counts`` has the graph's edge
type (the vertex type at these sizes) and that the counts sum to 3 x the triangle total."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, dataset_path
from gpu_util import host, make_graph, plc

pytestmark = pytest.mark.gpu

DATASETS = {"karate.csv": 45, "dolphins.csv": 95, "polbooks.csv": 560, "netscience.csv": 3764,
            "email-Eu-core.csv": 105461}


# ------------------------------------------------------------------ CPU truth
def symmetrize(s, d):
    """Both directions of every edge, duplicates dropped, self-loops kept."""
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    lo = int(min(s.min(), d.min()))
    span = int(max(s.max(), d.max())) - lo + 1
    assert span < 1 << 31
    key = np.unique(np.r_[(s - lo) * span + (d - lo), (d - lo) * span + (s - lo)])
    return key // span + lo, key % span + lo


def simple_adjacency(s, d, n):
    """0/1 matrix of the underlying simple graph: no self-loops, no repeated entries."""
    import scipy.sparse as sp
    keep = s != d
    A = sp.coo_matrix((np.ones(int(keep.sum()), np.int64), (s[keep], d[keep])), shape=(n, n)).tocsr()
    A.data[:] = 1  # tocsr() summed the repeated entries
    return A


def truth_plain(s, d, n):
    """counts[v] = (A @ A * A).sum(row v) / 2."""
    A = simple_adjacency(s, d, n)
    twice = np.asarray((A @ A).multiply(A).sum(axis=1)).ravel()
    assert (twice % 2 == 0).all()
    return twice // 2


def truth_oriented(s, d, n):
    """The same counts from the edges oriented low -> high (degree, id): L[a, b] = 1 when
    a < b in that order.  (L @ L.T * L)[a, b] is the number of triangles with a lowest
    and b in the middle, (L.T @ L * L)[b, c] the number with b in the middle and c highest."""
    A = simple_adjacency(s, d, n).tocoo()
    deg = np.bincount(A.row, minlength=n)
    up = (deg[A.row] < deg[A.col]) | ((deg[A.row] == deg[A.col]) & (A.row < A.col))
    import scipy.sparse as sp
    L = sp.coo_matrix((np.ones(int(up.sum()), np.int64), (A.row[up], A.col[up])), shape=(n, n)).tocsr()
    low_mid = (L @ L.T).multiply(L)
    mid_high = (L.T @ L).multiply(L)
    low = np.asarray(low_mid.sum(axis=1)).ravel()
    mid = np.asarray(low_mid.sum(axis=0)).ravel()
    high = np.asarray(mid_high.sum(axis=0)).ravel()
    assert low.sum() == mid.sum() == high.sum()
    return low + mid + high


class Case:
    """A symmetrised edge list, the ids the graph must report and each id's count.
    ``counts`` (indexed like ``ids``) is computed by scipy unless given."""

    def __init__(self, s, d, renumber, vdtype=np.int32, counts=None, symmetrized=False):
        self.s, self.d = (np.asarray(s, np.int64), np.asarray(d, np.int64)) if symmetrized else symmetrize(s, d)
        self.renumber, self.vdtype = renumber, vdtype
        self.ids = np.unique(np.r_[self.s, self.d]) if renumber else np.arange(int(self.s.max()) + 1)
        if counts is None:
            n = len(self.ids)
            counts = truth_oriented(np.searchsorted(self.ids, self.s), np.searchsorted(self.ids, self.d), n)
        self.counts = np.asarray(counts, np.int64)
        assert len(self.counts) == len(self.ids) and self.counts.sum() % 3 == 0
        self.triangles = int(self.counts.sum()) // 3

    def with_(self, renumber=None, vdtype=None):
        c = object.__new__(Case)
        c.__dict__.update(self.__dict__)
        if vdtype is not None:
            c.vdtype = vdtype
        if renumber is not None and renumber != self.renumber:
            assert self.renumber, "only a renumbered case can be switched"
            # without renumbering the graph has every id 0 .. max, the ones without edges too
            c.renumber = False
            c.ids = np.arange(int(self.ids.max()) + 1)
            c.counts = np.zeros(len(c.ids), np.int64)
            c.counts[self.ids] = self.counts
        return c

    def graph(self, transposed=False, options=None):
        return make_graph(self.s, self.d, None, transposed=transposed, renumber=self.renumber, symmetric=True,
                          vdtype=self.vdtype, options=options)


def check(case, vertices, counts):
    """Returns the counts by position in case.ids."""
    v, c = host(vertices), host(counts)
    assert v.dtype == np.dtype(case.vdtype) and c.dtype == v.dtype  # edge type = vertex type below 2^31 edges
    assert len(v) == len(case.ids) and len(c) == len(v)
    assert np.array_equal(np.sort(v), case.ids), "vertices is not a permutation of the graph's ids"
    if not case.renumber:
        assert np.array_equal(v, case.ids)
    by_id = np.empty(len(v), np.int64)
    by_id[np.searchsorted(case.ids, v)] = c
    assert np.array_equal(by_id, case.counts)
    assert int(c.astype(np.int64).sum()) == 3 * case.triangles
    return by_id


def run(case, transposed=False, options=None, calls=1):
    h, g = case.graph(transposed, options)
    out = None
    for _ in range(calls):  # the second call runs on the cached orientation
        by_id = check(case, *plc().triangle_count(h, g, None, False))
        assert out is None or np.array_equal(out, by_id)
        out = by_id
    return out


# ------------------------------------------------------------------ the graphs (built once)
@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(GOLDEN, "triangle_count_vectors.json")) as f:
        return json.load(f)


def dataset_edges(name):
    e = np.loadtxt(dataset_path(name), usecols=(0, 1), dtype=np.int64)
    return e[:, 0], e[:, 1]


@functools.lru_cache(maxsize=None)
def dataset(name):
    s, d = dataset_edges(name)
    return Case(s, d, renumber=True)


@functools.lru_cache(maxsize=None)
def rmat_case(scale):
    from oracle.rmat import rmat
    s, d = rmat(scale, 16 << scale, seed=7)
    case = Case(s, d, renumber=True)
    case.loop_entries = int((s == d).sum())  # self-loops among the generated entries; they stay in the graph
    return case


def clique_edges(ids):
    a, b = np.meshgrid(ids, ids, indexing="ij")
    keep = a < b
    return a[keep], b[keep]


@functools.lru_cache(maxsize=None)
def clique():
    n = 1500
    s, d = clique_edges(np.arange(n))
    return Case(s, d, renumber=True, counts=np.full(n, (n - 1) * (n - 2) // 2))  # C(1499, 2) = 1122751


@functools.lru_cache(maxsize=None)
def bipartite():
    n = 2000
    a, b = np.meshgrid(np.arange(n), np.arange(n, 2 * n), indexing="ij")
    return Case(a.ravel(), b.ravel(), renumber=True, counts=np.zeros(2 * n, np.int64))


@functools.lru_cache(maxsize=None)
def friendship(hub_last=False):
    """t triangles that share one hub; the hub is id 0, or the highest id."""
    t = 3000
    hub = 2 * t if hub_last else 0
    first = 0 if hub_last else 1
    a = first + 2 * np.arange(t)
    b = a + 1
    s = np.r_[np.full(t, hub), np.full(t, hub), a]
    d = np.r_[a, b, b]
    counts = np.ones(2 * t + 1, np.int64)
    counts[hub] = t
    return Case(s, d, renumber=True, counts=counts)


@functools.lru_cache(maxsize=None)
def clique_above_path():
    """A 5000-vertex path on ids 0..4999 and K_300 on ids 5000..5299, joined by one edge:
    the highest degrees sit on the highest ids."""
    p, k = 5000, 300
    ps = np.arange(p)  # 0-1, ..., 4998-4999, 4999-5000
    cs, cd = clique_edges(np.arange(p, p + k))
    counts = np.r_[np.zeros(p, np.int64), np.full(k, (k - 1) * (k - 2) // 2)]
    return Case(np.r_[ps, cs], np.r_[ps + 1, cd], renumber=True, counts=counts)


LONG_ROWS = {"clique": clique, "bipartite": bipartite, "friendship": friendship}


# ------------------------------------------------------------------ 0. the CPU truth itself
def test_cpu_truth_forms_agree_at_rmat12():
    c = rmat_case(12)
    n = len(c.ids)
    assert np.array_equal(truth_plain(np.searchsorted(c.ids, c.s), np.searchsorted(c.ids, c.d), n), c.counts)


# ------------------------------------------------------------------ 1. golden vectors
def golden_case(name):
    v = vectors()[name]
    if "edges" in v:
        s, d = dataset_edges(v["edges"])  # both directions, in the reference's order
    else:
        s, d = np.asarray(v["src"]), np.asarray(v["dst"])
    assert len(s) == v["num_edges"]
    return v, Case(s, d, renumber=False, symmetrized=True)


@pytest.mark.parametrize("name", ["small", "dolphins"])
def test_golden_vectors(name):
    v, case = golden_case(name)
    assert len(case.ids) == v["num_vertices"]
    if "all_counts" in v:
        assert case.counts.tolist() == v["all_counts"]
    if "triangles" in v:
        assert case.triangles == v["triangles"]
    h, g = case.graph()
    start = np.asarray(v["start"], np.int32)
    vertices, counts = plc().triangle_count(h, g, start, False)
    assert host(vertices).tolist() == v["start"] and host(counts).tolist() == v["result"]
    check(case, *plc().triangle_count(h, g, None, False))


# ------------------------------------------------------------------ 2. the datasets
@pytest.mark.parametrize("vdtype", [np.int32, np.int64])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("name", sorted(DATASETS))
def test_datasets(name, renumber, transposed, vdtype):
    case = dataset(name).with_(renumber=renumber, vdtype=vdtype)
    assert case.triangles == DATASETS[name]
    run(case, transposed)


# ------------------------------------------------------------------ 3. R-MAT
@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("scale,loops,triangles,largest", [(12, 207, 478805, 33425), (14, 335, 2824396, 138116)])
def test_rmat(scale, loops, triangles, largest, renumber):
    case = rmat_case(scale)
    assert case.loop_entries == loops and (case.s == case.d).any()
    assert case.triangles == triangles and int(case.counts.max()) == largest
    run(case.with_(renumber=renumber))


# ------------------------------------------------------------------ 4. long oriented rows
@pytest.mark.parametrize("name", sorted(LONG_ROWS))
def test_long_rows(name):
    run(LONG_ROWS[name]())


# ------------------------------------------------------------------ 5. ids that are not ranks
@pytest.mark.parametrize("make", [lambda: friendship(True), clique_above_path], ids=["friendship", "clique_above_path"])
def test_ids_that_are_not_ranks(make):
    case = make()
    renumbered = run(case)
    plain = run(case.with_(renumber=False))
    assert np.array_equal(renumbered, plain)


# ------------------------------------------------------------------ 6. paths and the cached orientation
def path_cases():
    return {"rmat12": lambda: rmat_case(12), "rmat14": lambda: rmat_case(14), **LONG_ROWS}


@pytest.mark.parametrize("name", sorted(path_cases()))
def test_paths_give_equal_arrays(name):
    case = path_cases()[name]()
    outs = [run(case, options={"tc_path": p}, calls=2) for p in (0, 1, 2)]
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


@pytest.mark.parametrize("path", [0, 1, 2])
def test_paths_without_renumbering(path):
    run(clique_above_path().with_(renumber=False), options={"tc_path": path}, calls=2)


def test_tc_path_is_range_checked():
    h = plc().ResourceHandle()
    with pytest.raises(ValueError, match="tc_path"):
        h.set_option("tc_path", 3)


# ------------------------------------------------------------------ 7. repeated entries, self-loops
@pytest.mark.parametrize("path", [0, 1, 2])
@pytest.mark.parametrize("renumber", [True, False])
def test_repeated_entries_count_once(renumber, path):
    s = np.array([0, 1, 1, 2, 2, 0] * 2)
    d = np.array([1, 0, 2, 1, 0, 2] * 2)
    h, g = make_graph(s, d, None, renumber=renumber, symmetric=True, options={"tc_path": path})
    vertices, counts = plc().triangle_count(h, g, None, False)
    assert sorted(host(vertices).tolist()) == [0, 1, 2] and host(counts).tolist() == [1, 1, 1]


@pytest.mark.parametrize("renumber", [True, False])
def test_self_loops_are_ignored(renumber):
    n = 200
    p = np.arange(n - 1)
    s, d = np.r_[p, p + 1, np.arange(n)], np.r_[p + 1, p, np.arange(n)]
    h, g = make_graph(s, d, None, renumber=renumber, symmetric=True)
    vertices, counts = plc().triangle_count(h, g, None, False)
    assert len(host(vertices)) == n and not host(counts).any()
    # ... and a triangle with loops on its corners still counts once
    s, d = np.array([0, 1, 1, 2, 2, 0, 0, 1, 2]), np.array([1, 0, 2, 1, 0, 2, 0, 1, 2])
    h, g = make_graph(s, d, None, renumber=renumber, symmetric=True)
    assert host(plc().triangle_count(h, g, None, False)[1]).tolist() == [1, 1, 1]


# ------------------------------------------------------------------ 8. start lists
@functools.lru_cache(maxsize=None)
def sparse_id_case():
    """karate with the ids spread out: id -> 1000 + 37 * id."""
    s, d = dataset_edges("karate.csv")
    return Case(1000 + 37 * s, 1000 + 37 * d, renumber=True)


def test_start_list_duplicates_and_order():
    case = sparse_id_case()
    h, g = case.graph()
    start = case.ids[[33, 0, 5, 33, 12, 0, 1]].astype(np.int32)
    vertices, counts = plc().triangle_count(h, g, start, True)
    assert host(vertices).dtype == np.int32 and host(counts).dtype == np.int32
    assert np.array_equal(host(vertices), start)
    assert np.array_equal(host(counts), case.counts[np.searchsorted(case.ids, start)])
    assert host(counts)[0] == 15 and host(counts)[1] == 18  # networkx.triangles(karate)[33], [0]


def test_empty_start_list():
    h, g = sparse_id_case().graph()
    vertices, counts = plc().triangle_count(h, g, np.zeros(0, np.int32), True)
    assert len(host(vertices)) == 0 and len(host(counts)) == 0


@pytest.mark.parametrize("renumber", [True, False])
def test_unknown_start_id(renumber):
    case = sparse_id_case() if renumber else dataset("karate.csv")
    h, g = case.graph()
    known = int(case.ids[0])
    for unknown in (known + 1 if renumber else 34, -5, 2 ** 31 - 1):
        start = np.array([known, unknown, known], np.int32)
        with pytest.raises(ValueError, match="invalid vertex IDs"):
            plc().triangle_count(h, g, start, True)
        vertices, counts = plc().triangle_count(h, g, start, False)
        assert np.array_equal(host(vertices), start)
        assert host(counts).tolist() == [int(case.counts[0]), 0, int(case.counts[0])]


def test_start_list_of_the_wrong_dtype():
    h, g = sparse_id_case().graph()
    with pytest.raises(ValueError, match="vertex type"):
        plc().triangle_count(h, g, np.array([1000], np.int64), False)


# ------------------------------------------------------------------ 9. refusals
def test_asymmetric_graph_is_refused():
    h, g = make_graph([0, 1], [1, 2], None, symmetric=False)
    with pytest.raises(ValueError, match="triangle_count currently supports undirected graphs only"):
        plc().triangle_count(h, g, None, False)


def test_multigraph_is_refused():
    p = plc()
    h = p.ResourceHandle()
    s, d = np.array([0, 1, 0, 1], np.int32), np.array([1, 0, 1, 0], np.int32)
    g = p.SGGraph(h, p.GraphProperties(is_symmetric=True, is_multigraph=True), s, d, None, store_transposed=False,
                  renumber=True)
    with pytest.raises(ValueError, match="does not support multi-graphs"):
        p.triangle_count(h, g, None, False)


def test_multi_gpu_graph_is_not_implemented():
    """One rank over RCCL, the setup of test_gpu_bench_parity.py's one-rank tests."""
    import torch
    import torch.distributed as dist
    import bench
    p = plc()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(bench.free_port())
    dist.init_process_group("gloo", rank=0, world_size=1)
    ctx = p.comms.init_rccl(1)
    try:
        h = p.ResourceHandle(ctx.ptr)
        s = torch.tensor([0, 1, 1, 2, 2, 0], dtype=torch.int32, device="cuda")
        d = torch.tensor([1, 0, 2, 1, 0, 2], dtype=torch.int32, device="cuda")
        g = p.MGGraph(h, p.GraphProperties(is_symmetric=True, is_multigraph=False), s, d, None,
                      store_transposed=False, num_edges=6)
        with pytest.raises(NotImplementedError, match="multi-GPU"):
            p.triangle_count(h, g, None, False)
        g = None
        h = None
    finally:
        torch.cuda.synchronize()
        p.trim_device_cache()
        ctx.free()
        dist.destroy_process_group()


# ------------------------------------------------------------------ 10. cugraph.triangle_count
@functools.lru_cache(maxsize=None)
def karate_nx():
    import networkx as nx
    s, d = dataset_edges("karate.csv")
    G = nx.Graph()
    G.add_edges_from(zip(s.tolist(), d.tolist()))
    return G, nx.triangles(G)


def test_cugraph_triangle_count_graph():
    import cugraph
    import pandas as pd
    nxG, want = karate_nx()
    s, d = dataset_edges("karate.csv")
    G = cugraph.Graph()
    G.from_pandas_edgelist(pd.DataFrame({"s": s, "d": d}), "s", "d")
    df = cugraph.triangle_count(G)
    assert list(df.columns) == ["vertex", "counts"]
    assert dict(zip(df["vertex"].tolist(), df["counts"].tolist())) == want
    assert sum(want.values()) == 3 * 45
    one = cugraph.triangle_count(G, 33)
    assert one["vertex"].tolist() == [33] and one["counts"].tolist() == [want[33]]
    for start in ([5, 0, 33, 5], pd.Series([2, 31])):
        df = cugraph.triangle_count(G, start)
        assert df["vertex"].tolist() == list(start) and df["counts"].tolist() == [want[v] for v in start]


def test_cugraph_triangle_count_networkx():
    import cugraph
    nxG, want = karate_nx()
    df = cugraph.triangle_count(nxG)
    assert dict(zip(df["vertex"].tolist(), df["counts"].tolist())) == want
    df = cugraph.triangle_count(nxG, [0, 33])
    assert df["vertex"].tolist() == [0, 33] and df["counts"].tolist() == [want[0], want[33]]
