"""Jaccard / Sorensen / overlap similarity and two-hop neighbours on the GPU (csrc/similarity.hip,
csrc/two_hop.hip through the C ABI and the Python layers) against numpy / scipy.

The oracle: A is the 0/1 CSR of the symmetrised edges with self-loops kept, d = its row sums,
c = (A @ A)[u, v] (for the graphs with hub rows of thousands of entries the same number is taken
as the product of rows u and v, which A's symmetry makes equal and which needs no A @ A), and a
score is computed in float64 and cast to the result dtype.  Every comparison of scores is exact
equality, but for the sum over karate's edges against networkx.  Two-hop results are compared as
sets with the off-diagonal nonzeros of A @ A."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, dataset_path
from gpu_util import host, make_graph, plc

pytestmark = pytest.mark.gpu

MEASURES = ("jaccard", "sorensen", "overlap")
PATHS = (0, 1, 2, 3)


# ------------------------------------------------------------------ CPU truth
def symmetrize(s, d):
    """Both directions of every edge, duplicates dropped, self-loops kept."""
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    span = int(max(s.max(), d.max())) + 1
    key = np.unique(np.r_[s * span + d, d * span + s])
    return key // span, key % span


class Truth:
    """The oracle of one symmetrised edge list; ids are the graph's external ids in ascending
    order (every id 0 .. max without renumbering)."""

    def __init__(self, s, d, renumber, symmetrized=False):
        import scipy.sparse as sp
        self.s, self.d = (np.asarray(s, np.int64), np.asarray(d, np.int64)) if symmetrized else symmetrize(s, d)
        self.renumber = renumber
        self.ids = np.unique(np.r_[self.s, self.d]) if renumber else np.arange(int(max(self.s.max(), self.d.max())) + 1)
        n = len(self.ids)
        si, di = np.searchsorted(self.ids, self.s), np.searchsorted(self.ids, self.d)
        self.A = sp.coo_matrix((np.ones(len(si), np.int64), (si, di)), shape=(n, n)).tocsr()
        self.A.data[:] = 1  # tocsr() summed the repeated entries
        self.deg = np.asarray(self.A.sum(axis=1)).ravel()
        self._A2 = None

    def index(self, ids):
        """Position of every external id in self.ids, -1 for an id the graph does not have."""
        ids = np.asarray(ids, np.int64)
        pos = np.clip(np.searchsorted(self.ids, ids), 0, len(self.ids) - 1)
        return np.where(self.ids[pos] == ids, pos, -1)

    def A2(self):
        if self._A2 is None:
            self._A2 = (self.A @ self.A).tocsr()
        return self._A2

    def parts(self, first, second, rows=False):
        """(c, d(first), d(second)) as int64 arrays; unknown ids have no neighbours."""
        u, v = self.index(first), self.index(second)
        ok = (u >= 0) & (v >= 0)
        c = np.zeros(len(u), np.int64)
        if ok.any():
            if rows:
                c[ok] = np.asarray(self.A[u[ok]].multiply(self.A[v[ok]]).sum(axis=1)).ravel()
            else:
                c[ok] = np.asarray(self.A2()[u[ok], v[ok]]).ravel()
        du = np.where(u >= 0, self.deg[np.maximum(u, 0)], 0)
        dv = np.where(v >= 0, self.deg[np.maximum(v, 0)], 0)
        return c, du, dv

    def scores(self, measure, first, second, dtype=np.float32, rows=False):
        return score(measure, *self.parts(first, second, rows), dtype)

    def two_hop(self):
        """The set of (first, second) external ids."""
        B = self.A2().tocoo()
        keep = B.row != B.col
        return set(zip(self.ids[B.row[keep]].tolist(), self.ids[B.col[keep]].tolist()))

    def graph(self, transposed=False, vdtype=np.int32, options=None, w=None, wdtype=np.float32):
        return make_graph(self.s, self.d, w, transposed=transposed, renumber=self.renumber, symmetric=True,
                          vdtype=vdtype, wdtype=wdtype, options=options)


def score(measure, c, du, dv, dtype=np.float32):
    c, du, dv = (np.asarray(x, np.float64) for x in (c, du, dv))
    num, den = {"jaccard": (c, du + dv - c), "sorensen": (2.0 * c, du + dv), "overlap": (c, np.minimum(du, dv))}[measure]
    out = np.zeros(len(c), np.float64)
    np.divide(num, den, out=out, where=den > 0)
    return out.astype(dtype)


def run(measure, h, g, first, second, vdtype=np.int32, use_weight=False, expensive=False):
    """The coefficients on the host; checks the two id arrays come back as given."""
    f = getattr(plc(), measure + "_coefficients")
    a, b = np.asarray(first, vdtype), np.asarray(second, vdtype)
    ra, rb, x = f(h, g, a, b, use_weight, expensive)
    assert np.array_equal(host(ra), a) and np.array_equal(host(rb), b)
    x = host(x)
    assert len(x) == len(a)
    return x


def same(got, want):
    assert got.dtype == want.dtype
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{len(bad)} of {len(want)} scores differ, first at {bad[:5]}: {got[bad[:5]]} != {want[bad[:5]]}"


@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(GOLDEN, "similarity_vectors.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def dataset(name, renumber=True):
    from oracle import graph as og
    s, d, _ = og.read_csv(dataset_path(name + ".csv"))
    return Truth(s, d, renumber)


def random_pairs(t, n, seed):
    rng = np.random.default_rng(seed)
    return t.ids[rng.integers(0, len(t.ids), n)], t.ids[rng.integers(0, len(t.ids), n)]


# ------------------------------------------------------------------ 1. golden vectors
@pytest.mark.parametrize("vdtype", [np.int32, np.int64])
@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("transposed", [False, True])
def test_golden_vectors(transposed, renumber, vdtype):
    v = vectors()
    h, g = make_graph(v["src"], v["dst"], None, transposed=transposed, renumber=renumber, symmetric=True,
                      vdtype=vdtype)
    for m in MEASURES:
        want = np.array([n / d for n, d in v[m]], np.float64).astype(np.float32)
        same(run(m, h, g, v["first"], v["second"], vdtype), want)
        same(score(m, v["counts"], v["degree_first"], v["degree_second"]), want)


def test_result_dtype_follows_the_weight_type():
    v = vectors()
    t = Truth(v["src"], v["dst"], True, symmetrized=True)
    for wdtype in (np.float32, np.float64):
        h, g = t.graph(w=np.full(len(t.s), 2.5), wdtype=wdtype)
        for m in MEASURES:
            x = run(m, h, g, v["first"], v["second"])
            want = np.array([n / d for n, d in v[m]], np.float64).astype(wdtype)
            same(x, want)  # the weights themselves are not used


# ------------------------------------------------------------------ 2. datasets
@pytest.mark.parametrize("name", ["karate", "dolphins", "polbooks", "netscience", "email-Eu-core"])
def test_datasets(name):
    t = dataset(name)
    h, g = t.graph()
    ra, rb = random_pairs(t, 2000, 11)
    first, second = np.r_[t.s, ra], np.r_[t.d, rb]
    for m in MEASURES:
        same(run(m, h, g, first, second), t.scores(m, first, second))


def test_karate_jaccard_sum_is_networkx():
    import networkx as nx
    t = dataset("karate")
    G = nx.Graph()
    G.add_edges_from(zip(t.s.tolist(), t.d.tolist()))
    edges = list(G.edges())
    assert len(edges) == 78
    want = sum(p for _, _, p in nx.jaccard_coefficient(G, edges))
    assert abs(want - 10.9038861) < 1e-7
    h, g = t.graph()
    x = run("jaccard", h, g, [u for u, _ in edges], [v for _, v in edges])
    # every float32 score is within 2^-25 of its float64 value (scores are at most 1)
    assert abs(float(x.astype(np.float64).sum()) - want) <= 78 * 2.0 ** -25


# ------------------------------------------------------------------ 3. row shapes
def twin_hubs(m, ka, kb):
    """Hubs 0 and 1 share m leaves and have ka, kb private leaves.  Returns the oracle and pairs
    that cover hub-hub, hub-leaf (a long row against a 1- or 2-entry row), leaf-leaf, (u, u)."""
    shared = np.arange(2, 2 + m)
    pa = np.arange(2 + m, 2 + m + ka)
    pb = np.arange(2 + m + ka, 2 + m + ka + kb)
    s = np.r_[np.zeros(m + ka, np.int64), np.ones(m + kb, np.int64)]
    d = np.r_[shared, pa, shared, pb]
    t = Truth(s, d, False)
    last = int(t.ids[-1])
    first = [0, 1, 0, 1, 0, 2, 1, 2, 2, last, last, 0, 2, m + 1, 0]
    second = [1, 0, 0, 1, 2, 0, last, 3, 2, 0, 1, m + 1, last, 2, last]
    # hub-hub: c = m, Jaccard m / (m + ka + kb)
    c, du, dv = t.parts([0], [1], rows=True)
    assert (int(c[0]), int(du[0]), int(dv[0])) == (m, m + ka, m + kb)
    return t, first, second


SHAPES = [((10, 3, 0), np.int32, {}),                       # thread
          ((63, 0, 1), np.int32, {}),                       # 63 and 64 entries: the first wave pair
          ((64, 0, 0), np.int32, {}),
          ((1000, 24, 0), np.int32, {}),                    # 1024 ids: the longer row is staged
          ((1000, 24, 0), np.int64, {}),                    # above the 512-id stage of 8-byte ids
          ((1500, 5000, 0), np.int32, {}),                  # unstaged, the long row above the stage
          ((6000, 0, 100), np.int32, {"sim_split_min": 128}),  # split
          ((6000, 0, 100), np.int32, {})]                   # split at the default threshold


@pytest.mark.parametrize("shape,vdtype,options", SHAPES)
def test_row_shapes_under_every_path(shape, vdtype, options):
    t, first, second = twin_hubs(*shape)
    h, g = t.graph(vdtype=vdtype, options=options)
    want = {m: t.scores(m, first, second, rows=True) for m in MEASURES}
    for path in PATHS:
        h.set_option("sim_path", path)
        for m in MEASURES:
            same(run(m, h, g, first, second, vdtype), want[m])


def test_complete_graph():
    n = 1500
    s, d = np.nonzero(~np.eye(n, dtype=bool))
    h, g = make_graph(s, d, None, renumber=False, symmetric=True)
    want = np.full(len(s), (n - 2) / n, np.float64).astype(np.float32)
    same(run("jaccard", h, g, s, d), want)
    h.set_option("sim_path", 1)
    same(run("jaccard", h, g, s[:20000], d[:20000]), want[:20000])


def test_complete_bipartite_graph():
    n = 2000
    a, b = np.divmod(np.arange(n * n, dtype=np.int64), n)
    s, d = np.r_[a, b + n], np.r_[b + n, a]
    h, g = make_graph(s, d, None, renumber=False, symmetric=True)
    rng = np.random.default_rng(5)
    left = rng.integers(0, n, 3000)
    other = rng.integers(0, n, 3000)
    first = np.r_[left, left + n, left]
    second = np.r_[other, other + n, other + n]
    want = np.r_[np.ones(6000), np.zeros(3000)].astype(np.float32)
    for path in (0, 3):
        h.set_option("sim_path", path)
        for m in MEASURES:
            same(run(m, h, g, first, second), want)


# ------------------------------------------------------------------ 4. R-MAT
@functools.lru_cache(maxsize=None)
def rmat_edges(scale, edges, seed):
    from oracle import rmat
    return rmat.rmat(scale, edges, seed=seed)


@pytest.mark.parametrize("renumber", [True, False])
def test_rmat(renumber):
    s, d = rmat_edges(12, 16 << 12, 7)
    t = Truth(s, d, renumber)
    h, g = t.graph()
    ra, rb = random_pairs(t, 10000, 3)
    first, second = np.r_[t.s, ra], np.r_[t.d, rb]
    for m in MEASURES:
        x = run(m, h, g, first, second)
        same(x, t.scores(m, first, second))
        same(run(m, h, g, first, second), x)  # the second call reads the cached degrees


# ------------------------------------------------------------------ 5. edge cases
def test_repeated_entries_and_self_loops():
    # 0: {0 (loop), 1, 2, 2}, 1: {0, 2}, 2: {0, 0, 1}; not symmetrised by the caller's hand: listed both ways
    s = [0, 0, 0, 0, 1, 1, 2, 2, 2]
    d = [0, 1, 2, 2, 0, 2, 0, 0, 1]
    h, g = make_graph(s, d, None, renumber=False, symmetric=True)
    first, second = [0, 0, 1, 0, 1], [1, 2, 2, 0, 1]
    # N(0) = {0, 1, 2}, N(1) = {0, 2}, N(2) = {0, 1}
    c, du, dv = [2, 2, 1, 3, 2], [3, 3, 2, 3, 2], [2, 2, 2, 3, 2]
    for path in PATHS:
        h.set_option("sim_path", path)
        for m in MEASURES:
            same(run(m, h, g, first, second), score(m, c, du, dv))
    assert run("jaccard", h, g, [0, 1], [0, 1]).tolist() == [1.0, 1.0]  # (u, u)


def test_isolated_and_unknown_ids_score_zero():
    h, g = make_graph([0, 1, 5, 6], [1, 0, 6, 5], None, renumber=False, symmetric=True)  # 2, 3, 4 have no edges
    first, second = [0, 2, 3, 0, 77, 0, 5], [2, 0, 3, 77, 78, -4, 6]
    for m in MEASURES:
        assert run(m, h, g, first, second).tolist() == [0.0] * 7
    h2, g2 = make_graph([10, 20], [20, 10], None, renumber=True, symmetric=True)
    for m in MEASURES:
        assert run(m, h2, g2, [10, 15, 10], [15, 20, 10]).tolist() == [0.0, 0.0, 1.0]
    for hh, gg, a, b in ((h, g, [0, 77], [1, 0]), (h2, g2, [10, 10], [20, 15])):
        with pytest.raises(ValueError, match="invalid vertex IDs"):
            run("jaccard", hh, gg, a, b, expensive=True)
    assert run("jaccard", h2, g2, [10], [20], expensive=True).tolist() == [0.0]


def test_empty_duplicate_and_ordered_pairs():
    t = dataset("karate")
    h, g = t.graph()
    for m in MEASURES:
        x = run(m, h, g, [], [])
        assert len(x) == 0 and x.dtype == np.float32
    first, second = [0, 33, 0, 1, 0, 33], [1, 32, 1, 0, 1, 32]
    x = run("jaccard", h, g, first, second)
    same(x, t.scores("jaccard", first, second))
    assert x[0] == x[2] == x[3] == x[4] and x[1] == x[5] and x[0] != x[1]


def test_refusals():
    p = plc()
    v = vectors()
    h, g = make_graph(v["src"], v["dst"], None, symmetric=True)
    with pytest.raises(ValueError, match="vertex type of graph and first must match"):
        p.jaccard_coefficients(h, g, np.asarray(v["first"], np.int64), np.asarray(v["second"], np.int32), False, False)
    with pytest.raises(ValueError, match="vertex type of graph and second must match"):
        p.jaccard_coefficients(h, g, np.asarray(v["first"], np.int32), np.asarray(v["second"], np.int64), False, False)
    with pytest.raises(ValueError):
        p.jaccard_coefficients(h, g, np.asarray(v["first"], np.int32), np.asarray(v["second"][:-1], np.int32),
                               False, False)
    for m in MEASURES:
        with pytest.raises(NotImplementedError, match="weighted similarity computations are not supported"):
            run(m, h, g, v["first"], v["second"], use_weight=True)
    h2, g2 = make_graph(v["src"][:8], v["dst"][:8], None, symmetric=False)
    props = p.GraphProperties(is_symmetric=True, is_multigraph=True)
    g3 = p.SGGraph(h, props, np.asarray(v["src"], np.int32), np.asarray(v["dst"], np.int32), None, renumber=True)
    for m in MEASURES:
        with pytest.raises(ValueError, match="undirected graphs only"):
            run(m, h2, g2, v["first"], v["second"])
        with pytest.raises(ValueError, match="multi-graphs"):
            run(m, h, g3, v["first"], v["second"])
    for name, bad in (("sim_path", 4), ("sim_path", -1), ("sim_split_min", 0), ("two_hop_budget", 0)):
        with pytest.raises(ValueError):
            h.set_option(name, bad)


def test_multi_gpu_graph_is_not_implemented():
    """One rank over RCCL, the setup of test_gpu_triangle_count.py's test of the same name."""
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
        for m in MEASURES:
            with pytest.raises(NotImplementedError, match="multi-GPU"):
                getattr(p, m + "_coefficients")(h, g, s[:2], d[:2], False, False)
        with pytest.raises(NotImplementedError, match="multi-GPU"):
            p.get_two_hop_neighbors(h, g)
        g = None
        h = None
    finally:
        torch.cuda.synchronize()
        p.trim_device_cache()
        ctx.free()
        dist.destroy_process_group()


# ------------------------------------------------------------------ 6. two-hop
def two_hop(h, g, start=None, vdtype=np.int32):
    a, b = plc().get_two_hop_neighbors(h, g, None if start is None else np.asarray(start, vdtype))
    a, b = host(a), host(b)
    assert a.dtype == np.dtype(vdtype) and b.dtype == a.dtype and len(a) == len(b)
    return a, b


def as_set(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    assert len(pairs) == len(a), "a pair appears twice"
    return pairs


@pytest.mark.parametrize("vdtype", [np.int32, np.int64])
@pytest.mark.parametrize("renumber", [True, False])
def test_two_hop_golden(renumber, vdtype):
    v = vectors()
    for transposed in (False, True):
        h, g = make_graph(v["src"], v["dst"], None, transposed=transposed, renumber=renumber, symmetric=True,
                          vdtype=vdtype)
        assert as_set(*two_hop(h, g, vdtype=vdtype)) == {tuple(p) for p in v["two_hop"]}


@pytest.mark.parametrize("name,count", [("karate", 664), ("dolphins", 1138), ("polbooks", 3968),
                                        ("netscience", 13002), ("email-Eu-core", 447292)])
def test_two_hop_datasets(name, count):
    t = dataset(name)
    h, g = t.graph()
    a, b = two_hop(h, g)
    assert len(a) == count
    got = as_set(a, b)
    assert got == t.two_hop()
    if name == "karate":
        adjacent = set(zip(t.s.tolist(), t.d.tolist()))
        assert len(got - adjacent) == 530
    a2, b2 = two_hop(h, g)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)  # the same order from call to call


@pytest.mark.parametrize("renumber", [True, False])
def test_two_hop_rmat(renumber):
    s, d = rmat_edges(10, 16 << 10, 7)
    t = Truth(s, d, renumber)
    h, g = t.graph()
    assert as_set(*two_hop(h, g)) == t.two_hop()
    # a few start vertices, one of them twice, one without edges when the ids are not renumbered
    start = [int(t.ids[0]), int(t.ids[5]), int(t.ids[-1]), int(t.ids[5])]
    want = {p for p in t.two_hop() if p[0] in start}
    assert as_set(*two_hop(h, g, start)) == want
    h.set_option("two_hop_budget", 4096)
    assert as_set(*two_hop(h, g)) == t.two_hop()


def test_two_hop_star_and_budget():
    n = 5000  # leaves 1 .. n around hub 0: every leaf-leaf pair comes from the hub's row
    leaves = np.arange(1, n + 1)
    t = Truth(np.zeros(n, np.int64), leaves, False)
    h, g = t.graph()
    a, b = two_hop(h, g)
    assert len(a) == n * (n - 1)
    assert not (a == 0).any() and not (b == 0).any() and not (a == b).any()
    key = a.astype(np.int64) * (n + 1) + b
    assert (np.diff(key) > 0).all() or len(np.unique(key)) == len(key)  # no pair twice
    # batches of at most 1024 walks: every leaf's 5000 walks are above it
    h.set_option("two_hop_budget", 1024)
    a2, b2 = two_hop(h, g)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    sa, sb = two_hop(h, g, [7, 7, 0, 4999])
    assert as_set(sa, sb) == {(u, int(x)) for u in (7, 4999) for x in leaves if x != u}


def test_two_hop_start_errors_and_directed_path():
    v = vectors()
    h, g = make_graph(v["src"], v["dst"], None, renumber=True, symmetric=True)
    for bad in ([0, 9], [-1]):
        with pytest.raises(ValueError):
            two_hop(h, g, bad)
    a, b = two_hop(h, g, [])
    assert len(a) == 0
    a, b = two_hop(h, g, [3, 3, 0, 3])
    assert as_set(a, b) == {tuple(p) for p in v["two_hop"] if p[0] in (0, 3)}
    for renumber in (True, False):
        for transposed in (False, True):
            h2, g2 = make_graph([0, 1], [1, 2], None, transposed=transposed, renumber=renumber, symmetric=False)
            assert as_set(*two_hop(h2, g2)) == {(0, 2)}


# ------------------------------------------------------------------ 7. the cugraph layer
@functools.lru_cache(maxsize=None)
def karate_graph():
    import cugraph
    import pandas as pd
    t = dataset("karate")
    G = cugraph.Graph()
    G.from_pandas_edgelist(pd.DataFrame({"s": t.s, "d": t.d}), "s", "d")
    return G


@pytest.mark.parametrize("measure", MEASURES)
def test_cugraph_all_edges_and_given_pairs(measure):
    import cugraph
    import pandas as pd
    t, G = dataset("karate"), karate_graph()
    f = getattr(cugraph, measure)
    col = measure + "_coeff"
    df = f(G)
    assert list(df.columns) == ["source", "destination", col]
    order = np.lexsort((t.d, t.s))
    assert np.array_equal(df["source"].to_numpy(), t.s[order]) and np.array_equal(df["destination"].to_numpy(), t.d[order])
    assert df["source"].dtype == np.int32 and df[col].dtype == np.float32
    same(df[col].to_numpy(), t.scores(measure, t.s[order], t.d[order]))
    pairs = pd.DataFrame({"a": [33, 0, 5, 33, 0], "b": [0, 33, 16, 0, 0], "ignored": [1, 2, 3, 4, 5]})
    df = f(G, pairs)
    assert list(df.columns) == ["source", "destination", col] and len(df) == 5
    assert df["source"].tolist() == [33, 0, 5, 33, 0] and df["destination"].tolist() == [0, 33, 16, 0, 0]
    same(df[col].to_numpy(), t.scores(measure, pairs["a"], pairs["b"]))
    same(getattr(cugraph, measure + "_coefficient")(G, [(33, 0), (0, 33)])[col].to_numpy(), df[col].to_numpy()[:2])


def test_cugraph_networkx_input_on_two_hop_pairs():
    import cugraph
    import networkx as nx
    t, G = dataset("karate"), karate_graph()
    hop = G.get_two_hop_neighbors()
    assert list(hop.columns) == ["first", "second"] and len(hop) == 664
    assert hop.equals(hop.sort_values(["first", "second"]).reset_index(drop=True))
    assert set(zip(hop["first"].tolist(), hop["second"].tolist())) == t.two_hop()
    some = G.get_two_hop_neighbors([0, 33])
    assert set(some["first"].tolist()) == {0, 33} and len(some) == int(hop["first"].isin([0, 33]).sum())
    N = nx.Graph()
    N.add_edges_from((f"n{u}", f"n{v}") for u, v in zip(t.s.tolist(), t.d.tolist()))
    ebunch = [(f"n{u}", f"n{v}") for u, v in zip(hop["first"].tolist(), hop["second"].tolist())]
    got = cugraph.jaccard_coefficient(N, ebunch)
    want = {(u, v): p for u, v, p in nx.jaccard_coefficient(N, ebunch)}
    assert set(got) == set(want) and len(got) == 664
    for k, p in want.items():
        assert got[k] == float(np.float32(p)), k
    every = cugraph.sorensen_coefficient(N)
    assert len(every) == 156 and all(isinstance(k, tuple) for k in every)
