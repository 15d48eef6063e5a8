"""Betweenness and edge betweenness centrality on the GPU (csrc/betweenness.hip through the C ABI and the
Python layers) against NetworkX, or against the numpy twin tests/betweenness_ref.py where the sources are a
list (NetworkX draws its own) or the graph has parallel edges.

Tolerances: non-zero scores within rtol 1e-10 (the twin and NetworkX agree within 1.4e-14 on these graphs,
all terms are non-negative, so there is no cancellation); a score that is 0 in the truth must be exactly
0; float32 results within rtol 1e-6 (one rounding).  Bit-equality is np.array_equal on the float64 values.

NetworkX's results for email-Eu-core are read from tests/golden/betweenness_email_nx.npz
(scripts/make_betweenness_golden.py): one call takes 5 to 9 seconds."""
import functools
import os

import numpy as np
import pytest

import betweenness_ref as ref
from conftest import GOLDEN, dataset_path
from gpu_util import host, make_graph, plc

pytestmark = pytest.mark.gpu

RTOL = 1e-10
UNDIRECTED = ["karate.csv", "dolphins.csv", "polbooks.csv", "netscience.csv"]
DIRECTED = ["email-Eu-core.csv", "karate-asymmetric.csv"]


def assert_scores(got, want, rtol=RTOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    zero = want == 0
    assert (got[zero] == 0).all(), "a score that is 0 in the truth is not exactly 0"
    err = np.abs(got[~zero] - want[~zero]) / want[~zero]
    worst = float(err.max()) if err.size else 0.0
    print(f"max relative error {worst:.3e} over {err.size} non-zero scores")
    assert worst <= rtol


# ------------------------------------------------------------------ cases
class Case:
    """The stored edges of a graph (both directions when symmetric), the ids it reports, and the edges in
    compact ids 0 .. n - 1 (positions in ``ids``) for the twin."""

    def __init__(self, s, d, symmetric, renumber=True, vdtype=np.int32):
        self.s, self.d = np.asarray(s, np.int64), np.asarray(d, np.int64)
        self.symmetric, self.renumber, self.vdtype = symmetric, renumber, vdtype
        self.ids = np.unique(np.r_[self.s, self.d]) if renumber else np.arange(int(max(self.s.max(), self.d.max())) + 1)
        self.n = len(self.ids)
        self.cs, self.cd = np.searchsorted(self.ids, self.s), np.searchsorted(self.ids, self.d)

    def graph(self, transposed=False, options=None):
        return make_graph(self.s, self.d, None, transposed=transposed, renumber=self.renumber,
                          symmetric=self.symmetric, vdtype=self.vdtype, options=options)

    def positions(self, sources):
        return None if sources is None else np.searchsorted(self.ids, np.asarray(sources, np.int64))

    def twin(self, sources=None, normalized=True, endpoints=False):
        return ref.betweenness(self.n, self.cs, self.cd, self.positions(sources), self.symmetric, normalized, endpoints)

    def twin_edges(self, sources=None, normalized=True):
        """{(src id, dst id): [scores of the stored entries of that pair]}"""
        row, col, x = ref.edge_betweenness(self.n, self.cs, self.cd, self.positions(sources), self.symmetric,
                                           normalized)
        return self.ids[row], self.ids[col], x

    def vertex_scores(self, h, g, k=None, normalized=True, endpoints=False):
        """The scores by position in ``ids``."""
        src = None if k is None else np.asarray(k, self.vdtype)
        vertices, values = plc().betweenness_centrality(h, g, src, None, normalized, endpoints, False)
        v, x = host(vertices), host(values)
        assert v.dtype == np.dtype(self.vdtype) and x.dtype == np.float64
        assert np.array_equal(np.sort(v), self.ids), "vertices is not a permutation of the graph's ids"
        out = np.empty(self.n, np.float64)
        out[np.searchsorted(self.ids, v)] = x
        return out

    def edge_scores(self, h, g, k=None, normalized=True):
        """(src, dst, values) sorted by (src, dst); entries of one pair keep their order."""
        src = None if k is None else np.asarray(k, self.vdtype)
        s, d, x = (host(t) for t in plc().edge_betweenness_centrality(h, g, src, None, normalized, False))
        assert s.dtype == np.dtype(self.vdtype) and d.dtype == s.dtype and x.dtype == np.float64
        assert len(s) == len(self.s) and len(d) == len(s) and len(x) == len(s)
        order = np.lexsort((d, s))  # stable
        return s[order], d[order], x[order]


def symmetrized(s, d):
    p = np.unique(np.r_[np.c_[s, d], np.c_[d, s]], axis=0)
    return p[:, 0], p[:, 1]


def dataset_edges(name):
    e = np.loadtxt(dataset_path(name), usecols=(0, 1), dtype=np.int64)
    return e[:, 0], e[:, 1]


@functools.lru_cache(maxsize=None)
def dataset(name):
    s, d = dataset_edges(name)
    if name in DIRECTED:
        p = np.unique(np.c_[s, d], axis=0)
        return Case(p[:, 0], p[:, 1], symmetric=False)
    return Case(*symmetrized(s, d), symmetric=True)


@functools.lru_cache(maxsize=None)
def nx_graph(name):
    import networkx as nx
    c = dataset(name)
    G = nx.Graph() if c.symmetric else nx.DiGraph()
    G.add_nodes_from(c.ids.tolist())
    G.add_edges_from(zip(c.s.tolist(), c.d.tolist()))
    return G


@functools.lru_cache(maxsize=None)
def email_golden():
    return np.load(os.path.join(GOLDEN, "betweenness_email_nx.npz"))


@functools.lru_cache(maxsize=None)
def nx_vertex(name, normalized, endpoints):
    if name == "email-Eu-core.csv":
        return email_golden()[f"bc_n{int(normalized)}_e{int(endpoints)}"]
    import networkx as nx
    bc = nx.betweenness_centrality(nx_graph(name), normalized=normalized, endpoints=endpoints)
    return np.array([bc[int(i)] for i in dataset(name).ids])


@functools.lru_cache(maxsize=None)
def nx_edges(name, normalized):
    """By distinct pair in ascending (src, dst) order: directed pairs, or the undirected pairs src < dst."""
    c = dataset(name)
    if name == "email-Eu-core.csv":
        return email_golden()[f"ebc_n{int(normalized)}"]
    import networkx as nx
    ebc = nx.edge_betweenness_centrality(nx_graph(name), normalized=normalized)
    keep = np.ones(len(c.s), bool) if not c.symmetric else c.s <= c.d
    return np.array([ebc[(a, b)] if (a, b) in ebc else ebc[(b, a)] for a, b in zip(c.s[keep].tolist(), c.d[keep].tolist())])


# ------------------------------------------------------------------ 1. all sources against NetworkX
@pytest.mark.parametrize("endpoints", [False, True])
@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("name", UNDIRECTED + DIRECTED)
def test_all_sources_against_networkx(name, normalized, endpoints):
    c = dataset(name)
    h, g = c.graph()
    assert_scores(c.vertex_scores(h, g, None, normalized, endpoints), nx_vertex(name, normalized, endpoints))
    assert h.last_iterations() == (c.n + 63) // 64


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("name", UNDIRECTED + DIRECTED)
def test_edge_scores_against_networkx(name, normalized):
    c = dataset(name)
    h, g = c.graph()
    s, d, x = c.edge_scores(h, g, None, normalized)
    order = np.lexsort((c.d, c.s))
    assert np.array_equal(s, c.s[order]) and np.array_equal(d, c.d[order])  # the cases' pairs are distinct
    if c.symmetric:  # NetworkX's score of an undirected edge is the sum of its two directions
        lo, hi = np.minimum(s, d), np.maximum(s, d)
        fold = np.lexsort((hi, lo))
        assert np.array_equal(lo[fold][0::2], lo[fold][1::2]) and np.array_equal(hi[fold][0::2], hi[fold][1::2])
        x = x[fold][0::2] + x[fold][1::2]
    assert_scores(x, nx_edges(name, normalized))


def test_netscience_is_disconnected_and_email_has_self_loops():
    import networkx as nx
    assert nx.number_connected_components(nx_graph("netscience.csv")) > 1
    c = dataset("email-Eu-core.csv")
    assert (c.s == c.d).any()


def test_twin_on_a_subset_of_email_sources():
    c = dataset("email-Eu-core.csv")
    src = c.ids[::17]
    h, g = c.graph()
    assert_scores(c.vertex_scores(h, g, src, True, True), c.twin(src, True, True))
    assert_scores(c.edge_scores(h, g, src, False)[2], c.twin_edges(src, False)[2])


# ------------------------------------------------------------------ 2. source lists against the twin
def netscience_sources(count):
    c = dataset("netscience.csv")
    return np.random.default_rng(count).choice(c.ids, size=count, replace=False)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_source_lists(count):
    c = dataset("netscience.csv")
    src = netscience_sources(count)
    h, g = c.graph()
    assert_scores(c.vertex_scores(h, g, src, True, False), c.twin(src, True, False))
    assert h.last_iterations() == (count + 63) // 64
    assert_scores(c.vertex_scores(h, g, src, False, True), c.twin(src, False, True))
    assert_scores(c.edge_scores(h, g, src, True)[2], c.twin_edges(src, True)[2])


def test_a_repeated_source_counts_again():
    c = dataset("netscience.csv")
    src = np.r_[netscience_sources(5), netscience_sources(5)[:2]]
    h, g = c.graph()
    once = c.vertex_scores(h, g, src[:5], False, False)
    twice = c.vertex_scores(h, g, src, False, False)
    assert_scores(twice, c.twin(src, False, False))
    assert not np.array_equal(once * 5 / 7, twice)
    assert_scores(c.edge_scores(h, g, src, False)[2], c.twin_edges(src, False)[2])


def test_an_empty_list_gives_zeros():
    c = dataset("netscience.csv")
    h, g = c.graph()
    for endpoints in (False, True):
        assert (c.vertex_scores(h, g, [], True, endpoints) == 0).all()
    assert (c.edge_scores(h, g, [], True)[2] == 0).all()
    assert h.last_iterations() == 0


def test_every_vertex_as_a_list_equals_no_list_bit_for_bit():
    c = dataset("netscience.csv")
    h, g = c.graph()
    # the graph's own order of the vertices: the order the NULL list stands for
    order = host(plc().betweenness_centrality(h, g, np.empty(0, np.int32), None, True, False, False)[0])
    for endpoints in (False, True):
        assert np.array_equal(c.vertex_scores(h, g, order, True, endpoints), c.vertex_scores(h, g, None, True, endpoints))
    assert np.array_equal(c.edge_scores(h, g, order, True)[2], c.edge_scores(h, g, None, True)[2])


# ------------------------------------------------------------------ 3. determinism
def test_two_calls_are_bit_equal():
    c = dataset("netscience.csv")
    src = netscience_sources(130)
    h, g = c.graph()
    h2, g2 = c.graph()
    a = c.vertex_scores(h, g, src, True, True)
    assert np.array_equal(a, c.vertex_scores(h, g, src, True, True))
    assert np.array_equal(a, c.vertex_scores(h2, g2, src, True, True))
    e = c.edge_scores(h, g, src, True)[2]
    assert np.array_equal(e, c.edge_scores(h, g, src, True)[2])
    assert np.array_equal(e, c.edge_scores(h2, g2, src, True)[2])


@pytest.mark.parametrize("name", ["netscience.csv", "email-Eu-core.csv"])
def test_batch_size_and_row_split_change_no_vertex_score_bit(name):
    """email-Eu-core has rows above 64 entries (up to 300 and more): bc_row_split = 64 sends them through the
    segments, 2048 does not."""
    c = dataset(name)
    src = c.ids[::3][:130]
    base = edges = None
    for options in ({"bc_batch": 64, "bc_row_split": 2048}, {"bc_batch": 1}, {"bc_batch": 7}, {"bc_row_split": 64},
                    {"bc_batch": 7, "bc_row_split": 64}):
        h, g = c.graph(options=options)
        got = c.vertex_scores(h, g, src, True, True)
        assert h.last_iterations() == -(-len(src) // options.get("bc_batch", 64))
        e = c.edge_scores(h, g, src, True)[2]
        if base is None:
            base, edges = got, e
            assert_scores(base, c.twin(src, True, True))
        assert np.array_equal(got, base), options
        if "bc_batch" not in options or options["bc_batch"] == 64:
            assert np.array_equal(e, edges), options  # the cut changes no edge score bit either
        assert_scores(e, edges)  # across batch sizes: the lanes of a batch are added first


def test_options_are_range_checked():
    h = plc().ResourceHandle()
    for name, bad in (("bc_batch", 0), ("bc_batch", 65), ("bc_batch", 1.5), ("bc_row_split", 63),
                      ("bc_row_split", 100), ("bc_row_split", 0)):
        with pytest.raises(ValueError, match=name):
            h.set_option(name, bad)
    for name, good in (("bc_batch", 1), ("bc_batch", 64), ("bc_row_split", 64), ("bc_row_split", 4096)):
        h.set_option(name, good)


# ------------------------------------------------------------------ 4. shapes where the kernel can go wrong
def path_case(n):
    p = np.arange(n - 1)
    return Case(np.r_[p, p + 1], np.r_[p + 1, p], symmetric=True)


def test_long_path_depth_above_255():
    n = 300
    c = path_case(n)
    h, g = c.graph()
    i = np.arange(n, dtype=np.float64)
    got = c.vertex_scores(h, g, [0], False, False)  # one source: vertex i lies before n - 1 - i others
    assert_scores(got, np.r_[0.0, (n - 1 - i[1:])] / 2 * n)
    assert_scores(got, c.twin([0], False, False))
    assert_scores(c.vertex_scores(h, g, None, False, False), i * (n - 1 - i))  # every source: exact integers
    assert_scores(c.vertex_scores(h, g, None, False, False), c.twin(None, False, False))
    s, d, x = c.edge_scores(h, g, None, False)
    lo = np.minimum(s, d).astype(np.float64)
    assert_scores(x, (lo + 1) * (n - 1 - lo) / 2)


def test_chain_of_diamonds_path_counts_above_32_bits():
    """40 diamonds a - (b | c) - a': 2^40 shortest paths from one end to the other."""
    m = 40
    s, d = [], []
    for i in range(m):
        a, b, cc, a2 = 3 * i, 3 * i + 1, 3 * i + 2, 3 * i + 3
        s += [a, a, b, cc]
        d += [b, cc, a2, a2]
    c = Case(*symmetrized(np.array(s), np.array(d)), symmetric=True)
    h, g = c.graph()
    for k in ([0], [0, 3 * m], None):
        assert_scores(c.vertex_scores(h, g, k, False, False), c.twin(k, False, False))
    # from one end, directed: joint i (vertex 3 i) lies on every path to the 3 (m - i) vertices after it
    cdir = Case(np.array(s), np.array(d), symmetric=False)
    h, g = cdir.graph()
    got = cdir.vertex_scores(h, g, [0], False, False)
    joints = np.arange(1, m)
    assert_scores(got[3 * joints], 3.0 * (m - joints))
    assert_scores(c.edge_scores(*c.graph(), [0], False)[2], c.twin_edges([0], False)[2])


@functools.lru_cache(maxsize=None)
def star_ring():
    """A hub (id 0) with 300 leaves and a ring through the leaves."""
    leaves = 1 + np.arange(300)
    s = np.r_[np.zeros(300, np.int64), leaves]
    d = np.r_[leaves, np.roll(leaves, -1)]
    return Case(*symmetrized(s, d), symmetric=True)


@pytest.mark.parametrize("renumber", [True, False])
def test_hub_row_in_segments(renumber):
    """bc_row_split = 64: the hub's row of 300 entries is 5 segments (the last of 44)."""
    base = star_ring()
    c = Case(base.s, base.d, True, renumber=renumber)
    h, g = c.graph(options={"bc_row_split": 64})
    h0, g0 = c.graph()
    for k in (None, [5, 17, 0, 200]):
        for endpoints in (False, True):
            got = c.vertex_scores(h, g, k, True, endpoints)
            assert_scores(got, c.twin(k, True, endpoints))
            assert np.array_equal(got, c.vertex_scores(h0, g0, k, True, endpoints))
        e = c.edge_scores(h, g, k, False)[2]
        assert_scores(e, c.twin_edges(k, False)[2])
        assert np.array_equal(e, c.edge_scores(h0, g0, k, False)[2])


def test_directed_hub_rows_in_both_orientations():
    """Out-star into a hub and in-star out of it: the in-row (count) and the out-row (discover, back) of
    vertex 0 are both cut."""
    a, b = 1 + np.arange(200), 201 + np.arange(150)
    s = np.r_[a, np.zeros(150, np.int64), a[:-1]]
    d = np.r_[np.zeros(200, np.int64), b, a[1:]]
    c = Case(s, d, symmetric=False)
    for transposed in (False, True):
        h, g = c.graph(transposed, options={"bc_row_split": 64})
        assert_scores(c.vertex_scores(h, g, None, False, True), c.twin(None, False, True))
        assert_scores(c.edge_scores(h, g, None, True)[2], c.twin_edges(None, True)[2])


def test_ids_without_edges_score_zero_and_reach_nothing():
    s, d = symmetrized(np.array([3, 4, 7, 12]), np.array([4, 7, 9, 15]))
    c = Case(s, d, symmetric=True, renumber=False)
    assert c.n == 16
    h, g = c.graph()
    for endpoints in (False, True):
        got = c.vertex_scores(h, g, None, False, endpoints)
        assert_scores(got, c.twin(None, False, endpoints))
        assert (got[[0, 1, 2, 5, 6, 8, 10, 11, 13, 14]] == 0).all()
    # as sources they reach nothing: only source 3 counts, the factor n / k still has k = 3
    assert_scores(c.vertex_scores(h, g, [0, 3, 13], False, True), c.twin([0, 3, 13], False, True))
    assert (c.vertex_scores(h, g, [0, 13], True, True) == 0).all()


def multigraph(s, d, symmetric):
    p = plc()
    h = p.ResourceHandle()
    g = p.SGGraph(h, p.GraphProperties(is_symmetric=symmetric, is_multigraph=True), np.asarray(s, np.int32),
                  np.asarray(d, np.int32), None, store_transposed=False, renumber=True)
    return h, g


def test_self_loops_and_parallel_edges():
    """Parallel edges are distinct paths, self-loops contribute nothing (pylibcugraph level: cugraph.Graph
    drops repeated edges)."""
    s = np.array([0, 0, 1, 1, 1, 2, 2, 3, 0, 4, 4])
    d = np.array([1, 1, 2, 1, 3, 4, 4, 4, 0, 5, 4])
    c = Case(s, d, symmetric=False)
    h, g = multigraph(s, d, False)
    for k in (None, [0], [1, 0]):
        assert_scores(c.vertex_scores(h, g, k, False, False), c.twin(k, False, False))
        got = c.edge_scores(h, g, k, False)
        row, col, want = c.twin_edges(k, False)
        assert np.array_equal(got[0], row) and np.array_equal(got[1], col)
        assert_scores(got[2], want)
    loops = got[0] == got[1]
    assert loops.sum() == 3 and (got[2][loops] == 0).all()
    # the undirected multigraph: both directions of every entry
    s2, d2 = np.r_[s, d], np.r_[d, s]
    c2 = Case(s2, d2, symmetric=True)
    h, g = multigraph(s2, d2, True)
    assert_scores(c2.vertex_scores(h, g, None, True, True), c2.twin(None, True, True))
    assert_scores(c2.edge_scores(h, g, None, True)[2], c2.twin_edges(None, True)[2])


@pytest.mark.parametrize("name", ["karate.csv", "karate-asymmetric.csv", "email-Eu-core.csv"])
def test_store_transposed_gives_the_same_scores(name):
    c = dataset(name)
    h, g = c.graph(False)
    ht, gt = c.graph(True)
    src = c.ids[::5]
    for k in (None, src):  # (the two graphs may number their vertices differently: another order of the sums)
        assert_scores(c.vertex_scores(ht, gt, k, True, True), c.vertex_scores(h, g, k, True, True))
        a, b = c.edge_scores(ht, gt, k, False), c.edge_scores(h, g, k, False)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert_scores(a[2], b[2])
    assert_scores(c.vertex_scores(ht, gt, src, False, False), c.twin(src, False, False))


@pytest.mark.parametrize("renumber", [True, False])
def test_int64_vertex_ids(renumber):
    base = dataset("karate.csv")
    c = Case(base.s, base.d, True, renumber=renumber, vdtype=np.int64)
    h, g = c.graph()
    assert_scores(c.vertex_scores(h, g, None, True, False), nx_vertex("karate.csv", True, False))
    assert_scores(c.vertex_scores(h, g, [5, 0, 33], False, True), c.twin([5, 0, 33], False, True))
    assert_scores(c.edge_scores(h, g, None, True)[2], c.twin_edges(None, True)[2])
    # ids above 2^31, renumbered
    big = Case(base.s * 1_000_003 + (1 << 33), base.d * 1_000_003 + (1 << 33), True, vdtype=np.int64)
    h, g = big.graph()
    assert_scores(big.vertex_scores(h, g, None, True, False), nx_vertex("karate.csv", True, False))
    src = big.ids[[7, 1]]
    assert_scores(big.edge_scores(h, g, src, False)[2], big.twin_edges(src, False)[2])


def test_profiling_covers_the_sweep():
    c = dataset("email-Eu-core.csv")
    h, g = c.graph()
    h.set_profiling(True)
    c.vertex_scores(h, g, c.ids[:100], True, False)
    assert h.last_iterations() == 2 and h.last_hot_kernel_launches() > 0 and h.last_hot_kernel_ms() > 0


# ------------------------------------------------------------------ 5. errors
def test_unknown_source_id():
    c = Case(1000 + 37 * dataset("karate.csv").s, 1000 + 37 * dataset("karate.csv").d, True)
    h, g = c.graph()
    for unknown in (int(c.ids[0]) + 1, -5, 2 ** 31 - 1):
        src = np.r_[c.ids[:3], unknown].astype(np.int32)
        with pytest.raises(ValueError, match="not in the graph"):
            plc().betweenness_centrality(h, g, src, None, True, False, False)
        with pytest.raises(ValueError, match="not in the graph"):
            plc().edge_betweenness_centrality(h, g, src, None, True, False)
    c = Case(dataset("karate.csv").s, dataset("karate.csv").d, True, renumber=False)
    h, g = c.graph()
    with pytest.raises(ValueError, match="not in the graph"):
        plc().betweenness_centrality(h, g, np.array([0, 34], np.int32), None, True, False, True)


def test_vertex_list_of_another_type():
    c = dataset("karate.csv")
    h, g = c.graph()
    with pytest.raises(ValueError, match="vertex type"):
        plc().betweenness_centrality(h, g, np.array([0, 1], np.int64), None, True, False, False)
    with pytest.raises(ValueError, match="vertex type"):
        plc().edge_betweenness_centrality(h, g, np.array([0, 1], np.int64), None, True, False)
    # plain Python ids take the graph's type
    assert_scores(host(plc().betweenness_centrality(h, g, [0, 1], None, True, False, False)[1]),
                  host(plc().betweenness_centrality(h, g, np.array([0, 1], np.int32), None, True, False, False)[1]))


def test_multi_gpu_graph_is_not_implemented():
    """One rank over RCCL, the setup of test_gpu_core_number.py's test of the same name."""
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
        with pytest.raises(NotImplementedError, match="multi-GPU betweenness centrality"):
            p.betweenness_centrality(h, g, None, None, True, False, False)
        with pytest.raises(NotImplementedError, match="multi-GPU betweenness centrality"):
            p.edge_betweenness_centrality(h, g, None, None, True, False)
        g = None
        h = None
    finally:
        torch.cuda.synchronize()
        p.trim_device_cache()
        ctx.free()
        dist.destroy_process_group()


# ------------------------------------------------------------------ 6. pylibcugraph k and cugraph
def test_k_as_an_int_draws_positions_of_the_vertices_order():
    import random
    c = dataset("netscience.csv")
    h, g = c.graph()
    p = plc()
    order = host(p.betweenness_centrality(h, g, [], None, True, False, False)[0])
    want_src = order[random.Random(11).sample(range(c.n), 20)]
    v, x = p.betweenness_centrality(h, g, 20, 11, True, False, False)
    v2, x2 = p.betweenness_centrality(h, g, want_src.astype(np.int32), None, True, False, False)
    assert np.array_equal(host(x), host(x2)) and np.array_equal(host(v), host(v2))
    assert np.array_equal(host(p.betweenness_centrality(h, g, 20, 11, True, False, False)[1]), host(x))
    assert not np.array_equal(host(p.betweenness_centrality(h, g, 20, 12, True, False, False)[1]), host(x))
    e = host(p.edge_betweenness_centrality(h, g, 20, 11, False, False)[2])
    assert np.array_equal(e, host(p.edge_betweenness_centrality(h, g, want_src.astype(np.int32), None, False, False)[2]))
    # k = n draws every vertex once: the scores of k = None up to the order of the sums
    assert_scores(host(p.betweenness_centrality(h, g, c.n, 3, True, False, False)[1]),
                  host(p.betweenness_centrality(h, g, None, None, True, False, False)[1]))
    with pytest.raises(ValueError, match="'k' must be in"):
        p.betweenness_centrality(h, g, c.n + 1, 0, True, False, False)


def cugraph_graph(name):
    import cugraph
    import pandas as pd
    s, d = dataset_edges(name)
    G = cugraph.Graph(directed=name in DIRECTED)
    G.from_pandas_edgelist(pd.DataFrame({"s": s, "d": d}), "s", "d")
    return G


@pytest.mark.parametrize("name", ["karate.csv", "karate-asymmetric.csv"])
def test_cugraph_betweenness_centrality(name):
    import cugraph
    c = dataset(name)
    G = cugraph_graph(name)
    for normalized, endpoints in ((True, False), (False, True)):
        df = cugraph.betweenness_centrality(G, normalized=normalized, endpoints=endpoints)
        assert list(df.columns) == ["vertex", "betweenness_centrality"] and len(df) == c.n
        assert df["betweenness_centrality"].dtype == np.float64
        got = df.sort_values("vertex")["betweenness_centrality"].to_numpy()
        assert_scores(got, nx_vertex(name, normalized, endpoints))
    df32 = cugraph.betweenness_centrality(G, result_dtype=np.float32)
    assert df32["betweenness_centrality"].dtype == np.float32
    assert_scores(df32.sort_values("vertex")["betweenness_centrality"].to_numpy(), nx_vertex(name, True, False), 1e-6)
    # k as a list of identifiers
    src = [int(c.ids[3]), int(c.ids[0]), int(c.ids[9])]
    df = cugraph.betweenness_centrality(G, k=src, normalized=False)
    assert_scores(df.sort_values("vertex")["betweenness_centrality"].to_numpy(), c.twin(src, False, False))
    with pytest.raises(ValueError, match="not in the graph"):
        cugraph.betweenness_centrality(G, k=[int(c.ids[0]), 10_000])


def test_cugraph_k_int_and_seed():
    import cugraph
    G = cugraph_graph("netscience.csv")
    n = G.number_of_vertices()

    def scores(**kw):
        return cugraph.betweenness_centrality(G, **kw).sort_values("vertex")["betweenness_centrality"].to_numpy()

    a = scores(k=25, seed=4)
    assert np.array_equal(a, scores(k=25, seed=4)) and not np.array_equal(a, scores(k=25, seed=5))
    assert_scores(scores(k=n, seed=1), scores())  # k = n as an int: every vertex, in another order
    e = cugraph.edge_betweenness_centrality(G, k=25, seed=4)
    assert e.equals(cugraph.edge_betweenness_centrality(G, k=25, seed=4))


def test_cugraph_weight_and_result_dtype():
    import cugraph
    G = cugraph_graph("karate.csv")
    for f in (cugraph.betweenness_centrality, cugraph.edge_betweenness_centrality):
        with pytest.raises(NotImplementedError, match="not currently supported"):
            f(G, weight="weights")
        with pytest.raises(TypeError, match="np.float32 or np.float64"):
            f(G, result_dtype=np.int64)


@pytest.mark.parametrize("name", ["karate.csv", "karate-asymmetric.csv"])
def test_cugraph_edge_betweenness_centrality(name):
    import cugraph
    c = dataset(name)
    G = cugraph_graph(name)
    for normalized in (True, False):
        df = cugraph.edge_betweenness_centrality(G, normalized=normalized)
        assert list(df.columns) == ["src", "dst", "betweenness_centrality"]
        if c.symmetric:  # folded: half the stored entries, every row src < dst
            assert len(df) == len(c.s) // 2 and (df["src"] < df["dst"]).all()
        else:
            assert len(df) == len(c.s)
        df = df.sort_values(["src", "dst"])
        assert_scores(df["betweenness_centrality"].to_numpy(), nx_edges(name, normalized))
    df32 = cugraph.edge_betweenness_centrality(G, result_dtype=np.float32).sort_values(["src", "dst"])
    assert df32["betweenness_centrality"].dtype == np.float32
    assert_scores(df32["betweenness_centrality"].to_numpy(), nx_edges(name, True), 1e-6)


def test_networkx_input_returns_dicts():
    import cugraph
    import networkx as nx
    G = nx_graph("karate.csv")
    bc = cugraph.betweenness_centrality(G, endpoints=True)
    want = nx.betweenness_centrality(G, endpoints=True)
    assert isinstance(bc, dict) and set(bc) == set(want)
    keys = sorted(want)
    assert_scores([bc[k] for k in keys], [want[k] for k in keys])
    ebc = cugraph.edge_betweenness_centrality(G, normalized=False)
    want = nx.edge_betweenness_centrality(G, normalized=False)
    assert isinstance(ebc, dict) and len(ebc) == len(want)
    pairs = sorted((min(a, b), max(a, b)) for a, b in want)
    assert sorted(ebc) == pairs
    assert_scores([ebc[p] for p in pairs], [want[p] if p in want else want[(p[1], p[0])] for p in pairs])
    # a list of node labels as k
    src = [3, 0, 9]
    got = cugraph.betweenness_centrality(G, k=src, normalized=False)
    c = dataset("karate.csv")
    assert_scores([got[int(i)] for i in c.ids], c.twin(src, False, False))
