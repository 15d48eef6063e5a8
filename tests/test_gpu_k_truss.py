"""k-truss on the GPU (csrc/k_truss.hip through the C ABI and the Python layers) against the CPU twin
(tests/k_truss_ref.py, itself checked against networkx.k_truss in tests/test_k_truss_api.py),
networkx.k_truss, or a closed form.

Every comparison is exact.  check() compares the surviving pairs as sorted (src, dst) lists with both
directions of every expected edge present exactly once, the dtypes, the offsets pair, the weights by
pair bit for bit, and ``ResourceHandle.last_iterations()`` with the twin's count of non-empty rounds.

The closed forms sit on the paths of the kernels: rows of 63 / 64 / 65 entries around the thread / wave
cut, 511 .. 513 and 1023 .. 1025 around the LDS stage of 8- and 4-byte ids and the split tier's cut
(kKtSplitMin 1024 entries), 5000 for an edge of several segments."""
import functools

import numpy as np
import pytest

from conftest import dataset_path
from gpu_util import host, make_graph, plc
from k_truss_ref import directed_pairs, k_truss, simple_edges

pytestmark = pytest.mark.gpu

DATASETS = ["karate.csv", "dolphins.csv", "polbooks.csv", "netscience.csv", "email-Eu-core.csv"]


# ------------------------------------------------------------------ helpers
def pair_weight(s, d):
    """A weight that depends on the unordered pair alone, exact in float32."""
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    return 0.5 + ((np.minimum(s, d) * 31 + np.maximum(s, d) * 17) % 4093) / 8.0


def both_ways(edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    return np.r_[e[:, 0], e[:, 1]], np.r_[e[:, 1], e[:, 0]]


@functools.lru_cache(maxsize=None)
def twin(key, k):
    """The twin's (edges, rounds) of a named graph, computed once and shared."""
    return k_truss(*GRAPHS[key](), k)


def expected(s, d, k, key=None):
    return twin(key, k) if key is not None else k_truss(s, d, k)


def call(s, d, k, w=None, options=None, **kw):
    h, g = make_graph(s, d, w, symmetric=True, options=options, **kw)
    return h, g, plc().k_truss_subgraph(h, g, k, False)


def check(h, result, want_edges, want_rounds, vdtype=np.int32, weight_of=None, wdtype=None, ids=lambda x: x):
    src, dst, w, off = result
    s, d = host(src), host(dst)
    assert s.dtype == np.dtype(vdtype) and d.dtype == s.dtype and len(s) == len(d)
    got = list(zip(s.tolist(), d.tolist()))
    assert len(set(got)) == len(got), "an entry was emitted twice"
    want = np.asarray(want_edges, np.int64).reshape(-1, 2)
    assert sorted(got) == directed_pairs(np.stack([ids(want[:, 0]), ids(want[:, 1])], axis=1))
    assert host(off).dtype == np.int64 and host(off).tolist() == [0, len(s)]
    if weight_of is None:
        assert w is None
    else:
        assert w is not None and host(w).dtype == np.dtype(wdtype) and len(host(w)) == len(s)
        assert np.array_equal(host(w).view(np.uint8), weight_of(s, d).astype(wdtype).view(np.uint8))
    assert h.last_iterations() == want_rounds
    return got


def run(s, d, k, key=None, weighted=False, wdtype=np.float32, options=None, ids=lambda x: x, **kw):
    """One graph, one call, checked against the twin.  ids maps the twin's ids to the graph's."""
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    edges, rounds = expected(s, d, k, key)
    w = pair_weight(s, d).astype(wdtype) if weighted else None
    h, g, res = call(ids(s), ids(d), k, w, options=options, wdtype=wdtype, **kw)
    inv = None
    if weighted:
        inv = lambda a, b: pair_weight(unmap(a, ids, s, d), unmap(b, ids, s, d))
    got = check(h, res, edges, rounds, vdtype=kw.get("vdtype", np.int32), weight_of=inv, wdtype=wdtype, ids=ids)
    return h, g, res, got


def unmap(a, ids, s, d):
    """The twin's id of every graph id in a."""
    base = np.unique(np.r_[s, d])
    mapped = ids(base)
    order = np.argsort(mapped)
    return base[order][np.searchsorted(mapped[order], a)]


# ------------------------------------------------------------------ the graphs
def complete(n, first=0):
    return [(first + a, first + b) for a in range(n) for b in range(a + 1, n)]


def book(n, groups=0):
    """Spine {0, 1} and pages 2 .. n + 1 adjacent to both; the first 5 * groups pages form disjoint K5s."""
    e = [(0, 1)] + [(0, p) for p in range(2, n + 2)] + [(1, p) for p in range(2, n + 2)]
    for g in range(groups):
        e += complete(5, 2 + 5 * g)
    return e


@functools.lru_cache(maxsize=None)
def dataset(name):
    """The file's simple graph, both directions, with the file's weight of each pair's first row."""
    data = np.loadtxt(dataset_path(name), dtype=np.float64, ndmin=2)
    a, b, w = data[:, 0].astype(np.int64), data[:, 1].astype(np.int64), data[:, 2]
    first = {}
    for x, y, z in zip(a.tolist(), b.tolist(), w.tolist()):
        if x != y:
            first.setdefault((min(x, y), max(x, y)), z)
    e = np.array(sorted(first), np.int64)
    s, d = both_ways(e)
    ww = np.array([first[(min(x, y), max(x, y))] for x, y in zip(s.tolist(), d.tolist())], np.float32)
    return s, d, ww


def dataset_sd(name):
    return dataset(name)[:2]


@functools.lru_cache(maxsize=None)
def gnp():
    import networkx as nx
    return both_ways(np.array(nx.gnp_random_graph(300, 0.08, seed=1).edges(), np.int64))


GRAPHS = {name: functools.partial(dataset_sd, name) for name in DATASETS}
GRAPHS["gnp"] = gnp
GRAPHS["grouped"] = lambda: both_ways(book(1100, 3))
GRAPHS["karate"] = GRAPHS["karate.csv"]
GRAPHS["polbooks"] = GRAPHS["polbooks.csv"]


# ------------------------------------------------------------------ 1. closed forms
def test_empty_edge_list():
    for k in (0, 3):
        h, g, res = call([], [], k)
        check(h, res, [], 0)


@pytest.mark.parametrize("name,edges", [
    ("path", [(i, i + 1) for i in range(9)]),
    ("star", [(0, i) for i in range(1, 80)]),
    ("c5", [(i, (i + 1) % 5) for i in range(5)]),
    ("k33", [(a, b) for a in range(3) for b in range(3, 6)]),
])
def test_triangle_free_graphs(name, edges):
    s, d = both_ways(edges)
    for k in (0, 1, 2):
        h, _, _, got = run(s, d, k)
        assert len(got) == 2 * len(edges) and h.last_iterations() == 0
    for k in (3, 4, 9):
        h, _, _, got = run(s, d, k)
        assert got == [] and h.last_iterations() == 1


def test_k4_and_the_diamond():
    s, d = both_ways(complete(4))
    assert len(run(s, d, 4)[3]) == 12
    h, _, _, got = run(s, d, 5)
    assert got == [] and h.last_iterations() == 1
    s, d = both_ways([(0, 1), (0, 2), (0, 3), (1, 2), (1, 3)])
    assert len(run(s, d, 3)[3]) == 10
    h, _, _, got = run(s, d, 4)  # the outer edges, then the spine
    assert got == [] and h.last_iterations() == 2


@pytest.mark.parametrize("n", [5, 64, 65, 70])
def test_complete_graphs(n):
    s, d = both_ways(complete(n))
    h, _, _, got = run(s, d, n)
    assert len(got) == n * (n - 1) and h.last_iterations() == 0
    h, _, _, got = run(s, d, n + 1)  # every triangle loses its three edges in the one round
    assert got == [] and h.last_iterations() == 1


@pytest.mark.parametrize("n", [63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 5000])
def test_book_graphs(n):
    s, d = both_ways(book(n))
    h, g, res, got = run(s, d, 3)
    assert len(got) == 2 * (2 * n + 1) and h.last_iterations() == 0
    res4 = plc().k_truss_subgraph(h, g, 4, False)  # the pages' edges, then the spine
    check(h, res4, [], 2)


@pytest.mark.parametrize("n", [511, 512])
def test_book_graphs_with_64_bit_ids(n):
    """The spine's rows have n + 1 entries: 512 8-byte ids fill the wave's LDS stage, 513 do not fit."""
    s, d = both_ways(book(n))
    h, g, res, got = run(s, d, 3, vdtype=np.int64)
    assert len(got) == 2 * (2 * n + 1)
    check(h, plc().k_truss_subgraph(h, g, 4, False), [], 2, vdtype=np.int64)


@pytest.mark.parametrize("vdtype", [np.int32, np.int64])
def test_grouped_book(vdtype):
    """Three K5s among the pages of a 1100-page book: the spine's rows are hub rows, and from k = 4 on
    most of their entries are dead."""
    s, d = GRAPHS["grouped"]()
    n, grouped = 1100, 15
    every = 2 * n + 1 + 3 * 10
    kept = 1 + 2 * grouped + 3 * 10
    h, g = make_graph(s, d, None, symmetric=True, vdtype=vdtype)
    for k, edges, rounds in [(3, every, 0), (4, kept, 1), (5, kept, 1), (6, kept, 1), (7, kept, 1), (8, 0, 2)]:
        want, want_rounds = twin("grouped", k)
        assert (len(want), want_rounds) == (edges, rounds)
        check(h, plc().k_truss_subgraph(h, g, k, False), want, rounds, vdtype=vdtype)


# ------------------------------------------------------------------ 2. datasets, the long cascade
@pytest.mark.parametrize("name", DATASETS)
def test_datasets_against_networkx(name):
    import networkx as nx
    s, d, w = dataset(name)
    G = nx.Graph()
    G.add_edges_from(zip(s.tolist(), d.tolist()))
    h, g = make_graph(s, d, w, symmetric=True)
    by_pair = dict(zip(zip(s.tolist(), d.tolist()), w.tolist()))
    weight_of = lambda a, b: np.array([by_pair[p] for p in zip(a.tolist(), b.tolist())], np.float32)
    for k in (3, 4, 5, 6, 8):
        want = sorted((min(u, v), max(u, v)) for u, v in nx.k_truss(G, k).edges())
        edges, rounds = twin(name, k)
        assert [tuple(e) for e in edges.tolist()] == want
        check(h, plc().k_truss_subgraph(h, g, k, False), want, rounds, weight_of=weight_of, wdtype=np.float32)


def test_long_cascade():
    s, d = gnp()
    edges, rounds = twin("gnp", 4)
    assert rounds >= 10  # (seen: 615 edges after 22 rounds; more than one chunk of rounds)
    run(s, d, 4, key="gnp")


# ------------------------------------------------------------------ 3. variants
VARIANT_KS = {"karate": [3, 4, 5], "polbooks": [5, 6], "grouped": [4, 8]}


@pytest.mark.parametrize("key", sorted(VARIANT_KS))
@pytest.mark.parametrize("variant", ["renumber_off", "int64", "transposed", "f32", "f64", "sparse_ids",
                                     "transposed_f64"])
def test_variants(key, variant):
    s, d = GRAPHS[key]()
    kw = {"renumber_off": dict(renumber=False), "int64": dict(vdtype=np.int64, weighted=True),
          "transposed": dict(transposed=True), "f32": dict(weighted=True),
          "f64": dict(weighted=True, wdtype=np.float64),
          "sparse_ids": dict(ids=lambda x: 1000 + 37 * np.asarray(x, np.int64), weighted=True),
          "transposed_f64": dict(transposed=True, weighted=True, wdtype=np.float64, renumber=False)}[variant]
    for k in VARIANT_KS[key]:
        run(s, d, k, key=key, **kw)


@pytest.mark.parametrize("key", sorted(VARIANT_KS))
@pytest.mark.parametrize("renumber", [True, False])
def test_self_loops_and_duplicates_give_the_cleaned_result(key, renumber):
    s, d = GRAPHS[key]()
    ids = np.unique(s)
    pick = slice(0, None, 3)
    ss = np.r_[s, ids[::2], s[pick], s[pick]]  # loops on every other vertex, a third of the entries three times
    dd = np.r_[d, ids[::2], d[pick], d[pick]]
    w = pair_weight(ss, dd).astype(np.float32)
    h, g = make_graph(ss, dd, w, symmetric=True, renumber=renumber)
    for k in [2] + VARIANT_KS[key]:
        edges, rounds = twin(key, k)
        assert len(simple_edges(ss, dd)) == len(simple_edges(s, d))
        check(h, plc().k_truss_subgraph(h, g, k, False), edges, rounds, weight_of=pair_weight, wdtype=np.float32)


@pytest.mark.parametrize("transposed", [False, True])
def test_a_repeated_entry_comes_back_as_its_first_stored_copy(transposed):
    """Every entry stored twice, the two copies with different weights: the result carries, per pair, the
    weight of the copy that comes first in the stored row, and the rows' order."""
    s, d = GRAPHS["karate"]()
    ss, dd = np.r_[s, s, np.arange(5)], np.r_[d, d, np.arange(5)]
    w = np.arange(len(ss), dtype=np.float32) + 0.5
    h, g = make_graph(ss, dd, w, symmetric=True, renumber=False, transposed=transposed)
    off, idx, aw = (host(x) for x in g.adjacency(h, transposed=transposed))
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    first = {}
    for r, c, x in zip(rows.tolist(), idx.tolist(), aw.tolist()):
        first.setdefault((r, c), x)
    assert len(idx) == 2 * len(s) + 5 and len(first) == len(s) + 5
    for k in (2, 4, 5):
        edges, rounds = twin("karate", k)
        src, dst, rw, _ = res = plc().k_truss_subgraph(h, g, k, False)
        got = check(h, res, edges, rounds, wdtype=np.float32,
                    weight_of=lambda a, b: np.array([first[p] for p in zip(a.tolist(), b.tolist())], np.float32))
        assert got == sorted(got)  # not renumbered: row order is ascending (src, dst)


# ------------------------------------------------------------------ 4. options, repeated calls, cached supports
def arrays(res):
    return [None if x is None else host(x).copy() for x in res]


def same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("key,k", [("karate", 4), ("polbooks", 5), ("grouped", 4), ("grouped", 8),
                                   ("email-Eu-core.csv", 8)])
def test_paths_give_identical_arrays(key, k):
    s, d = GRAPHS[key]()
    w = pair_weight(s, d).astype(np.float32)
    edges, rounds = twin(key, k)
    kept = []
    for path in (0, 1, 2):
        h, g, res = call(s, d, k, w, options={"kt_path": path})
        check(h, res, edges, rounds, weight_of=pair_weight, wdtype=np.float32)
        kept.append(arrays(res))
    assert same(kept[0], kept[1]) and same(kept[0], kept[2])


def test_kt_path_values_and_defaults():
    h = plc().ResourceHandle()
    for bad in (-1, 3):
        with pytest.raises(ValueError):
            h.set_option("kt_path", bad)
    h.set_option("kt_path", 2)
    h.set_option(None, 0)


@pytest.mark.parametrize("key", ["polbooks", "grouped"])
def test_repeated_calls_and_other_k(key):
    s, d = GRAPHS[key]()
    h, g = make_graph(s, d, None, symmetric=True)
    ks = VARIANT_KS[key]
    first = {}
    for k in ks + ks[::-1] + [2, 3]:  # the second and later calls start from the cached supports
        edges, rounds = twin(key, k)
        res = plc().k_truss_subgraph(h, g, k, False)
        check(h, res, edges, rounds)
        if k in first:
            assert same(first[k], arrays(res))
        first[k] = arrays(res)
    h2 = plc().ResourceHandle()  # another handle, the same graph
    check(h2, plc().k_truss_subgraph(h2, g, ks[0], False), *twin(key, ks[0]))


# ------------------------------------------------------------------ 5. cugraph layer
def cugraph_graph(s, d, w=None, **kw):
    import cugraph
    import pandas as pd
    G = cugraph.Graph()
    cols = {"src": s, "dst": d}
    if w is not None:
        cols["w"] = w
    G.from_pandas_edgelist(pd.DataFrame(cols), "src", "dst", "w" if w is not None else None, **kw)
    return G


def graph_pairs(G):
    e = G.edgelist
    return sorted(zip(e["src"].cpu().numpy().tolist(), e["dst"].cpu().numpy().tolist()))


@pytest.mark.parametrize("renumber", [True, False])
def test_cugraph_ktruss_subgraph(renumber):
    import cugraph
    s, d = GRAPHS["karate"]()
    w = pair_weight(s, d).astype(np.float32)
    G = cugraph_graph(s, d, w, renumber=renumber)
    for k in (3, 4, 5):
        edges, _ = twin("karate", k)
        for f in (cugraph.ktruss_subgraph, cugraph.k_truss):
            T = f(G, k)
            assert type(T) is type(G) and T._renumber == G._renumber and T.store_transposed == G.store_transposed
            assert graph_pairs(T) == directed_pairs(edges)
            e = T.edgelist
            assert np.array_equal(e["weights"].cpu().numpy(),
                                  pair_weight(e["src"].cpu().numpy(), e["dst"].cpu().numpy()).astype(np.float32))
        T = cugraph.ktruss_subgraph(G, k, use_weights=False)
        assert graph_pairs(T) == directed_pairs(edges) and T.edgelist["weights"] is None
    T = cugraph.ktruss_subgraph(G, 6)  # nothing is left
    assert type(T) is type(G) and T.edgelist is None
    assert cugraph.k_truss(G, 7).edgelist is None


def test_cugraph_k_truss_of_a_networkx_graph():
    import cugraph
    import networkx as nx
    K = nx.karate_club_graph()
    G = nx.relabel_nodes(K, {n: f"m{n}" for n in K.nodes()})
    for k in (3, 4, 5, 6):
        T, want = cugraph.k_truss(G, k), nx.k_truss(G, k)
        assert isinstance(T, nx.Graph) and not T.is_directed()
        assert {frozenset(e) for e in T.edges()} == {frozenset(e) for e in want.edges()}
        assert nx.is_isomorphic(T, want)
        assert all(T[u][v]["weight"] == G[u][v]["weight"] for u, v in T.edges())
    assert cugraph.k_truss(G, 6).number_of_edges() == 0


# ------------------------------------------------------------------ 6. errors through the C entry
def test_non_symmetric_graph_is_refused():
    h, g = make_graph([0, 1, 2], [1, 2, 0], None, symmetric=False)
    with pytest.raises(ValueError, match="undirected"):
        plc().k_truss_subgraph(h, g, 3, False)
    # flagged symmetric, but an entry has no reverse
    h, g = make_graph([0, 1, 1, 2, 0], [1, 0, 2, 1, 2], None, symmetric=True)
    with pytest.raises(ValueError, match="symmetric"):
        plc().k_truss_subgraph(h, g, 3, False)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="non-negative integer"):
            plc().k_truss_subgraph(h, g, bad, False)
