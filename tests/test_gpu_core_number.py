"""Core number and k-core on the GPU (csrc/core_number.hip through the C ABI and the Python
layers) against networkx.core_number of the simple graph, or a closed form.

Every comparison is integer equality for every vertex.  check() also asserts that ``vertices``
is a permutation of the graph's ids and that ``core_numbers`` has the graph's edge type (the
vertex type at these sizes).  k-cores are compared as sorted (src, dst) pairs with the set of
ordered pairs whose endpoints both have a core number of at least k, weights by pair."""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, dataset_path
from gpu_util import host, make_graph, plc

pytestmark = pytest.mark.gpu

DATASETS = ["karate.csv", "dolphins.csv", "polbooks.csv", "netscience.csv", "email-Eu-core.csv"]
IN, OUT, INOUT = 0, 1, 2  # cugraph_k_core_degree_type_t


# ------------------------------------------------------------------ CPU truth
def symmetrize(s, d):
    """Both directions of every edge, duplicates dropped, self-loops kept."""
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    lo = int(min(s.min(), d.min()))
    span = int(max(s.max(), d.max())) - lo + 1
    assert span < 1 << 31
    key = np.unique(np.r_[(s - lo) * span + (d - lo), (d - lo) * span + (s - lo)])
    return key // span + lo, key % span + lo


def nx_core_numbers(s, d, ids):
    """networkx.core_number of the simple graph, by position in ids (ids without edges: 0)."""
    import networkx as nx
    keep = s != d  # NetworkX raises on self-loops
    G = nx.Graph()
    G.add_edges_from(zip(s[keep].tolist(), d[keep].tolist()))
    cn = nx.core_number(G)
    return np.array([cn.get(int(i), 0) for i in ids], np.int64)


class Case:
    """A symmetrised edge list, the ids the graph must report and each id's core number
    (indexed like ``ids``; NetworkX's unless given)."""

    def __init__(self, s, d, renumber, vdtype=np.int32, core=None, symmetrized=False, w=None):
        self.s, self.d = (np.asarray(s, np.int64), np.asarray(d, np.int64)) if symmetrized else symmetrize(s, d)
        self.renumber, self.vdtype, self.w = renumber, vdtype, w
        self.ids = np.unique(np.r_[self.s, self.d]) if renumber else np.arange(int(self.s.max()) + 1)
        if core is None:
            core = nx_core_numbers(self.s, self.d, self.ids)
        self.core = np.asarray(core, np.int64)
        assert len(self.core) == len(self.ids)

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
            c.core = np.zeros(len(c.ids), np.int64)
            c.core[self.ids] = self.core
        return c

    def graph(self, transposed=False, options=None):
        return make_graph(self.s, self.d, self.w, transposed=transposed, renumber=self.renumber, symmetric=True,
                          vdtype=self.vdtype, options=options)

    def core_of(self, ids):
        return self.core[np.searchsorted(self.ids, ids)]

    def k_core_pairs(self, k, core_of=None):
        """Sorted distinct (src, dst) with both endpoints at core >= k, no loops."""
        core_of = core_of or self.core_of
        keep = (self.s != self.d) & (core_of(self.s) >= k) & (core_of(self.d) >= k)
        return sorted(set(zip(self.s[keep].tolist(), self.d[keep].tolist())))


def check(case, vertices, numbers, times=1):
    """Returns the core numbers by position in case.ids."""
    v, c = host(vertices), host(numbers)
    assert v.dtype == np.dtype(case.vdtype) and c.dtype == v.dtype  # edge type = vertex type below 2^31 edges
    assert len(v) == len(case.ids) and len(c) == len(v)
    assert np.array_equal(np.sort(v), case.ids), "vertices is not a permutation of the graph's ids"
    if not case.renumber:
        assert np.array_equal(v, case.ids)
    by_id = np.empty(len(v), np.int64)
    by_id[np.searchsorted(case.ids, v)] = c
    bad = np.flatnonzero(by_id != times * case.core)
    assert len(bad) == 0, f"{len(bad)} wrong, first: id {case.ids[bad[0]]} got {by_id[bad[0]]} want {case.core[bad[0]]}"
    return by_id


def run(case, transposed=False, options=None, calls=1):
    h, g = case.graph(transposed, options)
    out = None
    for _ in range(calls):
        by_id = check(case, *plc().core_number(h, g, None, False))
        assert out is None or np.array_equal(out, by_id)
        out = by_id
    return out


def check_k_core(case, k, result, core_of=None, weight_of=None):
    src, dst, w = result
    s, d = host(src), host(dst)
    assert s.dtype == np.dtype(case.vdtype) and d.dtype == s.dtype and len(s) == len(d)
    got = list(zip(s.tolist(), d.tolist()))
    assert len(set(got)) == len(got), "an entry was emitted twice"
    assert sorted(got) == case.k_core_pairs(k, core_of)
    if case.w is None:
        assert w is None
    else:
        assert w is not None and len(host(w)) == len(s)
        if weight_of is not None:
            assert np.array_equal(host(w), weight_of(s, d).astype(host(w).dtype))
    return got


# ------------------------------------------------------------------ the graphs (built once)
@functools.lru_cache(maxsize=None)
def vectors():
    with open(os.path.join(GOLDEN, "core_vectors.json")) as f:
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
    return Case(s, d, renumber=True)


def clique_edges(ids):
    a, b = np.meshgrid(ids, ids, indexing="ij")
    keep = a < b
    return a[keep], b[keep]


def assert_facts(case, facts):
    has_edges = np.isin(case.ids, np.r_[case.s, case.d])
    assert int(has_edges.sum()) == facts["vertices"]
    top = int(case.core.max())
    assert top == facts["largest_core"] and int((case.core == top).sum()) == facts["in_largest_core"]
    assert int(case.core.sum()) == facts["sum"]
    if "distinct" in facts:
        assert len(np.unique(case.core[case.core > 0])) == facts["distinct"]


# ------------------------------------------------------------------ 1. golden vectors
@functools.lru_cache(maxsize=None)
def small():
    v = vectors()["small"]
    case = Case(v["src"], v["dst"], renumber=False, symmetrized=True, w=np.asarray(v["weights"], np.float32))
    assert case.core.tolist() == v["core_numbers"]  # NetworkX agrees with the reference's vector
    return v, case


def test_golden_core_numbers():
    v, case = small()
    h, g = case.graph()
    vertices, numbers = plc().core_number(h, g, None, False)
    assert host(vertices).tolist() == list(range(7)) and host(numbers).tolist() == v["core_numbers"]
    check(case, vertices, numbers)


@pytest.mark.parametrize("given", [True, False])
def test_golden_k_core(given):
    v, case = small()
    h, g = case.graph()
    core = (np.arange(7, dtype=np.int32), np.asarray(v["core_numbers"], np.int32)) if given else None
    src, dst, w = plc().k_core(h, g, v["k"], None, core, False)
    # by internal row, ascending within the row: the order of the golden file
    assert host(src).tolist() == v["k_core_src"] and host(dst).tolist() == v["k_core_dst"]
    assert host(w).tolist() == [1.0] * 12 and host(w).dtype == np.float32
    check_k_core(case, 3, (src, dst, w))
    src, dst, w = plc().k_core(h, g, 0, None, core, False)
    assert len(host(src)) == 22 and len(host(w)) == 22
    check_k_core(case, 0, (src, dst, w))
    src, dst, w = plc().k_core(h, g, 4, None, core, False)
    assert len(host(src)) == 0 and len(host(dst)) == 0 and host(src).dtype == np.int32
    assert w is not None and len(host(w)) == 0 and host(w).dtype == np.float32  # still an array: the graph is weighted


# ------------------------------------------------------------------ 2. the datasets
@pytest.mark.parametrize("vdtype", [np.int32, np.int64])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("name", DATASETS)
def test_datasets(name, renumber, transposed, vdtype):
    base = dataset(name)
    assert_facts(base, vectors()["datasets"][name])
    run(base.with_(renumber=renumber, vdtype=vdtype), transposed)


def test_email_has_self_loops():
    c = dataset("email-Eu-core.csv")
    assert int((c.s == c.d).sum()) > 0


# ------------------------------------------------------------------ 3. R-MAT
@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("scale", [12, 14])
def test_rmat(scale, renumber):
    base = rmat_case(scale)
    assert (base.s == base.d).any(), "the generated graph is expected to hold self-loop entries"
    assert_facts(base, vectors()["rmat"][str(scale)])
    case = base.with_(renumber=renumber)
    outs = [run(case, options={"core_scan": scan}, calls=2) for scan in (1, 0)]
    assert np.array_equal(outs[0], outs[1])


# ------------------------------------------------------------------ 4. closed forms
def star(leaves, hub_last):
    hub = leaves if hub_last else 0
    leaf = np.arange(leaves) + (0 if hub_last else 1)
    return Case(np.full(leaves, hub), leaf, renumber=True, core=np.ones(leaves + 1, np.int64))


@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("hub_last", [False, True])
def test_star(hub_last, renumber):
    """One counter under 200,000 subtractions; the hub's row goes through the hub list."""
    run(star(200_000, hub_last).with_(renumber=renumber))


def test_clique():
    n = 1500
    s, d = clique_edges(np.arange(n))
    run(Case(s, d, renumber=True, core=np.full(n, n - 1)))


def test_complete_bipartite():
    a, b = np.meshgrid(np.arange(50), np.arange(50, 3050), indexing="ij")
    run(Case(a.ravel(), b.ravel(), renumber=True, core=np.full(3050, 50)))


def test_long_path_takes_many_chunks_of_rounds():
    n = 20_001
    p = np.arange(n - 1)
    case = Case(p, p + 1, renumber=True, core=np.ones(n, np.int64))
    h, g = case.graph()
    check(case, *plc().core_number(h, g, None, False))
    assert h.last_iterations() >= (n - 1) // 2  # two ends per round


def test_cycle():
    n = 10_000
    p = np.arange(n)
    run(Case(p, (p + 1) % n, renumber=True, core=np.full(n, 2)))


def disjoint_cliques(sizes):
    ss, dd, core, first = [], [], [], 0
    for n in sizes:
        s, d = clique_edges(np.arange(first, first + n))
        ss.append(s)
        dd.append(d)
        core.append(np.full(n, n - 1))
        first += n
    return Case(np.concatenate(ss), np.concatenate(dd), renumber=True, core=np.concatenate(core))


@pytest.mark.parametrize("sizes", [tuple(range(2, 121)), (2, 10, 300)], ids=["every_level", "gaps"])
@pytest.mark.parametrize("scan", [1, 0])
def test_disjoint_cliques(sizes, scan):
    case = disjoint_cliques(sizes)
    h, g = case.graph(options={"core_scan": scan})
    check(case, *plc().core_number(h, g, None, False))


@functools.lru_cache(maxsize=None)
def clique_above_path():
    """A 5000-vertex path on ids 0..4999 and K_300 on ids 5000..5299, joined by one edge:
    the highest degrees sit on the highest ids."""
    p, k = 5000, 300
    ps = np.arange(p)  # 0-1, ..., 4998-4999, 4999-5000
    cs, cd = clique_edges(np.arange(p, p + k))
    return Case(np.r_[ps, cs], np.r_[ps + 1, cd], renumber=True,
                core=np.r_[np.ones(p, np.int64), np.full(k, k - 1)])


def test_clique_above_path():
    case = clique_above_path()
    assert np.array_equal(run(case), run(case.with_(renumber=False)))


@pytest.mark.parametrize("renumber", [True, False])
def test_hub_in_a_clique(renumber):
    """Vertex 0 has 5000 leaves and belongs to a K_4: it is peeled to 3, not with its leaves."""
    leaves = 5000
    ks, kd = clique_edges(np.arange(4))
    s, d = np.r_[ks, np.zeros(leaves, np.int64)], np.r_[kd, 4 + np.arange(leaves)]
    run(Case(s, d, renumber=True, core=np.r_[np.full(4, 3), np.ones(leaves, np.int64)]).with_(renumber=renumber))


def test_ids_without_edges_have_core_zero():
    s, d = clique_edges(np.array([3, 4, 7, 9]))
    case = Case(np.r_[s, 12], np.r_[d, 15], renumber=False)
    assert case.core.tolist() == [0, 0, 0, 3, 3, 0, 0, 3, 0, 3, 0, 0, 1, 0, 0, 1]
    run(case)


# ------------------------------------------------------------------ 5. degree types
@pytest.mark.parametrize("make", [lambda: dataset("karate.csv"), lambda: rmat_case(12)], ids=["karate", "rmat12"])
def test_degree_types(make):
    """The enum is not reachable through pylibcugraph.core_number (it ignores degree_type as
    the reference does); the binding's private helper passes it to the C entry."""
    case = make()
    h, g = case.graph()
    base = check(case, *plc()._core_number(h, g, IN, False))
    assert np.array_equal(check(case, *plc()._core_number(h, g, OUT, False)), base)
    assert np.array_equal(check(case, *plc()._core_number(h, g, INOUT, False), times=2), 2 * base)


def test_bad_degree_type():
    h, g = dataset("karate.csv").graph()
    with pytest.raises(ValueError, match="degree_type"):
        plc()._core_number(h, g, 3, False)


def test_degree_type_warns_and_is_ignored():
    case = dataset("karate.csv")
    h, g = case.graph()
    with pytest.warns(Warning, match="'degree_type' parameter is ignored"):
        check(case, *plc().core_number(h, g, "bidirectional", False))


# ------------------------------------------------------------------ 6. repeated entries, self-loops
@pytest.mark.parametrize("renumber", [True, False])
def test_repeated_entries_count_once(renumber):
    s = np.array([0, 1, 1, 2, 2, 0] * 2)
    d = np.array([1, 0, 2, 1, 0, 2] * 2)
    h, g = make_graph(s, d, None, renumber=renumber, symmetric=True)
    vertices, numbers = plc().core_number(h, g, None, False)
    assert sorted(host(vertices).tolist()) == [0, 1, 2] and host(numbers).tolist() == [2, 2, 2]
    src, dst, w = plc().k_core(h, g, 2, None, None, False)
    assert sorted(zip(host(src).tolist(), host(dst).tolist())) == sorted(zip(s[:6].tolist(), d[:6].tolist()))
    assert w is None


@pytest.mark.parametrize("renumber", [True, False])
def test_self_loops_do_not_count(renumber):
    n = 200
    p = np.arange(n - 1)
    s, d = np.r_[p, p + 1, np.arange(n)], np.r_[p + 1, p, np.arange(n)]
    h, g = make_graph(s, d, None, renumber=renumber, symmetric=True)
    vertices, numbers = plc().core_number(h, g, None, False)
    assert len(host(vertices)) == n and (host(numbers) == 1).all()
    with pytest.raises(ValueError, match="self-loops"):
        plc().core_number(h, g, None, True)
    src, dst, _ = plc().k_core(h, g, 1, None, None, False)
    assert sorted(zip(host(src).tolist(), host(dst).tolist())) == sorted(zip(np.r_[p, p + 1].tolist(),
                                                                             np.r_[p + 1, p].tolist()))
    src, dst, _ = plc().k_core(h, g, 0, None, None, False)
    assert len(host(src)) == 2 * (n - 1) and (host(src) != host(dst)).all()


# ------------------------------------------------------------------ 7. k-core
def pair_weight(s, d):
    return 0.5 + ((np.minimum(s, d) * 31 + np.maximum(s, d) * 17) % 13)


@functools.lru_cache(maxsize=None)
def weighted_karate():
    s, d = symmetrize(*dataset_edges("karate.csv"))
    return Case(s, d, renumber=True, symmetrized=True, w=pair_weight(s, d).astype(np.float32))


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("transposed", [False, True])
def test_k_core_weights(k, transposed):
    case = weighted_karate()
    h, g = case.graph(transposed)
    got = check_k_core(case, k, plc().k_core(h, g, k, None, None, False), weight_of=pair_weight)
    assert (len(got) == 0) == (k > 4)


@functools.lru_cache(maxsize=None)
def sparse_id_case():
    """karate with the ids spread out: id -> 1000 + 37 * id."""
    s, d = dataset_edges("karate.csv")
    return Case(1000 + 37 * s, 1000 + 37 * d, renumber=True)


def test_k_core_from_a_shuffled_core_result():
    case = sparse_id_case()
    h, g = case.graph()
    order = np.random.default_rng(5).permutation(len(case.ids))
    core = (case.ids[order].astype(np.int32), case.core[order].astype(np.int32))
    for k in (2, 3, 4):
        check_k_core(case, k, plc().k_core(h, g, k, "bidirectional", core, True))  # degree_type is ignored


def test_k_core_from_a_partial_core_result():
    """Vertices the result does not list count as core 0."""
    case = sparse_id_case()
    h, g = case.graph()
    listed = case.ids[::2]
    core = (listed.astype(np.int32), case.core_of(listed).astype(np.int32))

    def core_of(ids):
        return np.where(np.isin(ids, listed), case.core_of(ids), 0)

    got = check_k_core(case, 2, plc().k_core(h, g, 2, None, core, True), core_of=core_of)
    assert 0 < len(got) < len(case.k_core_pairs(2))


def test_k_core_takes_the_numbers_as_given():
    case = dataset("karate.csv")
    h, g = case.graph()
    doubled = plc()._core_number(h, g, INOUT, False)
    assert check_k_core(case, 4, plc().k_core(h, g, 8, None, doubled, False))
    assert check_k_core(case, 4, plc().k_core(h, g, 8, "bidirectional", None, False))
    assert check_k_core(case, 4, plc().k_core(h, g, 7, None, doubled, False))  # 2 x core >= 7 is core >= 4


def test_k_core_bad_core_results():
    case = sparse_id_case()
    h, g = case.graph()
    ids, core = case.ids.astype(np.int32), case.core.astype(np.int32)
    with pytest.raises(ValueError, match="length"):
        plc().k_core(h, g, 2, None, (ids, core[:-1]), False)
    with pytest.raises(ValueError, match="vertex type"):
        plc().k_core(h, g, 2, None, (ids.astype(np.int64), core), False)
    with pytest.raises(ValueError, match="edge type"):
        plc().k_core(h, g, 2, None, (ids, core.astype(np.int64)), False)
    with pytest.raises(ValueError, match="degree_type"):
        plc().k_core(h, g, 2, "both", None, False)


@pytest.mark.parametrize("renumber", [True, False])
def test_k_core_unknown_id(renumber):
    case = sparse_id_case() if renumber else dataset("karate.csv").with_(renumber=False)
    h, g = case.graph()
    for unknown in (int(case.ids[0]) + 1 if renumber else 34, -5, 2 ** 31 - 1):
        ids = np.r_[case.ids[:10], unknown, case.ids[10:]].astype(np.int32)
        core = np.r_[case.core[:10], 9, case.core[10:]].astype(np.int32)
        with pytest.raises(ValueError, match="not in the graph"):
            plc().k_core(h, g, 3, None, (ids, core), True)
        check_k_core(case, 3, plc().k_core(h, g, 3, None, (ids, core), False))  # skipped without the check


@pytest.mark.parametrize("name", DATASETS)
def test_main_core(name):
    case = dataset(name)
    facts = vectors()["datasets"][name]
    k = facts["largest_core"]
    h, g = case.graph()
    got = check_k_core(case, k, plc().k_core(h, g, k, None, None, False))
    s = np.array([a for a, _ in got])
    members, degree = np.unique(s, return_counts=True)
    assert len(members) == facts["in_largest_core"] and int(degree.min()) >= k
    assert len(plc().k_core(h, g, k + 1, None, None, False)[0]) == 0


def distinct_weight(s, d):
    """pair_weight's pattern with no two pairs alike; exact in fp32 for ids below 256."""
    return 0.5 + np.minimum(s, d) * 256 + np.maximum(s, d)


@functools.lru_cache(maxsize=None)
def long_row_case(length):
    """K_4 on 0..3 and length - 3 further vertices, each joined to 0 and to 1: row 0 has `length`
    entries, 3 of them in the 3-core, and every vertex is in the 2-core."""
    import networkx as nx
    extra = np.arange(4, length + 1)
    ks, kd = clique_edges(np.arange(4))
    s, d = symmetrize(np.r_[ks, np.zeros_like(extra), np.ones_like(extra)], np.r_[kd, extra, extra])
    case = Case(s, d, renumber=True, symmetrized=True, w=distinct_weight(s, d).astype(np.float32))
    assert int((s == 0).sum()) == length and len(set(case.w.tolist())) == len(s) // 2
    G = nx.Graph()
    G.add_edges_from(zip(s.tolist(), d.tolist()))
    for k, edges in ((2, (length - 3) * 2 + 6), (3, 6), (4, 0)):
        want = nx.k_core(G, k).edges()
        assert len(want) == edges
        assert sorted([(a, b) for a, b in want] + [(b, a) for a, b in want]) == case.k_core_pairs(k)
    return case


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("length", [63, 64, 65, 128, 129])
def test_k_core_rows_at_the_wave_boundary(length, renumber, transposed):
    """Row 0 is taken by a thread below 64 entries and by a wave from 64 on: kept whole (k = 2),
    kept in 3 of its entries (k = 3), and dropped (k = 4); weights follow their entries."""
    case = long_row_case(length).with_(renumber=renumber)
    h, g = case.graph(transposed)
    for k in (2, 3):
        got = check_k_core(case, k, plc().k_core(h, g, k, None, None, False), weight_of=distinct_weight)
        if not renumber:
            assert got == sorted(got)  # by row, then by stored position: rows ascend
    src, dst, w = plc().k_core(h, g, 4, None, None, False)
    assert len(host(src)) == 0 and len(host(dst)) == 0 and host(src).dtype == np.int32
    assert w is not None and len(host(w)) == 0 and host(w).dtype == np.float32


def test_k_core_repeats_and_a_loop_in_a_wave_row():
    """The 65-entry row stores one entry twice (the copies weigh differently) and a loop: each pair
    comes back once, with the weight of its first stored copy, in the order of the rows."""
    base = long_row_case(65)
    s, d = np.r_[base.s, 0, 40, 0], np.r_[base.d, 40, 0, 0]
    w = np.r_[base.w, -1.0, -2.0, -3.0].astype(np.float32)
    case = Case(s, d, renumber=False, symmetrized=True, w=w)
    h, g = case.graph()
    off, idx, aw = (host(x) for x in g.adjacency(h, transposed=False))
    assert off[1] - off[0] == 67 and sorted(idx[:67].tolist()) == sorted([0, 40] + list(range(1, 66)))
    rows = np.repeat(np.arange(len(off) - 1), np.diff(off))
    first = {}
    for r, c, x in zip(rows.tolist(), idx.tolist(), aw.tolist()):
        first.setdefault((r, c), x)
    got = check_k_core(case, 2, plc().k_core(h, g, 2, None, None, False),
                       weight_of=lambda a, b: np.array([first[p] for p in zip(a.tolist(), b.tolist())], np.float32))
    assert got == sorted(got) and len(got) == len(base.s)


# ------------------------------------------------------------------ 8. refusals
def test_asymmetric_graph_is_refused():
    h, g = make_graph([0, 1], [1, 2], None, symmetric=False)
    with pytest.raises(ValueError, match="core_number currently supports only undirected graphs"):
        plc().core_number(h, g, None, False)
    with pytest.raises(ValueError, match="core_number currently supports only undirected graphs"):
        plc().k_core(h, g, 1, None, None, False)


def test_multigraph_is_refused():
    p = plc()
    h = p.ResourceHandle()
    s, d = np.array([0, 1, 0, 1], np.int32), np.array([1, 0, 1, 0], np.int32)
    g = p.SGGraph(h, p.GraphProperties(is_symmetric=True, is_multigraph=True), s, d, None, store_transposed=False,
                  renumber=True)
    with pytest.raises(ValueError, match="does not support multi-graphs"):
        p.core_number(h, g, None, False)
    with pytest.raises(ValueError, match="does not support multi-graphs"):
        p.k_core(h, g, 1, None, None, False)


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
        with pytest.raises(NotImplementedError, match="multi-GPU core_number"):
            p.core_number(h, g, None, False)
        with pytest.raises(NotImplementedError, match="multi-GPU k_core"):
            p.k_core(h, g, 1, None, None, False)
        g = None
        h = None
    finally:
        torch.cuda.synchronize()
        p.trim_device_cache()
        ctx.free()
        dist.destroy_process_group()


def test_core_scan_is_range_checked():
    h = plc().ResourceHandle()
    with pytest.raises(ValueError, match="core_scan"):
        h.set_option("core_scan", 2)
    h.set_option("core_scan", 0)
    h.set_option("core_scan", 1)


def test_profiling_covers_the_peel_kernel():
    case = rmat_case(12)
    h, g = case.graph()
    h.set_profiling(True)
    check(case, *plc().core_number(h, g, None, False))
    assert h.last_iterations() > 0 and h.last_hot_kernel_launches() >= h.last_iterations()
    assert h.last_hot_kernel_ms() > 0


# ------------------------------------------------------------------ 9. cugraph.core_number / k_core
@functools.lru_cache(maxsize=None)
def karate_nx():
    import networkx as nx
    s, d = dataset_edges("karate.csv")
    G = nx.Graph()
    G.add_edges_from(zip(s.tolist(), d.tolist()))
    return G, nx.core_number(G)


def karate_graph(weighted=False):
    import cugraph
    import pandas as pd
    s, d = dataset_edges("karate.csv")
    G = cugraph.Graph()
    cols = {"s": s, "d": d}
    if weighted:
        cols["w"] = pair_weight(s, d)
    G.from_pandas_edgelist(pd.DataFrame(cols), "s", "d", "w" if weighted else None)
    return G


def undirected(pairs):
    return {(min(a, b), max(a, b)) for a, b in pairs}


def edge_set(G):
    df = G.view_edge_list()
    return undirected(zip(df["src"].tolist(), df["dst"].tolist()))


def test_cugraph_core_number():
    import cugraph
    nxG, want = karate_nx()
    df = cugraph.core_number(karate_graph())
    assert list(df.columns) == ["vertex", "core_number"]
    assert dict(zip(df["vertex"].tolist(), df["core_number"].tolist())) == want
    with pytest.warns(Warning, match="'degree_type' parameter is ignored"):
        df = cugraph.core_number(karate_graph(), degree_type="incoming")
    assert dict(zip(df["vertex"].tolist(), df["core_number"].tolist())) == want
    got = cugraph.core_number(nxG)
    assert isinstance(got, dict) and got == want


def test_cugraph_k_core():
    import cugraph
    import networkx as nx
    import pandas as pd
    nxG, cn = karate_nx()
    G = karate_graph()
    for k in (None, 2):
        out = cugraph.k_core(G, k)
        assert type(out) is cugraph.Graph and not out.is_weighted()
        assert edge_set(out) == undirected(nx.k_core(nxG, k).edges())
    frame = pd.DataFrame({"vertex": list(cn), "values": list(cn.values())})
    assert edge_set(cugraph.k_core(G, 3, core_number=frame)) == undirected(nx.k_core(nxG, 3).edges())
    assert edge_set(cugraph.k_core(G, core_number=frame)) == undirected(nx.k_core(nxG).edges())
    assert cugraph.k_core(G, 5).edgelist is None  # above the largest core: no edges
    # weights follow their edges
    out = cugraph.k_core(karate_graph(weighted=True), 3)
    df = out.view_edge_list()
    assert out.is_weighted() and len(df) == nx.k_core(nxG, 3).number_of_edges()
    assert np.array_equal(df["weights"].to_numpy(), pair_weight(df["src"].to_numpy(), df["dst"].to_numpy()))


def test_cugraph_k_core_networkx():
    import cugraph
    import networkx as nx
    nxG, cn = karate_nx()
    for k in (None, 2):
        out = cugraph.k_core(nxG, k)
        assert isinstance(out, nx.Graph)
        assert undirected(out.edges()) == undirected(nx.k_core(nxG, k).edges())
