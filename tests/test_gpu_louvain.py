"""Louvain parity (csrc/louvain.hip through cugraph_louvain) against the oracle
(oracle/louvain.py) and the reference's golden vectors.

Integer weights make every sum exact in any order, so there the clustering must be
identical to the oracle's; with fractional weights the modularity must agree
within 1e-6 relative and equal the modularity of the returned partition."""
import numpy as np
import pytest

from conftest import dataset_path
from gpu_util import host, make_graph, plc
from oracle import graph as og
from oracle import louvain as olv
from oracle import rmat

pytestmark = pytest.mark.gpu


def run(h, G, max_level=100, resolution=1.0):
    v, c, q = plc().louvain(h, G, max_level, resolution, False)
    return host(v), host(c), q


def oracle_run(src, dst, w, renumber, max_level=100, resolution=1.0):
    G = og.create_graph(src, dst, w, renumber=renumber)
    s, d, ww = G.coo()
    c, q, levels = olv.louvain(G.num_vertices, s, d, ww, max_level, resolution)
    return G, c, q, levels


def test_c_golden(golden):
    g = golden["louvain_c"]
    h, G = make_graph(g["src"], g["dst"], g["w"], renumber=False)
    v, c, q = run(h, G, g["max_level"], g["resolution"])
    assert v.tolist() == list(range(g["num_vertices"]))
    assert c.tolist() == g["expected_clusters"]
    assert abs(q - g["expected_modularity"]) <= g["tol"] * abs(g["expected_modularity"])


def test_pylib_golden(golden):
    g = golden["louvain_pylib"]
    h, G = make_graph(g["src"], g["dst"], g["w"], renumber=True, symmetric=True)
    v, c, q = run(h, G, g["max_level"], g["resolution"])
    assert v.tolist() == g["expected_vertices"]
    assert c.tolist() == g["expected_clusters"]
    assert q == pytest.approx(g["expected_modularity"], abs=1e-12)


def test_karate_gtest(golden):
    g = golden["louvain_karate_gtest"]
    s, d, w = og.read_csv(dataset_path(g["dataset"]))
    h, G = make_graph(s, d, w, renumber=False, symmetric=True)
    v, c, q = run(h, G, g["max_level"], g["resolution"])
    assert h.last_louvain_levels() == g["expected_level"]
    a, b = np.float32(q), np.float32(g["expected_modularity"])
    assert abs(int(a.view(np.int32)) - int(b.view(np.int32))) <= 4  # ASSERT_FLOAT_EQ
    _, oc, oq, _ = oracle_run(s, d, w, renumber=False)
    assert np.array_equal(c, oc) and q == oq


@pytest.mark.parametrize("name", ["dolphins.csv", "netscience.csv", "polbooks.csv"])
def test_datasets_vs_oracle(name):
    s, d, w = og.read_csv(dataset_path(name))
    h, G = make_graph(s, d, w, renumber=True, symmetric=True)
    v, c, q = run(h, G)
    OG, oc, oq, olevels = oracle_run(s, d, w, renumber=True)
    assert np.array_equal(v, OG.number_map)
    assert h.last_louvain_levels() == olevels
    assert abs(q - oq) <= 1e-6 * abs(oq)
    ss, dd, ww = OG.coo()
    assert abs(olv.modularity(ss, dd, ww, c) - q) <= 1e-6 * abs(q)


@pytest.mark.parametrize("scale,integer", [(10, True), (12, True), (12, False)])
def test_rmat_vs_oracle(scale, integer):
    s, d = rmat.rmat(scale, 16 << scale, seed=7)
    w = rmat.rmat_weights(s.size, seed=8).astype(np.float64)
    if integer:
        w = np.floor(w * 8.0) + 1.0
    s, d, w = og.symmetrize_dedup(s, d, w)
    h, G = make_graph(s, d, w.astype(np.float32), renumber=True, symmetric=True)
    v, c, q = run(h, G)
    OG, oc, oq, olevels = oracle_run(s, d, w.astype(np.float32).astype(np.float64), renumber=True)
    assert np.array_equal(v, OG.number_map)
    ss, dd, ww = OG.coo()
    if integer:
        assert np.array_equal(c, oc)
        assert q == oq
        assert h.last_louvain_levels() == olevels
    else:
        assert abs(q - oq) <= 1e-6 * abs(oq)
    assert abs(olv.modularity(ss, dd, ww, c) - q) <= 1e-6 * abs(q)


def test_resolution_and_max_level():
    s, d, w = og.read_csv(dataset_path("karate.csv"))
    for res, ml in ((0.5, 100), (1.0, 1), (2.0, 2)):
        h, G = make_graph(s, d, w, renumber=False, symmetric=True)
        v, c, q = run(h, G, ml, res)
        _, oc, oq, olevels = oracle_run(s, d, w, renumber=False, max_level=ml, resolution=res)
        assert np.array_equal(c, oc) and q == pytest.approx(oq, rel=1e-12)
        assert h.last_louvain_levels() == olevels <= ml


def test_isolated_ids_inside_chunks():
    """Unrenumbered ids with isolated vertices between the connected ones (every third id
    has edges): zero-degree rows sit inside the hash chunks, where an edge's row is found
    by a binary search over the chunk's row offsets (empty rows share their start).
    Integer weights: the clustering and Q must be the oracle's exactly."""
    s, d = rmat.rmat(10, 16 << 10, seed=11)
    w = np.floor(rmat.rmat_weights(s.size, seed=12).astype(np.float64) * 8.0) + 1.0
    s, d, w = og.symmetrize_dedup(s, d, w)
    s, d = s * 3, d * 3
    h, G = make_graph(s, d, w.astype(np.float32), renumber=False, symmetric=True)
    v, c, q = run(h, G)
    OG, oc, oq, olevels = oracle_run(s, d, w, renumber=False)
    assert np.array_equal(c, oc) and q == oq
    assert h.last_louvain_levels() == olevels


def test_int64_and_double():
    s, d, w = og.read_csv(dataset_path("karate.csv"))
    h, G = make_graph(s, d, w, renumber=True, symmetric=True, vdtype=np.int64, wdtype=np.float64)
    v, c, q = run(h, G)
    assert c.dtype == np.int64
    OG, oc, oq, _ = oracle_run(s, d, w, renumber=True)
    assert np.array_equal(c, oc) and q == oq


def test_unweighted_graph_fails():
    s, d, _ = og.read_csv(dataset_path("karate.csv"))
    h, G = make_graph(s, d, None, renumber=False, symmetric=True)
    with pytest.raises(RuntimeError, match="weighted"):
        run(h, G)


def test_repeat_is_deterministic():
    s, d = rmat.rmat(12, 16 << 12, seed=3)
    w = rmat.rmat_weights(s.size, seed=4)
    s, d, w = og.symmetrize_dedup(s, d, w)
    h, G = make_graph(s, d, w.astype(np.float32), renumber=True, symmetric=True)
    a = run(h, G)
    b = run(h, G)
    assert np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_dendrogram_levels_compose_to_clusters():
    """cugraph_amd_heirarchical_clustering_result_get_level: the levels (reference
    Dendrogram) compose to the flattened clustering (flatten_dendrogram,
    louvain_impl.cuh:239-255) and the level count is the reported one."""
    s, d = rmat.rmat(11, 16 << 11, seed=3)
    w = np.floor(rmat.rmat_weights(s.size, seed=4).astype(np.float64) * 8.0) + 1.0
    s, d, w = og.symmetrize_dedup(s, d, w)
    h, G = make_graph(s, d, w, renumber=True, symmetric=True)
    v, c, q, levels = plc().louvain_dendrogram(h, G, 100, 1.0)
    lv = [host(x).astype(np.int64) for x in levels]
    assert len(lv) == h.last_louvain_levels() >= 2
    flat = np.arange(lv[0].size)
    for i, x in enumerate(lv):
        assert i == 0 or x.size == lv[i - 1].max() + 1
        flat = x[flat]
    assert np.array_equal(flat, host(c))


@pytest.mark.parametrize("renumber,opts", [(True, {}), (False, {}), (True, {"louvain_big_hash": 0}),
                                           (False, {"louvain_big_cap": 16}),
                                           (False, {"louvain_big_maxdeg": 3000}),
                                           (True, {"louvain_big_maxdeg": 4530}),
                                           (False, {"louvain_big_maxdeg": 4530}),
                                           (False, {"louvain_big_maxdeg": 2048})])
def test_hash_sweep_equals_sort_sweep(renumber, opts):
    """The LDS-hash local move (louvain.hip: k_sweep_hash for rows of <= 2048 edges,
    k_big_partials / k_big_buckets / k_big_move for heavier rows; fixed-point pair
    sums) against the sort + reduce_by_key local move (option louvain_hash = 0) on
    RMAT-16 with integer weights: every sum is exact in both, so the clustering,
    modularity and level count are identical.  Variants: heavy rows on the sort
    path inside the hash schedule (not a prefix of the rows without renumbering:
    gathered COO), and a (row, bucket) table cap of 16 that overflows, so the level
    falls back to the sort path for its heavy rows mid-sweep, and rows above 3000
    edges on the sort path beside the LDS passes (the > 2.5M-edge rule).  This graph's 17
    heavy level-0 rows have 4442 ... 4591 and 9645 edges, so the limit 3000 sends all of
    them to the sort path at level 0; the limit 4530 lies between two of them (9 rows
    taken, 8 not): with renumbering the rows not taken are a prefix of the
    degree-ordered rows (their sort-path COO is the level's own), without it they
    interleave with the taken ones (gathered COO), and the taken rows are indexed by
    their rank among the taken.  The limit 2048 takes no heavy row at any level.  (The
    64-bit pair keys of levels with >= 2^24 - 1 ids: test_hash_sweep_wide_keys, own
    process.)"""
    s, d = rmat.rmat(16, 16 << 16, seed=11)
    w = np.floor(rmat.rmat_weights(s.size, seed=12).astype(np.float64) * 8.0) + 1.0
    s, d, w = og.symmetrize_dedup(s, d, w)
    deg = np.bincount(s)
    assert deg.max() > 2048 and deg[0] <= 2048  # hub rows exist, and row 0 is not one
    heavy = deg[deg > 2048]
    assert (heavy > 4530).any() and (heavy <= 4530).any()  # the limit 4530 splits the hub rows
    h, G = make_graph(s, d, w, renumber=renumber, symmetric=True, options=opts)
    v, c, q = run(h, G)
    lv = h.last_louvain_levels()
    h2, G2 = make_graph(s, d, w, renumber=renumber, symmetric=True, options={"louvain_hash": 0})
    v2, c2, q2 = run(h2, G2)
    assert np.array_equal(v, v2) and np.array_equal(c, c2)
    assert q == q2 and lv == h2.last_louvain_levels()


def test_hash_sweep_wide_keys():
    """k_sweep_hash<u64> (levels with >= 2^24 - 1 ids) forced on RMAT-14 (option
    louvain_wide_keys): same clustering as the sort path."""
    s, d = rmat.rmat(14, 16 << 14, seed=5)
    w = np.floor(rmat.rmat_weights(s.size, seed=6).astype(np.float64) * 8.0) + 1.0
    s, d, w = og.symmetrize_dedup(s, d, w)
    out = {}
    for mode, opts in (("wide", {"louvain_wide_keys": 1}), ("sort", {"louvain_hash": 0})):
        h, G = make_graph(s, d, w, renumber=True, symmetric=True, options=opts)
        v, c, q = plc().louvain(h, G, 100, 1.0, False)
        out[mode] = (host(c), q)
    assert np.array_equal(out["wide"][0], out["sort"][0]) and out["wide"][1] == out["sort"][1]


def _nx_graph(s, d, w):
    import networkx as nx
    G = nx.Graph()
    G.add_weighted_edges_from(zip(s.tolist(), d.tolist(), w.tolist()))
    return G


@pytest.mark.parametrize("self_loops", [False, True])
def test_rmat14_quality_vs_networkx(self_loops):
    """The reference's Louvain quality rule (python/cugraph/cugraph/tests/
    test_louvain.py:96-103) on the bench's NetworkX-leg graph: RMAT-14, symmetrised,
    uniform [0, 1) weights (seed 43).  cugraph Q > 0.82 x the NetworkX Louvain Q
    (nx.community.louvain_communities(seed=42): python-louvain's best_partition, the
    reference's oracle, is absent) and cugraph's reported Q within 1e-4 of the
    NetworkX modularity of the returned partition.

    The datasets the reference runs this on have no self loops; RMAT-14 has 84.
    There NetworkX counts a self loop twice in a degree and once in m, the
    reference's stored-edge formula (common_methods.cuh:121-170) once in both, so
    with self loops the 1e-4 bar applies to the reference formula recomputed in
    fp64 and NetworkX's own convention must agree within 5e-4."""
    import networkx as nx
    s, d = rmat.rmat(14, 16 << 14, seed=42)
    w = rmat.rmat_weights(s.size, seed=43).astype(np.float64)
    s, d, w = og.symmetrize_dedup(s, d, w)
    if not self_loops:
        keep = s != d
        s, d, w = s[keep], d[keep], w[keep]
    assert (int((s == d).sum()) > 0) == self_loops
    w32 = w.astype(np.float32)
    h, G = make_graph(s, d, w32, symmetric=True)
    v, c, q = run(h, G)
    Gnx = _nx_graph(s, d, w32.astype(np.float64))
    q_nx = nx.community.modularity(Gnx, nx.community.louvain_communities(Gnx, weight="weight", resolution=1.0,
                                                                          seed=42), weight="weight")
    part = {}
    for x, k in zip(v.tolist(), c.tolist()):
        part.setdefault(k, set()).add(x)
    q_part_nx = nx.community.modularity(Gnx, list(part.values()), weight="weight")
    # the reference's formula on the stored (directed, symmetric) edges, fp64
    lab = dict(zip(v.tolist(), c.tolist()))
    cs = np.array([lab[x] for x in s.tolist()])
    cd = np.array([lab[x] for x in d.tolist()])
    ww = w32.astype(np.float64)
    m2 = ww.sum()
    kv = np.zeros(int(max(s.max(), d.max())) + 1)
    np.add.at(kv, s, ww)
    a = np.zeros(int(c.max()) + 1)
    np.add.at(a, c, kv[v])
    q_ref = ww[cs == cd].sum() / m2 - (a * a).sum() / (m2 * m2)
    print(f"RMAT-14 (self loops {self_loops}): cugraph Q {q:.6f}, recomputed {q_ref:.6f}, NetworkX modularity "
          f"of it {q_part_nx:.6f}, NetworkX Louvain Q {q_nx:.6f}")
    assert q > 0.82 * q_nx
    assert abs(q - q_ref) < 1e-4
    assert abs(q - q_part_nx) < (5e-4 if self_loops else 1e-4)


def test_rmat20_integer_vs_compiled_oracle():
    """The reference's Louvain usecase size (cpp/tests/community/louvain_test.cpp:430-442,
    RMAT(20, 32) symmetric): integer weights in [1, 4] keep every sum below 2^53
    (sum_c a_c^2 <= m^2 ~ 5.6e15), so the local-move gains, cluster weights and Q are
    exact in any order and the GPU must reproduce the oracle exactly: same clustering,
    same Q bits, same level count.  The oracle here is oracle/cpu_louvain.c (the numpy
    oracle's arithmetic compiled with OpenMP; tests/test_cpu_baseline.py pins the two
    together) on the oracle's own graph construction (oracle/graph.py)."""
    from oracle import cpu_native
    s, d = rmat.rmat(20, 16 << 20, seed=42)
    w = np.floor(rmat.rmat_weights(s.size, seed=43).astype(np.float64) * 4.0) + 1.0
    s, d, w = og.symmetrize_dedup(s, d, w)
    OG = og.create_graph(s, d, w, renumber=True)
    m = float(OG.weights.sum())
    assert m * m < 2.0**53
    h, G = make_graph(s, d, w.astype(np.float32), renumber=True, symmetric=True)
    v, c, q = run(h, G)
    levels = h.last_louvain_levels()
    assert np.array_equal(v, OG.number_map)
    oc, oq, olevels = cpu_native.louvain(OG.offsets, OG.indices, OG.weights, threads=16)
    print(f"RMAT-20 integer Louvain: V={OG.num_vertices} E={OG.num_edges} Q gpu {q!r} oracle {oq!r}, "
          f"levels {levels}/{olevels}, clusters {np.unique(c).size}")
    assert levels == olevels
    assert q == oq
    assert np.array_equal(c, oc)


@pytest.mark.parametrize("scale,wdtype", [(20, np.float32), (18, np.float64)])
def test_rmat_fractional_weights_vs_compiled_oracle(scale, wdtype):
    """R-MAT symmetric with random fractional weights: the bench's uniform [0, 1) fp32
    weights at RMAT-20, and fp64 weights (not rounded to fp32) at RMAT-18.  The sums
    are no longer exact: the GPU's cluster weights and pair sums are 64-bit fixed point
    (order-free), the oracle's fp64 in its own order, so near-tied gains may order
    differently and the partitions may differ (DESIGN.md §5 Louvain).  The bar is
    north_star's: the GPU's Q within 1e-6 relative of the compiled oracle's
    (oracle/cpu_louvain.c, same graph construction), and the reported Q within 1e-6 of
    the modularity of the returned partition recomputed in fp64."""
    from oracle import cpu_native
    s, d = rmat.rmat(scale, 16 << scale, seed=42)
    w = rmat.rmat_weights(s.size, seed=43).astype(np.float64)
    if wdtype == np.float32:
        w = w.astype(np.float32).astype(np.float64)
    s, d, w = og.symmetrize_dedup(s, d, w)
    OG = og.create_graph(s, d, w, renumber=True)
    h, G = make_graph(s, d, w.astype(wdtype), renumber=True, symmetric=True, wdtype=wdtype)
    v, c, q = run(h, G)
    levels = h.last_louvain_levels()
    assert np.array_equal(v, OG.number_map)
    oc, oq, olevels = cpu_native.louvain(OG.offsets, OG.indices, OG.weights, threads=16)
    src = np.repeat(np.arange(OG.num_vertices), np.diff(OG.offsets))
    q_part = olv.modularity(src, OG.indices, OG.weights, c)
    same = np.array_equal(c, oc)
    print(f"RMAT-{scale} {np.dtype(wdtype).name} weights: Q gpu {q!r} (recomputed {q_part!r}) oracle {oq!r}, "
          f"levels {levels}/{olevels}, clusters {np.unique(c).size}/{np.unique(oc).size}, identical clustering {same}")
    assert abs(q - oq) <= 1e-6 * abs(oq)
    assert abs(q - q_part) <= 1e-6 * abs(q_part)
