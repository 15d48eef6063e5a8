"""Uniform neighbour sampling and random walks on the GPU against the numpy twin (tests/sampling_ref.py).
Every comparison is exact: the sample is a pure function of (sample_seed, hop, slot, row), whichever kernel
tier (sample_path) handled the row.

Most cases run on one directed graph whose first twelve vertices have the out-degrees of LADDER (a sink, a
single neighbour, K - 1 / K / K + 1 for K = 10, one wave minus one / one wave / plus one / plus two, more
than two waves, more than a block's worth of row, and a row of 70000 that has to be spread over the grid);
the other vertices have out-degree 0 or 1 (vertices 12..139 lead back into the ladder, so hops and walks
keep meeting it)."""
import functools
import json
import os

import numpy as np
import pytest
from scipy.stats import chi2

import sampling_ref as ref
from conftest import GOLDEN, dataset_path
from gpu_util import host, make_graph, plc

pytestmark = pytest.mark.gpu

LADDER = [0, 1, 9, 10, 11, 63, 64, 65, 66, 130, 4097, 70000]
NV = 70001
FANS = [(10,), (1, 2), (-1,), (3, -1), (65,), (10, 5, 3)]


@functools.lru_cache(maxsize=None)
def ladder_edges():
    rng = np.random.default_rng(20240607)
    src, dst = [], []
    for r, d in enumerate(LADDER):
        # short rows point into the first 140 vertices, so later hops meet the ladder again
        src.append(np.full(d, r, dtype=np.int64))
        dst.append(rng.choice(140 if d <= 130 else NV, size=d, replace=False))
    near = np.arange(12, 140)  # each of these leads back to a ladder vertex that has out-edges
    src.append(near)
    dst.append(rng.integers(1, 12, size=len(near)))
    odd = np.arange(141, NV, 2)
    src.append(odd)
    dst.append(np.concatenate([[NV - 1], rng.integers(0, NV, size=len(odd) - 1)]))
    src, dst = np.concatenate(src), np.concatenate(dst).astype(np.int64)
    order = rng.permutation(len(src))
    w = rng.integers(1, 8, size=len(src)).astype(np.float32)
    return src[order], dst[order], w


@functools.lru_cache(maxsize=None)
def ladder_csr():
    return ref.build_csr(*ladder_edges(), NV)


@functools.lru_cache(maxsize=None)
def ladder_starts():
    return tuple(np.random.default_rng(5).permutation(np.repeat(np.arange(12), 2)).tolist())


def bits(w):
    return w.view(np.int32 if w.dtype == np.float32 else np.int64).astype(np.int64)


def canon(s, d, w, c):
    s, d, c = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64), np.asarray(c, dtype=np.int64)
    order = np.lexsort((bits(w), d, s))
    return s[order], d[order], w[order], c[order]


def gpu_sample(h, g, starts, fan, repl, seed=0, path=0, vdtype=np.int32):
    h.set_option("sample_seed", seed)
    h.set_option("sample_path", path)
    out = plc().uniform_neighbor_sample(h, g, np.asarray(starts, dtype=vdtype), np.asarray(fan, dtype=np.int32),
                                        repl, False, return_counts=True)
    return canon(*[host(t) for t in out])


def same(a, b):
    return all(x.dtype.kind == y.dtype.kind and np.array_equal(x, y) for x, y in zip(a[:2] + a[3:], b[:2] + b[3:])) \
        and np.array_equal(bits(a[2]), bits(b[2])) and a[2].dtype == b[2].dtype


class Ladder:
    def __init__(self):
        s, d, w = ladder_edges()
        self.h, self.g = make_graph(s, d, w, renumber=False)
        self.cache = {}

    def sample(self, fan, repl, seed=0, path=0):
        key = (tuple(fan), repl, seed, path)
        if key not in self.cache:
            self.cache[key] = gpu_sample(self.h, self.g, ladder_starts(), fan, repl, seed, path)
        return self.cache[key]


@pytest.fixture(scope="module")
def ladder():
    return Ladder()


@functools.lru_cache(maxsize=None)
def twin_sample(fan, repl, seed):
    return canon(*ref.neighbor_sample(ladder_csr(), ladder_starts(), fan, repl, seed))


# ---------------------------------------------------------------- neighbour sample against the twin
@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("repl", [True, False])
@pytest.mark.parametrize("fan", FANS)
def test_sample_matches_twin_on_every_path(ladder, fan, repl, seed):
    want = twin_sample(fan, repl, seed)
    assert len(want[0]) > 0
    for path in (0, 1, 2):
        got = ladder.sample(fan, repl, seed, path)
        assert got[0].shape == want[0].shape, (path, got[0].shape, want[0].shape)
        assert same(got, want), path


def variant_edges(kind):
    s, d, w = ladder_edges()
    if kind == "multigraph":  # two parallel edges of equal weight, two of different weight
        return (np.array([0, 0, 0, 0, 1, 2]), np.array([1, 1, 2, 2, 2, 0]),
                np.array([3, 3, 4, 5, 1, 1], dtype=np.float32), 3)
    return s, d, (None if kind == "unweighted" else w), NV


def id_maps(p, h, g, ext, s, d):
    """A renumbered graph of the edges (ext[s], ext[d]), ext[v] = 3 v + 5: (number_map, to_int) with internal
    id k being external number_map[k] and to_int[v] the internal id of vertex v (-1: v is in no edge, the
    graph does not have it).  The twin works in internal ids."""
    number_map = host(p.sssp(h, g, int(ext[s[0]]), 1e30, False, False)[0]).astype(np.int64)
    assert np.array_equal(np.sort(number_map), ext[np.union1d(s, d)])
    to_int = np.full(len(ext), -1, dtype=np.int64)
    to_int[(number_map - 5) // 3] = np.arange(len(number_map))
    return number_map, to_int


@pytest.mark.parametrize("kind", ["int64", "float64", "renumbered", "transposed", "unweighted", "multigraph"])
def test_sample_matches_twin_on_other_graph_kinds(kind):
    s, d, w, nv = variant_edges(kind)
    vdtype = np.int64 if kind == "int64" else np.int32
    wdtype = np.float64 if kind == "float64" else np.float32
    ext = np.arange(nv) * 3 + 5 if kind == "renumbered" else np.arange(nv)  # sparse external ids
    p = plc()
    h = p.ResourceHandle()
    props = p.GraphProperties(is_symmetric=False, is_multigraph=kind == "multigraph")
    g = p.SGGraph(h, props, ext[s].astype(vdtype), ext[d].astype(vdtype), None if w is None else w.astype(wdtype),
                  store_transposed=kind == "transposed", renumber=kind == "renumbered")
    number_map, to_int = id_maps(p, h, g, ext, s, d) if kind == "renumbered" else (ext, np.arange(nv))
    csr = ref.build_csr(to_int[s], to_int[d], None if w is None else w.astype(wdtype), len(number_map))
    starts = np.asarray([0, 1, 2, 0] if kind == "multigraph" else ladder_starts())
    for fan, repl in [((10, 5, 3), False), ((3, -1), True), ((2,), False), ((1, 2), True)]:
        ws, wd, ww, wc = ref.neighbor_sample(csr, to_int[starts], fan, repl, 0)
        want = canon(number_map[ws], number_map[wd], ww, wc)
        for path in (1, 2):
            got = gpu_sample(h, g, ext[starts], fan, repl, 0, path, vdtype)
            assert got[0].shape == want[0].shape and same(got, want), (fan, repl, path)
        if kind == "unweighted":
            assert got[2].dtype == np.float32 and np.all(got[2] == 1.0)
        if kind == "multigraph":  # the equal-weight pair is one triple, the other pair is two
            keys = list(zip(got[0].tolist(), got[1].tolist(), got[2].tolist()))
            assert len(keys) == len(set(keys))
            if fan == (10, 5, 3):  # row 0 is taken whole by its two slots
                assert (0, 1, 3.0) in keys and (0, 2, 4.0) in keys and (0, 2, 5.0) in keys
                assert sum(1 for k in keys if k[:2] == (0, 1)) == 1
                assert got[3][keys.index((0, 1, 3.0))] >= 4 and got[3][keys.index((0, 2, 4.0))] >= 2


# ---------------------------------------------------------------- properties that need no twin
@functools.lru_cache(maxsize=None)
def edge_weight_table():
    s, d, w = ladder_edges()  # a simple graph: (source, destination) -> weight
    key = s * NV + d
    order = np.argsort(key)
    assert len(np.unique(key)) == len(key)
    return key[order], w[order]


def assert_edges_of_input(s, d, w):
    key, wt = edge_weight_table()
    k = s * NV + d
    at = np.searchsorted(key, k)
    assert np.all(at < len(key)) and np.array_equal(key[at], k), "a returned pair is no edge of the input"
    assert np.array_equal(wt[at], w), "a returned edge does not carry its own weight"


@pytest.mark.parametrize("repl", [True, False])
@pytest.mark.parametrize("fan", FANS)
def test_every_returned_triple_is_an_input_edge(ladder, fan, repl):
    s, d, w, c = ladder.sample(fan, repl)
    assert_edges_of_input(s, d, w)
    assert np.all(c >= 1)
    assert len(np.unique(np.stack([s, d], axis=1), axis=0)) == len(s)


@pytest.mark.parametrize("k", [10, 65])
def test_one_hop_without_replacement_takes_min_k_d_distinct_edges(ladder, k):
    # every start once: exactly min(K, d) distinct edges, each drawn once
    s, d, w, c = gpu_sample(ladder.h, ladder.g, np.arange(12), (k,), False)
    for v, deg in enumerate(LADDER):
        mine = s == v
        assert mine.sum() == min(k, deg), (v, deg)
        assert np.all(c[mine] == 1)
    # every start twice: the two slots of a start draw independently (the slot number is part of the draw), so
    # a row taken whole comes back with count 2, and a sampled row with 2 K picks, no edge more than twice
    s, d, w, c = ladder.sample((k,), False)
    for v, deg in enumerate(LADDER):
        mine = s == v
        assert c[mine].sum() == 2 * min(k, deg), (v, deg)
        assert np.all(c[mine] <= 2) and min(k, deg) <= mine.sum() <= min(2 * k, deg)
        if deg <= k:
            assert np.all(c[mine] == 2)


def test_one_hop_with_replacement_draws_k_per_slot(ladder):
    s, d, w, c = ladder.sample((10,), True)
    for v, deg in enumerate(LADDER):
        assert c[s == v].sum() == (0 if deg == 0 else 20), (v, deg)


@pytest.mark.parametrize("repl", [True, False])
def test_fan_out_minus_one_returns_the_out_edges_of_the_starts(ladder, repl):
    s, d, w, c = ladder.sample((-1,), repl)
    es, ed, ew = ladder_edges()
    keep = es < 12
    want = canon(es[keep], ed[keep], ew[keep], np.full(keep.sum(), 2))
    assert same((s, d, w, c), want)


def test_two_calls_give_identical_arrays(ladder):
    p = plc()
    starts, fan = np.asarray(ladder_starts(), dtype=np.int32), np.asarray([10, 5, 3], dtype=np.int32)
    ladder.h.set_option("sample_seed", 0)
    ladder.h.set_option("sample_path", 0)
    a = [host(t) for t in p.uniform_neighbor_sample(ladder.h, ladder.g, starts, fan, False, False)]
    b = [host(t) for t in p.uniform_neighbor_sample(ladder.h, ladder.g, starts, fan, False, False)]
    assert len(a) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_another_seed_gives_another_sample_of_the_long_row(ladder):
    a, b = ladder.sample((10,), False, seed=0), ladder.sample((10,), False, seed=7)
    assert not np.array_equal(a[1][a[0] == 11], b[1][b[0] == 11])


def test_with_replacement_is_uniform_over_a_row(ladder):
    """2800 slots of the degree-65 vertex, fan-out 10 with replacement: the counts of its 65 edges against
    the uniform distribution, 64 degrees of freedom, the 1 - 1e-6 quantile.  Deterministic given the seed."""
    s, d, w, c = gpu_sample(ladder.h, ladder.g, [7] * 2800, (10,), True, seed=0)
    assert np.all(s == 7) and c.sum() == 28000
    got = np.concatenate([c, np.zeros(65 - len(c), dtype=np.int64)])
    e = 28000 / 65
    stat = float(((got - e) ** 2 / e).sum())
    print(f"chi2 {stat:.1f}, bound {chi2.ppf(1 - 1e-6, 64):.1f}")
    assert stat < chi2.ppf(1 - 1e-6, 64)


def test_reference_golden_cases():
    with open(os.path.join(GOLDEN, "sampling_vectors.json")) as f:
        v = json.load(f)
    for case in v["cases"]:
        ids = np.asarray(case["edge_ids"], dtype=np.int32)
        h, g = make_graph(case["src"], case["dst"], ids.view(np.float32), renumber=False)
        own = {(a, b): i for a, b, i in zip(case["src"], case["dst"], case["edge_ids"])}
        for path in (0, 1, 2):
            s, d, w, c = gpu_sample(h, g, case["start"], case["fan_out"], case["with_replacement"], 0, path)
            assert len(s) > 0
            for a, b, i in zip(s.tolist(), d.tolist(), w.view(np.int32).tolist()):
                assert own[(a, b)] == i  # every returned edge carries its own id, bit for bit
            if case["fan_out"] == [-1]:
                assert sorted(zip(s.tolist(), d.tolist())) == sorted(k for k in own if k[0] in case["start"])


# ---------------------------------------------------------------- walks
def gpu_walks(h, g, starts, length, seed, biased, vdtype=np.int32):
    h.set_option("sample_seed", seed)
    f = plc().biased_random_walks if biased else plc().uniform_random_walks
    paths, weights, got_length = f(h, g, np.asarray(starts, dtype=vdtype), length)
    assert got_length == length
    n = len(starts)
    return host(paths).reshape(n, length + 1), None if weights is None else host(weights).reshape(n, length)


WALK_STARTS = tuple(np.tile(np.arange(12), 2).tolist() + [0, 0])


@pytest.mark.parametrize("seed", [0, 7])
@pytest.mark.parametrize("length", [1, 5, 40])
@pytest.mark.parametrize("biased", [False, True])
def test_walks_match_twin(ladder, biased, length, seed):
    paths, weights = gpu_walks(ladder.h, ladder.g, WALK_STARTS, length, seed, biased)
    want_paths, want_weights = ref.walks(ladder_csr(), WALK_STARTS, length, seed, biased)
    assert paths.dtype == np.int32 and weights.dtype == np.float32
    assert np.array_equal(paths, want_paths) and np.array_equal(weights, want_weights)
    # every consecutive pair is an edge with its weight; after the sink a row is -1 / 0
    for row, wrow in zip(paths, weights):
        live = int((row >= 0).sum())
        assert np.all(row[:live] >= 0) and np.all(row[live:] == -1) and np.all(wrow[max(live - 1, 0):] == 0)
        if live > 1:
            assert_edges_of_input(row[:live - 1].astype(np.int64), row[1:live].astype(np.int64), wrow[:live - 1])
        if live <= length:
            assert ladder_csr()[0][row[live - 1] + 1] == ladder_csr()[0][row[live - 1]]  # it ended at a sink
    assert np.all(paths[-1, 1:] == -1)  # vertex 0 is the sink


@pytest.mark.parametrize("kind", ["int64", "renumbered", "unweighted"])
def test_walks_match_twin_on_other_graph_kinds(kind):
    s, d, w, nv = variant_edges(kind)
    vdtype = np.int64 if kind == "int64" else np.int32
    ext = np.arange(nv) * 3 + 5 if kind == "renumbered" else np.arange(nv)
    p = plc()
    h = p.ResourceHandle()
    g = p.SGGraph(h, p.GraphProperties(), ext[s].astype(vdtype), ext[d].astype(vdtype), w, store_transposed=False,
                  renumber=kind == "renumbered")
    number_map, to_int = id_maps(p, h, g, ext, s, d) if kind == "renumbered" else (ext, np.arange(nv))
    csr = ref.build_csr(to_int[s], to_int[d], w, len(number_map))
    starts = np.asarray(WALK_STARTS)
    for biased in ([False] if w is None else [False, True]):
        paths, weights = gpu_walks(h, g, ext[starts], 5, 0, biased, vdtype)
        want_paths, want_weights = ref.walks(csr, to_int[starts], 5, 0, biased)
        want_paths = np.where(want_paths >= 0, number_map[np.maximum(want_paths, 0)], -1)
        assert paths.dtype == vdtype and np.array_equal(paths, want_paths)
        if w is None:
            assert weights is None  # the unweighted graph has no weights array
        else:
            assert np.array_equal(weights, want_weights)


def star(weights, wdtype=np.float32):
    """Vertex 0 with one edge of every given weight, to vertices 1, 2, ..."""
    n = len(weights)
    return make_graph(np.zeros(n, dtype=np.int64), np.arange(1, n + 1), None if weights[0] is None else weights,
                      renumber=False, wdtype=wdtype)


def test_biased_walk_never_takes_a_zero_weight():
    h, g = star([0, 0, 5])
    paths, weights = gpu_walks(h, g, [0] * 200, 1, 0, True)
    assert np.all(paths[:, 1] == 3) and np.all(weights == 5)


def test_biased_walk_stops_on_a_row_of_zero_total():
    h, g = star([0, 0])
    paths, weights = gpu_walks(h, g, [0, 0], 2, 0, True)
    assert np.all(paths[:, 1:] == -1) and np.all(weights == 0)


def test_biased_walk_needs_weights_without_negatives():
    h, g = star([None, None])
    with pytest.raises(ValueError, match="weighted"):
        plc().biased_random_walks(h, g, np.asarray([0], dtype=np.int32), 2)
    h, g = star([1, -1, 2])
    with pytest.raises(ValueError, match="non-negative"):
        plc().biased_random_walks(h, g, np.asarray([0], dtype=np.int32), 2)
    paths, _ = gpu_walks(h, g, [0], 1, 0, False)  # a uniform walk does not mind
    assert paths[0, 1] in (1, 2, 3)


BIASED_SEED = 0


def test_biased_walk_follows_the_weights():
    """2000 walks of one step from a vertex with weights 1..7: the destinations against w / 28, 6 degrees of
    freedom, the 1 - 1e-6 quantile; the twin itself sits above p = 1e-3 for this seed."""
    w = np.arange(1, 8, dtype=np.float32)
    csr = ref.build_csr(np.zeros(7, dtype=np.int64), np.arange(1, 8), w, 8)
    twin, _ = ref.walks(csr, [0] * 2000, 1, BIASED_SEED, True)
    e = 2000 * w / 28

    def stat(paths):
        got = np.bincount(paths[:, 1], minlength=8)[1:]
        return float(((got - e) ** 2 / e).sum())
    assert chi2.sf(stat(twin), 6) > 1e-3
    h, g = star(w)
    paths, _ = gpu_walks(h, g, [0] * 2000, 1, BIASED_SEED, True)
    print(f"chi2 {stat(paths):.2f} (twin {stat(twin):.2f}), bound {chi2.ppf(1 - 1e-6, 6):.1f}")
    assert stat(paths) < chi2.ppf(1 - 1e-6, 6)
    assert np.array_equal(paths, twin)


# ---------------------------------------------------------------- errors and stubs
def test_argument_errors(ladder):
    p = plc()
    fan = np.asarray([2], dtype=np.int32)
    with pytest.raises(ValueError, match="not in the graph"):
        p.uniform_neighbor_sample(ladder.h, ladder.g, np.asarray([0, NV + 3], dtype=np.int32), fan, True, False)
    with pytest.raises(ValueError, match="levels"):
        p.uniform_neighbor_sample(ladder.h, ladder.g, np.asarray([0], dtype=np.int32),
                                  np.zeros(0, dtype=np.int32), True, False)
    with pytest.raises(ValueError, match="fan_out should be of type int"):
        p.uniform_neighbor_sample(ladder.h, ladder.g, np.asarray([0], dtype=np.int32),
                                  np.asarray([2], dtype=np.int64), True, False)
    with pytest.raises(ValueError, match="vertex type"):
        p.uniform_neighbor_sample(ladder.h, ladder.g, np.asarray([0], dtype=np.int64), fan, True, False)
    with pytest.raises(ValueError, match="vertex type"):
        p.uniform_random_walks(ladder.h, ladder.g, np.asarray([0], dtype=np.int64), 3)
    with pytest.raises(ValueError, match="not in the graph"):
        p.uniform_random_walks(ladder.h, ladder.g, np.asarray([-1], dtype=np.int32), 3)
    with pytest.raises(ValueError, match="sample_path"):
        ladder.h.set_option("sample_path", 3)
    with pytest.raises(ValueError, match="sample_seed"):
        ladder.h.set_option("sample_seed", 2.0**53)


def test_node2vec_is_a_stub(ladder):
    with pytest.raises(NotImplementedError, match="node2vec sampling is not implemented in this build"):
        plc().node2vec(ladder.h, ladder.g, np.asarray([1], dtype=np.int32), 4, False, 1.0, 1.0)


def test_result_getters_and_the_testing_constructor(ladder):
    """A sample call leaves start labels and the reference's host counts unset (NULL); a result made by
    cugraph_test_sample_result_create returns copies of the four arrays it was given."""
    import ctypes
    import torch
    from pylibcugraph import _lib
    from pylibcugraph._arrays import DeviceView, copy_view_to_tensor
    lib, h = _lib.lib, ladder.h.ptr
    start, fan = DeviceView(np.asarray([3, 4], dtype=np.int32)), np.asarray([2], dtype=np.int32)
    fview = lib.cugraph_type_erased_host_array_view_create(fan.ctypes.data_as(ctypes.c_void_p), 1, _lib.INT32)
    res = ctypes.c_void_p()
    _lib.call("cugraph_uniform_neighbor_sample", h, ladder.g.c_graph_ptr, start.ptr, fview, 0, 0, ctypes.byref(res))
    lib.cugraph_type_erased_host_array_view_free(fview)
    assert lib.cugraph_sample_result_get_start_labels(res) is None
    assert lib.cugraph_sample_result_get_counts(res) is None
    counts = copy_view_to_tensor(h, lib.cugraph_amd_sample_result_get_counts(res))
    assert counts.dtype == torch.int32 and counts.tolist() == [1, 1, 1, 1]
    lib.cugraph_sample_result_free(res)

    given = [np.asarray([0, 1, 2], dtype=np.int32), np.asarray([1, 2, 0], dtype=np.int32),
             np.asarray([0.5, 1.5, 2.5], dtype=np.float32), np.asarray([3, 1, 2], dtype=np.int32)]
    views = [DeviceView(a) for a in given]
    res = ctypes.c_void_p()
    _lib.call("cugraph_test_sample_result_create", h, *[v.ptr for v in views], ctypes.byref(res))
    getters = [lib.cugraph_sample_result_get_sources, lib.cugraph_sample_result_get_destinations,
               lib.cugraph_sample_result_get_index, lib.cugraph_amd_sample_result_get_counts]
    for get, want in zip(getters, given):
        got = host(copy_view_to_tensor(h, get(res)))
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert lib.cugraph_sample_result_get_start_labels(res) is None
    hv = lib.cugraph_sample_result_get_counts(res)  # the reference's getter: a host view
    assert lib.cugraph_type_erased_host_array_size(hv) == 3 and lib.cugraph_type_erased_host_array_type(hv) == _lib.INT32
    back = np.ctypeslib.as_array(ctypes.cast(lib.cugraph_type_erased_host_array_pointer(hv),
                                             ctypes.POINTER(ctypes.c_int32)), shape=(3,)).copy()
    assert back.tolist() == [3, 1, 2]
    lib.cugraph_type_erased_host_array_view_free(hv)
    lib.cugraph_sample_result_free(res)

    # walks: no path sizes
    res = ctypes.c_void_p()
    _lib.call("cugraph_uniform_random_walks", h, ladder.g.c_graph_ptr, start.ptr, 3, ctypes.byref(res))
    assert lib.cugraph_random_walk_result_get_path_sizes(res) is None
    assert lib.cugraph_random_walk_result_get_max_path_length(res) == 3
    lib.cugraph_random_walk_result_free(res)


# ---------------------------------------------------------------- the cugraph layer
@functools.lru_cache(maxsize=None)
def karate():
    import cugraph
    import pandas as pd
    from oracle import graph as og
    s, d, w = og.read_csv(dataset_path("karate.csv"))
    G = cugraph.Graph()
    G.from_pandas_edgelist(pd.DataFrame({"src": s, "dst": d, "w": w.astype(np.float32)}), "src", "dst", "w")
    return G, set(zip(s.tolist(), d.tolist())) | set(zip(d.tolist(), s.tolist()))


def test_cugraph_uniform_neighbor_sample_on_karate():
    import cugraph
    G, edges = karate()
    for repl in (True, False):
        df = cugraph.uniform_neighbor_sample(G, [0, 5, 33, 0], [3, 2], with_replacement=repl)
        assert list(df.columns) == ["sources", "destinations", "indices"] and len(df) > 0
        assert all((a, b) in edges for a, b in zip(df["sources"], df["destinations"]))
        assert set(df["sources"]) >= {0, 5, 33}
    df = cugraph.uniform_neighbor_sample(G, 0, [-1])
    assert sorted(df["destinations"]) == sorted(b for a, b in edges if a == 0)


def test_cugraph_random_walks_padded_and_unpadded_agree():
    import cugraph
    G, edges = karate()
    starts = [0, 33, 5, 0]
    pv, pw, ps = cugraph.random_walks(G, starts, max_depth=6, use_padding=True)
    cv, cw, cs = cugraph.random_walks(G, starts, max_depth=6, use_padding=False)
    assert len(pv) == 4 * 6 and len(pw) == 4 * 5 and list(ps) == list(cs) == [6] * 4  # karate has no sink
    assert list(cv) == list(pv) and list(cw) == list(pw)
    rows = np.asarray(pv).reshape(4, 6)
    assert list(rows[:, 0]) == starts
    assert all((a, b) in edges for r in rows for a, b in zip(r[:-1], r[1:]))
    # a directed path 0 -> 1 -> 2: the walks stop at 2, the sizes say where
    import pandas as pd
    D = cugraph.DiGraph()
    D.from_pandas_edgelist(pd.DataFrame({"s": [0, 1], "d": [1, 2]}), "s", "d", renumber=False)
    pv, pw, ps = cugraph.random_walks(D, [0, 1, 2], max_depth=4, use_padding=True)
    cv, cw, cs = cugraph.random_walks(D, [0, 1, 2], max_depth=4, use_padding=False)
    assert list(ps) == list(cs) == [3, 2, 1]
    assert list(pv) == [0, 1, 2, -1, 1, 2, -1, -1, 2, -1, -1, -1] and list(cv) == [0, 1, 2, 1, 2, 2]
    assert list(pw) == [1, 1, 0, 1, 0, 0, 0, 0, 0] and list(cw) == [1, 1, 1]
