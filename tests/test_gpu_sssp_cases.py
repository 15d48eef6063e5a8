"""SSSP at the inputs its kernels branch on, every result through
tests/sssp_check.py (distances the oracle's fixed point bit for bit; predecessors
tight, a tree, and the deterministic rule -- checked at every vertex):

 * integer and zero weights: ties at most vertices, tight edges between vertices at
   one distance (k_sssp_pred_probe / _scan's strict test, k_sssp_pred_level);
 * the tight in-edge at a chosen position of the in-list (probe: the first 4; scan:
   16 at a time from the 5th);
 * stars: a row over several 2048-edge chunks, chunks of 2048+ one-edge slots, slots
   across chunk starts, in push (k_relax) and pull (k_pull), light and heavy;
 * graphs whose light or heavy part is empty, sources without (light) edges
   (k_sssp_init's last branches), unreachable parts and unused ids;
 * sssp_delta x sssp_pull: results bit-equal to the default's, the cached parts
   rebuilt when delta changes;
 * int64 / float64, cutoff with predecessors, fp32 sums that overflow.
"""
import functools

import numpy as np
import pytest

from gpu_util import host, make_graph, plc
from oracle import graph as og
from sssp_check import check_sssp, four_vertex, grid, rmat_edges

pytestmark = pytest.mark.gpu

INF = float("inf")


def call(h, G, source, cutoff=INF):
    v, d, p = plc().sssp(h, G, source, cutoff, True, False)
    return host(v), host(d), host(p).astype(np.int64)


def check(s, d, w, v, dist, pred, source, cutoff=INF):
    """The library's result (vertices v in internal order, external ids) against the
    checker, over external ids 0..max; ties by internal id (tie_key), as the library
    breaks them."""
    n_ext = int(max(np.max(s), np.max(d), np.max(v))) + 1
    G2 = og.create_graph(s, d, np.asarray(w, dist.dtype), renumber=False, vertices=np.arange(n_ext))
    key = np.empty(n_ext, np.int64)
    key[v] = np.arange(v.size)
    absent = np.setdiff1d(np.arange(n_ext), v)
    key[absent] = v.size + np.arange(absent.size)
    fd = np.full(n_ext, np.finfo(dist.dtype).max, dist.dtype)
    fp = np.full(n_ext, -1, np.int64)
    fd[v] = dist
    fp[v] = pred
    return check_sssp(G2.offsets, G2.indices, G2.weights, source, fd, fp, cutoff, tie_key=key)


def run_check(s, d, w, sources, symmetric, renumber=False, options=None, cutoff=INF, vdtype=np.int32,
              wdtype=np.float32):
    """One graph, every source (an external id, or a callable of the number map);
    returns the results."""
    h, G = make_graph(s, d, w, renumber=renumber, symmetric=symmetric, vdtype=vdtype, wdtype=wdtype, options=options)
    out, nm = [], None
    for src in sources:
        src = int(src(nm)) if callable(src) else int(src)
        v, dist, pred = call(h, G, src, cutoff)
        assert dist.dtype == wdtype
        nm = v if nm is None else nm
        assert np.array_equal(v, nm)
        check(s, d, w, v, dist, pred, src, cutoff)
        out.append((dist, pred))
    return out


# ---- weights with ties and zeros

@functools.lru_cache(maxsize=None)
def _rmat(scale, weights, symmetric):
    return rmat_edges(scale, weights, symmetric)


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("weights", [(1, 3), (0, 2)])
def test_rmat11_integer_weights(weights, symmetric):
    s, d, w = _rmat(11, weights, symmetric)
    run_check(s, d, w, [int(s[0]), lambda nm: nm[1], lambda nm: nm[nm.size // 2], lambda nm: nm[-1]], symmetric,
              renumber=True)


def test_four_vertex_zero_edge():
    s, d, w = four_vertex()
    (dist, pred), = run_check(s, d, w, [0], True)
    assert pred.tolist() == [-1, 3, 3, 0]
    run_check(s, d, w, [1, 2, 3], True)


@pytest.mark.parametrize("src", [0, 517, 1023])
def test_grid_zero_one_weights(src):
    run_check(*grid(32, "01"), [src], True)


def test_all_weights_zero():
    s, d, w = grid(32, "zero")
    (dist, pred), = run_check(s, d, w, [33], True)
    assert not dist.any()
    s, d, w = _rmat(11, "unit", False)
    run_check(s, d, np.zeros(s.size), [int(s[0]), int(d[-1])], False, renumber=True)


def test_self_loop_zero_weight():
    run_check([0, 1, 1, 2], [1, 1, 2, 2], [1.0, 0.0, 0.0, 0.0], [0], False)


def test_parallel_edges():
    """Both copies of 0 -> 1 are kept: the lighter one decides, either is a witness."""
    (dist, pred), = run_check([0, 0, 1, 0], [1, 1, 2, 2], [5.0, 2.0, 1.0, 7.0], [0], False)
    assert dist.tolist() == [0.0, 2.0, 3.0] and pred.tolist() == [-1, 0, 1]


# ---- the tight in-edge's position in the in-list

def _fan(k, tight):
    """0 -> mids 1..k -> sink k + 1; only the mids at the in-list positions `tight`
    are on a shortest path."""
    mids = np.arange(1, k + 1)
    s = np.concatenate([np.zeros(k, np.int64), mids])
    d = np.concatenate([mids, np.full(k, k + 1)])
    w2 = np.full(k, 2.0)
    w2[list(tight)] = 1.0
    return s, d, np.concatenate([np.ones(k), w2])


_POS = [(k, p) for k in (4, 5, 20, 21, 40) for p in sorted({0, 3, 4, 19, 20, k - 1}) if p < k]


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("k,p", _POS)
def test_pred_position(k, p, symmetric):
    s, d, w = _fan(k, [p])
    if symmetric:
        s, d, w = np.concatenate([s, d]), np.concatenate([d, s]), np.concatenate([w, w])
    (dist, pred), = run_check(s, d, w, [0], symmetric)
    assert dist[k + 1] == 2.0 and pred[k + 1] == p + 1


@pytest.mark.parametrize("tight,want", [((2, 10), 3), ((3, 4), 4), ((19, 20), 20), ((5, 36), 6)])
def test_pred_two_tight(tight, want):
    s, d, w = _fan(40, tight)
    (dist, pred), = run_check(s, d, w, [0], False)
    assert pred[41] == want


# ---- chunk edges: stars

def _star(L, variant, weights):
    """Hub 0, L leaves, symmetric.  "pendant": every fifth leaf has a vertex of its own
    behind it (one- and two-edge slots mixed); "gaps": the leaves take every other id,
    the ids between have no edges (empty rows inside the chunks a pull walks)."""
    step = 2 if variant == "gaps" else 1
    leaves = 1 + step * np.arange(L)
    a, b = np.zeros(L, np.int64), leaves
    if variant == "pendant":
        f = leaves[::5]
        a = np.concatenate([a, f])
        b = np.concatenate([b, leaves[-1] + 1 + np.arange(f.size)])
    if weights == "unit":
        w = np.ones(a.size)
    else:
        w = (np.random.default_rng(L).integers(1, 1 << 20, a.size) / float(1 << 20))
    return np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w]), int(leaves[-1])


@pytest.mark.parametrize("variant", ["plain", "pendant", "gaps"])
@pytest.mark.parametrize("L", [2047, 2048, 2049, 3 * 2048 + 1])
def test_star_chunks(L, variant):
    """From a leaf: the hub's row is one list entry over 1-4 chunks, then every leaf is
    a one-edge slot.  delta 0.25 makes the unit weights (and most random ones) heavy;
    pull -1 / default / 1 << 20: push only, by size, nearly always pull."""
    for weights in ("unit", "random"):
        s, d, w, leaf = _star(L, variant, weights)
        for delta in (0, 0.25):
            res = [run_check(s, d, w, [leaf, 0], True, options={"sssp_pull": pull, "sssp_delta": delta})
                   for pull in (-1, 0, 1 << 20)]
            for r in res[1:]:
                for (d0, p0), (d1, p1) in zip(res[0], r):
                    assert np.array_equal(d0, d1) and np.array_equal(p0, p1)


# ---- empty parts, sources without edges, unreachable parts

def _circulant(n, offs):
    a = np.repeat(np.arange(n), len(offs))
    b = (a + np.tile(np.asarray(offs), n)) % n
    return np.concatenate([a, b]), np.concatenate([b, a]), np.ones(2 * a.size)


def test_unit_weights_all_heavy():
    s, d, w = _rmat(11, "unit", True)
    assert s.size / np.unique(s).size > 8  # delta = 8 * 1 / average degree < 1: no light edge
    run_check(s, d, w, [int(s[0]), lambda nm: nm[-1]], True, renumber=True)


def test_unit_weights_all_light():
    s, d, w = grid(32, "unit")
    assert s.size / 1024 < 8
    run_check(s, d, w, [0, 500], True)


def test_unit_weights_degree_8():
    s, d, w = _circulant(257, [1, 2, 3, 4])  # delta = 8 * 1 / 8: w < delta is decided by rounding
    assert np.all(np.bincount(s) == 8)
    run_check(s, d, w, [0, 100], True)


def test_source_without_out_edges():
    (dist, pred), = run_check([1, 1, 2], [0, 2, 3], [1.0, 1.0, 1.0], [0], False)
    assert (dist < 3e38).sum() == 1


def test_source_with_heavy_edges_only():
    s, d, w = grid(32, "unit")
    heavy = (s == 40) | (d == 40)
    w = np.where(heavy, 100.0, w)
    run_check(s, d, w, [40, 0], True)


def test_isolated_source_gaps_and_components():
    """Ids 0..9 a path, 10..19 unused, 20..29 a second path, 31 the last id: sources in
    a component, on an unused id (no edges) and at the far end."""
    a = np.concatenate([np.arange(0, 9), np.arange(20, 29), [29]])
    b = np.concatenate([np.arange(1, 10), np.arange(21, 30), [31]])
    w = 1.0 + (np.arange(a.size) % 3)
    s, d, w = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])
    res = run_check(s, d, w, [0, 15, 31, 25], True)
    assert (res[1][0] < 3e38).sum() == 1 and (res[0][0] < 3e38).sum() == 10
    run_check(a, b, w[:a.size], [0, 15, 31], False)


# ---- options

_DEFAULT = {}


def _default_result(symmetric):
    if symmetric not in _DEFAULT:
        s, d, w = _rmat(12, "uniform", symmetric)
        h, G = make_graph(s, d, w, renumber=True, symmetric=symmetric)
        src = int(s[0])
        v, dist, pred = call(h, G, src)
        check(s, d, w, v, dist, pred, src)
        _DEFAULT[symmetric] = (src, v, dist, pred)
    return _DEFAULT[symmetric]


def _lib_delta(scale, w, nv):
    """delta as sssp.hip computes it (double arithmetic, then weight_t)."""
    avg_w, avg_deg = float(np.sum(np.asarray(w, np.float32).astype(np.float64))) / w.size, w.size / nv
    return np.float32(max((scale if scale > 0 else 8.0) * avg_w / avg_deg, 1e-30))


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("pull", [-1, 0, 1, 64])
@pytest.mark.parametrize("delta", [0.25, 1, 64, 1e6])
def test_options_do_not_change_a_bit(delta, pull, symmetric):
    s, d, w = _rmat(12, "uniform", symmetric)
    src, v0, d0, p0 = _default_result(symmetric)
    dmax = float(d0[d0 < np.finfo(np.float32).max].max())
    # far from where rounding absorbs delta (the threshold step's other branch)
    assert dmax / float(_lib_delta(delta, w, v0.size)) < 2.0 ** 20
    assert dmax / float(_lib_delta(0, w, v0.size)) < 2.0 ** 20
    h, G = make_graph(s, d, w, renumber=True, symmetric=symmetric, options={"sssp_delta": delta, "sssp_pull": pull})
    v, dist, pred = call(h, G, src)
    assert np.array_equal(v, v0) and np.array_equal(dist, d0) and np.array_equal(pred, p0)


@pytest.mark.parametrize("symmetric", [True, False])
def test_delta_changes_on_one_graph(symmetric):
    """A, B, A on one handle and graph: the cached light / heavy parts are rebuilt."""
    s, d, w = _rmat(12, "uniform", symmetric)
    src, v0, d0, p0 = _default_result(symmetric)
    h, G = make_graph(s, d, w, renumber=True, symmetric=symmetric)
    for delta in (0.25, 64, 0.25, 0, 1e6, 0):
        h.set_option("sssp_delta", delta)
        v, dist, pred = call(h, G, src)
        assert np.array_equal(dist, d0) and np.array_equal(pred, p0), f"sssp_delta {delta}"


# ---- types and limits

def test_int64_float64():
    s, d, w = _rmat(10, "uniform", True)
    run_check(s, d, w, [int(s[0]), lambda nm: nm[-1]], True, renumber=True, vdtype=np.int64, wdtype=np.float64)
    s, d, w = _rmat(10, (0, 2), False)
    run_check(s, d, w, [int(s[0]), lambda nm: nm[1]], False, renumber=True, vdtype=np.int64, wdtype=np.float64)


@pytest.mark.parametrize("weights,cutoff", [("uniform", 0.05), ((0, 2), 2.0), ((1, 3), 4.0)])
def test_cutoff_with_predecessors(weights, cutoff):
    s, d, w = _rmat(11, weights, True)
    res = run_check(s, d, w, [int(s[0]), lambda nm: nm[0], lambda nm: nm[nm.size // 2]], True, renumber=True,
                    cutoff=cutoff)
    big = np.finfo(np.float32).max
    assert any(((dist < big).sum() > 1) and ((dist == big).sum() > 0) for dist, _ in res)


def test_fp32_sum_overflows():
    """0 - 1 - 2 with weights 2e38: the second hop's sum is inf, not below any cutoff."""
    for symmetric in (False, True):
        s, d, w = [0, 1], [1, 2], [2e38, 2e38]
        if symmetric:
            s, d, w = s + d, d + s, w + w
        (dist, pred), = run_check(s, d, w, [0], symmetric)
        assert dist[1] == np.float32(2e38) and dist[2] == np.finfo(np.float32).max and pred.tolist() == [-1, 0, -1]


def test_delta_absorbed_by_rounding():
    """A 64-vertex unit-weight path with sssp_delta 1e-9: delta is about 5e-10, so from
    the first far split on mf + delta == mf in fp32 and the threshold moves by
    sssp_threshold.hpp's one-ulp step (tests/test_sssp_threshold.py sweeps that
    function on the host): 63 buckets of one vertex each."""
    a = np.arange(63)
    s, d, w = np.concatenate([a, a + 1]), np.concatenate([a + 1, a]), np.ones(126)
    assert np.float32(1.0) + _lib_delta(1e-9, w, 64) == np.float32(1.0)
    (dist, pred), = run_check(s, d, w, [0], True, options={"sssp_delta": 1e-9})
    assert np.array_equal(dist, np.arange(64, dtype=np.float32))
