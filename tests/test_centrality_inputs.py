"""The inputs of tests/test_gpu_centrality_cases.py, checked on the CPU oracle: the
graphs have the rows the kernels branch on, the oracle converges where it is asked
to, the stop threshold can be taken from its trace, and a wrong kernel would be seen
-- hubs differ from authorities, a guess changes an early result, one dropped edge of
the 4097-edge row moves the result by well over the bar.  No GPU."""
import numpy as np
import pytest

import centrality_cases as cc
from oracle import centrality as oc

BOUNDS = (0, 1, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 4095, 4096)


def test_bins_graph_shape():
    s, d = cc.bins_graph()
    L = cc.layout("bins", False)
    assert L.n == cc.BINS_NV == 4118 and 16500 < s.size < 17500
    assert np.unique(s * L.n + d).size == s.size
    assert set(BOUNDS) <= set(L.indeg.tolist()) and 4097 in L.indeg
    assert all(L.indeg[z] == 0 and L.outdeg[z] == 1 for z in cc.ZEROS)
    assert (L.indeg == 0).sum() == len(cc.ZEROS)
    assert L.outdeg.max() >= 4096 and (L.outdeg == 0).sum() == 0
    # the spread ids keep the structure and leave gaps
    R = cc.layout("bins", True)
    assert R.n == L.n and np.array_equal(R.ids, cc.spread(np.arange(L.n)))
    assert np.array_equal(R.indeg, L.indeg) and np.array_equal(R.outdeg, L.outdeg)


def test_rmat_directed_shape():
    s, d = cc.rmat_directed()
    R, L = cc.layout("rmat", True), cc.layout("rmat", False)
    assert (R.n, s.size, R.indeg.max(), R.outdeg.max()) == (818, 6693, 245, 233)
    assert R.n < L.n <= 1024  # unrenumbered: vertices without an edge
    have = set(zip(s.tolist(), d.tolist()))
    assert sum((b, a) not in have for a, b in have) > s.size // 2  # directed


def test_weights_exact_in_fp32():
    for g in cc.GRAPHS:
        w = cc.layout(g, True).w
        assert np.array_equal(w.astype(np.float32).astype(np.float64), w) and w.min() > 0 and w.max() <= 1
        assert np.unique(w).size == 8


def test_choose_stop_rule():
    assert cc.choose_stop([100, 50, 20, 4, 2, 1]) == (4, np.sqrt(80.0))
    assert cc.choose_stop([100, 50, 20, 10, 2, 1]) == (5, np.sqrt(20.0))
    assert cc.choose_stop([100, 50, 25, 12, 6, 3]) is None
    # the threshold of the first k is under the floor: an earlier k
    assert cc.choose_stop([100, 10, 5, 1], floor=3.0) == (2, np.sqrt(1000.0))
    assert cc.choose_stop([100, 50, 5, 1], floor=20.0) is None
    # an earlier difference too close to the threshold
    assert cc.choose_stop([100, 3, 20, 4, 2, 0.25]) == (6, np.sqrt(0.5))


@pytest.mark.parametrize("graph", list(cc.GRAPHS))
def test_oracle_katz_and_hits_converge(graph):
    L = cc.layout(graph, True)
    for weighted in (False, True):
        x, trace = oc.katz(L.n, L.cs, L.cd, L.weights(weighted), L.alpha, 1.0, 1e-11, 100, return_trace=True)
        assert len(trace) < 50 and np.all(x > 0)
    h, a, diff, it = oc.hits(L.n, L.cs, L.cd, 1e-11, 100)
    assert it < 50 and diff < 1e-11


def test_oracle_eigenvector_converges_on_rmat():
    L = cc.layout("rmat", True)
    for weighted in (False, True):
        x, trace = oc.eigenvector_centrality(L.n, L.cs, L.cd, L.weights(weighted), 1e-13 / L.n, 100, return_trace=True)
        assert len(trace) < 50


def _check_stop(trace, stop, floor):
    assert stop is not None
    k, thr = stop
    assert trace[k - 1] * 2 <= thr <= min(trace[:k - 1]) / 2 and thr >= floor


def test_stop_rule_finds_every_case():
    for case in cc.KATZ_CASES + cc.KATZ_BETAS_CASES:
        for dtype in (np.float32, np.float64):
            r = cc.katz_ref(*case, dtype=dtype)
            L = cc.layout(case[0], case[1])
            _check_stop(r["trace"], r["stop"], cc.l1_floor(L.n, np.abs(r["raw"]).max()))
            assert r["iterations"] == r["stop"][0] >= 2
    for case in cc.EIGENVECTOR_CASES:
        r = cc.eigenvector_ref(*case)
        L = cc.layout(case[0], case[1])
        _check_stop(r["trace"], r["stop"], cc.l1_floor(L.n, np.abs(r["values"]).max()))
        assert r["epsilon"] * L.n == pytest.approx(r["stop"][1]) and r["iterations"] >= 4
    for graph in cc.HITS_STOP_GRAPHS:
        for renumber in (True, False):
            k, thr = cc.hits_stop(graph, renumber)
            assert k >= 4 and thr >= cc.l1_floor(cc.layout(graph, renumber).n, 1.0)
            # the oracle reports the index of the iteration that stopped
            assert cc.hits_ref(graph, renumber, thr, 100)[3] == k - 1


def test_hits_differences_on_bins_fall_too_slowly():
    """Why bins_graph() has no trace-chosen HITS run: from the fourth iteration on no
    difference is a quarter of the one before."""
    L = cc.layout("bins", True)
    trace = np.asarray(cc.hits_trace(L))
    assert cc.hits_stop("bins", True) is None and cc.hits_stop("bins", False) is None
    assert trace.size > 10 and trace[-1] < 1e-9 and np.all(trace[2:-1] / trace[3:] < 4)


def test_hubs_differ_from_authorities():
    for graph in cc.HITS_GRAPHS:
        for normalized in (True, False):
            h, a, _, _ = cc.hits_ref(graph, True, 0.0, cc.HITS_FIXED_ITERATIONS, normalized)
            assert cc.scaled_error(h, a) > 100 * cc.BAR32 and cc.scaled_error(a, h) > 100 * cc.BAR32


@pytest.mark.parametrize("graph,count", cc.GUESS_CASES)
def test_guess_changes_an_early_result(graph, count):
    L = cc.layout(graph, True)
    ids, vals, full = cc.guess_arrays(L, count)
    assert ids.size == count and np.unique(ids).size == count and vals.min() >= 0.1 and vals.max() < 1.1
    assert np.any(np.diff(ids) < 0) and np.count_nonzero(full) == count
    for iterations in (1, 2):
        h, a, _, _ = cc.hits_ref(graph, True, 0.0, iterations, True, count)
        h0, a0, _, _ = cc.hits_ref(graph, True, 0.0, iterations)
        assert cc.scaled_error(h0, h) > 100 * cc.BAR32 and cc.scaled_error(a0, a) > 100 * cc.BAR32
        if graph == "rmat":
            # values scattered to the neighbouring ids are another result as well (on
            # bins_graph() the pool vertices are too much alike for that to show)
            hm, am, _, _ = oc.hits(L.n, L.cs, L.cd, 0.0, iterations, initial_hubs=np.roll(full, 1))
            assert cc.scaled_error(hm, h) > 100 * cc.BAR32


def test_one_dropped_edge_moves_the_result():
    """Sensitivity of the bar: without the last edge of the 4097-edge row (what a
    block-per-row loop that ends one short computes) Katz and HITS move by at least 10x
    the fp32 bar.  Measured: Katz 1.22e-4; HITS authorities 5.56e-5 (normalised) and
    8.13e-5 -- the row's sum loses the hub value of a pool vertex with one out-edge,
    which is small; the first estimate of 2e-4 took an average one -- so the fp32 bar is
    5e-6, not 1e-5.  HITS hubs move by 0.32, but only because the oracle drops the edge
    from the out-adjacency too and the vertex is left without out-edges: not counted."""
    L = cc.layout("bins", False)
    row = cc.TARGET0 + cc.DEGREES.index(4097)
    last = np.flatnonzero(L.cd == row)[np.argmax(L.cs[L.cd == row])]
    assert L.indeg[row] == 4097 and L.cs[last] == 4096 and L.outdeg[4096] == 1
    keep = np.ones(L.cs.size, bool)
    keep[last] = False
    s, d = L.cs[keep], L.cd[keep]

    r = cc.katz_ref("bins", False, False)
    raw, _ = cc.katz_oracle(L, None, None, r["epsilon"], 100, s, d)
    moved = cc.scaled_error(raw / np.sqrt((raw ** 2).sum()), r["values"])
    print(f"katz, one edge dropped: {moved:.3e}")
    assert moved >= 10 * cc.BAR32

    for normalized in (True, False):
        h, a, _, _ = cc.hits_ref("bins", False, 0.0, cc.HITS_FIXED_ITERATIONS, normalized)
        h1, a1, _, _ = oc.hits(L.n, s, d, 0.0, cc.HITS_FIXED_ITERATIONS, normalize=normalized)
        eh, ea = cc.scaled_error(h1, h), cc.scaled_error(a1, a)
        print(f"hits normalized={normalized}, one edge dropped: hubs {eh:.3e} authorities {ea:.3e}")
        assert ea >= 10 * cc.BAR32
