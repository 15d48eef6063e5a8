"""Katz, eigenvector centrality and HITS (csrc/centrality.hip) where k_spmv and the
code around it branch, against oracle/centrality.py in fp64 on the same inputs
(tests/centrality_cases.py builds them, tests/test_centrality_inputs.py checks them):

 * rows of 0, 1, 3, 4, ... 128, 4095, 4096 and 4097 in-edges -- every bin of the
   schedule, the block-per-row branch, the zero-degree tail that must write y = 0;
 * directed graphs, both storage orders: the adjacency from transpose_impl and its
   `order`, hubs and authorities each against their own vector;
 * external ids 3 i + 5 on the renumbered graph; Katz betas by external id, full and
   ending early; a HITS guess looked up by either kernel, after 1 and 2 iterations;
 * the iteration counts and HITS's reported difference, the stop threshold taken from
   the oracle's trace with a factor of two to either side;
 * int64 ids with fp32 and fp64 weights; the error paths.

Error measure: max |got - ref| / max |ref| per vector, at most cc.BAR32 (fp32
storage) or cc.BAR64; every test prints what it saw.  On an MI355X, largest per
group: Katz 1.1e-7 (with betas 8.8e-8), HITS after 20 iterations 8.4e-8 hubs and
5.1e-8 authorities, HITS stopped by epsilon 6.0e-8 with the reported difference
8.5e-7 off relatively, HITS with a guess 9.2e-8, eigenvector 2.5e-8; fp64 3.5e-15.

bins_graph() has no HITS run stopped by epsilon: its differences fall by 3x an
iteration, the rule of cc.choose_stop() wants 4x, so the count there is checked by
the run that epsilon 0 takes to max_iterations.

What these would catch, from the CPU-side figures: a block-per-row loop that ends one
edge short moves Katz on bins_graph() by 1.2e-4 and HITS's authorities by 5.6e-5
(24 and 11 bars); `in` and `out` swapped in hits_impl is HITS of the reversed graph,
hubs for authorities, and the two are 0.14 apart on rmat_directed() and 1.0 on
bins_graph(); a guess that is ignored leaves the
result 4e-3 .. 0.3 away after 1 and 2 iterations.
"""
import numpy as np
import pytest

import centrality_cases as cc
from gpu_util import host, make_graph, plc

pytestmark = pytest.mark.gpu

MAX_ITERATIONS = 100


def bar_of(wdtype):
    return cc.BAR32 if wdtype == np.float32 else cc.BAR64


def graph_of(L, weighted, transposed, vdtype=np.int32, wdtype=np.float32):
    """The library gets copies: the layouts are shared and read-only."""
    return make_graph(np.array(L.src, vdtype), np.array(L.dst, vdtype), L.weights(weighted), transposed=transposed,
                      renumber=L.renumber, vdtype=vdtype, wdtype=wdtype)


def by_vertex(L, v, x, vdtype=np.int32, wdtype=np.float32):
    """The result by compact vertex; the vertices are the graph's, each once."""
    v, x = host(v), host(x)
    assert v.dtype == vdtype and x.dtype == wdtype
    assert np.array_equal(np.sort(v), L.ids)
    out = np.empty(L.n)
    out[np.searchsorted(L.ids, v)] = x
    return out


def check(name, got, ref, bar):
    err = cc.scaled_error(got, ref)
    print(f"{name}: scaled error {err:.3e} (bar {bar:.0e})")
    assert err <= bar, name
    return err


# ---- Katz

def run_katz(case, transposed, vdtype=np.int32, wdtype=np.float32):
    graph, renumber, weighted, betas = case
    L = cc.layout(graph, renumber)
    r = cc.katz_ref(*case, dtype=wdtype)
    h, G = graph_of(L, weighted, transposed, vdtype, wdtype)
    v, x = plc().katz_centrality(h, G, r["betas"], L.alpha, 1.0, r["epsilon"], MAX_ITERATIONS, False)
    got = by_vertex(L, v, x, vdtype, wdtype)
    bar = bar_of(wdtype)
    check(f"katz {case} transposed={transposed} {np.dtype(wdtype)}", got, r["values"], bar)
    assert h.last_iterations() == r["iterations"]
    return L, r, got


@pytest.mark.parametrize("transposed", [True, False])
@pytest.mark.parametrize("case", cc.KATZ_CASES, ids=str)
def test_katz_bins(case, transposed):
    L, r, got = run_katz(case, transposed)
    # nothing points at these: beta, divided by the norm
    zeros = np.searchsorted(L.ids, cc.spread(cc.ZEROS) if L.renumber else cc.ZEROS)
    assert np.all(L.indeg[zeros] == 0)
    l2 = np.sqrt((r["raw"] ** 2).sum())
    assert np.max(np.abs(got[zeros] - 1.0 / l2)) <= cc.BAR32 * r["values"].max()


@pytest.mark.parametrize("transposed", [True, False])
@pytest.mark.parametrize("case", cc.KATZ_BETAS_CASES, ids=str)
def test_katz_betas(case, transposed):
    L, r, got = run_katz(case, transposed)
    b = cc.betas_by_vertex(L, r["betas"])
    assert (b == 0).sum() > 0 if case[3] == "short" else b.min() >= 0.5
    zeros = np.flatnonzero(L.indeg == 0)
    l2 = np.sqrt((r["raw"] ** 2).sum())
    assert np.max(np.abs(got[zeros] - b[zeros] / l2)) <= cc.BAR32 * r["values"].max()


# ---- HITS

def run_hits(L, transposed, epsilon, max_iterations, normalized, guess=0, vdtype=np.int32, wdtype=np.float32):
    """HITS ignores edge weights, but computes in the graph's weight type, which an
    unweighted graph leaves at fp32: the fp64 runs carry weights."""
    h, G = graph_of(L, wdtype != np.float32, transposed, vdtype, wdtype)
    gv = gx = None
    if guess:
        ids, vals, _ = cc.guess_arrays(L, guess, wdtype)
        gv, gx = ids.astype(vdtype), vals
    v, hb, au = plc().hits(h, G, epsilon, max_iterations, gv, gx, normalized, False)
    diff, iterations = h._last_hits
    return by_vertex(L, v, hb, vdtype, wdtype), by_vertex(L, v, au, vdtype, wdtype), diff, iterations


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("transposed", [True, False])
@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("graph", cc.HITS_GRAPHS)
def test_hits_fixed_iterations(graph, renumber, transposed, normalized):
    """epsilon 0: no difference is below it, the count is max_iterations."""
    L = cc.layout(graph, renumber)
    n = cc.HITS_FIXED_ITERATIONS
    hubs, auth, diff, iterations = run_hits(L, transposed, 0.0, n, normalized)
    rh, ra, _, rit = cc.hits_ref(graph, renumber, 0.0, n, normalized)
    name = f"hits {graph} renumber={renumber} transposed={transposed} normalized={normalized}"
    check(name + " hubs", hubs, rh, cc.BAR32)
    check(name + " authorities", auth, ra, cc.BAR32)
    assert iterations == rit == n


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("transposed", [True, False])
@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("graph", cc.HITS_STOP_GRAPHS)
def test_hits_stops_where_the_oracle_does(graph, renumber, transposed, normalized):
    L = cc.layout(graph, renumber)
    k, thr = cc.hits_stop(graph, renumber)
    hubs, auth, diff, iterations = run_hits(L, transposed, thr, MAX_ITERATIONS, normalized)
    rh, ra, rdiff, rit = cc.hits_ref(graph, renumber, thr, MAX_ITERATIONS, normalized)
    name = f"hits {graph} renumber={renumber} transposed={transposed} normalized={normalized} epsilon={thr:.3g}"
    check(name + " hubs", hubs, rh, cc.BAR32)
    check(name + " authorities", auth, ra, cc.BAR32)
    print(f"{name}: iterations {iterations} (oracle {rit}), difference {diff:.9e} (oracle {rdiff:.9e}, "
          f"relative {abs(diff - rdiff) / rdiff:.3e})")
    assert iterations == rit == k - 1
    assert abs(diff - rdiff) <= cc.BAR32 * rdiff


@pytest.mark.parametrize("iterations", [1, 2])
@pytest.mark.parametrize("graph,count", cc.GUESS_CASES)
def test_hits_guess(graph, count, iterations):
    """After 1 and 2 iterations the result with and without the guess are 100 bars
    apart (tests/test_centrality_inputs.py): a guess ignored, put at other vertices or
    not divided by its sum fails here."""
    L = cc.layout(graph, True)
    hubs, auth, _, it = run_hits(L, False, 0.0, iterations, True, guess=count)
    rh, ra, _, _ = cc.hits_ref(graph, True, 0.0, iterations, True, count)
    name = f"hits {graph} guess of {count}, {iterations} iterations"
    check(name + " hubs", hubs, rh, cc.BAR32)
    check(name + " authorities", auth, ra, cc.BAR32)
    assert it == iterations


# ---- eigenvector

def run_eigenvector(case, transposed, vdtype=np.int32, wdtype=np.float32):
    graph, renumber, weighted = case
    L = cc.layout(graph, renumber)
    r = cc.eigenvector_ref(*case)
    h, G = graph_of(L, weighted, transposed, vdtype, wdtype)
    v, x = plc().eigenvector_centrality(h, G, r["epsilon"], MAX_ITERATIONS, False)
    check(f"eigenvector {case} transposed={transposed} {np.dtype(wdtype)}", by_vertex(L, v, x, vdtype, wdtype),
          r["values"], bar_of(wdtype))
    assert h.last_iterations() == r["iterations"]


@pytest.mark.parametrize("transposed", [True, False])
@pytest.mark.parametrize("case", cc.EIGENVECTOR_CASES, ids=str)
def test_eigenvector_rmat(case, transposed):
    run_eigenvector(case, transposed)


# ---- types

@pytest.mark.parametrize("wdtype", [np.float64, np.float32])
def test_int64_katz_betas(wdtype):
    run_katz(("bins", True, True, "full"), True, np.int64, wdtype)
    run_katz(("bins", False, True, "short"), False, np.int64, wdtype)


@pytest.mark.parametrize("wdtype", [np.float64, np.float32])
def test_int64_hits(wdtype):
    bar = bar_of(wdtype)
    for graph, transposed, guess, n in (("bins", False, 0, cc.HITS_FIXED_ITERATIONS), ("bins", True, cc.BINS_NV // 2, 2),
                                        ("rmat", True, 100, 2)):
        L = cc.layout(graph, True)
        hubs, auth, _, it = run_hits(L, transposed, 0.0, n, True, guess, np.int64, wdtype)
        rh, ra, _, _ = cc.hits_ref(graph, True, 0.0, n, True, guess, wdtype)
        name = f"hits int64 {np.dtype(wdtype)} {graph} transposed={transposed} guess={guess}"
        check(name + " hubs", hubs, rh, bar)
        check(name + " authorities", auth, ra, bar)
        assert it == n
    if wdtype == np.float64:  # fp64 storage: the reported difference at the fp64 bar as well
        k, thr = cc.hits_stop("rmat", True)
        L = cc.layout("rmat", True)
        _, _, diff, it = run_hits(L, True, thr, MAX_ITERATIONS, True, 0, np.int64, wdtype)
        _, _, rdiff, rit = cc.hits_ref("rmat", True, thr, MAX_ITERATIONS, True)
        print(f"hits int64 float64 difference relative {abs(diff - rdiff) / rdiff:.3e}")
        assert it == rit and abs(diff - rdiff) <= bar * rdiff


@pytest.mark.parametrize("wdtype", [np.float64, np.float32])
def test_int64_eigenvector(wdtype):
    run_eigenvector(("rmat", True, True), True, np.int64, wdtype)
    run_eigenvector(("rmat", True, True), False, np.int64, wdtype)
    if wdtype == np.float32:  # the weight type of a graph without weights
        run_eigenvector(("rmat", True, False), False, np.int64, wdtype)


# ---- errors

def small(renumber=True, w=None):
    L = cc.layout("rmat", renumber)
    return (L,) + make_graph(L.src, L.dst, w, transposed=True, renumber=renumber)


def test_eigenvector_not_converged():
    L, h, G = small()
    with pytest.raises(RuntimeError, match="Eigenvector Centrality failed to converge"):
        plc().eigenvector_centrality(h, G, 1e-9, 1, False)


def test_hits_one_iteration_is_no_error():
    L, h, G = small()
    plc().hits(h, G, 1e-9, 1, None, None, True, False)
    diff, iterations = h._last_hits
    assert iterations == 1 and diff > 1e-9
    assert h.last_iterations() == 1


def test_negative_epsilon():
    L, h, G = small()
    for call in (lambda: plc().katz_centrality(h, G, None, L.alpha, 1.0, -1e-6, 10, False),
                 lambda: plc().eigenvector_centrality(h, G, -1e-6, 10, False),
                 lambda: plc().hits(h, G, -1e-6, 10, None, None, True, False)):
        with pytest.raises(ValueError, match="epsilon should be non-negative"):
            call()


def test_katz_alpha_out_of_range():
    L, h, G = small()
    with pytest.raises(ValueError, match=r"alpha should be in \[0.0, 1.0\]"):
        plc().katz_centrality(h, G, None, 1.5, 1.0, 1e-6, 10, False)


def test_eigenvector_zero_weight_expensive_check():
    L = cc.layout("rmat", True)
    w = L.w.copy()
    w[w.size // 2] = 0.0
    _, h, G = small(w=w)
    with pytest.raises(ValueError, match="postive edge weights"):
        plc().eigenvector_centrality(h, G, 1e-6, 100, True)
    _, h, G = small(w=L.w)
    plc().eigenvector_centrality(h, G, 1e-6, 100, True)


def test_hits_negative_guess_expensive_check():
    L, h, G = small()
    ids, vals, _ = cc.guess_arrays(L, 100)
    bad = vals.copy()
    bad[17] = -0.25
    with pytest.raises(ValueError, match="initial guess values should be non-negative"):
        plc().hits(h, G, 1e-6, 10, ids.astype(np.int32), bad, True, True)
    plc().hits(h, G, 1e-6, 10, ids.astype(np.int32), vals, True, True)


@pytest.mark.parametrize("renumber", [True, False])
def test_hits_guess_id_not_in_graph(renumber):
    L, h, G = small(renumber=renumber)
    ids, vals, _ = cc.guess_arrays(L, 100)
    # renumbered: an id between two spread ids; else: one past the last vertex
    missing = int(L.ids[3]) + 1 if renumber else L.n
    assert missing not in set(L.ids.tolist())
    bad = ids.copy()
    bad[42] = missing
    with pytest.raises(ValueError, match="vertex id not in the graph"):
        plc().hits(h, G, 1e-6, 10, bad.astype(np.int32), vals, True, False)


def test_katz_betas_of_another_type():
    L, h, G = small()
    betas = cc.betas_array(L, "full", np.float64)
    with pytest.raises(ValueError, match="betas type must match the weight type"):
        plc().katz_centrality(h, G, betas, L.alpha, 1.0, 1e-6, 100, False)
