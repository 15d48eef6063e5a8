"""Inputs of the centrality tests (tests/test_centrality_inputs.py checks them on the
CPU, tests/test_gpu_centrality_cases.py runs them): two directed graphs, external
ids that are not 0..V-1, weights exact in fp32, and the stop threshold taken from the
oracle's own differences.  numpy only.

bins_graph(): 4118 vertices whose in-degrees are the bounds of every bin of
csrc/schedule.hpp -- pool P = 0..4096, a target T_k per degree d_k with edges
P[0:d_k] -> T_k and a back edge T_k -> P[k], every pool vertex an out-neighbour of
the target of degree 4096 (an out-row for a whole block as well), five vertices Z_i
-> P[100 + i] that nothing points at, and a chain P[i] -> P[i + 1], i < 50.
"""
import functools

import numpy as np

from oracle import centrality as oc
from oracle import graph as og
from oracle import rmat

DEGREES = (1, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 127, 128, 4095, 4096, 4097)
NPOOL = 4097
TARGET0 = NPOOL                      # T_k = TARGET0 + k
Z0 = TARGET0 + len(DEGREES)          # Z_i = Z0 + i
ZEROS = tuple(range(Z0, Z0 + 5))     # the in-degree-0 vertices
BINS_NV = Z0 + 5

# fp32 storage, fp64 sums: a numpy run that rounds to fp32 where the library stores gives
# 4e-8 .. 3e-7 on these graphs; one edge dropped from the 4097-edge row moves HITS's
# authorities by 5.6e-5 (tests/test_centrality_inputs.py), ten times this bar
BAR32 = 5e-6
BAR64 = 1e-10  # 4097 * 2^-53 per iteration, at most 50 iterations


def _dedup(s, d):
    s, d, _ = og.symmetrize_dedup(s, d, None, symmetrize=False)
    return s, d


@functools.lru_cache(maxsize=None)
def bins_graph():
    """(src, dst) int64, deduplicated."""
    s, d = [], []
    for k, deg in enumerate(DEGREES):
        s.append(np.arange(deg))
        d.append(np.full(deg, TARGET0 + k))
        s.append([TARGET0 + k])
        d.append([k])
    t = TARGET0 + DEGREES.index(4096)
    s.append(np.full(NPOOL, t))
    d.append(np.arange(NPOOL))
    s.append(np.asarray(ZEROS))
    d.append(100 + np.arange(len(ZEROS)))
    s.append(np.arange(50))
    d.append(1 + np.arange(50))
    s, d = _dedup(np.concatenate([np.asarray(x, np.int64) for x in s]),
                  np.concatenate([np.asarray(x, np.int64) for x in d]))
    s.setflags(write=False)
    d.setflags(write=False)
    return s, d


@functools.lru_cache(maxsize=None)
def rmat_directed():
    """(src, dst) int64: a scale-10 R-MAT, deduplicated, not symmetrised."""
    s, d = _dedup(*rmat.rmat(10, 8 << 10, seed=21))
    s.setflags(write=False)
    d.setflags(write=False)
    return s, d


def spread(v):
    """Vertex i -> external id 3 i + 5: not contiguous, and no renumbering is the identity."""
    return 3 * np.asarray(v, np.int64) + 5


def edge_weights(s, d):
    """w(u, v) = ((7 u + 13 v) % 8 + 1) / 8 -- in (0, 1], exact in fp32, a function of
    the edge's endpoints alone (no order of the edge list enters)."""
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    return ((7 * s + 13 * d) % 8 + 1) / 8.0


def compact(s, d, renumber):
    """(num_vertices, src, dst, ids) as the library numbers the vertex set, up to a
    permutation: renumber -- the sorted endpoints, 0..n-1 by rank; else 0..max as they
    are.  ids[i] is the input id of compact vertex i."""
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    if not renumber:
        n = int(max(s.max(), d.max())) + 1
        return n, s, d, np.arange(n, dtype=np.int64)
    ids = np.unique(np.concatenate([s, d]))
    return ids.size, np.searchsorted(ids, s), np.searchsorted(ids, d), ids


def scaled_error(got, ref):
    """max |got - ref| / max |ref|."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))


def l1_floor(nv, xmax):
    """Rounding floor of an L1 difference of nv fp32 values up to xmax, times 10."""
    return 10.0 * nv * 2.0 ** -24 * xmax


def choose_stop(trace, floor=0.0):
    """(k, threshold): the first iteration k >= 4 (counted from 1, trace[k - 1] its
    difference) with trace[k - 2] / trace[k - 1] >= 4, threshold = sqrt(trace[k - 2] *
    trace[k - 1]).  Where that threshold is below floor (thresholds only fall with k),
    the nearest earlier k >= 2 with the same ratio and a threshold >= floor instead.
    Every difference before k is at least twice the threshold and that of k at most
    half of it, so a run whose differences are within a factor of two of these stops at
    k and nowhere else.  None if there is no such k."""
    t = np.asarray(trace, np.float64)

    def at(k):
        if not (t[k - 1] > 0 and t[k - 2] / t[k - 1] >= 4):
            return None
        thr = float(np.sqrt(t[k - 2] * t[k - 1]))
        return thr if t[:k - 1].min() >= 2 * thr else None

    first = next((k for k in range(4, t.size + 1) if at(k) is not None), None)
    if first is None:
        return None
    for k in range(first, 1, -1):
        thr = at(k)
        if thr is not None and thr >= floor:
            return k, thr
    return None


def random_values(n, lo, seed, dtype=np.float32):
    """n values in [lo, lo + 1), rounded to dtype (the oracle gets the same numbers)."""
    return (lo + np.random.default_rng(seed).random(n)).astype(dtype)


# ---- the cases: what the library is given and what the oracle makes of it.  Every
# reference is computed once and shared; nothing below writes to one.

GRAPHS = {"bins": bins_graph, "rmat": rmat_directed}


class Layout:
    """One graph as the library gets it.  renumber: the spread external ids, renumbered
    by the library; else ids 0..max as they are.  src / dst / weights go to the library;
    n, cs, cd (compact ids) and w (float64) to the oracle; ids[i] is the external id of
    compact vertex i."""

    def __init__(self, graph, renumber):
        s, d = GRAPHS[graph]()
        self.graph, self.renumber = graph, renumber
        self.src, self.dst = (spread(s), spread(d)) if renumber else (s, d)
        self.n, self.cs, self.cd, self.ids = compact(self.src, self.dst, renumber)
        self.w = edge_weights(s, d)
        self.indeg = np.bincount(self.cd, minlength=self.n)
        self.outdeg = np.bincount(self.cs, minlength=self.n)
        self.alpha = 1.0 / (int(self.indeg.max()) + 1.0)

    def weights(self, weighted):
        return self.w if weighted else None


@functools.lru_cache(maxsize=None)
def layout(graph, renumber):
    return Layout(graph, renumber)


def betas_array(L, kind, dtype):
    """Katz betas by external id: "full" covers every id, "short" ends at half the
    largest one (the ids past its end count as 0); values in [0.5, 1.5)."""
    if kind is None:
        return None
    size = int(L.ids.max()) + 1
    return random_values(size if kind == "full" else size // 2, 0.5, 11, dtype)


def betas_by_vertex(L, arr):
    out = np.zeros(L.n)
    inside = L.ids < arr.size
    out[inside] = arr[L.ids[inside]]
    return out


def katz_oracle(L, w, b, eps, max_iterations, src=None, dst=None):
    return oc.katz(L.n, L.cs if src is None else src, L.cd if dst is None else dst, w, L.alpha, 1.0, eps,
                   max_iterations, betas=b, normalize=False, return_trace=True)


@functools.lru_cache(maxsize=None)
def katz_ref(graph, renumber, weighted, betas=None, dtype=np.float32):
    """dict: epsilon (from the trace), iterations, values, raw (not normalised), betas
    (the array for the library, or None)."""
    L = layout(graph, renumber)
    arr = betas_array(L, betas, dtype)
    b = None if arr is None else betas_by_vertex(L, arr)
    w = L.weights(weighted)
    raw, trace = katz_oracle(L, w, b, 1e-11, 200)
    stop = choose_stop(trace, l1_floor(L.n, np.abs(raw).max()))
    out = {"betas": arr, "trace": trace, "stop": stop}
    if stop is not None:
        k, eps = stop
        out["raw"], t = katz_oracle(L, w, b, eps, 100)
        assert len(t) == k
        out.update(epsilon=eps, iterations=k, values=out["raw"] / np.sqrt((out["raw"] ** 2).sum()))
    return out


@functools.lru_cache(maxsize=None)
def eigenvector_ref(graph, renumber, weighted):
    """dict: epsilon (threshold / nv), iterations, values."""
    L = layout(graph, renumber)
    w = L.weights(weighted)
    x, trace = oc.eigenvector_centrality(L.n, L.cs, L.cd, w, 1e-11 / L.n, 1000, return_trace=True)
    stop = choose_stop(trace, l1_floor(L.n, np.abs(x).max()))
    out = {"trace": trace, "stop": stop}
    if stop is not None:
        k, thr = stop
        out["values"], t = oc.eigenvector_centrality(L.n, L.cs, L.cd, w, thr / L.n, 100, return_trace=True)
        assert len(t) == k
        out.update(epsilon=thr / L.n, iterations=k)
    return out


def guess_arrays(L, count, dtype=np.float32):
    """(external ids in no order, values in [0.1, 1.1), the values by compact vertex, 0
    elsewhere)."""
    pick = np.random.default_rng(5).choice(L.n, count, replace=False)
    vals = random_values(count, 0.1, 7, dtype)
    full = np.zeros(L.n)
    full[pick] = vals
    return L.ids[pick], vals, full


@functools.lru_cache(maxsize=None)
def hits_ref(graph, renumber, epsilon, max_iterations, normalized=True, guess=0, dtype=np.float32):
    """The oracle's (hubs, authorities, difference, iterations); guess: how many
    vertices of guess_arrays() start with a value."""
    L = layout(graph, renumber)
    init = guess_arrays(L, guess, dtype)[2] if guess else None
    return oc.hits(L.n, L.cs, L.cd, epsilon, max_iterations, initial_hubs=init, normalize=normalized)


def hits_trace(L):
    """The oracle's differences down to 1e-9, far above where fp64 rounding shapes them."""
    return oc.hits(L.n, L.cs, L.cd, 1e-9, 200, return_trace=True)[4]


@functools.lru_cache(maxsize=None)
def hits_stop(graph, renumber):
    """(k, threshold) of choose_stop on the oracle's HITS differences, or None."""
    L = layout(graph, renumber)
    trace = hits_trace(L)
    return choose_stop(trace, l1_floor(L.n, 1.0))  # hubs are divided by their maximum


# (graph, renumber, weighted, betas)
KATZ_CASES = [("bins", r, w, None) for r in (True, False) for w in (False, True)]
KATZ_BETAS_CASES = [("bins", r, True, kind) for r in (True, False) for kind in ("full", "short")]
# (graph, renumber, weighted): bins_graph() is nearly bipartite, the oracle's power
# iteration does not converge on it in 5000 iterations
EIGENVECTOR_CASES = [("rmat", r, w) for r in (True, False) for w in (False, True)]
HITS_GRAPHS = ("bins", "rmat")
# choose_stop() finds no k on bins_graph(): its HITS differences fall by about 3x an
# iteration from the fourth on (tests/test_centrality_inputs.py holds that down)
HITS_STOP_GRAPHS = ("rmat",)
HITS_FIXED_ITERATIONS = 20
# (graph, vertices with a guess): above and below the 1024 ids at which the lookup
# changes kernels; always on the renumbered graph
GUESS_CASES = [("bins", BINS_NV // 2), ("bins", 100), ("rmat", 409), ("rmat", 100)]
