"""What an SSSP result must satisfy, checked without trusting how the oracle picks
predecessors: every vertex, nothing sampled.

The distances are the oracle's fixed point (oracle/sssp.py, the same dtype, bit for
bit).  The predecessors are checked from the distances alone:
 * -1 exactly at the source and at unreached vertices;
 * every other pred[v] -> v is an edge with fl(dist[pred[v]] + w) == dist[v];
 * they form a tree: pointer jumping takes every reached vertex through the source
   to -1 (two vertices at one distance joined by a zero weight, or by a weight that
   rounding absorbs, are tight for each other -- a rule that only asks for tightness
   lets them name each other);
 * they are the deterministic rule, restated here: the smallest id among the tight
   in-neighbours that are strictly closer (rank 0); failing that, rank k + 1 and the
   smallest id among the tight equal-distance in-neighbours of rank k, the smallest
   rank among them (the source has rank 0).  "Smallest id" is by tie_key.
"""
import numpy as np

from oracle import sssp as osssp


def pred_is_tree(pred, source, reached):
    """Pointer jumping: ceil(log2 V) + 1 doublings; every reached vertex must end at
    -1 having passed the source.  Returns the vertices that do not."""
    V = pred.size
    p = np.where(pred < 0, V, pred).astype(np.int64)
    p = np.append(p, V)  # slot V stands for -1
    seen = np.zeros(V + 1, bool)
    seen[source] = True
    for _ in range(int(np.ceil(np.log2(max(V, 2)))) + 1):
        seen = seen | seen[p]
        p = p[p]
    ok = (p[:V] == V) & seen[:V]
    return np.flatnonzero(reached & ~ok)


def rule_pred(off, idx, w, source, dist, tie_key=None):
    """The deterministic predecessors for these distances."""
    V = dist.size
    dtype = dist.dtype.type
    big = np.finfo(dtype).max
    key = np.arange(V, dtype=np.int64) if tie_key is None else np.asarray(tie_key, np.int64)
    u = np.repeat(np.arange(V, dtype=np.int64), np.diff(off))
    v = np.asarray(idx, np.int64)
    with np.errstate(over="ignore"):
        tight = (dist[u] < big) & (v != source) & ((dist[u] + w.astype(dtype)).astype(dtype) == dist[v])
    u, v = u[tight], v[tight]
    order = np.lexsort((key[u], v))  # by destination, then by the source's key
    u, v = u[order], v[order]
    pred = np.full(V, -1, np.int64)
    rank = np.full(V, -1, np.int64)
    rank[source] = 0
    closer = dist[u] < dist[v]
    first = np.ones(int(closer.sum()), bool)
    uc, vc = u[closer], v[closer]
    first[1:] = vc[1:] != vc[:-1]
    pred[vc[first]] = uc[first]
    rank[vc[first]] = 0
    ue, ve = u[~closer], v[~closer]
    k = 0
    while True:
        m = (rank[ve] < 0) & (rank[ue] == k)
        if not m.any():
            break
        um, vm = ue[m], ve[m]
        first = np.ones(um.size, bool)
        first[1:] = vm[1:] != vm[:-1]
        pred[vm[first]] = um[first]
        rank[vm[first]] = k + 1
        k += 1
    return pred, rank


def check_sssp(off, idx, w, source, dist, pred, cutoff=np.inf, tie_key=None):
    """off, idx, w: the out-edges as a CSR over ids 0..V-1; dist, pred over the same
    ids (pred holds ids, -1 for none)."""
    off = np.asarray(off, np.int64)
    idx = np.asarray(idx, np.int64)
    dist = np.asarray(dist)
    dtype = dist.dtype.type
    assert dtype in (np.float32, np.float64)
    w = np.asarray(w).astype(dtype)
    pred = np.asarray(pred).astype(np.int64)
    V = off.size - 1
    assert dist.shape == (V,) and pred.shape == (V,)
    big = np.finfo(dtype).max
    with np.errstate(over="ignore"):
        rd, _ = osssp.sssp(V, off, idx, w, source, cutoff=cutoff, dtype=dtype, tie_key=tie_key)
    bad = np.flatnonzero(dist != rd)
    assert bad.size == 0, f"{bad.size} distances differ from the fixed point, first at {bad[:5]}: " \
                          f"{dist[bad[:5]]} vs {rd[bad[:5]]}"
    reached = dist < big
    assert pred[source] == -1, f"pred[source] = {pred[source]}"
    none = pred < 0
    want_none = ~reached
    want_none[source] = True
    bad = np.flatnonzero(none != want_none)
    assert bad.size == 0, f"{bad.size} vertices: pred == -1 must hold exactly at the source and unreached, " \
                          f"first {bad[:5]}"
    assert np.all(pred[~none] < V) and np.all(pred[none] == -1)
    # a tight edge pred[v] -> v exists (any of parallel edges may be the witness)
    u = np.repeat(np.arange(V, dtype=np.int64), np.diff(off))
    with np.errstate(over="ignore"):
        tight = (dist[u] < big) & ((dist[u] + w).astype(dtype) == dist[idx])
    tkeys = np.unique(u[tight] * V + idx[tight])
    vv = np.flatnonzero(~none)
    bad = vv[~np.isin(pred[vv] * V + vv, tkeys)]
    assert bad.size == 0, f"{bad.size} predecessors are not tight in-neighbours, first {bad[:5]} <- {pred[bad[:5]]}"
    lost = pred_is_tree(pred, source, reached)
    assert lost.size == 0, f"predecessors are not a tree: {lost.size} of {int(reached.sum())} reached vertices " \
                           f"never get to the source, first {lost[:5]} <- {pred[lost[:5]]}"
    want, rank = rule_pred(off, idx, w, source, dist, tie_key)
    assert np.all(rank[reached] >= 0), "the rule leaves a reached vertex without a rank"
    bad = np.flatnonzero(pred != want)
    assert bad.size == 0, f"{bad.size} predecessors differ from the rule, first {bad[:5]}: {pred[bad[:5]]} vs " \
                          f"{want[bad[:5]]} (ranks {rank[bad[:5]]})"
    return rank


# ---- inputs the SSSP tests share (edge lists: src, dst, w; symmetric ones hold both directions)

def four_vertex():
    """The smallest graph on which "any tight in-neighbour" gives a cycle: 1 and 2 are
    both at distance 2 from 0 and joined by a zero weight."""
    s = np.array([0, 3, 3, 1]), np.array([3, 1, 2, 2]), np.array([1.0, 1.0, 1.0, 0.0])
    return np.concatenate([s[0], s[1]]), np.concatenate([s[1], s[0]]), np.concatenate([s[2], s[2]])


def grid(n=32, weights="01", seed=3):
    """n x n grid, symmetric; weights "01": 0 or 1 at random, "unit": all 1, "zero": all 0."""
    ids = np.arange(n * n).reshape(n, n)
    a = np.concatenate([ids[:, :-1].ravel(), ids[:-1, :].ravel()])
    b = np.concatenate([ids[:, 1:].ravel(), ids[1:, :].ravel()])
    if weights == "01":
        w = np.random.default_rng(seed).integers(0, 2, a.size).astype(np.float64)
    else:
        w = np.full(a.size, 1.0 if weights == "unit" else 0.0)
    return np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])


def rmat_edges(scale, weights, symmetric=True, seed=42):
    """RMAT(scale, 16 << scale), deduplicated; weights "uniform" ([0, 1)), "unit", or
    (lo, hi): integers lo..hi."""
    from oracle import graph as og
    from oracle import rmat
    s, d = rmat.rmat(scale, 16 << scale, seed=seed)
    x = rmat.rmat_weights(s.size, seed=43).astype(np.float64)
    if weights == "unit":
        x = np.ones(s.size)
    elif weights != "uniform":
        lo, hi = weights
        x = np.floor(x * (hi - lo + 1)) + lo
    return og.symmetrize_dedup(s, d, x, symmetrize=symmetric)
