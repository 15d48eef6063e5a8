"""A plain numpy / Python twin of csrc/betweenness.hip: Brandes' algorithm on the unweighted graph from an
explicit list of sources, with the endpoints and edge flags and the scaling rules of the reference's
betweenness_centrality.cu:368-452.

The graph is the list of stored edges over the vertices 0 .. n - 1 (a symmetric graph lists both
directions; a repeated pair is a parallel edge and counts as a distinct path; a self-loop contributes
nothing).  Every sum runs in row order: the rows are the out-edges sorted by (source, destination), the
order libcugraph_c stores them in, which is also the order of the edge scores.

    betweenness(n, src, dst, sources, symmetric, normalized=True, endpoints=False) -> float64[n]
    edge_betweenness(n, src, dst, sources, symmetric, normalized=True)
        -> (row source, row destination, float64 score) per stored edge, in row order

``sources`` lists vertex ids, each entry a source (a repeated id counts again); None means every vertex.
"""
import numpy as np


def rows(n, src, dst):
    """Out-edge rows: (offsets[n + 1], indices, row source per entry), entries sorted by (src, dst)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.lexsort((dst, src))
    s, d = src[order], dst[order]
    off = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(s, minlength=n), out=off[1:])
    return off, d, s


def _entries(off, verts):
    """Positions of the rows of ``verts``, row after row in order, and the row vertex of each."""
    lens = off[verts + 1] - off[verts]
    total = int(lens.sum())
    if total == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    ends = np.cumsum(lens)
    pos = np.arange(total) - np.repeat(ends - lens, lens) + np.repeat(off[verts], lens)
    return pos, np.repeat(verts, lens)


def _one_source(n, off, idx, s, bc, eb, endpoints):
    dist = np.full(n, -1, np.int64)
    sigma = np.zeros(n, np.float64)
    delta = np.zeros(n, np.float64)
    dist[s], sigma[s] = 0, 1.0
    levels = [np.array([s], np.int64)]
    while True:  # forward: discover level d, then count its paths
        d = len(levels)
        pos, u = _entries(off, levels[-1])
        w = idx[pos]
        new = np.unique(w[dist[w] == -1])
        if len(new) == 0:
            break
        dist[new] = d
        on = dist[w] == d
        np.add.at(sigma, w[on], sigma[u[on]])
        levels.append(new)
    for d in range(len(levels) - 1, -1, -1):  # backward: accumulation_kernel's arithmetic, in row order
        pos, u = _entries(off, levels[d])
        w = idx[pos]
        on = dist[w] == d + 1
        term = sigma[u[on]] * ((1.0 + delta[w[on]]) / sigma[w[on]])
        np.add.at(delta, u[on], term)  # unbuffered: one add per entry, in the order given
        if eb is not None:
            eb[pos[on]] += term
    if bc is not None:
        reached = dist > 0
        if endpoints:
            bc[reached] += 1.0
            bc[s] += float(reached.sum())
        bc[reached] += delta[reached]


def _vertex_scale(x, n, k, symmetric, normalized, endpoints):
    if normalized:
        if n > 2:
            x *= 1.0 / (n * (n - 1.0) if endpoints else (n - 1.0) * (n - 2.0))
    elif symmetric:
        x *= 1.0 / 2.0
    if k > 0 and n > 2 and (normalized or symmetric):
        x *= float(n) / float(k)
    return x


def _edge_scale(x, n, symmetric, normalized):
    if normalized:
        if n > 1:
            x *= 1.0 / (n * (n - 1.0))
    elif symmetric:
        x *= 1.0 / 2.0
    return x


def betweenness(n, src, dst, sources, symmetric, normalized=True, endpoints=False):
    off, idx, _ = rows(n, src, dst)
    sources = range(n) if sources is None else [int(s) for s in sources]
    bc = np.zeros(n, np.float64)
    for s in sources:
        _one_source(n, off, idx, s, bc, None, endpoints)
    return _vertex_scale(bc, n, len(sources), symmetric, normalized, endpoints)


def edge_betweenness(n, src, dst, sources, symmetric, normalized=True):
    off, idx, row = rows(n, src, dst)
    sources = range(n) if sources is None else [int(s) for s in sources]
    eb = np.zeros(len(idx), np.float64)
    for s in sources:
        _one_source(n, off, idx, s, None, eb, False)
    return row, idx, _edge_scale(eb, n, symmetric, normalized)
