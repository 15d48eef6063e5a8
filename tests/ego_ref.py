"""Induced subgraphs and ego nets in plain numpy: the twin the GPU tests compare with.

The graph is its list of *stored* edges (src[i], dst[i], w[i]): an undirected graph is given with both
directions, a self-loop or a repeated edge as often as it is stored.  The induced subgraph of a vertex set
is every stored edge with both ends in the set; the ego net of a seed is the subgraph induced by the
vertices within ``radius`` hops of it over the stored edges' direction, the seed included.  Edges come
back in stored order; callers that compare with another order sort.
"""
import numpy as np


def _arrays(src, dst, w):
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    return src, dst, (None if w is None else np.asarray(w))


def induced_subgraph(src, dst, w, vertices):
    """(src, dst, w or None) of the stored edges with both ends in ``vertices``."""
    src, dst, w = _arrays(src, dst, w)
    members = np.unique(np.asarray(vertices, np.int64))
    keep = np.isin(src, members) & np.isin(dst, members)
    return src[keep], dst[keep], (None if w is None else w[keep])


class Rows:
    """Out-rows of an edge list, built once and shared by many ego_vertices calls."""

    def __init__(self, src, dst):
        src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        self.n = int(max(src.max(initial=-1), dst.max(initial=-1))) + 1
        order = np.argsort(src, kind="stable")
        self.idx = dst[order]
        self.off = np.zeros(self.n + 1, np.int64)
        np.cumsum(np.bincount(src, minlength=self.n), out=self.off[1:])

    def neighbours(self, vertices):
        vertices = vertices[vertices < self.n]
        if len(vertices) == 0:
            return np.zeros(0, np.int64)
        return np.concatenate([self.idx[self.off[v]:self.off[v + 1]] for v in vertices.tolist()])


def ego_vertices(rows, seed, radius):
    """Sorted ids within ``radius`` hops of ``seed`` over the out-edges, the seed included."""
    members = np.asarray([seed], np.int64)
    frontier = members
    for _ in range(int(radius)):
        if len(frontier) == 0:
            break
        frontier = np.setdiff1d(np.unique(rows.neighbours(frontier)), members)
        members = np.union1d(members, frontier)
    return members


def ego_graph(src, dst, w, seed, radius, rows=None):
    rows = rows or Rows(src, dst)
    return induced_subgraph(src, dst, w, ego_vertices(rows, seed, radius))


def batched(src, dst, w, sets):
    """The subgraphs of several vertex sets back to back: (src, dst, w or None, offsets)."""
    parts = [induced_subgraph(src, dst, w, s) for s in sets]
    off = np.zeros(len(parts) + 1, np.int64)
    if parts:
        np.cumsum([len(p[0]) for p in parts], out=off[1:])
    cat = lambda k, dt: np.concatenate([p[k] for p in parts]) if parts else np.zeros(0, dt)
    return cat(0, np.int64), cat(1, np.int64), (None if w is None else cat(2, np.asarray(w).dtype)), off


def batched_ego(src, dst, w, seeds, radius):
    rows = Rows(src, dst)
    return batched(src, dst, w, [ego_vertices(rows, s, radius) for s in seeds])


def sorted_edges(s, d, w=None):
    """One subgraph's edges as a sorted list of (src, dst) or (src, dst, weight bits) tuples."""
    cols = [np.asarray(s).tolist(), np.asarray(d).tolist()]
    if w is not None:
        w = np.asarray(w)
        cols.append(w.view(np.uint32 if w.dtype.itemsize == 4 else np.uint64).tolist())
    return sorted(zip(*cols))
