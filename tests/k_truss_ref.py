"""A CPU twin of csrc/k_truss.hip for the tests: the underlying simple graph, every edge's triangle
support, and a round-synchronous peel.  The k-truss is the maximal subgraph in which every edge lies
in at least k - 2 triangles of the subgraph (networkx.k_truss's convention).

Round r removes, all at once, every edge whose support fell below k - 2 in round r - 1 (round 1: the
edges whose initial support is below it); a triangle that loses several edges in one round is taken
from each surviving edge's support once.  ``rounds`` counts the rounds that removed something, which
is what ``ResourceHandle.last_iterations()`` reports after the GPU call."""
import numpy as np


def simple_edges(src, dst):
    """The undirected edges (u < v) of the underlying simple graph, sorted, as an (m, 2) int64 array:
    self-loops dropped, both directions and repeats folded."""
    s, d = np.asarray(src, np.int64).ravel(), np.asarray(dst, np.int64).ravel()
    keep = s != d
    lo, hi = np.minimum(s[keep], d[keep]), np.maximum(s[keep], d[keep])
    if len(lo) == 0:
        return np.zeros((0, 2), np.int64)
    return np.unique(np.stack([lo, hi], axis=1), axis=0)


def supports(edges):
    """{(u, v): |N(u) & N(v)|} and the adjacency sets."""
    adj = {}
    for u, v in edges.tolist():
        adj.setdefault(u, set()).add(v)
        adj.setdefault(v, set()).add(u)
    return {(u, v): len(adj[u] & adj[v]) for u, v in edges.tolist()}, adj


def k_truss(src, dst, k):
    """(edges, rounds): the surviving undirected edges (u < v), sorted, (m', 2) int64; and the number of
    peel rounds that removed at least one edge."""
    edges = simple_edges(src, dst)
    t = int(k) - 2
    if t <= 0 or len(edges) == 0:
        return edges, 0
    sup, adj = supports(edges)
    key = lambda a, b: (a, b) if a < b else (b, a)
    frontier = [e for e in sup if sup[e] < t]
    queued = set(frontier)
    rounds = 0
    while frontier:
        rounds += 1
        now = set(frontier)
        nxt = []
        for e in frontier:
            u, v = e
            for w in adj[u] & adj[v]:
                e1, e2 = key(u, w), key(v, w)
                # of the triangle's edges removed in this round, the smallest takes it off the others
                if (e1 in now and e1 < e) or (e2 in now and e2 < e):
                    continue
                for x in (e1, e2):
                    if x not in now:
                        sup[x] -= 1
                        if sup[x] < t and x not in queued:
                            queued.add(x)
                            nxt.append(x)
        for u, v in frontier:
            adj[u].discard(v)
            adj[v].discard(u)
        frontier = nxt
    left = sorted(e for e in sup if e not in queued)
    return np.array(left, np.int64).reshape(-1, 2), rounds


def directed_pairs(edges):
    """Both directions of every edge as a sorted list of (src, dst)."""
    e = [tuple(x) for x in np.asarray(edges).reshape(-1, 2).tolist()]
    return sorted(e + [(b, a) for a, b in e])
