"""Inputs and checker of the BFS tests (tests/test_bfs_cases_host.py pins their facts on
the CPU, tests/test_gpu_bfs_cases.py runs them, tests/test_gpu_bfs.py uses the checker).
numpy and the oracle only.

case_graph(): one symmetric graph of three parts, in raw ids 0..V-1.

 * chain: BLOCKS blocks of BLOCK vertices, about 10 random edges per vertex inside its
   block and 3 random edges from each block to the next (open, not a ring): about 50
   levels from a source in block 0, so every kind of level transition of bfs_impl and
   every depth-limit cut point occurs many times.
 * hubs: one per degree of HUB_DEGREES (the top-down class and chunk edges of
   csrc/bfs.hip, the 256-lane bin of k_bottomup): degree - 1 pendant leaves and one
   edge to a chain vertex.
 * fans: a pool of NDECOY decoys (a ring lattice, each joined to the next 3, no edge to
   the chain) and, for every k of FAN_K and j of FAN_J, a path q - p - t from one chain
   vertex q of block 2, t also joined to the first k decoys and to j pendant leaves.
   Ids descend by degree after renumbering (decoys >= 6, p 2, leaves 1), so the sorted
   row of t is [k decoys, p, j leaves]; when t is discovered its only frontier neighbour
   is p: the parent sits at position exactly k of k + 1 + j entries.

view(name): the graph as the library gets it --
 renumbered  ids 3 v + 7, renumber=True
 identity    the oracle's internal ids of `renumbered`, renumber=False (degree order
             without a number map: the probe path)
 permuted    renumber=False under a random permutation of V + 1 ids, the last raw id
             isolated (the one-pass k_bottomup over adj.order)
 wide64      `renumbered` with int64 ids (1 << 33) + 1_000_003 v
 directed    the chain alone, every edge in one random direction, ids 3 v + 7,
             renumber=True, symmetric=False
 ring        not the case graph: a ring lattice of one degree, renumber=False, whose
             bottom-up probe sends whole 64-vertex chunks to the residual queue
"""
import functools

import numpy as np

from oracle import bfs as obfs
from oracle import graph as og

INT32_MAX = 2**31 - 1
INT64_MAX = np.iinfo(np.int64).max

BLOCKS, BLOCK = 24, 96
NCHAIN = BLOCKS * BLOCK
HUB_DEGREES = (16, 17, 1024, 1025, 2048, 2049, 4100)
NDECOY = 2050
FAN_K = (0, 1, 2, 3, 4, 7, 8, 10, 11, 12, 23, 24, 26, 27, 28, 43, 100, 1030, 2050)
FAN_J = (0, 1, 5)
SEED = 1
# view("ring"): every vertex joined to the RING_HALF next ones -- one degree, so ids are
# in degree order as they are; RING_SCHEDULE (alpha, beta) runs level 0 top-down and
# level 1 bottom-up (tests/test_bfs_cases_host.py)
RING_NV, RING_HALF, RING_SCHEDULE = 1088, 6, (300.0, 64.0)
# lane widths of k_bottomup by degree bin (csrc/schedule.hpp): (width, lowest, highest degree)
BU_BINS = ((1, 1, 3), (2, 4, 7), (4, 8, 15), (8, 16, 31), (16, 32, 63), (32, 64, 127), (64, 128, 4095),
           (256, 4096, 1 << 40))


def check_vs_oracle(s, d, v, dist, pred, sources_ext, depth_limit=None, inf=INT32_MAX):
    """The library's result (v: its vertex ids in internal order) against the oracle run
    over external ids 0..max, ties by the library's internal id."""
    n_ext = int(max(np.max(s, initial=0), np.max(d, initial=0), np.max(sources_ext))) + 1
    G = og.create_graph(s, d, None, renumber=False, vertices=np.arange(n_ext))
    key = np.full(n_ext, np.iinfo(np.int64).max // 2, dtype=np.int64)
    key[v] = np.arange(v.size)  # internal id = position in the result arrays
    # make the key a permutation (ids absent from the GPU graph never win)
    absent = np.setdiff1d(np.arange(n_ext), v)
    key[absent] = v.size + np.arange(absent.size)
    rd, rp = obfs.bfs(n_ext, G.offsets, G.indices, sources_ext, depth_limit, tie_key=key, invalid_distance=inf)
    assert np.array_equal(dist, rd[v])
    if pred is not None and pred.size:
        assert np.array_equal(pred, rp[v])


class CaseGraph:
    """src / dst: the symmetric, de-duplicated edges in raw ids; source: a vertex of
    block 0; q: the fans' shared chain vertex; hubs: degree -> (hub, one of its leaves);
    fans: (k, j, p, t); decoys: the pool; nv: the vertex count; nchain: the chain's
    vertices are the raw ids below it."""


@functools.lru_cache(maxsize=None)
def case_graph(seed=SEED, blocks=BLOCKS):
    rng = np.random.default_rng(seed)
    nchain = blocks * BLOCK
    s, d = [], []
    for b in range(blocks):
        u = np.repeat(np.arange(BLOCK), 10)
        w = (u + rng.integers(1, BLOCK, u.size)) % BLOCK
        s.append(b * BLOCK + u)
        d.append(b * BLOCK + w)
        if b + 1 < blocks:
            s.append(b * BLOCK + rng.integers(0, BLOCK, 3))
            d.append((b + 1) * BLOCK + rng.integers(0, BLOCK, 3))
    nxt = nchain
    G = CaseGraph()
    G.source = int(rng.integers(0, BLOCK))
    G.q = 2 * BLOCK + int(rng.integers(0, BLOCK))
    G.hubs = {}
    for i, deg in enumerate(HUB_DEGREES):
        hub, leaves = nxt, nxt + 1 + np.arange(deg - 1)
        nxt += deg
        anchor = (1 + 3 * i) * BLOCK % nchain + int(rng.integers(0, BLOCK))
        s += [np.full(deg - 1, hub), [hub]]
        d += [leaves, [anchor]]
        G.hubs[deg] = (hub, int(leaves[0]))
    G.decoys = nxt + np.arange(NDECOY)
    nxt += NDECOY
    for step in (1, 2, 3):
        s.append(G.decoys)
        d.append(np.roll(G.decoys, -step))
    G.fans = []
    for k in FAN_K:
        for j in FAN_J:
            p, t, leaves = nxt, nxt + 1, nxt + 2 + np.arange(j)
            nxt += 2 + j
            s += [[G.q, p], np.full(k, t), np.full(j, t)]
            d += [[p, t], G.decoys[:k], leaves]
            G.fans.append((k, j, p, t))
    s = np.concatenate([np.asarray(x, np.int64) for x in s])
    d = np.concatenate([np.asarray(x, np.int64) for x in d])
    G.src, G.dst, _ = og.symmetrize_dedup(s, d)
    G.nv, G.nchain = nxt, nchain
    G.src.setflags(write=False)
    G.dst.setflags(write=False)
    return G


class View:
    """One graph as the library gets it: src / dst / renumber / symmetric / vdtype go to
    make_graph.  csr: the oracle's graph in the numbering the library builds (renumber:
    descending degree, ties by ascending id; else the ids as they are); ids[i]: the id
    the library reports for internal vertex i; ext(raw): raw ids -> the library's ids;
    internal(raw): -> row of the result arrays."""

    def __init__(self, name, src, dst, renumber, symmetric, vdtype, raw_to_ext, nv=None):
        self.name, self.renumber, self.symmetric, self.vdtype = name, renumber, symmetric, vdtype
        self.src, self.dst = src, dst
        self.inf = INT32_MAX if vdtype == np.int32 else INT64_MAX
        self._ext = raw_to_ext
        if renumber:
            ids = np.unique(np.concatenate([src, dst]))
            # compact first: the oracle's stable sort and searches are the same on ranks
            self.csr = og.create_graph(np.searchsorted(ids, src), np.searchsorted(ids, dst), None, renumber=True)
            self.ids = ids[self.csr.number_map]
        else:
            self.csr = og.create_graph(src, dst, None, renumber=False, vertices=None if nv is None else np.arange(nv))
            self.ids = np.arange(self.csr.num_vertices, dtype=np.int64)
        self.nv = self.csr.num_vertices
        order = np.argsort(self.ids, kind="stable")
        self._sorted, self._order = self.ids[order], order
        for a in (self.src, self.dst, self.ids):
            a.setflags(write=False)

    def ext(self, raw):
        return self._ext(np.asarray(raw, np.int64))

    def internal_of_ext(self, ext):
        ext = np.asarray(ext, np.int64)
        pos = np.searchsorted(self._sorted, ext)
        assert np.array_equal(self._sorted[pos], ext)
        return self._order[pos]

    def internal(self, raw):
        return self.internal_of_ext(self.ext(raw))

    def degrees(self):
        return self.csr.degrees()


def _spread(v):
    return 3 * v + 7


def _wide(v):
    return (1 << 33) + 1_000_003 * v


@functools.lru_cache(maxsize=None)
def view(name, seed=SEED, blocks=BLOCKS):
    G = case_graph(seed, blocks)
    if name == "renumbered":
        return View(name, _spread(G.src), _spread(G.dst), True, True, np.int32, _spread)
    if name == "wide64":
        return View(name, _wide(G.src), _wide(G.dst), True, True, np.int64, _wide)
    if name == "identity":
        R = view("renumbered", seed, blocks)
        to_int = np.empty(G.nv, np.int64)
        to_int[(R.ids - 7) // 3] = np.arange(G.nv)
        return View(name, to_int[G.src], to_int[G.dst], False, True, np.int32, lambda v: to_int[v])
    if name == "permuted":
        perm = np.random.default_rng(seed + 100).permutation(G.nv + 1)
        last = int(np.flatnonzero(perm == G.nv)[0])  # the isolated raw id G.nv must not get the largest id:
        perm[[last, G.nv]] = perm[[G.nv, last]]      # renumber=False counts ids 0..max of the edge list
        if perm[G.nv] == G.nv:
            perm[[0, G.nv]] = perm[[G.nv, 0]]
        return View(name, perm[G.src], perm[G.dst], False, True, np.int32, lambda v: perm[v], nv=G.nv + 1)
    if name == "directed":
        m = (G.src < G.nchain) & (G.dst < G.nchain) & (G.src < G.dst)
        s, d = G.src[m], G.dst[m]
        flip = np.random.default_rng(seed + 200).random(s.size) < 0.5
        s, d = np.where(flip, d, s), np.where(flip, s, d)
        return View(name, _spread(s), _spread(d), True, False, np.int32, _spread)
    if name == "ring":
        u = np.repeat(np.arange(RING_NV), RING_HALF)
        w = (u + np.tile(1 + np.arange(RING_HALF), RING_NV)) % RING_NV
        s, d, _ = og.symmetrize_dedup(u, w)
        return View(name, s, d, False, True, np.int32, lambda v: v)
    raise KeyError(name)


def isolated_raw(seed=SEED, blocks=BLOCKS):
    """The raw id that `permuted` keeps isolated."""
    return case_graph(seed, blocks).nv


@functools.lru_cache(maxsize=None)
def _unlimited(V, sources):
    """(distances, predecessors as internal ids) of one unlimited oracle run; read-only."""
    src = V.internal_of_ext(np.asarray(sources, np.int64))
    dist, pred = obfs.bfs(V.nv, V.csr.offsets, V.csr.indices, src, None, invalid_distance=V.inf)
    dist.setflags(write=False)
    pred.setflags(write=False)
    return dist, pred


def eccentricity(V, sources):
    """The largest distance the oracle reaches from sources (ids as the library gets them)."""
    dist, _ = _unlimited(V, tuple(int(x) for x in sources))
    return int(dist[dist != V.inf].max())


def expected(V, sources, limit=None):
    """(distances, predecessors as the library's ids) by internal vertex, from one
    unlimited oracle run per (view, sources): under a depth limit L every distance above
    L is the invalid value and its predecessor -1.  sources: ids as the library gets
    them."""
    dist, pred = _unlimited(V, tuple(int(x) for x in sources))
    out_p = np.where(pred >= 0, V.ids[np.maximum(pred, 0)], -1)
    if limit is None:
        return dist.copy(), out_p
    cut = (dist != V.inf) & (dist > int(limit))
    return np.where(cut, V.inf, dist), np.where(cut, -1, out_p)


def parent_position(V, sources):
    """For every vertex, the position in its sorted row of the first entry at distance
    d - 1 (-1 for sources and unreached vertices).  sources: ids as the library gets them."""
    dist, _ = _unlimited(V, tuple(int(x) for x in sources))
    off, idx = V.csr.offsets, V.csr.indices
    major = V.csr.majors()
    e = np.flatnonzero((dist[major] != V.inf) & (dist[major] > 0) & (dist[idx] == dist[major] - 1))
    pos = np.full(V.nv, -1, np.int64)
    rows, first = np.unique(major[e], return_index=True)  # e ascends: the first edge of each row
    pos[rows] = e[first] - off[rows]
    return pos


def check_result(V, v, dist, pred, sources, limit=None):
    """The library's (vertices, distances, predecessors) against expected(): the vertex
    ids are the oracle's number map, so ties fall as the oracle's internal ids say."""
    assert np.array_equal(v, V.ids)
    ed, ep = expected(V, sources, limit)
    bad = np.flatnonzero(dist != ed)
    assert bad.size == 0, (V.name, limit, "distances", bad[:8], dist[bad[:8]], ed[bad[:8]])
    if pred is not None and pred.size:
        bad = np.flatnonzero(pred != ep)
        assert bad.size == 0, (V.name, limit, "predecessors", bad[:8], pred[bad[:8]], ep[bad[:8]], ed[bad[:8]])


def one_source(V):
    """The chain's source, as the library's id."""
    return (int(V.ext(case_graph().source)),)


def several_sources(V):
    """Chain vertices of four blocks, one of them twice."""
    raw = [case_graph().source, 5 * BLOCK + 3, 11 * BLOCK + 40, 11 * BLOCK + 40, 20 * BLOCK + 95]
    return tuple(int(x) for x in V.ext(raw))


# name -> (bfs_alpha, bfs_beta); "default" sets neither option
SCHEDULES = {"default": (40.0, 64.0), "all_bu": (1e9, 1e9), "flip": (1e9, 1e-9), "mixed": (1e9, 64.0),
             "never": (1e-9, 64.0)}


def alpha_beta(schedule):
    """A name of SCHEDULES, or (alpha, beta) itself."""
    return SCHEDULES[schedule] if isinstance(schedule, str) else schedule


def schedule_options(schedule):
    alpha, beta = alpha_beta(schedule)
    return {} if schedule == "default" else {"bfs_alpha": alpha, "bfs_beta": beta}


def queue_start(V, sources, schedule, direction_optimizing=True):
    """Whether bfs_impl puts the sources straight into the queues (level 0 top-down, the
    source check read with level 0's counters) instead of starting from the bitmap: ids
    in degree order (a renumbered graph, or one found sorted when the bottom-up schedule
    is built) and sources x largest degree <= (E - that) / alpha."""
    deg = V.degrees()
    m_src = len(sources) * int(deg.max())
    sorted_ids = V.renumber or (direction_optimizing and bool(np.all(np.diff(deg) <= 0)))
    return sorted_ids and (not direction_optimizing or
                           m_src <= (V.csr.num_edges - m_src) / alpha_beta(schedule)[0])


def level_directions(V, sources, schedule, limit=None, direction_optimizing=True):
    """The direction of every level bfs_impl (csrc/bfs.hip) counts, "T" top-down or "B"
    bottom-up, worked out on the CPU from the oracle's level sizes:

     * the switch rule next_dir_bu: after a top-down level, bottom-up iff m_f > m_u /
       alpha; after a bottom-up level, top-down iff n_f < V / beta (n_f, m_f: the
       frontier's vertices and edges, m_u: the edges of vertices not yet reached);
     * level 0 is top-down whatever alpha says when the sources go straight to the
       queues (ids in degree order and sources x largest degree <= (E - that) / alpha);
     * the first level of a bottom-up phase is launched with the next two (as far as
       the depth limit allows), and all three are counted even where the rule would
       have left bottom-up; a level that discovers nothing ends the traversal;
     * once a bottom-up level has run, a top-down level is launched with its successor
       (when the limit allows two) and both are counted.

    The string's length is last_bfs_levels(), its count of "B" last_bfs_bottom_up_steps()."""
    alpha, beta = alpha_beta(schedule)
    dist, _ = _unlimited(V, tuple(int(x) for x in sources))
    deg = V.degrees()
    top = int(dist[dist != V.inf].max())
    n = [int((dist == d).sum()) for d in range(top + 1)]
    m = [int(deg[dist == d].sum()) for d in range(top + 1)]
    E, nv = V.csr.num_edges, V.nv
    limit = 1 << 62 if limit is None else int(limit)

    def at(d):
        return (n[d], m[d]) if d <= top else (0, 0)

    def next_bu(cur_bu, nf, mf, mu):
        if not direction_optimizing:
            return False
        if not cur_bu:
            return mf > mu / alpha
        return not (nf < nv / beta)

    quick = queue_start(V, sources, schedule, direction_optimizing)
    out, d, bu, phase = [], 0, False, 0
    while at(d)[0] > 0 and d < limit:
        nf, mf = at(d)
        mu = E - sum(m[:d + 1])
        if quick and d == 0:
            mf, mu = 0, E
        bu = next_bu(bu, nf, mf, mu)
        if bu:
            nspec = min(2, limit - d - 1) if phase == 0 else 0
            over = False
            for _ in range(nspec):
                out.append("B")
                d += 1
                if at(d)[0] == 0:
                    over = True
                    break
            if over:
                break
            out.append("B")
            d += 1
            phase += nspec + 1
        else:
            phase = 0
            pair = "B" in out and not (quick and d == 0) and d + 1 < limit
            out.append("T")
            d += 1
            if pair:
                if at(d)[0] == 0:
                    break
                out.append("T")
                d += 1
    return "".join(out)
