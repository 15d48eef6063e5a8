"""PageRank dense segments (pagerank.hip kSegDense, k_seg_bases, push_body16 kDense): a
512-entry wave segment of the packed stream that is 512 consecutive real entries of one
window -- no jump, no padding -- and whose eight rows' sources each rise by at most 255
carries a flag in its segment base; the 16K-window kernels of 32-bit ids and fp32 ranks scan
such a segment four rows per DPP chain and add without a jump test.  The same integers go
to the same slots, so flags on (pr_dense = 1) must give the vertices, the rank bits and the
iteration count of flags off (pr_dense = 0) on the same graph and options, on the first
(calibrating) call and on a second call: equality, not a tolerance.  The flags themselves
are checked against a numpy twin of the builder's rule."""
import functools
import itertools

import numpy as np
import pytest

from gpu_util import host, make_graph, plc
from oracle import graph as og
from oracle import pagerank as opr
from test_gpu_pagerank import REL, rmat_graph
from test_gpu_pagerank_runs import _hub_graph, _symmetric

pytestmark = pytest.mark.gpu

CUT = 1024   # x~ layout cut of the pr_perm = 1 cases, as in test_gpu_pagerank_layout.py
SEG = 512    # entries of a wave segment
HUB = 8064   # sources of the hub LDS table


def _run(s, d, options, renumber=True):
    """Two calls on one graph: [(vertices, rank bits, iterations)] and the schedule's
    (dense segments, packed segments)."""
    h, G = make_graph(s, d, None, transposed=True, renumber=renumber, symmetric=True, options=options)
    out = []
    for _ in range(2):
        v, r = plc().pagerank(h, G, None, None, None, None, 0.85, 1e-6, 500, False)
        out.append((host(v), host(r).view(np.uint32), h.last_iterations()))
    return out, h.last_pagerank_dense()


def _same(got, want):
    for g in got:
        assert g[2] == want[0][2] and g[2] > 0
        assert np.array_equal(g[0], want[0][0])
        assert np.array_equal(g[1], want[0][1])


def _on_off(s, d, options, **kw):
    """pr_dense = 1 against pr_dense = 0, both calls of each; returns (dense, packed)."""
    off, rep_off = _run(s, d, dict(options, pr_dense=0), **kw)
    _same(off, off)
    on, rep = _run(s, d, dict(options, pr_dense=1), **kw)
    _same(on, off)
    assert rep_off == (0, rep[1])  # the same stream, no flag
    assert 0 <= rep[0] <= rep[1]
    return rep


def _twin(s, d, wb):
    """The builder's rule on the host, for a graph that is not renumbered, has no run rows
    and no x~ layout: every packed segment as (window, dense, source before its first
    entry, its last source); the last two are -1 where the segment is not dense."""
    dmax, pmax = (1 << (16 - wb)) - 2, (1 << wb) - 1
    s, d = s.astype(np.int64), d.astype(np.int64)
    order = np.lexsort((d & pmax, s, d >> wb))
    win, src = (d >> wb)[order], s[order]
    segs = []
    for w in np.unique(win):
        sw = src[win == w]
        D = np.diff(sw, prepend=0)                   # gap to the previous entry's source (0 before the first)
        m = np.where(D > dmax, -(-D // pmax), 0)     # jumps in front of an entry
        cm = np.cumsum(m)
        pos = np.arange(sw.size) + cm                # packed position of real entry k within the window
        for p in range(0, int(pos[-1]) + 1, SEG):
            k = int(np.searchsorted(pos, p))         # first real entry at a position >= p
            kl = k + SEG - 1
            dense = m[k] == 0 and kl < sw.size and cm[kl] == cm[k]
            base = int(sw[k] - D[k])
            if dense:
                assert pos[k] == p
                before = base
                for r in range(SEG // 64):
                    last = int(sw[k + 64 * r + 63])
                    dense = dense and last - before <= 255
                    before = last
            segs.append((int(w), bool(dense), base if dense else -1, int(sw[kl]) if dense else -1))
    return segs


def _counts(segs):
    return sum(1 for g in segs if g[1]), len(segs)


@functools.lru_cache(maxsize=None)
def _crafted():
    """Not renumbered, 12.5 K ids, one 16K window.  Sources 0 .. ~8600 in ascending order with
    8-40 destinations each (in a pool of ids above them) and id gaps of 1 or 2, so the stream
    is dense but for three gaps of 3 (one jump each): at the first position of segment 4, at
    the last position of segment 6 and in the middle of segment 10.  The sources run past the
    8064 of the hub table; the pool's own entries (sources above it) follow, and the window's
    last segment is padded.  Returns the edges and the stream positions of the three jumps."""
    n = 12_500
    rng = np.random.default_rng(5)
    ids, degs, jumps = [], [], []
    prev, pos = 0, 0

    def add(gap, deg):
        nonlocal prev, pos
        assert 8 <= deg <= 40
        prev += gap
        if gap > 2:
            jumps.append(pos)
            pos += 1
        ids.append(prev)
        degs.append(deg)
        pos += deg

    def clean_to(target):  # sources with gaps of 1 or 2 until the stream is exactly target entries long
        while pos < target:
            left = target - pos
            deg = int(rng.integers(8, 41)) if left > 80 else left // 2 if left > 40 else left
            add(int(rng.integers(1, 3)) if ids else 0, deg)

    clean_to(4 * SEG)
    add(3, 20)                 # the jump is the first entry of segment 4
    clean_to(7 * SEG - 1)
    add(3, 20)                 # the jump is the last entry of segment 6
    clean_to(10 * SEG + 200)
    add(3, 20)                 # a jump in the middle of segment 10
    while prev < HUB + 500:
        clean_to(pos + 2000)
    assert jumps == [4 * SEG, 7 * SEG - 1, 10 * SEG + 200]
    pool = np.arange(prev + 2, n)
    assert pool.size > 1000
    s = np.repeat(np.asarray(ids), degs)
    d = np.concatenate([rng.choice(pool, k, replace=False) for k in degs])
    s, d = _symmetric(s, d)
    assert max(s.max(), d.max()) < n
    return s, d, tuple(jumps)


def test_twin_on_crafted_graph():
    """The crafted graph has the segments it is meant to have (host only: the twin's view)."""
    s, d, jumps = _crafted()
    segs = _twin(s, d, 14)
    dense = [g[1] for g in segs]
    assert all(g[0] == 0 for g in segs)
    assert dense[:12] == [True, True, True, True, False, True, False, False, True, True, False, True]
    assert not dense[-1] and (s.size + len(jumps)) % SEG != 0        # the window's padded last segment
    assert any(g[1] and g[3] < HUB for g in segs)                     # wholly below the hub table
    assert any(g[1] and g[2] >= HUB for g in segs)                    # wholly above it
    assert sum(1 for g in segs if g[1] and g[2] < HUB <= g[3]) == 1   # one straddles it
    assert 0 < _counts(segs)[0] < _counts(segs)[1]


@pytest.mark.parametrize("hub,enc", list(itertools.product((0, 1), repeat=2)))
def test_crafted_graph(hub, enc):
    """Jumps at the first, the last and a middle position of a segment, the padded last
    segment, and dense segments below, above and across the end of the hub table, with the
    table on and off: the reporter's counts are the twin's, the ranks those without flags."""
    s, d, _ = _crafted()
    rep = _on_off(s, d, {"pr_win_bits": 14, "pr_runs": 0, "pr_perm": 0, "pr_hub": hub, "pr_enc": enc},
                  renumber=False)
    assert rep == _counts(_twin(s, d, 14))
    assert 0 < rep[0] < rep[1]


@functools.lru_cache(maxsize=None)
def _rows_255_256():
    """Not renumbered, for 4K windows (4-bit deltas, up to 14 in an entry).  Sources 0 .. ~2000
    with one destination each, all in the window of ids 8192 .. 8255, so an entry's delta is
    its source's id gap: gaps of 1, but row 3 of segment 0 rises by exactly 255 (63 gaps of 4
    and one of 3: still dense) and row 5 of segment 1 by 256 (64 gaps of 4: not dense)."""
    gaps = np.ones(3 * SEG + 100, np.int64)
    gaps[0] = 0
    gaps[3 * 64:4 * 64] = 4
    gaps[3 * 64] = 3
    gaps[SEG + 5 * 64:SEG + 6 * 64] = 4
    a = np.cumsum(gaps)
    assert a[4 * 64 - 1] - a[3 * 64 - 1] == 255 and a[SEG + 6 * 64 - 1] - a[SEG + 5 * 64 - 1] == 256
    assert a[-1] < 4096
    return _symmetric(a, 8192 + np.arange(a.size) % 64)


@pytest.mark.parametrize("graph,wb", [("crafted", 12), ("crafted", 13), ("crafted", 15), ("rows", 12), ("rows", 14)])
def test_other_window_sizes(graph, wb):
    """4K, 8K and 32K windows: their kernels have no dense path and mask the flag, so the
    ranks are those without flags; the builder's rule is the same at every size, a row rising
    by 255 is inside it and one rising by 256 is not."""
    s, d = _crafted()[:2] if graph == "crafted" else _rows_255_256()
    rep = _on_off(s, d, {"pr_win_bits": wb, "pr_runs": 0, "pr_perm": 0}, renumber=False)
    segs = _twin(s, d, wb)
    assert rep == _counts(segs)
    assert rep[0] > 0 or wb == 15  # (1-bit deltas: every new source is a jump, the crafted graph has no dense segment)
    if graph == "rows" and wb == 12:
        assert [g[1] for g in segs if g[0] == 2] == [True, False, True, False]


@pytest.mark.parametrize("runs", [0, 1])
def test_runs_beside_dense_segments(runs):
    """The hub graph of the run-row tests: without run rows its hubs' long runs of delta 0 lie
    in dense packed segments; with them the runs leave the stream and the other segments
    shift."""
    s, d = _hub_graph()
    rep = _on_off(s, d, {"pr_win_bits": 14, "pr_runs": runs, "pr_run_min": 64, "pr_perm": 0}, renumber=False)
    assert rep[0] > 0
    if runs == 0:
        assert rep == _counts(_twin(s, d, 14))


@functools.lru_cache(maxsize=None)
def _rmat(scale):
    s, d, _ = rmat_graph(scale, False, True)
    return s, d


@pytest.mark.parametrize("perm,fuse,enc,whole", list(itertools.product((0, 1), repeat=4)))
@pytest.mark.parametrize("scale", [16, 18])
def test_rmat(scale, perm, fuse, enc, whole):
    """Renumbered RMAT at 16K windows, with and without the x~ layout (the sources are
    positions then), fused and separate apply, encoded and plain x~, stored and added
    windows.  RMAT-18's first window is cut into several items, whose shares flush with
    atomics."""
    s, d = _rmat(scale)
    rep = _on_off(s, d, {"pr_win_bits": 14, "pr_perm": perm, "pr_perm_cut": CUT, "pr_perm_span": 1,
                         "pr_fuse": fuse, "pr_enc": enc, "pr_whole": whole})
    assert 0 < rep[0] < rep[1]


def test_shared_windows():
    """RMAT-16 with its first window cut into many items (as in the run-row tests): dense
    segments in the shares of a window that several items sum."""
    s, d = _rmat(16)
    for whole in (1, 0):
        rep = _on_off(s, d, {"pr_win_bits": 14, "pr_share_div": 16, "pr_whole": whole})
        assert rep[0] > 0


def test_dense_vs_oracle():
    s, d = _rmat(16)
    out, rep = _run(s, d, {"pr_win_bits": 14, "pr_dense": 1})
    assert rep[0] > 0
    og_g = og.create_graph(s, d, None, store_transposed=True, renumber=True)
    ref = np.zeros(int(og_g.number_map.max()) + 1)
    ref[og_g.number_map] = opr.pagerank_from_graph(og_g, alpha=0.85, epsilon=1e-6, max_iterations=500)
    vv = out[0][0]
    got = np.zeros(ref.size)
    got[vv] = out[0][1].view(np.float32)
    assert vv.size == og_g.num_vertices
    assert (np.abs(got[vv] - ref[vv]) / ref[vv]).max() < REL
