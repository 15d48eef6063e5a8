"""PageRank x~ layout (pagerank.hip build_x_layout): the x~ of the vertices past a cut is
stored at pos[v], clustered by the destination windows a vertex feeds, and the packed
push schedule is built in position space.  No sum is added or split, so the layout on
(pr_perm = 1) must give the vertices, the rank bits and the iteration count of the
layout off (pr_perm = 0), on the first (calibrating) call and on a second call on the
cached schedule.  The sums are integers and order-free: equality, not a tolerance."""
import functools
import itertools

import numpy as np
import pytest

from gpu_util import host, make_graph, plc
from oracle import graph as og
from oracle import pagerank as opr
from test_gpu_pagerank import REL, rmat_graph

pytestmark = pytest.mark.gpu

CUT = 1024  # rounded up to one window: every window but the first is permuted


def _plain(h, G):
    return plc().pagerank(h, G, None, None, None, None, 0.85, 1e-6, 500, False)


def _run(s, d, options, w=None, symmetric=True, renumber=True, call=_plain):
    """Two calls on one graph: [(vertices, rank bits, iterations)] and the schedule's
    (stream entries, permuted vertices)."""
    h, G = make_graph(s, d, w, transposed=True, renumber=renumber, symmetric=symmetric, options=options)
    out = []
    for _ in range(2):
        v, r = call(h, G)
        out.append((host(v), host(r).view(np.uint32), h.last_iterations()))
    return out, h.last_pagerank_schedule()


def _same(got, want):
    for g in got:
        assert g[2] == want[0][2] and g[2] > 0
        assert np.array_equal(g[0], want[0][0])
        assert np.array_equal(g[1], want[0][1])


@functools.lru_cache(maxsize=None)
def _rmat16():
    s, d, _ = rmat_graph(16, False, True)
    return s, d, int(np.unique(np.concatenate([s, d])).size)


@functools.lru_cache(maxsize=None)
def _rmat16_off(wb):
    s, d, _ = _rmat16()
    out, sched = _run(s, d, {"pr_win_bits": wb, "pr_perm": 0})
    assert sched[1] == 0
    _same(out, out)
    return out


@pytest.mark.parametrize("span", [1, 4, 0])
@pytest.mark.parametrize("wb", [14, 15, 12])
def test_layout_bitwise_equal(wb, span):
    """RMAT-16 (46.8 K vertices with edges: three 16K windows, the last partial) at 16K,
    32K and 4K windows, ranges of one window, of four, and the whole tail."""
    s, d, nv = _rmat16()
    assert 2 * 16384 < nv < 3 * 16384
    out, sched = _run(s, d, {"pr_win_bits": wb, "pr_perm": 1, "pr_perm_cut": CUT, "pr_perm_span": span})
    assert sched[1] == nv - (1 << wb)  # the cut rounded up to one window
    _same(out, _rmat16_off(wb))


@pytest.mark.parametrize("fuse,whole,hub,enc", list(itertools.product((0, 1), repeat=4)))
def test_layout_bitwise_equal_kernel_variants(fuse, whole, hub, enc):
    """16K windows: fused and separate apply, stored and added windows, hub x~ in LDS or
    gathered, encoded and plain x~ -- every writer and reader of x~."""
    s, d, nv = _rmat16()
    base = {"pr_win_bits": 14, "pr_fuse": fuse, "pr_whole": whole, "pr_hub": hub, "pr_enc": enc}
    off, _ = _run(s, d, dict(base, pr_perm=0))
    on, sched = _run(s, d, dict(base, pr_perm=1, pr_perm_cut=CUT, pr_perm_span=1))
    assert sched[1] == nv - 16384
    _same(on, off)
    _same(off, _rmat16_off(14))


def test_cut_rounded_up_to_a_window():
    s, d, nv = _rmat16()
    out, sched = _run(s, d, {"pr_win_bits": 14, "pr_perm": 1, "pr_perm_cut": 1000, "pr_perm_span": 1})
    assert sched[1] == nv - 16384
    _same(out, _rmat16_off(14))
    out, sched = _run(s, d, {"pr_win_bits": 14, "pr_perm": 1, "pr_perm_cut": 16385, "pr_perm_span": 1})
    assert sched[1] == nv - 32768
    _same(out, _rmat16_off(14))


@pytest.mark.parametrize("cut", ["nv", "above", "last_window"])
def test_inactive_layout_has_no_map(cut):
    """A cut at or past the last vertex (after rounding) leaves nothing to move: the
    schedule is the identity one, entry for entry, and no map is kept."""
    s, d, nv = _rmat16()
    c = {"nv": nv, "above": 1 << 20, "last_window": 2 * 16384 + 1}[cut]
    off, sched_off = _run(s, d, {"pr_win_bits": 14, "pr_perm": 0})
    out, sched = _run(s, d, {"pr_win_bits": 14, "pr_perm": 1, "pr_perm_cut": c, "pr_perm_span": 1})
    assert sched[1] == 0 and sched[0] == sched_off[0] > 0
    _same(out, off)


def _pendant_graph():
    """Not renumbered.  Hub 0 joined to leaves at the odd ids; a ring over the first half
    of the leaves (degree 3), the others pendant (degree 1, on the hub); the even ids
    never appear (degree 0).  About 60 K ids: rows of degree 3, 1 and 0 in every permuted
    range, the last window partial."""
    n = 30_000
    leaves = (1 + 2 * np.arange(n)).astype(np.int32)
    ring = leaves[: n // 2]
    s = np.concatenate([np.zeros(n, np.int32), ring])
    d = np.concatenate([leaves, np.roll(ring, -1)])
    return np.concatenate([s, d]), np.concatenate([d, s]), int(leaves[-1]) + 1


@pytest.mark.parametrize("wb,span", [(14, 1), (14, 0), (12, 4), (15, 1)])
def test_layout_short_and_empty_rows(wb, span):
    s, d, n = _pendant_graph()
    off, _ = _run(s, d, {"pr_win_bits": wb, "pr_perm": 0}, renumber=False)
    on, sched = _run(s, d, {"pr_win_bits": wb, "pr_perm": 1, "pr_perm_cut": CUT, "pr_perm_span": span},
                     renumber=False)
    assert off[0][0].size == n and sched[1] == n - (1 << wb)
    _same(on, off)
    # Against the oracle, in L1: both stop at an L1 step below epsilon, which leaves each
    # within alpha / (1 - alpha) * epsilon of the fixed point, plus the fp32 ranks' rounding
    # (2^-24 of a total mass of 1).  (The hub holds 0.27 of the mass, so a per-vertex
    # relative bound of 1e-6 is tighter than the stop rule allows here, layout or not.)
    eps, alpha = 1e-6, 0.85
    got = np.zeros(n)
    got[on[0][0]] = on[0][1].view(np.float32)
    ref = opr.pagerank(n, s, d, None, alpha, eps, 500)
    l1 = np.abs(got - ref).sum()
    print(f"L1 distance to the oracle {l1:.3e}")
    assert l1 < 2 * alpha / (1 - alpha) * eps + 2.0 ** -24


@pytest.mark.parametrize("what", ["personalized", "initial_guess"])
def test_layout_other_inputs(what):
    """Personalization and the initial guess are indexed by vertex, not by position."""
    s, d, nv = _rmat16()
    rng = np.random.default_rng(7)
    ids = rng.choice(np.unique(s), 2000, replace=False).astype(np.int32)
    vals = (rng.random(ids.size) + 0.1).astype(np.float32)
    if what == "personalized":
        def call(h, G):
            return plc().personalized_pagerank(h, G, None, None, None, None, ids, vals, 0.85, 1e-6, 500, False)
    else:
        def call(h, G):
            return plc().pagerank(h, G, None, None, ids, vals, 0.85, 1e-6, 500, False)
    off, _ = _run(s, d, {"pr_win_bits": 14, "pr_perm": 0}, call=call)
    for span in (1, 0):
        on, sched = _run(s, d, {"pr_win_bits": 14, "pr_perm": 1, "pr_perm_cut": CUT, "pr_perm_span": span}, call=call)
        assert sched[1] == nv - 16384
        _same(on, off)
    assert not np.array_equal(off[0][1], _rmat16_off(14)[0][1])  # (the inputs were used)


@pytest.mark.parametrize("graph", ["weighted", "non_symmetric"])
def test_identity_paths_keep_no_map(graph):
    """Weighted entries and the general build keep x~[v] at v whatever pr_perm says."""
    if graph == "weighted":
        s, d, w = rmat_graph(16, True, True)
        kw = dict(w=w.astype(np.float32), symmetric=True)
    else:
        s, d, _ = rmat_graph(16, False, False)
        kw = dict(symmetric=False)
    off, _ = _run(s, d, {"pr_win_bits": 14, "pr_perm": 0}, **kw)
    on, sched = _run(s, d, {"pr_win_bits": 14, "pr_perm": 1, "pr_perm_cut": CUT, "pr_perm_span": 1}, **kw)
    assert sched[1] == 0
    _same(on, off)


def test_layout_vs_oracle():
    s, d, nv = _rmat16()
    out, sched = _run(s, d, {"pr_win_bits": 14, "pr_perm": 1, "pr_perm_cut": CUT, "pr_perm_span": 1})
    assert sched[1] == nv - 16384
    og_g = og.create_graph(s, d, None, store_transposed=True, renumber=True)
    ref = np.zeros(int(og_g.number_map.max()) + 1)
    ref[og_g.number_map] = opr.pagerank_from_graph(og_g, alpha=0.85, epsilon=1e-6, max_iterations=500)
    vv = out[0][0]
    got = np.zeros(ref.size)
    got[vv] = out[0][1].view(np.float32)
    assert vv.size == og_g.num_vertices
    assert (np.abs(got[vv] - ref[vv]) / ref[vv]).max() < REL
