"""PageRank run rows (pagerank.hip k_run_flags, push_body16's run units): a run of
equal (destination window, source) of at least pr_run_min entries gives floor(L / 64)
rows of 64 slots and one source, which leave the packed stream; the push reads a row's
source and x~ word once and a lane only adds at its slot.  Moving entries
between the two storage forms adds the same integers, so run rows on (pr_runs = 1) must
give the vertices, the rank bits and the iteration count of run rows off (pr_runs = 0)
on the same graph and options, on the first (calibrating) call and on a second call on
the cached schedule: equality, not a tolerance."""
import functools
import itertools

import numpy as np
import pytest

from gpu_util import host, make_graph, plc
from oracle import graph as og
from oracle import pagerank as opr
from test_gpu_pagerank import REL, rmat_graph

pytestmark = pytest.mark.gpu

CUT = 1024  # x~ layout cut of the pr_perm = 1 cases, as in test_gpu_pagerank_layout.py


def _plain(h, G):
    return plc().pagerank(h, G, None, None, None, None, 0.85, 1e-6, 500, False)


def _run(s, d, options, w=None, renumber=True, call=_plain, wdtype=np.float32):
    """Two calls on one graph: [(vertices, rank bits, iterations)], the schedule's
    (stream entries, permuted vertices) and its (run rows, entries in run rows)."""
    h, G = make_graph(s, d, w, transposed=True, renumber=renumber, symmetric=True, options=options, wdtype=wdtype)
    out = []
    for _ in range(2):
        v, r = call(h, G)
        r = host(r)
        out.append((host(v), r.view(np.uint32 if r.dtype == np.float32 else np.uint64), h.last_iterations()))
    return out, h.last_pagerank_schedule(), h.last_pagerank_runs()


def _same(got, want):
    for g in got:
        assert g[2] == want[0][2] and g[2] > 0
        assert np.array_equal(g[0], want[0][0])
        assert np.array_equal(g[1], want[0][1])


def _on_off(s, d, options, tmin=64, **kw):
    """pr_runs = 1 against pr_runs = 0, both calls of each; returns the run-row report."""
    off, sched_off, runs_off = _run(s, d, dict(options, pr_runs=0), **kw)
    assert runs_off == (0, 0)
    _same(off, off)
    on, sched, runs = _run(s, d, dict(options, pr_runs=1, pr_run_min=tmin), **kw)
    _same(on, off)
    assert runs[1] == 64 * runs[0]
    if runs[0] == 0:
        assert sched == sched_off  # no run of tmin: the schedule without run rows
    return runs, sched, sched_off


def _expected_rows(s, d, wb, tmin):
    """Sum of floor(L / 64) over the runs of equal (destination window, source) of at
    least tmin entries -- ids as given (graphs that are not renumbered)."""
    key = (d.astype(np.int64) >> wb) * (int(max(s.max(), d.max())) + 1) + s.astype(np.int64)
    L = np.unique(key, return_counts=True)[1]
    return int((L[L >= tmin] // 64).sum())


def _symmetric(s, d):
    e = np.unique(np.stack([np.concatenate([s, d]), np.concatenate([d, s])], axis=1), axis=0)
    e = e[e[:, 0] != e[:, 1]]
    return e[:, 0].astype(np.int32), e[:, 1].astype(np.int32)


HUB_DEGREES = (63, 64, 65, 127, 128, 129, 511, 512, 513, 575, 1000)


@functools.lru_cache(maxsize=None)
def _hub_graph():
    """Not renumbered, 12.5 K ids (one 16K window, four 4K windows).  Eleven hubs with
    exactly HUB_DEGREES neighbours, spread over the ids so that some lie past the 8064
    sources of the hub LDS table; a ring over the other vertices (degree 2 plus the hubs
    they touch) sits between them."""
    n = 12_500
    rng = np.random.default_rng(11)
    hubs = 500 + 1100 * np.arange(len(HUB_DEGREES))
    assert hubs[-1] > 8064 and hubs[-1] < n
    low = np.setdiff1d(np.arange(n), hubs)
    s, d = [low], [np.roll(low, -1)]
    for hv, deg in zip(hubs, HUB_DEGREES):
        nb = rng.choice(low, deg, replace=False)
        s.append(np.full(deg, hv))
        d.append(nb)
    s, d = _symmetric(np.concatenate(s), np.concatenate(d))
    assert np.array_equal(np.bincount(s, minlength=n)[hubs], HUB_DEGREES)
    return s, d


@pytest.mark.parametrize("tmin", [64, 128])
@pytest.mark.parametrize("wb", [14, 15, 12])
def test_run_length_edges(wb, tmin):
    """Runs of exactly 63 ... 1000 entries: none below tmin gives a row, the others
    floor(L / 64) rows and L mod 64 packed entries (4K windows cut the runs further)."""
    s, d = _hub_graph()
    want = _expected_rows(s, d, wb, tmin)
    if wb >= 14:
        assert want == sum(L // 64 for L in HUB_DEGREES if L >= tmin)
    runs, sched, sched_off = _on_off(s, d, {"pr_win_bits": wb}, tmin, renumber=False)
    assert runs[0] == want > 0
    # the rows' entries left the packed stream (whose windows are padded to 512 entries)
    assert sched[0] <= sched_off[0]
    if wb >= 14:
        assert sched[0] <= sched_off[0] - 64 * want + 512


def _star_ring(n_leaves):
    """Hub 0 joined to leaves 1 .. n_leaves, a ring over the leaves."""
    leaves = np.arange(1, n_leaves + 1)
    return _symmetric(np.concatenate([np.zeros(n_leaves, np.int64), leaves]),
                      np.concatenate([leaves, np.roll(leaves, -1)]))


@pytest.mark.parametrize("wb", [14, 15])
def test_run_longer_than_a_unit(wb):
    """One source with 9000 entries in one window: 140 rows, more than the 128 of a unit
    (two run units), padded with 4 rows to a whole segment, and 40 packed entries."""
    s, d = _star_ring(9000)
    runs, _, _ = _on_off(s, d, {"pr_win_bits": wb}, renumber=False)
    assert runs[0] == 9000 // 64 == 140 and runs[0] % 8 != 0


@pytest.mark.parametrize("n,rows", [(65, 65), (128, 128)])
@pytest.mark.parametrize("wb", [14, 15, 12])
def test_complete_graphs(wb, n, rows):
    """K65: every source has exactly 64 entries, so the window's packed stream is empty
    (and 65 rows need 7 padding rows).  K128: one row and 63 packed entries per source."""
    i, j = np.meshgrid(np.arange(n), np.arange(n))
    s, d = _symmetric(i.ravel(), j.ravel())
    runs, sched, _ = _on_off(s, d, {"pr_win_bits": wb}, renumber=False)
    assert runs[0] == rows
    if n == 65:
        assert sched[0] == 0


@pytest.mark.parametrize("graph", ["ring", "rmat10"])
def test_no_runs(graph):
    """No run of pr_run_min: no run units, the reporter says 0 and the schedule is
    unchanged.  The ring has no run of 2.  RMAT-10's hubs do have more than 64 neighbours in
    a window (its 1024 vertices are one), so there pr_run_min is set above every degree."""
    if graph == "ring":
        v = np.arange(5000)
        s, d = _symmetric(v, np.roll(v, -1))
    else:
        s, d, _ = rmat_graph(10, False, True)
    for wb in (14, 12):
        runs, sched, sched_off = _on_off(s, d, {"pr_win_bits": wb}, 64 if graph == "ring" else 1 << 20)
        assert runs == (0, 0) and sched == sched_off and sched[0] > 0


@pytest.mark.parametrize("options", [{"pr_win_bits": 13}, {"pr_win_bits": 12, "pr_enc": 0}])
def test_kernels_without_run_path(options):
    """The 8K-window kernel and the 4K-window kernel for plain-float x~ have no run path:
    pr_runs = 1 is ignored there, the reporter says 0 and the schedule is the one without
    run rows (_on_off checks that), on a graph that has run rows at the other sizes."""
    s, d = _hub_graph()
    runs, _, _ = _on_off(s, d, options, renumber=False)
    assert runs == (0, 0)


@functools.lru_cache(maxsize=None)
def _rmat16():
    s, d, _ = rmat_graph(16, False, True)
    return s, d


def test_shared_windows():
    """RMAT-16 at 16K windows with the first window cut into many items: the windows
    summed by several items hold run units and packed units (win_multi / win_left count
    items over both kinds), with stored and with added whole windows."""
    s, d = _rmat16()
    for whole in (1, 0):
        runs, _, _ = _on_off(s, d, {"pr_win_bits": 14, "pr_share_div": 16, "pr_whole": whole})
        assert runs[0] > 128  # more than a unit's rows


@pytest.mark.parametrize("tmin", [64, 128])
@pytest.mark.parametrize("fuse,whole,hub,enc,perm", list(itertools.product((0, 1), repeat=5)))
def test_kernel_variants(fuse, whole, hub, enc, perm, tmin):
    """16K windows: fused and separate apply, stored and added windows, the hub table on
    and off (off: every row's source is past it), encoded and plain x~, with and without
    the x~ layout (the rows' sources are positions then)."""
    s, d = _rmat16()
    base = {"pr_win_bits": 14, "pr_fuse": fuse, "pr_whole": whole, "pr_hub": hub, "pr_enc": enc, "pr_perm": perm,
            "pr_perm_cut": CUT, "pr_perm_span": 1}
    runs, _, _ = _on_off(s, d, base, tmin)
    assert runs[0] > 0


def test_rows_past_the_hub_table():
    """Sources past the 8064 of the hub LDS table with run rows, hub table on: the hub
    graph's last hubs (ids above 8064, not renumbered)."""
    s, d = _hub_graph()
    assert np.unique(s[np.isin(s, 500 + 1100 * np.arange(11)) & (s > 8064)]).size >= 3
    for enc in (0, 1):
        runs, _, _ = _on_off(s, d, {"pr_win_bits": 14, "pr_hub": 1, "pr_enc": enc}, renumber=False)
        assert runs[0] == sum(L // 64 for L in HUB_DEGREES if L >= 64)


@pytest.mark.parametrize("enc", [0, 1])
def test_wide_windows(enc):
    """32K windows (32-bit LDS words and carries) on RMAT-16, and on a small dense graph
    whose x~ terms are large (high words and many carries in the run rows)."""
    s, d = _rmat16()
    runs, _, _ = _on_off(s, d, {"pr_win_bits": 15, "pr_enc": enc})
    assert runs[0] > 0
    i, j = np.meshgrid(np.arange(200), np.arange(200))
    s, d = _symmetric(i.ravel(), j.ravel())
    runs, _, _ = _on_off(s, d, {"pr_win_bits": 15, "pr_enc": enc}, renumber=False)
    assert runs[0] == 200 * (199 // 64)


def test_multigraph_run_longer_than_a_window():
    """Duplicate edges (graph creation keeps them) repeat a slot in a run: 500 leaves joined
    70 times each to one hub give a run of 35,000 entries of one source in one 16K window --
    more than a window's slots, over nine of k_run_flags' tiles -- and runs of 70 the other
    way."""
    leaves = np.repeat(np.arange(1, 501), 70)
    hub = np.zeros(leaves.size, np.int64)
    s, d = np.concatenate([hub, leaves]).astype(np.int32), np.concatenate([leaves, hub]).astype(np.int32)
    for wb in (14, 15):
        runs, _, _ = _on_off(s, d, {"pr_win_bits": wb}, renumber=False)
        assert runs[0] == 35000 // 64 + 500 == _expected_rows(s, d, wb, 64)


@pytest.mark.parametrize("what", ["fp64", "personalized", "initial_guess"])
def test_other_inputs(what):
    """Personalization and an initial guess on RMAT-14; fp64 ranks (all-ones fp64 weights:
    the packed push with plain fp64 x~) keep the schedule without run rows whatever pr_runs
    says -- the fp64 kernels have no run path -- and the same bits."""
    s, d, _ = rmat_graph(14, False, True)
    rng = np.random.default_rng(7)
    ids = rng.choice(np.unique(s), 1000, replace=False).astype(np.int32)
    kw = {}
    if what == "fp64":
        kw = dict(w=np.ones(s.size, np.float64), wdtype=np.float64)
        vals = None
    else:
        vals = (rng.random(ids.size) + 0.1).astype(np.float32)
    if what == "personalized":
        def call(h, G):
            return plc().personalized_pagerank(h, G, None, None, None, None, ids, vals, 0.85, 1e-6, 500, False)
    elif what == "initial_guess":
        def call(h, G):
            return plc().pagerank(h, G, None, None, ids, vals, 0.85, 1e-6, 500, False)
    else:
        call = _plain
    runs, _, _ = _on_off(s, d, {"pr_win_bits": 14}, call=call, **kw)
    assert (runs[0] == 0) if what == "fp64" else (runs[0] > 0)


def test_runs_vs_oracle():
    s, d = _rmat16()
    out, _, runs = _run(s, d, {"pr_win_bits": 14, "pr_runs": 1, "pr_run_min": 64})
    assert runs[0] > 0
    og_g = og.create_graph(s, d, None, store_transposed=True, renumber=True)
    ref = np.zeros(int(og_g.number_map.max()) + 1)
    ref[og_g.number_map] = opr.pagerank_from_graph(og_g, alpha=0.85, epsilon=1e-6, max_iterations=500)
    vv = out[0][0]
    got = np.zeros(ref.size)
    got[vv] = out[0][1].view(np.float32)
    assert vv.size == og_g.num_vertices
    assert (np.abs(got[vv] - ref[vv]) / ref[vv]).max() < REL
