"""The packed 16-bit push stream of PageRank (pagerank.hip assemble_packed), pinned from its
definition.  Both schedule builders -- the general one (build_push_from_coo: non-symmetric
graphs, 64-bit ids, pr_fast_build = 0) and the symmetric one-word-key one
(build_push_packed_sym) -- hand their sorted keys to the same assembler.  The rank tests
compare fixed-point sums, which do not depend on the order or the padding of the stream, so
they cannot see a stream whose jumps, padding or unit boundaries changed; the stream's
length can.

The definition: the entries of a destination window 2^wb rows wide, in (window, source,
slot) order.  An entry whose source lies D past the previous entry's of its window (past 0
at the window's first) codes D in its 16 bits when D <= dmax = 2^(16 - wb) - 2; else it
takes ceil(D / pmax) jump entries in front of it, pmax = 2^wb - 1.  Every window is then
padded to a multiple of 512 entries."""
import functools

import numpy as np
import pytest

from gpu_util import host, make_graph, plc
from oracle import pagerank as opr
from test_gpu_pagerank import REL
from test_gpu_pagerank_runs import _symmetric

SEG = 512    # entries of a wave segment: windows are padded to whole ones
UNIT = 8192  # entries of a unit: a longer window needs segment bases past its first unit


def _window_entries(src, dst, wb):
    """Per entry in (window, source) order: its window, its source gap D and whether it is
    its window's first."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    order = np.lexsort((dst, src, dst >> wb))
    w, s = (dst >> wb)[order], src[order]
    first = np.ones(w.size, bool)
    first[1:] = w[1:] != w[:-1]
    prev = np.concatenate([[0], s[:-1]])
    prev[first] = 0
    return w, s - prev, first


def stream_windows(src, dst, wb, nwin=None):
    """Unpadded packed length of every destination window of the edges src -> dst."""
    pmax, dmax = (1 << wb) - 1, (1 << (16 - wb)) - 2
    w, D, _ = _window_entries(src, dst, wb)
    cost = 1 + np.where(D > dmax, -(-D // pmax), 0)
    n = max(int(nwin or 0), int(w.max()) + 1 if w.size else 0)
    return np.bincount(w, weights=cost, minlength=n).astype(np.int64)


def stream_length(src, dst, wb):
    return int((-(-stream_windows(src, dst, wb) // SEG) * SEG).sum())


def test_stream_length_by_hand():
    """Three 4K windows (dmax 14, pmax 4095), worked by hand.
    Window 0, sources 5, 5, 10, 30, 9000: gaps 5, 0, 5 are coded (1 entry each); 20 takes
    one jump (2); 8970 takes ceil(8970 / 4095) = 3 jumps (4): 9 entries.
    Window 1: none.
    Window 2, sources 4096, 8191: 4096 from the window start takes 2 jumps (3), 4095 takes
    one (2): 5 entries.
    Padded: 512 + 0 + 512.
    The same edges in one 32K window (dmax 0, pmax 32767), sources 5, 5, 10, 30, 4096, 8191,
    9000: every new source takes one jump: 2 + 1 + 2 + 2 + 2 + 2 + 2 = 13."""
    src = np.array([5, 5, 10, 30, 9000, 4096, 8191])
    dst = np.array([1, 2, 1, 7, 3, 8192, 8200])
    assert stream_windows(src, dst, 12).tolist() == [9, 0, 5]
    assert stream_length(src, dst, 12) == 1024
    assert stream_windows(src, dst, 15).tolist() == [13]
    assert stream_length(src, dst, 15) == 512
    # whole segments take no padding, one entry more takes 511
    one = np.ones(513, np.int64)
    assert stream_length(one[:512], np.arange(512), 12) == 512
    assert stream_length(one, np.arange(513), 12) == 1024
    # a gap of exactly pmax is one jump, pmax + 1 two; dmax is still coded, dmax + 1 is not
    assert stream_windows([4095, 8191], [0, 0], 12).tolist() == [2 + 3]
    assert stream_windows([14, 29], [0, 0], 12).tolist() == [1 + 2]


def _block(a, b):
    i, j = np.meshgrid(a, b)
    return np.stack([i.ravel(), j.ravel()], axis=1)


WBS = (12, 14, 15)


@functools.lru_cache(maxsize=None)
def _stream_graph():
    """Not renumbered, 81,920 ids: low vertices L below 12,288 (4K windows 0, 1, 2; one
    16K and one 32K window), high vertices H from 65,536 (4K windows 16 .. 19), nothing
    between, so every window size has windows without an entry.  L has no edge inside
    itself: the sources of its windows are all in H, above every pmax (jumps at a window
    start).  The edges inside H join vertices from 77,824 on only, so in a window of H the
    last source from L and the first from H lie more than 2 x 32,767 apart (three jumps
    before one entry).  Complete bipartite blocks give most entries the source of the entry
    before them, so the stream packs even at 32K windows, where every new source takes a
    jump; the block of window 0 has 10,000 entries, more than a unit.

    Filler edges then bring window lengths to whole segments and to one entry more:
    4K windows 1 and 2; L (16K and 32K) to a whole number; H (16K and 32K) to one more.
    A filler of an L window joins a new vertex of it to a source the window already has
    (one entry at every window size), or a new last source right behind the window's last
    (one entry, two at 32K windows); H's own fillers join vertices of H (counted below)."""
    A1, B1 = np.arange(100, 200), np.arange(66000, 66100)    # window 0: 10,000 entries
    A2, B2 = np.arange(4200, 4240), np.arange(70000, 70030)  # window 1
    A3, B3 = np.arange(8300, 8350), np.arange(74000, 74020)  # window 2
    A4 = np.arange(20, 30)
    U, V = np.arange(78000, 78040), np.arange(79000, 79050)  # the edges inside H
    pairs = [_block(A1, B1), _block(A2, B2), _block(A3, B3), _block(A4, U), _block(U, V)]

    def graph():
        e = np.concatenate(pairs)
        return _symmetric(e[:, 0], e[:, 1])

    def lens(wb):
        return stream_windows(*graph(), wb, nwin=81920 >> wb)

    # 4K windows 1 and 2
    f1, f2 = -lens(12)[1] % SEG, (1 - lens(12)[2]) % SEG
    pairs.append(_block(A2[-1] + 1 + np.arange(f1), B2[:1]))
    pairs.append(_block(A3[-1] + 1 + np.arange(f2), B3[:1]))
    # L at 16K and at 32K windows: f0 entries of one each, g0 of (1, 2)
    l14, l15 = lens(14)[0], lens(15)[0]
    g0 = (l14 - l15) % SEG
    f0 = (-l14 - g0) % SEG
    pairs.append(_block(A1[-1] + 1 + np.arange(f0), B1[:1]))
    pairs.append(_block(A4[:1], U[-1] + 1 + np.arange(g0)))  # (U are L's last sources)
    # H at 16K and at 32K windows, by edges inside H.  Two vertices of U: both are sources
    # of H already, (2, 2).  U[0] and a new vertex right behind V, H's last source: the new
    # source takes one entry, two at 32K, (2, 3).  U[0] and a new vertex 10 past the last:
    # a jump at both sizes, (3, 3).
    h14, h15 = lens(14)[4], lens(15)[2]
    q = (h14 - h15) % SEG
    t = (1 - h14 - 2 * q) % SEG
    r = t % 2
    p = (t - 3 * r) % SEG // 2
    uu = np.array([(a, b) for i, a in enumerate(U) for b in U[i + 1:]])[:p].reshape(-1, 2)
    pairs.append(uu)
    pairs.append(_block(U[:1], V[-1] + 1 + np.arange(q)))
    pairs.append(_block(U[:1], V[-1] + q + 10 * (1 + np.arange(r))))

    s, d = graph()
    assert s.max() < 81920 and 20_000 < s.size < 100_000
    for wb in WBS:
        pmax = (1 << wb) - 1
        L = lens(wb)
        w, D, first = _window_entries(s, d, wb)
        assert (D[~first] > 2 * pmax).any()                    # several jumps before one entry
        assert (D[first] > pmax).any()                         # jumps at a window start
        assert (L[1:-1] == 0).any() and L[0] > 0 and L[-1] > 0  # a window without an entry
        assert ((L > 0) & (L % SEG == 0)).any() and (L % SEG == 1).any()  # pad 0 and pad 511
        assert (L > UNIT).any()                                # two units
        assert stream_length(s, d, wb) <= s.size + s.size // 2  # it packs
    return s, d


def test_stream_graph_properties():
    _stream_graph()


def _run(s, d, options, symmetric=True, vdtype=np.int32):
    """(vertices, rank bits, iterations), stream entries of the schedule"""
    h, G = make_graph(s, d, None, transposed=True, renumber=False, symmetric=symmetric, vdtype=vdtype,
                      options=dict(options, pr_perm=0, pr_runs=0))
    v, r = plc().pagerank(h, G, None, None, None, None, 0.85, 1e-6, 500, False)
    return (host(v), host(r).view(np.uint32), h.last_iterations()), h.last_pagerank_schedule()[0]


def _same(got, want):
    assert got[2] == want[2] > 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@functools.lru_cache(maxsize=None)
def _oracle(directed):
    s, d = _directed_graph() if directed else _stream_graph()
    return opr.pagerank(int(max(s.max(), d.max())) + 1, s, d, None, 0.85, 1e-6, 500)


def _close(out, ref):
    assert out[0].size == ref.size
    got = np.zeros(ref.size)
    got[out[0]] = out[1].view(np.float32)
    assert (np.abs(got - ref) / ref).max() < REL


@pytest.mark.gpu
@pytest.mark.parametrize("wb", WBS)
def test_stream_of_both_builders(wb):
    s, d = _stream_graph()
    want = stream_length(s, d, wb)
    fast, n_fast = _run(s, d, {"pr_win_bits": wb, "pr_fast_build": 1})
    general, n_general = _run(s, d, {"pr_win_bits": wb, "pr_fast_build": 0})
    plain, n_plain = _run(s, d, {"pr_win_bits": wb, "pr_packed": 0})
    print(f"wb {wb}: stream {want} by definition, fast build {n_fast}, general build {n_general}")
    assert n_fast == want and n_general == want and n_plain == 0
    _same(general, fast)
    _same(plain, fast)
    _close(fast, _oracle(False))


@functools.lru_cache(maxsize=None)
def _directed_graph():
    """The stream graph without one direction of every 97th edge."""
    s, d = _stream_graph()
    keep = np.arange(s.size) % 97 != 0
    return s[keep], d[keep]


@pytest.mark.gpu
@pytest.mark.parametrize("wb", WBS)
def test_stream_of_a_directed_graph(wb):
    s, d = _directed_graph()
    want = stream_length(s, d, wb)
    assert want <= s.size + s.size // 2
    out, n = _run(s, d, {"pr_win_bits": wb}, symmetric=False)
    print(f"wb {wb}: stream {want} by definition, general build {n}")
    assert n == want
    plain, n_plain = _run(s, d, {"pr_win_bits": wb, "pr_packed": 0}, symmetric=False)
    assert n_plain == 0
    _same(plain, out)
    _close(out, _oracle(True))


@pytest.mark.gpu
@pytest.mark.parametrize("wb", WBS)
def test_stream_of_64_bit_ids(wb):
    s, d = _stream_graph()
    want = stream_length(s, d, wb)
    i32, n32 = _run(s, d, {"pr_win_bits": wb})
    i64, n64 = _run(s, d, {"pr_win_bits": wb}, vdtype=np.int64)
    print(f"wb {wb}: stream {want} by definition, int32 ids {n32}, int64 ids {n64}")
    assert n32 == want and n64 == want
    assert i64[2] == i32[2] > 0
    assert np.array_equal(i64[0].astype(np.int64), i32[0].astype(np.int64)) and np.array_equal(i64[1], i32[1])


@pytest.mark.gpu
def test_stream_that_does_not_pack():
    """200 vertices, 20 ids apart, each joined to the vertex 60,000 past it, at 4K windows:
    every entry's source lies more than dmax = 14 past the one before, so every entry takes
    a jump, the stream would be twice the entries (more than 1.5 x) and both builders fall
    back to 32-bit entries."""
    v = 20 * np.arange(200)
    s, d = _symmetric(v, v + 60000)
    assert s.size == 400
    assert stream_windows(s, d, 12).sum() >= 2 * s.size > s.size + s.size // 2
    plain, n_plain = _run(s, d, {"pr_win_bits": 12, "pr_packed": 0})
    for fast in (1, 0):
        out, n = _run(s, d, {"pr_win_bits": 12, "pr_fast_build": fast})
        assert n == 0 == n_plain
        _same(out, plain)
