"""The facts tests/test_gpu_bfs_cases.py relies on, held on the CPU: an edit of the
builder in tests/bfs_cases.py that empties one of them fails here, not silently there."""
import numpy as np
import pytest

import bfs_cases as bc
from oracle import bfs as obfs

G = bc.case_graph()


one_source, several_sources = bc.one_source, bc.several_sources


def test_vertex_count_fills_no_word_or_wave():
    for name in ("renumbered", "identity", "permuted", "wide64"):
        nv = bc.view(name).nv
        assert nv % 64 != 0 and nv % 32 != 0, (name, nv)
    assert bc.view("permuted").nv == G.nv + 1


@pytest.mark.parametrize("name", ["renumbered", "identity", "permuted", "wide64"])
def test_deep_and_connected(name):
    V = bc.view(name)
    dist, _ = bc.expected(V, one_source(V))
    assert bc.eccentricity(V, one_source(V)) >= 40
    assert np.array_equal(dist != V.inf, V.degrees() > 0)
    assert int((V.degrees() == 0).sum()) == (1 if name == "permuted" else 0)


def test_external_ids_are_not_the_internal_ones():
    R, W, I = bc.view("renumbered"), bc.view("wide64"), bc.view("identity")
    assert R.ids.min() == 7 and not np.any(R.ids == np.arange(R.nv))
    assert W.ids.min() > 2**32 and np.array_equal((W.ids - (1 << 33)) // 1_000_003, (R.ids - 7) // 3)
    # identity: the same rows under the same numbering, and degrees never increase with the id
    assert np.array_equal(I.csr.offsets, R.csr.offsets) and np.array_equal(I.csr.indices, R.csr.indices)
    assert np.all(np.diff(I.degrees()) <= 0)
    assert np.any(np.diff(bc.view("permuted").degrees()) > 0)


@pytest.mark.parametrize("name", ["renumbered", "identity", "permuted", "wide64"])
def test_hubs_have_their_degrees(name):
    V = bc.view(name)
    deg = V.degrees()
    for want, (hub, leaf) in G.hubs.items():
        assert deg[V.internal(hub)] == want and deg[V.internal(leaf)] == 1
    assert deg.max() == 4100


@pytest.mark.parametrize("name", ["renumbered", "identity", "wide64"])
def test_fans_put_the_parent_at_position_k(name):
    V = bc.view(name)
    pos, deg = bc.parent_position(V, one_source(V)), V.degrees()
    dist, pred = bc.expected(V, one_source(V))
    assert len(G.fans) == len(bc.FAN_K) * len(bc.FAN_J) == 57
    at = {int(dist[V.internal(t)]) for _, _, _, t in G.fans}
    assert len(at) == 1  # every fan is discovered in one level
    for k, j, p, t in G.fans:
        i = V.internal(t)
        assert pos[i] == k and deg[i] == k + 1 + j, (k, j, pos[i], deg[i])
        assert pred[i] == V.ext(p)
        assert V.csr.indices[V.csr.offsets[i] + k] == V.internal(p)


def test_permuted_hits_later_rounds_of_every_lane_width():
    V = bc.view("permuted")
    pos, deg = bc.parent_position(V, one_source(V)), V.degrees()
    for w, lo, hi in bc.BU_BINS:
        assert np.any((deg >= lo) & (deg <= hi) & (pos >= w)), w


def test_parent_position_is_the_oracles_predecessor():
    for name in ("renumbered", "permuted"):
        V = bc.view(name)
        for src in (one_source(V), several_sources(V)):
            pos = bc.parent_position(V, src)
            dist, pred = bc.expected(V, src)
            got = np.flatnonzero(pos >= 0)
            assert np.array_equal(pos >= 0, (dist != V.inf) & (dist > 0))
            assert np.array_equal(V.ids[V.csr.indices[V.csr.offsets[got] + pos[got]]], pred[got])


@pytest.mark.parametrize("name", ["renumbered", "permuted", "wide64", "directed"])
@pytest.mark.parametrize("several", [False, True])
def test_truncation_rule_is_the_oracles_depth_limit(name, several):
    V = bc.view(name)
    src = several_sources(V) if several else one_source(V)
    ecc = bc.eccentricity(V, src)
    si = V.internal_of_ext(np.asarray(src))
    for L in (1, 2, 3, 7, ecc, ecc + 1, ecc + 5):
        rd, rp = obfs.bfs(V.nv, V.csr.offsets, V.csr.indices, si, L, invalid_distance=V.inf)
        ed, ep = bc.expected(V, src, L)
        assert np.array_equal(ed, rd)
        assert np.array_equal(ep, np.where(rp >= 0, V.ids[np.maximum(rp, 0)], -1))
        assert ed[ed != V.inf].max() == min(L, ecc)


def test_directed_view_is_deep_and_partly_unreachable():
    V = bc.view("directed")
    assert not V.symmetric and V.nv == G.nchain
    for src in (one_source(V), several_sources(V)):
        assert bc.eccentricity(V, src) >= 10
    assert np.any(bc.expected(V, one_source(V))[0] == V.inf)
    s, d = V.src, V.dst
    assert not np.any(np.isin(s * (1 << 32) + d, d * (1 << 32) + s))  # no edge in both directions


def test_expected_leaves_its_reference_unchanged():
    V = bc.view("renumbered")
    a, _ = bc.expected(V, one_source(V))
    a[:] = 0
    b, _ = bc.expected(V, one_source(V), 3)
    assert b.max() == V.inf and bc.expected(V, one_source(V))[0].max() == bc.eccentricity(V, one_source(V))


@pytest.mark.parametrize("name", ["renumbered", "identity", "permuted"])
def test_schedules_differ_by_their_counters(name):
    """(levels, bottom-up levels) as bfs_impl counts them, from the oracle's level sizes."""
    V = bc.view(name)
    src = one_source(V)
    ecc = bc.eccentricity(V, src)
    dirs = {s: bc.level_directions(V, src, s) for s in bc.SCHEDULES}
    dirs["top-down only"] = bc.level_directions(V, src, "default", direction_optimizing=False)
    assert all(len(x) == ecc + 1 for x in dirs.values())
    assert len({x.count("B") for x in dirs.values()}) == len(dirs)
    assert dirs["all_bu"] == "B" * (ecc + 1) and dirs["top-down only"] == "T" * (ecc + 1)
    assert dirs["flip"].count("BT") >= 5 and dirs["flip"].count("TB") >= 5
    assert dirs["flip"].startswith("BBBTTBBBTT")
    assert dirs["never"] == "T" * ecc + "B"  # m_u = 0 at the last level: m_f > m_u / alpha
    assert "BBBB" in dirs["mixed"] and "BBBB" not in dirs["flip"]
    # the queue start needs sources x 4100 <= (E - that) / alpha
    assert not bc.queue_start(V, src, "default") and not bc.queue_start(V, src, "all_bu")
    assert bc.queue_start(V, src, "never") == (name != "permuted")


@pytest.mark.parametrize("schedule", ["flip", "mixed"])
def test_limits_cut_every_kind_of_level(schedule):
    """Over the limits 1..ecc + 2 the loop ends after the first level of a bottom-up
    phase, after either level launched with it, after a top-down level and after the
    level launched with that one: (the last two directions run, the direction that
    would have followed)."""
    V = bc.view("renumbered")
    src = one_source(V)
    full = bc.level_directions(V, src, schedule)
    ends = set()
    for limit in range(1, len(full) + 2):
        dirs = bc.level_directions(V, src, schedule, limit)
        assert len(dirs) == min(limit, len(full)) and dirs == full[:len(dirs)]
        ends.add((dirs[-2:], full[len(dirs):len(dirs) + 1]))
    assert {("B", "B"), ("TB", "B"), ("BB", "B"), ("BB", "T"), ("BT", "T"), ("TT", "B")} <= ends


def test_fans_are_discovered_by_a_bottom_up_level():
    V = bc.view("renumbered")
    src = one_source(V)
    level = int(bc.expected(V, src)[0][V.internal(G.fans[0][3])])
    for schedule in ("all_bu", "flip"):
        assert bc.level_directions(V, src, schedule)[level - 1] == "B"


def test_ring_fills_the_last_residual_sub_queue_past_the_vertex_count():
    """k_bu_probe appends the misses of chunk c (64 vertices) to sub-queue c % 16, which
    starts at entry (c % 16) * residual_cap(V) of the residual array.  On the ring, level
    0 runs top-down from the queues -- the one kind of level after which bfs_impl swaps
    its two queue sets -- and level 1 bottom-up with every vertex of chunk 15 a miss: the
    entries 15 * cap .. 15 * cap + 63 are written, all past V, in the array that was the
    other queue set's before the swap."""
    V = bc.view("ring")
    nv, deg = V.nv, V.degrees()
    assert nv == bc.RING_NV and np.all(deg == 2 * bc.RING_HALF)
    chunks = (nv + 63) // 64
    cap = (chunks + 15) // 16 * 64  # residual_cap() of csrc/bfs.hip
    assert 15 * cap >= nv and chunks > 15
    src = (0,)
    assert bc.queue_start(V, src, bc.RING_SCHEDULE)
    dirs = bc.level_directions(V, src, bc.RING_SCHEDULE)
    assert dirs.startswith("TBBB")
    dist, _ = bc.expected(V, src)
    chunk15 = np.arange(15 * 64, 16 * 64)
    assert np.all(dist[chunk15] > 2)  # unvisited at level 1 and no neighbour in its frontier
    # more entries than any probe form covers: 3 + 8 with the head table, 8 without, 3 alone
    assert deg.min() > 11
