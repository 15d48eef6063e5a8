"""BFS on the case graph of tests/bfs_cases.py under forced direction schedules, at every
depth limit, with every probe form, id width, grid size and kind of source.  Every
comparison is exact equality with the oracle (bfs_cases.expected / check_result); the
level and bottom-up counters must be those bfs_cases.level_directions works out on the
CPU.

The schedules (options bfs_alpha / bfs_beta), with the level log (CGX_BFS_DEBUG) of the
chain's source on every symmetric view, T top-down, B bottom-up, 53 levels each:

 default  TTTTTTTTBBBTTBBBTTTTTTBBBTTBBBTTBBBTTTTBBBTTBBBTTBBBT  (bitmap start: one source
          of 4100 edges would be above the rule; a hub in the frontier sends it
          bottom-up, always for the three levels launched together, and the small chain
          frontiers send it back)
 all_bu   53 x B  (bitmap start)
 flip     BBBTT x 10, BBB  (a bottom-up level and its two speculated successors, a
          top-down level and its speculated successor: ten switches of each kind)
 mixed    BBBTTBBBTTBBBTTBBBBTTBBBTTBBBTTBBBBTTBBBBTTBBBBTTBBBT  (as flip, but a fourth
          bottom-up level wherever the third one found a hub's leaves)
 never    52 x T, B  (queue start on the views in degree order; the last level has no unexplored edge left, m_u = 0, and the rule
          m_f > m_u / alpha then says bottom-up whatever alpha is; it finds nothing)
"""
import functools

import numpy as np
import pytest

import bfs_cases as bc
from gpu_util import host, make_graph, plc

pytestmark = pytest.mark.gpu

G = bc.case_graph()
SCHEDULE_NAMES = tuple(bc.SCHEDULES)


@functools.lru_cache(maxsize=None)
def _graph(view, options):
    V = bc.view(view)
    return make_graph(V.src.copy(), V.dst.copy(), None, renumber=V.renumber, symmetric=V.symmetric, vdtype=V.vdtype,
                      options=dict(options))


def graph(view, schedule=None, **options):
    """(handle, graph) of a view, built once per set of options."""
    opts = dict(bc.schedule_options(schedule)) if schedule else {}
    opts.update(options)
    return _graph(view, tuple(sorted(opts.items())))


def run(h, g, V, sources, do, limit=None, pred=True):
    d, p, v = plc().bfs(h, g, np.asarray(sources, V.vdtype), do, limit or 0, pred, False)
    v, d, p = host(v), host(d), host(p)
    assert v.dtype == d.dtype == p.dtype == V.vdtype
    return v, d, p


def run_check(view, schedule, sources, limit=None, pred=True, **options):
    """One traversal against the oracle and the CPU's level directions; schedule None:
    top-down only."""
    V = bc.view(view)
    h, g = graph(view, schedule, **options)
    v, d, p = run(h, g, V, sources, schedule is not None, limit, pred)
    if not pred:
        assert p.size == 0
    bc.check_result(V, v, d, p if pred else None, sources, limit)
    dirs = bc.level_directions(V, sources, schedule or "default", limit, schedule is not None)
    assert (h.last_bfs_levels(), h.last_bfs_bottom_up_steps()) == (len(dirs), dirs.count("B")), (limit, dirs)
    return h, dirs


def level_log(capfd):
    err = capfd.readouterr().err
    return "".join({"top-down": "T", "bottom-up": "B"}[ln.split()[3]] for ln in err.splitlines()
                   if ln.startswith("[bfs] level"))


# ---- 1. schedules

@pytest.mark.parametrize("view", ["renumbered", "identity", "permuted"])
@pytest.mark.parametrize("schedule", SCHEDULE_NAMES + (None,))
def test_schedule_equals_oracle(view, schedule):
    V = bc.view(view)
    src = bc.one_source(V)
    h, dirs = run_check(view, schedule, src)
    assert h.last_bfs_levels() == bc.eccentricity(V, src) + 1
    if schedule == "all_bu":
        assert h.last_bfs_bottom_up_steps() == h.last_bfs_levels()
    if schedule in ("flip", "mixed", "default"):
        assert 0 < h.last_bfs_bottom_up_steps() < h.last_bfs_levels()
    if schedule is None:
        assert h.last_bfs_bottom_up_steps() == 0


@pytest.mark.parametrize("view", ["renumbered", "permuted"])
@pytest.mark.parametrize("schedule", SCHEDULE_NAMES)
def test_level_log_is_the_schedule(view, schedule, monkeypatch, capfd):
    """The level log shows the directions of the module docstring, level by level, and
    flip switches at least five times each way."""
    V = bc.view(view)
    src = bc.one_source(V)
    h, g = graph(view, schedule)
    monkeypatch.setenv("CGX_BFS_DEBUG", "1")
    capfd.readouterr()
    run(h, g, V, src, True)
    log = level_log(capfd)
    assert log == bc.level_directions(V, src, schedule)
    assert len(log) == h.last_bfs_levels() and log.count("B") == h.last_bfs_bottom_up_steps()
    if schedule == "flip":
        assert log.count("BT") >= 5 and log.count("TB") >= 5


# ---- 2. every depth limit

@pytest.mark.parametrize("view", ["renumbered", "permuted"])
@pytest.mark.parametrize("schedule", ["flip", "mixed", "all_bu", "default"])
def test_every_depth_limit(view, schedule):
    """A limit ends the loop after a bottom-up level, after either speculated bottom-up
    level, after a top-down level and after either level of a speculated top-down pair:
    each leaves the last top-down level's predecessors to another line of bfs_impl
    (tests/test_bfs_cases_host.py: the limits 1..ecc + 2 do cut at each of these)."""
    V = bc.view(view)
    src = bc.one_source(V)
    ecc = bc.eccentricity(V, src)
    for limit in range(1, ecc + 3):
        h, _ = run_check(view, schedule, src, limit)
        assert h.last_bfs_levels() == min(limit, ecc + 1)


# ---- 3. probe forms on the fans

FAN_LEVEL = int(bc.expected(bc.view("renumbered"), bc.one_source(bc.view("renumbered")))[0][
    bc.view("renumbered").internal(G.fans[0][3])])


@pytest.mark.parametrize("view", ["renumbered", "identity"])
@pytest.mark.parametrize("schedule", ["all_bu", "flip"])
@pytest.mark.parametrize("head,vec", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_probe_forms_on_the_fans(view, schedule, head, vec):
    """Parents at positions 0..2050 of rows of 1..2056 entries, on each side of every
    hand-over: head table -> 16-byte stage at 3, -> residual at 11 (at 3 without the
    stage, at 8 without the head table), the residual's 16-lane rounds from there."""
    V = bc.view(view)
    src = bc.one_source(V)
    opts = {k: v for k, v in (("bfs_head", head), ("bfs_probe_vec", vec)) if v == 0}
    dirs = bc.level_directions(V, src, schedule)
    assert dirs[FAN_LEVEL - 1] == "B"  # the level that discovers the fans' t runs bottom-up
    for limit in (None, FAN_LEVEL - 1, FAN_LEVEL, FAN_LEVEL + 1):
        run_check(view, schedule, src, limit, **opts)


# ---- 4. int64 ids

@pytest.mark.parametrize("schedule", ["all_bu", "flip", "never"])
@pytest.mark.parametrize("pred", [True, False])
def test_int64_ids(schedule, pred):
    V = bc.view("wide64")
    assert V.inf == np.iinfo(np.int64).max and V.ids.min() >= 2**33 > V.nv
    for src in (bc.one_source(V), bc.several_sources(V)):
        run_check("wide64", schedule, src, pred=pred)
    run_check("wide64", schedule, bc.one_source(V), FAN_LEVEL, pred=pred)


# ---- 5. one-block grids

@pytest.mark.parametrize("view", ["renumbered", "permuted"])
@pytest.mark.parametrize("schedule", ["flip", "default", "never"])
def test_one_block_grids(view, schedule):
    """Every top-down segment, the probe and the residual on one block: the grid-stride
    loops, the large class walking the chunks of several rows in one block (default and
    never run the level whose frontier holds the six fans above 1024 edges top-down, and
    never the four hubs that are sources)."""
    V = bc.view(view)
    one = {"bfs_td_cap": 1, "bfs_res_grid": 1, "bfs_probe_grid": 1}
    hubs = tuple(int(x) for x in V.ext([G.hubs[d][0] for d in (1025, 2048, 2049, 4100)]))
    for src in (bc.one_source(V), bc.several_sources(V), hubs):
        run_check(view, schedule, src, **one)


# ---- 6. no predecessors

@pytest.mark.parametrize("schedule", ["flip", "never"])
def test_no_predecessors(schedule):
    V = bc.view("renumbered")
    for src in (bc.one_source(V), bc.several_sources(V)):
        run_check("renumbered", schedule, src, pred=False)
    run_check("renumbered", schedule, bc.one_source(V), 7, pred=False)


# ---- 7. sources

def source_sets(V):
    rng = np.random.default_rng(9)
    hub, leaf = G.hubs[4100]
    many = rng.integers(0, G.nv, 1500)
    assert np.unique(many).size < many.size
    sets = {"hub4100": [hub], "leaf": [leaf],
            "mixed": [G.hubs[2049][0], leaf, 7 * bc.BLOCK + 1, leaf, G.source, G.hubs[2049][0], 23 * bc.BLOCK],
            "many": many}
    if V.name == "permuted":
        sets["isolated"] = [bc.isolated_raw()]
    return {k: tuple(int(x) for x in V.ext(v)) for k, v in sets.items()}


SOURCE_CASES = [(v, w) for v in ("renumbered", "permuted") for w in ("hub4100", "leaf", "mixed", "many")]
SOURCE_CASES.append(("permuted", "isolated"))  # (renumbering keeps no isolated id)


@pytest.mark.parametrize("view,which", SOURCE_CASES)
@pytest.mark.parametrize("schedule", ["default", "all_bu", "flip"])
def test_sources(view, schedule, which):
    """A 4100-edge hub (a bitmap start on a frontier of one large row), a pendant leaf,
    the isolated id, a list with duplicates, and 1500 ids with duplicates (above the
    1024 ids of the wave lookup of graph_build.hip)."""
    V = bc.view(view)
    src = source_sets(V)[which]
    h, dirs = run_check(view, schedule, src)
    if which == "isolated":
        v, d, p = run(h, graph(view, schedule)[1], V, src, True)
        assert dirs == "T" and h.last_bfs_levels() == 1
        assert np.flatnonzero(d != V.inf).tolist() == [V.internal(bc.isolated_raw())] and np.all(p == -1)


@pytest.mark.parametrize("which", ["hub4100", "mixed", "many"])
def test_sources_into_the_queues(which):
    """The same sources where bfs_impl puts them straight into the class queues: level 0
    expands the 4100-edge row in the large class.  Top-down only does so for any number
    of sources; never while sources x 4100 <= (E - that) / alpha, which 1500 are not."""
    V = bc.view("renumbered")
    src = source_sets(V)[which]
    assert bc.queue_start(V, src, "default", direction_optimizing=False)
    assert bc.queue_start(V, src, "never") == (which != "many")
    run_check("renumbered", "never", src)
    run_check("renumbered", None, src)


# ---- 8. an invalid source among valid ones

@pytest.mark.parametrize("schedule", ["default", "never", "all_bu"])
@pytest.mark.parametrize("bad", ["between", "negative", "above"])
def test_invalid_source_among_valid_ones(schedule, bad):
    """never: the sources go straight to the queues and the check comes back with level
    0's counters; default and all_bu: bitmap start, the check is read before level 0 (on
    this graph default's rule asks for sources x 4100 <= (E - that) / 40: none)."""
    V = bc.view("renumbered")
    h, g = graph("renumbered", schedule)
    good = bc.several_sources(V)
    wrong = {"between": int(V.ext(G.q)) + 1, "negative": -5, "above": int(V.ids.max()) + 1}[bad]
    assert wrong not in V.ids
    for srcs in ([wrong], list(good[:2]) + [wrong] + list(good[2:])):
        assert bc.queue_start(V, srcs, schedule) == (schedule == "never")
        with pytest.raises(ValueError):
            run(h, g, V, srcs, True)
        v, d, p = run(h, g, V, good, True)
        bc.check_result(V, v, d, p, good)
    bc.check_vs_oracle(V.src, V.dst, v, d, p, good)


# ---- the residual queue after a swap of the queue sets

@pytest.mark.parametrize("head,vec", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_ring_residual_after_queue_swap(head, vec):
    """tests/test_bfs_cases_host.py: after the top-down level 0 the probe of level 1
    gets the queue array that level 0 read, and fills the residual sub-queue of chunk
    15 past entry V of it -- the array must have room for every sub-queue."""
    V = bc.view("ring")
    opts = {k: v for k, v in (("bfs_head", head), ("bfs_probe_vec", vec)) if v == 0}
    for limit in (None, 2, 3):
        run_check("ring", bc.RING_SCHEDULE, (0,), limit, **opts)
    run_check("ring", bc.RING_SCHEDULE, (0, 500, 501), **opts)


# ---- 9. directed, top-down

@pytest.mark.parametrize("several", [False, True])
def test_directed_top_down(several):
    V = bc.view("directed")
    src = bc.several_sources(V) if several else bc.one_source(V)
    ecc = bc.eccentricity(V, src)
    h, _ = run_check("directed", None, src)
    assert h.last_bfs_levels() == ecc + 1
    for limit in range(1, ecc + 2):
        h, _ = run_check("directed", None, src, limit)
        assert h.last_bfs_levels() == min(limit, ecc + 1)
