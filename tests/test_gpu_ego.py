"""Induced subgraphs and ego nets on the GPU (csrc/subgraph.hip through the C ABI and the Python layers)
against the CPU twin (tests/ego_ref.py, itself checked against networkx in tests/test_ego_api.py) or
networkx itself.

Every comparison is exact.  same() compares the offsets entry by entry and every subgraph as its sorted
(src, dst, weight bits) rows; same_bytes() compares two results array by array, order included.

The closed forms sit on the paths of the kernels: rows of 63 / 64 / 65 entries around the thread / wave
cut, member lists of kIsectStageLen - 1 .. + 1 vertices (1024 4-byte ids, 512 8-byte ids) around the LDS
stage, a hub row cut into segments with sg_split_min set low, hits on both sides of a 64-entry step."""
import functools
import os

import numpy as np
import pytest

from conftest import dataset_path
from ego_ref import Rows, batched, ego_vertices
from gpu_util import host, make_graph, plc

pytestmark = pytest.mark.gpu

DATASETS = {"karate.csv": False, "dolphins.csv": False, "polbooks.csv": False, "netscience.csv": False,
            "email-Eu-core.csv": False, "karate-asymmetric.csv": True}


# ------------------------------------------------------------------ helpers
def edge_weight(s, d, copy=None):
    """A weight that tells every stored edge apart, exact in float32."""
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    c = np.zeros(len(s), np.int64) if copy is None else np.asarray(copy, np.int64)
    return 0.5 + ((s * 31 + d * 17 + c * 5) % 4093) / 8.0


def bits(w):
    return w.view(np.uint32 if w.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


def canon(s, d, w):
    """The rows (src, dst, weight bits) of one subgraph, sorted."""
    cols = [np.asarray(s).astype(np.int64), np.asarray(d).astype(np.int64)]
    cols.append(np.zeros(len(cols[0]), np.int64) if w is None else bits(np.asarray(w)).astype(np.int64))
    a = np.stack(cols, axis=1)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def same(result, want, vdtype=np.int32, wdtype=None):
    """result: the four device arrays; want: the twin's (src, dst, w or None, offsets)."""
    src, dst, w, off = result
    s, d, o = host(src), host(dst), host(off)
    ws, wd, ww, wo = want
    assert s.dtype == np.dtype(vdtype) and d.dtype == s.dtype and o.dtype == np.int64
    assert o.tolist() == wo.tolist() and len(s) == len(d) == int(wo[-1])
    if ww is None:
        assert w is None
    else:
        assert w is not None and host(w).dtype == np.dtype(wdtype) and len(host(w)) == len(s)
    hw = None if w is None else host(w)
    for i in range(len(wo) - 1):
        a, b = int(wo[i]), int(wo[i + 1])
        got = canon(s[a:b], d[a:b], None if hw is None else hw[a:b])
        exp = canon(ws[a:b], wd[a:b], None if ww is None else np.asarray(ww[a:b], wdtype))
        assert np.array_equal(got, exp), f"subgraph {i}"


def same_bytes(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            hx, hy = host(x), host(y)
            assert hx.dtype == hy.dtype and hx.tobytes() == hy.tobytes()


def ego(h, g, seeds, radius, vdtype=np.int32):
    return plc().ego_graph(h, g, np.asarray(seeds, vdtype), radius, False)


def induced(h, g, sets, vdtype=np.int32):
    off = np.zeros(len(sets) + 1, np.int64)
    np.cumsum([len(x) for x in sets], out=off[1:])
    flat = np.concatenate([np.asarray(x, vdtype) for x in sets]) if sets else np.zeros(0, vdtype)
    return plc().induced_subgraph(h, g, flat.astype(vdtype), off, False)


def twin_ego(s, d, w, seeds, radius):
    rows = Rows(s, d)
    return batched(s, d, w, [ego_vertices(rows, x, radius) for x in seeds])


@functools.lru_cache(maxsize=None)
def dataset(name):
    """The stored edges of a golden file: an undirected one both ways, every pair once, a loop once."""
    data = np.loadtxt(dataset_path(name), dtype=np.float64, ndmin=2)
    e = np.unique(data[:, :2].astype(np.int64), axis=0)
    if not DATASETS[name]:
        e = np.unique(np.concatenate([e, e[:, ::-1]]), axis=0)
    return e[:, 0].copy(), e[:, 1].copy()


def seeds_of(s, d, count, rng_seed=0):
    ids = np.unique(np.r_[s, d])
    rng = np.random.default_rng(rng_seed)
    return rng.choice(ids, size=count, replace=count > len(ids))


# ------------------------------------------------------------------ 1. datasets
@functools.lru_cache(maxsize=None)
def dataset_twin(name, radius):
    s, d = dataset(name)
    seeds = seeds_of(s, d, 6, rng_seed=len(s))
    return seeds, twin_ego(s, d, edge_weight(s, d).astype(np.float32), seeds, radius)


@pytest.mark.parametrize("radius", [0, 1, 2, 3])
@pytest.mark.parametrize("name", sorted(DATASETS))
def test_datasets_ego(name, radius):
    s, d = dataset(name)
    seeds, want = dataset_twin(name, radius)
    h, g = make_graph(s, d, edge_weight(s, d), symmetric=not DATASETS[name])
    same(ego(h, g, seeds, radius), want, wdtype=np.float32)


@pytest.mark.parametrize("name", sorted(DATASETS))
def test_datasets_induced(name):
    s, d = dataset(name)
    ids = np.unique(np.r_[s, d])
    rng = np.random.default_rng(len(ids))
    sets = [rng.choice(ids, size=k, replace=False) for k in (1, len(ids) // 5, 0, len(ids) // 2, len(ids))]
    w = edge_weight(s, d).astype(np.float32)
    h, g = make_graph(s, d, w, symmetric=not DATASETS[name])
    same(induced(h, g, sets), batched(s, d, w, sets), wdtype=np.float32)


# ------------------------------------------------------------------ 2. order, input order, duplicates
def test_output_order_and_determinism():
    s, d = dataset("email-Eu-core.csv")
    h, g = make_graph(s, d, None, symmetric=True, renumber=False)
    seeds = seeds_of(s, d, 12)
    a = ego(h, g, seeds, 2)
    b = ego(h, g, seeds, 2)
    same_bytes(a, b)
    src, dst, _, off = (host(x) for x in (a[0], a[1], a[0], a[3]))
    for i in range(len(seeds)):
        lo, hi = int(off[i]), int(off[i + 1])
        key = src[lo:hi].astype(np.int64) * 2**32 + dst[lo:hi]
        assert hi > lo and np.all(np.diff(key) > 0), f"subgraph {i} does not ascend by (source, destination)"
    same(a, twin_ego(s, d, None, seeds, 2))


@pytest.mark.parametrize("renumber", [True, False])
def test_shuffled_sets_and_duplicate_seeds(renumber):
    s, d = dataset("polbooks.csv")
    w = edge_weight(s, d).astype(np.float32)
    h, g = make_graph(s, d, w, symmetric=True, renumber=renumber)
    ids = np.unique(np.r_[s, d])
    rng = np.random.default_rng(5)
    sets = [np.sort(rng.choice(ids, size=k, replace=False)) for k in (40, 3, 70)]
    a = induced(h, g, sets)
    b = induced(h, g, [rng.permutation(x) for x in sets])
    c = induced(h, g, [x[::-1] for x in sets])
    same_bytes(a, b)
    same_bytes(a, c)
    same(a, batched(s, d, w, sets), wdtype=np.float32)
    # the same set twice is two subgraphs; a seed given three times is three
    same(induced(h, g, [sets[0], sets[0]]), batched(s, d, w, [sets[0], sets[0]]), wdtype=np.float32)
    seeds = [int(ids[3]), int(ids[9]), int(ids[3]), int(ids[3])]
    r = ego(h, g, seeds, 2)
    same(r, twin_ego(s, d, w, seeds, 2), wdtype=np.float32)
    src, dst, wt, off = (host(x) for x in r)
    first = slice(int(off[0]), int(off[1]))
    for k in (2, 3):
        again = slice(int(off[k]), int(off[k + 1]))
        assert src[first].tobytes() == src[again].tobytes() and dst[first].tobytes() == dst[again].tobytes()
        assert wt[first].tobytes() == wt[again].tobytes()


# ------------------------------------------------------------------ 3. edge cases
def small_graph():
    """The path 0 -> 1 -> 2 -> 3 -> 4 with a loop on 2, vertex 5 with only a self-loop, vertex 6 without
    any edge (an id of a graph that is not renumbered, unknown to one that is), and the pair 7 <-> 8."""
    s = [0, 1, 2, 3, 5, 2, 7, 8]
    d = [1, 2, 3, 4, 5, 2, 8, 7]
    return np.asarray(s, np.int64), np.asarray(d, np.int64)


def test_edge_cases():
    s, d = small_graph()
    w = edge_weight(s, d).astype(np.float32)
    h, g = make_graph(s, d, w, renumber=False)
    for radius in (0, 1, 2, 50):
        # 6 is isolated, 5 has only its loop, 4 is a sink, 0 starts the path
        seeds = [6, 5, 4, 0, 2, 7]
        same(ego(h, g, seeds, radius), twin_ego(s, d, w, seeds, radius), wdtype=np.float32)
    src, dst, wt, off = ego(h, g, [5, 2, 0], 0)
    assert host(src).tolist() == [5, 2] and host(dst).tolist() == [5, 2] and host(off).tolist() == [0, 1, 2, 2]
    # beyond the diameter: the whole reachable set, no more
    src, dst, _, off = ego(h, g, [0], 10**6)
    assert sorted(zip(host(src).tolist(), host(dst).tolist())) == [(0, 1), (1, 2), (2, 2), (2, 3), (3, 4)]
    # no seeds; no sets; an empty set between two others
    src, dst, wt, off = ego(h, g, [], 2)
    assert len(host(src)) == 0 and len(host(dst)) == 0 and len(host(wt)) == 0 and host(off).tolist() == [0]
    src, dst, wt, off = induced(h, g, [])
    assert len(host(src)) == 0 and host(off).tolist() == [0] and host(off).dtype == np.int64
    sets = [[2, 1, 3], [], [8, 7, 5]]
    r = induced(h, g, sets)
    same(r, batched(s, d, w, sets), wdtype=np.float32)
    assert host(r[3]).tolist() == [0, 3, 3, 6]
    same(induced(h, g, [[], []]), batched(s, d, w, [[], []]), wdtype=np.float32)


def test_errors():
    s, d = small_graph()
    h, g = make_graph(s, d, None, renumber=True)
    p = plc()
    ok = np.asarray([2, 1, 3, 8], np.int32)
    for off in ([1, 2, 4], [0, 3, 2], [0, 2, 3], [0, 2, 5], [0, 5]):
        with pytest.raises(ValueError, match="subgraph_offsets"):
            p.induced_subgraph(h, g, ok, np.asarray(off, np.int64), False)
    with pytest.raises(ValueError, match="subgraph_offsets"):
        p.induced_subgraph(h, g, ok, np.zeros(0, np.int64), False)
    for check in (False, True):
        with pytest.raises(ValueError, match="repeated"):
            p.induced_subgraph(h, g, np.asarray([2, 1, 2, 8], np.int32), np.asarray([0, 3, 4], np.int64), check)
        with pytest.raises(ValueError, match="not in the graph"):
            p.induced_subgraph(h, g, np.asarray([2, 6, 3], np.int32), np.asarray([0, 3], np.int64), check)
        with pytest.raises(ValueError, match="not in the graph"):
            p.ego_graph(h, g, np.asarray([2, 6], np.int32), 1, check)
    # the same vertex in two sets is no repeat
    same(induced(h, g, [[2, 1], [2, 3]]), batched(s, d, None, [[2, 1], [2, 3]]))
    with pytest.raises(ValueError, match="must match"):
        p.ego_graph(h, g, np.asarray([2], np.int64), 1, False)
    with pytest.raises(ValueError, match="must match"):
        p.induced_subgraph(h, g, np.asarray([2], np.int64), np.asarray([0, 1], np.int64), False)
    for name, bad in (("sg_path", 3), ("sg_path", -1), ("sg_split_min", 0), ("ego_budget", 0), ("ego_budget", 1.5)):
        with pytest.raises(ValueError):
            h.set_option(name, bad)


# ------------------------------------------------------------------ 4. multigraph, types
def multigraph():
    """Repeated edges (up to four copies), loops (one repeated), both directions of some pairs."""
    rng = np.random.default_rng(3)
    s = rng.integers(0, 40, 400)
    d = rng.integers(0, 40, 400)
    s = np.r_[s, s[:150], s[:60], s[:20], np.arange(10), np.arange(5)]
    d = np.r_[d, d[:150], d[:60], d[:20], np.arange(10), np.arange(5)]
    return s.astype(np.int64), d.astype(np.int64), np.arange(len(s))


def test_multigraph_returns_every_copy_with_its_weight():
    s, d, copy = multigraph()
    w = edge_weight(s, d, copy).astype(np.float32)  # copies of one pair differ: 5 * copy stays below 4093
    p = plc()
    h = p.ResourceHandle()
    g = p.SGGraph(h, p.GraphProperties(is_symmetric=False, is_multigraph=True), s.astype(np.int32),
                  d.astype(np.int32), w, store_transposed=False, renumber=True)
    sets = [np.arange(0, 40, 2), np.arange(10), np.arange(40)]
    r = induced(h, g, sets)
    same(r, batched(s, d, w, sets), wdtype=np.float32)
    assert int(host(r[3])[-1] - host(r[3])[-2]) == len(s)  # the whole vertex set: every stored edge
    seeds = [0, 7, 39]
    for radius in (0, 1, 2):
        same(ego(h, g, seeds, radius), twin_ego(s, d, w, seeds, radius), wdtype=np.float32)


@pytest.mark.parametrize("renumber", [True, False])
@pytest.mark.parametrize("wdtype", [None, np.float32, np.float64])
@pytest.mark.parametrize("vdtype", [np.int32, np.int64])
def test_type_combinations(vdtype, wdtype, renumber):
    s, d = dataset("dolphins.csv")
    if renumber:  # ids that need the lookup: sparse (the kernels themselves see internal ids only)
        s, d = s * 1000 + 7, d * 1000 + 7
    w = None if wdtype is None else edge_weight(s, d).astype(wdtype)
    h, g = make_graph(s, d, w, symmetric=True, renumber=renumber, vdtype=vdtype, wdtype=wdtype or np.float32)
    ids = np.unique(np.r_[s, d])
    seeds = ids[[0, 5, 30, 61]]
    same(ego(h, g, seeds, 2, vdtype), twin_ego(s, d, w, seeds, 2), vdtype, wdtype)
    sets = [ids[::3][::-1], ids[10:40]]
    same(induced(h, g, sets, vdtype), batched(s, d, w, sets), vdtype, wdtype)


# ------------------------------------------------------------------ 5. tiers
def hubs(degrees, leaves_from=16):
    """Hub i (id i) has out-edges to the first degrees[i] leaves; every third leaf points back at hub 0."""
    s, d = [], []
    for i, deg in enumerate(degrees):
        s += [i] * deg
        d += list(range(leaves_from, leaves_from + deg))
    back = list(range(leaves_from, leaves_from + max(degrees), 3))
    s += back
    d += [0] * len(back)
    return np.asarray(s, np.int64), np.asarray(d, np.int64)


def run_paths(s, d, sets, vdtype=np.int32, splits=(4096,), seeds=None, radius=1):
    """The twin's result, and the same bytes under every sg_path and every sg_split_min given."""
    w = edge_weight(s, d).astype(np.float32)
    want = batched(s, d, w, sets) if seeds is None else twin_ego(s, d, w, seeds, radius)
    first = None
    deg = np.bincount(s, minlength=int(max(s.max(), d.max())) + 1)
    for path, split in [(0, x) for x in splits] + [(1, 4096), (2, 4096)]:
        h, g = make_graph(s, d, w, renumber=False, vdtype=vdtype,
                          options={"sg_path": path, "sg_split_min": split})
        r = induced(h, g, sets, vdtype) if seeds is None else ego(h, g, seeds, radius, vdtype)
        if seeds is None:  # the split tier took the rows it should: 1024 entries per segment
            rows = np.concatenate([deg[np.asarray(x, np.int64)] for x in sets] + [np.zeros(0, np.int64)])
            rows = rows[rows >= split] if path == 0 else rows[:0]
            assert h.last_hot_kernel_launches() == int(((rows + 1023) // 1024).sum())
        if first is None:
            first = r
            same(r, want, vdtype, np.float32)
        else:
            same_bytes(first, r)
    return first


def test_rows_around_the_wave_cut():
    s, d = hubs([63, 64, 65, 1, 0, 130])
    leaves = np.arange(16, 16 + 130)
    sets = [np.r_[np.arange(6), leaves],             # every entry of every row is a hit
            np.r_[np.arange(6), leaves[::2]],        # every other one
            np.r_[0, 1, 2, leaves[60:68]],           # hits around entries 63 / 64 / 65
            np.r_[5, leaves[60:70], leaves[126:130]],  # on both sides of the 64-entry steps of a 130-entry row
            np.r_[5, leaves[63], leaves[64], leaves[127], leaves[128]],
            np.r_[1, 2, 5]]                          # no hit at all
    run_paths(s, d, sets)
    run_paths(s, d, [], seeds=[0, 1, 2, 5, 16, 17], radius=2)


@pytest.mark.parametrize("vdtype,stage", [(np.int32, 1024), (np.int64, 512)])
def test_member_lists_around_the_lds_stage(vdtype, stage):
    s, d = hubs([2000, 1100])
    leaves = np.arange(16, 16 + 2000)
    # the lists hold stage - 1, stage and stage + 1 vertices; a long row against each
    sets = [np.r_[0, 1, leaves[:n - 2]][::-1] for n in (stage - 1, stage, stage + 1)]
    sets += [np.r_[0, leaves[1000:1000 + stage - 1]], np.r_[1, leaves[1990:2000], leaves[:stage - 11]]]
    run_paths(s, d, sets, vdtype)


def test_hub_rows_through_the_split_tier():
    s, d = hubs([3000, 1024, 1025, 129, 127])
    leaves = np.arange(16, 16 + 3000)
    sets = [np.r_[np.arange(5), leaves],               # everything
            np.r_[np.arange(5), leaves[1020:1030], leaves[2040:2050], leaves[2999]],  # across segment cuts
            np.r_[0, leaves[::7]],
            np.r_[0, 3, 4, leaves[100:140]]]
    r = run_paths(s, d, sets, splits=(128, 1, 1024, 1025, 3000, 3001, 4096))
    assert int(host(r[3])[1]) == len(s)
    run_paths(s, d, [], splits=(128, 4096), seeds=[0, 16, 2], radius=2)


# ------------------------------------------------------------------ 6. the ego budget
def test_ego_budget_batches_and_bit_map():
    s, d = dataset("email-Eu-core.csv")
    seeds = seeds_of(s, d, 220, rng_seed=11)
    h, g = make_graph(s, d, None, symmetric=True)
    base = ego(h, g, seeds, 2)
    same(base, twin_ego(s, d, None, seeds, 2))
    hops = h.last_iterations()
    assert hops == 2
    # hop 1 expands a seed's row (at most 347 candidates), hop 2 thousands per seed: 4000 gives several
    # batches at hop 1 and the bit map for most seeds at hop 2, 300 the bit map nearly everywhere, 1 always,
    # 200000 several batches of many seeds at hop 2
    for budget in (200000, 4000, 300, 1):
        h.set_option("ego_budget", budget)
        same_bytes(base, ego(h, g, seeds, 2))
    h.set_option("ego_budget", 2**24)
    same_bytes(base, ego(h, g, seeds, 2))


# ------------------------------------------------------------------ 7. R-MAT
def test_rmat12():
    from oracle.rmat import rmat
    s, d = rmat(12, 16 << 12, seed=7)  # directed, with repeated edges and loops
    s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    seeds = seeds_of(s, d, 256, rng_seed=2)
    p = plc()
    h = p.ResourceHandle()
    g = p.SGGraph(h, p.GraphProperties(is_symmetric=False, is_multigraph=True), s.astype(np.int32),
                  d.astype(np.int32), None, store_transposed=False, renumber=True)
    base = ego(h, g, seeds, 2)
    same(base, twin_ego(s, d, None, seeds, 2))
    h.set_option("ego_budget", 20000)
    h.set_option("sg_split_min", 256)
    same_bytes(base, ego(h, g, seeds, 2))


# ------------------------------------------------------------------ 8. multi-GPU graph
def test_multi_gpu_graph_is_not_implemented():
    """One rank over RCCL, the setup of test_gpu_similarity.py's test of the same name."""
    import torch
    import torch.distributed as dist
    import bench
    p = plc()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(bench.free_port())
    dist.init_process_group("gloo", rank=0, world_size=1)
    ctx = p.comms.init_rccl(1)
    try:
        h = p.ResourceHandle(ctx.ptr)
        s = torch.tensor([0, 1, 1, 2, 2, 0], dtype=torch.int32, device="cuda")
        d = torch.tensor([1, 0, 2, 1, 0, 2], dtype=torch.int32, device="cuda")
        g = p.MGGraph(h, p.GraphProperties(is_symmetric=True, is_multigraph=False), s, d, None,
                      store_transposed=False, num_edges=6)
        with pytest.raises(NotImplementedError, match="multi-GPU"):
            p.ego_graph(h, g, s[:2], 1, False)
        with pytest.raises(NotImplementedError, match="multi-GPU"):
            p.induced_subgraph(h, g, s[:2], torch.tensor([0, 2], dtype=torch.int64, device="cuda"), False)
        g = None
        h = None
    finally:
        torch.cuda.synchronize()
        p.trim_device_cache()
        ctx.free()
        dist.destroy_process_group()


# ------------------------------------------------------------------ 9. the Python layer
def nx_dataset(name, weighted=True):
    import networkx as nx
    data = np.loadtxt(dataset_path(name), dtype=np.float64, ndmin=2)
    G = nx.DiGraph() if DATASETS[name] else nx.Graph()
    for a, b in data[:, :2].astype(np.int64).tolist():
        if weighted:
            G.add_edge(a, b, weight=float(edge_weight([min(a, b)], [max(a, b)])[0]))
        else:
            G.add_edge(a, b)
    return G


def cu_graph(G, weighted=True, **kw):
    import cugraph
    import pandas as pd
    rows = [(u, v, dd.get("weight", 1.0)) for u, v, dd in G.edges(data=True)]
    df = pd.DataFrame({"s": [r[0] for r in rows], "d": [r[1] for r in rows],
                       "w": np.asarray([r[2] for r in rows], np.float32)})
    C = cugraph.Graph(directed=G.is_directed())
    C.from_pandas_edgelist(df, "s", "d", "w" if weighted else None, **kw)
    return C


def nx_rows(H, weighted=True):
    out = []
    for u, v, dd in H.edges(data=True):
        wt = np.float32(dd["weight"]).item() if weighted else None
        out.append((u, v, wt))
        if not H.is_directed() and u != v:
            out.append((v, u, wt))
    return sorted(out)


def cu_rows(C, weighted=True):
    if C.edgelist is None:
        return []
    e = C.edgelist
    w = host(e["weights"]).tolist() if weighted else [None] * len(e["src"])
    return sorted(zip(host(e["src"]).tolist(), host(e["dst"]).tolist(), w))


@pytest.mark.parametrize("name", ["karate.csv", "karate-asymmetric.csv", "dolphins.csv"])
def test_cugraph_layer_on_a_cugraph_graph(name):
    import cugraph
    import networkx as nx
    G = nx_dataset(name)
    C = cu_graph(G)
    nodes = sorted(G.nodes())
    for n, radius in ((nodes[0], 1), (nodes[5], 2), (nodes[-1], 0), (nodes[2], 3)):
        E = cugraph.ego_graph(C, n, radius=radius)
        assert type(E) is type(C) and E.is_directed() == C.is_directed()
        assert cu_rows(E) == nx_rows(nx.ego_graph(G, n, radius=radius))
    assert cu_rows(cugraph.ego_graph(C, nodes[0])) == nx_rows(nx.ego_graph(G, nodes[0], radius=1))
    S = nodes[::2][::-1]
    sub = cugraph.subgraph(C, S)
    assert cu_rows(sub) == nx_rows(G.subgraph(S)) and sub.is_weighted()
    import pandas as pd
    assert cu_rows(cugraph.subgraph(C, pd.Series(S))) == nx_rows(G.subgraph(S))
    assert cugraph.subgraph(C, []).edgelist is None and cugraph.subgraph(C, [nodes[0]]).edgelist is None
    with pytest.raises(ValueError):
        cugraph.subgraph(C, [nodes[0], 10**6])
    with pytest.raises(ValueError):
        cugraph.subgraph(C, [nodes[0], nodes[0]])
    seeds = [nodes[3], nodes[0], nodes[3]]
    df, off = cugraph.batched_ego_graphs(C, seeds, radius=2)
    assert list(df.columns) == ["src", "dst", "weight"] and isinstance(off, pd.Series) and len(off) == 4
    for i, n in enumerate(seeds):
        part = df.iloc[int(off[i]):int(off[i + 1])]
        got = sorted(zip(part["src"].tolist(), part["dst"].tolist(), part["weight"].tolist()))
        assert got == nx_rows(nx.ego_graph(G, n, radius=2))
    df, off = cugraph.batched_ego_graphs(C, [], radius=2)
    assert len(df) == 0 and off.tolist() == [0]
    # unweighted, not renumbered, transposed storage: carried over to the result
    U = cu_graph(G, weighted=False, renumber=False, store_transposed=True)
    E = cugraph.ego_graph(U, nodes[5], radius=2)
    assert cu_rows(E, False) == nx_rows(nx.ego_graph(G, nodes[5], radius=2), False)
    assert not E.is_weighted() and E._renumber is False and E.store_transposed is True
    df, off = cugraph.batched_ego_graphs(U, [nodes[1]])
    assert list(df.columns) == ["src", "dst"]


@pytest.mark.parametrize("directed", [False, True])
def test_cugraph_layer_on_a_networkx_graph(directed):
    import cugraph
    import networkx as nx
    import pandas as pd
    base = nx_dataset("karate-asymmetric.csv" if directed else "karate.csv")
    label = lambda n: "v%02d" % n
    G = nx.relabel_nodes(base, label)
    E = cugraph.ego_graph(G, label(3), radius=2)
    want = nx.ego_graph(G, label(3), radius=2)
    assert isinstance(E, nx.DiGraph if directed else nx.Graph) and E.is_directed() == directed
    assert nx_rows(E) == nx_rows(want)
    S = [label(n) for n in sorted(base.nodes())[::3]]
    sub = cugraph.subgraph(G, S)
    assert nx_rows(sub) == nx_rows(G.subgraph(S)) and sub.is_directed() == directed
    seeds = [label(2), label(9)]
    df, off = cugraph.batched_ego_graphs(G, seeds, radius=1)
    assert isinstance(df, pd.DataFrame) and isinstance(off, list) and len(off) == 3 and off[0] == 0
    for i, n in enumerate(seeds):
        part = df.iloc[off[i]:off[i + 1]]
        got = sorted(zip(part["src"].tolist(), part["dst"].tolist(), part["weight"].tolist()))
        assert got == nx_rows(nx.ego_graph(G, n, radius=1))
    with pytest.raises(ValueError, match="not valid"):
        cugraph.subgraph(G, ["nobody"])
