"""Digests of Louvain results for comparing two builds of the library bit for bit
(CUGRAPH_AMD_LIB selects the library; run once per build and diff the outputs).
One line per case: sha256 of the cluster array, Q as hex, the level count and sha256 of
every dendrogram level.  Graphs come from the device R-MAT generator (seed 42; weights
seed 43), symmetrised and deduplicated.  Measurement aid, not product.
usage: louvain_digest.py [sg] [mg]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cugraph-forked_amd"))
sys.path.insert(0, ROOT)


def sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def edges(p, h, scale, weights):
    import torch
    n = 16 << scale
    s, d = p.generators.generate_rmat_edgelist(h, scale, n, 0.57, 0.19, 0.19, 42, False, True)
    w = p.generators.generate_edge_weights(h, n, 43)
    s, d, w = p.generators.symmetrize_dedup(h, s, d, w, True)
    if weights == "int":
        w = torch.floor(w * 4.0) + 1.0
    elif weights == "int8":
        w = torch.floor(w * 8.0) + 1.0
    elif weights == "fp64":  # not representable in fp32
        w = w.double() / 3.0
    return s, d, w


def line(name, p, h, g):
    v, c, q, levels = p.louvain_dendrogram(h, g, 100, 1.0)
    print(f"{name}: clusters {sha(c)} Q {float(q).hex()} levels {len(levels)} " + " ".join(sha(x) for x in levels),
          flush=True)


def sg(p):
    import torch
    props = p.GraphProperties(is_symmetric=True, is_multigraph=False)
    for name, scale, weights in (("sg rmat20 int", 20, "int"), ("sg rmat20 fp32", 20, "fp32"),
                                 ("sg rmat18 fp64", 18, "fp64")):
        h = p.ResourceHandle()
        s, d, w = edges(p, h, scale, weights)
        line(name, p, h, p.SGGraph(h, props, s, d, w, store_transposed=False, renumber=True))
    h = p.ResourceHandle()
    s, d, w = edges(p, h, 16, "int8")
    deg = torch.bincount(s.to(torch.int64))
    heavy = torch.sort(deg[deg > 2048]).values
    mid = int(heavy[heavy.numel() // 2 - 1]) if heavy.numel() > 1 else 0
    print(f"sg rmat16: {heavy.numel()} rows over 2048 edges, degrees {heavy.tolist()}, mid limit {mid}", flush=True)
    for renumber, opts in ((True, {}), (False, {}), (True, {"louvain_big_hash": 0}), (False, {"louvain_big_cap": 16}),
                           (False, {"louvain_big_maxdeg": 3000}), (True, {"louvain_big_maxdeg": 4530}),
                           (False, {"louvain_big_maxdeg": 4530}), (True, {"louvain_big_maxdeg": mid}),
                           (False, {"louvain_big_maxdeg": mid}), (False, {"louvain_big_maxdeg": 2048}),
                           (True, {"louvain_wide_keys": 1}), (True, {"louvain_hash": 0})):
        h = p.ResourceHandle()
        for k, x in opts.items():
            h.set_option(k, x)
        line(f"sg rmat16 renumber={renumber} {opts}", p, h,
             p.SGGraph(h, props, s, d, w, store_transposed=False, renumber=renumber))


def mg(p):
    import torch.distributed as dist
    import bench
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(bench.free_port())
    dist.init_process_group("gloo", rank=0, world_size=1)
    ctx = p.comms.init_rccl(1)
    try:
        h = p.ResourceHandle(ctx.ptr)
        props = p.GraphProperties(is_symmetric=True, is_multigraph=False)
        for name, weights in (("mg1 rmat20 fp32", "fp32"), ("mg1 rmat20 int", "int")):
            s, d, w = edges(p, h, 20, weights)
            g = p.MGGraph(h, props, s, d, w, store_transposed=False, num_edges=s.numel())
            line(name, p, h, g)
            g = None
        h = None
    finally:
        ctx.free()
        dist.destroy_process_group()


if __name__ == "__main__":
    import pylibcugraph
    which = sys.argv[1:] or ["sg", "mg"]
    if "sg" in which:
        sg(pylibcugraph)
    if "mg" in which:
        mg(pylibcugraph)
