"""Digests of the integer-valued algorithms around the shared row intersection, for comparing
two builds of the library bit for bit (CUGRAPH_AMD_LIB selects the library; run once per build
and diff the outputs).  One line per case with the sha256 of every result array: triangle counts
under each tc_path; all-edge Jaccard, Sorensen and overlap under each sim_path (path 0 also with
sim_split_min 128); two-hop neighbours from a fixed start list; WCC labels; core numbers.
Graphs come from the device R-MAT generator (seed 42), symmetrised and deduplicated, renumbered
and not, with int32 and int64 ids.  Measurement aid, not product.
usage: intersect_digest.py [SCALES=16,20]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cugraph-forked_amd"))
sys.path.insert(0, ROOT)


def sha(*ts):
    return " ".join(hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16] for t in ts)


def one(p, torch, scale, renumber, idtype):
    h = p.ResourceHandle()
    s, d = p.generators.generate_rmat_edgelist(h, scale, 16 << scale, seed=42)
    s, d, _ = p.generators.symmetrize_dedup(h, s, d, None, True)
    s, d = s.to(idtype), d.to(idtype)
    g = p.SGGraph(h, p.GraphProperties(is_symmetric=True), s, d, None, store_transposed=False, renumber=renumber)
    name = f"rmat{scale} renumber={renumber} {str(idtype).split('.')[-1]}"
    print(f"{name}: V {g.number_of_vertices()} E {g.number_of_edges()}", flush=True)
    for path in (0, 1, 2):
        h.set_option(None, 0)
        h.set_option("tc_path", path)
        print(f"{name} tc_path={path}: {sha(*p.triangle_count(h, g, None, False))}", flush=True)
    for path, split in ((0, None), (0, 128), (1, None), (2, None), (3, None)):
        h.set_option(None, 0)
        h.set_option("sim_path", path)
        if split:
            h.set_option("sim_split_min", split)
        out = [sha(getattr(p, m + "_coefficients")(h, g, s, d, False, False)[2])
               for m in ("jaccard", "sorensen", "overlap")]
        print(f"{name} sim_path={path}{f' sim_split_min={split}' if split else ''}: {' '.join(out)}", flush=True)
    h.set_option(None, 0)
    nv = 1 << scale
    start = torch.arange(0, nv, nv // 256, dtype=idtype, device=s.device)[:256]
    start = start[torch.isin(start, s)]
    print(f"{name} two-hop from {start.numel()}: {sha(*p.get_two_hop_neighbors(h, g, start))}", flush=True)
    print(f"{name} wcc: {sha(*p.weakly_connected_components(h, g, False))}", flush=True)
    print(f"{name} core: {sha(*p.core_number(h, g, None, False))}", flush=True)
    del g
    p.trim_device_cache()


if __name__ == "__main__":
    import torch
    import pylibcugraph
    for scale in [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "16,20").split(",")]:
        for renumber in (True, False):
            for idtype in (torch.int32, torch.int64):
                one(pylibcugraph, torch, scale, renumber, idtype)
