"""Ego-net and induced-subgraph timing (measurement aid, not product): one process, one GPU.
On the benchmark's symmetric, renumbered R-MAT graph (bench.build_rmat_graph) of the given scale, A/B
through the handle options, every figure the median of TIMED calls after one warm-up (host clock around
the call, device idle on both sides):
  * ego_graph of SEEDS1 seeds at radius 1 and of SEEDS2 seeds at radius 2: sg_path 0 / 1 / 2, several
    sg_split_min, several ego_budget;
  * one induced_subgraph of a single large set (every second vertex): sg_path and sg_split_min;
  * the reference's shape of the computation with what the library had before: one bfs with depth_limit
    per seed, the reached vertices compacted, then the same extraction -- against ego_graph on the same seeds.
Every variant's arrays are compared with the defaults' (equal: True is printed once per group).

usage: ego_time.py [SCALE=20] [SEEDS1=1024] [SEEDS2=16] [TIMED=5]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cugraph-forked_amd"))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    import pylibcugraph as p
    arg = lambda i, default: int(sys.argv[i]) if len(sys.argv) > i else default
    scale, seeds1, seeds2, timed = arg(1, 20), arg(2, 1024), arg(3, 16), arg(4, 5)
    h = p.ResourceHandle()
    g, roots, _ = bench.build_rmat_graph(p, h, scale, transposed=False, want_roots=seeds1)
    print(f"R-MAT-{scale}: V {g.number_of_vertices()} E {g.number_of_edges()}, {len(roots)} seeds", flush=True)
    roots = torch.as_tensor(roots, dtype=torch.int32, device="cuda")

    def median_ms(f):
        res = f()  # warm-up
        torch.cuda.synchronize()
        ts = []
        for _ in range(timed):
            del res
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), res

    def group(title, f, variants):
        base, equal = None, True
        for name, options in variants:
            h.set_option(None, 0)
            for k, v in options.items():
                h.set_option(k, v)
            med, lo, res = median_ms(f)
            note = ""
            if base is None:
                base = [None if x is None else x.clone() for x in res]
                note = f"  [{res[0].numel()} edges, {h.last_hot_kernel_launches()} split segments]"
            else:
                equal = equal and all(torch.equal(a, b) for a, b in zip(base, res) if a is not None)
            print(f"{title} | {name}: median {med:.2f} ms (min {lo:.2f}){note}", flush=True)
            del res
        h.set_option(None, 0)
        print(f"{title} | arrays equal under every setting: {equal}", flush=True)
        del base
        p.trim_device_cache()
        torch.cuda.empty_cache()

    extraction = [("defaults", {}), ("sg_path=1", {"sg_path": 1}), ("sg_path=2", {"sg_path": 2}),
                  ("sg_split_min=64", {"sg_split_min": 64}), ("sg_split_min=128", {"sg_split_min": 128}),
                  ("sg_split_min=512", {"sg_split_min": 512}), ("sg_split_min=1024", {"sg_split_min": 1024}),
                  ("sg_split_min=4096", {"sg_split_min": 4096}), ("sg_split_min=16384", {"sg_split_min": 16384}),
                  ("sg_split_min=2^40 (off)", {"sg_split_min": 2**40})]
    budgets = [(f"ego_budget=2^{b}", {"ego_budget": 2**b}) for b in (18, 20, 22, 24, 27, 28)]
    for radius, seeds in ((1, roots), (2, roots[:seeds2])):
        group(f"ego radius {radius}, {seeds.numel()} seeds", lambda: p.ego_graph(h, g, seeds, radius, False),
              extraction + budgets)

    # one large set: every second vertex
    _, _, verts = p.bfs(h, g, roots[:1], False, 1, False, False)
    big = verts[::2].contiguous()
    off = torch.tensor([0, big.numel()], dtype=torch.int64, device="cuda")
    group(f"induced subgraph of {big.numel()} vertices", lambda: p.induced_subgraph(h, g, big, off, False), extraction)

    # the reference's shape: a BFS with a depth limit per seed, then the same extraction
    def per_seed_bfs(seeds, radius):
        parts, sizes = [], [0]
        for i in range(seeds.numel()):
            dist, _, v = p.bfs(h, g, seeds[i:i + 1], True, radius, False, False)
            reached = v[dist <= radius]
            parts.append(reached)
            sizes.append(sizes[-1] + reached.numel())
        offs = torch.tensor(sizes, dtype=torch.int64, device="cuda")
        return p.induced_subgraph(h, g, torch.cat(parts), offs, False)

    for radius, seeds in ((1, roots), (2, roots[:seeds2])):
        a, _, ra = median_ms(lambda: p.ego_graph(h, g, seeds, radius, False))
        b, _, rb = median_ms(lambda: per_seed_bfs(seeds, radius))
        same = all(torch.equal(x, y) for x, y in zip(ra, rb) if x is not None)
        print(f"radius {radius}, {seeds.numel()} seeds: ego_graph {a:.2f} ms, one bfs per seed + extraction {b:.2f} ms "
              f"(ratio {b / a:.1f}), arrays equal: {same}", flush=True)
        del ra, rb
        p.trim_device_cache()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
