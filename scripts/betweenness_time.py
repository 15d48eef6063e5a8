"""Betweenness centrality timing (measurement aid, not product): one GPU.
On the benchmark's symmetric R-MAT graph (bench.build_rmat_graph, edge factor 16), per scale, K sources
drawn once with a fixed seed, for every bc_batch given, alternating the settings REPS times after one
warm-up call each: the host clock around the C call (stream idle on both sides) and the library's own
event time around the sweep's launches (last_hot_kernel_ms, profiling on, a call of its own), the batches
(last_iterations) and the launches.  Then whether all settings gave bit-equal vertex scores, and one
edge betweenness call at the first setting.

Every scale runs in a process of its own under a time limit; the first one that fails or runs out of time
ends the script.

usage: betweenness_time.py [SCALES=20] [K=256] [BATCHES=64,1] [REPS=2] [LIMIT_S=500]
"""
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cugraph-forked_amd"))
sys.path.insert(0, ROOT)


def call(f, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def one(scale, k, batches, reps):
    import torch
    import bench
    import pylibcugraph as p
    h = p.ResourceHandle()
    g, _, _ = bench.build_rmat_graph(p, h, scale, transposed=False)
    nv = g.number_of_vertices()
    print(f"R-MAT-{scale}: V {nv} E {g.number_of_edges()}, {k} sources", flush=True)
    order = p.betweenness_centrality(h, g, [], None, True, False, False)[0]
    src = order[torch.as_tensor(random.Random(7).sample(range(nv), k), device=order.device)].contiguous()

    def run():
        return p.betweenness_centrality(h, g, src, None, True, False, False)

    wall = {b: [] for b in batches}
    hot = {b: [] for b in batches}
    kept, info = {}, {}
    for rep in range(reps + 1):  # rep 0 warms every setting up
        for b in batches:
            h.set_option(None, 0)
            h.set_option("bc_batch", b)
            h.set_profiling(False)
            t, (v, x) = call(run, torch)
            h.set_profiling(True)
            _, x2 = run()
            ms, launches, n = h.last_hot_kernel_ms(), h.last_hot_kernel_launches(), h.last_iterations()
            h.set_profiling(False)
            if rep:
                wall[b].append(t)
                hot[b].append(ms)
            kept[b], info[b] = x.clone(), (n, launches)
            assert torch.equal(x, x2)
            del v, x, x2
    for b in batches:
        n, launches = info[b]
        print(f"bc_batch={b}: {statistics.mean(wall[b]):.1f} ms per call (min {min(wall[b]):.1f}, max {max(wall[b]):.1f}); "
              f"sweep kernels {statistics.mean(hot[b]):.1f} ms (min {min(hot[b]):.1f}, max {max(hot[b]):.1f}) over "
              f"{launches} launches, {n} batches", flush=True)
    print(f"vertex scores bit-equal across bc_batch: {all(torch.equal(kept[batches[0]], kept[b]) for b in batches)}",
          flush=True)
    h.set_option(None, 0)
    h.set_option("bc_batch", batches[0])
    t, res = call(lambda: p.edge_betweenness_centrality(h, g, src, None, True, False), torch)
    del res
    t, res = call(lambda: p.edge_betweenness_centrality(h, g, src, None, True, False), torch)
    print(f"edge betweenness, bc_batch={batches[0]}: {t:.1f} ms per call", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(int(sys.argv[2]), int(sys.argv[3]), [int(x) for x in sys.argv[4].split(",")], int(sys.argv[5]))
        return
    scales = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "20").split(",")]
    k = sys.argv[2] if len(sys.argv) > 2 else "256"
    batches = sys.argv[3] if len(sys.argv) > 3 else "64,1"
    reps = sys.argv[4] if len(sys.argv) > 4 else "2"
    limit = float(sys.argv[5]) if len(sys.argv) > 5 else 500.0
    for scale in scales:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(scale), k, batches, reps],
                               timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"R-MAT-{scale}: no result within {limit:.0f} s; stopping", flush=True)
            sys.exit(124)
        if r.returncode != 0:
            print(f"R-MAT-{scale}: exit status {r.returncode}; stopping", flush=True)
            sys.exit(1)


if __name__ == "__main__":
    main()
