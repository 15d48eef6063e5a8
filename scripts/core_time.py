"""Core number / k-core timing (measurement aid, not product): one GPU.
On the benchmark's symmetric R-MAT graph (bench.build_rmat_graph, edge factor 16), per scale
and for core_scan 1 (a level's scan reads the compacted list of the vertices not yet peeled)
and 0 (it reads every vertex): 1 warm-up and TIMED core_number calls; prints the mean ms per
call (host clock around the C call, stream idle on both sides), the rounds
(last_iterations), the distinct levels and the largest core of the result, the library's own
event time around the peel launches (last_hot_kernel_ms, profiling on, one more call), and
whether the two settings gave equal arrays.  Then one k_core at the main core from the
computed numbers.

Every scale runs in a process of its own under a time limit; the first one that fails or runs
out of time ends the script.

usage: core_time.py [SCALES=20,22,24] [TIMED=3] [LIMIT_S=300]
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cugraph-forked_amd"))
sys.path.insert(0, ROOT)

WARM = 1


def call(f, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def one(scale, timed):
    import torch
    import bench
    import pylibcugraph as p
    h = p.ResourceHandle()
    g, _, _ = bench.build_rmat_graph(p, h, scale, transposed=False)
    print(f"R-MAT-{scale}: V {g.number_of_vertices()} E {g.number_of_edges()}", flush=True)
    kept = {}
    for scan in (1, 0):
        h.set_option(None, 0)
        h.set_option("core_scan", scan)
        h.set_profiling(False)
        ts = []
        for i in range(WARM + timed):
            t, res = call(lambda: p.core_number(h, g, None, False), torch)
            if i >= WARM:
                ts.append(t)
            del res
        rounds = h.last_iterations()
        h.set_profiling(True)
        v, c = p.core_number(h, g, None, False)
        hot, launches = h.last_hot_kernel_ms(), h.last_hot_kernel_launches()
        h.set_profiling(False)
        by_ext = torch.zeros(1 << scale, dtype=torch.int64, device=c.device)
        by_ext[v.to(torch.int64)] = c.to(torch.int64)
        kept[scan] = by_ext
        levels = int(torch.unique(by_ext[by_ext > 0]).numel())
        print(f"core_scan={scan}: mean {statistics.mean(ts):.3f} ms per call (min {min(ts):.3f}, max {max(ts):.3f}); "
              f"{rounds} rounds, {levels} distinct levels, largest core {int(by_ext.max())}, "
              f"{int((by_ext == by_ext.max()).sum())} vertices in it; peel kernels {hot:.3f} ms over {launches} "
              f"launches", flush=True)
        if scan == 0:
            del v, c
    print(f"core_scan settings equal: {bool(torch.equal(kept[1], kept[0]))}", flush=True)
    h.set_option(None, 0)
    v, c = p.core_number(h, g, None, False)
    k = int(c.max())
    t, (src, dst, w) = call(lambda: p.k_core(h, g, k, None, (v, c), False), torch)
    print(f"k_core at the main core (k = {k}, core numbers given): {t:.3f} ms, {src.numel()} entries", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(int(sys.argv[2]), int(sys.argv[3]))
        return
    scales = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "20,22,24").split(",")]
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    limit = float(sys.argv[3]) if len(sys.argv) > 3 else 300.0
    for scale in scales:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(scale), str(timed)],
                               timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"R-MAT-{scale}: no result within {limit:.0f} s; stopping", flush=True)
            sys.exit(124)
        if r.returncode != 0:
            print(f"R-MAT-{scale}: exit status {r.returncode}; stopping", flush=True)
            sys.exit(1)


if __name__ == "__main__":
    main()
