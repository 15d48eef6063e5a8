"""k-truss timing (measurement aid, not product): one process, one GPU.
On the benchmark's symmetric, renumbered R-MAT graphs (bench.build_rmat_graph) of the given scales, for
k = 4, 8 and 16: the first k_truss_subgraph call on a fresh graph (it builds the simple rows, the edge ids
and the supports, then peels), then a call with every other k on the same graph, which starts from the
cached supports and is the peel and the extraction alone.  Prints, per call, the milliseconds (host clock
around the C call, stream idle on both sides), the peel rounds (last_iterations) and the surviving stored
edges; for the calls after the first also the library's own event time around the peel launches
(last_hot_kernel_ms, profiling on, one more call).  Then, on the same graph, triangle_count (first call,
then the mean of TIMED warm calls) as the yardstick for the support pass, and whether kt_path 0 / 1 / 2
give equal arrays at k = 8 on the smallest scale.

usage: ktruss_time.py [SCALES=18,20] [TIMED=3]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cugraph-forked_amd"))
sys.path.insert(0, ROOT)

KS = (4, 8, 16)


def timed_call(f, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def main():
    import torch
    import bench
    import pylibcugraph as p
    scales = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "18,20").split(",")]
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    h = p.ResourceHandle()
    for scale in scales:
        for k in KS:
            g, _, _ = bench.build_rmat_graph(p, h, scale, transposed=False)  # fresh: nothing cached
            if k == KS[0]:
                print(f"R-MAT-{scale}: V {g.number_of_vertices()} E {g.number_of_edges()}", flush=True)
            t, res = timed_call(lambda: p.k_truss_subgraph(h, g, k, False), torch)
            print(f"R-MAT-{scale} k={k}: first call (supports + peel) {t:.2f} ms, {h.last_iterations()} rounds, "
                  f"{res[0].numel()} stored edges left", flush=True)
            del res
            if k == KS[0]:
                for k2 in KS[1:] + KS[:1]:
                    t, res = timed_call(lambda: p.k_truss_subgraph(h, g, k2, False), torch)
                    rounds, left = h.last_iterations(), res[0].numel()
                    del res
                    h.set_profiling(True)
                    res = p.k_truss_subgraph(h, g, k2, False)
                    hot, launches = h.last_hot_kernel_ms(), h.last_hot_kernel_launches()
                    h.set_profiling(False)
                    del res
                    print(f"R-MAT-{scale} k={k2}: cached supports (peel + extraction) {t:.2f} ms, {rounds} rounds, "
                          f"{left} stored edges left; peel launches alone {hot:.2f} ms over {launches} launches",
                          flush=True)
                first, res = timed_call(lambda: p.triangle_count(h, g, None, False), torch)
                del res
                ts = []
                for _ in range(timed):
                    t, res = timed_call(lambda: p.triangle_count(h, g, None, False), torch)
                    ts.append(t)
                    del res
                print(f"R-MAT-{scale} triangle_count on the same graph: first call {first:.2f} ms, then mean "
                      f"{statistics.mean(ts):.2f} ms (min {min(ts):.2f})", flush=True)
            del g
            p.trim_device_cache()
    scale = min(scales)
    kept = []
    for path in (0, 1, 2):
        h.set_option(None, 0)
        h.set_option("kt_path", path)
        g, _, _ = bench.build_rmat_graph(p, h, scale, transposed=False)
        t, res = timed_call(lambda: p.k_truss_subgraph(h, g, 8, False), torch)
        print(f"R-MAT-{scale} k=8 kt_path={path}: first call {t:.2f} ms", flush=True)
        kept.append([x.clone() for x in res[:2]])
        del res, g
        p.trim_device_cache()
    h.set_option(None, 0)
    same = all(torch.equal(a, b) for other in kept[1:] for a, b in zip(kept[0], other))
    print(f"kt_path settings equal: {bool(same)}", flush=True)


if __name__ == "__main__":
    main()
