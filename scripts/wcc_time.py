"""Weakly connected components timing (measurement aid, not product): one process,
one GPU.  On the benchmark's symmetric R-MAT graph (bench.build_rmat_graph), 2 warm-up
and 10 timed calls each with wcc_sample=0 (every row fully linked) and with the
default; prints the mean ms per call (host clock around the C call, stream idle on
both sides), the library's own event time around the link and compress launches
(last_hot_kernel_ms, profiling on, a second set of calls) and the component counts.
Then scipy.sparse.csgraph.connected_components on R-MAT-CPU_SCALE from the numpy
generator, as the CPU yardstick.

usage: wcc_time.py [SCALE=24] [CPU_SCALE=20]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cugraph-forked_amd"))
sys.path.insert(0, ROOT)

WARM, TIMED = 2, 10


def timed_calls(p, h, g, torch):
    ts = []
    for i in range(WARM + TIMED):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = p.weakly_connected_components(h, g, False)
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
        del res
    return ts


def main():
    import numpy as np
    import torch
    import bench
    import pylibcugraph as p
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    cpu_scale = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    h = p.ResourceHandle()
    g, _, _ = bench.build_rmat_graph(p, h, scale, transposed=False)
    print(f"R-MAT-{scale}: V {g.number_of_vertices()} E {g.number_of_edges()}", flush=True)
    labels = {}
    for name, k in (("wcc_sample=0", 0), ("default", None)):
        h.set_option(None, 0)
        if k is not None:
            h.set_option("wcc_sample", k)
        h.set_profiling(False)
        ts = timed_calls(p, h, g, torch)
        h.set_profiling(True)
        hot = []
        for _ in range(TIMED):
            res = p.weakly_connected_components(h, g, False)
            hot.append(h.last_hot_kernel_ms())
            launches = h.last_hot_kernel_launches()
        labels[name] = res[1].clone()
        del res
        print(f"{name}: mean {statistics.mean(ts):.3f} ms per call (min {min(ts):.3f}, max {max(ts):.3f}), "
              f"last_hot_kernel_ms mean {statistics.mean(hot):.3f} over {launches} launches", flush=True)
    h.set_profiling(False)
    a, b = labels["wcc_sample=0"], labels["default"]
    sizes = torch.bincount(b.to(torch.int64))
    print(f"labels equal: {bool(torch.equal(a, b))}; components {int((sizes > 0).sum())}, "
          f"largest {int(sizes.max())}", flush=True)
    del g, labels, a, b

    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    from oracle import rmat
    s, d = rmat.rmat(cpu_scale, 16 << cpu_scale, seed=42)
    n = 1 << cpu_scale
    A = sp.coo_matrix((np.ones(2 * len(s), np.int8), (np.r_[s, d], np.r_[d, s])), shape=(n, n)).tocsr()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        nc, _ = connected_components(A, directed=False)
        ts.append((time.perf_counter() - t0) * 1e3)
    print(f"scipy connected_components R-MAT-{cpu_scale} (V {n}, E {A.nnz}): median {statistics.median(ts):.1f} ms, "
          f"{nc} components (ids without edges included)", flush=True)


if __name__ == "__main__":
    main()
