"""Triangle counting timing (measurement aid, not product): one process, one GPU.
On the benchmark's symmetric R-MAT graph (bench.build_rmat_graph), for tc_path 0 (by
row size), 1 (a thread per oriented edge) and 2 (a wave per oriented edge): the first
call on a fresh graph (it builds the orientation), then 1 warm-up and TIMED calls;
prints the mean ms per call (host clock around the C call, stream idle on both
sides), the library's own event time around the count and finish launches
(last_hot_kernel_ms, profiling on, a second set of calls), the triangle total and
whether the three paths gave equal arrays.  Also the oriented edge count and the bytes
the oriented rows hold (the least the count kernel must read).  Then an exact scipy
count on R-MAT-CPU_SCALE from the numpy generator, as the CPU yardstick.

usage: tc_time.py [SCALE=20] [CPU_SCALE=12] [TIMED=5]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cugraph-forked_amd"))
sys.path.insert(0, ROOT)

WARM = 1


def call(p, h, g, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = p.triangle_count(h, g, None, False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def oriented_edges(g, h, torch):
    """(entries - self-loops) / 2 of the deduplicated symmetric adjacency."""
    off, idx, _ = g.adjacency(h, transposed=False)
    deg = (off[1:] - off[:-1]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(deg.numel(), dtype=idx.dtype, device=idx.device), deg)
    loops = int((rows == idx).sum())
    return (int(idx.numel()) - loops) // 2, idx.element_size(), off.element_size()


def main():
    import numpy as np
    import torch
    import bench
    import pylibcugraph as p
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    cpu_scale = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    timed = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    h = p.ResourceHandle()
    counts = {}
    for path in (0, 1, 2):
        h.set_option(None, 0)
        h.set_option("tc_path", path)
        h.set_profiling(False)
        g, _, _ = bench.build_rmat_graph(p, h, scale, transposed=False)  # fresh: no cached orientation
        if path == 0:
            V, E = g.number_of_vertices(), g.number_of_edges()
            eo, vb, eb = oriented_edges(g, h, torch)
            least = eo * vb + 2 * (V + 1) * eb
            print(f"R-MAT-{scale}: V {V} E {E}; oriented edges {eo}, oriented rows {eo * vb / 1e6:.1f} MB, "
                  f"with the two offset arrays {least / 1e6:.1f} MB", flush=True)
        first, res = call(p, h, g, torch)
        del res
        ts = []
        for i in range(WARM + timed):
            t, res = call(p, h, g, torch)
            if i >= WARM:
                ts.append(t)
            del res
        h.set_profiling(True)
        hot = []
        for _ in range(timed):
            res = p.triangle_count(h, g, None, False)
            hot.append(h.last_hot_kernel_ms())
            launches = h.last_hot_kernel_launches()
        h.set_profiling(False)
        v, c = res
        by_ext = torch.zeros(1 << scale, dtype=torch.int64, device=c.device)
        by_ext[v.to(torch.int64)] = c.to(torch.int64)
        counts[path] = by_ext
        total = int(by_ext.sum()) // 3
        m = statistics.mean(hot)
        print(f"tc_path={path}: first call {first:.3f} ms, then mean {statistics.mean(ts):.3f} ms per call "
              f"(min {min(ts):.3f}, max {max(ts):.3f}), last_hot_kernel_ms mean {m:.3f} over {launches} launches "
              f"= {least / m / 1e6:.2f} GB/s of the least bytes; triangles {total}, largest count "
              f"{int(by_ext.max())}", flush=True)
        del res, v, c, g
        p.trim_device_cache()
    print(f"paths equal: {bool(torch.equal(counts[0], counts[1]) and torch.equal(counts[0], counts[2]))}", flush=True)

    if cpu_scale <= 0:
        return
    import scipy.sparse as sp
    from oracle import rmat
    s, d = rmat.rmat(cpu_scale, 16 << cpu_scale, seed=42)
    n = 1 << cpu_scale
    keep = s != d
    A = sp.coo_matrix((np.ones(2 * int(keep.sum()), np.int64), (np.r_[s[keep], d[keep]], np.r_[d[keep], s[keep]])),
                      shape=(n, n)).tocsr()
    A.data[:] = 1
    t0 = time.perf_counter()
    per_vertex = np.asarray((A @ A).multiply(A).sum(axis=1)).ravel() // 2
    ms = (time.perf_counter() - t0) * 1e3
    print(f"scipy (A @ A * A) R-MAT-{cpu_scale} (V {n}, E {A.nnz}): {ms:.1f} ms, {int(per_vertex.sum()) // 3} triangles",
          flush=True)
    if cpu_scale == scale:
        print(f"GPU == scipy: {bool(np.array_equal(counts[0].cpu().numpy(), per_vertex))}", flush=True)


if __name__ == "__main__":
    main()
