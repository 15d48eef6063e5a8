"""Similarity / two-hop timing (measurement aid, not product): one GPU.
On a symmetric R-MAT graph of its own (pylibcugraph.generators, edge factor 16, seed 42,
symmetrised and de-duplicated, renumbered): all-edge Jaccard (every stored entry is a pair) under
sim_path 0 / 1 / 2 / 3 and, for the paths that read it, a few sim_split_min values; then two-hop
neighbours from 1024 start vertices (every (V / 1024)-th external id) under a few two_hop_budget
values.  Per setting: WARM warm-up calls, then TIMED calls; prints the median, minimum and maximum
ms per call (host clock around the C call, stream idle on both sides) and the spread
(max - min) / median, the library's own event time around the similarity launches
(last_hot_kernel_ms, one more call with profiling on), and whether every setting gave the same
array as the default.  Forced sim_path 1 (a thread per pair, hub pairs included) is skipped above
R-MAT-20 unless asked for.

The scale runs in a process of its own under a time limit.

usage: similarity_time.py [SCALE=20] [TIMED=5] [LIMIT_S=500] [PATHS=0,1,2,3]
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cugraph-forked_amd"))
sys.path.insert(0, ROOT)

WARM = 2
SPLIT_MINS = (512, 1024, 4096, 16384, 1 << 40)
BUDGETS = (1 << 20, 1 << 22, 1 << 24, 1 << 26, 1 << 28)


def call(f, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def timed_calls(f, timed, torch):
    ts, res = [], None
    for i in range(WARM + timed):
        del res
        t, res = call(f, torch)
        if i >= WARM:
            ts.append(t)
    return ts, res


def line(ts):
    med = statistics.median(ts)
    return f"median {med:.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, spread {(max(ts) - min(ts)) / med * 100:.1f} %)"


def one(scale, timed, paths):
    import torch
    import pylibcugraph as p
    h = p.ResourceHandle()
    s, d = p.generators.generate_rmat_edgelist(h, scale, 16 << scale, seed=42)
    s, d, _ = p.generators.symmetrize_dedup(h, s, d, None, True)
    g = p.SGGraph(h, p.GraphProperties(is_symmetric=True), s, d, None, store_transposed=False, renumber=True)
    print(f"R-MAT-{scale}: V {g.number_of_vertices()} E {g.number_of_edges()}; pairs: all {s.numel()} entries",
          flush=True)

    def jaccard():
        return p.jaccard_coefficients(h, g, s, d, False, False)[2]

    h.set_option(None, 0)
    base = jaccard().clone()
    for path in paths:
        for split in (SPLIT_MINS if path in (0, 3) else (None,)):
            if path == 3 and split != SPLIT_MINS[0]:
                continue  # forced split does not read the threshold
            h.set_option(None, 0)
            h.set_option("sim_path", path)
            if split is not None and path == 0:
                h.set_option("sim_split_min", split)
            ts, res = timed_calls(jaccard, timed, torch)
            h.set_profiling(True)
            res = jaccard()
            hot, launches = h.last_hot_kernel_ms(), h.last_hot_kernel_launches()
            h.set_profiling(False)
            name = f"sim_path={path}" + (f" sim_split_min={split}" if path == 0 else "")
            print(f"{name}: {line(ts)}; kernels {hot:.3f} ms over {launches} launches; "
                  f"equal to the default: {bool(torch.equal(res, base))}", flush=True)
            del res
    h.set_option(None, 0)
    ts, _ = timed_calls(jaccard, timed, torch)
    print(f"defaults again: {line(ts)}", flush=True)

    nv = 1 << scale
    start = torch.arange(0, nv, nv // 1024, dtype=torch.int32, device="cuda")[:1024]
    present = torch.isin(start, s)
    start = start[present]
    kept = None
    for budget in BUDGETS:
        h.set_option(None, 0)
        h.set_option("two_hop_budget", budget)
        ts, (a, b) = timed_calls(lambda: p.get_two_hop_neighbors(h, g, start), timed, torch)
        same = kept is None or (torch.equal(a, kept[0]) and torch.equal(b, kept[1]))
        kept = kept or (a.clone(), b.clone())
        print(f"two-hop from {start.numel()} start vertices, two_hop_budget={budget}: {line(ts)}; {a.numel()} pairs; "
              f"equal to the first: {same}", flush=True)
        del a, b


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(int(sys.argv[2]), int(sys.argv[3]), [int(x) for x in sys.argv[4].split(",")])
        return
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    limit = float(sys.argv[3]) if len(sys.argv) > 3 else 500.0
    paths = sys.argv[4] if len(sys.argv) > 4 else ("0,1,2,3" if scale <= 20 else "0,2,3")
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(scale), str(timed), paths],
                           timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"R-MAT-{scale}: no result within {limit:.0f} s; stopping", flush=True)
        sys.exit(124)
    if r.returncode != 0:
        print(f"R-MAT-{scale}: exit status {r.returncode}; stopping", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
