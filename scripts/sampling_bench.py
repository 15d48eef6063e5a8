"""Neighbour sampling / random walk timing (measurement aid, not product): one GPU.
On a symmetric R-MAT graph of its own (pylibcugraph.generators, edge factor 16, seed 42, symmetrised and
de-duplicated, weights from generate_edge_weights on the stored entries, renumbered), from 2^16 start
vertices -- the first 2^16 of a seeded (numpy default_rng(42)) permutation of the graph's vertex ids:

  * fan-out [25, 10] with replacement and without (sample_path 0, and for the latter also 1 and 2: the A/B
    that decides from which fan-out on a slot's Floyd sampler goes to a wave);
  * the same A/B at fan-outs [5, 5], [64] and [256], on both sides of the default's switch;
  * uniform and biased walks of length 80 (the first biased call also builds the running sums).

Per setting: WARM warm-up calls, then TIMED calls; prints the median, minimum and maximum ms per call (host
clock around the C call, stream idle on both sides), picks/s or steps/s from the median, the library's own
event time around the pick / walk kernels (last_hot_kernel_ms, one more call with profiling on), and for
the A/B whether every path gave the same arrays.  The last line is one JSON object with the numbers.

The scale runs in a process of its own under a time limit.

usage: sampling_bench.py [SCALE=24] [TIMED=5] [LIMIT_S=500]
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cugraph-forked_amd"))
sys.path.insert(0, ROOT)

WARM = 2
STARTS = 1 << 16
WALK_LENGTH = 80


def timed_calls(f, timed, torch):
    ts, res = [], None
    for i in range(WARM + timed):
        del res
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = f()
        torch.cuda.synchronize()
        if i >= WARM:
            ts.append((time.perf_counter() - t0) * 1e3)
    return ts, res


def line(ts):
    med = statistics.median(ts)
    return f"median {med:.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, spread {(max(ts) - min(ts)) / med * 100:.1f} %)"


def one(scale, timed):
    import numpy as np
    import torch
    import pylibcugraph as p
    h = p.ResourceHandle()
    s, d = p.generators.generate_rmat_edgelist(h, scale, 16 << scale, seed=42)
    s, d, _ = p.generators.symmetrize_dedup(h, s, d, None, True)
    w = p.generators.generate_edge_weights(h, s.numel(), seed=42)
    g = p.SGGraph(h, p.GraphProperties(is_symmetric=True), s, d, w, store_transposed=False, renumber=True)
    ids = torch.unique(s)
    n = min(STARTS, ids.numel())
    pick = torch.as_tensor(np.random.default_rng(42).permutation(ids.numel())[:n].copy(), device="cuda")
    start = ids[pick].contiguous()
    print(f"R-MAT-{scale}: V {g.number_of_vertices()} E {g.number_of_edges()}; {n} start vertices", flush=True)
    out = {"scale": scale, "vertices": g.number_of_vertices(), "edges": g.number_of_edges(), "starts": n}

    def hot(f):
        h.set_profiling(True)
        res = f()
        ms = h.last_hot_kernel_ms()
        h.set_profiling(False)
        del res
        return ms

    def sample(fan, repl, path, name, base=None):
        h.set_option(None, 0)
        h.set_option("sample_path", path)
        fan_out = np.asarray(fan, dtype=np.int32)

        def f():
            return p.uniform_neighbor_sample(h, g, start, fan_out, repl, False, return_counts=True)
        ts, res = timed_calls(f, timed, torch)
        picks = int(res[3].sum().item())
        med = statistics.median(ts)
        kernel_ms = hot(f)
        same = "" if base is None else f"; equal to sample_path 0: {all(torch.equal(a, b) for a, b in zip(res, base))}"
        print(f"{name}: {line(ts)}; {picks} picks, {len(res[0])} distinct edges, {picks / med / 1e3:.1f} M picks/s; "
              f"pick kernels {kernel_ms:.3f} ms{same}", flush=True)
        out[name] = {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "picks": picks,
                     "picks_per_s": picks / med * 1e3, "last_hot_kernel_ms": kernel_ms}
        return [t.clone() for t in res]

    sample([25, 10], True, 0, "fan_out_25_10_with_replacement")
    for fan in ([25, 10], [5, 5], [64], [256]):
        tag = "_".join(str(k) for k in fan)
        base = sample(fan, False, 0, f"fan_out_{tag}_without_replacement")
        for path in (1, 2):
            sample(fan, False, path, f"fan_out_{tag}_without_replacement_sample_path_{path}", base)
        del base

    h.set_option(None, 0)
    for name, f in (("uniform_walks", p.uniform_random_walks), ("biased_walks", p.biased_random_walks)):
        def call(f=f):
            return f(h, g, start, WALK_LENGTH)
        t0 = time.perf_counter()
        first = call()
        torch.cuda.synchronize()
        first_ms = (time.perf_counter() - t0) * 1e3
        del first
        ts, res = timed_calls(call, timed, torch)
        steps = int((res[0].view(n, WALK_LENGTH + 1)[:, 1:] >= 0).sum().item())
        med = statistics.median(ts)
        kernel_ms = hot(call)
        print(f"{name} of length {WALK_LENGTH}: {line(ts)}; first call {first_ms:.1f} ms; {steps} steps, "
              f"{steps / med / 1e3:.1f} M steps/s; walk kernel {kernel_ms:.3f} ms", flush=True)
        out[name] = {"median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "first_call_ms": first_ms, "steps": steps,
                     "steps_per_s": steps / med * 1e3, "last_hot_kernel_ms": kernel_ms}
        del res
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one":
        one(int(sys.argv[2]), int(sys.argv[3]))
        return
    scale = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    timed = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    limit = float(sys.argv[3]) if len(sys.argv) > 3 else 500.0
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", str(scale), str(timed)], timeout=limit)
    except subprocess.TimeoutExpired:
        print(f"R-MAT-{scale}: no result within {limit:.0f} s; stopping", flush=True)
        sys.exit(124)
    if r.returncode != 0:
        print(f"R-MAT-{scale}: exit status {r.returncode}; stopping", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
