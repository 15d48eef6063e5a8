"""Write profiles/r01_bench.md from profiles/r01_bench_n1.json + r01_bench_kernel_stats.csv."""
import csv
import json
import re
import sys

tag = sys.argv[1] if len(sys.argv) > 1 else "r01"
d = json.loads(open(f"profiles/{tag}_bench_n1.json").read())
rows = list(csv.DictReader(open(f"profiles/{tag}_bench_kernel_stats.csv")))
r = d["roofline"]


def short(n):
    n = n.replace("rocprim::ROCPRIM_400200_NS::detail::", "").replace("cgx::(anonymous namespace)::", "")
    return n.replace("void ", "")[:90]


# the headline's kernels: from 2^23 vertices the 16K-window push with the apply fused in
# (no k_pr_apply launch; the k_pr_apply / k_pr_push16 launches in the run are RMAT-22's)
fused = any("k_pr_push16_w14" in x["Name"] for x in rows)
push = next(x for x in rows if ("k_pr_push16_w14" if fused else "k_pr_push") in x["Name"])
app = None if fused else next((x for x in rows if "k_pr_apply" in x["Name"]), None)


def live_avg_ns(kernel):
    """Average launch of a PageRank kernel from the per-launch trace extract
    (profiles/<tag>_pr_launches.csv), dropping the post-convergence no-op launches
    (below 10 % of the median): the stats CSV averages them in."""
    try:
        d = [float(r["duration_ns"]) for r in csv.DictReader(open(f"profiles/{tag}_pr_launches.csv"))
             if r["kernel"] == kernel]
    except OSError:
        return None, 0, 0
    if not d:
        return None, 0, 0
    med = sorted(d)[len(d) // 2]
    live = [x for x in d if x >= 0.1 * med]
    live_med[kernel] = sorted(live)[len(live) // 2]
    return sum(live) / len(live), len(live), len(d)


live_med = {}


push_live, push_n, push_all = live_avg_ns("k_pr_push16_w14" if fused else "k_pr_push16")
app_live, _, _ = (None, 0, 0) if fused else live_avg_ns("k_pr_apply")
push_ns = push_live if push_live else float(push["AverageNs"])
app_ns = app_live if app_live else (float(app["AverageNs"]) if app else 0.0)
pa = (push_ns + app_ns) / 1e3
ev = r["avg_kernel_ms"] * 1e3
out = [
    f"# Profile {tag}: `bench.py` on one MI355X",
    "",
    f"Sources:",
    f"- `profiles/{tag}_bench_n1.json`: the bench line from `python bench.py --full` (default legs).",
    f"- `profiles/{tag}_bench_kernel_stats.csv`: `rocprofv3 --kernel-trace --stats -- python3 bench.py --full --no-traffic",
    "  --no-cpu-baseline` (`scripts/gpu_round.sh`). Graph construction is in the trace but in no timed region.",
    f"- `profiles/{tag}_louvain_launches.md`, `profiles/{tag}_sssp_kernels.md`, `profiles/{tag}_pr_launches.csv`: per-launch",
    "  extracts of the same run's kernel trace (`scripts/round_extracts.py`), where present.",
    "",
    "## PageRank iteration (the roofline kernel pair)",
    "",
    "| kernel | launches | avg µs (rocprof) |",
    "|---|---|---|",
    f"| `{short(push['Name']).split('(')[0]}` | {push['Calls']} | {float(push['AverageNs']) / 1e3:.1f} |",
] + ([f"| `{short(app['Name']).split('(')[0]}` | {app['Calls']} | {float(app['AverageNs']) / 1e3:.1f} |"] if app else []) + [
    "",
    (f"- Without the post-convergence no-op launches ({push_all - push_n} of {push_all} push launches under 10 % of "
     f"the median, from `profiles/{tag}_pr_launches.csv`): push {push_ns / 1e3:.1f} µs, apply {app_ns / 1e3:.1f} µs."
     if push_live else "- (no per-launch trace extract: averages include the no-op launches)"),
    (f"- Median live push launch {live_med.get('k_pr_push16_w14' if fused else 'k_pr_push16', 0) / 1e3:.1f} µs: the average also holds each "
     "graph's first chunk, which runs before the queues are re-dealt by measured cost." if push_live else ""),
    f"- rocprof push{'' if fused else ' + apply'} = {pa:.1f} µs per iteration{' (apply fused into the push)' if fused else ''}. The bench's HIP events around the launches (gap",
    f"  included) give {ev:.1f} µs; the two agree within {abs(ev - pa) / pa * 100:.1f} %.",
    f"- Algorithmic bytes per iteration: 4E + 16V = {r['algorithmic_bytes_per_launch'] / 1e6:.1f} MB, giving {r['achieved']:.0f} GB/s =",
    f"  **{r['frac'] * 100:.1f} % of 8 TB/s**.",
    f"- Measured HBM traffic per iteration (2×FETCH_SIZE + WRITE_SIZE, separate PMC passes) = {r['traffic'] / 1e6:.0f} MB,",
    f"  i.e. {r['traffic'] / (r['avg_kernel_ms'] * 1e-3) / 1e12:.2f} TB/s actually moved. The measured stream-copy ceiling",
    f"  (4 GiB device copy) is {r.get('copy_ceiling_gbs', r.get('stream_copy_gbs', 0)) / 1e3:.2f} TB/s.",
    "",
    "## Other legs",
    "",
    f"- BFS RMAT-24: {d['bfs']['mteps_harmonic_mean']:.0f} MTEPS harmonic mean (Graph500 counting),",
    f"  {d['bfs']['stored_edge_mteps_harmonic_mean']:.0f} stored-edge MTEPS, {d['bfs']['ms_mean']:.2f} ms per traversal.",
    f"  NetworkX: {d['bfs'].get('cpu_baseline', {}).get('value', float('nan')):.2f} MTEPS ({d['bfs'].get('cpu_baseline', {}).get('sample', '')}).",
    f"- Louvain RMAT-23: {d['louvain']['time_s']:.3f} s, Q {d['louvain']['modularity']:.4f}, {d['louvain']['levels']} levels.",
    f"  NetworkX: {d['louvain'].get('cpu_baseline', {}).get('value', float('nan')):.2f} s ({d['louvain'].get('cpu_baseline', {}).get('sample', '')}).",
    f"- PageRank CPU baseline: {d['cpu_baseline']['value']:.3g} edges/s ({d['cpu_baseline']['sample']}).",
    "",
    "## Top kernels of the whole run",
    "",
    "| kernel | calls | avg µs | % |",
    "|---|---|---|---|",
]
for x in rows[:15]:
    out.append(f"| `{short(x['Name'])}` | {x['Calls']} | {float(x['AverageNs']) / 1e3:.1f} | {x['Percentage'][:5]} |")
open(f"profiles/{tag}_bench.md", "w").write("\n".join(out) + "\n")
