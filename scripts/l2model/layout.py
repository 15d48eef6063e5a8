"""x~ layout model (pagerank.hip build_x_layout): (window, 128-B x~ line) pairs and the misses
of the 8 LRU L2s for the production packed schedule, with x~ of the vertices past a cut stored
in (largest neighbour window, second largest, id) order inside ranges of `span` windows.

usage: layout.py SCALE WIN_BITS CUT LAYOUT...   (after mk24.py SCALE; l2sim3 built in /tmp/ana)
LAYOUT: id (today), rand (control: the tail shuffled), or a span (1, 4, ...; 0 = the whole tail).
The schedule replayed is the entry-dealt one of build_items: windows, or equal shares of a window
above 1.5 x E / (blocks x 4) entries, groups of 128 consecutive items dealt to the 8 queues by
entries (the measured-cost re-deal is not modelled); blocks = 256 from 16K windows, else 512."""
import subprocess
import sys

import numpy as np

sc, wb, cut = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
src = np.load(f"/tmp/ana/src{sc}.npy")
dst = np.load(f"/tmp/ana/dst{sc}.npy")
nv = int(max(src.max(), dst.max())) + 1
E, U, W = src.size, 8192, 1 << wb
cut = -(-cut // W) * W
nblk = 256 if wb >= 14 else 512
win = (dst >> wb).astype(np.int64)
nwin = int(win.max()) + 1

# the two largest neighbour windows of every vertex (rows are sorted: its last two entries)
k = (src.astype(np.int64) << 32) | dst
k.sort()
s_sorted, d_sorted = (k >> 32).astype(np.int32), (k & 0xFFFFFFFF).astype(np.int32)
del k
row_end = np.searchsorted(s_sorted, np.arange(nv), side="right")
row_beg = np.searchsorted(s_sorted, np.arange(nv), side="left")
deg = row_end - row_beg
w1 = np.where(deg > 0, d_sorted[np.maximum(row_end - 1, 0)] >> wb, 0).astype(np.int64)
w2 = np.where(deg > 1, d_sorted[np.maximum(row_end - 2, 0)] >> wb, 0).astype(np.int64)
del s_sorted, d_sorted


def positions(layout):
    pos = np.arange(nv, dtype=np.int64)
    if layout == "id" or cut >= nv:
        return pos
    tail = np.arange(cut, nv)
    if layout == "rand":
        pos[tail] = cut + np.random.default_rng(1).permutation(tail.size)
        return pos
    span = int(layout)
    rng = (tail - cut) // (span * W) if span else np.zeros(tail.size, np.int64)
    order = np.lexsort((tail, w2[tail], w1[tail], rng))  # stable: ties by id
    pos[tail[order]] = cut + np.arange(tail.size)
    return pos


for layout in sys.argv[4:]:
    ss = positions(layout)[src]
    key = (win << 32) | ss
    key.sort()
    ws = (key >> 32).astype(np.int32)
    ss = (key & 0xFFFFFFFF).astype(np.int32)
    del key
    pairs = np.unique((ws.astype(np.int64) << 24) | (ss >> 5))
    tail_pairs = int(((pairs & ((1 << 24) - 1)) >= (cut >> 5)).sum())
    wstart = np.searchsorted(ws, np.arange(nwin + 1))
    tg = max(U, E // (nblk * 4))
    it = []
    for w in range(nwin):
        a, b = int(wstart[w]), int(wstart[w + 1])
        if b == a:
            continue
        n = max(1, (b - a + tg // 2) // tg)
        cuts = np.linspace(a, b, n + 1).astype(np.int64)
        it += [(cuts[i], cuts[i + 1]) for i in range(n) if cuts[i + 1] > cuts[i]]
    it = np.array(it, np.int64)
    G = 128
    ng = -(-len(it) // G)
    gsz = np.array([(it[g * G:(g + 1) * G, 1] - it[g * G:(g + 1) * G, 0]).sum() for g in range(ng)])
    load, gx = np.zeros(8), np.zeros(ng, int)
    for g in np.argsort(-gsz, kind="stable"):
        gx[g] = int(np.argmin(load))
        load[gx[g]] += gsz[g]
    items = np.array([(a, b, gx[i // G]) for i, (a, b) in enumerate(it)], np.int64)
    ss.tofile("/tmp/ana/s.bin")
    items.tofile("/tmp/ana/t3.bin")
    sim = subprocess.run(["/tmp/ana/l2sim3", "/tmp/ana/s.bin", "/tmp/ana/t3.bin", str(nv), str(U), "32768", "-1", "64",
                          str(nblk)], capture_output=True, text=True).stdout.strip()
    print(f"RMAT-{sc} wb {wb} cut {cut} layout {layout}: pairs {pairs.size / 1e6:.2f} M, tail pairs "
          f"{tail_pairs / 1e6:.2f} M, items {len(items)}; {sim}", flush=True)
