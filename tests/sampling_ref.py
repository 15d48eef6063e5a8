"""numpy twin of csrc/sample.hpp, sampling.hip and random_walks.hip: the draw, the hop loop with its slot
numbering, Floyd's sampler, the distinct triples with their counts, and both kinds of walk.  Everything
works in internal ids on a CSR built here by a stable sort on (source, destination), and reproduces the
library bit for bit (include/cugraph_c/sampling_algorithms.h states the contract)."""
import numpy as np

U = np.uint64
GOLDEN = 0x9E3779B97F4A7C15


def sm(x):
    """splitmix64 on uint64 values."""
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=U) + U(GOLDEN)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        return z ^ (z >> U(31))


def draw(seed, stream, i, j):
    key = U(((int(seed) * GOLDEN) & (2**64 - 1)) ^ int(stream))
    return sm(sm(sm(key) ^ np.asarray(i, dtype=U)) ^ np.asarray(j, dtype=U))


def index(r, n):
    """High 64 bits of r * n through 32-bit halves, for n < 2^32."""
    r, n = np.asarray(r, dtype=U), np.asarray(n, dtype=U)
    assert np.all(n < U(2**32))
    hi, lo = r >> U(32), r & U(0xFFFFFFFF)
    return ((hi * n + ((lo * n) >> U(32))) >> U(32)).astype(np.int64)


def unit(r):
    return (np.asarray(r, dtype=U) >> U(11)).astype(np.float64) * 2.0**-53


def build_csr(src, dst, w, nv):
    """(offsets, indices, weights | None), parallel edges in input order."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.lexsort((dst, src))  # stable
    off = np.zeros(nv + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=nv), out=off[1:])
    return off, dst[order], None if w is None else np.asarray(w)[order]


def floyd(seed, hop, i, d, k):
    """Row positions of Robert Floyd's sampler: k distinct values below d, in pick order."""
    t = np.arange(k)
    r = index(draw(seed, hop, i, t), d - k + t + 1)
    seen, out = set(), []
    for tt in range(k):
        p = int(r[tt]) if int(r[tt]) not in seen else d - k + tt
        seen.add(p)
        out.append(p)
    return np.asarray(out, dtype=np.int64)


def neighbor_sample(csr, starts, fan_out, with_replacement, seed=0):
    """(sources, destinations, weights, counts): the distinct triples of all hops, sorted, internal ids;
    weights are ones (float32) without a weight array."""
    off, idx, w = csr
    front, picked = np.asarray(starts, dtype=np.int64), []
    for hop, k in enumerate(fan_out):
        pos = [np.zeros(0, dtype=np.int64)]
        for i, v in enumerate(front):
            rs, d = off[v], off[v + 1] - off[v]
            if d == 0:
                continue
            if k <= 0 or (not with_replacement and d <= k):
                p = np.arange(d)
            elif with_replacement:
                p = index(draw(seed, hop, i, np.arange(k)), d)
            else:
                p = floyd(seed, hop, i, int(d), int(k))
            pos.append(rs + p)
        pos = np.concatenate(pos)
        picked.append(pos)
        front = idx[pos]
    pos = np.concatenate(picked) if picked else np.zeros(0, dtype=np.int64)
    s, d = np.searchsorted(off, pos, side="right") - 1, idx[pos]
    wv = np.ones(len(pos), dtype=np.float32) if w is None else w[pos]
    bits = wv.view(np.int32 if wv.dtype == np.float32 else np.int64).astype(np.int64)
    rows, first, counts = np.unique(np.stack([s, d, bits], axis=1), axis=0, return_index=True, return_counts=True)
    return rows[:, 0], rows[:, 1], wv[first], counts


def walks(csr, starts, max_length, seed=0, biased=False):
    """(paths [n, max_length + 1], weights [n, max_length] | None), internal ids, -1 / 0 after a sink."""
    off, idx, w = csr
    n = len(starts)
    paths = np.full((n, max_length + 1), -1, dtype=np.int64)
    wout = None if w is None else np.zeros((n, max_length), dtype=w.dtype)
    for i, v in enumerate(starts):
        paths[i, 0] = v
        for s in range(max_length):
            rs, d = off[v], off[v + 1] - off[v]
            if d == 0:
                break
            r = draw(seed, s, i, 0)
            if biased:
                cum = np.cumsum(w[rs:rs + d].astype(np.float64))
                if not cum[-1] > 0:
                    break
                p = rs + int(np.searchsorted(cum, unit(r) * cum[-1], side="right"))
            else:
                p = rs + int(index(r, d))
            v = int(idx[p])
            paths[i, s + 1] = v
            if wout is not None:
                wout[i, s] = w[p]
    return paths, wout
