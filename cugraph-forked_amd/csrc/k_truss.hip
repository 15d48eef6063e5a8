// k-truss subgraph: edge peeling by triangle support over the symmetric adjacency.
//
// Reference: community/legacy/ktruss.cu and python community/ktruss_subgraph.py (semantics), the C
// names of later releases (c_api/k_truss.cpp, induced_subgraph_result).  The k-truss is the maximal
// subgraph in which every edge lies in at least k - 2 triangles of the subgraph (the reference's
// convention and networkx.k_truss's); k <= 2 keeps every edge.  The work is done on the underlying
// simple graph, as core_number.hip does: a self-loop or a repeated row entry neither forms nor
// counts a triangle and is not emitted; a repeated entry is represented by its first stored copy.
// The result is the surviving stored edges, both directions, in the order of the rows; it is integer
// work throughout, so no option and no schedule changes it.  DESIGN.md, k-truss.
//
// What does not depend on k is built on the first call and kept on the adjacency (as tc_ooff and
// sim_deg are):
//   * the simple rows: a count pass flags a row that holds a loop or a repeat; without one the
//     adjacency's rows are used as they are, else the kept entries are compacted into a copy that
//     remembers the stored position of each;
//   * edge ids: rows ascend, so the entries of row u above u are its tail.  Edge (u, v), u < v, gets
//     id ubase[u] + (its place in that tail), ubase the prefix sum of the tail sizes.  eid[] holds
//     the id at every position of the simple rows: the position of u in row v finds v's place in
//     row u's tail by a search, so both directions carry the same id.  esrc / epos give u and the
//     position of v in row u back from an id;
//   * supports: sup[e] = |N(u) & N(v)| over the simple rows, one intersection per edge with
//     intersect.hpp's isect_merge / isect_wave_count and isect_ignore, binned as similarity.hip bins
//     its pairs (thread, wave, and the split tier for an edge between two hub rows).  Only the split
//     tier adds with atomics.  32 bits: a support is below the largest degree.
//
// The peel (t = k - 2) is round-synchronous and device-driven like core_number.hip's.  Per edge:
// sup[e], and round[e] = 0 while the edge is alive, else the round in which it was put on a frontier.
// A scan puts every edge with sup < t on frontier 1.  Round r takes every frontier edge e = (u, v)
// and intersects rows u and v with the position-reporting forms; a common w gives e1 = (u, w) and
// e2 = (v, w) from eid[] at the two positions.
//   * 0 < round[e1] < r or 0 < round[e2] < r: the triangle was destroyed in an earlier round, skip;
//   * of the triangle's edges with round == r only the one with the smallest id acts, so a triangle
//     that loses two or three edges in one round is subtracted once;
//   * the acting edge does fetch_sub(sup[x], 1) for each x of e1, e2 with round[x] != r; the
//     subtraction that sees old == t stores round[x] = r + 1 and appends x to the next frontier.
// round values <= r are final before round r is launched (they were stored by earlier launches); a
// value r + 1 read during round r means "alive", as 0 does, and both are treated alike.
//
// Why an edge is put on a frontier exactly once, and exactly when its support falls below t:
//   * between rounds, every alive edge x (round 0) has sup[x] >= t and sup[x] = its triangles whose
//     three edges are all alive.  True after the scan (sup < t went to frontier 1; the initial
//     supports count every triangle).  In round r every triangle that is alive at its start and has
//     an edge on frontier r has exactly one acting edge, which subtracts one from each of its edges
//     not on the frontier: each alive edge loses one per triangle it loses;
//   * every operation on sup[x] after the support pass is a fetch_sub of 1, so the values the
//     operations see are distinct and descending: at most one sees old == t, and one does as soon as
//     the value falls from t to t - 1.  An edge the scan took had sup < t from the start, so no
//     subtraction ever sees t for it; it is on frontier 1 only;
//   * an edge with round r + 1 may still be subtracted from during round r (other triangles of it die
//     in the same round); those see old < t and do nothing else.  From round r + 1 on nothing touches
//     it: on its own frontier round == r, afterwards every triangle of it is skipped.
// An edge is appended at most once in the whole call, so a frontier list of as many entries as there
// are edges never overflows.
//
// Rounds (all on the handle's stream): items (thread and wave tiers, hub-hub edges listed), split
// (a wave per segment of a listed edge's shorter row), control.  The host enqueues kKtChunkRounds of
// them and reads the state block once per chunk; rounds after the end return at once.  Grids are
// fixed and stride over counts read from the state block.  A frontier edge is binned as
// triangle_count.hip bins an oriented edge: the thread merges when both rows are below
// kIsectWaveLen, otherwise the wave probes the longer row (staged in LDS when it fits and pays) with
// the shorter one's entries; an edge whose shorter row has kKtSplitMin entries or more goes to the
// split tier.  Appends cost one counter add per group of lanes that arrive together (a wave in the
// wave tiers).  Only vector stores and ordinary atomics are used.
//
// Extraction: row_extract.hpp over the positions whose edge is alive (kt_rows).
#include "capi.hpp"
#include "intersect.hpp"
#include "prims.hpp"
#include "row_extract.hpp"

#include <algorithm>
#include <climits>

namespace cgx {

namespace {

constexpr int kKtBlock        = kIsectBlock;
constexpr int kKtSplitMin     = 1024;  // an edge whose shorter row has this many entries or more: the split tier
constexpr int kKtSegBits      = 39;    // heavy word: segments in the low bits (sim_seg_len), list position above
constexpr int kKtGridPerCu    = 8;
constexpr int kKtChunkRounds  = 16;    // rounds enqueued per host read
constexpr size_t kKtChunk     = (size_t)1 << 24;  // support pass: edges per launch
constexpr int64_t kKtHeavyMax = (int64_t)1 << 24;  // listed edges per launch the heavy word's high bits can number;
                                                   // a graph with more hub-hub edges leaves them to the wave tier

struct kt_heavy {
  long long edge;
  long long first;  // its first segment number
};

struct kt_state {
  unsigned long long nf[2];  // frontier sizes
  count_t heavy_word;        // (listed edges << kKtSegBits) | segments, of this round
  unsigned long long rounds; // rounds that had a frontier
  unsigned r;                // the round being peeled, from 1
  int fp;                    // the current frontier
  int done;
  int bad;                   // an append past a list's end (cannot happen; never written past it)
};

template <typename V, typename E>
struct kt_args {
  E const* off;   // the simple rows
  V const* idx;
  E const* eid;
  V const* esrc;
  E const* epos;
  int* sup;
  unsigned* round;
  E* front[2];    // m entries each
  long long m;    // edges
  int t;          // k - 2
  kt_heavy* heavy;
  unsigned long long heavy_cap;
  kt_state* st;
  int path;       // tuning_t::kt_path
  int split;      // the split tier is on
};

// ---------------------------------------------------------------- simple rows, edge ids
// A wave per row: the entries that are neither the row's own vertex nor a repeat of the entry before
// them are counted (kidx == nullptr: len[v], and *dirty when a row drops an entry) or written in their
// order to kidx / korig from koff[v] on.
template <typename V, typename E>
__global__ __launch_bounds__(kKtBlock) void k_kt_clean(E const* off, V const* idx, int64_t nv, E const* koff, E* len,
                                                      int* dirty, V* kidx, E* korig)
{
  int const lane          = threadIdx.x & 63;
  int64_t const wave      = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  int64_t const num_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t v = wave; v < nv; v += num_waves) {
    long long const b = (long long)off[v], e = (long long)off[v + 1];
    long long kept    = 0;  // wave-uniform
    for (long long j0 = b; j0 < e; j0 += 64) {
      long long const j = j0 + lane;
      bool keep         = false;
      V w               = 0;
      if (j < e) {
        w    = idx[j];
        keep = (int64_t)w != v && (j == b || idx[j - 1] != w);
      }
      unsigned long long const m = __ballot(keep);
      if (kidx && keep) {
        long long const q = (long long)koff[v] + kept + __popcll(m & ((1ull << lane) - 1ull));
        kidx[q]           = w;
        korig[q]          = (E)j;
      }
      kept += __popcll(m);
    }
    if (!kidx && lane == 0) {
      len[v] = (E)kept;
      if (kept != e - b) atomicOr(dirty, 1);
    }
  }
}

// ucnt[v] = entries of simple row v above v (its tail: rows ascend and hold no v)
template <typename V, typename E>
__global__ __launch_bounds__(kKtBlock) void k_kt_upper(E const* off, V const* idx, int64_t nv, E* ucnt)
{
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) {
    E lo = off[v], hi = off[v + 1];
    E const e = hi;
    while (lo < hi) {
      E const mid = lo + ((hi - lo) >> 1);
      if ((int64_t)idx[mid] < v) lo = mid + 1;
      else hi = mid;
    }
    ucnt[v] = e - lo;
  }
}

// A wave per row u: eid at every position; esrc / epos of the edges u owns (the entries above u).
// info[0]: a position whose reverse entry is missing (the graph is not symmetric); info[1]: edges whose
// two rows both have kKtSplitMin entries or more.
template <typename V, typename E>
__global__ __launch_bounds__(kKtBlock) void k_kt_eid(E const* off, V const* idx, int64_t nv, E const* ubase, E* eid,
                                                    V* esrc, E* epos, unsigned long long* info)
{
  int const lane          = threadIdx.x & 63;
  int64_t const wave      = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  int64_t const num_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  unsigned long long heavy = 0;
  bool bad                 = false;
  for (int64_t u = wave; u < nv; u += num_waves) {
    long long const b = (long long)off[u], e = (long long)off[u + 1];
    long long const ub = (long long)ubase[u];
    long long const tail = e - ((long long)ubase[u + 1] - ub);  // the first position above u
    for (long long j = b + lane; j < e; j += 64) {
      long long const v = (long long)idx[j];
      if (j >= tail) {
        long long const id = ub + (j - tail);
        eid[j]             = (E)id;
        esrc[id]           = (V)u;
        epos[id]           = (E)j;
        if (e - b >= kKtSplitMin && (long long)off[v + 1] - (long long)off[v] >= kKtSplitMin) ++heavy;
      } else {  // v < u: the edge is row v's; u lies in that row's tail
        long long const vb = (long long)off[v], ve = (long long)off[v + 1];
        long long const vt = ve - ((long long)ubase[v + 1] - (long long)ubase[v]);
        long long lo = vt, hi = ve;
        while (lo < hi) {
          long long const mid = (lo + hi) >> 1;
          if ((int64_t)idx[mid] < u) lo = mid + 1;
          else hi = mid;
        }
        if (vb <= lo && lo < ve && (int64_t)idx[lo] == u) {
          eid[j] = (E)((long long)ubase[v] + (lo - vt));
        } else {
          eid[j] = 0;
          bad    = true;
        }
      }
    }
  }
  if (bad) __hip_atomic_fetch_or(info, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  heavy = (unsigned long long)wave_sum_ll((long long)heavy);
  if (lane == 0 && heavy) __hip_atomic_fetch_add(info + 1, heavy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- triangles of a frontier edge
// The `hit` of the position-reporting intersections: ea / eb are eid[] at the starts of the two rows.
template <typename E>
struct kt_tri {
  int* sup;
  unsigned* round;
  E* next;
  unsigned long long* nnext;
  unsigned long long cap;
  int* bad;
  E const* ea;
  E const* eb;
  long long e;
  unsigned r;
  int t;
  __device__ __forceinline__ void drop(long long x) const
  {
    int const old = __hip_atomic_fetch_sub(sup + x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == t) {
      __hip_atomic_store(round + x, r + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      list_append(next, nnext, cap, bad, (E)x);
    }
  }
  template <typename V>
  __device__ __forceinline__ void operator()(V, long long i, long long j) const
  {
    long long const e1 = (long long)ea[i], e2 = (long long)eb[j];
    unsigned const r1 = ld_relaxed(round + e1), r2 = ld_relaxed(round + e2);
    if (r1 - 1u < r - 1u || r2 - 1u < r - 1u) return;      // 0 < round < r: destroyed earlier
    if ((r1 == r && e1 < e) || (r2 == r && e2 < e)) return;  // another edge of this round acts
    if (r1 != r) drop(e1);
    if (r2 != r) drop(e2);
  }
};

template <typename V, typename E>
__device__ __forceinline__ kt_tri<E> kt_make_tri(kt_args<V, E> const& a, long long e, unsigned r, long long sa,
                                                long long sb)
{
  int const np = a.st->fp ^ 1;
  return kt_tri<E>{a.sup, a.round, a.front[np], &a.st->nf[np], (unsigned long long)a.m, &a.st->bad,
                   a.eid + sa,  a.eid + sb, e, r, a.t};
}

// One edge per thread and 256-edge chunk.  kPeel: the edges of the current frontier, their triangles
// handled by kt_tri.  Otherwise (the support pass) edges e0 .. e0 + cnt, sup[e] = the intersection's size;
// sup is zero on entry and the edges left to the split tier keep their zero.
template <typename V, typename E, bool kPeel>
__global__ __launch_bounds__(kKtBlock) void k_kt_items(kt_args<V, E> a, long long e0, long long cnt)
{
  kt_state* st = a.st;
  long long n  = cnt;
  E const* F   = nullptr;
  unsigned r   = 0;
  if constexpr (kPeel) {
    if (st->done) return;
    int const fp = st->fp;
    n            = (long long)(st->nf[fp] < (unsigned long long)a.m ? st->nf[fp] : (unsigned long long)a.m);
    F            = a.front[fp];
    r            = st->r;
  }
  int const tid = threadIdx.x, lane = tid & 63;
  V* const stage = isect_stage<V>();
  for (long long k0 = blockIdx.x * (long long)kKtBlock; k0 < n; k0 += (long long)gridDim.x * kKtBlock) {
    long long const k = k0 + tid;
    long long e = 0, a0 = 0, la = 0, b0 = 0, lb = 0;
    bool const work = k < n;
    if (work) {
      e                 = kPeel ? (long long)F[k] : e0 + k;
      long long const u = (long long)a.esrc[e];
      long long const v = (long long)a.idx[a.epos[e]];
      a0                = (long long)a.off[u];
      la                = (long long)a.off[u + 1] - a0;
      b0                = (long long)a.off[v];
      lb                = (long long)a.off[v + 1] - b0;
    }
    long long const ns  = la < lb ? la : lb;
    bool const by_split = work && a.split && a.path == 0 && ns >= kKtSplitMin;
    bool const by_wave =
      work && !by_split && (a.path == 2 || (a.path == 0 && (la >= kIsectWaveLen || lb >= kIsectWaveLen)));
    if (by_split) {
      long long const len  = sim_seg_len(ns);
      count_t const nseg   = (count_t)((ns + len - 1) / len);
      count_t const before = __hip_atomic_fetch_add(&st->heavy_word, ((count_t)1 << kKtSegBits) | nseg,
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      // one add gives the position and the segment number together: positions ascend with them
      count_t const pos = before >> kKtSegBits;
      if (pos < a.heavy_cap) a.heavy[pos] = kt_heavy{e, (long long)(before & (((count_t)1 << kKtSegBits) - 1))};
      else atomicOr(&st->bad, 1);
    } else if (work && !by_wave) {
      if constexpr (kPeel) isect_merge_at<V>(a.idx + a0, la, a.idx + b0, lb, kt_make_tri<V, E>(a, e, r, a0, b0));
      else a.sup[e] = (int)isect_merge<V>(a.idx + a0, la, a.idx + b0, lb, isect_ignore{});
    }
    // the edges left to the wave, one after the other
    unsigned long long m = __ballot(by_wave);
    while (m) {  // wave-uniform
      int const l = __ffsll((long long)m) - 1;
      m &= m - 1;
      long long const ee = __shfl(e, l, 64);
      long long sa = __shfl(a0, l, 64), nsw = __shfl(la, l, 64);
      long long sb = __shfl(b0, l, 64), nl = __shfl(lb, l, 64);
      isect_shorter_first(sa, nsw, sb, nl);
      if constexpr (kPeel) {
        isect_wave_at<V>(a.idx + sa, 0, nsw, a.idx + sb, nl, stage, kIsectStageDiv, lane,
                         kt_make_tri<V, E>(a, ee, r, sa, sb));
      } else {
        count_t const cw =
          isect_wave_count<V>(a.idx + sa, 0, nsw, a.idx + sb, nl, stage, kIsectStageDiv, lane, isect_ignore{});
        if (lane == 0) a.sup[ee] = (int)cw;
      }
    }
  }
}

// A wave per segment of the listed edges' shorter rows.  heavy_word holds (edges << kKtSegBits | segments).
template <typename V, typename E, bool kPeel>
__global__ __launch_bounds__(kKtBlock) void k_kt_split(kt_args<V, E> a)
{
  kt_state* st = a.st;
  if ((kPeel && st->done) || st->bad) return;
  int const tid = threadIdx.x, lane = tid & 63;
  V* const stage         = isect_stage<V>();
  count_t const word     = st->heavy_word;
  long long const nlist  = (long long)(word >> kKtSegBits);
  long long const nsegs  = (long long)(word & (((count_t)1 << kKtSegBits) - 1));
  if (nlist == 0) return;
  unsigned const r       = st->r;
  long long const wave   = (blockIdx.x * (long long)blockDim.x + tid) >> 6;
  long long const nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long sgm = wave; sgm < nsegs; sgm += nwaves) {  // wave-uniform
    // the last list entry whose first segment is not above sgm (heavy[0].first == 0)
    long long lo = 0, hi = nlist - 1;
    while (lo < hi) {
      long long const mid = (lo + hi + 1) >> 1;
      if (a.heavy[mid].first <= sgm) lo = mid;
      else hi = mid - 1;
    }
    kt_heavy const hp = a.heavy[lo];
    long long const u = (long long)a.esrc[hp.edge];
    long long const v = (long long)a.idx[a.epos[hp.edge]];
    long long sa = (long long)a.off[u], ns = (long long)a.off[u + 1] - sa;
    long long sb = (long long)a.off[v], nl = (long long)a.off[v + 1] - sb;
    isect_shorter_first(sa, ns, sb, nl);
    long long const len = sim_seg_len(ns);
    long long const s0  = (sgm - hp.first) * len;
    long long const s1  = s0 + len < ns ? s0 + len : ns;
    if (s0 >= s1) continue;
    if constexpr (kPeel) {
      isect_wave_at<V>(a.idx + sa, s0, s1, a.idx + sb, nl, stage, kIsectStageDiv, lane,
                       kt_make_tri<V, E>(a, hp.edge, r, sa, sb));
    } else {
      count_t const cw =
        isect_wave_count<V>(a.idx + sa, s0, s1, a.idx + sb, nl, stage, kIsectStageDiv, lane, isect_ignore{});
      if (lane == 0 && cw) __hip_atomic_fetch_add(a.sup + hp.edge, (int)cw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// ---------------------------------------------------------------- peel: start, control
__global__ void k_kt_init(kt_state* st)
{
  kt_state s{};
  s.r = 1;
  *st = s;
}

// frontier 1: every edge whose support is below t
template <typename V, typename E>
__global__ __launch_bounds__(kKtBlock) void k_kt_scan(kt_args<V, E> a)
{
  kt_state* st = a.st;
  for (long long e = blockIdx.x * (long long)kKtBlock + threadIdx.x; e < a.m; e += (long long)gridDim.x * kKtBlock)
    if (a.sup[e] < a.t) {
      a.round[e] = 1u;
      list_append(a.front[0], &st->nf[0], (unsigned long long)a.m, &st->bad, (E)e);
    }
}

__global__ void k_kt_ctl(kt_state* st)
{
  if (st->done) return;
  int const fp = st->fp;
  if (st->nf[fp]) ++st->rounds;
  st->nf[fp]     = 0;
  st->heavy_word = 0;
  st->fp         = fp ^ 1;
  ++st->r;
  if (st->bad || st->nf[fp ^ 1] == 0) st->done = 1;
}

// ---------------------------------------------------------------- extraction
template <typename E>
__device__ __forceinline__ bool kt_alive(E const* eid, unsigned const* round, long long j)
{
  return !round || round[eid[j]] == 0u;
}

// row_extract.hpp's test: every simple row, its positions whose edge is alive (round == nullptr: all of
// them).  orig: the stored position of every entry of a cleaned copy (nullptr: the position itself).
template <typename E>
struct kt_rows {
  E const* eid;
  unsigned const* round;
  E const* orig;
  __device__ __forceinline__ bool row(int64_t) const { return true; }
  __device__ __forceinline__ bool keep(int64_t, long long, long long j) const { return kt_alive(eid, round, j); }
  __device__ __forceinline__ long long wpos(long long j) const { return orig ? (long long)orig[j] : j; }
};

inline unsigned kt_grid() { return (unsigned)(std::max(device_cu_count(), 1) * kKtGridPerCu); }

// The simple rows, the edge ids and the supports of `adj`, once.
template <typename V, typename E>
void kt_build(handle_t& h, graph_t& g, adjacency_t& adj)
{
  if (adj.kt_valid) return;
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  E const* off     = adj.offsets.data<E>();
  V const* idx     = adj.indices.data<V>();
  unsigned const row_grid = grid_for((size_t)nv * 64, kKtBlock, 1u << 16);

  // simple rows
  buffer koff, kidx, korig;
  bool clean = true;
  {
    dbuf<E> len((size_t)nv + 1, s);
    dbuf<int> dirty(1, s);
    HIP_CHECK(hipMemsetAsync(len.data() + nv, 0, sizeof(E), s));
    HIP_CHECK(hipMemsetAsync(dirty.data(), 0, sizeof(int), s));
    hipLaunchKernelGGL((k_kt_clean<V, E>), dim3(row_grid), dim3(kKtBlock), 0, s, off, idx, nv, (E const*)nullptr,
                       len.data(), dirty.data(), (V*)nullptr, (E*)nullptr);
    CGX_LAUNCH_CHECK();
    clean = to_host_scalar(dirty.data(), s) == 0;
    if (!clean) {
      koff.resize(((size_t)nv + 1) * sizeof(E), s);
      exclusive_scan<E, E>(len.data(), koff.data<E>(), (size_t)nv + 1, s);
      size_t const kept = (size_t)to_host_scalar(koff.data<E>() + nv, s);
      kidx.resize(std::max<size_t>(kept, 1) * sizeof(V), s);
      korig.resize(std::max<size_t>(kept, 1) * sizeof(E), s);
      hipLaunchKernelGGL((k_kt_clean<V, E>), dim3(row_grid), dim3(kKtBlock), 0, s, off, idx, nv,
                         (E const*)koff.data<E>(), (E*)nullptr, (int*)nullptr, kidx.data<V>(), korig.data<E>());
      CGX_LAUNCH_CHECK();
      off = koff.data<E>();
      idx = kidx.data<V>();
    }
  }
  size_t const entries = clean ? (size_t)g.num_edges : (size_t)to_host_scalar(off + nv, s);

  // edge ids
  dbuf<E> ucnt((size_t)nv + 1, s);
  buffer ubase(((size_t)nv + 1) * sizeof(E), s);
  HIP_CHECK(hipMemsetAsync(ucnt.data() + nv, 0, sizeof(E), s));
  hipLaunchKernelGGL((k_kt_upper<V, E>), dim3(grid_for((size_t)nv, kKtBlock, 1u << 16)), dim3(kKtBlock), 0, s, off, idx,
                     nv, ucnt.data());
  CGX_LAUNCH_CHECK();
  exclusive_scan<E, E>(ucnt.data(), ubase.data<E>(), (size_t)nv + 1, s);
  int64_t const m = (int64_t)to_host_scalar(ubase.data<E>() + nv, s);
  // an undirected simple graph stores every edge twice
  CGX_INPUT((size_t)m * 2 == entries, "Invalid input argument: k_truss_subgraph needs a symmetric graph.");
  buffer eid(std::max<size_t>(entries, 1) * sizeof(E), s);
  buffer esrc(std::max<size_t>((size_t)m, 1) * sizeof(V), s);
  buffer epos(std::max<size_t>((size_t)m, 1) * sizeof(E), s);
  buffer sup(std::max<size_t>((size_t)m, 1) * sizeof(int), s);
  int64_t heavy_edges = 0;
  if (m > 0) {
    dbuf<unsigned long long> info(2, s);
    HIP_CHECK(hipMemsetAsync(info.data(), 0, 2 * sizeof(unsigned long long), s));
    hipLaunchKernelGGL((k_kt_eid<V, E>), dim3(row_grid), dim3(kKtBlock), 0, s, off, idx, nv,
                       (E const*)ubase.data<E>(), eid.data<E>(), esrc.data<V>(), epos.data<E>(), info.data());
    CGX_LAUNCH_CHECK();
    auto const hi = to_host(info.data(), 2, s);
    CGX_INPUT(hi[0] == 0, "Invalid input argument: k_truss_subgraph needs a symmetric graph.");
    heavy_edges = (int64_t)hi[1];

    // supports
    bool const split       = heavy_edges > 0 && heavy_edges <= kKtHeavyMax;
    size_t const chunk     = std::min((size_t)m, kKtChunk);
    size_t const heavy_cap = split ? std::min((size_t)heavy_edges, chunk) : 0;
    dbuf<kt_heavy> heavy(std::max<size_t>(heavy_cap, 1), s);
    dbuf<kt_state> st(1, s);
    HIP_CHECK(hipMemsetAsync(sup.data(), 0, (size_t)m * sizeof(int), s));
    kt_args<V, E> a{};
    a.off       = off;
    a.idx       = idx;
    a.eid       = eid.data<E>();
    a.esrc      = esrc.data<V>();
    a.epos      = epos.data<E>();
    a.sup       = sup.data<int>();
    a.m         = (long long)m;
    a.heavy     = heavy.data();
    a.heavy_cap = (unsigned long long)heavy_cap;
    a.st        = st.data();
    a.path      = h.tune.kt_path;
    a.split     = split ? 1 : 0;
    for (size_t p0 = 0; p0 < (size_t)m; p0 += chunk) {
      size_t const c = std::min(chunk, (size_t)m - p0);
      hipLaunchKernelGGL(k_kt_init, dim3(1), dim3(1), 0, s, st.data());
      hipLaunchKernelGGL((k_kt_items<V, E, false>), dim3(grid_for(c, kKtBlock, kt_grid())), dim3(kKtBlock), 0, s, a,
                         (long long)p0, (long long)c);
      // the list's length stays on the device; an empty list ends the launch at once
      hipLaunchKernelGGL((k_kt_split<V, E, false>), dim3(kt_grid()), dim3(kKtBlock), 0, s, a);
      CGX_LAUNCH_CHECK();
      // (the state block is read per chunk: the next chunk's init clears it)
      CGX_EXPECTS(to_host_scalar(&st.data()->bad, s) == 0, CUGRAPH_UNKNOWN_ERROR,
                  "k_truss: the support pass's edge list overflowed");
    }
  }
  adj.kt_clean = clean;
  adj.kt_edges = m;
  adj.kt_heavy = heavy_edges;
  adj.kt_off   = std::move(koff);
  adj.kt_idx   = std::move(kidx);
  adj.kt_orig  = std::move(korig);
  adj.kt_eid   = std::move(eid);
  adj.kt_esrc  = std::move(esrc);
  adj.kt_epos  = std::move(epos);
  adj.kt_sup   = std::move(sup);
  adj.kt_valid = true;
}

template <typename V, typename E, typename W>
void kt_impl(handle_t& h, graph_t& g, size_t k, induced_subgraph_result_t& res)
{
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  reset_hot(h);
  auto finish = [&](size_t total) {  // the one subgraph's offsets
    res.offsets = std::make_unique<device_array_t>(2, INT64, s);
    int64_t const two[2] = {0, (int64_t)total};
    HIP_CHECK(hipMemcpyAsync(res.offsets->buf.data(), two, sizeof(two), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));  // `two` is read by then
  };
  auto empty = [&] {
    alloc_edge_arrays(g, 0, s, res.src, res.dst, res.weights);
    finish(0);
  };
  if (nv == 0 || g.num_edges == 0) return empty();
  adjacency_t& adj = ensure_adjacency(h, g, g.store_transposed);  // symmetric: either orientation
  kt_build<V, E>(h, g, adj);
  int64_t const m = adj.kt_edges;
  if (m == 0) return empty();
  E const* off  = adj.kt_clean ? adj.offsets.data<E>() : adj.kt_off.data<E>();
  V const* idx  = adj.kt_clean ? adj.indices.data<V>() : adj.kt_idx.data<V>();
  E const* orig = adj.kt_clean ? nullptr : adj.kt_orig.data<E>();
  E const* eid  = adj.kt_eid.data<E>();

  // ---- peel
  dbuf<unsigned> round;
  if (k > 2) {
    dbuf<int> sup((size_t)m, s);
    dbuf<E> lists((size_t)m * 2, s);
    bool const split       = adj.kt_heavy > 0 && adj.kt_heavy <= kKtHeavyMax;
    size_t const heavy_cap = split ? (size_t)adj.kt_heavy : 0;
    dbuf<kt_heavy> heavy(std::max<size_t>(heavy_cap, 1), s);
    dbuf<kt_state> st(1, s);
    round.resize((size_t)m, s);
    HIP_CHECK(hipMemcpyAsync(sup.data(), adj.kt_sup.data(), (size_t)m * sizeof(int), hipMemcpyDeviceToDevice, s));
    HIP_CHECK(hipMemsetAsync(round.data(), 0, (size_t)m * sizeof(unsigned), s));
    kt_args<V, E> a{};
    a.off       = off;
    a.idx       = idx;
    a.eid       = eid;
    a.esrc      = adj.kt_esrc.data<V>();
    a.epos      = adj.kt_epos.data<E>();
    a.sup       = sup.data();
    a.round     = round.data();
    a.front[0]  = lists.data();
    a.front[1]  = lists.data() + m;
    a.m         = (long long)m;
    a.t         = (int)std::min<size_t>(k - 2, (size_t)INT_MAX);  // supports are below INT_MAX
    a.heavy     = heavy.data();
    a.heavy_cap = (unsigned long long)heavy_cap;
    a.st        = st.data();
    a.path      = h.tune.kt_path;
    a.split     = split ? 1 : 0;
    unsigned const grid = kt_grid();
    hipLaunchKernelGGL(k_kt_init, dim3(1), dim3(1), 0, s, st.data());
    hipLaunchKernelGGL((k_kt_scan<V, E>), dim3(grid_for((size_t)m, kKtBlock, grid)), dim3(kKtBlock), 0, s, a);
    CGX_LAUNCH_CHECK();
    auto* hs = h.pinned_as<kt_state>();
    // every round before the last peels an edge
    unsigned long long const round_cap = (unsigned long long)m + 2ull;
    size_t launches = 1;
    chunk_timer timer{h, s};  // one interval per round, folded after every chunk's read
    while (true) {
      for (int i = 0; i < kKtChunkRounds; ++i) {
        timer.begin();
        hipLaunchKernelGGL((k_kt_items<V, E, true>), dim3(grid), dim3(kKtBlock), 0, s, a, 0ll, 0ll);
        hipLaunchKernelGGL((k_kt_split<V, E, true>), dim3(grid), dim3(kKtBlock), 0, s, a);
        timer.end();
        hipLaunchKernelGGL(k_kt_ctl, dim3(1), dim3(1), 0, s, st.data());
        CGX_LAUNCH_CHECK();
      }
      launches += 2 * (size_t)kKtChunkRounds;
      HIP_CHECK(hipMemcpyAsync(hs, st.data(), sizeof(kt_state), hipMemcpyDeviceToHost, s));
      HIP_CHECK(hipStreamSynchronize(s));
      timer.fold();
      CGX_EXPECTS(!hs->bad, CUGRAPH_UNKNOWN_ERROR, "k_truss: an edge list overflowed");
      if (hs->done) break;
      CGX_EXPECTS(hs->rounds <= round_cap && hs->r < 0xfffffff0u, CUGRAPH_UNKNOWN_ERROR,
                  "k_truss: more rounds than edges allow");
    }
    h.last_iterations = (size_t)hs->rounds;
    timer.report(launches);
  }

  // ---- extraction
  kt_rows<E> const alive{eid, k > 2 ? round.data() : nullptr, orig};
  finish(extract_rows(h, g, off, idx, g.weighted ? adj.weights.data<W>() : (W const*)nullptr, alive, res.src, res.dst,
                      res.weights));
}

}  // namespace

void run_k_truss(handle_t& h, graph_t& g, size_t k, induced_subgraph_result_t& res)
{
  dispatch_vew(g.vertex_type, g.edge_type, g.weight_type, [&](auto t) {
    using T = decltype(t);
    kt_impl<typename T::vertex_t, typename T::edge_t, typename T::weight_t>(h, g, k, res);
  });
}

}  // namespace cgx
