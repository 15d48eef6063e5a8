// Triangle counting: sorted-set intersection over oriented adjacency rows.
//
// Reference: community/triangle_count_impl.cuh (drop self-loops, keep the edges from the
// lower to the higher (degree, id) endpoint, intersect the rows of every kept edge) and
// c_api/triangle_count.cpp.  Same semantics and checks; the orientation is restated for
// this store (Triangle counting).
//
// Every vertex gets a rank, and the oriented row N+(u) is the part of u's row that
// outranks u.  A triangle {a, b, c} with rank a < b < c is then found exactly once, as
// c in N+(a) & N+(b) on the oriented edge (a, b); any total order gives that, the
// degree order keeps the oriented rows short.
//   * degree-sorted adjacency (renumbered graphs): the ids are the ranks, a smaller id
//     outranks a larger one, and N+(u) is the head of u's row (rows ascend): one
//     binary search per vertex, no copy of the entries;
//   * any other adjacency: w outranks u when deg(w) > deg(u), or the degrees are equal
//     and w < u.  The kept entries are compacted into a CSR of their own; they keep
//     their ids, so the rows still ascend and intersect by id.
// Either way the structure is (base, ooff, idx): row u = idx[base[u] .. + ooff[u+1] - ooff[u]),
// and ooff[V] oriented edges are the work items.  It is built on the first call and kept
// on the adjacency.
//
// Counting (one launch, no host read): a thread takes one oriented edge (u, v), found by a
// search of its index in ooff.  Short rows are merged by the thread; an edge with a row of
// kIsectWaveLen entries or more is handed to the wave, whose lanes look the shorter row's
// entries up in the longer one by binary search, in the wave's LDS slice when it fits and
// pays (intersect.hpp holds the merge, the probe and the staging; tc_sink is what this file
// passes as their `hit`).  A hub row is many work items, so it is spread over as many blocks as its size
// asks for.  Per triangle only the third vertex costs an atomic; the edge's own count goes
// to v once per edge and to u once per run of lanes that share u.  Repeated entries of a
// row are skipped on both sides, so they neither add nor multiply triangles.
// On a degree-sorted adjacency the third vertices below id kTcHubs, which take nearly all the hits
// of a power-law graph, are summed in the block's LDS and flushed once per block.
// Counts are summed in 64 bits with device-scope atomics and read by the next launch.
#include "capi.hpp"
#include "intersect.hpp"
#include "prims.hpp"

namespace cgx {

namespace {

constexpr int kTcBlock     = kIsectBlock;
constexpr int kTcHubs      = 2048;  // degree-sorted: third-vertex hits on ids below this are summed in LDS (16 KiB)
constexpr int kTcGridPerCu = 8;     // blocks per CU of the count launch; each flushes its hub sums once

// Where a triangle's third vertex is counted.  Third vertices are the highest-ranked ones, so on a
// power-law graph nearly all hits land on a few hub counters (R-MAT-20: one of them takes 7.5 M of
// 424 M); ids below `hubs` (0 unless the ids are the ranks) go to the block's LDS sums instead.
struct tc_sink {
  count_t* cnt;
  count_t* hub;  // LDS, kTcHubs entries
  long long hubs;
  template <typename V>
  __device__ __forceinline__ void operator()(V w) const  // the `hit` of intersect.hpp
  {
    if ((long long)w < hubs) __hip_atomic_fetch_add(hub + w, (count_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else bump(cnt + w, 1);
  }
};

// ---------------------------------------------------------------- orientation
// degree-sorted: len[v] = entries of row v below v
template <typename V, typename E>
__global__ __launch_bounds__(kTcBlock) void k_tc_head_len(E const* off, V const* idx, int64_t nv, E* len)
{
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) {
    E const b = off[v];
    E lo = b, hi = off[v + 1];
    while (lo < hi) {
      E const mid = lo + ((hi - lo) >> 1);
      if (idx[mid] < (V)v) lo = mid + 1;
      else hi = mid;
    }
    len[v] = lo - b;
  }
}

// Any other adjacency, a wave per row: the entries that outrank the row's vertex are counted
// (out == nullptr: len[v]) or written in their order to out[ooff[v] ..).
template <typename V, typename E>
__global__ __launch_bounds__(kTcBlock) void k_tc_rank_rows(E const* off, V const* idx, int64_t nv, E const* ooff,
                                                          E* len, V* out)
{
  int const lane          = threadIdx.x & 63;
  int64_t const wave      = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  int64_t const num_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t v = wave; v < nv; v += num_waves) {
    long long const b = (long long)off[v], e = (long long)off[v + 1];
    long long const dv = e - b;
    long long kept     = 0;  // wave-uniform
    for (long long j0 = b; j0 < e; j0 += 64) {
      long long const j = j0 + lane;
      bool keep         = false;
      V w               = 0;
      if (j < e) {
        w                  = idx[j];
        long long const dw = (long long)off[w + 1] - (long long)off[w];
        keep               = dw > dv || (dw == dv && (int64_t)w < v);
      }
      unsigned long long const m = __ballot(keep);
      if (out && keep) out[(long long)ooff[v] + kept + __popcll(m & ((1ull << lane) - 1))] = w;
      kept += __popcll(m);
    }
    if (!out && lane == 0) len[v] = (E)kept;
  }
}

// ---------------------------------------------------------------- counting
// One oriented edge per thread and 256-edge chunk.  path: tuning_t::tc_path; hubs: kTcHubs when the
// ids are the ranks, else 0.
template <typename V, typename E>
__global__ __launch_bounds__(kTcBlock) void k_tc_count(E const* base, E const* ooff, V const* idx, int64_t nv,
                                                      int path, int hubs, count_t* cnt)
{
  __shared__ count_t hub[kTcHubs];
  int const tid = threadIdx.x, lane = tid & 63;
  for (int i = tid; i < hubs; i += kTcBlock) hub[i] = 0;
  __syncthreads();
  tc_sink const out{cnt, hub, (long long)hubs};
  V* const stage     = isect_stage<V>();
  long long const ne = (long long)ooff[nv];
  for (long long k0 = blockIdx.x * (long long)kTcBlock; k0 < ne; k0 += (long long)gridDim.x * kTcBlock) {
    long long const k = k0 + tid;
    long long u = -1, v = -1, a0 = 0, la = 0, b0 = 0, lb = 0;
    if (k < ne) {
      // the row of edge k: the first u with ooff[u + 1] > k (ooff[nv] = ne > k ends the search below nv)
      int64_t lo = 0, hi = nv - 1;
      while (lo < hi) {
        int64_t const mid = (lo + hi) >> 1;
        if ((long long)ooff[mid + 1] <= k) lo = mid + 1;
        else hi = mid;
      }
      u                  = lo;
      long long const ou = (long long)ooff[u];
      a0                 = (long long)base[u];
      la                 = (long long)ooff[u + 1] - ou;
      long long const j  = a0 + (k - ou);
      v                  = (long long)idx[j];
      if (j > a0 && (long long)idx[j - 1] == v) {
        lb = 0;  // a repeated entry of u's row: counted with its first copy
      } else {
        b0 = (long long)base[v];
        lb = (long long)ooff[v + 1] - (long long)ooff[v];
      }
    }
    bool const work    = lb > 0;  // la >= 1 whenever there is an edge
    bool const by_wave = work && (path == 2 || (path == 0 && (la >= kIsectWaveLen || lb >= kIsectWaveLen)));
    count_t c          = 0;
    if (work && !by_wave) {
      c = isect_merge<V>(idx + a0, la, idx + b0, lb, out);
      if (c) bump(cnt + v, c);
    }
    // u's share: consecutive edges share u, so the lanes of a run add up first
    {
      count_t cu = c;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        count_t const t    = __shfl_down(cu, o, 64);
        long long const uo = __shfl_down(u, o, 64);
        if (lane + o < 64 && uo == u) cu += t;
      }
      long long const up = __shfl_up(u, 1, 64);
      if (cu && (lane == 0 || up != u)) bump(cnt + u, cu);
    }
    // the edges left to the wave, one after the other
    unsigned long long m = __ballot(by_wave);
    while (m) {  // wave-uniform
      int const l = __ffsll((long long)m) - 1;
      m &= m - 1;
      long long const uu = __shfl(u, l, 64), vv = __shfl(v, l, 64);
      long long sa = __shfl(a0, l, 64), ns = __shfl(la, l, 64);
      long long sb = __shfl(b0, l, 64), nl = __shfl(lb, l, 64);
      isect_shorter_first(sa, ns, sb, nl);
      count_t const cw = isect_wave_count<V>(idx + sa, 0, ns, idx + sb, nl, stage, kIsectStageDiv, lane, out);
      if (lane == 0 && cw) {
        bump(cnt + uu, cw);
        bump(cnt + vv, cw);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < hubs; i += kTcBlock)
    if (hub[i]) bump(cnt + i, hub[i]);
}

// counts[i] = cnt[ids[i]] (ids == nullptr: cnt[i]); an id outside [0, nv) counts 0.
// flag: a count that does not fit the result type.
template <typename V, typename E>
__global__ __launch_bounds__(kTcBlock) void k_tc_finish(count_t const* cnt, int64_t nv, V const* ids, size_t n,
                                                       E* counts, int* flag)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    int64_t const id = ids ? (int64_t)ids[i] : (int64_t)i;
    count_t const c  = (id >= 0 && id < nv) ? cnt[id] : 0;
    if (sizeof(E) == 4 && c > (count_t)INT32_MAX) atomicOr(flag, 1);
    counts[i] = (E)c;
  }
}

// Builds the oriented rows of `adj` once (the only host read: their total).
template <typename V, typename E>
void tc_orient(handle_t& h, graph_t& g, adjacency_t& adj)
{
  if (adj.tc_edges >= 0) return;
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  E const* off     = adj.offsets.data<E>();
  V const* idx     = adj.indices.data<V>();
  dbuf<E> len((size_t)nv + 1, s);
  HIP_CHECK(hipMemsetAsync(len.data() + nv, 0, sizeof(E), s));
  unsigned const row_grid = grid_for((size_t)nv * 64, kTcBlock, 1u << 16);
  if (adj.degree_sorted) {
    hipLaunchKernelGGL((k_tc_head_len<V, E>), dim3(grid_for((size_t)nv, kTcBlock, 1u << 16)), dim3(kTcBlock), 0, s,
                       off, idx, nv, len.data());
  } else {
    hipLaunchKernelGGL((k_tc_rank_rows<V, E>), dim3(row_grid), dim3(kTcBlock), 0, s, off, idx, nv, (E const*)nullptr,
                       len.data(), (V*)nullptr);
  }
  CGX_LAUNCH_CHECK();
  buffer ooff(((size_t)nv + 1) * sizeof(E), s);
  exclusive_scan<E, E>(len.data(), ooff.data<E>(), (size_t)nv + 1, s);
  int64_t const total = (int64_t)to_host_scalar(ooff.data<E>() + nv, s);
  buffer oidx;
  if (!adj.degree_sorted && total > 0) {
    oidx.set_stream(s);
    oidx.resize((size_t)total * sizeof(V));
    hipLaunchKernelGGL((k_tc_rank_rows<V, E>), dim3(row_grid), dim3(kTcBlock), 0, s, off, idx, nv,
                       (E const*)ooff.data<E>(), (E*)nullptr, oidx.data<V>());
    CGX_LAUNCH_CHECK();
  }
  adj.tc_ooff  = std::move(ooff);
  adj.tc_oidx  = std::move(oidx);
  adj.tc_edges = total;
}

template <typename V, typename E>
void tc_impl(handle_t& h, graph_t& g, array_view_t const* start, bool expensive, triangle_count_result_t& res)
{
  hipStream_t s       = h.stream;
  int64_t const nv    = g.num_vertices;
  reset_hot(h);
  size_t n = (size_t)nv;
  dbuf<V> ids;  // internal ids of the start list
  if (start) {
    n            = start->size;
    res.vertices = std::make_unique<device_array_t>(n, g.vertex_type, s);
    ids.resize(n, s);
    if (n) {
      HIP_CHECK(hipMemcpyAsync(res.vertices->buf.data(), start->data, n * sizeof(V), hipMemcpyDefault, s));
      HIP_CHECK(hipMemcpyAsync(ids.data(), start->data, n * sizeof(V), hipMemcpyDefault, s));
      renumber_ext_to_int_unchecked(h, g, ids.data(), n);  // ids not in the graph become -1
      if (expensive)  // triangle_count_impl.cuh:169-187
        expect_ids_in_range<V>(ids.data(), nullptr, n, nv, "Invalid input arguments: invalid vertex IDs in *vertices.",
                               s);
    }
  } else {
    res.vertices = number_map_copy(h, g);
  }
  res.counts = std::make_unique<device_array_t>(n, g.edge_type, s);
  if (n == 0) return;
  E* counts = res.counts->buf.data<E>();
  if (nv == 0 || g.num_edges == 0) {
    HIP_CHECK(hipMemsetAsync(counts, 0, n * sizeof(E), s));
    return;
  }
  // symmetric: either orientation is the same adjacency
  adjacency_t& adj = ensure_adjacency(h, g, g.store_transposed);
  tc_orient<V, E>(h, g, adj);
  E const* ooff = adj.tc_ooff.data<E>();
  E const* base = adj.degree_sorted ? adj.offsets.data<E>() : ooff;
  V const* idx  = adj.degree_sorted ? adj.indices.data<V>() : adj.tc_oidx.data<V>();

  dbuf<count_t> cnt((size_t)nv, s);
  dbuf<int> flag(1, s);
  HIP_CHECK(hipMemsetAsync(cnt.data(), 0, (size_t)nv * sizeof(count_t), s));
  HIP_CHECK(hipMemsetAsync(flag.data(), 0, sizeof(int), s));
  chunk_timer timer{h, s};
  timer.begin();
  size_t launches = 1;
  if (adj.tc_edges > 0) {
    int const hubs = adj.degree_sorted ? (int)std::min<int64_t>(nv, kTcHubs) : 0;
    unsigned const grid =
      grid_for((size_t)adj.tc_edges, kTcBlock, (unsigned)std::max(device_cu_count(), 1) * kTcGridPerCu);
    hipLaunchKernelGGL((k_tc_count<V, E>), dim3(grid), dim3(kTcBlock), 0, s, base, ooff, idx, nv, h.tune.tc_path, hubs,
                       cnt.data());
    ++launches;
  }
  hipLaunchKernelGGL((k_tc_finish<V, E>), dim3(grid_for(n, kTcBlock, 1u << 16)), dim3(kTcBlock), 0, s,
                     (count_t const*)cnt.data(), nv, start ? (V const*)ids.data() : (V const*)nullptr, n, counts,
                     flag.data());
  CGX_LAUNCH_CHECK();
  timer.end();
  timer.report(launches);
  if (sizeof(E) == 4)  // the one read of the call, after the last launch
    CGX_EXPECTS(to_host_scalar(flag.data(), s) == 0, CUGRAPH_UNSUPPORTED_TYPE_COMBINATION,
                "triangle_count: a vertex's count does not fit the graph's 32-bit edge type; "
                "build the graph with 64-bit edge offsets.");
}

}  // namespace

void run_triangle_count(handle_t& h, graph_t& g, array_view_t const* start, bool expensive,
                        triangle_count_result_t& res)
{
  dispatch_ve(g.vertex_type, g.edge_type, [&](auto t) {
    using T = decltype(t);
    tc_impl<typename T::vertex_t, typename T::edge_t>(h, g, start, expensive, res);
  });
}

}  // namespace cgx
