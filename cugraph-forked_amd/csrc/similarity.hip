// Jaccard, Sorensen and overlap similarity of vertex pairs: sorted-row intersection sizes.
//
// Reference: c_api/similarity.cpp (entry points; the snapshot's body is unimplemented),
// link_prediction/similarity_impl.cuh (intersection size and the two degrees per pair, then one
// functor per measure) and link_prediction/legacy/jaccard.cu.  Semantics are restated in
// include/cugraph_c/similarity_algorithms.h and DESIGN.md (Similarity / two-hop):
// N(u) is the set of distinct ids of u's stored row (a self-loop makes u a member, a repeated
// entry counts once), d(u) = |N(u)|, c = |N(u) & N(v)|, and the score is computed from those
// integers in double and rounded once to the weight type.  Everything before that rounding is
// integer work, so no option and no schedule changes a result bit.
//
// d(u) is kept per vertex on the adjacency (sim_deg, built on the first call as tc_ooff is).
// Counting, one work item per pair, by the sizes of the two stored rows:
//   * thread: a merge of two short rows that skips runs of equal ids;
//   * wave (a row of kSimWaveLen entries or more): the lanes look the shorter row's entries up in
//     the longer one by binary search, in the wave's LDS slice when it fits and pays;
//   * split (the shorter row has sim_split_min entries or more): one hub-hub pair on one wave is a
//     long serial tail, so the pair is put on a device-built list with a range of segment numbers;
//     a second grid-stride launch gives every segment of the shorter row to a wave of its own and
//     sums the segment counts into the pair's counter with device-scope integer atomics.
// No host read sits between the launches: the list's length stays on the device.
// The merge, the probe, the staging and their constants are intersect.hpp's, shared with
// triangle_count.hip; similarity counts only, so it passes isect_ignore as their `hit`.
// kSimWaveLen and kSimStageDiv are the shared wave cut and stage ratio unless an A/B build overrides
// them; with the default sim_split_min they were kept after scripts/similarity_time.py on R-MAT-20
// (DESIGN.md keeps the table: wave cuts 32 .. 256 and stage ratios 1/8, 1/64 equal within the spread,
// split thresholds from 4096 up free).  kSimSegLen and kSimGridPerCu are still guesses: no run has
// varied them.
#include "capi.hpp"
#include "intersect.hpp"
#include "prims.hpp"

#include <algorithm>

namespace cgx {

namespace {

constexpr int kSimBlock     = kIsectBlock;
constexpr int kSimSegBits   = 39;  // heavy-list word: segments in the low bits (sim_seg_len), list position above
constexpr int kSimGridPerCu = 8;
constexpr size_t kSimChunk  = (size_t)1 << 24;  // pairs per launch: list positions fit the word's high bits

// ---------------------------------------------------------------- distinct degrees
// a wave per row: entries that differ from their predecessor
template <typename V, typename E>
__global__ __launch_bounds__(kSimBlock) void k_sim_degrees(E const* off, V const* idx, int64_t nv, E* deg)
{
  int const lane          = threadIdx.x & 63;
  int64_t const wave      = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  int64_t const num_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t v = wave; v < nv; v += num_waves) {
    long long const b = (long long)off[v], e = (long long)off[v + 1];
    long long c       = 0;
    for (long long j = b + lane; j < e; j += 64) c += (j == b || idx[j - 1] != idx[j]) ? 1 : 0;
    c = wave_sum_ll(c);
    if (lane == 0) deg[v] = (E)c;
  }
}

// ---------------------------------------------------------------- counting
struct sim_heavy {
  long long pair;   // index into the chunk's pairs
  long long first;  // its first segment number
};

// the row of an internal id; an id outside [0, nv) has no neighbours
template <typename E>
__device__ __forceinline__ void sim_row(E const* off, int64_t nv, long long u, long long& begin, long long& len)
{
  begin = 0;
  len   = 0;
  if (u >= 0 && u < nv) {
    begin = (long long)off[u];
    len   = (long long)off[u + 1] - begin;
  }
}

// One pair per thread and 256-pair chunk.  path: tuning_t::sim_path.  cnt[k] is zero on entry; the
// pairs left to the split tier go to heavy[] and keep their zero.
template <typename V, typename E>
__global__ __launch_bounds__(kSimBlock) void k_sim_count(E const* off, V const* idx, int64_t nv, V const* first,
                                                         V const* second, long long n, int path, long long split_min,
                                                         count_t* cnt, sim_heavy* heavy, count_t* heavy_word)
{
  int const tid = threadIdx.x, lane = tid & 63;
  V* const stage = isect_stage<V>();
  for (long long k0 = blockIdx.x * (long long)kSimBlock; k0 < n; k0 += (long long)gridDim.x * kSimBlock) {
    long long const k = k0 + tid;
    long long a0 = 0, la = 0, b0 = 0, lb = 0;
    if (k < n) {
      sim_row<E>(off, nv, (long long)first[k], a0, la);
      sim_row<E>(off, nv, (long long)second[k], b0, lb);
    }
    bool const work     = la > 0 && lb > 0;
    long long const ns  = la < lb ? la : lb;
    bool const by_split = work && (path == 3 || (path == 0 && ns >= split_min));
    bool const by_wave  = work && !by_split && (path == 2 || (path == 0 && (la >= kSimWaveLen || lb >= kSimWaveLen)));
    if (by_split) {
      long long const len  = sim_seg_len(ns);
      count_t const nseg   = (count_t)((ns + len - 1) / len);
      count_t const before = __hip_atomic_fetch_add(heavy_word, ((count_t)1 << kSimSegBits) | nseg, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
      // one add gives the position and the segment number together: positions ascend with them
      heavy[before >> kSimSegBits] = sim_heavy{k, (long long)(before & (((count_t)1 << kSimSegBits) - 1))};
    } else if (work && !by_wave) {
      cnt[k] = isect_merge<V>(idx + a0, la, idx + b0, lb, isect_ignore{});
    }
    // the pairs left to the wave, one after the other
    unsigned long long m = __ballot(by_wave);
    while (m) {  // wave-uniform
      int const l = __ffsll((long long)m) - 1;
      m &= m - 1;
      long long sa = __shfl(a0, l, 64), nsw = __shfl(la, l, 64);
      long long sb = __shfl(b0, l, 64), nl = __shfl(lb, l, 64);
      isect_shorter_first(sa, nsw, sb, nl);
      count_t const cw =
        isect_wave_count<V>(idx + sa, 0, nsw, idx + sb, nl, stage, kSimStageDiv, lane, isect_ignore{});
      if (lane == l) cnt[k] = cw;
    }
  }
}

// A wave per segment of the heavy list.  heavy_word holds (pairs << kSimSegBits | segments).
template <typename V, typename E>
__global__ __launch_bounds__(kSimBlock) void k_sim_split(E const* off, V const* idx, V const* first, V const* second,
                                                         sim_heavy const* heavy, count_t const* heavy_word,
                                                         count_t* cnt)
{
  int const tid = threadIdx.x, lane = tid & 63;
  V* const stage          = isect_stage<V>();
  count_t const word     = *heavy_word;
  long long const npairs  = (long long)(word >> kSimSegBits);
  long long const nsegs   = (long long)(word & (((count_t)1 << kSimSegBits) - 1));
  long long const wave    = (blockIdx.x * (long long)blockDim.x + tid) >> 6;
  long long const nwaves  = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long sgm = wave; sgm < nsegs; sgm += nwaves) {  // wave-uniform
    // the last list entry whose first segment is not above sgm (heavy[0].first == 0)
    long long lo = 0, hi = npairs - 1;
    while (lo < hi) {
      long long const mid = (lo + hi + 1) >> 1;
      if (heavy[mid].first <= sgm) lo = mid;
      else hi = mid - 1;
    }
    sim_heavy const hp = heavy[lo];
    // listed pairs have both ids in range and both rows non-empty
    long long const u = (long long)first[hp.pair], v = (long long)second[hp.pair];
    long long sa = (long long)off[u], ns = (long long)off[u + 1] - sa;
    long long sb = (long long)off[v], nl = (long long)off[v + 1] - sb;
    isect_shorter_first(sa, ns, sb, nl);
    long long const len = sim_seg_len(ns);
    long long const s0  = (sgm - hp.first) * len;
    long long const s1  = s0 + len < ns ? s0 + len : ns;
    if (s0 >= s1) continue;
    count_t const cw = isect_wave_count<V>(idx + sa, s0, s1, idx + sb, nl, stage, kSimStageDiv, lane, isect_ignore{});
    if (lane == 0 && cw) bump(cnt + hp.pair, cw);
  }
}

// measure: 0 Jaccard, 1 Sorensen, 2 overlap.  The score comes from the three integers in double and
// is rounded once to W; a zero denominator scores 0.
template <typename V, typename E, typename W>
__global__ __launch_bounds__(kSimBlock) void k_sim_finish(count_t const* cnt, E const* deg, int64_t nv, V const* first,
                                                          V const* second, size_t n, int measure, W* score)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    long long const u = (long long)first[i], v = (long long)second[i];
    double const du   = (u >= 0 && u < nv) ? (double)deg[u] : 0.0;
    double const dv   = (v >= 0 && v < nv) ? (double)deg[v] : 0.0;
    double const c    = (double)cnt[i];
    double num, den;
    if (measure == 0) {
      num = c;
      den = du + dv - c;
    } else if (measure == 1) {
      num = 2.0 * c;
      den = du + dv;
    } else {
      num = c;
      den = du < dv ? du : dv;
    }
    score[i] = den > 0.0 ? (W)(num / den) : (W)0;
  }
}

template <typename V, typename E>
void sim_degrees(handle_t& h, graph_t& g, adjacency_t& adj)
{
  if (adj.sim_deg_valid) return;
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  buffer deg((size_t)std::max<int64_t>(nv, 1) * sizeof(E), s);
  if (nv > 0) {
    hipLaunchKernelGGL((k_sim_degrees<V, E>), dim3(grid_for((size_t)nv * 64, kSimBlock, 1u << 16)), dim3(kSimBlock), 0,
                       s, adj.offsets.data<E>(), adj.indices.data<V>(), nv, deg.data<E>());
    CGX_LAUNCH_CHECK();
  }
  adj.sim_deg       = std::move(deg);
  adj.sim_deg_valid = true;
}

template <typename V, typename E, typename W>
void sim_impl(handle_t& h, graph_t& g, array_view_t const& first, array_view_t const& second, int measure,
              bool expensive, similarity_result_t& res)
{
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  size_t const n   = first.size;
  reset_hot(h);
  res.similarity = std::make_unique<device_array_t>(n, g.weight_type, s);
  if (n == 0) return;
  W* score = res.similarity->buf.data<W>();
  dbuf<V> a(n, s), b(n, s);  // internal ids; an id that is not in the graph becomes -1 or stays out of range
  HIP_CHECK(hipMemcpyAsync(a.data(), first.data, n * sizeof(V), hipMemcpyDefault, s));
  HIP_CHECK(hipMemcpyAsync(b.data(), second.data, n * sizeof(V), hipMemcpyDefault, s));
  renumber_ext_to_int_unchecked(h, g, a.data(), n);
  renumber_ext_to_int_unchecked(h, g, b.data(), n);
  if (expensive)
    expect_ids_in_range<V>(a.data(), b.data(), n, nv, "Invalid input arguments: invalid vertex IDs in *vertex_pairs.",
                           s);
  if (nv == 0 || g.num_edges == 0) {
    HIP_CHECK(hipMemsetAsync(score, 0, n * sizeof(W), s));
    return;
  }
  // symmetric: either orientation is the same adjacency
  adjacency_t& adj = ensure_adjacency(h, g, g.store_transposed);
  sim_degrees<V, E>(h, g, adj);
  E const* off = adj.offsets.data<E>();
  V const* idx = adj.indices.data<V>();

  dbuf<count_t> cnt(n, s);
  size_t const chunk = std::min(n, kSimChunk);
  dbuf<sim_heavy> heavy(chunk, s);
  dbuf<count_t> word(1, s);
  HIP_CHECK(hipMemsetAsync(cnt.data(), 0, n * sizeof(count_t), s));
  chunk_timer timer{h, s};
  timer.begin();
  long long const split_min = std::max<long long>(h.tune.sim_split_min, 1);
  unsigned const max_grid   = (unsigned)std::max(device_cu_count(), 1) * kSimGridPerCu;
  size_t launches           = 1;
  for (size_t p0 = 0; p0 < n; p0 += chunk) {
    size_t const m = std::min(chunk, n - p0);
    HIP_CHECK(hipMemsetAsync(word.data(), 0, sizeof(count_t), s));
    hipLaunchKernelGGL((k_sim_count<V, E>), dim3(grid_for(m, kSimBlock, max_grid)), dim3(kSimBlock), 0, s, off, idx, nv,
                       (V const*)a.data() + p0, (V const*)b.data() + p0, (long long)m, h.tune.sim_path, split_min,
                       cnt.data() + p0, heavy.data(), word.data());
    // the list's length stays on the device; an empty list ends the launch at once
    hipLaunchKernelGGL((k_sim_split<V, E>), dim3(max_grid), dim3(kSimBlock), 0, s, off, idx, (V const*)a.data() + p0,
                       (V const*)b.data() + p0, (sim_heavy const*)heavy.data(), (count_t const*)word.data(),
                       cnt.data() + p0);
    CGX_LAUNCH_CHECK();
    launches += 2;
  }
  hipLaunchKernelGGL((k_sim_finish<V, E, W>), dim3(grid_for(n, kSimBlock, 1u << 16)), dim3(kSimBlock), 0, s,
                     (count_t const*)cnt.data(), (E const*)adj.sim_deg.data<E>(), nv, (V const*)a.data(),
                     (V const*)b.data(), n, measure, score);
  CGX_LAUNCH_CHECK();
  timer.end();
  timer.report(launches);
}

}  // namespace

void run_similarity(handle_t& h, graph_t& g, array_view_t const& first, array_view_t const& second, int measure,
                    bool expensive, similarity_result_t& res)
{
  dispatch_vew(g.vertex_type, g.edge_type, g.weight_type, [&](auto t) {
    using T = decltype(t);
    sim_impl<typename T::vertex_t, typename T::edge_t, typename T::weight_t>(h, g, first, second, measure, expensive,
                                                                            res);
  });
}

}  // namespace cgx
