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
// The intersection helpers repeat triangle_count.hip's tc_merge / tc_probe with a plain counter in
// place of tc_sink; that file is left as it is.
// kSimWaveLen, kSimStageDiv and the stage size are triangle_count.hip's constants; with the default
// sim_split_min they were kept after scripts/similarity_time.py on R-MAT-20 (DESIGN.md keeps the
// table: wave cuts 32 .. 256 and stage ratios 1/8, 1/64 equal within the spread, split thresholds from
// 4096 up free).  kSimSegLen and kSimGridPerCu are still guesses: no run has varied them.
#include "capi.hpp"
#include "prims.hpp"

#include <algorithm>

namespace cgx {

namespace {

// A/B builds (Similarity / two-hop) override the two cuts on the compiler's command line
#ifndef CGX_SIM_WAVE_LEN
#define CGX_SIM_WAVE_LEN 64
#endif
#ifndef CGX_SIM_STAGE_DIV
#define CGX_SIM_STAGE_DIV 64
#endif

constexpr int kSimBlock      = 256;
constexpr int kSimWaveLen    = CGX_SIM_WAVE_LEN;  // a pair with a row of at least this many entries: the wave
constexpr int kSimStageBytes = 4096;  // LDS slice of a wave (1024 4-byte or 512 8-byte ids), 16 KiB per block
constexpr int kSimStageDiv   = CGX_SIM_STAGE_DIV;  // stage the longer row when the probing part has at least
                                                   // 1/64 of its entries (0: never)
constexpr int kSimSegLen     = 256;   // entries of the shorter row per split segment (4 probes per lane)
constexpr int kSimSegBits    = 39;    // heavy-list word: segments in the low bits, list position above
constexpr int kSimGridPerCu  = 8;
constexpr size_t kSimChunk   = (size_t)1 << 24;  // pairs per launch: list positions fit the word's high bits

using count_t = unsigned long long;

// segments of a split pair whose shorter row has ns entries: at most 2^14 + 1 of them, so a chunk's
// segment numbers stay below 2^kSimSegBits
__device__ __forceinline__ long long sim_seg_len(long long ns)
{
  long long const by_count = (ns + 16383) >> 14;
  return by_count > kSimSegLen ? by_count : kSimSegLen;
}

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
// a thread merges two short rows; runs of equal ids count once
template <typename V>
__device__ __forceinline__ count_t sim_merge(V const* A, long long na, V const* B, long long nb)
{
  count_t c   = 0;
  long long i = 0, j = 0;
  while (i < na && j < nb) {
    V const x = A[i], y = B[j];
    if (x < y) ++i;
    else if (y < x) ++j;
    else {
      ++c;
      do ++i; while (i < na && A[i] == x);
      do ++j; while (j < nb && B[j] == x);
    }
  }
  return c;
}

// the lanes of a wave look the entries [s0, s1) of row S up in L (global memory or the wave's LDS
// slice); returns this lane's hits.  A repeated entry is left to its first copy, which may lie
// before s0.
template <typename V>
__device__ __forceinline__ count_t sim_probe(V const* S, long long s0, long long s1, V const* L, long long nl, int lane)
{
  count_t c = 0;
  for (long long i = s0 + lane; i < s1; i += 64) {
    V const x = S[i];
    if (i > 0 && S[i - 1] == x) continue;
    long long lo = 0, hi = nl;
    while (lo < hi) {
      long long const mid = (lo + hi) >> 1;
      if (L[mid] < x) lo = mid + 1;
      else hi = mid;
    }
    if (lo < nl && L[lo] == x) ++c;
  }
  return c;
}

// entries [s0, s1) of S against the whole of L by one wave, L staged when it fits and pays;
// returns the wave's sum in every lane
template <typename V>
__device__ __forceinline__ count_t sim_wave_count(V const* S, long long s0, long long s1, V const* L, long long nl,
                                                  V* stage, int stage_len, int lane)
{
  count_t cw;
  if (nl <= stage_len && (s1 - s0) * kSimStageDiv >= nl) {
    // DS operations of one wave complete in order; the barriers only pin the compiler
    __builtin_amdgcn_wave_barrier();
    for (long long j = lane; j < nl; j += 64) stage[j] = L[j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    cw = sim_probe<V>(S, s0, s1, stage, nl, lane);
    __builtin_amdgcn_wave_barrier();
  } else {
    cw = sim_probe<V>(S, s0, s1, L, nl, lane);
  }
  return (count_t)wave_sum_ll((long long)cw);
}

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
  constexpr int kStage = kSimStageBytes / (int)sizeof(V);
  __shared__ V stage_all[(kSimBlock / 64) * kStage];
  int const tid = threadIdx.x, lane = tid & 63;
  V* const stage = stage_all + (tid >> 6) * kStage;
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
      cnt[k] = sim_merge<V>(idx + a0, la, idx + b0, lb);
    }
    // the pairs left to the wave, one after the other
    unsigned long long m = __ballot(by_wave);
    while (m) {  // wave-uniform
      int const l = __ffsll((long long)m) - 1;
      m &= m - 1;
      long long sa = __shfl(a0, l, 64), nsw = __shfl(la, l, 64);
      long long sb = __shfl(b0, l, 64), nl = __shfl(lb, l, 64);
      if (nsw > nl) {  // S: the shorter row, L: the longer
        long long t = sa; sa = sb; sb = t;
        t = nsw; nsw = nl; nl = t;
      }
      count_t const cw = sim_wave_count<V>(idx + sa, 0, nsw, idx + sb, nl, stage, kStage, lane);
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
  constexpr int kStage = kSimStageBytes / (int)sizeof(V);
  __shared__ V stage_all[(kSimBlock / 64) * kStage];
  int const tid = threadIdx.x, lane = tid & 63;
  V* const stage          = stage_all + (tid >> 6) * kStage;
  count_t const word      = *heavy_word;
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
    if (ns > nl) {
      long long t = sa; sa = sb; sb = t;
      t = ns; ns = nl; nl = t;
    }
    long long const len = sim_seg_len(ns);
    long long const s0  = (sgm - hp.first) * len;
    long long const s1  = s0 + len < ns ? s0 + len : ns;
    if (s0 >= s1) continue;
    count_t const cw = sim_wave_count<V>(idx + sa, s0, s1, idx + sb, nl, stage, kStage, lane);
    if (lane == 0 && cw) __hip_atomic_fetch_add(cnt + hp.pair, cw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

template <typename V>
__global__ __launch_bounds__(kSimBlock) void k_sim_bad_ids(V const* a, V const* b, size_t n, int64_t nv, int* bad)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    if (a[i] < 0 || (int64_t)a[i] >= nv || b[i] < 0 || (int64_t)b[i] >= nv) atomicOr(bad, 1);
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
  hipStream_t s       = h.stream;
  int64_t const nv    = g.num_vertices;
  size_t const n      = first.size;
  h.last_iterations   = 0;
  h.last_hot_ms       = 0;
  h.last_hot_launches = 0;
  res.similarity      = std::make_unique<device_array_t>(n, g.weight_type, s);
  if (n == 0) return;
  W* score = res.similarity->buf.data<W>();
  dbuf<V> a(n, s), b(n, s);  // internal ids; an id that is not in the graph becomes -1 or stays out of range
  HIP_CHECK(hipMemcpyAsync(a.data(), first.data, n * sizeof(V), hipMemcpyDefault, s));
  HIP_CHECK(hipMemcpyAsync(b.data(), second.data, n * sizeof(V), hipMemcpyDefault, s));
  renumber_ext_to_int_unchecked(h, g, a.data(), n);
  renumber_ext_to_int_unchecked(h, g, b.data(), n);
  if (expensive) {
    dbuf<int> bad(1, s);
    HIP_CHECK(hipMemsetAsync(bad.data(), 0, sizeof(int), s));
    hipLaunchKernelGGL(k_sim_bad_ids<V>, dim3(grid_for(n, kSimBlock, 4096)), dim3(kSimBlock), 0, s, a.data(), b.data(),
                       n, nv, bad.data());
    CGX_LAUNCH_CHECK();
    CGX_INPUT(to_host_scalar(bad.data(), s) == 0, "Invalid input arguments: invalid vertex IDs in *vertex_pairs.");
  }
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
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (h.profiling) {
    e0 = h.event(0);
    e1 = h.event(1);
    HIP_CHECK(hipEventRecord(e0, s));
  }
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
  if (h.profiling) {
    HIP_CHECK(hipEventRecord(e1, s));
    HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    h.last_hot_ms       = ms;
    h.last_hot_launches = launches;
  }
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
