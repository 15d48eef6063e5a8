// Core number and k-core: level-by-level peeling over the symmetric adjacency.
//
// Reference: cores/core_number_impl.cuh (degrees, then levels k = smallest remaining degree,
// a frontier per level), c_api/core_number.cpp, c_api/k_core.cpp, c_api/core_result.cpp.  The
// reference snapshot's cugraph::k_core is "Not implemented"; k_core here does what the header
// documents (Core number / k-core).  The method is the peeling of ParK / PKC
// (Kabir & Madduri) in its GPU form (Ahmad et al., ICDE 2023), run device-driven the way
// sssp.hip runs its rounds.
//
// deg[] is the result's core number array.  It starts as the degree in the underlying simple
// graph times delta (delta = 1, or 2 for K_CORE_DEGREE_TYPE_INOUT): the entries of the row that
// are neither the row's own vertex nor a repeat of the entry before them (rows ascend, so both
// are local tests).  A vertex is "peeled" once it has been put on a frontier; its slot then
// holds its core number for good.
//
// One level k:
//   scan   the vertices not yet peeled: deg == k goes to the frontier, deg > k to the other
//          remaining list (so later scans read survivors only), their smallest degree is kept;
//   peel   for every entry u of a frontier row with deg[u] > k (a relaxed load):
//            old = fetch_sub(deg[u], delta)
//            old == k + delta : u has reached level k, it goes to the next frontier
//            old <= k         : u was at level k already, delta is added back
//          until the next frontier is empty; then k becomes the smallest remaining degree.
//
// Why a vertex is put on a frontier exactly once, and ends with its core number:
//   * while deg[u] > k every operation on it is a fetch_sub whose old value is > k (an add-back
//     needs old <= k), so the value falls by delta per operation and exactly one operation
//     sees old == k + delta.  Degrees, k and delta are all multiples of delta, so the value
//     cannot step over k + delta;
//   * from that operation on the value is k minus delta per subtraction still to be added
//     back: it never rises above k again, every later fetch_sub sees old <= k and is undone,
//     and no later operation can see old == k + delta.  When the level's kernels have ended the
//     value is k;
//   * a vertex the scan put on the frontier has deg == k and is covered by the same argument
//     from its first subtraction on; a load that shows <= k skips it altogether;
//   * a stale load can only show an older, larger value: the fetch_sub then sees old <= k and
//     is undone.  A load never shows <= k for a vertex that is still above k.
// Between levels every surviving vertex has deg > k, and the next k is at most their smallest
// degree, so the scan's "deg == k" finds the whole level.  The smallest degree is tracked as the
// minimum of the scan's survivors and of every value a subtraction left above k; values of
// vertices peeled later in the level can make it too small, never too large and never <= k.  A
// too small one costs an empty scan round, whose minimum is exact (nothing was peeled after it).
//
// Rounds (all on the handle's stream): scan (returns at once unless a level starts), peel, peel
// waves, peel hubs, control.  The host enqueues kCoreChunkRounds of them and reads the state block
// once per chunk; rounds after the end return at once.  Every grid is fixed and strides over
// counts it reads from the state block.  Frontier rows are binned by size as wcc.hip bins its
// rows: a thread per row below kCoreWaveRow entries (the lanes of a wave step together, so appends
// are staged per wave); rows below kCoreHubRow are listed and taken a wave per row, dealt over
// the whole grid; longer rows are listed and spread over the hub grid in kCoreHubSeg-entry
// segments.  List appends cost one counter add per wave.
//
// k-core: core numbers per internal id (computed here, or scattered from the caller's result),
// then row_extract.hpp's extraction with the test kcore_rows.
#include "capi.hpp"
#include "prims.hpp"
#include "row_extract.hpp"

#include <algorithm>
#include <limits>

namespace cgx {

namespace {

constexpr int kCoreBlock       = 256;
constexpr int kCoreWaveRow     = 64;    // rows with at least this many entries: one wave
constexpr int kCoreHubRow      = 4096;  // ... and from here on: listed, the whole hub grid in segments
constexpr int kCoreHubSeg      = 1024;  // entries per block and step of a hub row
constexpr int kCoreHubSkew     = 61;    // blocks between the first segments of consecutive hub rows
constexpr int kCoreSpan        = 1024;  // consecutive entries a wave takes per step of the degree pass
constexpr int kCoreDegreePerCu = 16;    // blocks per CU of the degree pass, at most
constexpr int kCoreGridPerCu   = 4;     // blocks per CU of the scan and peel grids
constexpr int kCoreHubPerCu    = 2;     // blocks per CU of the hub grid
constexpr int kCoreChunkRounds = 16;    // rounds enqueued per host read

template <typename E>
struct core_state {
  E k;                        // the level being peeled
  E mindeg;                   // a lower bound above k of the smallest degree not yet peeled
  unsigned long long nf[2];   // frontier sizes
  unsigned long long nr[2];   // remaining-list sizes
  unsigned long long nmid;    // rows listed for a wave by this round's peel
  unsigned long long nhub;    // hub rows listed by this round's peel
  unsigned long long rounds;
  unsigned long long levels;  // levels that peeled something
  int fp, rp;                 // the current frontier / remaining list
  int scan;                   // the next round starts a level
  int first;                  // no remaining list yet: the scan reads every vertex
  int done;
  int bad;                    // an append past a list's end (cannot happen; never written past it)
};

template <typename V, typename E>
struct core_args {
  E const* off;
  V const* idx;
  int64_t nv;
  E* deg;
  E delta;
  V* front[2];  // nv entries each
  V* rem[2];    // nv entries each (compact only)
  V* mids;
  unsigned long long mid_cap;
  V* hubs;
  unsigned long long hub_cap;
  core_state<E>* st;
  int compact;  // tuning_t::core_scan
};

template <typename E>
__device__ __forceinline__ void publish_min(E* slot, E mn)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    E const t = __shfl_xor(mn, o, 64);
    mn        = t < mn ? t : mn;
  }
  if ((threadIdx.x & 63) == 0 && mn != std::numeric_limits<E>::max())
    __hip_atomic_fetch_min(slot, mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------- degrees
// the row of entry t < off[nv]: the first r in [lo, hi] with off[r + 1] > t
template <typename E>
__device__ __forceinline__ int64_t core_row_of(E const* off, int64_t lo, int64_t hi, long long t)
{
  while (lo < hi) {
    int64_t const mid = (lo + hi) >> 1;
    if ((long long)off[mid + 1] <= t) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// deg[v] += delta x the entries of row v that are neither v nor a repeat (deg zero before); loops: a row
// holds its own vertex.  The entries are taken in their own space, kCoreSpan consecutive ones per wave
// and step, whatever rows they belong to: on a degree-sorted adjacency the first rows hold a large
// part of all entries, and a pass by rows leaves them to a few blocks.  The span's first and last row
// are searched once, an entry's row between the two; lanes that share a row add once.
template <typename V, typename E>
__global__ __launch_bounds__(kCoreBlock) void k_core_degree(E const* off, V const* idx, int64_t nv, E delta, E* deg,
                                                           int* loops)
{
  int const lane        = threadIdx.x & 63;
  long long const ne    = (long long)off[nv];
  long long const wave  = (blockIdx.x * (long long)kCoreBlock + threadIdx.x) >> 6;
  long long const waves = ((long long)gridDim.x * kCoreBlock) >> 6;
  bool loop             = false;
  for (long long t0 = wave * kCoreSpan; t0 < ne; t0 += waves * kCoreSpan) {  // wave-uniform
    long long const t1 = t0 + kCoreSpan < ne ? t0 + kCoreSpan : ne;
    int64_t const r0   = core_row_of(off, 0, nv - 1, t0);
    int64_t const r1   = core_row_of(off, r0, nv - 1, t1 - 1);
    for (long long j0 = t0; j0 < t1; j0 += 64) {
      long long const j = j0 + lane;
      bool const in     = j < t1;
      long long r       = r0;
      bool valid        = false;
      if (in) {
        r         = core_row_of(off, r0, r1, j);
        V const u = idx[j];
        if ((long long)u == r) loop = true;
        else valid = j == (long long)off[r] || idx[j - 1] != u;
      }
      unsigned long long const vm = __ballot(valid);
      long long const before      = __shfl_up(r, 1, 64);
      bool const head             = in && (lane == 0 || before != r);
      unsigned long long const hm = __ballot(head);
      if (head) {  // the lanes [lane, end) share row r
        unsigned long long const above = lane == 63 ? 0ull : hm >> (lane + 1);
        int const end                  = above ? lane + __ffsll((long long)above) : 64;
        unsigned long long const upto  = end == 64 ? ~0ull : (1ull << end) - 1ull;
        int const c                    = __popcll(vm & upto & ~((1ull << lane) - 1ull));
        if (c) __hip_atomic_fetch_add(deg + r, (E)c * delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  if (loop) atomicOr(loops, 1);
}

template <typename E>
__global__ void k_core_init(core_state<E>* st, E delta)
{
  core_state<E> s{};
  s.k      = delta;  // no degree is below it; an empty first level costs one round
  s.mindeg = std::numeric_limits<E>::max();
  s.scan   = 1;
  s.first  = 1;
  *st      = s;
}

// ---------------------------------------------------------------- scan
template <typename V, typename E>
__global__ __launch_bounds__(kCoreBlock) void k_core_scan(core_args<V, E> a)
{
  core_state<E>* st = a.st;
  if (st->done || !st->scan) return;
  E const k       = st->k;
  int const fp = st->fp, rp = st->rp;
  bool const all  = !a.compact || st->first;
  int64_t const n = all ? a.nv : (int64_t)(st->nr[rp] < (unsigned long long)a.nv ? st->nr[rp] : a.nv);
  V const* src    = a.rem[rp];
  E mn            = std::numeric_limits<E>::max();
  for (int64_t base = blockIdx.x * (int64_t)kCoreBlock; base < n; base += (int64_t)gridDim.x * kCoreBlock) {
    int64_t const i = base + threadIdx.x;
    bool in_f = false, in_r = false;
    V v = 0;
    if (i < n) {
      v         = all ? (V)i : src[i];
      E const d = a.deg[v];
      in_f      = d == k;
      in_r      = d > k;  // (peeled and isolated vertices are below k)
      if (in_r && d < mn) mn = d;
    }
    list_append_if(a.front[fp], &st->nf[fp], (unsigned long long)a.nv, &st->bad, in_f, v);
    if (a.compact) {
      list_append_if(a.rem[rp ^ 1], &st->nr[rp ^ 1], (unsigned long long)a.nv, &st->bad, in_r, v);
    } else {
      unsigned long long const m = __ballot(in_r);
      if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1)
        __hip_atomic_fetch_add(&st->nr[rp ^ 1], (unsigned long long)__popcll(m), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  publish_min(&st->mindeg, mn);
}

// ---------------------------------------------------------------- peel
// entry j of the row [b, ..) of frontier vertex v; true: its vertex has reached level k
template <typename V, typename E>
__device__ __forceinline__ bool peel_entry(core_args<V, E> const& a, E k, V v, long long b, long long j, V& u, E& mn)
{
  u = a.idx[j];
  if (u == v || (j > b && a.idx[j - 1] == u)) return false;
  E* const p = a.deg + u;
  if (ld_relaxed(p) <= k) return false;
  E const old = __hip_atomic_fetch_sub(p, a.delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (old == k + a.delta) return true;
  if (old <= k) __hip_atomic_fetch_add(p, a.delta, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else if (old - a.delta < mn) mn = old - a.delta;
  return false;
}

// The frontier's rows: a block takes 256 frontier vertices at a time.
template <typename V, typename E>
__global__ __launch_bounds__(kCoreBlock) void k_core_peel(core_args<V, E> a)
{
  core_state<E>* st = a.st;
  if (st->done) return;
  int const tid    = threadIdx.x;
  E const k        = st->k;
  int const fp     = st->fp;
  int64_t const n  = (int64_t)(st->nf[fp] < (unsigned long long)a.nv ? st->nf[fp] : a.nv);  // (never above nv)
  V const* F       = a.front[fp];
  V* const next    = a.front[fp ^ 1];
  unsigned long long* const nnext = &st->nf[fp ^ 1];
  unsigned long long const cap    = (unsigned long long)a.nv;
  E mn             = std::numeric_limits<E>::max();
  for (int64_t base = blockIdx.x * (int64_t)kCoreBlock; base < n; base += (int64_t)gridDim.x * kCoreBlock) {
    int64_t const i = base + tid;
    V v             = 0;
    long long b = 0, e = 0;
    if (i < n) {
      v = F[i];
      b = (long long)a.off[v];
      e = (long long)a.off[v + 1];
    }
    long long const len = e - b;
    // light rows: the wave's lanes step through their rows together
    bool const light    = len > 0 && len < kCoreWaveRow;
    long long const top = wave_max_ll(light ? len : 0);
    for (long long t = 0; t < top; ++t) {
      V u      = 0;
      bool hit = false;
      if (light && t < len) hit = peel_entry(a, k, v, b, b + t, u, mn);
      list_append_if(next, nnext, cap, &st->bad, hit, u);
    }
    list_append_if(a.mids, &st->nmid, a.mid_cap, &st->bad, len >= kCoreWaveRow && len < kCoreHubRow, v);
    list_append_if(a.hubs, &st->nhub, a.hub_cap, &st->bad, len >= kCoreHubRow, v);
  }
  publish_min(&st->mindeg, mn);
}

// The rows this round's k_core_peel listed for a wave: one wave per row, dealt over the grid (a late
// frontier is a few thousand long rows: left to the waves that read them they would keep a few CUs busy).
template <typename V, typename E>
__global__ __launch_bounds__(kCoreBlock) void k_core_peel_waves(core_args<V, E> a)
{
  core_state<E>* st = a.st;
  if (st->done) return;
  unsigned long long n = st->nmid;
  if (n > a.mid_cap) n = a.mid_cap;
  if (n == 0) return;
  int const lane = threadIdx.x & 63;
  E const k      = st->k;
  int const fp   = st->fp;
  V* const next  = a.front[fp ^ 1];
  unsigned long long* const nnext = &st->nf[fp ^ 1];
  unsigned long long const cap    = (unsigned long long)a.nv;
  E mn           = std::numeric_limits<E>::max();
  unsigned long long const wave   = (blockIdx.x * (unsigned long long)kCoreBlock + threadIdx.x) >> 6;
  unsigned long long const waves  = ((unsigned long long)gridDim.x * kCoreBlock) >> 6;
  for (unsigned long long r = wave; r < n; r += waves) {  // wave-uniform
    V const v         = a.mids[r];
    long long const b = (long long)a.off[v], e = (long long)a.off[v + 1];
    for (long long j0 = b; j0 < e; j0 += 64) {
      long long const j = j0 + lane;
      V u               = 0;
      bool hit          = false;
      if (j < e) hit = peel_entry(a, k, v, b, j, u, mn);
      list_append_if(next, nnext, cap, &st->bad, hit, u);
    }
  }
  publish_min(&st->mindeg, mn);
}

// The hub rows this round's k_core_peel listed: every row in segments dealt over the grid, each row's
// first segment on another block so that several short hub rows do not queue on the same blocks.
template <typename V, typename E>
__global__ __launch_bounds__(kCoreBlock) void k_core_peel_hubs(core_args<V, E> a)
{
  core_state<E>* st = a.st;
  if (st->done) return;
  unsigned long long n = st->nhub;
  if (n > a.hub_cap) n = a.hub_cap;
  if (n == 0) return;
  int const tid = threadIdx.x;
  E const k     = st->k;
  int const fp  = st->fp;
  V* const next = a.front[fp ^ 1];
  unsigned long long* const nnext = &st->nf[fp ^ 1];
  unsigned long long const cap    = (unsigned long long)a.nv;
  E mn          = std::numeric_limits<E>::max();
  for (unsigned long long h = 0; h < n; ++h) {
    V const v         = a.hubs[h];
    long long const b = (long long)a.off[v], e = (long long)a.off[v + 1];
    long long const first = (long long)((blockIdx.x + gridDim.x - (unsigned)((h * kCoreHubSkew) % gridDim.x)) % gridDim.x);
    for (long long s0 = b + first * kCoreHubSeg; s0 < e; s0 += (long long)gridDim.x * kCoreHubSeg) {
      long long const s1 = s0 + kCoreHubSeg < e ? s0 + kCoreHubSeg : e;
      for (long long j0 = s0; j0 < s1; j0 += kCoreBlock) {
        long long const j = j0 + tid;
        V u               = 0;
        bool hit          = false;
        if (j < s1) hit = peel_entry(a, k, v, b, j, u, mn);
        list_append_if(next, nnext, cap, &st->bad, hit, u);
      }
    }
  }
  publish_min(&st->mindeg, mn);
}

// ---------------------------------------------------------------- control
template <typename E>
__global__ void k_core_ctl(core_state<E>* st)
{
  if (st->done) return;
  ++st->rounds;
  int const fp = st->fp;
  int rp       = st->rp;
  if (st->scan) {  // the scan filled the other remaining list
    rp ^= 1;
    st->rp         = rp;
    st->nr[rp ^ 1] = 0;
    st->scan       = 0;
    st->first      = 0;
    if (st->nf[fp]) ++st->levels;
  }
  st->nmid   = 0;
  st->nhub   = 0;
  st->nf[fp] = 0;
  if (st->bad) {
    st->done = 1;
  } else if (st->nf[fp ^ 1]) {  // more of this level
    st->fp = fp ^ 1;
  } else if (st->nr[rp] == 0 || st->mindeg == std::numeric_limits<E>::max()) {
    st->done = 1;
  } else {  // the next level that can hold a vertex; empty ones in between are skipped
    st->k      = st->mindeg;
    st->mindeg = std::numeric_limits<E>::max();
    st->scan   = 1;
  }
}

inline unsigned core_grid(int per_cu) { return (unsigned)(std::max(device_cu_count(), 1) * per_cu); }

// deg = core numbers of every internal id (nv entries, edge type), delta = 1 or 2
template <typename V, typename E>
void core_numbers(handle_t& h, graph_t& g, E delta, bool expensive, E* deg)
{
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  reset_hot(h);
  if (nv == 0) return;
  if (g.num_edges == 0) {
    HIP_CHECK(hipMemsetAsync(deg, 0, (size_t)nv * sizeof(E), s));
    return;
  }
  adjacency_t& adj = ensure_adjacency(h, g, g.store_transposed);  // symmetric: either orientation
  E const* off     = adj.offsets.data<E>();
  V const* idx     = adj.indices.data<V>();
  dbuf<int> loops(1, s);
  HIP_CHECK(hipMemsetAsync(loops.data(), 0, sizeof(int), s));
  HIP_CHECK(hipMemsetAsync(deg, 0, (size_t)nv * sizeof(E), s));
  hipLaunchKernelGGL((k_core_degree<V, E>),
                     dim3(grid_for((size_t)g.num_edges, kCoreSpan * (kCoreBlock / 64), core_grid(kCoreDegreePerCu))),
                     dim3(kCoreBlock), 0, s, off, idx, nv, delta, deg, loops.data());
  CGX_LAUNCH_CHECK();
  if (expensive)  // core_number_impl.cuh:103-106
    CGX_INPUT(to_host_scalar(loops.data(), s) == 0, "Invalid input argument: graph_view has self-loops.");

  bool const compact = h.tune.core_scan != 0;
  dbuf<V> lists((size_t)nv * (compact ? 4 : 2), s);
  unsigned long long const hub_cap = (unsigned long long)(g.num_edges / kCoreHubRow + 1);
  dbuf<V> hubs((size_t)hub_cap, s);
  // a vertex is listed at most once in the whole call; the counts restart every round
  unsigned long long const mid_cap = (unsigned long long)std::min<int64_t>(nv, g.num_edges / kCoreWaveRow + 1);
  dbuf<V> mids((size_t)mid_cap, s);
  dbuf<core_state<E>> st(1, s);
  core_args<V, E> a{};
  a.off      = off;
  a.idx      = idx;
  a.nv       = nv;
  a.deg      = deg;
  a.delta    = delta;
  a.front[0] = lists.data();
  a.front[1] = lists.data() + nv;
  a.rem[0]   = compact ? lists.data() + 2 * nv : nullptr;
  a.rem[1]   = compact ? lists.data() + 3 * nv : nullptr;
  a.mids     = mids.data();
  a.mid_cap  = mid_cap;
  a.hubs     = hubs.data();
  a.hub_cap  = hub_cap;
  a.st       = st.data();
  a.compact  = compact ? 1 : 0;
  hipLaunchKernelGGL(k_core_init<E>, dim3(1), dim3(1), 0, s, st.data(), delta);
  CGX_LAUNCH_CHECK();

  unsigned const grid = core_grid(kCoreGridPerCu), hub_grid = core_grid(kCoreHubPerCu);
  auto* hs            = h.pinned_as<core_state<E>>();
  // every round peels a vertex or is the one empty scan round before a round that does
  unsigned long long const round_cap = 2ull * (unsigned long long)nv + 4ull;
  size_t launches = 0;
  chunk_timer timer{h, s};  // one interval per round, folded after every chunk's read
  while (true) {
    for (int r = 0; r < kCoreChunkRounds; ++r) {
      hipLaunchKernelGGL((k_core_scan<V, E>), dim3(grid), dim3(kCoreBlock), 0, s, a);
      timer.begin();
      hipLaunchKernelGGL((k_core_peel<V, E>), dim3(grid), dim3(kCoreBlock), 0, s, a);
      hipLaunchKernelGGL((k_core_peel_waves<V, E>), dim3(grid), dim3(kCoreBlock), 0, s, a);
      hipLaunchKernelGGL((k_core_peel_hubs<V, E>), dim3(hub_grid), dim3(kCoreBlock), 0, s, a);
      timer.end();
      hipLaunchKernelGGL(k_core_ctl<E>, dim3(1), dim3(1), 0, s, st.data());
      CGX_LAUNCH_CHECK();
    }
    launches += 3 * (size_t)kCoreChunkRounds;
    HIP_CHECK(hipMemcpyAsync(hs, st.data(), sizeof(core_state<E>), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    timer.fold();
    CGX_EXPECTS(!hs->bad, CUGRAPH_UNKNOWN_ERROR, "core_number: a vertex list overflowed");
    if (hs->done) break;
    CGX_EXPECTS(hs->rounds <= round_cap, CUGRAPH_UNKNOWN_ERROR, "core_number: more rounds than vertices allow");
  }
  h.last_iterations = (size_t)hs->rounds;
  timer.report(launches);
}

// ---------------------------------------------------------------- k-core
// core[ids[i]] = vals[i]; an id outside [0, nv) is skipped and flagged
template <typename V, typename E>
__global__ __launch_bounds__(kCoreBlock) void k_core_scatter(V const* ids, E const* vals, size_t n, int64_t nv, E* out,
                                                            int* bad)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    int64_t const id = (int64_t)ids[i];
    if (id >= 0 && id < nv) out[id] = vals[i];
    else atomicOr(bad, 1);
  }
}

template <typename V, typename E>
__device__ __forceinline__ bool kcore_keep(V const* idx, E const* cn, unsigned long long k, int64_t v, long long b,
                                           long long j)
{
  V const u = idx[j];
  if ((int64_t)u == v || (j > b && idx[j - 1] == u)) return false;
  return (unsigned long long)cn[u] >= k;
}

// row_extract.hpp's test: the rows of the core's vertices, their entries whose other end is in the
// core too (no loops, no repeats); weights lie beside the entries
template <typename V, typename E>
struct kcore_rows {
  V const* idx;
  E const* cn;
  unsigned long long k;
  __device__ __forceinline__ bool row(int64_t v) const { return (unsigned long long)cn[v] >= k; }
  __device__ __forceinline__ bool keep(int64_t v, long long b, long long j) const
  {
    return kcore_keep(idx, cn, k, v, b, j);
  }
  __device__ __forceinline__ long long wpos(long long j) const { return j; }
};

template <typename V, typename E, typename W>
void k_core_impl(handle_t& h, graph_t& g, size_t k, E delta, core_result_t const* given, bool expensive,
                 k_core_result_t& res)
{
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  dbuf<E> cn;
  if (given) {
    // c_api/k_core.cpp: the core result's arrays are in the graph's types
    CGX_INPUT(given->vertices && given->core_numbers && given->vertices->size == given->core_numbers->size,
              "Invalid input argument: core_result vertices and core_numbers differ in length");
    CGX_INPUT(given->vertices->type == g.vertex_type, "vertex type of graph and core_result vertices must match");
    CGX_INPUT(given->core_numbers->type == g.edge_type, "edge type of graph and core_result core_numbers must match");
  }
  if (nv == 0 || g.num_edges == 0) {
    reset_hot(h);
    return alloc_edge_arrays(g, 0, s, res.src, res.dst, res.weights);
  }
  adjacency_t& adj = ensure_adjacency(h, g, g.store_transposed);  // symmetric: either orientation
  cn.resize((size_t)nv, s);
  if (given) {
    reset_hot(h);
    size_t const n = given->vertices->size;
    HIP_CHECK(hipMemsetAsync(cn.data(), 0, (size_t)nv * sizeof(E), s));  // not listed: core 0
    if (n) {
      dbuf<V> ids(n, s);
      HIP_CHECK(hipMemcpyAsync(ids.data(), given->vertices->buf.data(), n * sizeof(V), hipMemcpyDeviceToDevice, s));
      renumber_ext_to_int_unchecked(h, g, ids.data(), n);  // ids not in the graph become -1
      dbuf<int> bad(1, s);
      HIP_CHECK(hipMemsetAsync(bad.data(), 0, sizeof(int), s));
      hipLaunchKernelGGL((k_core_scatter<V, E>), dim3(grid_for(n, kCoreBlock, 4096)), dim3(kCoreBlock), 0, s,
                         (V const*)ids.data(), (E const*)given->core_numbers->buf.data<E>(), n, nv, cn.data(),
                         bad.data());
      CGX_LAUNCH_CHECK();
      if (expensive)
        CGX_INPUT(to_host_scalar(bad.data(), s) == 0,
                  "Invalid input argument: core_result holds a vertex id that is not in the graph.");
    }
  } else {
    core_numbers<V, E>(h, g, delta, expensive, cn.data());
  }
  V const* idx = adj.indices.data<V>();
  extract_rows(h, g, adj.offsets.data<E>(), idx, g.weighted ? adj.weights.data<W>() : (W const*)nullptr,
               kcore_rows<V, E>{idx, cn.data(), (unsigned long long)k}, res.src, res.dst, res.weights);
}

}  // namespace

// delta: 1 (K_CORE_DEGREE_TYPE_IN / _OUT) or 2 (_INOUT)
void run_core_number(handle_t& h, graph_t& g, int delta, bool expensive, core_result_t& res)
{
  dispatch_ve(g.vertex_type, g.edge_type, [&](auto t) {
    using T = decltype(t);
    using V = typename T::vertex_t;
    using E = typename T::edge_t;
    res.vertices     = number_map_copy(h, g);
    res.core_numbers = std::make_unique<device_array_t>((size_t)g.num_vertices, g.edge_type, h.stream);
    core_numbers<V, E>(h, g, (E)delta, expensive, res.core_numbers->buf.data<E>());
  });
}

void run_k_core(handle_t& h, graph_t& g, size_t k, int delta, core_result_t const* given, bool expensive,
                k_core_result_t& res)
{
  dispatch_vew(g.vertex_type, g.edge_type, g.weight_type, [&](auto t) {
    using T = decltype(t);
    using E = typename T::edge_t;
    k_core_impl<typename T::vertex_t, E, typename T::weight_t>(h, g, k, (E)delta, given, expensive, res);
  });
}

}  // namespace cgx
