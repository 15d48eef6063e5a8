// Weakly connected components: a lock-free union-find over the symmetric adjacency.
//
// Reference: components/weakly_connected_components_impl.cuh (a frontier-based multi-source
// traversal with "arbitrary" labels) and c_api/weakly_connected_components.cpp.  This build
// keeps the interface and fixes the labels: the label of a vertex is the smallest internal
// id of its component (WCC).
//
// parent[] is the result's label array.  Invariants, held by every store below:
//   * parent[x] <= x, and a slot's value only ever decreases;
//   * a root (parent[x] == x) changes only by a compare-and-swap that hooks it under a
//     SMALLER root, so the smallest id of a set is never hooked and ends as its root;
//   * a non-root slot is only ever lowered (atomic min) to another ancestor.
// So every value read, however stale (the XCD L2s are not coherent), is an ancestor of the
// slot, find() follows strictly decreasing ids and ends, and a failed compare-and-swap
// returns a strictly smaller id to go on from: nothing here can spin.
//
// Phases (all on the handle's stream, no host read):
//   init      parent[v] = min(v, first neighbour)            plain stores, own slot
//   sample    r = 0 .. k-1: link(v, r-th neighbour), compress   (k = option wcc_sample)
//   pick      giant = root of the largest-degree vertex      (vertex 0 when degree sorted)
//   link      rows whose root is not the giant: neighbours from position k on, by degree:
//             a thread per light row, a wave per row from 64 entries, hub rows (from 1024)
//             listed and spread over the whole grid in 1024-entry segments
//   compress  parent[v] = root(v)
// A skipped row loses nothing: the graph is symmetric, so an edge to a vertex outside the
// giant's set is linked from that vertex's row (or was one of its first k entries).  The
// guess can therefore only change the time taken, never a label.
#include "capi.hpp"
#include "prims.hpp"

namespace cgx {

namespace {

constexpr int kWccBlock  = 256;
constexpr int kWaveRow   = 64;    // rows with at least this many entries left: one wave
constexpr int kHubRow    = 1024;  // ... and from here on: listed, the whole grid in segments
constexpr int kHubSeg    = 1024;  // entries per block and step of a hub row
constexpr int kHubBlocks = 2048;

// root of x, halving the path on the way: a non-root slot is lowered to its grandparent
template <typename V>
__device__ __forceinline__ V find(V* parent, V x)
{
  V q = ld_relaxed(parent + x);
  while (q != x) {
    V g = ld_relaxed(parent + q);
    if (g == q) return q;
    __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = g;
    q = ld_relaxed(parent + x);
  }
  return x;
}

// joins the sets of u and v, returns the root they share afterwards as far as this thread saw
template <typename V>
__device__ __forceinline__ V link(V* parent, V u, V v)
{
  V ru = find(parent, u), rv = find(parent, v);
  while (ru != rv) {
    V hi = ru > rv ? ru : rv, lo = ru > rv ? rv : ru;
    V seen = hi;
    if (__hip_atomic_compare_exchange_strong(parent + hi, &seen, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT))
      return lo;
    // hi was hooked by someone else meanwhile: seen < hi is its parent
    ru = find(parent, seen);
    rv = find(parent, lo);
  }
  return ru;
}

template <typename V, typename E>
__global__ __launch_bounds__(kWccBlock) void k_wcc_init(E const* off, V const* idx, int64_t nv, V* parent)
{
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) {
    E b = off[v], e = off[v + 1];
    V p = (V)v;
    if (e > b) {  // an empty row has no first entry (the last vertex: off[v] == E)
      V n0 = idx[b];
      p    = n0 < p ? n0 : p;
    }
    parent[v] = p;
  }
}

template <typename V, typename E>
__global__ __launch_bounds__(kWccBlock) void k_wcc_sample(E const* off, V const* idx, int64_t nv, int r, V* parent)
{
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) {
    E b = off[v], e = off[v + 1];
    if (e - b > (E)r) link(parent, (V)v, idx[b + r]);
  }
}

template <typename V>
__global__ __launch_bounds__(kWccBlock) void k_wcc_compress(int64_t nv, V* parent)
{
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) {
    V p = ld_relaxed(parent + v);
    if (p == (V)v) continue;
    V r = find(parent, p);
    // atomic min, not a store: another thread's halving may still lower this slot to an
    // ancestor above the root, and must not land after a plain store of the root
    if (r != p) __hip_atomic_fetch_min(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// st[0] = largest degree, st[1] = the smallest vertex that has it (st = {0, ~0} before)
template <typename E>
__global__ __launch_bounds__(kWccBlock) void k_wcc_maxdeg(E const* off, int64_t nv, unsigned long long* st)
{
  unsigned long long m = 0;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long d = (unsigned long long)(off[v + 1] - off[v]);
    m                    = d > m ? d : m;
  }
  for (int o = 32; o > 0; o >>= 1) {
    unsigned long long t = __shfl_xor(m, o, 64);
    m                    = t > m ? t : m;
  }
  if ((threadIdx.x & 63) == 0 && m > 0) atomicMax(st, m);
}

template <typename E>
__global__ __launch_bounds__(kWccBlock) void k_wcc_argmax(E const* off, int64_t nv, unsigned long long* st)
{
  unsigned long long const m = st[0];
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nv; v += (int64_t)gridDim.x * blockDim.x)
    if ((unsigned long long)(off[v + 1] - off[v]) == m) atomicMin(st + 1, (unsigned long long)v);
}

// giant[0] = root of the guessed vertex (after a compress: its parent)
template <typename V>
__global__ void k_wcc_pick(V const* parent, unsigned long long const* st, int64_t nv, V* giant)
{
  unsigned long long hub = st ? st[1] : 0ull;
  if (hub >= (unsigned long long)nv) hub = 0;
  giant[0] = parent[hub];
}

// Links every row that is not in the giant's set with its entries from position k on.
// A block takes 256 consecutive rows at a time: light rows by their thread, rows with
// 64..1023 entries left one after the other by their wave, longer rows go to `hubs`.
template <typename V, typename E>
__global__ __launch_bounds__(kWccBlock) void k_wcc_link_rows(E const* off, V const* idx, int64_t nv, int k,
                                                            V const* giant, V* parent, V* hubs,
                                                            unsigned* hub_count, unsigned hub_cap)
{
  int const tid = threadIdx.x, lane = tid & 63;
  V const g0 = giant ? giant[0] : (V)-1;
  for (int64_t base = blockIdx.x * (int64_t)kWccBlock; base < nv; base += (int64_t)gridDim.x * kWccBlock) {
    int64_t const v = base + tid;
    long long b = 0, e = 0;
    if (v < nv) {
      b = (long long)off[v] + k;
      e = (long long)off[v + 1];
      if (giant && ld_relaxed(parent + v) == g0) e = b;  // in the giant's set: nothing to do
    }
    long long const rem = e > b ? e - b : 0;
    if (rem > 0 && rem < kWaveRow) {
      V cur = (V)v;
      for (long long j = b; j < e; ++j) cur = link(parent, cur, idx[j]);
    } else if (rem >= kHubRow) {
      unsigned pos = atomicAdd(hub_count, 1u);
      if (pos < hub_cap) hubs[pos] = (V)v;
    }
    unsigned long long m = __ballot(rem >= kWaveRow && rem < kHubRow);
    while (m) {  // wave-uniform
      int const l = __ffsll((long long)m) - 1;
      m &= m - 1;
      long long const bb = __shfl(b, l, 64), ee = __shfl(e, l, 64);
      V cur = (V)(base + (tid - lane) + l);
      for (long long j = bb + lane; j < ee; j += 64) cur = link(parent, cur, idx[j]);
    }
  }
}

// The listed hub rows: every row's remaining entries in 1024-entry segments dealt over the grid.
template <typename V, typename E>
__global__ __launch_bounds__(kWccBlock) void k_wcc_link_hubs(E const* off, V const* idx, int k, V* parent,
                                                            V const* hubs, unsigned const* hub_count,
                                                            unsigned hub_cap)
{
  unsigned n = hub_count[0];
  if (n > hub_cap) n = hub_cap;
  for (unsigned i = 0; i < n; ++i) {
    V const v         = hubs[i];
    long long const b = (long long)off[v] + k, e = (long long)off[v + 1];
    V cur             = v;
    for (long long s0 = b + (long long)blockIdx.x * kHubSeg; s0 < e; s0 += (long long)gridDim.x * kHubSeg) {
      long long const s1 = s0 + kHubSeg < e ? s0 + kHubSeg : e;
      for (long long j = s0 + threadIdx.x; j < s1; j += kWccBlock) cur = link(parent, cur, idx[j]);
    }
  }
}

inline unsigned wcc_grid(int64_t n) { return grid_for((size_t)(n > 0 ? n : 1), kWccBlock, 1u << 16); }

template <typename V, typename E>
void wcc_impl(handle_t& h, graph_t& g, labeling_result_t& res)
{
  hipStream_t s     = h.stream;
  int64_t const nv  = g.num_vertices;
  res.vertices      = number_map_copy(h, g);
  res.labels        = std::make_unique<device_array_t>((size_t)nv, g.vertex_type, s);
  reset_hot(h);
  if (nv == 0) return;
  // symmetric: either orientation is the same adjacency
  adjacency_t& adj = ensure_adjacency(h, g, g.store_transposed);
  E const* off     = adj.offsets.data<E>();
  V const* idx     = adj.indices.data<V>();
  V* parent        = res.labels->buf.data<V>();
  int const k      = g.num_edges > 0 ? std::max(h.tune.wcc_sample, 0) : 0;
  unsigned const grid = wcc_grid(nv);
  size_t launches  = 0;

  hipLaunchKernelGGL((k_wcc_init<V, E>), dim3(grid), dim3(kWccBlock), 0, s, off, idx, nv, parent);
  CGX_LAUNCH_CHECK();
  if (g.num_edges == 0) return;  // every vertex is its own component

  dbuf<V> giant;
  dbuf<unsigned long long> st;
  if (k > 0) {
    giant.resize(1, s);
    if (!adj.degree_sorted) {  // guess: the set of the largest-degree vertex
      st.resize(2, s);
      HIP_CHECK(hipMemsetAsync(st.data(), 0, sizeof(unsigned long long), s));
      HIP_CHECK(hipMemsetAsync(st.data() + 1, 0xff, sizeof(unsigned long long), s));
      hipLaunchKernelGGL(k_wcc_maxdeg<E>, dim3(grid), dim3(kWccBlock), 0, s, off, nv, st.data());
      hipLaunchKernelGGL(k_wcc_argmax<E>, dim3(grid), dim3(kWccBlock), 0, s, off, nv, st.data());
      CGX_LAUNCH_CHECK();
    }
  }
  unsigned const hub_cap = (unsigned)std::min<int64_t>(g.num_edges / kHubRow + 1, (int64_t)1 << 30);
  dbuf<V> hubs(hub_cap, s);
  dbuf<unsigned> hub_count(1, s);
  HIP_CHECK(hipMemsetAsync(hub_count.data(), 0, sizeof(unsigned), s));

  chunk_timer timer{h, s};
  timer.begin();
  for (int r = 0; r < k; ++r) {
    hipLaunchKernelGGL((k_wcc_sample<V, E>), dim3(grid), dim3(kWccBlock), 0, s, off, idx, nv, r, parent);
    hipLaunchKernelGGL(k_wcc_compress<V>, dim3(grid), dim3(kWccBlock), 0, s, nv, parent);
    CGX_LAUNCH_CHECK();
    launches += 2;
  }
  if (k > 0) {
    hipLaunchKernelGGL(k_wcc_pick<V>, dim3(1), dim3(1), 0, s, parent, adj.degree_sorted ? nullptr : st.data(), nv,
                       giant.data());
    CGX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((k_wcc_link_rows<V, E>), dim3(wcc_grid(nv)), dim3(kWccBlock), 0, s, off, idx, nv, k,
                     k > 0 ? giant.data() : nullptr, parent, hubs.data(), hub_count.data(), hub_cap);
  hipLaunchKernelGGL((k_wcc_link_hubs<V, E>), dim3(kHubBlocks), dim3(kWccBlock), 0, s, off, idx, k, parent,
                     hubs.data(), hub_count.data(), hub_cap);
  hipLaunchKernelGGL(k_wcc_compress<V>, dim3(grid), dim3(kWccBlock), 0, s, nv, parent);
  CGX_LAUNCH_CHECK();
  launches += 3;
  h.last_iterations = (size_t)k;
  timer.end();
  timer.report(launches);
}

}  // namespace

void run_wcc(handle_t& h, graph_t& g, bool expensive, labeling_result_t& res)
{
  (void)expensive;  // weakly_connected_components_impl.cuh:289-291: nothing to check
  dispatch_ve(g.vertex_type, g.edge_type, [&](auto t) {
    using T = decltype(t);
    wcc_impl<typename T::vertex_t, typename T::edge_t>(h, g, res);
  });
}

}  // namespace cgx
