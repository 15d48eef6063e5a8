// Betweenness and edge betweenness centrality: Brandes' algorithm on the unweighted graph, up to 64
// sources at a time, lane s of a wave carrying source s of the batch.
//
// Reference: centrality/betweenness_centrality.cu (one source at a time, a thread-per-vertex kernel over
// all V vertices per depth, betweenness_centrality_kernels.cuh:27-118) and the C entry points of later
// cuGraph releases (the 22.10 snapshot has none).  The arithmetic per source is the reference's; the
// schedule is not (Betweenness centrality).
//
// State of a batch of B sources, each [V x B] with the source index fastest, so that a wave that visits
// vertex w reads or writes one contiguous run of B values (256 B of levels, 512 B of path counts at B = 64):
//   dist   int32   level of w from source s, -1 if not reached
//   sigma  double  shortest paths from source s to w
//   delta  double  dependency of source s on w
// plus the union frontiers: level d's list holds every vertex that is at level d for at least one source of
// the batch, once (claimed through stamp[w], which holds the id of the last (batch, level) that listed w).
// The lists are kept one after the other: they are the stack of the backward sweep.
//
// Forward, level d:
//   discover  a wave per vertex u of list d-1; lanes with dist[u][s] == d-1 are active.  For every
//             out-neighbour w a lane that sees dist[w][s] == -1 stores d (racing waves store the same
//             value); if any lane of the wave stored, lane 0 exchanges stamp[w] and appends w to list d when
//             the old value was another level's.  The list's order may differ from run to run; nothing
//             below depends on it.
//   count     a wave per vertex v of list d; lane s with dist[v][s] == d sums sigma[u][s] over the
//             in-neighbours u with dist[u][s] == d-1.
// Backward, level d from the deepest down:
//   back      a wave per vertex v of list d; lane s with dist[v][s] == d sums
//             sigma[v][s] * ((1 + delta[w][s]) / sigma[w][s]) over the out-neighbours w with
//             dist[w][s] == d+1 (accumulation_kernel's arithmetic).  For edge betweenness the term of an
//             entry is summed over the lanes by a butterfly and lane 0 adds it to eb[j]: entry j belongs
//             to one row, a row to one wave of the launch, so this is a plain read-add-write.
// After the batch a thread per vertex adds delta[v][0 .. B) into bc[v] in source order.
//
// No floating-point atomics anywhere, and every sum has one fixed shape: a row is summed in blocks of 64
// consecutive entries by row position (a block in row order from zero, the blocks in row order from
// zero).  A row longer than bc_row_split entries is cut into segments of that many entries, a wave each;
// the segments store their blocks' sums and a wave per row adds them in the same order, so the cut (a
// multiple of 64) changes no bit.  A source's values do not depend on its lane or on the other sources of
// its batch, and bc[v] is added in source order across the batches, so the vertex scores are a pure
// function of (graph, source list).  Edge scores add the lanes of a batch first: they are the same on
// every run at a given batch size.
#include "capi.hpp"
#include "prims.hpp"

#include <algorithm>
#include <climits>
#include <vector>

// a * b + c must round twice wherever it is written, in every kernel alike
#pragma clang fp contract(off)

namespace cgx {

namespace {

constexpr int kBcBlock     = 256;
constexpr int kBcGridPerCu = 8;    // blocks per CU of the wave-per-row grids, at most
constexpr int kBcStep      = 64;   // entries per block of a row's sum
constexpr int kBcAhead     = 4;    // entries whose state reads a wave has in flight together (divides kBcStep)
constexpr int32_t kBcNoLevel = -2; // stands for the level of an entry that is not the lane's to read

enum { BC_DISCOVER = 0, BC_COUNT = 1, BC_BACK = 2 };

template <typename T>
__device__ __forceinline__ void bc_st(T* p, T v)
{
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the same tree in every lane: lane l adds its partner's value, and a + b == b + a
__device__ __forceinline__ double bc_wave_sum(double v)
{
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename V, typename E>
struct bc_args {
  E const* off;  // the rows this phase walks: out-edges (discover, back) or in-edges (count)
  V const* idx;
  int nb;        // sources of the batch = stride of the state
  int d;         // the level
  int32_t* dist;
  double* sigma;
  double* delta;
  long long split;  // rows above it are hub rows
  V const* list;    // the phase's list (discover: level d-1, else level d)
  long long n;
  // discover
  int* stamp;
  int stamp_id;
  V* next;  // level d's list
  unsigned long long* nnext;
  unsigned long long next_cap;
  double* eb;  // edge scores by out-edge position (edge betweenness)
  // hub rows of `off`
  int const* seg_hub;
  int const* seg_k;
  long long nseg;
  V const* hub_v;
  long long const* hub_pb;  // a hub row's first block in `partial`
  long long nhub;
  double* partial;  // [blocks x nb]
};

// Entries [j0, min(j0 + 64, e)) of a row, for the lane's source: their sum (count, back), or their
// discovery.  Every lane of the wave must call it.
template <int PH, bool EDGE, typename V, typename E>
__device__ __forceinline__ double bc_block(bc_args<V, E> const& a, bool mine, double sv, long long j0, long long e,
                                           int lane)
{
  long long const j = j0 + lane;
  V const mine_w    = j < e ? a.idx[j] : (V)0;
  int const cnt     = (int)(e - j0 < kBcStep ? e - j0 : kBcStep);
  double q          = 0;
  // kBcAhead entries at a time: their levels are read first, then what depends on a level, so that a wave
  // has several reads in flight (one entry at a time left it waiting on one 256 B read after the other).
  // The adds keep the entries' order, and an entry that does not count adds 0.0, which changes no bit of a
  // non-negative sum.
  for (int t0 = 0; t0 < cnt; t0 += kBcAhead) {  // wave-uniform
    V w[kBcAhead];
    size_t p[kBcAhead];
    int32_t dd[kBcAhead];
#pragma unroll
    for (int u = 0; u < kBcAhead; ++u) {
      w[u] = __shfl(mine_w, (t0 + u) & 63, 64);  // past cnt: another entry's vertex or 0, never used
      p[u] = (size_t)w[u] * (size_t)a.nb + (size_t)lane;  // read by lanes below nb only (mine)
    }
#pragma unroll
    for (int u = 0; u < kBcAhead; ++u) dd[u] = (mine && t0 + u < cnt) ? ld_relaxed(a.dist + p[u]) : kBcNoLevel;
    if constexpr (PH == BC_DISCOVER) {
#pragma unroll
      for (int u = 0; u < kBcAhead; ++u) {
        if (t0 + u >= cnt) break;  // wave-uniform
        // a level read before another wave's store of the same d: this wave stores d too, and the exchange
        // below shows that the vertex is listed already
        bool const stored = dd[u] == -1;
        if (stored) bc_st(a.dist + p[u], (int32_t)a.d);
        if (__ballot(stored) && lane == 0 && ld_relaxed(a.stamp + w[u]) != a.stamp_id &&
            __hip_atomic_exchange(a.stamp + w[u], a.stamp_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) !=
              a.stamp_id) {
          unsigned long long const pos =
            __hip_atomic_fetch_add(a.nnext, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (pos < a.next_cap) a.next[pos] = w[u];  // (a vertex is claimed once per level: never above V)
        }
      }
    } else if constexpr (PH == BC_COUNT) {
      double sg[kBcAhead];
#pragma unroll
      for (int u = 0; u < kBcAhead; ++u) sg[u] = dd[u] == a.d - 1 ? a.sigma[p[u]] : 0.0;
#pragma unroll
      for (int u = 0; u < kBcAhead; ++u) q += sg[u];
    } else {
      double dl[kBcAhead], sw[kBcAhead];
#pragma unroll
      for (int u = 0; u < kBcAhead; ++u) {
        bool const hit = dd[u] == a.d + 1;
        dl[u]          = hit ? a.delta[p[u]] : 0.0;
        sw[u]          = hit ? a.sigma[p[u]] : 1.0;
      }
#pragma unroll
      for (int u = 0; u < kBcAhead; ++u) {
        bool const hit = dd[u] == a.d + 1;
        double term    = 0;
        if (hit) {
          double const factor = (1.0 + dl[u]) / sw[u];
          term                = sv * factor;
        }
        q += term;
        if constexpr (EDGE) {
          if (__ballot(hit)) {  // wave-uniform
            double const all = bc_wave_sum(term);
            if (lane == 0) a.eb[j0 + t0 + u] += all;
          }
        }
      }
    }
  }
  return q;
}

template <int PH>
__device__ __forceinline__ int bc_own_level(int d)
{
  return PH == BC_DISCOVER ? d - 1 : d;
}

// The phase's list, a wave per vertex; hub rows are left to k_bc_hubs.
template <int PH, bool EDGE, typename V, typename E>
__global__ __launch_bounds__(kBcBlock) void k_bc_rows(bc_args<V, E> a)
{
  int const lane        = threadIdx.x & 63;
  long long const wave  = (blockIdx.x * (long long)kBcBlock + threadIdx.x) >> 6;
  long long const waves = ((long long)gridDim.x * kBcBlock) >> 6;
  for (long long r = wave; r < a.n; r += waves) {  // wave-uniform
    V const v         = a.list[r];
    long long const b = (long long)a.off[v], e = (long long)a.off[v + 1];
    if (e - b > a.split) continue;
    size_t const pv = (size_t)v * (size_t)a.nb + (size_t)lane;
    bool const mine = lane < a.nb && a.dist[pv] == bc_own_level<PH>(a.d);
    double const sv = (PH == BC_BACK && mine) ? a.sigma[pv] : 0.0;
    double acc      = 0;
    for (long long j0 = b; j0 < e; j0 += kBcStep) acc += bc_block<PH, EDGE>(a, mine, sv, j0, e, lane);
    if (PH == BC_COUNT && mine) a.sigma[pv] = acc;
    if (PH == BC_BACK && mine) a.delta[pv] = acc;
  }
}

// Every hub row's segments, a wave each; a row none of whose lanes is at the phase's level is skipped.
// Count and back store every block's sum for k_bc_hub_sum.
template <int PH, bool EDGE, typename V, typename E>
__global__ __launch_bounds__(kBcBlock) void k_bc_hubs(bc_args<V, E> a)
{
  int const lane        = threadIdx.x & 63;
  long long const wave  = (blockIdx.x * (long long)kBcBlock + threadIdx.x) >> 6;
  long long const waves = ((long long)gridDim.x * kBcBlock) >> 6;
  for (long long sg = wave; sg < a.nseg; sg += waves) {  // wave-uniform
    int const h     = a.seg_hub[sg];
    V const v       = a.hub_v[h];
    size_t const pv = (size_t)v * (size_t)a.nb + (size_t)lane;
    bool const mine = lane < a.nb && a.dist[pv] == bc_own_level<PH>(a.d);
    if (!__ballot(mine)) continue;
    long long const k   = a.seg_k[sg];
    long long const end = (long long)a.off[v + 1];
    long long const b   = (long long)a.off[v] + k * a.split;
    long long const e   = b + a.split < end ? b + a.split : end;
    double const sv     = (PH == BC_BACK && mine) ? a.sigma[pv] : 0.0;
    long long blk       = a.hub_pb[h] + k * (a.split / kBcStep);
    for (long long j0 = b; j0 < e; j0 += kBcStep, ++blk) {
      double const q = bc_block<PH, EDGE>(a, mine, sv, j0, e, lane);
      if (PH != BC_DISCOVER && lane < a.nb) a.partial[(size_t)blk * (size_t)a.nb + (size_t)lane] = q;
    }
  }
}

// A wave per hub row: its blocks' sums in row order, as k_bc_rows adds them.
template <int PH, typename V, typename E>
__global__ __launch_bounds__(kBcBlock) void k_bc_hub_sum(bc_args<V, E> a)
{
  int const lane        = threadIdx.x & 63;
  long long const wave  = (blockIdx.x * (long long)kBcBlock + threadIdx.x) >> 6;
  long long const waves = ((long long)gridDim.x * kBcBlock) >> 6;
  for (long long h = wave; h < a.nhub; h += waves) {  // wave-uniform
    V const v       = a.hub_v[h];
    size_t const pv = (size_t)v * (size_t)a.nb + (size_t)lane;
    bool const mine = lane < a.nb && a.dist[pv] == a.d;
    if (!__ballot(mine)) continue;
    long long const len  = (long long)a.off[v + 1] - (long long)a.off[v];
    long long const nblk = (len + kBcStep - 1) / kBcStep;
    long long const pb   = a.hub_pb[h];
    double acc           = 0;
    if (mine)
      for (long long i = 0; i < nblk; ++i) acc += a.partial[(size_t)(pb + i) * (size_t)a.nb + (size_t)lane];
    if (PH == BC_COUNT && mine) a.sigma[pv] = acc;
    if (PH == BC_BACK && mine) a.delta[pv] = acc;
  }
}

// Level 0: source s of the batch is at level 0 with one path, for lane s alone.
template <typename V>
__global__ void k_bc_init(V const* src, int nb, int32_t* dist, double* sigma, int* stamp, int stamp_id, V* list,
                          unsigned long long* n)
{
  int const s = (int)threadIdx.x;
  if (s >= nb) return;
  V const v      = src[s];
  size_t const p = (size_t)v * (size_t)nb + (size_t)s;
  dist[p]        = 0;
  sigma[p]       = 1.0;
  if (__hip_atomic_exchange(stamp + v, stamp_id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != stamp_id)
    list[__hip_atomic_fetch_add(n, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)] = v;  // at most nb <= V
}

// reach[s] = vertices source s reached, itself included (zero before)
__global__ __launch_bounds__(kBcBlock) void k_bc_reach(int32_t const* dist, long long nv, int nb,
                                                       unsigned long long* reach)
{
  int const lane        = threadIdx.x & 63;
  long long const wave  = (blockIdx.x * (long long)kBcBlock + threadIdx.x) >> 6;
  long long const waves = ((long long)gridDim.x * kBcBlock) >> 6;
  if (lane >= nb) return;
  unsigned long long c = 0;
  for (long long v = wave; v < nv; v += waves) c += dist[(size_t)v * (size_t)nb + (size_t)lane] >= 0 ? 1u : 0u;
  if (c) __hip_atomic_fetch_add(reach + lane, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// bc[v] += the batch's dependencies on v, in source order (betweenness_centrality.cu:297-346: with
// endpoints a reached vertex gains 1 per source and the source the vertices it reached minus 1)
__global__ __launch_bounds__(kBcBlock) void k_bc_accumulate(long long nv, int nb, int32_t const* dist,
                                                            double const* delta, int endpoints,
                                                            unsigned long long const* reach, double* bc)
{
  for (long long v = blockIdx.x * (long long)kBcBlock + threadIdx.x; v < nv; v += (long long)gridDim.x * kBcBlock) {
    double x = bc[v];
    for (int s = 0; s < nb; ++s) {
      size_t const p   = (size_t)v * (size_t)nb + (size_t)s;
      int32_t const dd = dist[p];
      if (dd > 0) {
        if (endpoints) x += 1.0;
        x += delta[p];
      } else if (dd == 0 && endpoints) {
        x += (double)(reach[s] - 1ull);
      }
    }
    bc[v] = x;
  }
}

__global__ __launch_bounds__(kBcBlock) void k_bc_scale(double* p, size_t n, double f)
{
  for (size_t i = blockIdx.x * (size_t)kBcBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBcBlock) p[i] *= f;
}

// ---------------------------------------------------------------- hub rows
// out[0] hub rows (more than split entries), out[1] their segments, out[2] their 64-entry blocks
template <typename E>
__global__ __launch_bounds__(kBcBlock) void k_bc_hub_count(E const* off, long long nv, long long split,
                                                           unsigned long long* out)
{
  for (long long v = blockIdx.x * (long long)kBcBlock + threadIdx.x; v < nv; v += (long long)gridDim.x * kBcBlock) {
    long long const len = (long long)off[v + 1] - (long long)off[v];
    if (len <= split) continue;
    atomicAdd(out + 0, 1ull);
    atomicAdd(out + 1, (unsigned long long)((len + split - 1) / split));
    atomicAdd(out + 2, (unsigned long long)((len + kBcStep - 1) / kBcStep));
  }
}

// The tables of the rows k_bc_hub_count counted (ctr zero before).  Which slot a row gets differs from
// run to run; a row's segments and blocks are consecutive, which is all the sums depend on.
template <typename V, typename E>
__global__ __launch_bounds__(kBcBlock) void k_bc_hub_fill(E const* off, long long nv, long long split,
                                                          unsigned long long* ctr, V* hub_v, long long* hub_pb,
                                                          int* seg_hub, int* seg_k)
{
  for (long long v = blockIdx.x * (long long)kBcBlock + threadIdx.x; v < nv; v += (long long)gridDim.x * kBcBlock) {
    long long const len = (long long)off[v + 1] - (long long)off[v];
    if (len <= split) continue;
    long long const nseg = (len + split - 1) / split;
    long long const h    = (long long)atomicAdd(ctr + 0, 1ull);
    long long const s0   = (long long)atomicAdd(ctr + 1, (unsigned long long)nseg);
    hub_v[h]             = (V)v;
    hub_pb[h]            = (long long)atomicAdd(ctr + 2, (unsigned long long)((len + kBcStep - 1) / kBcStep));
    for (long long k = 0; k < nseg; ++k) {
      seg_hub[s0 + k] = (int)h;
      seg_k[s0 + k]   = (int)k;
    }
  }
}

template <typename V>
struct bc_hubs {
  long long nhub = 0, nseg = 0, nblk = 0;
  dbuf<V> hub_v;
  dbuf<long long> hub_pb;
  dbuf<int> seg_hub, seg_k;
};

template <typename V, typename E>
void bc_build_hubs(handle_t& h, E const* off, long long nv, long long split, bc_hubs<V>& t)
{
  hipStream_t s = h.stream;
  dbuf<unsigned long long> ctr(3, s);
  HIP_CHECK(hipMemsetAsync(ctr.data(), 0, 3 * sizeof(unsigned long long), s));
  unsigned const grid = grid_for((size_t)nv, kBcBlock, 4096);
  hipLaunchKernelGGL(k_bc_hub_count<E>, dim3(grid), dim3(kBcBlock), 0, s, off, nv, split, ctr.data());
  CGX_LAUNCH_CHECK();
  auto const c = to_host(ctr.data(), 3, s);
  t.nhub = (long long)c[0], t.nseg = (long long)c[1], t.nblk = (long long)c[2];
  if (!t.nhub) return;
  CGX_EXPECTS(t.nseg < INT_MAX, CUGRAPH_UNKNOWN_ERROR, "betweenness: too many hub row segments");
  t.hub_v.resize((size_t)t.nhub, s);
  t.hub_pb.resize((size_t)t.nhub, s);
  t.seg_hub.resize((size_t)t.nseg, s);
  t.seg_k.resize((size_t)t.nseg, s);
  HIP_CHECK(hipMemsetAsync(ctr.data(), 0, 3 * sizeof(unsigned long long), s));
  hipLaunchKernelGGL((k_bc_hub_fill<V, E>), dim3(grid), dim3(kBcBlock), 0, s, off, nv, split, ctr.data(),
                     t.hub_v.data(), t.hub_pb.data(), t.seg_hub.data(), t.seg_k.data());
  CGX_LAUNCH_CHECK();
}

inline unsigned bc_wave_grid(long long waves)
{
  unsigned const cap = (unsigned)(std::max(device_cu_count(), 1) * kBcGridPerCu);
  return grid_for((size_t)std::max<long long>(waves, 1) * 64, kBcBlock, cap);
}

// ---------------------------------------------------------------- the sweep
// bc (vertex scores, nv, zero before) or eb (edge scores by out-edge position, zero before) gets the
// unscaled sums over the k sources src[0 .. k) (internal ids)
template <typename V, typename E>
void bc_sweep(handle_t& h, graph_t& g, V const* src, size_t k, bool endpoints, double* bc, double* eb)
{
  hipStream_t s      = h.stream;
  long long const nv = g.num_vertices;
  bool const edges   = eb != nullptr;
  adjacency_t& out   = ensure_adjacency(h, g, false);
  adjacency_t& in    = ensure_adjacency(h, g, true);  // the same object when the graph is symmetric
  long long const split = h.tune.bc_row_split;

  bc_hubs<V> hub_out, hub_in_own;
  bc_build_hubs<V, E>(h, out.offsets.data<E>(), nv, split, hub_out);
  bool const same = &in == &out;
  if (!same) bc_build_hubs<V, E>(h, in.offsets.data<E>(), nv, split, hub_in_own);
  bc_hubs<V>& hub_in = same ? hub_out : hub_in_own;

  // the state: 20 bytes per (vertex, source); the batch is halved until it fits
  int B = (int)std::min<size_t>((size_t)h.tune.bc_batch, k);
  dbuf<int32_t> dist;
  dbuf<double> sigma, delta;
  while (true) {
    try {
      size_t const n = (size_t)nv * (size_t)B;
      dist.resize(n, s);
      sigma.resize(n, s);
      delta.resize(n, s);
      break;
    } catch (cgx::error const& e) {
      if (e.code != CUGRAPH_ALLOC_ERROR || B == 1) throw;
      dist.free();
      sigma.free();
      delta.free();
      B /= 2;
    }
  }
  dbuf<double> partial((size_t)std::max(hub_out.nblk, hub_in.nblk) * (size_t)B, s);
  dbuf<int> stamp((size_t)nv, s);
  HIP_CHECK(hipMemsetAsync(stamp.data(), 0, (size_t)nv * sizeof(int), s));
  int stamp_id = 0;
  dbuf<unsigned long long> ctr(1, s), reach(64, s);
  size_t cap = (size_t)nv * 2 + 64;  // the lists of the batch's levels, grown as the levels come
  dbuf<V> stack(cap, s);
  auto* pinned = h.pinned_as<unsigned long long>();

  bc_args<V, E> a{};
  a.dist    = dist.data();
  a.sigma   = sigma.data();
  a.delta   = delta.data();
  a.split   = split;
  a.stamp   = stamp.data();
  a.nnext   = ctr.data();
  a.eb      = eb;
  a.partial = partial.data();
  auto rows_of = [&](adjacency_t& adj, bc_hubs<V>& t) {
    a.off     = adj.offsets.data<E>();
    a.idx     = adj.indices.data<V>();
    a.seg_hub = t.seg_hub.data();
    a.seg_k   = t.seg_k.data();
    a.nseg    = t.nseg;
    a.hub_v   = t.hub_v.data();
    a.hub_pb  = t.hub_pb.data();
    a.nhub    = t.nhub;
  };
  auto next_stamp = [&] {
    if (stamp_id == INT_MAX) {
      HIP_CHECK(hipMemsetAsync(stamp.data(), 0, (size_t)nv * sizeof(int), s));
      stamp_id = 0;
    }
    return ++stamp_id;
  };
  auto read_count = [&] {
    HIP_CHECK(hipMemcpyAsync(pinned, ctr.data(), sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return (long long)*pinned;
  };

  size_t launches = 0, batches = 0;
  chunk_timer timer{h, s};
  std::vector<long long> first;  // first[d] = where level d's list starts in the stack
  for (size_t base = 0; base < k; base += (size_t)B) {
    int const nb = (int)std::min<size_t>((size_t)B, k - base);
    a.nb         = nb;
    HIP_CHECK(hipMemsetAsync(dist.data(), 0xFF, (size_t)nv * (size_t)nb * sizeof(int32_t), s));
    HIP_CHECK(hipMemsetAsync(ctr.data(), 0, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(k_bc_init<V>, dim3(1), dim3(64), 0, s, src + base, nb, dist.data(), sigma.data(), stamp.data(),
                       next_stamp(), stack.data(), ctr.data());
    CGX_LAUNCH_CHECK();
    first.assign(1, 0);
    long long total = read_count();
    first.push_back(total);
    int depth = 0;  // the deepest level that holds a vertex
    for (int d = 1;; ++d) {
      CGX_EXPECTS(d < INT_MAX - 1, CUGRAPH_UNKNOWN_ERROR, "betweenness: more levels than a level can number");
      if ((size_t)total + (size_t)nv > cap) {  // level d's list has at most nv entries
        size_t const grown = std::max(cap * 2, (size_t)total + (size_t)nv);
        dbuf<V> bigger(grown, s);
        HIP_CHECK(hipMemcpyAsync(bigger.data(), stack.data(), (size_t)total * sizeof(V), hipMemcpyDeviceToDevice, s));
        stack = std::move(bigger);
        cap   = grown;
      }
      HIP_CHECK(hipMemsetAsync(ctr.data(), 0, sizeof(unsigned long long), s));
      rows_of(out, hub_out);
      a.d        = d;
      a.list     = stack.data() + first[d - 1];
      a.n        = first[d] - first[d - 1];
      a.stamp_id = next_stamp();
      a.next     = stack.data() + total;
      a.next_cap = (unsigned long long)nv;
      timer.begin();
      hipLaunchKernelGGL((k_bc_rows<BC_DISCOVER, false, V, E>), dim3(bc_wave_grid(a.n)), dim3(kBcBlock), 0, s, a);
      ++launches;
      if (a.nhub) {
        hipLaunchKernelGGL((k_bc_hubs<BC_DISCOVER, false, V, E>), dim3(bc_wave_grid(a.nseg)), dim3(kBcBlock), 0, s, a);
        ++launches;
      }
      timer.end();
      CGX_LAUNCH_CHECK();
      long long const n = read_count();
      timer.fold();
      CGX_EXPECTS(n <= nv, CUGRAPH_UNKNOWN_ERROR, "betweenness: a level's list overflowed");
      if (n == 0) break;
      depth = d;
      total += n;
      first.push_back(total);
      rows_of(in, hub_in);
      a.list = stack.data() + first[d];
      a.n    = n;
      timer.begin();
      hipLaunchKernelGGL((k_bc_rows<BC_COUNT, false, V, E>), dim3(bc_wave_grid(n)), dim3(kBcBlock), 0, s, a);
      ++launches;
      if (a.nhub) {
        hipLaunchKernelGGL((k_bc_hubs<BC_COUNT, false, V, E>), dim3(bc_wave_grid(a.nseg)), dim3(kBcBlock), 0, s, a);
        hipLaunchKernelGGL((k_bc_hub_sum<BC_COUNT, V, E>), dim3(bc_wave_grid(a.nhub)), dim3(kBcBlock), 0, s, a);
        launches += 2;
      }
      timer.end();
      CGX_LAUNCH_CHECK();
    }
    // backward: the vertex scores need no dependency of a source on itself (level 0), the edge scores do
    rows_of(out, hub_out);
    timer.begin();
    for (int d = depth; d >= (edges ? 0 : 1); --d) {
      a.d    = d;
      a.list = stack.data() + first[d];
      a.n    = first[d + 1] - first[d];
      if (edges) hipLaunchKernelGGL((k_bc_rows<BC_BACK, true, V, E>), dim3(bc_wave_grid(a.n)), dim3(kBcBlock), 0, s, a);
      else hipLaunchKernelGGL((k_bc_rows<BC_BACK, false, V, E>), dim3(bc_wave_grid(a.n)), dim3(kBcBlock), 0, s, a);
      ++launches;
      if (a.nhub) {
        if (edges)
          hipLaunchKernelGGL((k_bc_hubs<BC_BACK, true, V, E>), dim3(bc_wave_grid(a.nseg)), dim3(kBcBlock), 0, s, a);
        else
          hipLaunchKernelGGL((k_bc_hubs<BC_BACK, false, V, E>), dim3(bc_wave_grid(a.nseg)), dim3(kBcBlock), 0, s, a);
        hipLaunchKernelGGL((k_bc_hub_sum<BC_BACK, V, E>), dim3(bc_wave_grid(a.nhub)), dim3(kBcBlock), 0, s, a);
        launches += 2;
      }
    }
    if (!edges) {
      if (endpoints) {
        HIP_CHECK(hipMemsetAsync(reach.data(), 0, 64 * sizeof(unsigned long long), s));
        hipLaunchKernelGGL(k_bc_reach, dim3(bc_wave_grid(nv)), dim3(kBcBlock), 0, s, (int32_t const*)dist.data(), nv,
                           nb, reach.data());
        ++launches;
      }
      hipLaunchKernelGGL(k_bc_accumulate, dim3(grid_for((size_t)nv, kBcBlock, 4096)), dim3(kBcBlock), 0, s, nv, nb,
                         (int32_t const*)dist.data(), (double const*)delta.data(), endpoints ? 1 : 0,
                         (unsigned long long const*)reach.data(), bc);
      ++launches;
    }
    timer.end();
    CGX_LAUNCH_CHECK();
    ++batches;
  }
  HIP_CHECK(hipStreamSynchronize(s));
  h.last_iterations = batches;
  timer.report(launches);
}

// the row of entry t < off[nv]: the first r with off[r + 1] > t
template <typename V, typename E>
__global__ __launch_bounds__(kBcBlock) void k_bc_edge_rows(E const* off, long long nv, long long ne, V* src)
{
  for (long long t = blockIdx.x * (long long)kBcBlock + threadIdx.x; t < ne; t += (long long)gridDim.x * kBcBlock) {
    long long lo = 0, hi = nv - 1;
    while (lo < hi) {
      long long const mid = (lo + hi) >> 1;
      if ((long long)off[mid + 1] <= t) lo = mid + 1;
      else hi = mid;
    }
    src[t] = (V)lo;
  }
}

void bc_scale(handle_t& h, double* p, size_t n, double f)
{
  if (!n || f == 1.0) return;
  hipLaunchKernelGGL(k_bc_scale, dim3(grid_for(n, kBcBlock, 4096)), dim3(kBcBlock), 0, h.stream, p, n, f);
  CGX_LAUNCH_CHECK();
}

template <typename V, typename E>
void bc_impl(handle_t& h, graph_t& g, array_view_t const* vertex_list, bool normalized, bool endpoints,
             centrality_result_t* vres, edge_centrality_result_t* eres)
{
  hipStream_t s      = h.stream;
  long long const nv = g.num_vertices, ne = g.num_edges;
  reset_hot(h);
  // the sources as internal ids: the list's, or every vertex
  size_t const k = vertex_list ? vertex_list->size : (size_t)nv;
  dbuf<V> src(k, s);
  if (vertex_list) {
    if (k) {
      HIP_CHECK(hipMemcpyAsync(src.data(), vertex_list->data, k * sizeof(V), hipMemcpyDefault, s));
      renumber_ext_to_int(h, g, src.data(), k, true);  // throws on an id that is not in the graph
    }
  } else if (k) {
    iota<V>(src.data(), k, (V)0, s);
  }
  double const n     = (double)nv;
  double* values     = nullptr;
  size_t nvalues     = 0;
  if (vres) {
    vres->vertices = number_map_copy(h, g);
    vres->values   = std::make_unique<device_array_t>((size_t)nv, FLOAT64, s);
    values         = vres->values->buf.data<double>();
    nvalues        = (size_t)nv;
  } else {
    eres->src    = std::make_unique<device_array_t>((size_t)ne, g.vertex_type, s);
    eres->dst    = std::make_unique<device_array_t>((size_t)ne, g.vertex_type, s);
    eres->values = std::make_unique<device_array_t>((size_t)ne, FLOAT64, s);
    values       = eres->values->buf.data<double>();
    nvalues      = (size_t)ne;
  }
  if (nvalues) HIP_CHECK(hipMemsetAsync(values, 0, nvalues * sizeof(double), s));
  if (nv && ne && k) bc_sweep<V, E>(h, g, src.data(), k, endpoints, vres ? values : nullptr, vres ? nullptr : values);
  // betweenness_centrality.cu:368-452: one factor for the normalisation, one for the sources used
  double f = 1.0;
  if (vres) {
    if (normalized) {
      if (nv > 2) f /= endpoints ? n * (n - 1.0) : (n - 1.0) * (n - 2.0);
    } else if (g.symmetric) {
      f /= 2.0;
    }
    bc_scale(h, values, nvalues, f);
    if (k > 0 && nv > 2 && (normalized || g.symmetric)) bc_scale(h, values, nvalues, n / (double)k);
  } else {
    if (normalized) {
      if (nv > 1) f /= n * (n - 1.0);
    } else if (g.symmetric) {
      f /= 2.0;
    }
    bc_scale(h, values, nvalues, f);
    if (ne) {
      adjacency_t& out = ensure_adjacency(h, g, false);
      hipLaunchKernelGGL((k_bc_edge_rows<V, E>), dim3(grid_for((size_t)ne, kBcBlock, 8192)), dim3(kBcBlock), 0, s,
                         (E const*)out.offsets.data<E>(), nv, ne, eres->src->buf.data<V>());
      CGX_LAUNCH_CHECK();
      HIP_CHECK(hipMemcpyAsync(eres->dst->buf.data(), out.indices.data(), (size_t)ne * sizeof(V),
                               hipMemcpyDeviceToDevice, s));
      unrenumber_int_to_ext(h, g, eres->src->buf.data(), (size_t)ne);
      unrenumber_int_to_ext(h, g, eres->dst->buf.data(), (size_t)ne);
    }
  }
}

}  // namespace

// exactly one of vres (vertex scores) and eres (edge scores, one per stored edge in out-edge order)
void run_betweenness(handle_t& h, graph_t& g, array_view_t const* vertex_list, bool normalized, bool endpoints,
                     centrality_result_t* vres, edge_centrality_result_t* eres)
{
  dispatch_ve(g.vertex_type, g.edge_type, [&](auto t) {
    using T = decltype(t);
    bc_impl<typename T::vertex_t, typename T::edge_t>(h, g, vertex_list, normalized, endpoints, vres, eres);
  });
}

}  // namespace cgx
