// Routing layer of the multi-GPU path: everything an algorithm needs to send
// elements (edges, (id, value) pairs, candidate keys) to the rank that owns them.
//
//  * owners_of_global: the destination rank of each global id;
//  * lower_bounds: first position of each target in a sorted array -- the per-rank
//    blocks of an array sorted by owner, by id or by (id << 32 | x) key, and the row
//    offsets of sorted rows; rank_counts / bounds_to_counts turn the P + 1 bounds
//    into the counts `exchange` takes (no per-element counting, on either side);
//  * route_by / permute / route_columns: order positions by destination rank and
//    exchange any number of columns in that order, one gathered copy alive at a time;
//  * edges_to_source_owner: the 2D block's edges at the owner of their source (the 1D
//    partition by rows BFS, SSSP and Louvain start from), row_keys / split_row_keys:
//    the (row << 32 | destination) sort key of such rows.
//
// None of this runs inside a timed iteration: graph setup, per-call level setup,
// per-round candidate routing.  The radix sorts are the cost; every temporary is
// released as soon as its last reader is enqueued (RMAT-26 on one rank: 2.1G edges,
// 4-8 B each per array).
#pragma once

#include "comm.hpp"
#include "mg_graph.hpp"
#include "prims.hpp"

#include <algorithm>
#include <tuple>

namespace cgx {

inline unsigned blocks(int64_t n) { return grid_for(n > 0 ? n : 1, kBlock, 16384); }

// the P + 1 vertex offsets on the device
inline dbuf<int64_t> device_voff(mg_graph_t const& mg, hipStream_t s)
{
  dbuf<int64_t> d(mg.P + 1, s);
  to_device(d.data(), mg.voff.data(), (size_t)mg.P + 1, s);
  return d;
}

// ---------------------------------------------------------------- owners
template <typename V>
__global__ void k_owners_of_global(V const* ids, int64_t n, int64_t const* voff, int P, int self, int* dest)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t const v = (int64_t)ids[i];
    dest[i]         = (self >= 0 && (v < 0 || v >= voff[P])) ? self : mg_owner_of_global(v, voff, P);
  }
}

// dest[i] = owner rank of the global id ids[i].  self >= 0: ids outside [0, V) stay
// on this rank (values that are not vertices pass through an id translation).
template <typename V>
void owners_of_global(V const* ids, int64_t n, int64_t const* voff_d, int P, int* dest, hipStream_t s, int self = -1)
{
  if (!n) return;
  hipLaunchKernelGGL(k_owners_of_global<V>, dim3(blocks(n)), dim3(kBlock), 0, s, ids, n, voff_d, P, self, dest);
  CGX_LAUNCH_CHECK();
}

// ---------------------------------------------------------------- bounds
// keys and targets of lower_bounds, compared as unsigned 64-bit values
template <typename T>
struct key_of {  // the array's elements
  T const* a;
  __device__ unsigned long long operator()(int64_t i) const { return (unsigned long long)a[i]; }
};
struct target_index {  // q itself: a rank in a sorted owner array, a row in sorted row ids
  __device__ unsigned long long operator()(int64_t q) const { return (unsigned long long)q; }
};
struct target_voff {  // rank q's first id (shift 0), or its first (id << 32 | x) key (shift 32)
  int64_t const* voff;
  int shift;
  __device__ unsigned long long operator()(int64_t q) const { return (unsigned long long)voff[q] << shift; }
};

template <typename Key, typename Target>
__global__ void k_lower_bounds(Key key, int64_t n, Target target, int64_t m, int64_t* out)
{
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q <= m; q += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long const t = target(q);
    int64_t lo = 0, hi = n;
    while (lo < hi) {
      int64_t const mid = (lo + hi) >> 1;
      if (key(mid) < t) lo = mid + 1;
      else hi = mid;
    }
    out[q] = lo;
  }
}

// out[q] = first i in [0, n] with key(i) >= target(q), q = 0..m (keys ascending).
// One small block for the P + 1 owner bounds, a grid-stride launch for row offsets.
// (Two binary searches per rank instead of a per-element atomicAdd onto P counters,
// which serialised at the memory side: 14 ms for 2.4M elements on one rank.)
template <typename Key, typename Target>
void lower_bounds(Key key, int64_t n, Target target, int64_t m, int64_t* out, hipStream_t s)
{
  hipLaunchKernelGGL((k_lower_bounds<Key, Target>), dim3(blocks(m + 1)), dim3(kBlock), 0, s, key, n, target, m, out);
  CGX_LAUNCH_CHECK();
}

// P + 1 bounds (device) -> the P block lengths (host)
inline std::vector<size_t> bounds_to_counts(int64_t const* bounds_d, int P, hipStream_t s)
{
  auto hb = to_host(bounds_d, (size_t)P + 1, s);
  std::vector<size_t> c(P);
  for (int q = 0; q < P; ++q) c[q] = (size_t)(hb[q + 1] - hb[q]);
  return c;
}

// per-rank counts of a sorted array: rank q's block starts at the first key >= target(q)
template <typename Key, typename Target>
std::vector<size_t> rank_counts(Key key, int64_t n, Target target, int P, hipStream_t s)
{
  dbuf<int64_t> bnd(P + 1, s);
  lower_bounds(key, n, target, P, bnd.data(), s);
  return bounds_to_counts(bnd.data(), P, s);
}

// ---------------------------------------------------------------- routing
// positions [0, n) ordered by destination rank; per-rank counts on the host
struct routing {
  size_t n = 0;
  dbuf<int64_t> perm;  // sorted position -> original position
  std::vector<size_t> counts;
};

// in_place: the sort runs double-buffered over `dest` and the buffers here (both
// overwritten), so rocPRIM allocates no copies of its own
inline routing route_by(int* dest, size_t n, int P, hipStream_t s, bool in_place = false)
{
  routing rt;
  rt.n = n;
  rt.perm.resize(std::max<size_t>(n, 1), s);
  rt.counts.assign(P, 0);
  if (!n) return rt;
  dbuf<int> d2(n, s);
  dbuf<int64_t> iv(n, s);
  iota<int64_t>(iv.data(), n, 0, s);
  int const* sorted = d2.data();
  if (!in_place) {
    radix_sort_pairs<int, int64_t>(dest, d2.data(), iv.data(), rt.perm.data(), n, 0, bits_for(P), s);
  } else if (!radix_sort_pairs_db<int, int64_t>(dest, d2.data(), iv.data(), rt.perm.data(), n, 0, bits_for(P), s)) {
    sorted = dest;
    std::swap(iv, rt.perm);
  }
  rt.counts = rank_counts(key_of<int>{sorted}, (int64_t)n, target_index{}, P, s);
  return rt;
}

template <typename T>
dbuf<T> permute(T const* in, dbuf<int64_t> const& perm, size_t n, hipStream_t s)
{
  dbuf<T> out(std::max<size_t>(n, 1), s);
  gather<T, int64_t>(out.data(), in, perm.data(), n, s);
  return out;
}

// one column in destination order, exchanged (the gathered copy is released on return)
template <typename T>
dbuf<T> route_column(comm_t& comm, routing const& rt, T const* col, std::vector<size_t>& rcounts, hipStream_t s)
{
  auto t = permute<T>(col, rt.perm, rt.n, s);
  return exchange<T>(comm, t.data(), rt.counts, rcounts, s);
}

// several columns, one after the other in argument order
template <typename... T>
std::tuple<dbuf<T>...> route_columns(comm_t& comm, routing const& rt, std::vector<size_t>& rcounts, hipStream_t s,
                                     T const*... cols)
{
  return std::tuple<dbuf<T>...>{route_column<T>(comm, rt, cols, rcounts, s)...};
}

// ---------------------------------------------------------------- rows by source owner
template <typename V, typename W>
struct owner_edges {
  int64_t n = 0;
  dbuf<V> src, dst;  // global ids; every src is a vertex of this rank
  dbuf<W> w;         // empty unless asked for
};

// The 2D block's edges sent to the owner of their source, in rank order of the
// senders.  Collective.  Live at the peak (the sort): owner, sorted owner, iota and
// permutation arrays, 24 B per edge; the first three go before the first column moves,
// the permutation after the last.
template <typename V, typename W>
owner_edges<V, W> edges_to_source_owner(handle_t& h, graph_t& g, bool want_weights)
{
  hipStream_t s  = h.stream;
  mg_graph_t& mg = *g.mg;
  comm_t& comm   = *h.mg->world;
  int64_t const ne = mg.ne;
  routing rt;
  {
    auto voff_d = device_voff(mg, s);
    dbuf<int> dest(std::max<int64_t>(ne, 1), s);
    owners_of_global<V>(mg.src.data<V>(), ne, voff_d.data(), mg.P, dest.data(), s);
    rt = route_by(dest.data(), (size_t)ne, mg.P, s, /*in_place=*/true);
  }
  owner_edges<V, W> out;
  std::vector<size_t> rc;
  out.src = route_column<V>(comm, rt, mg.src.data<V>(), rc, s);
  out.dst = route_column<V>(comm, rt, mg.dst.data<V>(), rc, s);
  if (want_weights) out.w = route_column<W>(comm, rt, mg.w.data<W>(), rc, s);
  out.n = (int64_t)out.src.n;
  return out;
}

template <typename V>
__global__ void k_row_keys(V const* src, V const* dst, int64_t n, int64_t base, unsigned long long* keys)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    keys[i] = ((unsigned long long)((int64_t)src[i] - base) << 32) | (unsigned long long)(uint32_t)dst[i];
}

// keys[i] = (src[i] - base) << 32 | dst[i]: sorted, the rows of [base, ...) in order,
// destinations ascending inside a row
template <typename V>
void row_keys(V const* src, V const* dst, int64_t n, int64_t base, unsigned long long* keys, hipStream_t s)
{
  if (!n) return;
  hipLaunchKernelGGL(k_row_keys<V>, dim3(blocks(n)), dim3(kBlock), 0, s, src, dst, n, base, keys);
  CGX_LAUNCH_CHECK();
}

static __global__ void k_split_row_keys(unsigned long long const* keys, int64_t n, uint32_t* row, uint32_t* col, int cb)
{
  unsigned long long const mask = cb >= 64 ? ~0ull : (1ull << cb) - 1;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    row[i] = (uint32_t)(keys[i] >> cb);
    col[i] = (uint32_t)(keys[i] & mask);
  }
}

// key = row << cb | col back into its halves (cb = 32: the row_keys form; Louvain's
// compact sweep keys pass the bits of their cluster ids)
inline void split_row_keys(unsigned long long const* keys, int64_t n, uint32_t* row, uint32_t* col, hipStream_t s,
                           int cb = 32)
{
  if (!n) return;
  hipLaunchKernelGGL(k_split_row_keys, dim3(blocks(n)), dim3(kBlock), 0, s, keys, n, row, col, cb);
  CGX_LAUNCH_CHECK();
}

}  // namespace cgx
