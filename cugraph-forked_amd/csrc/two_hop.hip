// Two-hop neighbours: every ordered pair (u, v), u != v, with a walk u -> w -> v over the out-edges.
//
// Reference: c_api/graph_functions.cpp (cugraph_two_hop_neighbors; the snapshot's body is
// unimplemented) and traversal/two_hop_neighbors.cu (expand every row's walks, sort, unique, drop
// u == v; pairs that are also adjacent stay).  Restated in include/cugraph_c/graph_functions.h.
//
// The source rows are taken in ascending internal id.  Pairs with different first vertices never
// collide, so consecutive source rows form batches whose walks stay under two_hop_budget:
//   * a batch: a wave per source row writes the packed key first * V + second of every walk (64 row
//     entries at a time, the lanes share the walks of those entries evenly), the keys are
//     radix-sorted, and the first key of every run with first != second is kept;
//   * a row whose walks alone exceed the budget: its walks set bits of a V-bit map instead (a wave
//     per row entry over the whole grid), and the map's set bits, without the row's own, are its pairs.
// Every batch leaves an exact-size block of sorted keys; at the end the blocks are unpacked into the
// two result arrays and mapped to external ids.  Temporary memory is the budget (two key buffers and
// the flags) plus O(V) plus the result, never the sum of deg(dst) over all edges.  The output is in
// (first, second) order of the internal ids: the same from call to call and for every budget.
#include "capi.hpp"
#include "prims.hpp"

#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <vector>

namespace cgx {

namespace {

constexpr int kThBlock     = 256;
constexpr int kThGridPerCu = 8;

using pkey_t = unsigned long long;

template <typename V>
__global__ __launch_bounds__(kThBlock) void k_th_mark(V const* ids, size_t n, uint8_t* flags)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    flags[ids[i]] = 1;  // ids were range-checked by the renumbering
}

// a wave per source: walks[i] = sum of deg(w) over the entries w of the source's row
template <typename V, typename E>
__global__ __launch_bounds__(kThBlock) void k_th_walks(E const* off, V const* idx, V const* srcs, int64_t ns,
                                                       long long* walks)
{
  int const lane          = threadIdx.x & 63;
  int64_t const wave      = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  int64_t const num_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t i = wave; i < ns; i += num_waves) {
    int64_t const u   = srcs ? (int64_t)srcs[i] : i;
    long long const b = (long long)off[u], e = (long long)off[u + 1];
    long long c       = 0;
    for (long long j = b + lane; j < e; j += 64) {
      V const w = idx[j];
      c += (long long)off[w + 1] - (long long)off[w];
    }
    c = wave_sum_ll(c);
    if (lane == 0) walks[i] = c;
  }
}

// a wave per source i0 <= i < i1: the keys of its walks go to keys[wofs[i] - wofs[i0] ..)
template <typename V, typename E>
__global__ __launch_bounds__(kThBlock) void k_th_expand(E const* off, V const* idx, V const* srcs, int64_t i0,
                                                        int64_t i1, long long const* wofs, int64_t nv, pkey_t* keys)
{
  int const lane          = threadIdx.x & 63;
  int64_t const wave      = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  int64_t const num_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  long long const base    = wofs[i0];
  for (int64_t i = i0 + wave; i < i1; i += num_waves) {  // wave-uniform
    int64_t const u   = srcs ? (int64_t)srcs[i] : i;
    long long const b = (long long)off[u], e = (long long)off[u + 1];
    pkey_t* const out  = keys + (wofs[i] - base);
    pkey_t const hi    = (pkey_t)u * (pkey_t)nv;
    long long run     = 0;
    for (long long j0 = b; j0 < e; j0 += 64) {
      long long const j = j0 + lane;
      long long wb = 0, dw = 0;
      if (j < e) {
        V const w = idx[j];
        wb        = (long long)off[w];
        dw        = (long long)off[w + 1] - wb;
      }
      long long incl = dw;  // walks of lanes 0 .. lane
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        long long const t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
      }
      long long const excl  = incl - dw;
      long long const total = __shfl(incl, 63, 64);
      for (long long t0 = 0; t0 < total; t0 += 64) {  // every lane runs every round: the shuffles need them all
        long long const t = t0 + lane;
        long long const q = t < total ? t : total - 1;
        int lo = 0, hi_l = 63;  // the lane whose walks hold q: the first with incl > q
#pragma unroll
        for (int it = 0; it < 6; ++it) {
          int const mid     = (lo + hi_l) >> 1;
          long long const v = __shfl(incl, mid, 64);
          if (v <= q) lo = mid + 1;
          else hi_l = mid;
        }
        long long const er = __shfl(excl, lo, 64);
        long long const br = __shfl(wb, lo, 64);
        if (t < total) out[run + t] = hi + (pkey_t)idx[br + (q - er)];
      }
      run += total;
    }
  }
}

// the first key of every run, unless its two vertices are the same
__global__ __launch_bounds__(kThBlock) void k_th_heads(pkey_t const* keys, size_t n, pkey_t nv, uint8_t* flags)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    pkey_t const k = keys[i];
    flags[i]      = ((i == 0 || keys[i - 1] != k) && (k / nv != k % nv)) ? 1 : 0;
  }
}

// the row above the budget: a wave per entry of row u sets the bits of that entry's row
template <typename V, typename E>
__global__ __launch_bounds__(kThBlock) void k_th_set_bits(E const* off, V const* idx, int64_t u, unsigned* bits)
{
  int const lane          = threadIdx.x & 63;
  int64_t const wave      = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  int64_t const num_waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  long long const b = (long long)off[u], e = (long long)off[u + 1];
  for (long long j = b + wave; j < e; j += num_waves) {
    V const w          = idx[j];
    long long const wb = (long long)off[w], we = (long long)off[w + 1];
    for (long long t = wb + lane; t < we; t += 64) {
      unsigned long long const x = (unsigned long long)idx[t];
      atomicOr(bits + (x >> 5), 1u << (x & 31));
    }
  }
}

// set bits per word, the bit of u itself left out (words + 1 entries, the last one 0)
__global__ __launch_bounds__(kThBlock) void k_th_bit_counts(unsigned const* bits, size_t words, int64_t u,
                                                            long long* counts)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i <= words; i += (size_t)gridDim.x * blockDim.x) {
    unsigned w = i < words ? bits[i] : 0u;
    if (i == (size_t)(u >> 5)) w &= ~(1u << (u & 31));
    counts[i] = __popc(w);
  }
}

__global__ __launch_bounds__(kThBlock) void k_th_bit_keys(unsigned const* bits, size_t words, int64_t u, pkey_t nv,
                                                          long long const* wofs, pkey_t* keys)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
    unsigned w = bits[i];
    if (i == (size_t)(u >> 5)) w &= ~(1u << (u & 31));
    long long o = wofs[i];
    while (w) {
      int const bit = __ffs((int)w) - 1;
      w &= w - 1;
      keys[o++] = (pkey_t)u * nv + ((pkey_t)i << 5) + (pkey_t)bit;
    }
  }
}

template <typename V>
__global__ __launch_bounds__(kThBlock) void k_th_unpack(pkey_t const* keys, size_t n, pkey_t nv, V* first, V* second)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    pkey_t const k = keys[i];
    first[i]      = (V)(k / nv);
    second[i]     = (V)(k % nv);
  }
}

template <typename In, typename Out>
size_t select_flagged(In in, uint8_t const* flags, Out* out, size_t n, hipStream_t s)
{
  dbuf<size_t> cnt(1, s);
  size_t tmp = 0;
  HIP_CHECK(rocprim::select(nullptr, tmp, in, flags, out, cnt.data(), n, s));
  buffer t(tmp, s);
  HIP_CHECK(rocprim::select(t.data(), tmp, in, flags, out, cnt.data(), n, s));
  return to_host_scalar(cnt.data(), s);
}

template <typename V, typename E>
void two_hop_impl(handle_t& h, graph_t& g, array_view_t const* start, vertex_pairs_t& res)
{
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  auto empty       = [&] {
    res.first  = std::make_unique<device_array_t>(0, g.vertex_type, s);
    res.second = std::make_unique<device_array_t>(0, g.vertex_type, s);
  };
  CGX_EXPECTS(nv < ((int64_t)1 << 32), CUGRAPH_UNSUPPORTED_TYPE_COMBINATION,
              "two_hop_neighbors: the packed (first, second) keys need fewer than 2^32 vertices");
  // the sources: every vertex, or the start list's distinct internal ids in ascending order
  dbuf<V> srcs;
  int64_t ns = nv;
  if (start) {
    size_t const n = start->size;
    if (n == 0 || nv == 0) {
      CGX_INPUT(n == 0, "Invalid input argument: vertex id not in the graph.");
      return empty();
    }
    dbuf<V> ids(n, s);
    HIP_CHECK(hipMemcpyAsync(ids.data(), start->data, n * sizeof(V), hipMemcpyDefault, s));
    renumber_ext_to_int(h, g, ids.data(), n, true);  // an unknown id: CUGRAPH_INVALID_INPUT
    dbuf<uint8_t> flags((size_t)nv, s);
    HIP_CHECK(hipMemsetAsync(flags.data(), 0, (size_t)nv, s));
    hipLaunchKernelGGL(k_th_mark<V>, dim3(grid_for(n, kThBlock, 4096)), dim3(kThBlock), 0, s, (V const*)ids.data(), n,
                       flags.data());
    CGX_LAUNCH_CHECK();
    srcs.resize((size_t)nv, s);
    ns = (int64_t)select_flagged(rocprim::counting_iterator<V>(0), flags.data(), srcs.data(), (size_t)nv, s);
  }
  if (nv == 0 || g.num_edges == 0 || ns == 0) return empty();
  adjacency_t& adj = ensure_adjacency(h, g, false);  // out-edges
  E const* off     = adj.offsets.data<E>();
  V const* idx     = adj.indices.data<V>();
  V const* sp      = start ? (V const*)srcs.data() : (V const*)nullptr;
  unsigned const grid = (unsigned)std::max(device_cu_count(), 1) * kThGridPerCu;

  dbuf<long long> walks((size_t)ns + 1, s), wofs((size_t)ns + 1, s);
  HIP_CHECK(hipMemsetAsync(walks.data() + ns, 0, sizeof(long long), s));
  hipLaunchKernelGGL((k_th_walks<V, E>), dim3(grid_for((size_t)ns * 64, kThBlock, grid)), dim3(kThBlock), 0, s, off,
                     idx, sp, ns, walks.data());
  CGX_LAUNCH_CHECK();
  exclusive_scan<long long, long long>(walks.data(), wofs.data(), (size_t)ns + 1, s);
  std::vector<long long> const hw = to_host(walks.data(), (size_t)ns, s);
  std::vector<V> hsrc;
  if (start) hsrc = to_host((V const*)srcs.data(), (size_t)ns, s);

  long long const budget = std::max<long long>(h.tune.two_hop_budget, 1);
  long long cap          = 0;  // the largest batch
  for (int64_t i = 0; i < ns;) {
    if (hw[i] > budget) { ++i; continue; }
    long long sum = 0;
    for (; i < ns && hw[i] <= budget && sum + hw[i] <= budget; ++i) sum += hw[i];
    cap = std::max(cap, sum);
  }
  dbuf<pkey_t> k0, k1;
  dbuf<uint8_t> flags;
  if (cap > 0) {
    k0.resize((size_t)cap, s);
    k1.resize((size_t)cap, s);
    flags.resize((size_t)cap, s);
  }
  int const key_bits = bits_for((unsigned long long)nv * (unsigned long long)nv - 1);
  std::vector<dbuf<pkey_t>> blocks;  // sorted distinct keys, in source order
  size_t total = 0;
  auto keep = [&](pkey_t const* keys, size_t n) {
    if (!n) return;
    dbuf<pkey_t> blk(n, s);
    HIP_CHECK(hipMemcpyAsync(blk.data(), keys, n * sizeof(pkey_t), hipMemcpyDeviceToDevice, s));
    blocks.push_back(std::move(blk));
    total += n;
  };
  size_t const words = ((size_t)nv + 31) / 32;
  dbuf<unsigned> bits;
  dbuf<long long> bcnt, bofs;
  for (int64_t i = 0; i < ns;) {
    if (hw[i] > budget) {  // a row above the budget, through the V-bit map
      int64_t const u = start ? (int64_t)hsrc[i] : i;
      if (bits.size() == 0) {
        bits.resize(words, s);
        bcnt.resize(words + 1, s);
        bofs.resize(words + 1, s);
      }
      HIP_CHECK(hipMemsetAsync(bits.data(), 0, words * sizeof(unsigned), s));
      hipLaunchKernelGGL((k_th_set_bits<V, E>), dim3(grid), dim3(kThBlock), 0, s, off, idx, u, bits.data());
      hipLaunchKernelGGL(k_th_bit_counts, dim3(grid_for(words + 1, kThBlock, grid)), dim3(kThBlock), 0, s,
                         (unsigned const*)bits.data(), words, u, bcnt.data());
      CGX_LAUNCH_CHECK();
      exclusive_scan<long long, long long>(bcnt.data(), bofs.data(), words + 1, s);
      size_t const n = (size_t)to_host_scalar(bofs.data() + words, s);
      if (n) {
        dbuf<pkey_t> blk(n, s);
        hipLaunchKernelGGL(k_th_bit_keys, dim3(grid_for(words, kThBlock, grid)), dim3(kThBlock), 0, s,
                           (unsigned const*)bits.data(), words, u, (pkey_t)nv, (long long const*)bofs.data(),
                           blk.data());
        CGX_LAUNCH_CHECK();
        blocks.push_back(std::move(blk));
        total += n;
      }
      ++i;
      continue;
    }
    int64_t const i0 = i;
    long long sum    = 0;
    for (; i < ns && hw[i] <= budget && sum + hw[i] <= budget; ++i) sum += hw[i];
    if (sum == 0) continue;
    hipLaunchKernelGGL((k_th_expand<V, E>), dim3(grid_for((size_t)(i - i0) * 64, kThBlock, grid)), dim3(kThBlock), 0,
                       s, off, idx, sp, i0, i, (long long const*)wofs.data(), nv, k0.data());
    CGX_LAUNCH_CHECK();
    radix_sort_keys<pkey_t>(k0.data(), k1.data(), (size_t)sum, 0, key_bits, s);
    hipLaunchKernelGGL(k_th_heads, dim3(grid_for((size_t)sum, kThBlock, 1u << 16)), dim3(kThBlock), 0, s,
                       (pkey_t const*)k1.data(), (size_t)sum, (pkey_t)nv, flags.data());
    CGX_LAUNCH_CHECK();
    size_t const n = select_flagged((pkey_t const*)k1.data(), flags.data(), k0.data(), (size_t)sum, s);
    keep(k0.data(), n);
  }
  k0.free();
  k1.free();
  flags.free();
  res.first  = std::make_unique<device_array_t>(total, g.vertex_type, s);
  res.second = std::make_unique<device_array_t>(total, g.vertex_type, s);
  size_t at  = 0;
  for (auto& blk : blocks) {
    hipLaunchKernelGGL(k_th_unpack<V>, dim3(grid_for(blk.size(), kThBlock, 1u << 16)), dim3(kThBlock), 0, s,
                       (pkey_t const*)blk.data(), blk.size(), (pkey_t)nv, res.first->buf.data<V>() + at,
                       res.second->buf.data<V>() + at);
    CGX_LAUNCH_CHECK();
    at += blk.size();
    blk.free();
  }
  unrenumber_int_to_ext(h, g, res.first->buf.data(), total);
  unrenumber_int_to_ext(h, g, res.second->buf.data(), total);
}

}  // namespace

void run_two_hop(handle_t& h, graph_t& g, array_view_t const* start, vertex_pairs_t& res)
{
  dispatch_ve(g.vertex_type, g.edge_type, [&](auto t) {
    using T = decltype(t);
    two_hop_impl<typename T::vertex_t, typename T::edge_t>(h, g, start, res);
  });
}

}  // namespace cgx
