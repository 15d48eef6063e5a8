// The entries of the adjacency rows that pass a test, as a (src, dst, weights) edge list in external
// ids: a count pass per row, a scan, a fill pass, the number map.  Header-only; k_core and
// k_truss_subgraph supply the test, subgraph.hip uses the result-array helpers only.
//
// The test is a small device struct passed by value:
//   bool row(int64_t v) const                                 is row v visited at all
//   bool keep(int64_t v, long long b, long long j) const      entry j of row v, whose row starts at b
//   long long wpos(long long j) const                         where entry j's weight is stored
// Kept entries come out in the order of the rows, and in stored order within a row.  Nothing on the
// output is atomic, so the result is the same bytes on every run.
#pragma once

#include "capi.hpp"
#include "prims.hpp"

namespace cgx {

constexpr int kRowExtractBlock   = 256;
constexpr int kRowExtractWaveRow = 64;  // rows with at least this many entries take a wave

// The kept entries of every row: counted into cnt[v] (pos == nullptr) or written in row order from
// pos[v] on.  A thread per light row, a wave per row from kRowExtractWaveRow entries.  The 256 rows of
// a block lie gridDim.x apart: on a degree-sorted adjacency the longest rows are the first ones and so
// go to different blocks.
template <typename V, typename E, typename W, typename P>
__global__ __launch_bounds__(kRowExtractBlock) void k_extract_rows(E const* off, V const* idx, W const* w, int64_t nv,
                                                                  P p, E const* pos, E* cnt, V* src, V* dst, W* wout)
{
  int const tid = threadIdx.x, lane = tid & 63;
  int64_t const apart = (int64_t)gridDim.x;
  for (int64_t base = 0; base < nv; base += apart * kRowExtractBlock) {
    int64_t const v = base + tid * apart + blockIdx.x;
    long long b = 0, e = 0;
    if (v < nv && p.row(v)) {  // a row that is not visited is an empty one
      b = (long long)off[v];
      e = (long long)off[v + 1];
    }
    long long const len = e - b;
    if (v < nv && len < kRowExtractWaveRow) {
      long long c        = 0;
      long long const p0 = pos ? (long long)pos[v] : 0;
      for (long long j = b; j < e; ++j) {
        if (!p.keep(v, b, j)) continue;
        if (pos) {
          src[p0 + c] = (V)v;
          dst[p0 + c] = idx[j];
          if (wout) wout[p0 + c] = w[p.wpos(j)];
        }
        ++c;
      }
      if (!pos) cnt[v] = (E)c;
    }
    unsigned long long m = __ballot(len >= kRowExtractWaveRow);
    while (m) {  // wave-uniform
      int const l = __ffsll((long long)m) - 1;
      m &= m - 1;
      long long const bb = __shfl(b, l, 64), ee = __shfl(e, l, 64);
      int64_t const vv   = base + (tid - lane + l) * apart + blockIdx.x;
      long long c        = pos ? (long long)pos[vv] : 0;  // wave-uniform
      long long const c0 = c;
      for (long long j0 = bb; j0 < ee; j0 += 64) {
        long long const j = j0 + lane;
        bool const keep   = j < ee && p.keep(vv, bb, j);
        unsigned long long const km = __ballot(keep);
        if (pos && keep) {
          long long const q = c + __popcll(km & ((1ull << lane) - 1ull));
          src[q]            = (V)vv;
          dst[q]            = idx[j];
          if (wout) wout[q] = w[p.wpos(j)];
        }
        c += __popcll(km);
      }
      if (!pos && lane == 0) cnt[vv] = (E)(c - c0);
    }
  }
}

// src, dst and (on a weighted graph) weights of n edges in the graph's types; n == 0 is the empty result
inline void alloc_edge_arrays(graph_t& g, size_t n, hipStream_t s, std::unique_ptr<device_array_t>& src,
                              std::unique_ptr<device_array_t>& dst, std::unique_ptr<device_array_t>& weights)
{
  src = std::make_unique<device_array_t>(n, g.vertex_type, s);
  dst = std::make_unique<device_array_t>(n, g.vertex_type, s);
  if (g.weighted) weights = std::make_unique<device_array_t>(n, g.weight_type, s);
}

// internal ids -> the caller's, both ends of n edges
inline void unrenumber_edge_arrays(handle_t& h, graph_t& g, device_array_t& src, device_array_t& dst, size_t n)
{
  unrenumber_int_to_ext(h, g, src.buf.data(), n);
  unrenumber_int_to_ext(h, g, dst.buf.data(), n);
}

// The entries of the rows (off, idx, weights w or nullptr) that pass `p`, into src / dst / weights;
// returns their number.  One host read: the result's size.
template <typename V, typename E, typename W, typename P>
size_t extract_rows(handle_t& h, graph_t& g, E const* off, V const* idx, W const* w, P p,
                    std::unique_ptr<device_array_t>& src, std::unique_ptr<device_array_t>& dst,
                    std::unique_ptr<device_array_t>& weights)
{
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  dbuf<E> cnt((size_t)nv + 1, s), pos((size_t)nv + 1, s);
  HIP_CHECK(hipMemsetAsync(cnt.data() + nv, 0, sizeof(E), s));
  unsigned const grid = grid_for((size_t)nv, kRowExtractBlock, 1u << 16);
  hipLaunchKernelGGL((k_extract_rows<V, E, W, P>), dim3(grid), dim3(kRowExtractBlock), 0, s, off, idx, w, nv, p,
                     (E const*)nullptr, cnt.data(), (V*)nullptr, (V*)nullptr, (W*)nullptr);
  CGX_LAUNCH_CHECK();
  exclusive_scan<E, E>(cnt.data(), pos.data(), (size_t)nv + 1, s);
  size_t const total = (size_t)to_host_scalar(pos.data() + nv, s);
  alloc_edge_arrays(g, total, s, src, dst, weights);
  if (total == 0) return 0;
  hipLaunchKernelGGL((k_extract_rows<V, E, W, P>), dim3(grid), dim3(kRowExtractBlock), 0, s, off, idx, w, nv, p,
                     (E const*)pos.data(), (E*)nullptr, src->buf.data<V>(), dst->buf.data<V>(),
                     g.weighted ? weights->buf.data<W>() : (W*)nullptr);
  CGX_LAUNCH_CHECK();
  unrenumber_edge_arrays(h, g, *src, *dst, total);
  return total;
}

}  // namespace cgx
