// Uniform and biased random walks on the out-edge CSR (reference sampling/random_walks_impl.cuh:90-190;
// its biased selector is CUGRAPH_FAIL("biased sampling not implemented"), so the biased step follows the
// comment at random_walks_impl.cuh:126-131: an edge is taken with probability weight / row total).
//
// Walk i starts at start[i]; step s from vertex v with a row of d entries takes, with sample.hpp's draw,
//   uniform  row position index(draw(seed, s, i, 0), d)
//   biased   the first position p with cum[p] > unit(draw(seed, s, i, 0)) * cum[d - 1], where cum is the
//            row's inclusive prefix sum of weights in double, added left to right (tests/sampling_ref.py:
//            numpy's cumsum); a row whose total is 0 is a sink
// and a vertex without out-edges ends the walk: the rest of its row is -1 and its weights 0.
//
// One launch runs every step, a thread per walk: a step is a dependent chain of two gathers (the row's
// offsets, then the picked entry), so the parallelism is the number of walks.  The biased step finds p by
// binary search in cum, O(log d) also on hub rows.  cum is built once per adjacency (8 B per edge, cached
// beside sim_deg): a wave takes 64 consecutive rows, a lane sums a row below 64 entries by itself and the
// wave sums a longer one together, 64 coalesced loads at a time added in order through shuffles.
#include "capi.hpp"
#include "prims.hpp"
#include "sample.hpp"

#include <algorithm>

namespace cgx {
namespace {

template <typename E, typename W>
__global__ void __launch_bounds__(kBlock) k_row_cum(E const* off, W const* w, int64_t nv, double* cum, int* bad)
{
  int const lane       = threadIdx.x & 63;
  int64_t const wave   = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) >> 6;
  int64_t const nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t base = wave * 64; base < nv; base += nwaves * 64) {
    int64_t r  = base + lane;
    int64_t rs = 0, d = 0;
    if (r < nv) {
      rs = (int64_t)off[r];
      d  = (int64_t)off[r + 1] - rs;
    }
    bool neg = false;
    if (d < 64) {
      double acc = 0;
      for (int64_t j = 0; j < d; ++j) {
        double x = (double)w[rs + j];
        neg |= !(x >= 0);
        acc += x;
        cum[rs + j] = acc;
      }
    }
    unsigned long long big = __ballot(d >= 64);
    while (big) {
      int k = __ffsll((long long)big) - 1;
      big &= big - 1;
      int64_t brs = __shfl(rs, k, 64), bd = __shfl(d, k, 64);
      double carry = 0;
      for (int64_t c = 0; c < bd; c += 64) {
        bool in  = c + lane < bd;
        double x = in ? (double)w[brs + c + lane] : 0.0;
        neg |= !(x >= 0);
        int const nt = (int)(bd - c < 64 ? bd - c : 64);
        double mine  = 0;
        for (int t = 0; t < nt; ++t) {
          carry += __shfl(x, t, 64);
          if (lane == t) mine = carry;
        }
        if (in) cum[brs + c + lane] = mine;
      }
    }
    if (neg) atomicOr(bad, 1);
  }
}

// cum: null for uniform walks
template <typename V, typename E, typename W>
__global__ void k_walk(V const* start, int64_t n, int64_t len, E const* off, V const* idx, W const* w,
                       double const* cum, uint64_t sk, V* paths, W* wout)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    V v    = start[i];
    V* row = paths + i * (len + 1);
    W* wr  = wout ? wout + i * len : nullptr;
    row[0] = v;
    int64_t s = 0;
    for (; s < len; ++s) {
      int64_t rs = (int64_t)off[v];
      int64_t d  = (int64_t)off[v + 1] - rs;
      if (d == 0) break;
      uint64_t r = sample_draw(sk, (uint64_t)s, (uint64_t)i, 0);
      int64_t p;
      if (!cum) {
        p = rs + (int64_t)sample_index(r, (uint64_t)d);
      } else {
        double total = cum[rs + d - 1];
        if (!(total > 0)) break;
        double x   = sample_unit(r) * total;
        int64_t lo = 0, hi = d - 1;  // x < total = cum[d - 1]
        while (lo < hi) {
          int64_t mid = (lo + hi) >> 1;
          if (cum[rs + mid] > x) hi = mid;
          else lo = mid + 1;
        }
        p = rs + lo;
      }
      v          = idx[p];
      row[s + 1] = v;
      if (wr) wr[s] = w[p];
    }
    for (; s < len; ++s) {
      row[s + 1] = (V)-1;
      if (wr) wr[s] = W(0);
    }
  }
}

template <typename V, typename E, typename W>
void ensure_cum(handle_t& h, graph_t& g, adjacency_t& adj)
{
  if (adj.cum_valid) return;
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  buffer cum((size_t)std::max<int64_t>(g.num_edges, 1) * sizeof(double), s);
  dbuf<int> bad(1, s);
  HIP_CHECK(hipMemsetAsync(bad.data(), 0, sizeof(int), s));
  if (nv > 0 && g.num_edges > 0) {
    hipLaunchKernelGGL((k_row_cum<E, W>), dim3(grid_for((size_t)nv, kBlock, 1u << 16)), dim3(kBlock), 0, s,
                       adj.offsets.data<E>(), adj.weights.data<W>(), nv, cum.data<double>(), bad.data());
    CGX_LAUNCH_CHECK();
  }
  CGX_INPUT(to_host_scalar(bad.data(), s) == 0,
            "Invalid input argument: biased random walks need non-negative edge weights");
  adj.cum       = std::move(cum);
  adj.cum_valid = true;
}

template <typename V, typename E, typename W>
void walks_impl(handle_t& h, graph_t& g, array_view_t const& start, size_t max_length, bool biased,
                random_walk_result_t& res)
{
  hipStream_t s = h.stream;
  reset_hot(h);
  adjacency_t& adj = ensure_adjacency(h, g, false);
  if (biased) ensure_cum<V, E, W>(h, g, adj);
  size_t const n = start.size;
  int64_t const len = (int64_t)max_length;
  res.max_length = max_length;
  res.paths      = std::make_unique<device_array_t>(n * (max_length + 1), g.vertex_type, s);
  if (g.weighted) res.weights = std::make_unique<device_array_t>(n * max_length, g.weight_type, s);
  if (n == 0) return;
  dbuf<V> first(n, s);
  HIP_CHECK(hipMemcpyAsync(first.data(), start.data, n * sizeof(V), hipMemcpyDefault, s));
  renumber_ext_to_int(h, g, first.data(), n, true);  // CUGRAPH_INVALID_INPUT for an id the graph lacks
  chunk_timer timer{h, s};
  timer.begin();
  hipLaunchKernelGGL((k_walk<V, E, W>), dim3(grid_for(n, kBlock, 1u << 16)), dim3(kBlock), 0, s,
                     (V const*)first.data(), (int64_t)n, len, adj.offsets.data<E>(), adj.indices.data<V>(),
                     g.weighted ? adj.weights.data<W>() : (W const*)nullptr,
                     biased ? adj.cum.data<double>() : (double const*)nullptr, sample_seed_key(h.tune.sample_seed),
                     res.paths->buf.data<V>(), g.weighted ? res.weights->buf.data<W>() : (W*)nullptr);
  CGX_LAUNCH_CHECK();
  timer.end();
  unrenumber_int_to_ext(h, g, res.paths->buf.data(), n * (max_length + 1));  // -1 stays -1
  timer.report(1);
}

}  // namespace

void run_random_walks(handle_t& h, graph_t& g, array_view_t const& start, size_t max_length, bool biased,
                      random_walk_result_t& res)
{
  dispatch_vew(g.vertex_type, g.edge_type, g.weight_type, [&](auto t) {
    using T = decltype(t);
    walks_impl<typename T::vertex_t, typename T::edge_t, typename T::weight_t>(h, g, start, max_length, biased, res);
  });
}

}  // namespace cgx
