// Uniform neighbour sampling on the out-edge CSR (reference sampling/uniform_neighbor_sampling_impl.hpp,
// sampling_utils_impl.cuh, prims/per_v_random_select_transform_outgoing_e.cuh).
//
// A hop takes the frontier array (slot i holds a vertex, duplicates are slots of their own) and a fan-out K
// and gives, slot after slot, the picked edges; their destinations are the next hop's frontier.  Which edges
// a slot picks depends on (sample_seed, hop, i, its row) alone -- sample.hpp's draw -- so no launch shape
// changes the result and tests/sampling_ref.py restates it bit for bit:
//   row of d entries, d == 0            nothing
//   K <= 0                              the whole row, in row order
//   with replacement                    pick j is row position index(draw(seed, hop, i, j), d), j < K
//   without replacement, d <= K         the whole row, in row order
//   without replacement, d > K          Robert Floyd's sampler: for t = 0 .. K - 1, m = d - K + t,
//                                       r = index(draw(seed, hop, i, t), m + 1), pick t = r unless an earlier
//                                       pick of the slot is r, then m
//
// Per hop: k_count (picks per slot), an exclusive scan, one host read of the total, then
//   k_pick_flat   a thread per OUTPUT entry, its slot found by binary search in the offsets: the picks with
//                 replacement and the rows taken whole, so a hub row is spread over the grid;
//   k_floyd_wave  a wave per Floyd slot: lane t draws r_t, the K steps are resolved in order with a shuffle
//                 and a ballot each, chunks of 64 with the earlier chunks' picks in LDS;
//   k_floyd_thread  a thread per Floyd slot, testing against the picks it wrote (tuning_t::sample_path).
// Edges travel as positions in the CSR.  At the end one radix sort of all positions and their run lengths
// give the distinct edges and how often each was drawn; positions of parallel edges with the same weight bits
// are first folded onto the first of them (only then a second sort runs), as the reference's
// count_and_remove_duplicates merges equal (source, destination, weight) triples.
#include "capi.hpp"
#include "prims.hpp"
#include "sample.hpp"

#include <algorithm>

namespace cgx {
namespace {

constexpr int kWaveMaxK      = 1024;  // picks of one slot a wave keeps in LDS; a larger fan-out runs a thread per slot
constexpr int kFloydWaveMinK = 64;    // sample_path 0: fan-outs from here on go to a wave per slot; below, a thread
                                      // per slot measured as fast or faster (fan-outs 5 and 25)
constexpr int kWavesPerBlock = kBlock / 64;

// picks of every slot; cnt[nf] = 0 for the scan's total
template <typename V, typename E>
__global__ void k_count(V const* front, int64_t nf, E const* off, int64_t K, bool repl, int64_t* cnt)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= nf; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t c = 0;
    if (i < nf) {
      V v       = front[i];
      int64_t d = (int64_t)(off[v + 1] - off[v]);
      c         = d == 0 ? 0 : (K <= 0 ? d : (repl ? K : (d < K ? d : K)));
    }
    cnt[i] = c;
  }
}

template <typename V, typename E>
__global__ void k_pick_flat(V const* front, int64_t nf, E const* off, V const* idx, int64_t const* out_off,
                            int64_t total, int64_t K, bool repl, uint64_t sk, uint64_t hop, int64_t* pos, V* nxt)
{
  for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = 0, hi = nf;  // the last slot whose offset is <= o (out_off[nf] = total > o)
    while (lo < hi) {
      int64_t mid = (lo + hi) >> 1;
      if (out_off[mid] <= o) lo = mid + 1;
      else hi = mid;
    }
    int64_t i  = lo - 1;
    int64_t j  = o - out_off[i];
    V v        = front[i];
    int64_t rs = (int64_t)off[v];
    int64_t d  = (int64_t)off[v + 1] - rs;
    int64_t p;
    if (K <= 0 || (!repl && d <= K)) p = rs + j;
    else if (repl) p = rs + (int64_t)sample_index(sample_draw(sk, hop, (uint64_t)i, (uint64_t)j), (uint64_t)d);
    else continue;  // a Floyd slot
    pos[o] = p;
    nxt[o] = idx[p];
  }
}

template <typename V, typename E>
__global__ void __launch_bounds__(kBlock)
  k_floyd_wave(V const* front, int64_t nf, E const* off, V const* idx, int64_t const* out_off, int64_t K, uint64_t sk,
               uint64_t hop, int64_t* pos, V* nxt)
{
  __shared__ uint64_t prev[kWavesPerBlock][kWaveMaxK];  // this slot's picks of the chunks before (row positions)
  int const lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t i = blockIdx.x * (int64_t)kWavesPerBlock + w; i < nf; i += (int64_t)gridDim.x * kWavesPerBlock) {
    V v        = front[i];
    int64_t rs = (int64_t)off[v];
    int64_t d  = (int64_t)off[v + 1] - rs;
    if (d <= K) continue;  // taken whole by k_pick_flat
    int64_t o = out_off[i];
    for (int64_t c = 0; c < K; c += 64) {
      int64_t t  = c + lane;
      uint64_t r = 0;
      if (t < K) r = sample_index(sample_draw(sk, hop, (uint64_t)i, (uint64_t)t), (uint64_t)(d - K + t + 1));
      uint64_t pick = 0;
      int const nt  = (int)(K - c < 64 ? K - c : 64);
      for (int k = 0; k < nt; ++k) {
        uint64_t rk = __shfl(r, k, 64);
        bool hit    = lane < k && pick == rk;
        for (int64_t u = lane; u < c; u += 64) hit |= prev[w][u] == rk;
        bool any = __ballot(hit) != 0ull;
        if (lane == k) pick = any ? (uint64_t)(d - K + c + k) : rk;
      }
      if (t < K) {
        pos[o + t]  = rs + (int64_t)pick;
        nxt[o + t]  = idx[rs + (int64_t)pick];
        prev[w][t] = pick;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the next chunk's lanes read every lane's prev
    }
  }
}

template <typename V, typename E>
__global__ void k_floyd_thread(V const* front, int64_t nf, E const* off, V const* idx, int64_t const* out_off,
                               int64_t K, uint64_t sk, uint64_t hop, int64_t* pos, V* nxt)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nf; i += (int64_t)gridDim.x * blockDim.x) {
    V v        = front[i];
    int64_t rs = (int64_t)off[v];
    int64_t d  = (int64_t)off[v + 1] - rs;
    if (d <= K) continue;
    int64_t o = out_off[i];
    for (int64_t t = 0; t < K; ++t) {
      int64_t m = d - K + t;
      int64_t r = (int64_t)sample_index(sample_draw(sk, hop, (uint64_t)i, (uint64_t)t), (uint64_t)(m + 1));
      bool hit  = false;
      for (int64_t u = 0; u < t; ++u) hit |= pos[o + u] == rs + r;
      int64_t p = rs + (hit ? m : r);
      pos[o + t] = p;
      nxt[o + t] = idx[p];
    }
  }
}

// ---------------------------------------------------------------- distinct edges and their counts
__global__ void k_heads(uint64_t const* key, int64_t n, int* flag)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x)
    flag[i] = i < n && (i == 0 || key[i] != key[i - 1]) ? 1 : 0;
}

// first[k] = where run k starts; first[runs] = n
__global__ void k_run_first(int const* flag, int64_t const* rank, int64_t n, int64_t* first)
{
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x)
    if (i == n || flag[i]) first[rank[i]] = i;
}

// run k of the sorted keys -> its key and the sum of its values (val null: its length)
__global__ void k_reduce_runs(uint64_t const* key, int64_t const* val, int64_t const* first, int64_t runs,
                              uint64_t* ukey, int64_t* uval)
{
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < runs; k += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = first[k], b = first[k + 1];
    int64_t sum = b - a;
    if (val) {
      sum = 0;
      for (int64_t i = a; i < b; ++i) sum += val[i];
    }
    ukey[k] = key[a];
    uval[k] = sum;
  }
}

// the row that holds CSR position p: the last r with off[r] <= p (empty rows are stepped over)
template <typename E>
__device__ __forceinline__ int64_t row_of(E const* off, int64_t nv, int64_t p)
{
  int64_t lo = 0, hi = nv;
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if ((int64_t)off[mid] <= p) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

__device__ __forceinline__ bool same_bits(float a, float b) { return __float_as_uint(a) == __float_as_uint(b); }
__device__ __forceinline__ bool same_bits(double a, double b)
{
  return __double_as_longlong(a) == __double_as_longlong(b);
}

// a position becomes the first position of its row with the same destination and the same weight bits
template <typename V, typename E, typename W>
__global__ void k_fold_parallel(uint64_t* key, int64_t n, E const* off, int64_t nv, V const* idx, W const* w,
                                int* changed)
{
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    int64_t p = (int64_t)key[k];
    if (p == 0 || idx[p - 1] != idx[p]) continue;  // the common case: no lookup of the row
    int64_t rs = (int64_t)off[row_of(off, nv, p)];
    int64_t c  = p;
    for (int64_t q = p - 1; q >= rs && idx[q] == idx[p]; --q)
      if (!w || same_bits(w[q], w[p])) c = q;
    if (c != p) {
      key[k] = (uint64_t)c;
      atomicOr(changed, 1);
    }
  }
}

template <typename V, typename E, typename W>
__global__ void k_emit(uint64_t const* key, int64_t const* count, int64_t n, E const* off, int64_t nv, V const* idx,
                       W const* w, V* src, V* dst, W* index, E* counts)
{
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    int64_t p = (int64_t)key[k];
    src[k]    = (V)row_of(off, nv, p);
    dst[k]    = idx[p];
    if (w) index[k] = w[p];  // a copy: the bits may be edge ids in disguise
    else index[k] = W(1);
    counts[k] = (E)count[k];
  }
}

// sorted keys (and values) -> distinct keys with summed values; returns their number (one host read)
int64_t reduce_sorted(uint64_t const* key, int64_t const* val, int64_t n, dbuf<uint64_t>& ukey, dbuf<int64_t>& uval,
                      hipStream_t s)
{
  dbuf<int> flag((size_t)n + 1, s);
  dbuf<int64_t> rank((size_t)n + 1, s);
  unsigned const grid = grid_for((size_t)n + 1, kBlock, 8192);
  hipLaunchKernelGGL(k_heads, dim3(grid), dim3(kBlock), 0, s, key, n, flag.data());
  CGX_LAUNCH_CHECK();
  exclusive_scan<int, int64_t>(flag.data(), rank.data(), (size_t)n + 1, s);
  int64_t const runs = to_host_scalar(rank.data() + n, s);
  dbuf<int64_t> first((size_t)runs + 1, s);
  hipLaunchKernelGGL(k_run_first, dim3(grid), dim3(kBlock), 0, s, (int const*)flag.data(), (int64_t const*)rank.data(),
                     n, first.data());
  CGX_LAUNCH_CHECK();
  ukey.resize((size_t)runs, s);
  uval.resize((size_t)runs, s);
  if (runs) {
    hipLaunchKernelGGL(k_reduce_runs, dim3(grid_for((size_t)runs, kBlock, 8192)), dim3(kBlock), 0, s, key, val,
                       (int64_t const*)first.data(), runs, ukey.data(), uval.data());
    CGX_LAUNCH_CHECK();
  }
  return runs;
}

template <typename V, typename E, typename W>
void sample_impl(handle_t& h, graph_t& g, array_view_t const& start, int32_t const* fan_out, size_t hops, bool repl,
                 sample_result_t& res)
{
  hipStream_t s    = h.stream;
  int64_t const nv = g.num_vertices;
  reset_hot(h);
  adjacency_t& adj = ensure_adjacency(h, g, false);
  E const* off     = adj.offsets.data<E>();
  V const* idx     = adj.indices.data<V>();
  W const* wgt     = g.weighted ? adj.weights.data<W>() : nullptr;
  uint64_t const sk = sample_seed_key(h.tune.sample_seed);

  int64_t nf = (int64_t)start.size;
  dbuf<V> front((size_t)nf, s);
  if (nf) {
    HIP_CHECK(hipMemcpyAsync(front.data(), start.data, (size_t)nf * sizeof(V), hipMemcpyDefault, s));
    renumber_ext_to_int(h, g, front.data(), (size_t)nf, true);  // CUGRAPH_INVALID_INPUT for an id the graph lacks
  }

  unsigned const max_grid = (unsigned)std::max(device_cu_count(), 1) * 32;
  std::vector<dbuf<int64_t>> picked;  // every hop's edge positions
  int64_t all = 0;
  chunk_timer timer{h, s};
  size_t launches = 0;
  for (size_t hop = 0; hop < hops && nf > 0; ++hop) {
    int64_t const K = fan_out[hop];
    dbuf<int64_t> cnt((size_t)nf + 1, s), out_off((size_t)nf + 1, s);
    hipLaunchKernelGGL((k_count<V, E>), dim3(grid_for((size_t)nf + 1, kBlock, 8192)), dim3(kBlock), 0, s,
                       (V const*)front.data(), nf, off, K, repl, cnt.data());
    CGX_LAUNCH_CHECK();
    exclusive_scan<int64_t, int64_t>(cnt.data(), out_off.data(), (size_t)nf + 1, s);
    int64_t const total = to_host_scalar(out_off.data() + nf, s);
    cnt.free();
    dbuf<int64_t> pos((size_t)total, s);
    dbuf<V> nxt((size_t)total, s);
    if (total) {
      timer.begin();
      hipLaunchKernelGGL((k_pick_flat<V, E>), dim3(grid_for((size_t)total, kBlock, max_grid)), dim3(kBlock), 0, s,
                         (V const*)front.data(), nf, off, idx, (int64_t const*)out_off.data(), total, K, repl, sk,
                         (uint64_t)hop, pos.data(), nxt.data());
      CGX_LAUNCH_CHECK();
      ++launches;
      if (!repl && K > 0) {  // rows longer than K: Floyd's sampler
        int const path = h.tune.sample_path;
        bool const wave = K <= kWaveMaxK && (path == 2 || (path == 0 && K >= kFloydWaveMinK));
        if (wave)
          hipLaunchKernelGGL((k_floyd_wave<V, E>), dim3(grid_for((size_t)nf * 64, kBlock, max_grid)), dim3(kBlock), 0,
                             s, (V const*)front.data(), nf, off, idx, (int64_t const*)out_off.data(), K, sk,
                             (uint64_t)hop, pos.data(), nxt.data());
        else
          hipLaunchKernelGGL((k_floyd_thread<V, E>), dim3(grid_for((size_t)nf, kBlock, max_grid)), dim3(kBlock), 0, s,
                             (V const*)front.data(), nf, off, idx, (int64_t const*)out_off.data(), K, sk,
                             (uint64_t)hop, pos.data(), nxt.data());
        CGX_LAUNCH_CHECK();
        ++launches;
      }
      timer.end();
    }
    all += total;
    picked.push_back(std::move(pos));
    front = std::move(nxt);
    nf    = total;
  }
  front.free();

  // all hops' positions in one array, sorted; run lengths are the counts
  dbuf<uint64_t> ukey;
  dbuf<int64_t> ucnt;
  int64_t nu = 0;
  if (all) {
    dbuf<uint64_t> key((size_t)all, s), sorted((size_t)all, s);
    int64_t at = 0;
    for (auto& p : picked) {
      if (p.size())
        HIP_CHECK(hipMemcpyAsync(key.data() + at, p.data(), p.size() * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
      at += (int64_t)p.size();
      p.free();
    }
    int const bits = bits_for((unsigned long long)std::max<int64_t>(g.num_edges, 1));
    radix_sort_keys<uint64_t>(key.data(), sorted.data(), (size_t)all, 0, bits, s);
    key.free();
    nu = reduce_sorted(sorted.data(), nullptr, all, ukey, ucnt, s);
    sorted.free();
    // parallel edges with equal weights count as one edge
    dbuf<int> changed(1, s);
    HIP_CHECK(hipMemsetAsync(changed.data(), 0, sizeof(int), s));
    hipLaunchKernelGGL((k_fold_parallel<V, E, W>), dim3(grid_for((size_t)nu, kBlock, 8192)), dim3(kBlock), 0, s,
                       ukey.data(), nu, off, nv, idx, wgt, changed.data());
    CGX_LAUNCH_CHECK();
    if (to_host_scalar(changed.data(), s) != 0) {
      dbuf<uint64_t> k2((size_t)nu, s), fkey;
      dbuf<int64_t> c2((size_t)nu, s), fcnt;
      radix_sort_pairs<uint64_t, int64_t>(ukey.data(), k2.data(), ucnt.data(), c2.data(), (size_t)nu, 0, bits, s);
      nu   = reduce_sorted(k2.data(), c2.data(), nu, fkey, fcnt, s);
      ukey = std::move(fkey);
      ucnt = std::move(fcnt);
    }
  }
  res.src    = std::make_unique<device_array_t>((size_t)nu, g.vertex_type, s);
  res.dst    = std::make_unique<device_array_t>((size_t)nu, g.vertex_type, s);
  res.index  = std::make_unique<device_array_t>((size_t)nu, g.weight_type, s);
  res.counts = std::make_unique<device_array_t>((size_t)nu, g.edge_type, s);
  if (nu) {
    hipLaunchKernelGGL((k_emit<V, E, W>), dim3(grid_for((size_t)nu, kBlock, 8192)), dim3(kBlock), 0, s,
                       (uint64_t const*)ukey.data(), (int64_t const*)ucnt.data(), nu, off, nv, idx, wgt,
                       res.src->buf.data<V>(), res.dst->buf.data<V>(), res.index->buf.data<W>(),
                       res.counts->buf.data<E>());
    CGX_LAUNCH_CHECK();
    unrenumber_int_to_ext(h, g, res.src->buf.data(), (size_t)nu);
    unrenumber_int_to_ext(h, g, res.dst->buf.data(), (size_t)nu);
  }
  timer.report(launches);
}

}  // namespace

void run_uniform_neighbor_sample(handle_t& h, graph_t& g, array_view_t const& start, int32_t const* fan_out,
                                 size_t hops, bool with_replacement, sample_result_t& res)
{
  dispatch_vew(g.vertex_type, g.edge_type, g.weight_type, [&](auto t) {
    using T = decltype(t);
    sample_impl<typename T::vertex_t, typename T::edge_t, typename T::weight_t>(h, g, start, fan_out, hops,
                                                                               with_replacement, res);
  });
}

}  // namespace cgx
