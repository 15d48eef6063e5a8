// Induced subgraphs and ego nets: cugraph_extract_induced_subgraph and cugraph_extract_ego.
//
// Reference: structure/induced_subgraph_impl.cuh (a thread per (subgraph, vertex) that binary-searches
// every row entry in the member list) and community/legacy/egonet.cu (a whole BFS over V-length arrays
// per seed, then the same extraction).  Restated in include/cugraph_c/graph_functions.h and
// community_algorithms.h.
//
// Both entries end in one extraction over one representation: the sorted 64-bit keys slot * V + vertex
// of every (subgraph, member) pair (subgraph_keys.hpp) and the subgraphs' offsets into them.  A work
// item is a key: the out-row of its vertex against the member list of its slot, two ascending
// sequences.  Extraction is count -> scan -> fill, the fill repeating the count's decisions:
//   * a thread for a short row, by merge or by binary search in the list (sg_row_hits);
//   * a wave from kIsectWaveLen row entries: 64 entries at a time, every lane one binary search, the
//     list staged in the wave's LDS slice as vertex ids when it fits and pays; a hit's output position
//     is the hits before it, from a ballot and a popcount;
//   * rows of sg_split_min entries or more are cut into segments of kSgSegLen entries, a wave each; the
//     segments' counts are scanned, so a segment knows its base.
// No atomic touches the output: positions come from scans alone, so the edges of a subgraph ascend by
// (internal source, stored row position) whatever the path.
//
// Ego sets grow for all sources together.  A hop expands the frontier keys' rows into candidate keys
// slot * V + neighbour, radix-sorts them, keeps the first of every run that is not a member yet, and
// merges what is left (the next frontier) into the members.  Whole slots are expanded in batches of at
// most ego_budget candidates; a slot whose hop alone exceeds the budget sets the bits of a V-bit map
// instead (atomicOr: the order of the bits' arrival changes nothing), clears its members' bits, and
// reads the next frontier off the map.  Both give the same ascending keys.
#include "capi.hpp"
#include "intersect.hpp"
#include "prims.hpp"
#include "row_extract.hpp"
#include "subgraph_keys.hpp"

#include <rocprim/device/device_merge.hpp>

#include <algorithm>
#include <vector>

namespace cgx {

namespace {

constexpr int kSgGridPerCu = 8;

enum : int { kSgNone = 0, kSgThread = 1, kSgWave = 2, kSgSplit = 3 };

// path: tuning_t::sg_path
__device__ __forceinline__ int sg_tier(long long len, long long nl, int path, long long split_min)
{
  if (len == 0 || nl == 0) return kSgNone;
  if (path == 1) return kSgThread;
  if (path == 2) return kSgWave;
  if (len >= split_min) return kSgSplit;
  return len >= kIsectWaveLen ? kSgWave : kSgThread;
}

template <typename V, typename E>
struct sg_in {
  E const* off;
  V const* idx;
  sg_key_t const* keys;   // [m] sorted member keys
  long long const* soff;  // [slots + 1] the slots' ranges in keys
  long long m;
  sg_key_t nv;
  int path;
  long long split_min;
  int stage_div;
};

template <typename V>
struct sg_out {
  V* src;
  V* dst;
  void const* gw;  // the adjacency's weights, or null
  void* w;
  int wbytes;  // 4 or 8
};

// the stored edge at position p of the adjacency, source u, to output position o
template <typename V>
__device__ __forceinline__ void sg_put(sg_out<V> const& out, V const* idx, long long o, V u, long long p)
{
  out.src[o] = u;
  out.dst[o] = idx[p];
  if (out.gw) {
    if (out.wbytes == 4) static_cast<uint32_t*>(out.w)[o] = static_cast<uint32_t const*>(out.gw)[p];
    else static_cast<uint64_t*>(out.w)[o] = static_cast<uint64_t const*>(out.gw)[p];
  }
}

struct sg_item {
  long long u   = 0;  // the member vertex
  long long b   = 0;  // its row
  long long len = 0;
  long long lb  = 0;  // its slot's member list
  long long nl  = 0;
  long long base = 0;  // slot * V (as bits of a sg_key_t)
};

template <typename V, typename E>
__device__ __forceinline__ sg_item sg_decode(sg_in<V, E> const& a, long long w)
{
  sg_item it;
  sg_key_t const key  = a.keys[w];
  sg_key_t const slot = key / a.nv;
  it.base = (long long)(slot * a.nv);
  it.u    = (long long)(key - slot * a.nv);
  it.b    = (long long)a.off[it.u];
  it.len  = (long long)a.off[it.u + 1] - it.b;
  it.lb   = a.soff[slot];
  it.nl   = a.soff[slot + 1] - it.lb;
  return it;
}

// A wave: positions [s0, s1) of the row, 64 at a time, each lane one binary search in list[0, nl)
// (staged in `stage` as vertex ids when it fits and pays).  emit(j, r) for the hit at row position j,
// r = the hits of [s0, j) -- ascending j, every copy of a repeated entry.  Returns the hits in every lane.
template <typename V, typename F>
__device__ __forceinline__ long long sg_wave_hits(V const* row, long long s0, long long s1, sg_key_t const* list,
                                                  long long nl, sg_key_t base, V* stage, int stage_div, int lane,
                                                  F const& emit)
{
  bool const staged = stage_div > 0 && nl <= kIsectStageLen<V> && (s1 - s0) * stage_div >= nl;
  if (staged) {
    // DS operations of one wave complete in order; the barriers only pin the compiler
    __builtin_amdgcn_wave_barrier();
    for (long long j = lane; j < nl; j += 64) stage[j] = (V)(list[j] - base);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  long long run = 0;
  for (long long j0 = s0; j0 < s1; j0 += 64) {  // wave-uniform
    long long const j = j0 + lane;
    bool hit          = false;
    if (j < s1) {
      V const x    = row[j];
      long long lo = 0, hi = nl;
      if (staged) {
        while (lo < hi) {
          long long const mid = (lo + hi) >> 1;
          if (stage[mid] < x) lo = mid + 1;
          else hi = mid;
        }
        hit = lo < nl && stage[lo] == x;
      } else {
        sg_key_t const k = base + (sg_key_t)x;
        while (lo < hi) {
          long long const mid = (lo + hi) >> 1;
          if (list[mid] < k) lo = mid + 1;
          else hi = mid;
        }
        hit = lo < nl && list[lo] == k;
      }
    }
    unsigned long long const mask = __ballot(hit);
    if (hit) emit(j, run + (long long)__popcll(mask & ((1ull << lane) - 1ull)));
    run += (long long)__popcll(mask);
  }
  if (staged) __builtin_amdgcn_wave_barrier();
  return run;
}

// One item per thread and 256-item chunk; the items left to the wave go one after the other.  Count
// (Fill false): cnt[w] = the item's hits, 0 for a split item, whose segments go to nseg[w].  Fill: the
// hits of the thread and wave items go to ooff[w] on.
template <bool Fill, typename V, typename E>
__global__ __launch_bounds__(kIsectBlock) void k_sg_items(sg_in<V, E> a, long long* cnt, long long* nseg,
                                                          long long const* ooff, sg_out<V> out)
{
  int const tid = threadIdx.x, lane = tid & 63;
  V* const stage = isect_stage<V>();
  for (long long k0 = blockIdx.x * (long long)kIsectBlock; k0 < a.m; k0 += (long long)gridDim.x * kIsectBlock) {
    long long const w = k0 + tid;
    sg_item it;
    int tier = kSgNone;
    if (w < a.m) {
      it   = sg_decode(a, w);
      tier = sg_tier(it.len, it.nl, a.path, a.split_min);
    }
    long long c = 0;
    if (tier == kSgThread) {
      if constexpr (Fill) {
        long long o = ooff[w];
        sg_row_hits<V>(a.idx + it.b, it.len, a.keys + it.lb, it.nl, (sg_key_t)it.base,
                       [&](long long j) { sg_put<V>(out, a.idx, o++, (V)it.u, it.b + j); });
      } else {
        c = sg_row_hits<V>(a.idx + it.b, it.len, a.keys + it.lb, it.nl, (sg_key_t)it.base, [](long long) {});
      }
    }
    unsigned long long todo = __ballot(tier == kSgWave);
    while (todo) {  // wave-uniform
      int const l = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      long long const u = __shfl(it.u, l, 64), b = __shfl(it.b, l, 64), len = __shfl(it.len, l, 64);
      long long const lb = __shfl(it.lb, l, 64), nl = __shfl(it.nl, l, 64), base = __shfl(it.base, l, 64);
      if constexpr (Fill) {
        long long const o = ooff[k0 + (tid - lane) + l];
        sg_wave_hits<V>(a.idx + b, 0, len, a.keys + lb, nl, (sg_key_t)base, stage, a.stage_div, lane,
                        [&](long long j, long long r) { sg_put<V>(out, a.idx, o + r, (V)u, b + j); });
      } else {
        long long const cw = sg_wave_hits<V>(a.idx + b, 0, len, a.keys + lb, nl, (sg_key_t)base, stage, a.stage_div,
                                             lane, [](long long, long long) {});
        if (lane == l) c = cw;
      }
    }
    if constexpr (!Fill) {
      if (w < a.m) {
        cnt[w]  = c;
        nseg[w] = tier == kSgSplit ? sg_segments(it.len) : 0;
      }
    }
  }
}

// A wave per segment of the split rows.  segoff[w] = the segments before item w (m + 1 entries).
// Count: segcnt[sg] = the segment's hits.  Fill: they go to ooff[w] + the hits of the item's earlier
// segments (segscan = the exclusive scan of segcnt).
template <bool Fill, typename V, typename E>
__global__ __launch_bounds__(kIsectBlock) void k_sg_segments(sg_in<V, E> a, long long const* segoff, long long nsegs,
                                                             long long* segcnt, long long const* segscan,
                                                             long long const* ooff, sg_out<V> out)
{
  int const tid = threadIdx.x, lane = tid & 63;
  V* const stage         = isect_stage<V>();
  long long const wave   = (blockIdx.x * (long long)blockDim.x + tid) >> 6;
  long long const nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long sg = wave; sg < nsegs; sg += nwaves) {  // wave-uniform
    // the last item whose first segment is not above sg: the one that owns it (segoff[m] = nsegs > sg)
    long long lo = 0, hi = a.m;
    while (lo < hi) {
      long long const mid = (lo + hi + 1) >> 1;
      if (segoff[mid] <= sg) lo = mid;
      else hi = mid - 1;
    }
    long long const w  = lo;
    sg_item const it   = sg_decode(a, w);
    long long const s0 = (sg - segoff[w]) * kSgSegLen;
    long long const s1 = s0 + kSgSegLen < it.len ? s0 + kSgSegLen : it.len;
    if constexpr (Fill) {
      long long const o = ooff[w] + segscan[sg] - segscan[segoff[w]];
      sg_wave_hits<V>(a.idx + it.b, s0, s1, a.keys + it.lb, it.nl, (sg_key_t)it.base, stage, a.stage_div, lane,
                      [&](long long j, long long r) { sg_put<V>(out, a.idx, o + r, (V)it.u, it.b + j); });
    } else {
      long long const cw = sg_wave_hits<V>(a.idx + it.b, s0, s1, a.keys + it.lb, it.nl, (sg_key_t)it.base, stage,
                                           a.stage_div, lane, [](long long, long long) {});
      if (lane == 0) segcnt[sg] = cw;
    }
  }
}

// cnt[w] of the split items: the sum of their segments' counts
__global__ __launch_bounds__(kBlock) void k_sg_split_counts(long long const* segoff, long long const* segscan,
                                                           long long m, long long* cnt)
{
  for (long long w = blockIdx.x * (long long)blockDim.x + threadIdx.x; w < m; w += (long long)gridDim.x * blockDim.x)
    if (segoff[w + 1] > segoff[w]) cnt[w] = segscan[segoff[w + 1]] - segscan[segoff[w]];
}

// ---------------------------------------------------------------- keys
// keys[j] = slot(j) * nv + ids[j], slot(j) the subgraph whose range of offs[0 .. ns] holds j
template <typename V>
__global__ __launch_bounds__(kBlock) void k_sg_pack(V const* ids, long long n, long long const* offs, long long ns,
                                                    sg_key_t nv, sg_key_t* keys)
{
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < n; j += (long long)gridDim.x * blockDim.x) {
    long long lo = 0, hi = ns;  // the last slot with offs[slot] <= j (offs[0] = 0, offs[ns] = n > j)
    while (lo < hi) {
      long long const mid = (lo + hi + 1) >> 1;
      if (offs[mid] <= j) lo = mid;
      else hi = mid - 1;
    }
    keys[j] = (sg_key_t)lo * nv + (sg_key_t)ids[j];
  }
}

__global__ __launch_bounds__(kBlock) void k_sg_repeats(sg_key_t const* keys, long long n, int* bad)
{
  for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x + 1; j < n;
       j += (long long)gridDim.x * blockDim.x)
    if (keys[j] == keys[j - 1]) atomicOr(bad, 1);
}

// bounds[i] = the first position of keys[0, n) not below i * nv, i = 0 .. ns; with fofs, also
// sums[i] = fofs[bounds[i]]
__global__ __launch_bounds__(kBlock) void k_sg_slot_bounds(sg_key_t const* keys, long long n, sg_key_t nv,
                                                           long long ns, long long* bounds, long long const* fofs,
                                                           long long* sums)
{
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i <= ns;
       i += (long long)gridDim.x * blockDim.x) {
    long long const p = sg_lower_bound(keys, n, (sg_key_t)i * nv);
    bounds[i]         = p;
    if (sums) sums[i] = fofs[p];
  }
}

template <typename V>
__global__ __launch_bounds__(kBlock) void k_ego_seed_keys(V const* ids, long long n, sg_key_t nv, sg_key_t* keys)
{
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    keys[i] = (sg_key_t)i * nv + (sg_key_t)ids[i];
}

// ---------------------------------------------------------------- ego hops
// deg[i] = the row length of frontier key i's vertex; deg[n] = 0
template <typename E>
__global__ __launch_bounds__(kBlock) void k_ego_degrees(E const* off, sg_key_t const* fr, long long n, sg_key_t nv,
                                                        long long* deg)
{
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i <= n;
       i += (long long)gridDim.x * blockDim.x) {
    long long d = 0;
    if (i < n) {
      sg_key_t const v = fr[i] % nv;
      d                = (long long)off[v + 1] - (long long)off[v];
    }
    deg[i] = d;
  }
}

// Frontier keys [f0, f1), 64 per wave and step; the lanes share the rows' entries evenly.  Keys: the
// candidate of entry t of the range goes to out[fofs[.] - fofs[f0] + .].  Bits (one slot's keys): the
// neighbour's bit is set instead.
template <bool Bits, typename V, typename E>
__global__ __launch_bounds__(kBlock) void k_ego_expand(E const* off, V const* idx, sg_key_t const* fr, long long f0,
                                                       long long f1, long long const* fofs, sg_key_t nv,
                                                       sg_key_t* out, unsigned* bits)
{
  int const lane          = threadIdx.x & 63;
  long long const wave    = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
  long long const nwaves  = ((long long)gridDim.x * blockDim.x) >> 6;
  long long const nchunks = (f1 - f0 + 63) >> 6;
  long long const base    = fofs[f0];
  for (long long c = wave; c < nchunks; c += nwaves) {  // wave-uniform
    long long const i = f0 + c * 64 + lane;
    long long wb = 0, dw = 0, hi = 0;
    if (i < f1) {
      sg_key_t const key  = fr[i];
      sg_key_t const slot = key / nv;
      sg_key_t const v    = key - slot * nv;
      hi                  = (long long)(slot * nv);
      wb                  = (long long)off[v];
      dw                  = (long long)off[v + 1] - wb;
    }
    long long incl = dw;  // entries of lanes 0 .. lane
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      long long const t = __shfl_up(incl, o, 64);
      if (lane >= o) incl += t;
    }
    long long const excl  = incl - dw;
    long long const total = __shfl(incl, 63, 64);
    long long const obase = fofs[f0 + c * 64] - base;
    for (long long t0 = 0; t0 < total; t0 += 64) {  // every lane runs every round: the shuffles need them all
      long long const t = t0 + lane;
      long long const q = t < total ? t : total - 1;
      int lo = 0, hi_l = 63;  // the lane whose entries hold q: the first with incl > q
#pragma unroll
      for (int it = 0; it < 6; ++it) {
        int const mid     = (lo + hi_l) >> 1;
        long long const v = __shfl(incl, mid, 64);
        if (v <= q) lo = mid + 1;
        else hi_l = mid;
      }
      long long const er = __shfl(excl, lo, 64);
      long long const br = __shfl(wb, lo, 64);
      long long const hr = __shfl(hi, lo, 64);
      if (t < total) {
        sg_key_t const x = (sg_key_t)idx[br + (q - er)];
        if constexpr (Bits) atomicOr(bits + (x >> 5), 1u << (x & 31));
        else out[obase + t] = (sg_key_t)hr + x;
      }
    }
  }
}

// the first key of every run, unless it is a member already
__global__ __launch_bounds__(kBlock) void k_ego_new(sg_key_t const* keys, size_t n, sg_key_t const* members,
                                                    long long m, uint8_t* flags)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    sg_key_t const k = keys[i];
    bool keep        = i == 0 || keys[i - 1] != k;
    if (keep) {
      long long const p = sg_lower_bound(members, m, k);
      keep              = !(p < m && members[p] == k);
    }
    flags[i] = keep ? 1 : 0;
  }
}

// the members [m0, m1) of one slot leave its map
__global__ __launch_bounds__(kBlock) void k_ego_clear_bits(sg_key_t const* members, long long m0, long long m1,
                                                           sg_key_t base, unsigned* bits)
{
  for (long long i = m0 + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < m1;
       i += (long long)gridDim.x * blockDim.x) {
    sg_key_t const x = members[i] - base;
    atomicAnd(bits + (x >> 5), ~(1u << (x & 31)));
  }
}

// set bits per word (words + 1 entries, the last one 0)
__global__ __launch_bounds__(kBlock) void k_ego_bit_counts(unsigned const* bits, size_t words, long long* counts)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i <= words; i += (size_t)gridDim.x * blockDim.x)
    counts[i] = i < words ? __popc(bits[i]) : 0;
}

__global__ __launch_bounds__(kBlock) void k_ego_bit_keys(unsigned const* bits, size_t words, sg_key_t base,
                                                         long long const* wofs, sg_key_t* keys)
{
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) {
    unsigned w  = bits[i];
    long long o = wofs[i];
    while (w) {
      int const bit = __ffs((int)w) - 1;
      w &= w - 1;
      keys[o++] = base + ((sg_key_t)i << 5) + (sg_key_t)bit;
    }
  }
}

template <typename In, typename Out>
size_t sg_select_flagged(In in, uint8_t const* flags, Out* out, size_t n, hipStream_t s)
{
  dbuf<size_t> cnt(1, s);
  size_t tmp = 0;
  HIP_CHECK(rocprim::select(nullptr, tmp, in, flags, out, cnt.data(), n, s));
  buffer t(tmp, s);
  HIP_CHECK(rocprim::select(t.data(), tmp, in, flags, out, cnt.data(), n, s));
  return to_host_scalar(cnt.data(), s);
}

unsigned sg_grid() { return (unsigned)std::max(device_cu_count(), 1) * kSgGridPerCu; }

// ---------------------------------------------------------------- extraction
void sg_empty_result(handle_t& h, graph_t& g, size_t ns, induced_subgraph_result_t& res)
{
  hipStream_t s = h.stream;
  alloc_edge_arrays(g, 0, s, res.src, res.dst, res.weights);
  res.offsets = std::make_unique<device_array_t>(ns + 1, INT64, s);
  HIP_CHECK(hipMemsetAsync(res.offsets->buf.data(), 0, (ns + 1) * sizeof(long long), s));
}

// keys: the m sorted member keys; soff: the ns + 1 offsets of the subgraphs into them (device)
template <typename V, typename E>
void sg_extract(handle_t& h, graph_t& g, sg_key_t const* keys, long long m, long long const* soff, size_t ns,
                induced_subgraph_result_t& res)
{
  hipStream_t s = h.stream;
  if (m == 0 || g.num_edges == 0) return sg_empty_result(h, g, ns, res);
  adjacency_t& adj = ensure_adjacency(h, g, false);  // out-edges: sources are row vertices
  sg_in<V, E> a;
  a.off       = adj.offsets.data<E>();
  a.idx       = adj.indices.data<V>();
  a.keys      = keys;
  a.soff      = soff;
  a.m         = m;
  a.nv        = (sg_key_t)g.num_vertices;
  a.path      = h.tune.sg_path;
  a.split_min = std::max<long long>(h.tune.sg_split_min, 1);
  a.stage_div = kIsectStageDiv;
  unsigned const grid  = sg_grid();
  unsigned const igrid = grid_for((size_t)m, kIsectBlock, grid);
  sg_out<V> none{};

  dbuf<long long> cnt((size_t)m + 1, s), nseg((size_t)m + 1, s), segoff((size_t)m + 1, s), ooff((size_t)m + 1, s);
  HIP_CHECK(hipMemsetAsync(cnt.data() + m, 0, sizeof(long long), s));
  HIP_CHECK(hipMemsetAsync(nseg.data() + m, 0, sizeof(long long), s));
  hipLaunchKernelGGL((k_sg_items<false, V, E>), dim3(igrid), dim3(kIsectBlock), 0, s, a, cnt.data(), nseg.data(),
                     (long long const*)nullptr, none);
  CGX_LAUNCH_CHECK();
  exclusive_scan<long long, long long>(nseg.data(), segoff.data(), (size_t)m + 1, s);
  long long const nsegs = to_host_scalar(segoff.data() + m, s);
  h.last_hot_launches   = (size_t)nsegs;  // the split tier's segments (ext.h, cugraph_amd_last_hot_kernel_launches)
  nseg.free();
  dbuf<long long> segcnt, segscan;
  unsigned const sgrid = grid_for((size_t)nsegs * 64, kIsectBlock, grid);
  if (nsegs > 0) {
    segcnt.resize((size_t)nsegs + 1, s);
    segscan.resize((size_t)nsegs + 1, s);
    HIP_CHECK(hipMemsetAsync(segcnt.data() + nsegs, 0, sizeof(long long), s));
    hipLaunchKernelGGL((k_sg_segments<false, V, E>), dim3(sgrid), dim3(kIsectBlock), 0, s, a,
                       (long long const*)segoff.data(), nsegs, segcnt.data(), (long long const*)nullptr,
                       (long long const*)nullptr, none);
    CGX_LAUNCH_CHECK();
    exclusive_scan<long long, long long>(segcnt.data(), segscan.data(), (size_t)nsegs + 1, s);
    segcnt.free();
    hipLaunchKernelGGL(k_sg_split_counts, dim3(grid_for((size_t)m, kBlock, grid)), dim3(kBlock), 0, s,
                       (long long const*)segoff.data(), (long long const*)segscan.data(), m, cnt.data());
    CGX_LAUNCH_CHECK();
  }
  exclusive_scan<long long, long long>(cnt.data(), ooff.data(), (size_t)m + 1, s);
  cnt.free();
  size_t const total = (size_t)to_host_scalar(ooff.data() + m, s);

  alloc_edge_arrays(g, total, s, res.src, res.dst, res.weights);
  res.offsets = std::make_unique<device_array_t>(ns + 1, INT64, s);
  gather<long long, long long>(res.offsets->buf.data<long long>(), ooff.data(), soff, ns + 1, s);
  if (total == 0) return;
  sg_out<V> out;
  out.src    = res.src->buf.data<V>();
  out.dst    = res.dst->buf.data<V>();
  out.gw     = g.weighted ? adj.weights.data() : nullptr;
  out.w      = g.weighted ? res.weights->buf.data() : nullptr;
  out.wbytes = (int)dtype_size(g.weight_type);
  hipLaunchKernelGGL((k_sg_items<true, V, E>), dim3(igrid), dim3(kIsectBlock), 0, s, a, (long long*)nullptr,
                     (long long*)nullptr, (long long const*)ooff.data(), out);
  CGX_LAUNCH_CHECK();
  if (nsegs > 0) {
    hipLaunchKernelGGL((k_sg_segments<true, V, E>), dim3(sgrid), dim3(kIsectBlock), 0, s, a,
                       (long long const*)segoff.data(), nsegs, (long long*)nullptr, (long long const*)segscan.data(),
                       (long long const*)ooff.data(), out);
    CGX_LAUNCH_CHECK();
  }
  unrenumber_edge_arrays(h, g, *res.src, *res.dst, total);
}

char const* const kSgFitMsg =
  ": the packed (subgraph, vertex) keys need subgraphs x vertices to fit 64 bits";

template <typename V, typename E>
void induced_impl(handle_t& h, graph_t& g, array_view_t const& offsets, array_view_t const& vertices,
                  induced_subgraph_result_t& res)
{
  hipStream_t s    = h.stream;
  size_t const ns  = offsets.size - 1;
  size_t const n   = vertices.size;
  int64_t const nv = g.num_vertices;
  std::vector<long long> hoff(ns + 1);
  HIP_CHECK(hipMemcpyAsync(hoff.data(), offsets.data, (ns + 1) * sizeof(long long), hipMemcpyDefault, s));
  HIP_CHECK(hipStreamSynchronize(s));
  bool ok = hoff[0] == 0 && hoff[ns] == (long long)n;
  for (size_t i = 0; ok && i < ns; ++i) ok = hoff[i] <= hoff[i + 1];
  CGX_INPUT(ok, "Invalid input argument: subgraph_offsets must start at 0, not decrease and end at the size of "
                "subgraph_vertices.");
  CGX_EXPECTS(sg_keys_fit(ns, (unsigned long long)nv), CUGRAPH_NOT_IMPLEMENTED,
              std::string("extract_induced_subgraph") + kSgFitMsg);
  if (n == 0) return sg_empty_result(h, g, ns, res);
  CGX_INPUT(nv > 0, "Invalid input argument: vertex id not in the graph.");
  dbuf<V> ids(n, s);
  HIP_CHECK(hipMemcpyAsync(ids.data(), vertices.data, n * sizeof(V), hipMemcpyDefault, s));
  renumber_ext_to_int(h, g, ids.data(), n, true);  // an unknown id: CUGRAPH_INVALID_INPUT
  dbuf<long long> soff(ns + 1, s);
  to_device(soff.data(), hoff.data(), ns + 1, s);
  dbuf<sg_key_t> k0(n, s), k1(n, s);
  hipLaunchKernelGGL(k_sg_pack<V>, dim3(grid_for(n, kBlock, sg_grid())), dim3(kBlock), 0, s, (V const*)ids.data(),
                     (long long)n, (long long const*)soff.data(), (long long)ns, (sg_key_t)nv, k0.data());
  CGX_LAUNCH_CHECK();
  radix_sort_keys<sg_key_t>(k0.data(), k1.data(), n, 0, sg_key_bits(ns, (unsigned long long)nv), s);
  k0.free();
  dbuf<int> bad(1, s);
  HIP_CHECK(hipMemsetAsync(bad.data(), 0, sizeof(int), s));
  hipLaunchKernelGGL(k_sg_repeats, dim3(grid_for(n, kBlock, sg_grid())), dim3(kBlock), 0, s,
                     (sg_key_t const*)k1.data(), (long long)n, bad.data());
  CGX_LAUNCH_CHECK();
  CGX_INPUT(to_host_scalar(bad.data(), s) == 0,  // also waits for the copy out of hoff
            "Invalid input argument: a vertex is repeated inside one subgraph.");
  sg_extract<V, E>(h, g, k1.data(), (long long)n, soff.data(), ns, res);
  HIP_CHECK(hipStreamSynchronize(s));  // the temporaries go out of scope
}

// one hop of every slot: the next frontier (ascending keys that are no members yet) into `next`
template <typename V, typename E>
void ego_hop(handle_t& h, graph_t& g, adjacency_t& adj, size_t ns, dbuf<sg_key_t> const& members,
             dbuf<sg_key_t> const& frontier, dbuf<sg_key_t>& next)
{
  hipStream_t s       = h.stream;
  sg_key_t const nv   = (sg_key_t)g.num_vertices;
  E const* off        = adj.offsets.data<E>();
  V const* idx        = adj.indices.data<V>();
  long long const nf  = (long long)frontier.size();
  long long const nm  = (long long)members.size();
  unsigned const grid = sg_grid();

  dbuf<long long> deg((size_t)nf + 1, s), fofs((size_t)nf + 1, s), fslot(ns + 1, s), slotc(ns + 1, s);
  hipLaunchKernelGGL(k_ego_degrees<E>, dim3(grid_for((size_t)nf + 1, kBlock, grid)), dim3(kBlock), 0, s, off,
                     (sg_key_t const*)frontier.data(), nf, nv, deg.data());
  CGX_LAUNCH_CHECK();
  exclusive_scan<long long, long long>(deg.data(), fofs.data(), (size_t)nf + 1, s);
  deg.free();
  hipLaunchKernelGGL(k_sg_slot_bounds, dim3(grid_for(ns + 1, kBlock, grid)), dim3(kBlock), 0, s,
                     (sg_key_t const*)frontier.data(), nf, nv, (long long)ns, fslot.data(),
                     (long long const*)fofs.data(), slotc.data());
  CGX_LAUNCH_CHECK();
  std::vector<long long> const hslot = to_host(fslot.data(), ns + 1, s);
  std::vector<long long> const hc    = to_host(slotc.data(), ns + 1, s);
  auto cand = [&](size_t i) { return hc[i + 1] - hc[i]; };  // slot i's candidates this hop

  long long const budget = std::max<long long>(h.tune.ego_budget, 1);
  long long cap          = 0;  // the largest batch
  bool heavy             = false;
  for (size_t i = 0; i < ns;) {
    if (cand(i) > budget) { heavy = true; ++i; continue; }
    long long sum = 0;
    for (; i < ns && cand(i) <= budget && sum + cand(i) <= budget; ++i) sum += cand(i);
    cap = std::max(cap, sum);
  }
  dbuf<sg_key_t> k0, k1;
  dbuf<uint8_t> flags;
  if (cap > 0) {
    k0.resize((size_t)cap, s);
    k1.resize((size_t)cap, s);
    flags.resize((size_t)cap, s);
  }
  size_t const words = ((size_t)nv + 31) / 32;
  dbuf<unsigned> bits;
  dbuf<long long> bcnt, bofs, mslot;
  std::vector<long long> hmslot;
  if (heavy) {
    bits.resize(words, s);
    bcnt.resize(words + 1, s);
    bofs.resize(words + 1, s);
    mslot.resize(ns + 1, s);
    hipLaunchKernelGGL(k_sg_slot_bounds, dim3(grid_for(ns + 1, kBlock, grid)), dim3(kBlock), 0, s,
                       (sg_key_t const*)members.data(), nm, nv, (long long)ns, mslot.data(),
                       (long long const*)nullptr, (long long*)nullptr);
    CGX_LAUNCH_CHECK();
    hmslot = to_host(mslot.data(), ns + 1, s);
  }
  int const key_bits = sg_key_bits(ns, nv);
  std::vector<dbuf<sg_key_t>> blocks;  // the new keys, in slot order
  size_t total = 0;
  for (size_t i = 0; i < ns;) {
    if (cand(i) > budget) {  // a slot above the budget, through the V-bit map
      long long const f0 = hslot[i], f1 = hslot[i + 1];
      sg_key_t const base = (sg_key_t)i * nv;
      HIP_CHECK(hipMemsetAsync(bits.data(), 0, words * sizeof(unsigned), s));
      hipLaunchKernelGGL((k_ego_expand<true, V, E>), dim3(grid_for((size_t)(f1 - f0), kBlock, grid)), dim3(kBlock), 0,
                         s, off, idx, (sg_key_t const*)frontier.data(), f0, f1, (long long const*)fofs.data(), nv,
                         (sg_key_t*)nullptr, bits.data());
      hipLaunchKernelGGL(k_ego_clear_bits, dim3(grid_for((size_t)(hmslot[i + 1] - hmslot[i]), kBlock, grid)),
                         dim3(kBlock), 0, s, (sg_key_t const*)members.data(), hmslot[i], hmslot[i + 1], base,
                         bits.data());
      hipLaunchKernelGGL(k_ego_bit_counts, dim3(grid_for(words + 1, kBlock, grid)), dim3(kBlock), 0, s,
                         (unsigned const*)bits.data(), words, bcnt.data());
      CGX_LAUNCH_CHECK();
      exclusive_scan<long long, long long>(bcnt.data(), bofs.data(), words + 1, s);
      size_t const n = (size_t)to_host_scalar(bofs.data() + words, s);
      if (n) {
        dbuf<sg_key_t> blk(n, s);
        hipLaunchKernelGGL(k_ego_bit_keys, dim3(grid_for(words, kBlock, grid)), dim3(kBlock), 0, s,
                           (unsigned const*)bits.data(), words, base, (long long const*)bofs.data(), blk.data());
        CGX_LAUNCH_CHECK();
        blocks.push_back(std::move(blk));
        total += n;
      }
      ++i;
      continue;
    }
    size_t const i0 = i;
    long long sum   = 0;
    for (; i < ns && cand(i) <= budget && sum + cand(i) <= budget; ++i) sum += cand(i);
    if (sum == 0) continue;
    long long const f0 = hslot[i0], f1 = hslot[i];
    hipLaunchKernelGGL((k_ego_expand<false, V, E>), dim3(grid_for((size_t)(f1 - f0), kBlock, grid)), dim3(kBlock), 0,
                       s, off, idx, (sg_key_t const*)frontier.data(), f0, f1, (long long const*)fofs.data(), nv,
                       k0.data(), (unsigned*)nullptr);
    CGX_LAUNCH_CHECK();
    radix_sort_keys<sg_key_t>(k0.data(), k1.data(), (size_t)sum, 0, key_bits, s);
    hipLaunchKernelGGL(k_ego_new, dim3(grid_for((size_t)sum, kBlock, 1u << 16)), dim3(kBlock), 0, s,
                       (sg_key_t const*)k1.data(), (size_t)sum, (sg_key_t const*)members.data(), nm, flags.data());
    CGX_LAUNCH_CHECK();
    size_t const n = sg_select_flagged((sg_key_t const*)k1.data(), flags.data(), k0.data(), (size_t)sum, s);
    if (n) {
      dbuf<sg_key_t> blk(n, s);
      HIP_CHECK(hipMemcpyAsync(blk.data(), k0.data(), n * sizeof(sg_key_t), hipMemcpyDeviceToDevice, s));
      blocks.push_back(std::move(blk));
      total += n;
    }
  }
  next.resize(total, s);
  size_t at = 0;
  for (auto& blk : blocks) {
    HIP_CHECK(hipMemcpyAsync(next.data() + at, blk.data(), blk.size() * sizeof(sg_key_t), hipMemcpyDeviceToDevice, s));
    at += blk.size();
    blk.free();
  }
}

template <typename V, typename E>
void ego_impl(handle_t& h, graph_t& g, array_view_t const& sources, size_t radius, induced_subgraph_result_t& res)
{
  hipStream_t s    = h.stream;
  size_t const ns  = sources.size;
  int64_t const nv = g.num_vertices;
  if (ns == 0) return sg_empty_result(h, g, 0, res);
  CGX_EXPECTS(sg_keys_fit(ns, (unsigned long long)nv), CUGRAPH_NOT_IMPLEMENTED,
              std::string("extract_ego") + kSgFitMsg);
  CGX_INPUT(nv > 0, "Invalid input argument: vertex id not in the graph.");
  dbuf<V> ids(ns, s);
  HIP_CHECK(hipMemcpyAsync(ids.data(), sources.data, ns * sizeof(V), hipMemcpyDefault, s));
  renumber_ext_to_int(h, g, ids.data(), ns, true);  // an unknown id: CUGRAPH_INVALID_INPUT
  if (g.num_edges == 0) return sg_empty_result(h, g, ns, res);
  adjacency_t& adj = ensure_adjacency(h, g, false);
  dbuf<sg_key_t> members(ns, s), frontier(ns, s);
  hipLaunchKernelGGL(k_ego_seed_keys<V>, dim3(grid_for(ns, kBlock, sg_grid())), dim3(kBlock), 0, s,
                     (V const*)ids.data(), (long long)ns, (sg_key_t)nv, members.data());
  CGX_LAUNCH_CHECK();
  HIP_CHECK(hipMemcpyAsync(frontier.data(), members.data(), ns * sizeof(sg_key_t), hipMemcpyDeviceToDevice, s));
  size_t hops = 0;
  for (; hops < radius && frontier.size() > 0; ++hops) {
    dbuf<sg_key_t> next;
    ego_hop<V, E>(h, g, adj, ns, members, frontier, next);
    if (next.size() > 0) {
      size_t const nm = members.size(), nn = next.size();
      dbuf<sg_key_t> merged(nm + nn, s);
      size_t tmp = 0;
      HIP_CHECK(rocprim::merge(nullptr, tmp, (sg_key_t const*)members.data(), (sg_key_t const*)next.data(),
                               merged.data(), nm, nn, rocprim::less<sg_key_t>(), s));
      buffer t(tmp, s);
      HIP_CHECK(rocprim::merge(t.data(), tmp, (sg_key_t const*)members.data(), (sg_key_t const*)next.data(),
                               merged.data(), nm, nn, rocprim::less<sg_key_t>(), s));
      members = std::move(merged);
    }
    frontier = std::move(next);
  }
  h.last_iterations = hops;
  dbuf<long long> soff(ns + 1, s);
  hipLaunchKernelGGL(k_sg_slot_bounds, dim3(grid_for(ns + 1, kBlock, sg_grid())), dim3(kBlock), 0, s,
                     (sg_key_t const*)members.data(), (long long)members.size(), (sg_key_t)nv, (long long)ns,
                     soff.data(), (long long const*)nullptr, (long long*)nullptr);
  CGX_LAUNCH_CHECK();
  sg_extract<V, E>(h, g, members.data(), (long long)members.size(), soff.data(), ns, res);
  HIP_CHECK(hipStreamSynchronize(s));  // the temporaries go out of scope
}

}  // namespace

void run_induced_subgraph(handle_t& h, graph_t& g, array_view_t const& offsets, array_view_t const& vertices,
                          induced_subgraph_result_t& res)
{
  reset_hot(h);
  dispatch_ve(g.vertex_type, g.edge_type, [&](auto t) {
    using T = decltype(t);
    induced_impl<typename T::vertex_t, typename T::edge_t>(h, g, offsets, vertices, res);
  });
}

void run_extract_ego(handle_t& h, graph_t& g, array_view_t const& sources, size_t radius,
                     induced_subgraph_result_t& res)
{
  reset_hot(h);
  dispatch_ve(g.vertex_type, g.edge_type, [&](auto t) {
    using T = decltype(t);
    ego_impl<typename T::vertex_t, typename T::edge_t>(h, g, sources, radius, res);
  });
}

}  // namespace cgx
