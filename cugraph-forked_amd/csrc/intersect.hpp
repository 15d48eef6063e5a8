// Intersection of two sorted adjacency rows: the one copy that triangle_count.hip and
// similarity.hip share (Row intersection).  Rows ascend and may repeat an id; a
// repeated id counts once.  `hit(x)` is called once per distinct common id x (triangle
// counting adds to the third vertex there, similarity passes isect_ignore).
//   * isect_merge: one thread, two short rows;
//   * isect_probe: one lane's share of a wave that looks entries [s0, s1) of the shorter
//     row up in the longer one by binary search;
//   * isect_wave_count: the whole wave, with the longer row staged in the wave's LDS
//     slice when it fits and pays;
//   * isect_merge_at, isect_probe_at, isect_wave_at: the same three with `hit(x, i, j)`,
//     the positions of x's first copies in the two rows (k_truss.hip).
// The thread-level pieces and sim_seg_len are plain C++ that a host-only program can
// include (tests/c/intersect_test.cpp, intersect_at_test.cpp); the wave-level ones need the HIP compiler.
#pragma once

#if defined(__HIPCC__)
#include "prims.hpp"
#define CGX_ISECT_FN __host__ __device__ __forceinline__
#else
#define CGX_ISECT_FN inline
#endif

namespace cgx {

// A/B builds (Similarity / two-hop) override similarity's two cuts on the
// compiler's command line; triangle counting keeps kIsectWaveLen / kIsectStageDiv
#ifndef CGX_SIM_WAVE_LEN
#define CGX_SIM_WAVE_LEN kIsectWaveLen
#endif
#ifndef CGX_SIM_STAGE_DIV
#define CGX_SIM_STAGE_DIV kIsectStageDiv
#endif

constexpr int kIsectBlock      = 256;   // threads per block of the kernels that intersect
constexpr int kIsectWaveLen    = 64;    // a work item with a row of at least this many entries: the wave
constexpr int kIsectStageBytes = 4096;  // LDS slice of a wave (1024 4-byte or 512 8-byte ids), 16 KiB per block
constexpr int kIsectStageDiv   = 64;    // stage the longer row when the probing part has at least 1/64 of
                                        // its entries (0: never)
constexpr int kSimWaveLen      = CGX_SIM_WAVE_LEN;
constexpr int kSimStageDiv     = CGX_SIM_STAGE_DIV;
constexpr int kSimSegLen       = 256;   // entries of the shorter row per split segment (4 probes per lane)

template <typename V>
constexpr int kIsectStageLen = kIsectStageBytes / (int)sizeof(V);

using count_t = unsigned long long;

struct isect_ignore {
  template <typename V>
  CGX_ISECT_FN void operator()(V) const
  {
  }
};

// entries per segment of a split pair whose shorter row has ns entries: at most 2^14 + 1
// segments, so a chunk's segment numbers stay below 2^39 (similarity.hip kSimSegBits)
CGX_ISECT_FN long long sim_seg_len(long long ns)
{
  long long const by_count = (ns + 16383) >> 14;
  return by_count > kSimSegLen ? by_count : kSimSegLen;
}

// S: the shorter row, L: the longer
CGX_ISECT_FN void isect_shorter_first(long long& s, long long& ns, long long& l, long long& nl)
{
  if (ns > nl) {
    long long t = s; s = l; l = t;
    t = ns; ns = nl; nl = t;
  }
}

// a thread merges two short rows; runs of equal ids count once
template <typename V, typename F>
CGX_ISECT_FN count_t isect_merge(V const* A, long long na, V const* B, long long nb, F const& hit)
{
  count_t c   = 0;
  long long i = 0, j = 0;
  while (i < na && j < nb) {
    V const x = A[i], y = B[j];
    if (x < y) ++i;
    else if (y < x) ++j;
    else {
      hit(x);
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
template <typename V, typename F>
CGX_ISECT_FN count_t isect_probe(V const* S, long long s0, long long s1, V const* L, long long nl, int lane,
                                 F const& hit)
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
    if (lo < nl && L[lo] == x) {
      hit(x);
      ++c;
    }
  }
  return c;
}

// The position-reporting forms (k_truss.hip reads an edge id at each of the two positions):
// `hit(x, i, j)` gets, once per distinct common id x, the positions of the first copy of x in
// the two rows -- A[i] == B[j] == x for the merge, S[i] == L[j] == x for the probe.
template <typename V, typename F>
CGX_ISECT_FN count_t isect_merge_at(V const* A, long long na, V const* B, long long nb, F const& hit)
{
  count_t c   = 0;
  long long i = 0, j = 0;
  while (i < na && j < nb) {
    V const x = A[i], y = B[j];
    if (x < y) ++i;
    else if (y < x) ++j;
    else {
      hit(x, i, j);
      ++c;
      do ++i; while (i < na && A[i] == x);
      do ++j; while (j < nb && B[j] == x);
    }
  }
  return c;
}

// one lane's share of entries [s0, s1) of S, as isect_probe; the lower bound is x's first copy in L
template <typename V, typename F>
CGX_ISECT_FN count_t isect_probe_at(V const* S, long long s0, long long s1, V const* L, long long nl, int lane,
                                    F const& hit)
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
    if (lo < nl && L[lo] == x) {
      hit(x, i, lo);
      ++c;
    }
  }
  return c;
}

#if defined(__HIPCC__)
__device__ __forceinline__ void bump(count_t* p, count_t c)
{
  __hip_atomic_fetch_add(p, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the calling wave's LDS slice of kIsectStageLen<V> ids (a kIsectBlock-thread block)
template <typename V>
__device__ __forceinline__ V* isect_stage()
{
  __shared__ V stage_all[(kIsectBlock / 64) * kIsectStageLen<V>];
  return stage_all + (threadIdx.x >> 6) * kIsectStageLen<V>;
}

// entries [s0, s1) of S against the whole of L by one wave, L staged when it fits and pays;
// returns the wave's sum in every lane
template <typename V, typename F>
__device__ __forceinline__ count_t isect_wave_count(V const* S, long long s0, long long s1, V const* L, long long nl,
                                                    V* stage, int stage_div, int lane, F const& hit)
{
  count_t cw;
  if (nl <= kIsectStageLen<V> && (s1 - s0) * stage_div >= nl) {
    // DS operations of one wave complete in order; the barriers only pin the compiler
    __builtin_amdgcn_wave_barrier();
    for (long long j = lane; j < nl; j += 64) stage[j] = L[j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    cw = isect_probe<V>(S, s0, s1, (V const*)stage, nl, lane, hit);
    __builtin_amdgcn_wave_barrier();
  } else {
    cw = isect_probe<V>(S, s0, s1, L, nl, lane, hit);
  }
  return (count_t)wave_sum_ll((long long)cw);
}
// the same by isect_probe_at: `hit` gets positions in S and in L (staged or not, the position is L's);
// returns this lane's hits, nothing is summed
template <typename V, typename F>
__device__ __forceinline__ count_t isect_wave_at(V const* S, long long s0, long long s1, V const* L, long long nl,
                                                 V* stage, int stage_div, int lane, F const& hit)
{
  count_t c;
  if (nl <= kIsectStageLen<V> && (s1 - s0) * stage_div >= nl) {
    __builtin_amdgcn_wave_barrier();
    for (long long j = lane; j < nl; j += 64) stage[j] = L[j];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    c = isect_probe_at<V>(S, s0, s1, (V const*)stage, nl, lane, hit);
    __builtin_amdgcn_wave_barrier();
  } else {
    c = isect_probe_at<V>(S, s0, s1, L, nl, lane, hit);
  }
  return c;
}
// (The ballot loop that hands a wave its heavy items one after the other stays in the kernels:
// as a helper taking a lambda it cost no register but rescheduled the loop head, and similarity's
// wave tier measured 1 % slower; profiles/intersect_refactor.md.)
#endif

}  // namespace cgx
