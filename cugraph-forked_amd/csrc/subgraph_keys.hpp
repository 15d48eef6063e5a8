// Induced subgraphs and ego nets (subgraph.hip): the packed (subgraph slot, vertex) keys and the
// thread-level membership test, as plain C++ that a host-only program can include
// (tests/c/ego_keys_test.cpp).
//
// A member vertex v of subgraph `slot` is the 64-bit key slot * V + v.  Keys of one call sort by slot
// and then by vertex, so the sorted key array is every subgraph's ascending member list back to back,
// and slot * V is the value to add to a row entry before it is looked up in that list.
#pragma once

#if defined(__HIPCC__)
#define CGX_SG_FN __host__ __device__ __forceinline__
#else
#define CGX_SG_FN inline
#endif

namespace cgx {

using sg_key_t = unsigned long long;

constexpr long long kSgSegLen = 1024;  // row entries per segment of the split tier: 16 steps of a wave

// slots * nv must fit 64 bits: the largest key is slots * nv - 1, and slots * nv itself is the bound
// the last slot's range is searched with.  No slots or no vertices always fit.
CGX_SG_FN bool sg_keys_fit(unsigned long long slots, unsigned long long nv)
{
  return slots == 0 || nv == 0 || slots <= ~0ull / nv;
}

// radix sort bits of the keys below slots * nv (sg_keys_fit holds); at least 1
CGX_SG_FN int sg_key_bits(unsigned long long slots, unsigned long long nv)
{
  unsigned long long const top = (slots == 0 || nv == 0) ? 0 : slots * nv - 1;
  int b                        = 0;
  while (b < 64 && (top >> b) != 0) ++b;
  return b == 0 ? 1 : b;
}

// segments of a split row of len entries
CGX_SG_FN long long sg_segments(long long len) { return (len + kSgSegLen - 1) / kSgSegLen; }

// whether a thread looks every row entry up in the list (true) or merges the two (false): the search
// costs about len * log2(nl) probes, the merge len + nl steps
CGX_SG_FN bool sg_search_pays(long long len, long long nl)
{
  int lg = 1;
  while (lg < 63 && (1ll << lg) < nl) ++lg;
  return len * lg < len + nl;
}

// first position of keys[0, n) that is not below k
CGX_SG_FN long long sg_lower_bound(sg_key_t const* keys, long long n, sg_key_t k)
{
  long long lo = 0, hi = n;
  while (lo < hi) {
    long long const mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One thread: emit(j) for every position j of row[0, len), in ascending j, whose entry is a member,
// that is, base + row[j] is in list[0, nl).  The row ascends and may repeat an id: every copy is emitted.
// The list ascends without repeats.  Returns the number of hits.
template <typename V, typename F>
CGX_SG_FN long long sg_row_hits(V const* row, long long len, sg_key_t const* list, long long nl, sg_key_t base,
                                F const& emit)
{
  long long c = 0;
  if (len == 0 || nl == 0) return 0;
  if (sg_search_pays(len, nl)) {
    for (long long j = 0; j < len; ++j) {
      sg_key_t const k   = base + (sg_key_t)row[j];
      long long const lo = sg_lower_bound(list, nl, k);
      if (lo < nl && list[lo] == k) {
        emit(j);
        ++c;
      }
    }
    return c;
  }
  long long i = 0;
  for (long long j = 0; j < len; ++j) {
    sg_key_t const k = base + (sg_key_t)row[j];
    while (i < nl && list[i] < k) ++i;
    if (i == nl) break;
    if (list[i] == k) {  // the list position stays: the next row entry may be another copy
      emit(j);
      ++c;
    }
  }
  return c;
}

}  // namespace cgx
