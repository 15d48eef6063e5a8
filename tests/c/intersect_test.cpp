/*
 * The thread-level pieces of csrc/intersect.hpp on the host: isect_merge (the thread tier of
 * triangle counting and similarity), isect_probe (one lane of their wave tier) and sim_seg_len
 * (the split tier's segment length).  Rows are sorted and repeat ids, in int32 and int64, with
 * every pair of lengths from {0, 1, 2, 63, 64, 65, 1024, 1025}:
 *   - the merge count, the probe count summed over lanes 0..63 and std::set_intersection of the
 *     de-duplicated rows agree;
 *   - `hit` receives every common id exactly once, from the merge and from the probe;
 *   - the probe summed over a partition of S into [s0, s1) segments gives the same count, also
 *     when a cut falls inside a run of equal ids (the first copy lies before s0);
 *   - sim_seg_len(ns) gives at most 2^14 + 1 segments for ns from 1 up to 2^40.
 */
#include "intersect.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iterator>
#include <vector>

static unsigned long long rng_state = 42;
static unsigned rnd()
{
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned)(rng_state >> 33);
}

// n ascending ids from `base` on; a step of 0 (one in three) repeats the previous id
template <typename V>
static std::vector<V> make_row(int n, V base)
{
  std::vector<V> r((size_t)n);
  V x = base + (V)(rnd() % 3);
  for (int i = 0; i < n; ++i) {
    if (i) x += (V)(rnd() % 3);
    r[(size_t)i] = x;
  }
  return r;
}

template <typename V>
struct collect {
  std::vector<V>* out;
  void operator()(V x) const { out->push_back(x); }
};

// the probe of entries [s0, s1) by a whole wave
template <typename V>
static cgx::count_t wave_probe(std::vector<V> const& S, long long s0, long long s1, std::vector<V> const& L,
                               std::vector<V>* hits)
{
  cgx::count_t c = 0;
  for (int lane = 0; lane < 64; ++lane)
    c += cgx::isect_probe<V>(S.data(), s0, s1, L.data(), (long long)L.size(), lane, collect<V>{hits});
  return c;
}

// the probe summed over the segments that `cuts` (ascending, within [0, ns]) make of S
template <typename V>
static cgx::count_t probe_cut(std::vector<V> const& S, std::vector<V> const& L, std::vector<long long> cuts)
{
  cuts.push_back((long long)S.size());
  cgx::count_t c = 0;
  long long s0   = 0;
  std::vector<V> ignored;
  for (long long s1 : cuts) {
    c += wave_probe<V>(S, s0, s1, L, &ignored);
    s0 = s1;
  }
  return c;
}

template <typename V>
static int rows(char const* name, V base)
{
  int const lens[] = {0, 1, 2, 63, 64, 65, 1024, 1025};
  long checked = 0, bad = 0, inside_run = 0;
  for (int na : lens)
    for (int nb : lens) {
      std::vector<V> const A = make_row<V>(na, base), B = make_row<V>(nb, base);
      std::vector<V> ua = A, ub = B, want;
      ua.erase(std::unique(ua.begin(), ua.end()), ua.end());
      ub.erase(std::unique(ub.begin(), ub.end()), ub.end());
      std::set_intersection(ua.begin(), ua.end(), ub.begin(), ub.end(), std::back_inserter(want));

      std::vector<V> merged, probed;
      cgx::count_t const cm =
        cgx::isect_merge<V>(A.data(), (long long)na, B.data(), (long long)nb, collect<V>{&merged});
      cgx::count_t const cp = wave_probe<V>(A, 0, na, B, &probed);
      std::sort(probed.begin(), probed.end());  // lanes interleave the entries; the merge ascends already
      bool ok = cm == want.size() && cp == want.size() && merged == want && probed == want;
      ok = ok && cgx::isect_merge<V>(A.data(), (long long)na, B.data(), (long long)nb, cgx::isect_ignore{}) == cm;

      // partitions of S = A: single entries, 7 and 256 entries per segment, and every cut inside a run
      for (long long len : {1LL, 7LL, 256LL}) {
        std::vector<long long> cuts;
        for (long long c = len; c < na; c += len) cuts.push_back(c);
        ok = ok && probe_cut<V>(A, B, cuts) == cm;
      }
      std::vector<long long> run_cuts;
      for (long long i = 1; i < na; ++i)
        if (A[(size_t)i - 1] == A[(size_t)i]) run_cuts.push_back(i);
      inside_run += (long)run_cuts.size();
      ok = ok && probe_cut<V>(A, B, run_cuts) == cm;
      if (!run_cuts.empty()) ok = ok && probe_cut<V>(A, B, {run_cuts[run_cuts.size() / 2]}) == cm;

      ++checked;
      if (!ok) {
        ++bad;
        std::printf("FAIL %s na %d nb %d: merge %llu probe %llu want %zu\n", name, na, nb, cm, cp, want.size());
      }
    }
  std::printf("%s: %ld length pairs, %ld cuts inside a run of equal ids, %ld bad\n", name, checked, inside_run, bad);
  return bad || !inside_run ? 1 : 0;
}

static int shorter_first()
{
  long long s = 10, ns = 7, l = 20, nl = 3;
  cgx::isect_shorter_first(s, ns, l, nl);
  bool ok = s == 20 && ns == 3 && l == 10 && nl == 7;
  cgx::isect_shorter_first(s, ns, l, nl);
  ok = ok && s == 20 && ns == 3 && l == 10 && nl == 7;
  if (!ok) std::printf("FAIL isect_shorter_first\n");
  return ok ? 0 : 1;
}

static int seg_len()
{
  long bad = 0, checked = 0;
  auto check = [&](long long ns) {
    if (ns < 1 || ns > (1LL << 40)) return;
    long long const len = cgx::sim_seg_len(ns);
    ++checked;
    if (len < cgx::kSimSegLen || (ns + len - 1) / len > (1LL << 14) + 1) {
      ++bad;
      std::printf("FAIL sim_seg_len(%lld) = %lld\n", ns, len);
    }
  };
  for (long long ns = 1; ns <= (1LL << 23); ++ns) check(ns);  // every length up to twice 2^14 * 256
  for (int b = 23; b <= 40; ++b)
    for (long long d = -70000; d <= 70000; ++d) check((1LL << b) + d);
  for (long long ns = 1LL << 23; ns <= (1LL << 40); ns += 999983LL * 131) check(ns);
  std::printf("sim_seg_len: %ld lengths, %ld bad\n", checked, bad);
  return bad ? 1 : 0;
}

int main()
{
  int bad = 0;
  bad += rows<int32_t>("int32", 0);
  bad += rows<int32_t>("int32 near max", INT32_MAX - 4096);
  bad += rows<int64_t>("int64", (int64_t)1 << 33);
  bad += shorter_first();
  bad += seg_len();
  std::printf(bad ? "FAIL intersect\n" : "PASS intersect\n");
  return bad ? 1 : 0;
}
