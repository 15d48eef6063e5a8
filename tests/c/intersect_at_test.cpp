/*
 * The position-reporting forms of csrc/intersect.hpp on the host: isect_merge_at (the thread tier of
 * the k-truss peel) and isect_probe_at (one lane of its wave tiers).  Rows are sorted and repeat ids,
 * in int32 and int64, with every pair of lengths from {0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024,
 * 1025}.  Against a brute-force model (every distinct common id with the positions of its first copy
 * in both rows):
 *   - the merge reports exactly the model's (x, i, j), in ascending order, and returns their number;
 *   - the probe summed over lanes 0..63 reports the same triples (as a set: lanes interleave);
 *   - the probe summed over a partition of S into [s0, s1) segments reports them too, each once, also
 *     when a cut falls inside a run of equal ids (the first copy then lies before s0);
 *   - the counts equal isect_merge's and isect_probe's, the forms triangle counting and similarity use.
 */
#include "intersect.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <tuple>
#include <vector>

static unsigned long long rng_state = 7;
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
using triple = std::tuple<V, long long, long long>;

template <typename V>
struct collect {
  std::vector<triple<V>>* out;
  void operator()(V x, long long i, long long j) const { out->push_back(triple<V>{x, i, j}); }
};

// every distinct common id with the first position of it in A and in B, by exhaustive search
template <typename V>
static std::vector<triple<V>> model(std::vector<V> const& A, std::vector<V> const& B)
{
  std::vector<triple<V>> out;
  for (size_t i = 0; i < A.size(); ++i) {
    if (i && A[i - 1] == A[i]) continue;
    for (size_t j = 0; j < B.size(); ++j)
      if (B[j] == A[i]) {
        out.push_back(triple<V>{A[i], (long long)i, (long long)j});
        break;
      }
  }
  return out;
}

// the probe of entries [s0, s1) by a whole wave
template <typename V>
static cgx::count_t wave_probe(std::vector<V> const& S, long long s0, long long s1, std::vector<V> const& L,
                               std::vector<triple<V>>* hits)
{
  cgx::count_t c = 0;
  for (int lane = 0; lane < 64; ++lane)
    c += cgx::isect_probe_at<V>(S.data(), s0, s1, L.data(), (long long)L.size(), lane, collect<V>{hits});
  return c;
}

// the probe over the segments that `cuts` (ascending, within [0, ns]) make of S; the triples sorted
template <typename V>
static std::vector<triple<V>> probe_cut(std::vector<V> const& S, std::vector<V> const& L, std::vector<long long> cuts,
                                        cgx::count_t* count)
{
  cuts.push_back((long long)S.size());
  std::vector<triple<V>> hits;
  long long s0 = 0;
  *count       = 0;
  for (long long s1 : cuts) {
    *count += wave_probe<V>(S, s0, s1, L, &hits);
    s0 = s1;
  }
  std::sort(hits.begin(), hits.end());
  return hits;
}

template <typename V>
static int rows(char const* name, V base)
{
  int const lens[] = {0, 1, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025};
  long checked = 0, bad = 0, inside_run = 0, repeats_hit = 0;
  for (int na : lens)
    for (int nb : lens) {
      std::vector<V> const A = make_row<V>(na, base), B = make_row<V>(nb, base);
      std::vector<triple<V>> const want = model<V>(A, B);
      for (auto const& t : want) {
        size_t const i = (size_t)std::get<1>(t), j = (size_t)std::get<2>(t);
        if ((i + 1 < A.size() && A[i + 1] == A[i]) || (j + 1 < B.size() && B[j + 1] == B[j])) ++repeats_hit;
      }

      std::vector<triple<V>> merged;
      cgx::count_t const cm =
        cgx::isect_merge_at<V>(A.data(), (long long)na, B.data(), (long long)nb, collect<V>{&merged});
      bool ok = cm == want.size() && merged == want;  // the model ascends, so does the merge
      ok = ok && cgx::isect_merge<V>(A.data(), (long long)na, B.data(), (long long)nb, cgx::isect_ignore{}) == cm;

      cgx::count_t cp = 0;
      ok = ok && probe_cut<V>(A, B, {}, &cp) == want && cp == cm;
      {
        cgx::count_t plain = 0;
        for (int lane = 0; lane < 64; ++lane)
          plain += cgx::isect_probe<V>(A.data(), 0, na, B.data(), (long long)nb, lane, cgx::isect_ignore{});
        ok = ok && plain == cm;
      }
      // partitions of S = A: single entries, 7 and 256 entries per segment, and every cut inside a run
      for (long long len : {1LL, 7LL, 256LL}) {
        std::vector<long long> cuts;
        for (long long c = len; c < na; c += len) cuts.push_back(c);
        ok = ok && probe_cut<V>(A, B, cuts, &cp) == want && cp == cm;
      }
      std::vector<long long> run_cuts;
      for (long long i = 1; i < na; ++i)
        if (A[(size_t)i - 1] == A[(size_t)i]) run_cuts.push_back(i);
      inside_run += (long)run_cuts.size();
      ok = ok && probe_cut<V>(A, B, run_cuts, &cp) == want && cp == cm;
      if (!run_cuts.empty()) ok = ok && probe_cut<V>(A, B, {run_cuts[run_cuts.size() / 2]}, &cp) == want && cp == cm;

      ++checked;
      if (!ok) {
        ++bad;
        std::printf("FAIL %s na %d nb %d: merge %llu probe %llu want %zu\n", name, na, nb, cm, cp, want.size());
      }
    }
  std::printf("%s: %ld length pairs, %ld cuts inside a run of equal ids, %ld hits on a repeated id, %ld bad\n", name,
              checked, inside_run, repeats_hit, bad);
  return bad || !inside_run || !repeats_hit ? 1 : 0;
}

int main()
{
  int bad = 0;
  bad += rows<int32_t>("int32", 0);
  bad += rows<int32_t>("int32 near max", INT32_MAX - 4096);
  bad += rows<int64_t>("int64", (int64_t)1 << 33);
  std::printf(bad ? "FAIL intersect_at\n" : "PASS intersect_at\n");
  return bad ? 1 : 0;
}
