/*
 * The SSSP threshold step on the host (csrc/sssp_threshold.hpp, the function
 * k_sssp_ctl and the multi-GPU loop call): for old <= mf and delta > 0, over fp32 and
 * fp64 values that include mf / delta = 2^23, 2^24, 2^25, 2^40 (delta absorbed by
 * rounding), denormal deltas and mf next to the type's max:
 *   - thr > mf and thr > old (the far split that follows moves at least the vertices
 *     at mf: the loop of buckets always advances);
 *   - thr == old + delta whenever that already exceeds mf (the buckets of every
 *     input that never met the absorbed case are what they were).
 */
#include "sssp_threshold.hpp"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

template <typename W>
static int sweep(char const* name)
{
  using L     = std::numeric_limits<W>;
  W const max = L::max();
  std::vector<W> mfs = {W(0), L::denorm_min(), L::min(), W(1e-20), W(0.5), W(1), W(1.5), W(3), W(1000.25),
                        W(1 << 23), W(1 << 24), W(1 << 25), std::ldexp(W(1), 40), std::ldexp(W(1), 100),
                        std::nextafter(std::nextafter(max, W(0)), W(0)), std::nextafter(max, W(0))};
  std::vector<W> deltas = {L::denorm_min(), L::denorm_min() * W(7), L::min(), W(1e-30), W(1e-9), W(0.125), W(0.129),
                           W(1), W(64), W(1e6), std::ldexp(W(1), 60)};
  // and, for every mf, the deltas with mf / delta = 2^23, 2^24, 2^25, 2^40
  int const ratios[] = {23, 24, 25, 40};
  long checked = 0, absorbed = 0, bad = 0;
  for (W mf : mfs) {
    std::vector<W> ds = deltas;
    for (int r : ratios)
      if (mf > W(0) && std::ldexp(mf, -r) > W(0)) ds.push_back(std::ldexp(mf, -r));
    // old <= mf: far below, the bucket before mf, one ulp below, equal
    std::vector<W> olds = {W(0), mf / W(2), mf, mf > W(0) ? std::nextafter(mf, W(0)) : W(0)};
    for (W delta : ds) {
      if (mf - delta >= W(0)) olds.push_back(mf - delta);
      if (mf - delta / W(2) >= W(0)) olds.push_back(mf - delta / W(2));
      for (W old : olds) {
        if (!(old <= mf)) continue;
        W const thr  = cgx::next_threshold(old, delta, mf);
        W const step = old + delta;
        ++checked;
        absorbed += mf + delta == mf;
        bool ok = thr > mf && thr > old;
        if (step > mf) ok = ok && thr == step;
        if (!ok) {
          ++bad;
          std::printf("FAIL %s: old %.17g delta %.17g mf %.17g -> thr %.17g (old + delta %.17g)\n", name, (double)old,
                      (double)delta, (double)mf, (double)thr, (double)step);
        }
      }
    }
  }
  std::printf("%s: %ld cases, %ld with mf + delta == mf, %ld failed\n", name, checked, absorbed, bad);
  return bad != 0 || absorbed == 0;
}

int main()
{
  int rc = sweep<float>("fp32");
  rc |= sweep<double>("fp64");
  if (rc == 0) std::printf("PASS threshold\n");
  return rc;
}
