// The near-far threshold step of SSSP (sssp.hip k_sssp_ctl, mg_sssp.hip): plain C++
// that a host-only program can include (tests/c/sssp_threshold_test.cpp).
#pragma once

#if defined(__HIPCC__)
#define CGX_HD __host__ __device__
#else
#define CGX_HD
#endif

namespace cgx {

// the next representable value above a non-negative finite x (max -> inf): the bit
// pattern plus one
CGX_HD inline float next_above(float x)
{
  unsigned int b;
  __builtin_memcpy(&b, &x, sizeof b);
  b += 1u;
  __builtin_memcpy(&x, &b, sizeof b);
  return x;
}
CGX_HD inline double next_above(double x)
{
  unsigned long long b;
  __builtin_memcpy(&b, &x, sizeof b);
  b += 1ull;
  __builtin_memcpy(&x, &b, sizeof b);
  return x;
}

// The threshold after `old` when the far set's smallest distance is mf (old <= mf,
// both non-negative and finite, delta > 0): old + delta when that is past mf (the
// next bucket, as the reference steps), else mf + delta (the empty buckets between
// skipped).  Always > mf and > old, so a far split moves at least the vertices at mf:
// where delta is absorbed by rounding (mf + delta == mf, mf / delta >= 2^25 in fp32)
// the step is one ulp of mf.
template <typename W>
CGX_HD inline W next_threshold(W old, W delta, W mf)
{
  W thr = old + delta;
  if (mf < thr) return thr;
  thr        = mf + delta;
  W const up = next_above(mf);
  return thr < up ? up : thr;
}

}  // namespace cgx
