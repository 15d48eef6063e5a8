// The counter-based generator behind R-MAT (rmat.hip), neighbour sampling (sampling.hip) and
// random walks (random_walks.hip).  Nothing here keeps state: a value depends on its arguments
// alone, so a result does not depend on the launch shape, and tests/sampling_ref.py (and
// oracle/rmat.py for R-MAT) restates every function bit for bit in numpy.
//
//   draw(seed, stream, i, j) = sm(sm(sm(seed * 0x9E3779B97F4A7C15 ^ stream) ^ i) ^ j)
//   index(r, n) = high 64 bits of r * n          a position in [0, n)
//   unit(r)     = (r >> 11) * 2^-53              a double in [0, 1)
//
// stream: the hop of a neighbour sample / the step of a walk; i: the slot's position in that
// hop's frontier / the walk's position in the start list; j: the number of the draw in the slot.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace cgx {

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z          = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z          = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// seed * golden ratio, once per kernel
__host__ __device__ __forceinline__ uint64_t sample_seed_key(uint64_t seed) { return seed * 0x9E3779B97F4A7C15ull; }

// draw() with the seed already multiplied (sample_seed_key)
__host__ __device__ __forceinline__ uint64_t sample_draw(uint64_t seed_key, uint64_t stream, uint64_t i, uint64_t j)
{
  return splitmix64(splitmix64(splitmix64(seed_key ^ stream) ^ i) ^ j);
}

__device__ __forceinline__ uint64_t sample_index(uint64_t r, uint64_t n) { return __umul64hi(r, n); }

__host__ __device__ __forceinline__ double sample_unit(uint64_t r)
{
  return (double)(r >> 11) * (1.0 / 9007199254740992.0);
}

}  // namespace cgx
