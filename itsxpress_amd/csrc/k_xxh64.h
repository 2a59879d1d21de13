// k_xxh64.h -- XXH64 over a stream of 32-bit key words (device code).  The routine k_derep.hip has always hashed with, shared with
// k_ftable.hip: both units compile the same statements, and tests/test_gpu_parity.py holds them to the xxhash module's digests.
// get(j) is word j of the key; the digest is XXH64 of the words' little-endian bytes.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace itsx {

static constexpr uint64_t XP1 = 11400714785074694791ULL, XP2 = 14029467366897019727ULL,
                          XP3 = 1609587929392839161ULL, XP4 = 9650029242287828579ULL,
                          XP5 = 2870177450012600261ULL;
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ uint64_t xround(uint64_t acc, uint64_t in) { acc += in * XP2; acc = rotl64(acc, 31); return acc * XP1; }
__device__ __forceinline__ uint64_t xmerge(uint64_t acc, uint64_t v) { acc ^= xround(0, v); return acc * XP1 + XP4; }

template <class F>
__device__ __forceinline__ uint64_t xxh64_words(const F &get, int n, uint64_t seed)
{
  uint64_t h;
  int j = 0;
  auto get64 = [&](int i) { return (uint64_t)get(i) | ((uint64_t)get(i + 1) << 32); };
  if (n >= 8) {
    uint64_t v1 = seed + XP1 + XP2, v2 = seed + XP2, v3 = seed, v4 = seed - XP1;
    do {
      v1 = xround(v1, get64(j)); v2 = xround(v2, get64(j + 2));
      v3 = xround(v3, get64(j + 4)); v4 = xround(v4, get64(j + 6));
      j += 8;
    } while (j + 8 <= n);
    h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
    h = xmerge(h, v1); h = xmerge(h, v2); h = xmerge(h, v3); h = xmerge(h, v4);
  } else {
    h = seed + XP5;
  }
  h += (uint64_t)n * 4ull;
  while (j + 2 <= n) { h ^= xround(0, get64(j)); h = rotl64(h, 27) * XP1 + XP4; j += 2; }
  if (j < n) { h ^= (uint64_t)get(j) * XP1; h = rotl64(h, 23) * XP2 + XP3; }
  h ^= h >> 33; h *= XP2; h ^= h >> 29; h *= XP3; h ^= h >> 32;
  return h;
}

}  // namespace itsx
