// The loader's keyed permutation of [0, N): the one definition of mix64, LoaderPerm and loader_index, shared by
// loader.hip (one key set per epoch, made on the host) and group_eval.hip (one key set per group, made on the device).
// The definition stands in loader.hip's header comment; tests/loader_numpy.py restates it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct LoaderPerm {
  uint64_t key[4];
  uint64_t n;
  int32_t half;
  int32_t shuffle;
};

__host__ __device__ __forceinline__ LoaderPerm make_perm(int64_t n, uint64_t seed, int64_t epoch, int shuffle) {
  LoaderPerm pm;
  for (int r = 0; r < 4; ++r) pm.key[r] = mix64(seed ^ mix64((uint64_t)epoch * 0x100000001B3ull + (uint64_t)r));
  int bits = 2;
  while (bits < 62 && (1ull << bits) < (uint64_t)n) bits += 2;
  pm.n = (uint64_t)n;
  pm.half = bits / 2;
  pm.shuffle = shuffle;
  return pm;
}

__device__ __forceinline__ int64_t loader_index(const LoaderPerm& pm, int64_t p) {
  if (!pm.shuffle) return p;
  const uint64_t mask = (1ull << pm.half) - 1;
  uint64_t x = (uint64_t)p;
  do {
    uint64_t l = x >> pm.half, r = x & mask;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint64_t t = l ^ ((mix64(pm.key[k] ^ r) >> 32) & mask);
      l = r;
      r = t;
    }
    x = (l << pm.half) | r;
  } while (x >= pm.n);
  return (int64_t)x;
}

}  // namespace
