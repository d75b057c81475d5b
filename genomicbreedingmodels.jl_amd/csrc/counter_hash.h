// The project's counter-based hash (the splitmix64 finaliser): the synthetic genotype generator (stats.hip,
// bit-identical to oracle/gbm_oracle.c) and the eigensolver's start block (pcs.hip) draw from it. One definition,
// so that the two cannot drift apart. Include from .hip files (host code may call it too: the ordinal
// sampler's start draws, bayes_ordinal.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gbm {

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

}  // namespace gbm
