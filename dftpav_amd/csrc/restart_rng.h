// restart_rng.h -- the generator of the seeded restart sampler (its definition is stated in full in restart.hip): shared by
// restart.hip and plan.hip so that a (seed, hypothesis, restart) gives the same bits in both.
#pragma once
#include <hip/hip_runtime.h>

namespace dftpav {

__host__ __device__ inline unsigned long long splitmix64(unsigned long long s0, unsigned long long k) {
  unsigned long long z = s0 + k * 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
__host__ __device__ inline double u01(unsigned long long s0, unsigned long long k) {
  return ((double)(splitmix64(s0, k) >> 11) + 0.5) * 1.1102230246251565e-16; // 2^-53
}

// the SplitMix64 stream of (hypothesis, restart)
__host__ __device__ inline unsigned long long restart_stream(unsigned long long seed, int hyp, int r) {
  return splitmix64(seed, 1ull + (unsigned long long)hyp * 65536ull + (unsigned long long)r);
}

} // namespace dftpav
