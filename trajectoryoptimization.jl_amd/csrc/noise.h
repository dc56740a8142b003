// noise.h — counter-based standard normals for the stochastic policy rollout (to_policy_rollout_mc, k_policy.h).
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) keyed by the caller's seed and
// counted by WHAT is drawn, not by where it is computed:
//   key      (seed lo, seed hi)
//   counter  (global trajectory, global sample, k, kind * 256 + j)      k: 0-based step, kind 0 = process noise w, 1 = measurement
//                                                                        noise v, j: index of the pair of normals within the knot
// One call gives r0..r3; u1 = (((r1 << 32 | r0) >> 11) + 0.5) 2^-53, u2 likewise from (r2, r3): both in (0, 1), never 0 or 1.
// Box-Muller: z[2j] = sqrt(-2 ln u1) cos(2 pi u2), z[2j+1] = sqrt(-2 ln u1) sin(2 pi u2); |z| <= sqrt(2 * 54 ln 2) = 8.66.
// A draw therefore does not depend on the lane map, the chunking of the download or how a batch is sharded over handles, and costs
// no memory traffic.  Plain C++ (32 x 32 -> 64 multiplies, no builtins): the same text compiles for the host
// (tests/host_shim/policy_noise_harness.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace to {

__host__ __device__ __forceinline__ void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// 53 bits of (hi, lo), centred in their cell: (0, 1) open at both ends
__host__ __device__ __forceinline__ double philox_uniform(uint32_t lo, uint32_t hi) {
  const uint64_t v = ((uint64_t)hi << 32 | lo) >> 11;
  return ((double)v + 0.5) * 0x1p-53;
}

__host__ __device__ __forceinline__ void uniform_pair(uint64_t seed, uint32_t traj, uint32_t sample, uint32_t k, uint32_t kind, uint32_t j,
                                                      double* u1, double* u2) {
  const uint32_t ctr[4] = {traj, sample, k, kind * 256u + j}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
  uint32_t r[4];
  philox4x32_10(ctr, key, r);
  *u1 = philox_uniform(r[0], r[1]);
  *u2 = philox_uniform(r[2], r[3]);
}

// the j-th pair of standard normals that sample (traj, sample) draws at step k for noise kind `kind`
__host__ __device__ __forceinline__ void normal_pair(uint64_t seed, uint32_t traj, uint32_t sample, uint32_t k, uint32_t kind, uint32_t j,
                                                     double* z0, double* z1) {
  double u1, u2;
  uniform_pair(seed, traj, sample, k, kind, j, &u1, &u2);
  const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
  *z0 = r * cos(a);
  *z1 = r * sin(a);
}

}  // namespace to
