// The normal generator of sample_posterior, for the device (sample_normals_kernel, kernels_sample.hip) and for a host compiler
// (tests/c/philox_check.cpp), as exp_dev.h is.  Counter-based: value j of draw s of stream e under a 64-bit seed is a function of
// (seed, e, s, j) alone, so how the work is cut into passes, chunks and workgroups changes no bit.
//   block function   Philox4x32-10 (Salmon et al., SC'11; Random123): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85
//   key              (seed & 0xffffffff, seed >> 32)
//   counter          (p, s, e, 0), p = j >> 1: one block gives the pair of points 2p, 2p + 1
//   uniforms         u1 = ((x0 >> 5) 2^26 + (x1 >> 6) + 1) 2^-53 in (0, 1],  u2 = ((x2 >> 5) 2^26 + (x3 >> 6)) 2^-53 in [0, 1)   (53 bits each)
//   Box-Muller       r = sqrt(-2 ln u1),  z[2p] = r cos(2 pi u2),  z[2p + 1] = r sin(2 pi u2);  |z| <= sqrt(106 ln 2) = 8.57
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MOGP_PHILOX_FN __host__ __device__ inline
#else
#define MOGP_PHILOX_FN inline
#endif

namespace mogp {

struct PhiloxWords {
  uint32_t x[4];
};

MOGP_PHILOX_FN PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return PhiloxWords{{c0, c1, c2, c3}};
}

// the two uniforms of a block
MOGP_PHILOX_FN void philox_uniforms(const PhiloxWords& w, double& u1, double& u2) {
  const double two26 = 67108864.0, twom53 = 1.1102230246251565404236316680908203125e-16;
  u1 = ((double)(w.x[0] >> 5) * two26 + (double)(w.x[1] >> 6) + 1.0) * twom53;
  u2 = ((double)(w.x[2] >> 5) * two26 + (double)(w.x[3] >> 6)) * twom53;
}

// the normals of the points 2p and 2p + 1 of draw s of stream `stream`
MOGP_PHILOX_FN void philox_normal_pair(unsigned long long seed, uint32_t stream, uint32_t s, uint32_t p, double& z0, double& z1) {
  const PhiloxWords w = philox4x32_10(p, s, stream, 0u, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
  double u1, u2;
  philox_uniforms(w, u1, u2);
  const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586476925286766559 * u2;
#if defined(__HIP_DEVICE_COMPILE__)
  double sn, cs;
  sincos(a, &sn, &cs);
  z0 = r * cs;
  z1 = r * sn;
#else
  z0 = r * cos(a);
  z1 = r * sin(a);
#endif
}

}  // namespace mogp
