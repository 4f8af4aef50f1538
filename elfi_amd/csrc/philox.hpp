// Counter-based normals on the device: Philox4x32-10 (Salmon et al., Random123; known answers in tests/test_gauss_gpu.py)
// + Box-Muller in f64.  Normal number e of stream (seed, stream) is the same wherever it is drawn: by
// elfihip_randn_dev into memory, or inside the fused example kernels (gauss.hip, summaries.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace elfihip {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// ---- the draw primitives: every 53-bit uniform and unit exponential of the library is made of these -----------------------
// the 53-bit integer of two 32-bit words: all of `hi` above the top 21 bits of `lo`
__device__ __forceinline__ uint64_t word53(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 21) | (lo >> 11); }

// the two 53-bit integers of Philox counter (c0, c1) of (seed, stream): words 0, 1 and words 2, 3
__device__ __forceinline__ void words53(uint64_t seed, uint64_t stream, uint32_t c0, uint32_t c1, uint64_t& a, uint64_t& b) {
  uint32_t r[4];
  philox4x32_10(c0, c1, (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
  a = word53(r[0], r[1]);
  b = word53(r[2], r[3]);
}
// ... of the 64-bit counter p
__device__ __forceinline__ void words53(uint64_t seed, uint64_t stream, uint64_t p, uint64_t& a, uint64_t& b) {
  words53(seed, stream, (uint32_t)p, (uint32_t)(p >> 32), a, b);
}

// a 53-bit integer as a uniform in [0, 1), and in (0, 1]: a logarithm's argument that is never zero
__device__ __forceinline__ double unit_co(uint64_t x) { return (double)x * 0x1.0p-53; }
__device__ __forceinline__ double unit_oc(uint64_t x) { return (double)(x + 1) * 0x1.0p-53; }
// ... and as a unit exponential
__device__ __forceinline__ double unit_exponential(uint64_t x) { return -log(unit_oc(x)); }

// the two 53-bit uniforms in [0, 1) of Philox counter (c0, c1) of (seed, stream), each converted as soon as it is assembled
// (words53 assembles both first: the same values, but the compiler schedules the callers differently)
__device__ __forceinline__ void uniform53_pair(uint64_t seed, uint64_t stream, uint32_t c0, uint32_t c1, double& u0, double& u1) {
  uint32_t r[4];
  philox4x32_10(c0, c1, (uint32_t)stream, (uint32_t)(stream >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
  u0 = unit_co(word53(r[0], r[1]));
  u1 = unit_co(word53(r[2], r[3]));
}

// the 53-bit uniform in [0, 1) of the first two words of counter idx of stream (seed, stream): what a ROMC region's sample
// (romc.hip) and a slice sampler's draw (slice_gamma.hip) take, one counter each
__device__ __forceinline__ double uniform53_first(uint64_t seed, uint64_t stream, uint64_t idx) {
  uint64_t a, b;
  words53(seed, stream, idx, a, b);
  return unit_co(a);
}

// standard normals number 2p and 2p+1 of stream (seed, stream)
__device__ __forceinline__ void normal_pair(uint64_t seed, uint64_t stream, uint64_t p, double& z0, double& z1) {
  uint64_t a, b;
  words53(seed, stream, p, a, b);
  const double u1 = unit_oc(a), u2 = unit_co(b);
  const double rad = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  z0 = rad * cs;
  z1 = rad * sn;
}

}  // namespace elfihip
