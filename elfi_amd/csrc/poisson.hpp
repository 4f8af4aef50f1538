// Counter-based Poisson variates on the device: poisson_draw(lam, seed, stream, e) is a deterministic function of lam and
// the words of the library's generator (philox.hpp), so element e is the same number wherever it is drawn -- by
// elfihip_poisson_dev into memory or inside a fused example kernel (series.hip: Ricker).  tests/ricker_ref.py states the
// same rule in NumPy.
//
// Attempt j = 0, 1, ... of element e reads Philox counter e of stream (seed, stream + j): u1 = word53(r0, r1) 2^-53
// and u2 the same of words 2, 3, both in [0, 1) (philox.hpp: uniform53_pair).
//   lam NaN, lam < 0, lam > 2^53   NaN (NumPy's RandomState.poisson raises ValueError for the whole batch instead)
//   lam == 0                       0, no draw
//   0 < lam < 10                   inversion on u1 of attempt 0: p = F = exp(-lam), k = 0; while u1 > F: k += 1, p = p (lam /
//                                  k), F = F + p.  F saturates just below 1, so a u1 above the saturated F would never end
//                                  the loop: it stops at k = ELFIHIP_POISSON_MAX_K, 37 standard deviations out at lam = 10.
//   lam >= 10                      Hoermann's PTRS (transformed rejection with squeeze; the algorithm of NumPy's legacy
//                                  poisson), one attempt per stream.  An attempt rejects with probability 0.25 at lam =
//                                  10 and below 0.14 at large lam, so all ELFIHIP_POISSON_MAX_ATTEMPTS rejecting has
//                                  probability below 1e-38 (1e-50 at large lam); floor(lam) is returned then.  That bound
//                                  exists ONLY so that the loop is finite -- no kernel here may spin.
// Every expression keeps the operation order written here, FMA contraction off.
#pragma once

#include <cmath>

#include "../../include/elfihip.h"
#include "philox.hpp"

namespace elfihip {

// (forced inline: as a call its registers are added to the caller's, which halves the Ricker kernel's wavefronts per SIMD)
__device__ __forceinline__ double poisson_draw(double lam, uint64_t seed, uint64_t stream, uint64_t e) {
#pragma clang fp contract(off)
  if (!(lam >= 0.0) || lam > 0x1.0p53) return __builtin_nan("");
  if (lam == 0.0) return 0.0;
  double u1, u2;
  if (lam < 10.0) {
    uniform53_pair(seed, stream, (uint32_t)e, (uint32_t)(e >> 32), u1, u2);
    double p = exp(-lam), F = p;
    int k = 0;
    while (u1 > F && k < ELFIHIP_POISSON_MAX_K) {
      ++k;
      p = p * (lam / (double)k);
      F = F + p;
    }
    return (double)k;
  }
  const double slam = sqrt(lam), loglam = log(lam);
  const double b = 0.931 + 2.53 * slam;
  const double a = -0.059 + 0.02483 * b;
  const double invalpha = 1.1239 + 1.1328 / (b - 3.4);
  const double vr = 0.9277 - 3.6224 / (b - 2.0);
  for (int j = 0; j < ELFIHIP_POISSON_MAX_ATTEMPTS; ++j) {
    uniform53_pair(seed, stream + (uint64_t)j, (uint32_t)e, (uint32_t)(e >> 32), u1, u2);
    const double U = u1 - 0.5, V = u2, us = 0.5 - fabs(U);
    const double k = floor((((2.0 * a) / us + b) * U + lam) + 0.43);
    if (us >= 0.07 && V <= vr) return k;
    if (k < 0.0 || (us < 0.013 && V > us)) continue;
    const double lhs = (log(V) + log(invalpha)) - log(a / (us * us) + b);
    const double rhs = (-lam + k * loglam) - lgamma(k + 1.0);
    if (lhs <= rhs) return k;
  }
  return floor(lam);
}

}  // namespace elfihip
