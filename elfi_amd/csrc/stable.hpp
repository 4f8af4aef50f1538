// Symmetric (beta = 0) alpha-stable variates on the device, S1 parameterisation: the Chambers-Mallows-Stuck transform as
// SciPy 1.15's levy_stable.rvs evaluates it (scipy/stats/_levy_stable: _rvs_Z1), in SciPy's order of operations, FMA
// contraction off -- so the device differs from NumPy only through tan, sin, cos and pow (and log, in the exponential
// variate).  tests/toad_ref.py states the same rule in NumPy beside a first-order error bound.
//
//   stable_transform(alpha, scale, TH, W), TH in (-pi/2, pi/2) an angle, W > 0 a standard exponential:
//     alpha NaN or outside (0, 2], scale NaN or negative      NaN for that element
//     alpha == 1      ((2 / pi) ((pi / 2) tan TH)) scale      SciPy's alpha1func at beta = 0, its constants as doubles
//     otherwise       aTH = alpha TH
//                     Z = (W / (cos TH / tan aTH + sin TH)) ((cos aTH + sin aTH tan TH) / W) ^ (1 / alpha)
//                     the variate is Z scale
//   stable_draw(alpha, scale, seed, stream, e) reads Philox counter e of stream (seed, stream):
//     TH = u1 pi + (-pi / 2), u1 = word53(r0, r1) 2^-53 in [0, 1)                        (SciPy: uniform.rvs(loc, scale))
//     W  = -log(u2),          u2 = (word53(r2, r3) + 1) 2^-53 in (0, 1]                  (philox.hpp: unit_co, unit_exponential)
//   so element e is the same number wherever it is drawn: by elfihip_stable_dev into memory or inside toad.hip.
// The skewed law and the S0 parameterisation are stable_general below (the stochastic-volatility example, sv.hip, uses them).
#pragma once

#include <cmath>

#include "philox.hpp"

namespace elfihip {

#define ELFIHIP_PI 3.141592653589793        // np.pi
#define ELFIHIP_HALF_PI 1.5707963267948966  // np.pi / 2
#define ELFIHIP_TWO_BY_PI 0.6366197723675814  // 2 / np.pi

__device__ __forceinline__ bool stable_valid(double alpha, double scale) { return alpha > 0.0 && alpha <= 2.0 && scale >= 0.0; }

__device__ __forceinline__ double stable_transform(double alpha, double scale, double TH, double W) {
#pragma clang fp contract(off)
  if (!stable_valid(alpha, scale)) return __builtin_nan("");
  const double tanTH = tan(TH);
  if (alpha == 1.0) return (ELFIHIP_TWO_BY_PI * (ELFIHIP_HALF_PI * tanTH)) * scale;
  const double aTH = alpha * TH;
  const double cosTH = cos(TH);
  const double den = cosTH / tan(aTH) + sin(TH);
  const double num = cos(aTH) + sin(aTH) * tanTH;
  const double Z = (W / den) * pow(num / W, 1.0 / alpha);
  return Z * scale;
}

// the angle and the exponential of Philox counter e of stream (seed, stream)
__device__ __forceinline__ void stable_angle_expo(uint64_t seed, uint64_t stream, uint64_t e, double& TH, double& W) {
#pragma clang fp contract(off)
  uint64_t a, b;
  words53(seed, stream, e, a, b);
  const double u1 = unit_co(a), u2 = unit_oc(b);
  TH = u1 * ELFIHIP_PI + (-ELFIHIP_HALF_PI);
  W = -log(u2);
}

__device__ __forceinline__ double stable_draw(double alpha, double scale, uint64_t seed, uint64_t stream, uint64_t e) {
  double TH, W;
  stable_angle_expo(seed, stream, e, TH, W);
  return stable_transform(alpha, scale, TH, W);
}

// ---- the general law: beta in [-1, 1], a location, S1 or S0 -----------------------------------------------------------------
// SciPy 1.15's levy_stable.rvs(alpha, beta, loc, scale) per element, in SciPy's order of operations (tests/sv_ref.py states
// the same rule in NumPy beside a first-order error bound):
//   stable_z1(alpha, beta, TH, W), _rvs_Z1:
//     alpha == 1   (2 / pi) ((pi / 2 + beta TH) tan TH - beta log(((pi / 2) W cos TH) / (pi / 2 + beta TH)))       alpha1func
//     beta == 0    stable_transform(alpha, 1, TH, W): the symmetric expression above, one and the same              beta0func
//     otherwise    val0 = beta tan(pi alpha / 2), th0 = atan(val0) / alpha,                                         otherwise
//                  val3 = W / (cos TH / tan(alpha (th0 + TH)) + sin TH),
//                  val3 (((cos aTH + sin aTH tan TH) - val0 (sin aTH - cos aTH tan TH)) / W) ^ (1 / alpha)
//   stable_general(alpha, beta, loc, scale, s0, TH, W):
//     alpha NaN or outside (0, 2], beta NaN or outside [-1, 1], scale NaN or negative      NaN for that element
//     X1 = Z scale + loc                                                                    rv_continuous.rvs
//     alpha == 1:  X1 = X1 + (((2 beta) scale) log(scale)) / pi                             levy_stable.rvs, the S1 shift
//     s0:          X1 - ((((beta 2) scale) log(scale)) / pi) at alpha == 1,                 ... and the shift to S0
//                  X1 - (scale beta) tan((pi alpha) / 2) elsewhere
//   so scale == 0 at alpha == 1 is 0 log 0 = NaN, as in SciPy.  SciPy raises for the whole call where a parameter is
//   invalid; here that element alone is NaN.
__device__ __forceinline__ bool stable_valid_general(double alpha, double beta, double scale) {
  return alpha > 0.0 && alpha <= 2.0 && beta >= -1.0 && beta <= 1.0 && scale >= 0.0;
}

__device__ __forceinline__ double stable_z1(double alpha, double beta, double TH, double W) {
#pragma clang fp contract(off)
  if (alpha == 1.0) {
    const double s = ELFIHIP_HALF_PI + beta * TH;
    return ELFIHIP_TWO_BY_PI * (s * tan(TH) - beta * log(((ELFIHIP_HALF_PI * W) * cos(TH)) / s));
  }
  if (beta == 0.0) return stable_transform(alpha, 1.0, TH, W);
  const double val0 = beta * tan((ELFIHIP_PI * alpha) / 2.0);
  const double th0 = atan(val0) / alpha;
  const double cosTH = cos(TH), tanTH = tan(TH);
  const double val3 = W / (cosTH / tan(alpha * (th0 + TH)) + sin(TH));
  const double aTH = alpha * TH;
  const double ca = cos(aTH), sa = sin(aTH);
  return val3 * pow(((ca + sa * tanTH) - val0 * (sa - ca * tanTH)) / W, 1.0 / alpha);
}

__device__ __forceinline__ double stable_general(double alpha, double beta, double loc, double scale, bool s0, double TH,
                                                 double W) {
#pragma clang fp contract(off)
  if (!stable_valid_general(alpha, beta, scale)) return __builtin_nan("");
  double x = stable_z1(alpha, beta, TH, W) * scale + loc;
  if (alpha == 1.0) {
    const double lg = log(scale);
    x = x + (((2.0 * beta) * scale) * lg) / ELFIHIP_PI;
    if (s0) x = x - ((((beta * 2.0) * scale) * lg) / ELFIHIP_PI);
  } else if (s0) {
    x = x - (scale * beta) * tan((ELFIHIP_PI * alpha) / 2.0);
  }
  return x;
}

}  // namespace elfihip
