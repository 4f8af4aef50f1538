// Normal cdf, its inverse and Owen's T function on the device, for the acquisition rules built on the variance of the unnormalised
// approximate posterior (elfi/methods/bo/acquisition.py:392-463, 795-821: MaxVar, RandMaxVar, ExpIntVar).  The reference
// evaluates scipy.stats.skewnorm.cdf there; with z = (x - loc) / scale that is  Phi(z) - 2 T(z, a)  [Owen 1956],
// T(h, a) = (1 / 2 pi) int_0^a exp(-h^2 (1 + x^2) / 2) / (1 + x^2) dx.  Every shape parameter on this path lies in [0, 1]
// (sigma_n / sqrt(sigma_n^2 + 2 v), sqrt((A - d) / (A + d))), so the integral is taken directly: Gauss-Legendre panels
// whose width shrinks with |h| (the integrand falls like exp(-h^2 x^2 / 2)), ten points each, no case analysis.
// Accuracy of this rule, measured in binary64 against 50-digit values (tests/golden/special_fn.npz, written by
// oracle/make_golden_special.py; tests/test_special_reference.py holds a transcription of the loop below to them):
//   absolute:  |T - exact| <= 1.1e-14 for every h and 0 <= a <= 1;  W = Phi(z) Phi(-z) - 2 T(z, b) to 2.1e-14
//   relative:  |h| <= 6: 2.5e-13 (worst just below a panel edge, |h| a = 4/3 with one panel; 1.6e-13 on the test grid)
//              6 < |h| <= 12: 6e-15;  12 < |h| <= 28: 4e-14;  28 < |h| <= 37: 6e-14 (the rounding of h^2 (1 + x^2) / 2
//              near 700 in front of exp);  beyond |h| = 37.5 T is subnormal and only the absolute figure holds
// A first CPU comparison had suggested 8e-8 relative at |h| = 20, a >= 0.9: that was the reference integration's
// setting, not this rule (1.1e-14 relative there).
#pragma once

#include <hip/hip_runtime.h>

namespace elfihip {

__device__ __forceinline__ double norm_cdf(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

__device__ __forceinline__ double norm_pdf(double z) { return 0.39894228040143267794 * exp(-0.5 * z * z); }

// Phi^-1(p): the normal scores of the semiparametric synthetic likelihood (semibsl.hip).  HIP's normcdfinv with the ends
// pinned: norm_ppf(1/2) = +0 exactly (normcdfinv returns -0), norm_ppf(0) = -inf, norm_ppf(1) = +inf, NaN outside [0, 1].
// Accuracy of normcdfinv on gfx950, measured on an MI355X against 50-digit values (sqrt 2 erfinv(2 p - 1) in mpmath):
// relative error <= 3.6e-16 on the rank grids i / (n + 1), n = 5, 257, 1000 (SciPy's ndtri on the same points: 5.1e-16;
// tests/test_semibsl_gpu.py checks the scores against 16 x that figure), 4.2e-16 on the half ranks i / 2002 and on 2000
// uniform p, 3.2e-16 for p = 1e-1 ... 1e-298, 7.3e-17 for p = 1/2 +- k 2^-53.  A Newton step on a residual that keeps its
// relative accuracy (erf about the centre, erfc in the tails) was measured too and gains nothing (4.3e-16): not kept.
__device__ inline double norm_ppf(double p) {
  if (!(p > 0.0)) return p == 0.0 ? -INFINITY : NAN;
  if (!(p < 1.0)) return p == 1.0 ? INFINITY : NAN;
  if (p == 0.5) return 0.0;
  return normcdfinv(p);
}

// T(h, a) for 0 <= a <= 1 (any h)
__device__ inline double owens_t(double h, double a) {
  // 10-point Gauss-Legendre on [-1, 1]: abscissae (positive half) and weights
  const double gx[5] = {0.14887433898163121088, 0.43339539412924719080, 0.67940956829902440623,
                        0.86506336668898451073, 0.97390652851717172008};
  const double gw[5] = {0.29552422471475287017, 0.26926671930999635509, 0.21908636251598204400,
                        0.14945134915058059315, 0.06667134430868813759};
  if (!(a > 0.0)) return 0.0;
  const double ah = fabs(h) * a;
  int panels = 1 + (int)(0.75 * ah);       // panel width <= 4 / (3 |h|): accuracy in the header comment
  if (panels > 96) panels = 96;
  const double w = a / panels, hh = -0.5 * h * h;
  double sum = 0.0;
  for (int p = 0; p < panels; ++p) {
    const double mid = (p + 0.5) * w, half = 0.5 * w;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const double x1 = mid - half * gx[i], x2 = mid + half * gx[i];
      const double q1 = 1.0 + x1 * x1, q2 = 1.0 + x2 * x2;
      s += gw[i] * (exp(hh * q1) / q1 + exp(hh * q2) / q2);
    }
    sum += s * half;
  }
  return sum * 0.15915494309189533577;  // 1 / 2 pi
}

}  // namespace elfihip
