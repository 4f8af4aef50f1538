// What the two Gaussian synthetic likelihoods share (synlik.hip: m <= 64; synlik_wide.hip: 65 to 256 summaries): the
// whitening launch in front of both, rows -> rows W^T and y -> W y, one kernel for every m (each translation unit gets its
// own copy), and the constant of the unbiased estimator.
#pragma once

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace elfihip {

// rows -> rows W^T (sequential k), one output element per thread and step
static __global__ __launch_bounds__(256) void synlik_whiten_kernel(const double* X, int64_t rows, int m, int64_t ldx,
                                                                   const double* W, const double* y, double* Xw, double* yw) {
  const int64_t total = rows * m;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / m;
    const int j = (int)(e - r * m);
    const double* x = X + r * ldx;
    const double* w = W + (int64_t)j * m;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += x[k] * w[k];
    Xw[e] = s;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < m) {
    const double* w = W + (int64_t)threadIdx.x * m;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += w[k] * y[k];
    yw[threadIdx.x] = s;
  }
}

// log c(d, n - 2) - log c(d, n - 1) - d/2 log(1 - 1/n) - d/2 log(2 pi) of Ghurye & Olkin's unbiased estimator
// (pdf_methods.py:168-171, wcon :319-341); NaN where a gamma function's argument is not positive (n <= d + 1)
inline double unbiased_const(int d, int64_t n) {
  if (n <= (int64_t)d + 1) return NAN;
  long double a = 0.5L * d * logl(2.0L);
  for (int x = 0; x < d; ++x) a -= lgammal(0.5L * (long double)(n - 2 - x)) - lgammal(0.5L * (long double)(n - 1 - x));
  a -= 0.5L * d * logl(1.0L - 1.0L / (long double)n);
  a -= 0.5L * d * logl(2.0L * 3.14159265358979323846264338327950288L);
  return (double)a;
}

}  // namespace elfihip
