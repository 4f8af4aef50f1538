// One lane sorts one short row in place: the per-row sort of daycare.hip's distance, gnk.hip's columns and series.hip's
// M/G/1 quantiles (rows of a few dozen to a few hundred values in LDS; wg_sort.hpp has the workgroup's sort of long rows).
#pragma once

#include <hip/hip_runtime.h>

namespace elfihip {

// np.sort's order: a NaN is greater than every number
__device__ __forceinline__ bool nan_last_after(double a, double b) { return a > b || (a != a && b == b); }

// Shell sort of y[0 .. m) in place (Knuth's gaps 1, 4, 13, ...): after(a, b) says that a belongs behind b
template <class After>
__device__ __forceinline__ void shell_sort(double* y, int m, After after) {
  int g = 1;
  while (g < m / 3) g = 3 * g + 1;
  for (; g >= 1; g /= 3) {
    for (int i = g; i < m; ++i) {
      const double x = y[i];
      int j = i;
      while (j >= g && after(y[j - g], x)) {
        y[j] = y[j - g];
        j -= g;
      }
      y[j] = x;
    }
  }
}

}  // namespace elfihip
