// NumPy's summation order on the device (summaries.hip's row statistics, dist_metrics.hpp's correlation mean).
//
// np.add.reduce along a contiguous axis is a pairwise sum: fewer than 8 terms in order; 8 .. 128 terms by eight
// interleaved accumulators over stride 8, combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the tail in order; more than
// 128 terms split at n/2 - (n/2 mod 8) and both halves summed the same way.  The reduction hands that sum at most one
// buffer of its iterator at a time (np.getbufsize(), 8192 elements by default), so an axis longer than that is summed
// piece by piece, the pieces added to the result in order (np_pairwise_row).  With FMA contraction off the results are
// BIT-IDENTICAL to NumPy.
#pragma once

namespace elfihip {

// One block of at most 128 terms: f(i) yields element i of a[lo .. lo + n).
template <class F>
__device__ __forceinline__ double np_pairwise_block(F f, int lo, int n) {
#pragma clang fp contract(off)
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += f(lo + i);
    return r;
  }
  double r[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = f(lo + j);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] += f(lo + i + j);
  }
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += f(lo + i);
  return res;
}

// NumPy's pairwise_sum over a[lo .. lo + n), any n (recursive above 128 terms).
template <class F>
__device__ double np_pairwise(F f, int lo, int n) {
#pragma clang fp contract(off)
  if (n <= 128) return np_pairwise_block(f, lo, n);
  int n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise(f, lo, n2) + np_pairwise(f, lo + n2, n - n2);
}

// np.add.reduce over a whole row of n terms: pieces of NumPy's default buffer size, each summed pairwise, added in order.
constexpr int NP_BUFSIZE = 8192;

template <class F>
__device__ double np_pairwise_row(F f, int n) {
#pragma clang fp contract(off)
  double r = np_pairwise(f, 0, n < NP_BUFSIZE ? n : NP_BUFSIZE);
  for (int lo = NP_BUFSIZE; lo < n; lo += NP_BUFSIZE) r += np_pairwise(f, lo, n - lo < NP_BUFSIZE ? n - lo : NP_BUFSIZE);
  return r;
}

// The same sum with at most D splits, inlined (no call, no stack): exact for every n whose split tree is at most D deep
// -- D = 2 covers n <= 299, the widest row of the tile kernels.  A piece still above 128 terms at depth D is summed
// in order (not NumPy's order; callers only reach it beyond the exact range they document).
template <int D, class F>
__device__ __forceinline__ double np_pairwise_bounded(F f, int lo, int n) {
#pragma clang fp contract(off)
  if (n <= 128) return np_pairwise_block(f, lo, n);
  if constexpr (D == 0) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += f(lo + i);
    return r;
  } else {
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_bounded<D - 1>(f, lo, n2) + np_pairwise_bounded<D - 1>(f, lo + n2, n - n2);
  }
}

}  // namespace elfihip
