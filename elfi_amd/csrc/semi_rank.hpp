// What the two semiparametric likelihoods share (semibsl.hip: semiBSL; wsemibsl.hip: the whitened form): the arguments
// and the launch of the column kernel, the workgroup reductions, and the rank of a value within a column held in LDS.
#pragma once

#include "common.hpp"
#include "special.hpp"
#include "syn_gram.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int SEMI_MAX_N = 16384;   // one column (128 KB) + the reduction buffer in the 160 KB of LDS
constexpr int SEMI_RED = 256;
constexpr int SEMI_STATS = 2 * SL_MAX_M + 8;   // per (group, prefix): eta (64), logpdf (64), the denominator

struct SemiArgs {
  const double* X;          // (G n, m), pitch ldx
  int64_t n, ldx;
  int m, K, P, MP;
  const double* y;          // (m)
  const int64_t* prefixes;  // (K) ascending, last == n
  const double* penalties;  // (P) or NULL
  double* Q;                // scratch (G K, n, MP): normal scores of the first prefixes[k] rows
  double* stats;            // scratch (G K, SEMI_STATS)
  double* loglik;           // (G, K, max(P, 1))
  double* u;                // (G, m) or NULL
  double* rho;              // (G, m, m) or NULL
  double* scores;           // (G, n, m) or NULL
};

// The column kernel of semibsl.hip over GK * m workgroups on the context's stream: Q, stats and, if asked for, u and scores.
int semibsl_launch_column(elfihip_ctx* ctx, const SemiArgs& A, int64_t GK);

#if defined(__HIPCC__)
// The sum / the maximum over the workgroup of one value per thread, in a fixed tree; every thread gets it.
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = SEMI_RED / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ double block_max(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = SEMI_RED / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = fmax(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}

// The normal score Phi^-1(r / np1) of xi within the pp values at col2 (pp a multiple of 4; NaN padding counts in no
// comparison): r = #{x_t < xi} + (#{x_t = xi} + 1) / 2, the 1-based rank with ties at the average rank, by counting --
// every lane reads the same x_t (a broadcast), nothing is sorted.
__device__ __forceinline__ double rank_score(const double2* col2, int pp, double xi, double np1) {
  int lt = 0, eq = 0;
  for (int t = 0; t < pp / 2; t += 2) {
    const double2 a = col2[t], b = col2[t + 1];
    lt += (a.x < xi) + (a.y < xi) + (b.x < xi) + (b.y < xi);
    eq += (a.x == xi) + (a.y == xi) + (b.x == xi) + (b.y == xi);
  }
  const double r = (double)lt + 0.5 * (double)(eq + 1);
  return norm_ppf(r / np1);
}
#endif

}  // namespace elfihip
