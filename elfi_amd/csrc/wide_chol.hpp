// The factorisation the two wide likelihoods share (synlik_wide.hip: the Gaussian one; semibsl_wide.hip: the
// semiparametric one): the shape of a job's slab and the left-looking panel Cholesky of one workgroup on it.
#pragma once

#include "common.hpp"
#include "mfma_f64.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int SW_MIN_M = 65, SW_MAX_M = 256;
constexpr int SW_BLK = 64;             // edge of a block of the moments / the Gram matrix
constexpr int SW_PAN = 32;             // columns of a factorisation panel
constexpr int SW_PP = SW_PAN + 1;      // pitch of the panel in LDS
constexpr int SW_ROW_TILES = 5;        // 16-row tiles of a panel per wave: ceil(ceil(257 / 16) / 4)
constexpr size_t SW_SCRATCH_CAP = (size_t)256 << 20;   // bytes of ctx->scratch one call may hold (half moments, half slabs)

inline int wide_mpad(int m) { return (m + SW_BLK - 1) / SW_BLK * SW_BLK; }
inline int wide_pitch(int m) { return (m + SW_PAN - 1) / SW_PAN * SW_PAN; }
// doubles of one job's slab: rows 0 .. m of the factor
inline size_t wide_slab(int m) { return (size_t)(m + 1) * wide_pitch(m); }
// doubles of LDS the factorisation takes: the panel, the diagonal of the factor and the solved extra row
inline size_t wide_chol_lds(int m) { return (size_t)(m + 1) * SW_PP + 2 * (size_t)wide_mpad(m); }

#if defined(__HIPCC__)
// Left-looking blocked Cholesky factorisation of the m x m matrix entry(i, j <= i) with entry(m, j) as an extra row, whose
// forward solve is the factorisation's update, by one workgroup of 256 threads on the slab L (rows 0 .. m at pitch pw, in
// global memory).  Per 32-column panel: the update sum_k L[i][k] L[j][k] over the panels already factored is accumulated by
// MFMA from the slab (each lane loads four consecutive k of one row, 32 bytes), the panel's own entries are formed in the
// same lane and the difference goes to the LDS panel P ((m + 1, SW_PP)); the 32 x 32 diagonal block is factored there and
// the rows below solved, column by column; the panel is written back once.  The unfactored matrix is never stored: every
// word of the slab is written exactly once.  dg (m) receives the diagonal of the factor, z (m) the solved extra row; both
// are in LDS and visible to every thread on return.  False, for every thread, at the first pivot that is not positive.
template <class Entry>
__device__ __forceinline__ bool wide_panel_chol(double* L, int pw, int m, double* P, double* dg, double* z, const Entry& entry) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int lr = lane >> 4, lc = lane & 15;
  for (int c0 = 0; c0 < m; c0 += SW_PAN) {
    const int nr = m + 1 - c0;                       // rows c0 .. m
    const int nc = m - c0 < SW_PAN ? m - c0 : SW_PAN;
    const int nrt = (nr + 15) / 16;
    // update by the factored panels: acc[t][ct] = sum_{k < c0} L[c0 + 16 rt + .][k] L[c0 + 16 ct + .][k]; rows past m are
    // read from row m and dropped.  A lane's four consecutive k feed four consecutive MFMAs (a permutation of k that both
    // operands share).
    v4d acc[SW_ROW_TILES][2];
#pragma unroll
    for (int t = 0; t < SW_ROW_TILES; ++t) acc[t][0] = acc[t][1] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int rb0 = c0 + lc < m ? c0 + lc : m, rb1 = c0 + 16 + lc < m ? c0 + 16 + lc : m;
    for (int kk = 0; kk < c0; kk += 16) {
      const double4 b0 = *reinterpret_cast<const double4*>(L + (size_t)rb0 * pw + kk + 4 * lr);
      const double4 b1 = *reinterpret_cast<const double4*>(L + (size_t)rb1 * pw + kk + 4 * lr);
#pragma unroll
      for (int t = 0; t < SW_ROW_TILES; ++t) {
        const int rt = wv + 4 * t;
        if (rt < nrt) {
          const int row = c0 + 16 * rt + lc < m ? c0 + 16 * rt + lc : m;
          const double4 a = *reinterpret_cast<const double4*>(L + (size_t)row * pw + kk + 4 * lr);
          acc[t][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b0.x, acc[t][0], 0, 0, 0);
          acc[t][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b0.y, acc[t][0], 0, 0, 0);
          acc[t][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.z, b0.z, acc[t][0], 0, 0, 0);
          acc[t][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.w, b0.w, acc[t][0], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b1.x, acc[t][1], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b1.y, acc[t][1], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.z, b1.z, acc[t][1], 0, 0, 0);
          acc[t][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.w, b1.w, acc[t][1], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < SW_ROW_TILES; ++t) {
      const int rt = wv + 4 * t;
      if (rt < nrt) {
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int pr = 16 * rt + lr + 4 * r, c = 16 * ct + lc;
            if (pr < nr) P[pr * SW_PP + c] = entry(c0 + pr, c0 + c) - acc[t][ct][r];
          }
      }
    }
    __syncthreads();
    // the panel's own columns: right-looking inside the panel, in LDS
    for (int j = 0; j < nc; ++j) {
      const double piv = P[j * SW_PP + j];   // the same word for every thread: the branch is uniform
      if (!(piv > 0.0)) return false;
      const double d = sqrt(piv);            // (nobody writes P[j][j] from here on)
      if (tid == 0) dg[c0 + j] = d;
      for (int r = j + 1 + tid; r < nr; r += 256) P[r * SW_PP + j] = P[r * SW_PP + j] / d;
      __syncthreads();
      const int c = j + 1 + (tid & 31);
      if (c < nc)
        for (int r = c + (tid >> 5); r < nr; r += 8) P[r * SW_PP + c] -= P[r * SW_PP + j] * P[c * SW_PP + j];
      __syncthreads();
    }
    for (int e = tid; e < nr * SW_PAN; e += 256) {
      const int r = e / SW_PAN, c = e - r * SW_PAN;
      const double v = P[r * SW_PP + c];
      L[(size_t)(c0 + r) * pw + c0 + c] = v;
      if (r == nr - 1 && c < nc) z[c0 + c] = v;
    }
    __syncthreads();   // the panel is in the slab (and P free) before the next update reads it
  }
  return true;
}
#endif

}  // namespace elfihip
