// What the group-statistic kernels share on the device (synlik.hip, semibsl.hip: the two synthetic likelihoods;
// logratio.hip: BOLFIRE's weighted Gram matrix): the shape of the LDS buffers, the MFMA step of the m x m sum of outer
// products and, for the likelihoods, the Cholesky factorisation with an extra row.  All stage rows 32 at a time, sum every
// chunk from zero and add it to the running total (two-level summation), so a matrix entry is the same sequence of
// operations whatever else the launch holds.  The chunk loops stay written out in each kernel: as a __forceinline__ helper
// here (zero chk, the gram_step loop, tot += chk) the loop changed all four instruction streams of semibsl_finish_kernel
// and its VGPR counts (T = 3: 64 -> 124 or 118, T = 4: 96 -> 132 or 156, by the helper's spelling), and a shared
// tile-to-LDS store changed all four as well (811 -> 812, 837 -> 825, 928 reordered, 1064 -> 1062 instructions); what that
// costs is not measured.  The host side these files share is in group_args.hpp and common.hpp.
#pragma once

#include "mfma_f64.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int SL_RC = 32;        // rows per staged chunk (8 MFMA steps)
constexpr int SL_MAX_M = 64;

template <int T>
struct GramShape {
  static constexpr int MP = 16 * T;                          // padded m
  static constexpr int SP = (MP % 32 == 0) ? MP + 16 : MP;   // pitch of the staged rows: pitch mod 32 == 16, so the two
                                                             // rows a half-wave reads fall into different banks
  static constexpr int LP = MP + 1;                          // pitch of the m x m matrices
  static constexpr int NT = (T * T + 3) / 4;                 // tiles per wave
};

// One MFMA step: chk += sum over the four staged rows at `row` (this lane's row lane >> 4, column lane & 15 of tile 0)
// of their outer product; tile q = wave + 4 i of the T x T tiles belongs to accumulator i of wave `wv`.
template <int T>
__device__ __forceinline__ void gram_step(v4d (&chk)[GramShape<T>::NT], const double* row, int wv) {
#pragma unroll
  for (int i = 0; i < GramShape<T>::NT; ++i) {
    const int q = wv + 4 * i;
    if (q < T * T) {
      const int ti = q / T, tj = q - ti * T;
      chk[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(row[16 * ti], row[16 * tj], chk[i], 0, 0, 0);
    }
  }
}

// Right-looking Cholesky factorisation, in place, of the lower triangle of the m x m matrix in L (pitch LP) with row m as
// an extra row: after it row m holds the forward solve of what it held.  dg receives the diagonal of the factor.  All 256
// threads; false (for every thread) at the first pivot that is not positive.
template <int LP>
__device__ __forceinline__ bool chol_extra_row(double* L, double* dg, int m) {
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  for (int j = 0; j < m; ++j) {
    const double piv = L[j * LP + j];   // the same word for every thread: the branch is uniform
    if (!(piv > 0.0)) return false;
    const double d = sqrt(piv);         // (nobody writes L[j][j] from here on)
    if (tid == 0) dg[j] = d;
    if (j + 1 + tid <= m) L[(j + 1 + tid) * LP + j] = L[(j + 1 + tid) * LP + j] / d;
    __syncthreads();
    for (int i = j + 1 + ty; i <= m; i += 16) {
      const double lij = L[i * LP + j];
      for (int k = j + 1 + tx; k <= i && k < m; k += 16) L[i * LP + k] -= lij * L[k * LP + j];
    }
    __syncthreads();
  }
  return true;
}

}  // namespace elfihip
