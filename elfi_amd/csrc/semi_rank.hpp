// What the semiparametric likelihoods share (semibsl.hip: semiBSL; wsemibsl.hip: the whitened form; semibsl_wide.hip:
// semiBSL above 64 summaries, which takes the column kernel, the row bound and the device helpers): the arguments
// and the launch of the column kernel, the entry points' first checks and the set-up before the launches, the workgroup
// reductions, and the rank of a value within a column held in LDS.
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

// The wide layout of the column kernel (semibsl_wide.hip: 65 to 256 summaries).  A launch holds the (group, prefix) jobs
// job0 .. job0 + jobs - 1 of the call, job = g K + k; Q and stats are the launch's own and counted from its first job.
//   Q      (jobs, m, NP) column-major: the scores of one column are consecutive, NP = n rounded up to a multiple of 32
//   stats  (jobs, SEMI_WIDE_STATS): eta at 0, logpdf at SEMI_WIDE_M, the denominator at 2 SEMI_WIDE_M
// MP is not used.  u and scores stay (G, m) and (G, n, m) of the whole call.
constexpr int SEMI_WIDE_M = 256;
constexpr int SEMI_WIDE_STATS = 2 * SEMI_WIDE_M + 8;
struct SemiWideArgs : SemiArgs {
  int64_t job0;
  int NP;
};
int semibsl_launch_column_wide(elfihip_ctx* ctx, const SemiWideArgs& A, int64_t jobs);

// The checks both likelihoods' entry points begin with; `what` names the likelihood in the texts.  Each goes on with its own
// bound on the number of workgroups and the check of the lists.
inline int semi_check(elfihip_ctx* ctx, const char* what, const void* X, int64_t G, int64_t n, int m, int64_t ldx,
                      const void* y, const void* loglik) {
  ELFIHIP_REQUIRE(ctx, m >= 1 && m <= SL_MAX_M, "%s: %d summaries; 1 to %d are supported", what, m, SL_MAX_M);
  ELFIHIP_REQUIRE(ctx, n >= 2 && n <= SEMI_MAX_N, "%s: %lld rows per group; 2 to %d are supported", what, (long long)n,
                  SEMI_MAX_N);
  ELFIHIP_REQUIRE(ctx, G >= 1 && ldx >= m, "bad shape G=%lld n=%lld m=%d ldx=%lld", (long long)G, (long long)n, m,
                  (long long)ldx);
  ELFIHIP_REQUIRE(ctx, X && y && loglik, "NULL data pointer");
  return ELFIHIP_OK;
}

// What both likelihoods do before their launches, on device rows, y and outputs and host lists (checked): the parameter
// block [prefixes Ke][penalties P] goes to the device, the scratch is reserved as [Q][extra_doubles, the caller's][stats],
// and A is filled in.
inline int semi_setup(elfihip_ctx* ctx, SemiArgs& A, const double* dX, int64_t G, int64_t n, int m, int64_t ldx,
                      const double* dy, const int64_t* prefixes, int K, const double* penalties, int P,
                      size_t extra_doubles, double* dll, double* du, double* drho, double* dscores) {
  const GroupParams B = group_params(prefixes, K, n, nullptr, penalties, P);
  double* dpar;
  ELFIHIP_TRY(upload_group_params(ctx, B, 0, &dpar));
  const int MP = 16 * group_tiles(m);
  const size_t GK = (size_t)G * B.Ke, qd = GK * (size_t)n * MP;
  ELFIHIP_CHECK_HIP(ctx, ctx->scratch.reserve((qd + extra_doubles + GK * SEMI_STATS) * sizeof(double)));
  A.X = dX;
  A.n = n;
  A.ldx = ldx;
  A.m = m;
  A.K = B.Ke;
  A.P = P;
  A.MP = MP;
  A.y = dy;
  A.prefixes = reinterpret_cast<const int64_t*>(dpar);
  A.penalties = P > 0 ? dpar + B.pen : nullptr;
  A.Q = ctx->scratch.as<double>();
  A.stats = A.Q + qd + extra_doubles;
  A.loglik = dll;
  A.u = du;
  A.rho = drho;
  A.scores = dscores;
  return ELFIHIP_OK;
}

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
