// The wide semiparametric synthetic likelihood (semiBSL) on gfx950: 65 to 256 summaries, with the semantics of semibsl.hip.
//
// semibsl.hip's finish kernel holds Q^T Q, rho and the factor in the LDS of one workgroup, which ends at 64 columns.  Here
// the work after the column kernel is split in two kernels with a global workspace between them.  Unlike the Gaussian wide
// form (synlik_wide.hip) no sums are shared between the prefixes of a group -- the ranks of the first p rows are their
// own -- so the unit of work is the (group, prefix) job from the first kernel on.
//
//   column    semibsl.hip's kernel in its wide layout (semi_rank.hpp: SemiWideArgs): one workgroup per (job, column); the
//             scores of a column go to Q[job][column][row], consecutive words, eta and logpdf to the job's statistics.
//   gram      one workgroup of 256 threads per (job, lower-triangle pair (bi, bj <= bi) of 64-column blocks): 3, 6 or 10
//             per job.  It streams the job's p rows 32 at a time: a chunk of a block is 64 runs of 32 consecutive
//             doubles, one per column, and stays column-major in LDS at a pitch of 34 doubles.  Consecutive lanes copy
//             consecutive rows (global: 256-byte runs; LDS: consecutive words).  The MFMA operand of lane (k = lane >> 4,
//             c = lane & 15) is word 34 c + k of a tile: over a half-wave (two k, sixteen c) the 4-byte bank pairs
//             (4 c + 2 k) mod 64 are all different, so neither side of the transposition has a bank conflict.  A
//             row-major slab at synlik_wide.hip's pitch of 80 reads as well but takes the copy at a stride of 80 words,
//             16 lanes to a bank.  2 x 64 x 34 doubles = 34 816 bytes of LDS.  The 16 tiles of the block are dealt four to
//             a wave (wave w: column tile w, the four row tiles), one v_mfma_f64_16x16x4_f64 per tile and 4 rows; every
//             chunk is summed from zero and then added to the total (syn_gram.hpp's two-level order).  Rows >= p and
//             columns >= m are staged as zero.  The epilogue writes rho = S / denominator, the diagonal exactly 1, into
//             the job's padded matrix, and for the full group into the caller's rho: one value at (i, j) and (j, i).
//   finish    one workgroup of 256 threads per (job, penalty): the left-looking panel Cholesky of wide_chol.hpp on the
//             job's slab, entry (i, j) = (1 - l) rho_ij + l [i == j] (corr_warton: no eps) formed as it is needed and eta
//             riding along as row m; then semibsl_finish_kernel's sums in index order in one thread and its formula.
// The gram and finish kernels are templates on their argument struct (semi_wide.hpp): wsemibsl_wide.hip, the whitened form,
// runs the gram kernel with a covariance epilogue as well and the finish kernel on the scaled matrix.
// No atomics, every sum in a fixed order: one (group, prefix, penalty) result depends neither on G, K, P nor on how the
// host cuts the jobs into launches to keep the workspace under the context's cap.  -inf with the status left at
// ELFIHIP_OK: as semibsl.hip (a u_j of 0 or 1, a column without spread, a non-positive pivot, a non-finite value, p = 2).
#include "semi_wide.hpp"

#include <algorithm>
#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

namespace elfihip {

// Args (semi_wide.hpp) picks the epilogue: SemiGramArgs rho of the scores at Q; SemiCovArgs their covariance for the whitened
// form, C_ab = ((Q^T Q)_ab - s_a s_b / p) / (p - 1), every block of the job's padded matrix, one value at (a, b) and (b, a).
// The column sums s of the staged columns are taken from the staged chunks in the two-level order (a thread per column: the
// 32 staged rows in order, then the total), so every workgroup that holds column a has the same bits of s_a.
template <class Args>
__global__ __launch_bounds__(256) void semibsl_wide_gram_kernel(Args A) {
  constexpr bool COV = std::is_same<Args, SemiCovArgs>::value;
  __shared__ __align__(16) double stage[2 * SW_BLK * SMW_CP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = A.m;
  const int64_t lj = blockIdx.x / (unsigned)A.pairs;
  const int pair = (int)(blockIdx.x - lj * A.pairs);
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= pair) ++bi;
  const int bj = pair - bi * (bi + 1) / 2;
  const bool diag = bi == bj;
  const int64_t gk = A.job0 + lj;
  const int p = (int)A.prefixes[gk % A.K];
  const double* Qj = A.Q + lj * m * A.NP;
  const double* stA = stage;
  const double* stB = diag ? stage : stage + SW_BLK * SMW_CP;
  const int slabs = diag ? 1 : 2;

  v4d tot[4], chk[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) tot[i] = (v4d){0.0, 0.0, 0.0, 0.0};
  const int lr = lane >> 4, lc = lane & 15;
  [[maybe_unused]] double stot = 0.0;   // COV: the sum of staged column tid
  for (int r0 = 0; r0 < p; r0 += SMW_RC) {
    __syncthreads();  // the previous chunk is consumed
    for (int e = tid; e < slabs * SW_BLK * SMW_RC; e += 256) {
      const int sc = e / SMW_RC, rr = e - sc * SMW_RC;   // sc: slab and column within it
      const int col = SW_BLK * (sc < SW_BLK ? bi : bj) + (sc & (SW_BLK - 1));
      const int r = r0 + rr;
      stage[sc * SMW_CP + rr] = (r < p && col < m) ? Qj[(int64_t)col * A.NP + r] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) chk[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int nr = p - r0 < SMW_RC ? p - r0 : SMW_RC;
    for (int s = 0; 4 * s < nr; ++s) {
      const double* colA = stA + lc * SMW_CP + 4 * s + lr;
      const double b = stB[(16 * wv + lc) * SMW_CP + 4 * s + lr];
#pragma unroll
      for (int i = 0; i < 4; ++i) chk[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(colA[16 * i * SMW_CP], b, chk[i], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) tot[i] += chk[i];
    if constexpr (COV) {
      if (tid < slabs * SW_BLK) {
        double sc = 0.0;
        for (int rr = 0; rr < SMW_RC; ++rr) sc += stage[tid * SMW_CP + rr];   // rows beyond p are zeros
        stot += sc;
      }
    }
  }

  double* Rj = A.R + (size_t)lj * A.mpad * A.mpad;
  if constexpr (COV) {
    __shared__ double csum[2 * SW_BLK];   // the column sums of block bi, then of block bj
    if (tid < slabs * SW_BLK) csum[tid] = stot;
    __syncthreads();
    const double dp = (double)p;
    const int cl = 16 * wv + lc;
    const int col = SW_BLK * bj + cl;
    const double sb = csum[(diag ? 0 : SW_BLK) + cl];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = 16 * i + lr + 4 * r;
        const int row = SW_BLK * bi + rl;
        if (col <= row) {   // (above the diagonal of a diagonal block: its mirror writes)
          const double v = (tot[i][r] - csum[rl] * sb / dp) / (dp - 1.0);
          Rj[(size_t)row * A.mpad + col] = v;
          Rj[(size_t)col * A.mpad + row] = v;
        }
      }
    return;
  }
  const double den = A.stats[lj * SEMI_WIDE_STATS + 2 * SEMI_WIDE_M];
  double* rho = (A.rho && p == A.n) ? A.rho + (gk / A.K) * m * m : nullptr;
  const int col = SW_BLK * bj + 16 * wv + lc;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = SW_BLK * bi + 16 * i + lr + 4 * r;
      const double v = row == col ? 1.0 : tot[i][r] / den;
      Rj[(size_t)row * A.mpad + col] = v;
      if (rho && row < m && col <= row) {   // (col <= row < m; above the diagonal of a diagonal block: its mirror writes)
        rho[(size_t)row * m + col] = v;
        rho[(size_t)col * m + row] = v;
      }
    }
}

// Args (semi_wide.hpp): SemiWideFinArgs the matrix and eta above; WsemiWideFinArgs the whitened form's scaled entry
// d_i ((1 - l) rho_ij + l [i == j]) d_j with eta_w as row m, and -inf before the factorisation if a d is not positive and finite.
template <class Args>
__global__ __launch_bounds__(256) void semibsl_wide_finish_kernel(Args A) {
  constexpr bool SCALED = std::is_same<Args, WsemiWideFinArgs>::value;
  extern __shared__ __align__(16) double lds[];
  const int m = A.m, mpad = A.mpad;
  double* P = lds;                            // (m + 1, SW_PP) the panel
  double* dg = P + (size_t)(m + 1) * SW_PP;   // diagonal of the factor
  double* z = dg + mpad;                      // the solved eta
  double* eta = z + mpad;
  double* lpv = eta + mpad;                   // logpdf of the columns
  const int tid = threadIdx.x;
  const int Pe = A.P > 0 ? A.P : 1;
  const int64_t fj = A.fjob0 + blockIdx.x;
  const int pi = (int)(fj % Pe);
  const int64_t lj = fj / Pe;
  const int64_t gk = A.job0 + lj;
  const int p = (int)A.prefixes[gk % A.K];
  const double* Rj = A.R + (size_t)lj * mpad * mpad;
  const double* st = A.stats + lj * SEMI_WIDE_STATS;
  double* L = A.slabs + (size_t)blockIdx.x * (size_t)(m + 1) * A.pw;
  double* out = A.loglik + (gk * Pe + pi);
  if (p == 2) {   // every column of scores is +-(a, b): rho has rank one
    if (tid == 0) *out = -INFINITY;
    return;
  }
  [[maybe_unused]] double* dsc = lpv + mpad;   // SCALED: d
  if constexpr (SCALED) {
    const double* ws = A.wst + lj * WSEMI_WIDE_STATS;
    double d = 1.0;
    if (tid < m) {
      eta[tid] = ws[SEMI_WIDE_M + tid];   // eta_w
      lpv[tid] = st[SEMI_WIDE_M + tid];
      dsc[tid] = d = ws[tid];
    }
    if (__syncthreads_or(!(d > 0.0 && d <= 1.7976931348623157e308))) {
      if (tid == 0) *out = -INFINITY;
      return;
    }
  } else {
    if (tid < m) {
      eta[tid] = st[tid];
      lpv[tid] = st[SEMI_WIDE_M + tid];
    }
    __syncthreads();
  }
  const double lam = A.P > 0 ? A.penalties[pi] : 0.0;
  const double gam = 1.0 - lam;
  // entry (i, j <= i) of the matrix to factor, row m eta: its forward solve is the factorisation's own update
  const auto entry = [&](int i, int j) -> double {
    if (j >= m || j > i) return 0.0;
    if (i == m) return eta[j];
    const double v = i == j ? gam + lam : gam * Rj[(size_t)i * mpad + j];
    if constexpr (SCALED)
      return dsc[i] * (v * dsc[j]);
    else
      return v;
  };
  if (!wide_panel_chol(L, A.pw, m, P, dg, z, entry)) {
    if (tid == 0) *out = -INFINITY;
    return;
  }
  if (tid == 0) {
    double quad = 0.0, ee = 0.0, logdet = 0.0, lps = 0.0;
    for (int j = 0; j < m; ++j) {
      quad += z[j] * z[j];
      ee += eta[j] * eta[j];
      logdet += log(dg[j]);
      lps += lpv[j];
    }
    double ll = -0.5 * (2.0 * logdet + (quad - ee)) + lps;
    if (!(fabs(ll) <= 1.7976931348623157e308)) ll = -INFINITY;   // NaN or an infinity of either sign
    *out = ll;
  }
}

static int semi_wide_check(elfihip_ctx* ctx, const void* X, int64_t G, int64_t n, int m, int64_t ldx, const void* y,
                           const int64_t* prefixes, int K, const double* penalties, int P, const void* loglik) {
  ELFIHIP_REQUIRE(ctx, m >= SW_MIN_M && m <= SW_MAX_M,
                  "wide semiparametric likelihood: %d summaries; %d to %d are supported (elfihip_semi_loglik takes 1 to %d)",
                  m, SW_MIN_M, SW_MAX_M, SW_MIN_M - 1);
  ELFIHIP_REQUIRE(ctx, n >= 2 && n <= SEMI_MAX_N, "wide semiparametric likelihood: %lld rows per group; 2 to %d are supported",
                  (long long)n, SEMI_MAX_N);
  ELFIHIP_REQUIRE(ctx, G >= 1 && G <= 0x7fffffff && ldx >= m, "bad shape G=%lld n=%lld m=%d ldx=%lld", (long long)G,
                  (long long)n, m, (long long)ldx);
  ELFIHIP_REQUIRE(ctx, X && y && loglik, "NULL data pointer");
  const std::string bad = group_lists_error(prefixes, K, penalties, P, n);
  ELFIHIP_REQUIRE(ctx, bad.empty(), "%s", bad.c_str());
  return ELFIHIP_OK;
}

template <class Args>
static int launch_gram(elfihip_ctx* ctx, const Args& M, int64_t jobs, const char* name) {
  hipLaunchKernelGGL(semibsl_wide_gram_kernel<Args>, dim3((unsigned)(jobs * M.pairs)), dim3(256), 0, ctx->stream, M);
  return launch_status(ctx, name);
}

int semibsl_wide_launch_gram(elfihip_ctx* ctx, const SemiGramArgs& M, int64_t jobs) {
  return launch_gram(ctx, M, jobs, "wide semiparametric likelihood gram kernel");
}

int semibsl_wide_launch_cov(elfihip_ctx* ctx, const SemiCovArgs& M, int64_t jobs) {
  return launch_gram(ctx, M, jobs, "wide whitened semiparametric likelihood covariance kernel");
}

// extra: doubles of LDS behind the factorisation's and the two vectors
template <class Args>
static int launch_finish(elfihip_ctx* ctx, const Args& F, int64_t count, size_t extra, const char* name) {
  const size_t lds = (wide_chol_lds(F.m) + 2 * (size_t)F.mpad + extra) * sizeof(double);
  ELFIHIP_TRY(set_lds(ctx, semibsl_wide_finish_kernel<Args>, lds, 48 * 1024));
  hipLaunchKernelGGL(semibsl_wide_finish_kernel<Args>, dim3((unsigned)count), dim3(256), lds, ctx->stream, F);
  return launch_status(ctx, name);
}

int semibsl_wide_launch_finish(elfihip_ctx* ctx, const SemiWideFinArgs& F, int64_t count) {
  return launch_finish(ctx, F, count, 0, "wide semiparametric likelihood finish kernel");
}

int semibsl_wide_launch_finish_scaled(elfihip_ctx* ctx, const WsemiWideFinArgs& F, int64_t count) {
  return launch_finish(ctx, F, count, (size_t)F.mpad, "wide whitened semiparametric likelihood finish kernel");
}

// Device rows, y and outputs; host prefixes and penalties (checked above).
static int semi_wide_dev_impl(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                              const int64_t* prefixes, int K, const double* penalties, int P, double* dll, double* du,
                              double* drho, double* dscores) {
  const GroupParams B = group_params(prefixes, K, n, nullptr, penalties, P);
  double* dpar;
  ELFIHIP_TRY(upload_group_params(ctx, B, 0, &dpar));
  const int Ke = B.Ke, Pe = P > 0 ? P : 1;
  const int mpad = wide_mpad(m), pw = wide_pitch(m), NP = (int)((n + SMW_RC - 1) / SMW_RC * SMW_RC);
  const int nb = mpad / SW_BLK, pairs = nb * (nb + 1) / 2;

  // The workspace, in doubles: [Q of Jc jobs][their rho][their statistics][Fc slabs].  Half the cap bounds the first three,
  // half the slabs; one job and one slab are the least a launch needs.  A launch has at most 2^31 - 1 workgroups: Jc m of
  // the column kernel (m > pairs, so the gram kernel's Jc pairs fit as well) and Fc of the finish kernel.
  const size_t cap = (ctx->wide_cap ? ctx->wide_cap : SW_SCRATCH_CAP) / sizeof(double);
  const size_t qd = (size_t)m * NP, rd = (size_t)mpad * mpad, slab = wide_slab(m);
  const size_t per_job = qd + rd + SEMI_WIDE_STATS;
  const int64_t J = G * Ke;
  const int64_t Jc = (int64_t)std::min<size_t>(std::min<size_t>((size_t)J, (size_t)(0x7fffffff / m)), std::max<size_t>(1, cap / 2 / per_job));
  const int64_t Fc = (int64_t)std::min<size_t>(std::min<size_t>((size_t)Jc * Pe, 0x7fffffff), std::max<size_t>(1, cap / 2 / slab));
  ELFIHIP_CHECK_HIP(ctx, ctx->scratch.reserve(((size_t)Jc * per_job + (size_t)Fc * slab) * sizeof(double)));

  SemiWideArgs C;
  C.X = dX;
  C.n = n;
  C.ldx = ldx;
  C.m = m;
  C.K = Ke;
  C.P = P;
  C.MP = 0;
  C.y = dy;
  C.prefixes = reinterpret_cast<const int64_t*>(dpar);
  C.penalties = P > 0 ? dpar + B.pen : nullptr;
  C.Q = ctx->scratch.as<double>();
  double* dR = C.Q + (size_t)Jc * qd;
  C.stats = dR + (size_t)Jc * rd;
  C.loglik = dll;
  C.u = du;
  C.rho = nullptr;   // the gram kernel's
  C.scores = dscores;
  C.NP = NP;
  SemiGramArgs M;
  M.Q = C.Q;
  M.stats = C.stats;
  M.R = dR;
  M.rho = drho;
  M.prefixes = C.prefixes;
  M.n = n;
  M.m = m;
  M.mpad = mpad;
  M.NP = NP;
  M.K = Ke;
  M.pairs = pairs;
  SemiWideFinArgs F;
  F.R = dR;
  F.stats = C.stats;
  F.slabs = C.stats + (size_t)Jc * SEMI_WIDE_STATS;
  F.loglik = dll;
  F.prefixes = C.prefixes;
  F.penalties = C.penalties;
  F.m = m;
  F.mpad = mpad;
  F.pw = pw;
  F.K = Ke;
  F.P = P;
  for (int64_t j0 = 0; j0 < J; j0 += Jc) {
    const int64_t jc = std::min<int64_t>(Jc, J - j0);
    C.job0 = M.job0 = F.job0 = j0;
    ELFIHIP_TRY(semibsl_launch_column_wide(ctx, C, jc));
    ELFIHIP_TRY(semibsl_wide_launch_gram(ctx, M, jc));
    for (int64_t f0 = 0; f0 < jc * Pe; f0 += Fc) {
      F.fjob0 = f0;
      ELFIHIP_TRY(semibsl_wide_launch_finish(ctx, F, std::min<int64_t>(Fc, jc * Pe - f0)));
    }
  }
  return ELFIHIP_OK;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_semi_loglik_wide_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx,
                                 const double* dy, const int64_t* prefixes, int K, const double* penalties, int P,
                                 double* dloglik, double* du, double* drho, double* dscores) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(semi_wide_check(ctx, dX, G, n, m, ldx, dy, prefixes, K, penalties, P, dloglik));
  DeviceGuard g(ctx->device);
  return semi_wide_dev_impl(ctx, dX, G, n, m, ldx, dy, prefixes, K, penalties, P, dloglik, du, drho, dscores);
}

int elfihip_semi_loglik_wide(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* y,
                             const int64_t* prefixes, int K, const double* penalties, int P, double* loglik, double* u,
                             double* rho, double* scores) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(semi_wide_check(ctx, X, G, n, m, ldx, y, prefixes, K, penalties, P, loglik));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)G * (size_t)n, md = (size_t)m * sizeof(double);
  const size_t nll = group_results(G, prefixes, K, P);
  // in: [X rows m][y m]; out: [loglik][u G m][rho G m m][scores G n m]
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((rows * m + (size_t)m) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((nll + (size_t)G * m + (size_t)G * m * m + (scores ? rows * m : 0)) * sizeof(double)));
  double* dX = ctx->in.as<double>();
  double* dy = dX + rows * m;
  double* dll = ctx->out.as<double>();
  double* du = dll + nll;
  double* drho = du + (size_t)G * m;
  double* dsc = drho + (size_t)G * m * m;
  ELFIHIP_TRY(upload_rows(ctx, dX, X, rows, m, ldx));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dy, y, md, hipMemcpyHostToDevice, st));
  ELFIHIP_TRY(semi_wide_dev_impl(ctx, dX, G, n, m, m, dy, prefixes, K, penalties, P, dll, u ? du : nullptr,
                                 rho ? drho : nullptr, scores ? dsc : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(loglik, dll, nll * sizeof(double), hipMemcpyDeviceToHost, st));
  if (u) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(u, du, (size_t)G * md, hipMemcpyDeviceToHost, st));
  if (rho) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(rho, drho, (size_t)G * m * md, hipMemcpyDeviceToHost, st));
  if (scores) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(scores, dsc, rows * md, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
