// Batched semiparametric synthetic likelihood (semiBSL; An, Nott & Drovandi 2020) on gfx950.
//
// Replaces, for G groups of n simulated summary rows at once, what elfi/methods/bsl/pdf_methods.py:179-264
// (semi_param_kernel_estimate) does per call in a Python loop over the columns -- a scipy gaussian_kde per column, its
// integral, the Gaussian rank correlation (gaussian_rank_corr.py:30-52), corr_warton, LU and an inverse -- and what
// log_SL_stdev / select_penalty loop over: prefixes of the same rows and a list of penalties.
//
// Two launches.
//   column   one workgroup of 256 threads per (group, prefix, column).  The first p entries of the column sit in LDS.
//            Mean and variance by a shifted two-pass sum give the bandwidth h = (3 p / 4)^(-1/5) std (ddof 1: Silverman's
//            rule as scipy's gaussian_kde applies it in one dimension).  With z_i = (y - x_i) / h:
//              logpdf = logsumexp_i(-z_i^2 / 2) - log p - log h - log(2 pi) / 2   (about the largest exponent: a far-away
//                       y gives a finite, very negative value, not log 0)
//              u      = min(1, sum_i Phi(z_i) / p),  eta = Phi^-1(u)
//            Ranks by counting, straight from LDS: r_i = #{x_t < x_i} + (#{x_t = x_i} + 1) / 2 -- every lane reads the
//            same x_t (a broadcast), ties get the average rank exactly, nothing is sorted; p^2 / 256 comparisons per
//            thread.  Scores q_i = Phi^-1(r_i / (p + 1)) go to a scratch matrix (G K, n, MP).  The workgroup of column 0
//            also sums the denominator sum_i Phi^-1(i / (p + 1))^2.
//   finish   one workgroup per (group, prefix): Q^T Q by v_mfma_f64_16x16x4_f64 with the 32-row staging and the
//            two-level summation of synlik.hip (syn_gram.hpp), then in LDS rho = Q^T Q / denominator with the diagonal
//            set to exactly 1, and per penalty (1 - l) rho + l I (corr_warton: no eps), the Cholesky factor with eta as
//            an extra row, and  -(log|rho| + (z^T z - eta^T eta)) / 2 + sum_j logpdf_j.
// Every sum is a per-thread strided sum followed by a fixed tree over the 256 threads, or the MFMA order above: no
// atomics, and nothing depends on G, on the other prefixes or on the other penalties of the call -- prefix p of a long
// group has the bits of a group of p rows.
// -inf, with the status left at ELFIHIP_OK: a u_j of 0 or 1 (eta infinite), a non-positive pivot, a non-finite value; a
// column without spread (h = 0; a decided divergence: the reference raises LinAlgError from gaussian_kde there); two rows
// and more than one column (every column of scores is +-(a, b): rho has rank one; the reference returns about -1e16 from
// the noise of its LU).
#include "common.hpp"
#include "special.hpp"
#include "syn_gram.hpp"

#include <algorithm>
#include <cmath>

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

__global__ __launch_bounds__(256) void semibsl_column_kernel(SemiArgs A) {
  extern __shared__ __align__(16) double lds[];
  double* red = lds;              // (SEMI_RED)
  double* col = lds + SEMI_RED;   // the column, NaN up to a multiple of 4 (a NaN counts in no comparison)
  const int tid = threadIdx.x, m = A.m;
  const int j = (int)(blockIdx.x % (unsigned)m);
  const int64_t gk = blockIdx.x / (unsigned)m;
  const int k = (int)(gk % A.K);
  const int64_t g = gk / A.K;
  const int p = (int)A.prefixes[k];
  const int pp = (p + 3) & ~3;
  const bool full = p == A.n;
  const double* xg = A.X + g * A.n * A.ldx + j;
  for (int i = tid; i < pp; i += 256) col[i] = i < p ? xg[(int64_t)i * A.ldx] : NAN;
  __syncthreads();
  const double dp = (double)p;

  // bandwidth
  const double c = col[0];
  double s = 0.0;
  for (int i = tid; i < p; i += 256) s += col[i] - c;
  const double mean = c + block_sum(s, red) / dp;
  s = 0.0;
  for (int i = tid; i < p; i += 256) {
    const double d = col[i] - mean;
    s += d * d;
  }
  const double var = block_sum(s, red) / (dp - 1.0);
  const double h = pow(0.75 * dp, -0.2) * sqrt(var);

  // the kernel density estimate at y and its integral up to y
  const double yj = A.y[j];
  double mx = -INFINITY;
  for (int i = tid; i < p; i += 256) {
    const double z = (yj - col[i]) / h;
    mx = fmax(mx, -0.5 * (z * z));
  }
  mx = block_max(mx, red);
  double se = 0.0, sc = 0.0;
  for (int i = tid; i < p; i += 256) {
    const double z = (yj - col[i]) / h;
    se += exp(-0.5 * (z * z) - mx);
    sc += norm_cdf(z);
  }
  se = block_sum(se, red);
  sc = block_sum(sc, red);
  double* st = A.stats + gk * SEMI_STATS;
  if (tid == 0) {
    double lp = mx + log(se) - log(dp) - log(h) - 0.91893853320467274178;
    if (!(h > 0.0 && h <= 1.7976931348623157e308)) lp = -INFINITY;   // no spread, or a value that is not finite
    const double u = fmin(1.0, sc / dp);
    st[j] = norm_ppf(u);
    st[SL_MAX_M + j] = lp;
    if (A.u && full) A.u[g * m + j] = u;
  }

  // ranks -> normal scores
  const double np1 = dp + 1.0;
  double* Qg = A.Q + gk * A.n * A.MP + j;
  const double2* col2 = reinterpret_cast<const double2*>(col);
  for (int i = tid; i < p; i += 256) {
    const double xi = col[i];
    int lt = 0, eq = 0;
    for (int t = 0; t < pp / 2; t += 2) {
      const double2 a = col2[t], b = col2[t + 1];
      lt += (a.x < xi) + (a.y < xi) + (b.x < xi) + (b.y < xi);
      eq += (a.x == xi) + (a.y == xi) + (b.x == xi) + (b.y == xi);
    }
    const double r = (double)lt + 0.5 * (double)(eq + 1);
    const double q = norm_ppf(r / np1);
    Qg[(int64_t)i * A.MP] = q;
    if (A.scores && full) A.scores[(g * A.n + i) * m + j] = q;
  }

  // the denominator of the rank correlation depends on p alone: the workgroup of column 0 sums it
  if (j == 0) {
    s = 0.0;
    for (int i = tid; i < p; i += 256) {
      const double q = norm_ppf((double)(i + 1) / np1);
      s += q * q;
    }
    s = block_sum(s, red);
    if (tid == 0) st[2 * SL_MAX_M] = s;
  }
}

template <int T>
struct SemiShape : GramShape<T> {
  using GramShape<T>::MP;
  using GramShape<T>::SP;
  using GramShape<T>::LP;
  static constexpr int DOUBLES = SL_RC * SP + MP * LP + (MP + 1) * LP + 3 * MP;
  static_assert(DOUBLES * sizeof(double) <= 160 * 1024);
};

template <int T>
__global__ __launch_bounds__(256) void semibsl_finish_kernel(SemiArgs A) {
  using Sh = SemiShape<T>;
  constexpr int MP = Sh::MP, SP = Sh::SP, LP = Sh::LP, NT = Sh::NT;
  extern __shared__ __align__(16) double lds[];
  double* stage = lds;                  // (SL_RC, SP) scores, zero beyond p and beyond m
  double* S = stage + SL_RC * SP;       // (MP, LP) Q^T Q, then rho
  double* L = S + MP * LP;              // (MP + 1, LP) the matrix being factorised + eta
  double* eta = L + (MP + 1) * LP;
  double* lpv = eta + MP;               // logpdf of the columns
  double* dg = lpv + MP;                // diagonal of the factor
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = A.m;
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t gk = blockIdx.x;
  const int k = (int)(gk % A.K);
  const int64_t g = gk / A.K;
  const int p = (int)A.prefixes[k];
  const double* Qg = A.Q + gk * A.n * MP;
  const double* st = A.stats + gk * SEMI_STATS;
  if (tid < MP) {
    eta[tid] = tid < m ? st[tid] : 0.0;
    lpv[tid] = tid < m ? st[SL_MAX_M + tid] : 0.0;
  }
  const double den = st[2 * SL_MAX_M];

  v4d tot[NT], chk[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) tot[i] = (v4d){0.0, 0.0, 0.0, 0.0};
  const int lr = lane >> 4, lc = lane & 15;
  for (int r0 = 0; r0 < p; r0 += SL_RC) {
    __syncthreads();  // the previous chunk is consumed
    for (int e = tid; e < SL_RC * MP; e += 256) {
      const int rr = e / MP, c = e - rr * MP;
      const int r = r0 + rr;
      stage[rr * SP + c] = (r < p && c < m) ? Qg[(int64_t)r * MP + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NT; ++i) chk[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    const int nr = p - r0 < SL_RC ? p - r0 : SL_RC;
    for (int s = 0; 4 * s < nr; ++s) gram_step<T>(chk, stage + (4 * s + lr) * SP + lc, wv);
#pragma unroll
    for (int i = 0; i < NT; ++i) tot[i] += chk[i];
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int q = wv + 4 * i;
    if (q < T * T) {
      const int ti = q / T, tj = q - ti * T;
#pragma unroll
      for (int r = 0; r < 4; ++r) S[(16 * ti + lr + 4 * r) * LP + 16 * tj + lc] = tot[i][r];
    }
  }
  __syncthreads();
  for (int i = ty; i < m; i += 16)
    for (int j = tx; j < m; j += 16) {
      const double v = i == j ? 1.0 : S[i * LP + j] / den;
      S[i * LP + j] = v;
      if (A.rho && p == A.n) A.rho[(g * m + i) * m + j] = v;
    }
  const int Pe = A.P > 0 ? A.P : 1;
  for (int pi = 0; pi < Pe; ++pi) {
    __syncthreads();
    const double lam = A.P > 0 ? A.penalties[pi] : 0.0;
    const double gam = 1.0 - lam;
    for (int i = ty; i < m; i += 16)
      for (int j = tx; j <= i; j += 16) L[i * LP + j] = i == j ? gam + lam : gam * S[i * LP + j];
    if (tid < m) L[m * LP + tid] = eta[tid];   // eta as row m of the factor: its forward solve is the factorisation's own update
    __syncthreads();
    const bool ok = chol_extra_row<LP>(L, dg, m);
    if (tid == 0) {
      double ll = -INFINITY;
      if (ok && !(p == 2 && m > 1)) {
        double quad = 0.0, ee = 0.0, logdet = 0.0, lps = 0.0;
        for (int j = 0; j < m; ++j) {
          const double z = L[m * LP + j];
          quad += z * z;
          ee += eta[j] * eta[j];
          logdet += log(dg[j]);
          lps += lpv[j];
        }
        ll = -0.5 * (2.0 * logdet + (quad - ee)) + lps;
        if (!(fabs(ll) <= 1.7976931348623157e308)) ll = -INFINITY;   // NaN or an infinity of either sign
      }
      A.loglik[(gk * Pe) + pi] = ll;
    }
  }
}

static int semibsl_check(elfihip_ctx* ctx, const void* X, int64_t G, int64_t n, int m, int64_t ldx, const void* y,
                         const int64_t* prefixes, int K, const double* penalties, int P, const void* loglik) {
  ELFIHIP_REQUIRE(ctx, m >= 1 && m <= SL_MAX_M, "semiparametric likelihood: %d summaries; 1 to %d are supported", m,
                  SL_MAX_M);
  ELFIHIP_REQUIRE(ctx, n >= 2 && n <= SEMI_MAX_N, "semiparametric likelihood: %lld rows per group; 2 to %d are supported",
                  (long long)n, SEMI_MAX_N);
  ELFIHIP_REQUIRE(ctx, G >= 1 && ldx >= m, "bad shape G=%lld n=%lld m=%d ldx=%lld", (long long)G, (long long)n, m,
                  (long long)ldx);
  ELFIHIP_REQUIRE(ctx, X && y && loglik, "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, G * (int64_t)(prefixes ? K : 1) * m <= 0x7fffffff, "G K m = %lld x %d x %d workgroups are too many",
                  (long long)G, prefixes ? K : 1, m);
  const std::string bad = group_lists_error(prefixes, K, penalties, P, n);
  ELFIHIP_REQUIRE(ctx, bad.empty(), "%s", bad.c_str());
  return ELFIHIP_OK;
}

// Device rows, y and outputs; host prefixes and penalties (checked above).
static int semibsl_dev_impl(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                            const int64_t* prefixes, int K, const double* penalties, int P, double* dll, double* du,
                            double* drho, double* dscores) {
  hipStream_t st = ctx->stream;
  // parameter block: [prefixes Ke][penalties P]
  const GroupParams B = group_params(prefixes, K, n, nullptr, penalties, P);
  const int Ke = B.Ke;
  const int64_t GK = G * Ke;
  const int MP = 16 * group_tiles(m);
  ELFIHIP_CHECK_HIP(ctx, ctx->par.reserve(B.words.size() * sizeof(double)));
  double* dpar = ctx->par.as<double>();
  // pageable host memory: the copy is done with it when hipMemcpyAsync returns (common.hpp: pageable uploads)
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar, B.words.data(), B.words.size() * sizeof(double), hipMemcpyHostToDevice, st));
  const size_t qd = (size_t)GK * (size_t)n * MP;
  ELFIHIP_CHECK_HIP(ctx, ctx->scratch.reserve((qd + (size_t)GK * SEMI_STATS) * sizeof(double)));
  SemiArgs A;
  A.X = dX;
  A.n = n;
  A.ldx = ldx;
  A.m = m;
  A.K = Ke;
  A.P = P;
  A.MP = MP;
  A.y = dy;
  A.prefixes = reinterpret_cast<const int64_t*>(dpar);
  A.penalties = P > 0 ? dpar + B.pen : nullptr;
  A.Q = ctx->scratch.as<double>();
  A.stats = A.Q + qd;
  A.loglik = dll;
  A.u = du;
  A.rho = drho;
  A.scores = dscores;
  const size_t bytes = (size_t)(SEMI_RED + ((n + 3) & ~(int64_t)3)) * sizeof(double);
  ELFIHIP_TRY(set_lds(ctx, semibsl_column_kernel, bytes, 48 * 1024));
  hipLaunchKernelGGL(semibsl_column_kernel, dim3((unsigned)(GK * m)), dim3(256), bytes, st, A);
  ELFIHIP_TRY(launch_status(ctx, "semiparametric likelihood column kernel"));
  return launch_by_tiles(
      ctx, m, (unsigned)GK, "semiparametric likelihood finish kernel",
      [](auto T) { return semibsl_finish_kernel<decltype(T)::value>; },
      [](auto T) { return (size_t)SemiShape<decltype(T)::value>::DOUBLES * sizeof(double); }, A);
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_semi_loglik_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                            const int64_t* prefixes, int K, const double* penalties, int P, double* dloglik, double* du,
                            double* drho, double* dscores) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(semibsl_check(ctx, dX, G, n, m, ldx, dy, prefixes, K, penalties, P, dloglik));
  DeviceGuard g(ctx->device);
  return semibsl_dev_impl(ctx, dX, G, n, m, ldx, dy, prefixes, K, penalties, P, dloglik, du, drho, dscores);
}

int elfihip_semi_loglik(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* y,
                        const int64_t* prefixes, int K, const double* penalties, int P, double* loglik, double* u,
                        double* rho, double* scores) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(semibsl_check(ctx, X, G, n, m, ldx, y, prefixes, K, penalties, P, loglik));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)G * (size_t)n, md = (size_t)m * sizeof(double);
  const size_t nll = (size_t)G * (prefixes ? K : 1) * (P > 0 ? P : 1);
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
  ELFIHIP_TRY(semibsl_dev_impl(ctx, dX, G, n, m, m, dy, prefixes, K, penalties, P, dll, u ? du : nullptr,
                               rho ? drho : nullptr, scores ? dsc : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(loglik, dll, nll * sizeof(double), hipMemcpyDeviceToHost, st));
  if (u) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(u, du, (size_t)G * md, hipMemcpyDeviceToHost, st));
  if (rho) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(rho, drho, (size_t)G * m * md, hipMemcpyDeviceToHost, st));
  if (scores) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(scores, dsc, rows * md, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
