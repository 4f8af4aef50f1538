// The slice samplers for the adjustment parameters gamma of the misspecification-robust synthetic likelihood (Frazier &
// Drovandi 2021) on gfx950: G independent chains' states in one launch.
//
// Replaces, between two likelihood evaluations of elfi.BSL (_init_round),
//     slice_gamma_mean      elfi/methods/bsl/slice_gamma_mean.py:35-138
//     slice_gamma_variance  elfi/methods/bsl/slice_gamma_variance.py:31-115
// which walk the m coordinates one by one, step out and shrink, and pay a scipy.stats.multivariate_normal.logpdf -- an
// eigendecomposition of the m x m covariance -- for every trial point.
//
// One workgroup of ONE wavefront per problem, lane i = coordinate i.  Within a coordinate every trial point is a rank-one
// change of what one factorisation gives, so a trial costs O(m) (mean) or O(1) (variance) instead of O(m^3):
//   mean      one Cholesky factor L of cov per call; per coordinate z = L^-1 (y - mean - std o gamma), t = std_ii L^-1 e_ii;
//             the quadratic form at g' is |z - (g' - g_ii) t|^2 and the determinant never changes;
//   variance  per coordinate the factor of B = cov + diag((std o gamma)^2) with coordinate ii's own term REMOVED, so the
//             change delta = (std_ii g')^2 is never negative and nothing cancels; with u = L^-1 e_ii, v = L^-1 (y - mean),
//             a = u'u, b = u'v, q = v'v a trial is log det B + log1p(delta a) and q - delta b^2 / (1 + delta a).
// The lower triangle of cov (diagonal included) and the factor live in ONE m x m LDS array: the factor is kept transposed in
// the strict upper triangle (entry L[i][k] at [k][i], so lane i's reads of its row are 64 neighbouring words) and its
// diagonal in a lane register.  Only the lower triangle of cov is read, as SciPy's eigh reads it.
//
// Everything that decides control flow -- the targets, the bounds, the draws, the counters, the pivots -- is reduced to the
// same bits in all 64 lanes (sg_sum64: a DPP sum inside each row of 16 lanes, then the four rows in a fixed order through
// scalar reads) and read as a scalar: no loop has a divergent exit, and the barriers around the LDS array cannot wait for a
// wavefront on another path.  No atomics, a fixed order in every sum, FMA contraction off; a problem's result does not
// depend on G.  Every loop is bounded by m or max_iter.
//
// The statement is in include/elfihip.h and, in NumPy, in tests/slice_gamma_ref.py.
#include "common.hpp"

#include <cfloat>
#include <cmath>

#include "philox.hpp"
#include "syn_gram.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int SG_THREADS = 64;          // one wavefront
constexpr int SG_LP = SL_MAX_M + 1;     // pitch of the LDS matrix
constexpr int64_t SG_MAX_ITER = 1 << 20;

struct SgArgs {
  int adjustment, m;
  const double *y, *mean, *cov;   // (G, m), (G, m), (G, m, ldc)
  int64_t ldc;
  const double *gamma_in, *loglik_in;
  double tau, w;
  int64_t max_iter;
  const double* U;   // (G, n_u) or NULL: Philox
  int64_t n_u;
  uint64_t seed, stream;
  double *gamma_out, *loglik_out;
  long long *used, *evals;
  int32_t* status;
};

// the value lane 0 holds, as a scalar (every lane holds the same bits where this is used)
__device__ __forceinline__ double sg_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// the value lane `src` holds (src the same in every lane), as a scalar
__device__ __forceinline__ double sg_lane(double v, int src) {
  const int s = __builtin_amdgcn_readfirstlane(src);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), s), __builtin_amdgcn_readlane(__double2loint(v), s));
}
// the sum over the 64 lanes, the same bits in every lane: each row of 16 by DPP, then (r0 + r1) + (r2 + r3)
__device__ __forceinline__ double sg_sum64(double v) {
  v = lanes16_sum(v);
  return (sg_lane(v, 0) + sg_lane(v, 16)) + (sg_lane(v, 32) + sg_lane(v, 48));
}
__device__ __forceinline__ bool sg_finite(double v) { return v - v == 0.0; }

// Left-looking Cholesky factorisation of the matrix whose strict lower triangle is in A and whose diagonal entry i lane i
// holds in `diag`: on return lane i holds the factor's diagonal entry in dg and L[i][k], k < i, is at A[k][i].  false (in
// every lane) at the first pivot that is not positive.
__device__ __forceinline__ bool sg_factor(double* A, int m, int lane, double diag, double& dg) {
  dg = 1.0;
  for (int j = 0; j < m; ++j) {
    double s = lane == j ? diag : (lane > j && lane < m ? A[lane * SG_LP + j] : 0.0);
    if (lane >= j && lane < m) {
#pragma unroll 8      // eight pairs of LDS reads in flight; the subtractions keep their order
      for (int k = 0; k < j; ++k) s -= A[k * SG_LP + lane] * A[k * SG_LP + j];
    }
    const double piv = sg_lane(s, j);
    if (!(piv > 0.0)) return false;
    const double d = sqrt(piv);
    if (lane == j) dg = d;
    if (lane > j && lane < m) A[j * SG_LP + lane] = s / d;      // row j of the transposed factor: read from column j + 1 on
    __syncthreads();
  }
  return true;
}

// x = L^-1 b and x2 = L^-1 b2 by columns: lane i gives its entries of the right-hand sides and receives the solutions'
__device__ __forceinline__ void sg_solve2(const double* A, int m, int lane, double dg, double& b, double& b2) {
  for (int j = 0; j < m; ++j) {
    const double d = sg_lane(dg, j);
    const double xj = sg_lane(b, j) / d, x2j = sg_lane(b2, j) / d;
    if (lane == j) {
      b = xj;
      b2 = x2j;
    }
    if (lane > j && lane < m) {
      const double l = A[j * SG_LP + lane];
      b -= l * xj;
      b2 -= l * x2j;
    }
  }
}

struct SgState {
  int64_t used, evals;
  int status;
};

// one double in [0, 1): the caller's, or the 53-bit uniform of Philox counter `used` of the problem's stream
__device__ __forceinline__ bool sg_draw(const SgArgs& A, int64_t g, SgState& S, double& d) {
  if (A.U) {
    if (S.used >= A.n_u) {
      S.status = ELFIHIP_SLICE_OUT_OF_DRAWS;
      return false;
    }
    d = sg_uniform(A.U[g * A.n_u + S.used]);
  } else {
    d = sg_uniform(uniform53_first(A.seed, A.stream + (uint64_t)g, (uint64_t)S.used));
  }
  ++S.used;
  return true;
}

template <int ADJ>
__device__ __forceinline__ void sg_run(const SgArgs& A, int64_t g, double* s_A, int lane, SgState& S, double& gam, double& ll_out) {
  constexpr double LOG_2PI = 1.8378770664093453;    // SciPy's _LOG_2PI = log(2 pi)
  const int m = A.m;
  const bool in = lane < m;
  const double tau = A.tau, w = A.w;
  const int64_t max_iter = A.max_iter;
  const double* cov = A.cov + g * (int64_t)m * A.ldc;
  for (int i = 0; i < m; ++i)
    if (lane <= i) s_A[i * SG_LP + lane] = cov[(int64_t)i * A.ldc + lane];      // the lower triangle, rows coalesced
  __syncthreads();
  const double cdiag = in ? s_A[lane * SG_LP + lane] : 1.0;
  const double sd = sqrt(cdiag);
  const double resid0 = in ? A.y[g * m + lane] - A.mean[g * m + lane] : 0.0;     // y - mean (the variance form's residual)
  const double ybase = in ? A.y[g * m + lane] : 0.0, mbase = in ? A.mean[g * m + lane] : 0.0;
  gam = in ? A.gamma_in[g * m + lane] : 0.0;
  double loglik = sg_uniform(A.loglik_in[g]);      // the reference's variable: the LAST likelihood evaluated
  ll_out = loglik;                                 // ... and the last ACCEPTED one
  const double rate = 1.0 / tau, log_tau = log(tau);
  const double prior_const = (double)m * log(rate / 2.0);

  double dg = 1.0, logdet = 0.0;
  if (ADJ == 0) {
    if (!sg_factor(s_A, m, lane, cdiag, dg)) {
      S.status = ELFIHIP_SLICE_NONFINITE;
      return;
    }
    logdet = 2.0 * sg_sum64(in ? log(dg) : 0.0);
  }

  for (int ii = 0; ii < m; ++ii) {
    double z, t, qa = 0.0, qb = 0.0, qq = 0.0;
    if (ADJ == 0) {
      z = in ? ybase - (mbase + sd * gam) : 0.0;
      t = lane == ii ? sd : 0.0;
      sg_solve2(s_A, m, lane, dg, z, t);
    } else {
      const double sg = sd * gam;
      if (!sg_factor(s_A, m, lane, lane == ii ? cdiag : cdiag + sg * sg, dg)) {
        S.status = ELFIHIP_SLICE_NONFINITE;
        return;
      }
      logdet = 2.0 * sg_sum64(in ? log(dg) : 0.0);
      z = lane == ii ? 1.0 : 0.0;     // u
      t = resid0;                     // v
      sg_solve2(s_A, m, lane, dg, z, t);
      qa = sg_sum64(in ? z * z : 0.0);
      qb = sg_sum64(in ? z * t : 0.0);
      qq = sg_sum64(in ? t * t : 0.0);
    }
    const double g_ii = sg_lane(gam, ii), sd_ii = sg_lane(sd, ii);

    // log prior of gamma with coordinate ii at x
    auto prior = [&](double x) -> double {
      const double gi = lane == ii ? x : gam;
      if (ADJ == 0) return prior_const - rate * sg_sum64(in ? fabs(gi) : 0.0);
      return sg_sum64(in ? (gi < 0.0 ? -INFINITY : -(gi / tau) - log_tau) : 0.0);
    };
    // log-likelihood with coordinate ii at x
    auto lik = [&](double x) -> double {
      ++S.evals;
      if (ADJ == 0) {
        const double dx = x - g_ii;
        const double r = in ? z - dx * t : 0.0;
        return -0.5 * (((double)m * LOG_2PI + logdet) + sg_sum64(r * r));
      }
      const double sx = sd_ii * x, delta = sx * sx, den = 1.0 + delta * qa;
      return -0.5 * (((double)m * LOG_2PI + (logdet + log1p(delta * qa))) + (qq - (delta * (qb * qb)) / den));
    };

    double d;
    if (!sg_draw(A, g, S, d)) return;
    const double e = -log(1.0 - d);
    const double target = (loglik + prior(g_ii)) - e;
    if (!sg_finite(target)) {
      S.status = ELFIHIP_SLICE_NONFINITE;
      return;
    }
    double lower = ADJ == 0 ? g_ii - w : 0.0, upper = g_ii + w;
    if (ADJ == 0) {
      for (int64_t i = 0; i <= max_iter; ++i) {
        loglik = lik(lower);
        const double tx = loglik + prior(lower);
        if (!sg_finite(tx)) {
          S.status = ELFIHIP_SLICE_NONFINITE;
          return;
        }
        if (tx < target) break;
        lower = lower - w;
      }
    }
    for (int64_t i = 0; i <= max_iter; ++i) {
      loglik = lik(upper);
      const double tx = loglik + prior(upper);
      if (!sg_finite(tx)) {
        S.status = ELFIHIP_SLICE_NONFINITE;
        return;
      }
      if (tx < target) break;
      upper = upper + w;
    }
    for (int64_t i = 0; i < max_iter; ++i) {
      if (!sg_draw(A, g, S, d)) return;
      const double prop = lower + (upper - lower) * d;
      loglik = lik(prop);
      const double tx = loglik + prior(prop);
      if (!sg_finite(tx)) {
        S.status = ELFIHIP_SLICE_NONFINITE;
        return;
      }
      if (tx > target) {
        if (lane == ii) gam = prop;
        ll_out = loglik;
        break;
      }
      if (prop < g_ii)
        lower = prop;
      else
        upper = prop;
    }
  }
}

__global__ __launch_bounds__(SG_THREADS) void slice_gamma_kernel(SgArgs A) {
  __shared__ double s_A[SL_MAX_M * SG_LP];
  const int lane = threadIdx.x;
  const int64_t g = blockIdx.x;
  SgState S;
  S.used = 0;
  S.evals = 0;
  S.status = ELFIHIP_SLICE_OK;
  double gam = 0.0, ll = 0.0;
  if (A.adjustment == 0)
    sg_run<0>(A, g, s_A, lane, S, gam, ll);
  else
    sg_run<1>(A, g, s_A, lane, S, gam, ll);
  const bool ok = S.status == ELFIHIP_SLICE_OK;
  if (lane < A.m) A.gamma_out[g * A.m + lane] = ok ? gam : NAN;
  if (lane == 0) {
    A.loglik_out[g] = ok ? ll : NAN;
    A.used[g] = S.used;
    A.evals[g] = S.evals;
    A.status[g] = S.status;
  }
}

static int sg_check(elfihip_ctx* ctx, int adjustment, int64_t G, int m, int64_t ldc, double tau, double w, int64_t max_iter,
                    int64_t n_u) {
  ELFIHIP_REQUIRE(ctx, adjustment == ELFIHIP_SLICE_MEAN || adjustment == ELFIHIP_SLICE_VARIANCE,
                  "adjustment %d: 0 (mean) or 1 (variance)", adjustment);
  ELFIHIP_REQUIRE(ctx, G >= 0 && G <= (int64_t)0x7fffffff, "G=%lld problems: too many for one launch", (long long)G);
  ELFIHIP_REQUIRE(ctx, m >= 1 && m <= SL_MAX_M, "m=%d adjustment parameters: 1 to %d", m, SL_MAX_M);
  ELFIHIP_REQUIRE(ctx, ldc >= m, "leading dimension below the row length");
  ELFIHIP_REQUIRE(ctx, tau > 0.0 && tau <= DBL_MAX, "tau must be positive and finite");
  ELFIHIP_REQUIRE(ctx, w > 0.0 && w <= DBL_MAX, "w must be positive and finite");
  ELFIHIP_REQUIRE(ctx, max_iter >= 0 && max_iter <= SG_MAX_ITER, "max_iter=%lld: 0 to %lld", (long long)max_iter, (long long)SG_MAX_ITER);
  ELFIHIP_REQUIRE(ctx, n_u >= 0, "n_u is negative");
  return ELFIHIP_OK;
}

static int sg_impl(elfihip_ctx* ctx, int adjustment, int64_t G, int m, const double* dy, const double* dmean, const double* dcov,
                   int64_t ldc, const double* dgamma_in, const double* dloglik_in, double tau, double w, int64_t max_iter,
                   const double* dU, int64_t n_u, uint64_t seed, uint64_t stream, double* dgamma_out, double* dloglik_out,
                   int64_t* dused, int64_t* devals, int32_t* dstatus) {
  ELFIHIP_TRY(sg_check(ctx, adjustment, G, m, ldc, tau, w, max_iter, n_u));
  if (G == 0) return ELFIHIP_OK;
  ELFIHIP_REQUIRE(ctx, dy && dmean && dcov && dgamma_in && dloglik_in && dgamma_out && dloglik_out && dused && devals && dstatus,
                  "NULL pointer");
  SgArgs A;
  A.adjustment = adjustment;
  A.m = m;
  A.y = dy;
  A.mean = dmean;
  A.cov = dcov;
  A.ldc = ldc;
  A.gamma_in = dgamma_in;
  A.loglik_in = dloglik_in;
  A.tau = tau;
  A.w = w;
  A.max_iter = max_iter;
  A.U = dU;
  A.n_u = n_u;
  A.seed = seed;
  A.stream = stream;
  A.gamma_out = dgamma_out;
  A.loglik_out = dloglik_out;
  A.used = reinterpret_cast<long long*>(dused);
  A.evals = reinterpret_cast<long long*>(devals);
  A.status = dstatus;
  hipLaunchKernelGGL(slice_gamma_kernel, dim3((unsigned)G), dim3(SG_THREADS), 0, ctx->stream, A);
  return launch_status(ctx, "slice_gamma_kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_slice_gamma_dev(elfihip_ctx* ctx, int adjustment, int64_t G, int m, const double* dy, const double* dmean,
                            const double* dcov, int64_t ldc, const double* dgamma_in, const double* dloglik_in, double tau,
                            double w, int64_t max_iter, const double* dU, int64_t n_u, uint64_t seed, uint64_t stream,
                            double* dgamma_out, double* dloglik_out, int64_t* dused, int64_t* devals, int32_t* dstatus) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return sg_impl(ctx, adjustment, G, m, dy, dmean, dcov, ldc, dgamma_in, dloglik_in, tau, w, max_iter, dU, n_u, seed, stream,
                 dgamma_out, dloglik_out, dused, devals, dstatus);
}

int elfihip_slice_gamma(elfihip_ctx* ctx, int adjustment, int64_t G, int m, const double* y, const double* mean, const double* cov,
                        int64_t ldc, const double* gamma_in, const double* loglik_in, double tau, double w, int64_t max_iter,
                        const double* U, int64_t n_u, uint64_t seed, uint64_t stream, double* gamma_out, double* loglik_out,
                        int64_t* used, int64_t* evals, int32_t* status) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(sg_check(ctx, adjustment, G, m, ldc, tau, w, max_iter, n_u));
  if (G == 0) return ELFIHIP_OK;
  ELFIHIP_REQUIRE(ctx, y && mean && cov && gamma_in && loglik_in && gamma_out && loglik_out && used && evals && status, "NULL pointer");
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)G, gm = n * (size_t)m, D = sizeof(double);
  const size_t nu = U ? n * (size_t)n_u : 0;
  // in: y, mean, gamma (G m each), cov (G m m), loglik (G), U (G n_u); out: gamma (G m), loglik (G), used, evals (G), status (G)
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((3 * gm + gm * (size_t)m + n + nu) * D));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((gm + n) * D + 2 * n * sizeof(int64_t) + n * sizeof(int32_t)));
  double* dy = ctx->in.as<double>();
  double* dmean = dy + gm;
  double* dgam = dmean + gm;
  double* dcov = dgam + gm;
  double* dll = dcov + gm * (size_t)m;
  double* dU = dll + n;
  double* ogam = ctx->out.as<double>();
  double* oll = ogam + gm;
  int64_t* oused = reinterpret_cast<int64_t*>(oll + n);
  int64_t* oevals = oused + n;
  int32_t* ostatus = reinterpret_cast<int32_t*>(oevals + n);
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dy, y, gm * D, hipMemcpyHostToDevice, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dmean, mean, gm * D, hipMemcpyHostToDevice, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dgam, gamma_in, gm * D, hipMemcpyHostToDevice, st));
  ELFIHIP_TRY(upload_rows(ctx, dcov, cov, gm, m, ldc));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dll, loglik_in, n * D, hipMemcpyHostToDevice, st));
  if (nu) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dU, U, nu * D, hipMemcpyHostToDevice, st));
  ELFIHIP_TRY(sg_impl(ctx, adjustment, G, m, dy, dmean, dcov, m, dgam, dll, tau, w, max_iter, U ? dU : nullptr, n_u, seed, stream,
                      ogam, oll, oused, oevals, ostatus));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(gamma_out, ogam, gm * D, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(loglik_out, oll, n * D, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(used, oused, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(evals, oevals, n * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(status, ostatus, n * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
