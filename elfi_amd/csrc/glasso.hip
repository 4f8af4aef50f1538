// Graphical-lasso shrinkage of the synthetic likelihood's covariance (BSLasso, An et al. 2019) on gfx950: B matrices x P
// penalties in one launch.
//
// Replaces sklearn.covariance.graphical_lasso as elfi/methods/bsl/pdf_methods.py:113-120 calls it, and the M x 20 such
// calls of pre_sample_methods.select_penalty (:215-318, its default shrinkage).
//
// Problem: S symmetric positive semi-definite (m x m, m <= 64), alpha >= 0; the W = Theta^-1 that minimises
//     -log det Theta + tr(S Theta) + alpha sum_{i != j} |Theta_ij|            (the diagonal is not penalised: diag W = diag S)
// by block coordinate descent over columns (Friedman, Hastie & Tibshirani 2008): for column j the lasso
//     beta = argmin 1/2 beta' W11 beta - s12' beta + alpha |beta|_1            (W11: W without row and column j)
// by cyclic coordinate descent, then w12 = W11 beta.
//
// One workgroup of ONE wavefront per (matrix, penalty) problem, lane i = row i.
//   LDS        W and the coefficients (row j = column j's beta, kept for the next sweep's warm start), pitch 65 doubles: a
//              row is 64 neighbouring words, a column read walks the banks.  2 m 65 doubles: 65 KiB at m = 64, two problems
//              per CU.
//   column     s12 is one row of S from memory (S is symmetric: row j is read for column j).  Lane i keeps
//              q_i = (W11 beta)_i in a register; coordinate k reads q_k, beta_k, s_k and W_kk from lane k as scalars,
//              soft-thresholds, and every lane applies q_i += delta W_ik -- W is symmetric, so that is the contiguous row
//              k.  Nothing is done for delta == 0: a sparse solution costs what its active set costs.  q is summed from
//              zero at the start and at the end of a column, so w12 carries no drift of the incremental updates.
//   stopping   threshold tol max_i S_ii.  The lasso ends when the largest |delta| W_kk of a sweep is at or below it (or
//              after GL_INNER_SWEEPS sweeps), the descent when the largest change of any w12 entry in a sweep over all
//              columns is (or after max_iter sweeps: status 2).  A value that is not finite ends both at once (status 0).
//   Theta      from the columns, as scikit-learn takes it: theta22 = 1 / (w22 - w12' beta), theta12 = -beta theta22, entry
//              (a, b) from column max(a, b).
//   alpha == 0 or m == 1: W = S, bit for bit (scikit-learn returns emp_cov there); Theta = S^-1 from the Cholesky factor.
//   finish     optionally the Gaussian log-likelihood of y under N(mean, W): the factorisation of W in place (lane i = row
//              i, left-looking; synlik.hip's chol_extra_row is written for 256 threads), the forward solve of the residual,
//              the log-determinant.  A pivot that is not positive gives -inf.
// Every problem starts from scikit-learn's start (W = S with the off-diagonal scaled by 0.95, beta = 0): no warm start
// from a neighbouring penalty, so a problem's result does not depend on what else is in the call.  Everything that decides
// control flow is a scalar read from one lane or a reduction with the same bits in every lane (DPP inside a row of 16
// lanes, the four rows in a fixed order): no loop has a divergent exit.  No atomics, FMA contraction off.  The only
// synchronisation is the LDS fence after a column's write-back (a workgroup of one wavefront has no barrier to wait at).
//
// The statement is in include/elfihip.h and, in NumPy, in tests/glasso_ref.py.
#include "common.hpp"

#include <cfloat>
#include <cmath>

#include "syn_gram.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int GL_THREADS = 64;           // one wavefront
constexpr int GL_LP = SL_MAX_M + 1;      // pitch of the LDS matrices
constexpr int GL_INNER_SWEEPS = 1000;    // cap of the lasso's sweeps for one column
constexpr int GL_MAX_ITER = 1 << 20;

struct GlArgs {
  const double* S;          // (B, m, lds): matrix b at S + b sstride
  int64_t lds, sstride;
  int m, P, standardise, max_iter;
  const double* alphas;     // (P)
  double tol;
  double* W;                // (B, P, m, m) or NULL
  double* Theta;            // (B, P, m, m) or NULL
  int32_t* n_iter;          // (B, P) or NULL
  int32_t* status;          // (B, P)
  // the likelihood finish; loglik NULL: the solver alone
  const double* mean;       // (B, m)
  const double* y;          // (m)
  const double* Wh;         // (m, m) whitening or NULL: y -> Wh y
  double* loglik;           // (B, P)
};

// (the three reads below are slice_gamma.hip's sg_lane / sg_sum64, restated: that file's instructions stay as they are)
// the value lane `src` holds (src the same in every lane), as a scalar
__device__ __forceinline__ double gl_lane(double v, int src) {
  const int s = __builtin_amdgcn_readfirstlane(src);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), s), __builtin_amdgcn_readlane(__double2loint(v), s));
}
// the sum over the 64 lanes, the same bits in every lane: each row of 16 by DPP, then (r0 + r1) + (r2 + r3)
__device__ __forceinline__ double gl_sum64(double v) {
  v = lanes16_sum(v);
  return (gl_lane(v, 0) + gl_lane(v, 16)) + (gl_lane(v, 32) + gl_lane(v, 48));
}
// the larger of two, a NaN of either wins (fmax would drop it)
__device__ __forceinline__ double gl_max(double a, double b) { return (a >= b || a != a) ? a : b; }
// the largest over the 64 lanes, a NaN in any lane wins; the same bits in every lane
__device__ __forceinline__ double gl_max64(double v) {
  v = gl_max(v, dpp_move_f64<0xB1>(v));    // quad_perm [1, 0, 3, 2]
  v = gl_max(v, dpp_move_f64<0x4E>(v));    // quad_perm [2, 3, 0, 1]
  v = gl_max(v, dpp_move_f64<0x141>(v));   // row_half_mirror
  v = gl_max(v, dpp_move_f64<0x140>(v));   // row_mirror
  return gl_max(gl_max(gl_lane(v, 0), gl_lane(v, 16)), gl_max(gl_lane(v, 32), gl_lane(v, 48)));
}
__device__ __forceinline__ bool gl_finite(double v) { return v - v == 0.0; }

// (W11 beta)_lane summed from zero in the order of k: row k of the symmetric W for every beta_k that is not zero.  beta is
// zero in lane j and beyond m, so row and column j stay out; what lane j itself receives is not used.
__device__ __forceinline__ double gl_matvec(const double* Wm, int m, int lane, double beta) {
  double q = 0.0;
  for (int k = 0; k < m; ++k) {
    const double bk = gl_lane(beta, k);
    if (bk != 0.0) q += bk * Wm[k * GL_LP + lane];
  }
  return q;
}

// Left-looking Cholesky factorisation in place of the matrix whose strict lower triangle is in A and whose diagonal entry
// i lane i holds in `diag`: on return lane i holds the factor's diagonal entry in dg and L[i][k], k < i, is at A[k][i].
// false (in every lane) at the first pivot that is not positive.
__device__ __forceinline__ bool gl_factor(double* A, int m, int lane, double diag, double& dg) {
  dg = 1.0;
  for (int j = 0; j < m; ++j) {
    double s = lane == j ? diag : (lane > j && lane < m ? A[lane * GL_LP + j] : 0.0);
    if (lane >= j && lane < m) {
#pragma unroll 8
      for (int k = 0; k < j; ++k) s -= A[k * GL_LP + lane] * A[k * GL_LP + j];
    }
    const double piv = gl_lane(s, j);
    if (!(piv > 0.0)) return false;
    const double d = sqrt(piv);
    if (lane == j) dg = d;
    if (lane > j && lane < m) A[j * GL_LP + lane] = s / d;
    __syncthreads();
  }
  return true;
}

// b <- L^-1 b by columns: lane i gives its entry of the right-hand side and receives the solution's
__device__ __forceinline__ void gl_forward(const double* A, int m, int lane, double dg, double& b) {
  for (int j = 0; j < m; ++j) {
    const double xj = gl_lane(b, j) / gl_lane(dg, j);
    if (lane == j) b = xj;
    if (lane > j && lane < m) b -= A[j * GL_LP + lane] * xj;
  }
}

// b <- L^-T b: L[j][i], i < j, is at A[i][j]
__device__ __forceinline__ void gl_backward(const double* A, int m, int lane, double dg, double& b) {
  for (int j = m - 1; j >= 0; --j) {
    const double xj = gl_lane(b, j) / gl_lane(dg, j);
    if (lane == j) b = xj;
    if (lane < j) b -= A[lane * GL_LP + j] * xj;
  }
}

__global__ __launch_bounds__(GL_THREADS) void glasso_kernel(GlArgs A) {
  extern __shared__ __align__(16) double gl_lds[];
  const int lane = threadIdx.x, m = A.m;
  double* Wm = gl_lds;                 // (m, GL_LP) W, symmetric; at the end its upper triangle takes the Cholesky factor
  double* Bc = gl_lds + m * GL_LP;     // (m, GL_LP) row j: beta of column j
  const bool in = lane < m;
  const int64_t b = blockIdx.x / A.P, prob = blockIdx.x;
  const double alpha = A.alphas[blockIdx.x - b * A.P];
  const double* Sg = A.S + b * A.sstride;
  const bool scaled = A.standardise != 0;

  // the problem's matrix: S, or with `standardise` S_ij / (sd_i sd_j)
  const double sraw = in ? Sg[(int64_t)lane * A.lds + lane] : 1.0;
  const double sd = scaled ? sqrt(sraw) : 1.0;
  auto entry = [&](int r) -> double {      // entry (r, lane), lane < m
    const double v = Sg[(int64_t)r * A.lds + lane];
    return scaled ? v / (sd * gl_lane(sd, r)) : v;
  };
  const bool plain = alpha == 0.0 || m == 1;      // W = S
  double diag = 0.0;
  for (int r = 0; r < m; ++r) {
    if (in) {
      const double v = entry(r);
      if (lane == r) diag = v;
      Wm[r * GL_LP + lane] = (lane == r || plain) ? v : v * 0.95;
      Bc[r * GL_LP + lane] = 0.0;
    }
  }
  __syncthreads();
  const double thr = A.tol * gl_max64(in ? diag : 0.0);

  int it = 0, status = 1;
  if (!plain) {
    status = 2;
    while (it < A.max_iter) {
      double change = 0.0;
      for (int j = 0; j < m; ++j) {
        const bool act = in && lane != j;
        const double s = act ? entry(j) : 0.0;
        double beta = act ? Bc[j * GL_LP + lane] : 0.0;
        double q = gl_matvec(Wm, m, lane, beta);
        for (int sweep = 0; sweep < GL_INNER_SWEEPS; ++sweep) {
          double step = 0.0;
          for (int k = 0; k < m; ++k) {
            if (k == j) continue;
            const double wkk = gl_lane(diag, k), bk = gl_lane(beta, k);
            const double r = gl_lane(s, k) - (gl_lane(q, k) - wkk * bk);      // s_k - sum_{l != k} W_kl beta_l
            const double t = fabs(r) - alpha;
            const double nb = t > 0.0 ? copysign(t, r) / wkk : (t == t ? 0.0 : t);
            const double d = nb - bk;
            if (d != 0.0) {
              q += d * Wm[k * GL_LP + lane];
              if (lane == k) beta = nb;
              step = gl_max(step, fabs(d) * wkk);
            }
          }
          if (!(step > thr)) break;      // converged, or not a number
        }
        q = gl_matvec(Wm, m, lane, beta);
        change = gl_max(change, gl_max64(act ? fabs(q - Wm[j * GL_LP + lane]) : 0.0));
        if (act) {
          Wm[j * GL_LP + lane] = q;
          Wm[lane * GL_LP + j] = q;
          Bc[j * GL_LP + lane] = beta;
        }
        __syncthreads();
      }
      ++it;
      if (!(change > thr)) {
        status = gl_finite(change) ? 1 : 0;
        break;
      }
    }
  }

  const int64_t mm = (int64_t)m * m;
  if (A.W && in)
    for (int r = 0; r < m; ++r) A.W[prob * mm + (int64_t)r * m + lane] = Wm[r * GL_LP + lane];

  // Theta and the status from the columns
  double* Th = A.Theta ? A.Theta + prob * mm : nullptr;
  if (!plain) {
    bool good = true;
    for (int j = 0; j < m; ++j) {
      const bool act = in && lane != j;
      const double beta = act ? Bc[j * GL_LP + lane] : 0.0;
      const double t22 = 1.0 / (gl_lane(diag, j) - gl_sum64(act ? Wm[j * GL_LP + lane] * beta : 0.0));
      good = good && t22 > 0.0 && gl_finite(t22);
      if (Th) {
        if (lane == j) Th[(int64_t)j * m + j] = t22;
        if (lane < j) {
          const double t12 = -beta * t22;
          Th[(int64_t)j * m + lane] = t12;
          Th[(int64_t)lane * m + j] = t12;
        }
      }
    }
    if (!good) status = 0;
  }

  // the factor of W: Theta = S^-1 of the plain case, the likelihood
  double ll = -INFINITY;
  if (plain || A.loglik) {
    __syncthreads();
    double dg;
    const bool ok = gl_factor(Wm, m, lane, diag, dg);
    if (plain) {
      status = ok ? 1 : 0;
      if (Th && in)
        for (int c = 0; c < m; ++c) {
          double x = ok ? (lane == c ? 1.0 : 0.0) : NAN;
          if (ok) {
            gl_forward(Wm, m, lane, dg, x);
            gl_backward(Wm, m, lane, dg, x);
          }
          Th[(int64_t)c * m + lane] = x;
        }
    }
    if (A.loglik && ok) {
      double yw = 0.0;
      if (in) {
        if (A.Wh) {
          const double* w = A.Wh + (int64_t)lane * m;
          for (int k = 0; k < m; ++k) yw += w[k] * A.y[k];
        } else {
          yw = A.y[lane];
        }
      }
      double z = in ? yw - A.mean[b * m + lane] : 0.0;
      gl_forward(Wm, m, lane, dg, z);
      const double quad = gl_sum64(in ? z * z : 0.0);
      const double logdet = 2.0 * gl_sum64(in ? log(dg) : 0.0);
      ll = -0.5 * (((double)m * 1.8378770664093453 + logdet) + quad);
      if (!gl_finite(ll)) ll = -INFINITY;
    }
  }
  if (lane == 0) {
    if (A.loglik) A.loglik[prob] = ll;
    if (A.n_iter) A.n_iter[prob] = it;
    A.status[prob] = status;
  }
}

static int gl_check(elfihip_ctx* ctx, int64_t B, int m, int64_t ld, const double* alphas, int P, double tol, int max_iter) {
  ELFIHIP_REQUIRE(ctx, m >= 1 && m <= SL_MAX_M, "graphical lasso: a %d x %d matrix; 1 to %d rows are supported", m, m, SL_MAX_M);
  ELFIHIP_REQUIRE(ctx, B >= 1 && ld >= m, "bad shape B=%lld m=%d ld=%lld", (long long)B, m, (long long)ld);
  ELFIHIP_REQUIRE(ctx, alphas && P >= 1, "graphical lasso needs at least one penalty");
  ELFIHIP_REQUIRE(ctx, B * (int64_t)P <= 0x7fffffff, "B=%lld x P=%d problems: too many for one launch", (long long)B, P);
  for (int p = 0; p < P; ++p)
    ELFIHIP_REQUIRE(ctx, alphas[p] >= 0.0 && alphas[p] <= DBL_MAX, "penalty %d is negative or not finite", p);
  ELFIHIP_REQUIRE(ctx, tol > 0.0 && tol <= DBL_MAX, "tol must be positive and finite");
  ELFIHIP_REQUIRE(ctx, max_iter >= 1 && max_iter <= GL_MAX_ITER, "max_iter=%d: 1 to %d", max_iter, GL_MAX_ITER);
  return ELFIHIP_OK;
}

// The penalties go to `dalphas` (device, P doubles) from pageable host memory (common.hpp: pageable uploads), then the launch.
static int gl_launch(elfihip_ctx* ctx, GlArgs& A, int64_t B, const double* alphas, double* dalphas) {
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dalphas, alphas, (size_t)A.P * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  A.alphas = dalphas;
  const size_t lds = 2 * (size_t)A.m * GL_LP * sizeof(double);
  ELFIHIP_TRY(set_lds(ctx, glasso_kernel, lds, 48 * 1024));
  hipLaunchKernelGGL(glasso_kernel, dim3((unsigned)(B * A.P)), dim3(GL_THREADS), lds, ctx->stream, A);
  return launch_status(ctx, "graphical lasso kernel");
}

static int gl_solve_dev(elfihip_ctx* ctx, const double* dS, int64_t B, int m, int64_t lds, const double* alphas, int P, double tol,
                        int max_iter, double* dW, double* dTheta, int32_t* dn_iter, int32_t* dstatus) {
  ELFIHIP_CHECK_HIP(ctx, ctx->par.reserve((size_t)P * sizeof(double)));
  GlArgs A = {};
  A.S = dS;
  A.lds = lds;
  A.sstride = (int64_t)m * lds;
  A.m = m;
  A.P = P;
  A.max_iter = max_iter;
  A.tol = tol;
  A.W = dW;
  A.Theta = dTheta;
  A.n_iter = dn_iter;
  A.status = dstatus;
  return gl_launch(ctx, A, B, alphas, ctx->par.as<double>());
}

static int gl_loglik_check(elfihip_ctx* ctx, const void* X, int64_t G, int64_t n, int m, int64_t ldx, const void* y,
                           const double* alphas, int P, double tol, int max_iter, const void* loglik, const void* status) {
  ELFIHIP_TRY(gl_check(ctx, G, m, ldx, alphas, P, tol, max_iter));
  ELFIHIP_REQUIRE(ctx, G <= 0x7fffffff && n >= 2, "bad shape G=%lld n=%lld m=%d ldx=%lld", (long long)G, (long long)n, m,
                  (long long)ldx);
  ELFIHIP_REQUIRE(ctx, X && y && loglik && status, "NULL data pointer");
  return ELFIHIP_OK;
}

// The group moments from the synthetic-likelihood kernel (synlik.hip) into the context's `sel` work space -- `scratch` is
// that call's own, for the whitened rows -- then one problem per (group, penalty).
static int gl_loglik_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                         const double* dWh, const double* alphas, int P, int standardise, double tol, int max_iter,
                         double* dll, int32_t* dstatus, double* dmean, double* dcov) {
  const size_t g = (size_t)G, gm = g * m, gmm = gm * m;
  // sel: [loglik without shrinkage G][mean G m][cov G m m][alphas P]
  ELFIHIP_CHECK_HIP(ctx, ctx->sel.reserve((g + gm + gmm + (size_t)P) * sizeof(double)));
  double* ll0 = ctx->sel.as<double>();
  double* smean = ll0 + g;
  double* scov = smean + gm;
  ELFIHIP_TRY(elfihip_syn_loglik_dev(ctx, dX, G, n, m, ldx, dy, dWh, 0, nullptr, nullptr, 0, nullptr, 0, ll0, smean, scov));
  GlArgs A = {};
  A.S = scov;
  A.lds = m;
  A.sstride = (int64_t)m * m;
  A.m = m;
  A.P = P;
  A.standardise = standardise ? 1 : 0;
  A.max_iter = max_iter;
  A.tol = tol;
  A.W = dcov;
  A.status = dstatus;
  A.mean = smean;
  A.y = dy;
  A.Wh = dWh;
  A.loglik = dll;
  ELFIHIP_TRY(gl_launch(ctx, A, G, alphas, scov + gmm));
  if (dmean) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dmean, smean, gm * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  return ELFIHIP_OK;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_graphical_lasso_dev(elfihip_ctx* ctx, const double* dS, int64_t B, int m, int64_t lds, const double* alphas, int P,
                                double tol, int max_iter, double* dW, double* dTheta, int32_t* dn_iter, int32_t* dstatus) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(gl_check(ctx, B, m, lds, alphas, P, tol, max_iter));
  ELFIHIP_REQUIRE(ctx, dS && dW && dstatus, "NULL data pointer");
  DeviceGuard g(ctx->device);
  return gl_solve_dev(ctx, dS, B, m, lds, alphas, P, tol, max_iter, dW, dTheta, dn_iter, dstatus);
}

int elfihip_graphical_lasso(elfihip_ctx* ctx, const double* S, int64_t B, int m, int64_t lds, const double* alphas, int P,
                            double tol, int max_iter, double* W, double* Theta, int32_t* n_iter, int32_t* status) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(gl_check(ctx, B, m, lds, alphas, P, tol, max_iter));
  ELFIHIP_REQUIRE(ctx, S && W && status, "NULL data pointer");
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t bmm = (size_t)B * m * m, bp = (size_t)B * P, D = sizeof(double);
  // in: [S B m m]; out: [W B P m m][Theta B P m m][n_iter B P][status B P]
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(bmm * D));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(2 * bmm * P * D + 2 * bp * sizeof(int32_t)));
  double* dS = ctx->in.as<double>();
  double* dW = ctx->out.as<double>();
  double* dTheta = dW + bmm * P;
  int32_t* dit = reinterpret_cast<int32_t*>(dTheta + bmm * P);
  int32_t* dstat = dit + bp;
  ELFIHIP_TRY(upload_rows(ctx, dS, S, (size_t)B * m, m, lds));
  ELFIHIP_TRY(gl_solve_dev(ctx, dS, B, m, m, alphas, P, tol, max_iter, dW, Theta ? dTheta : nullptr, n_iter ? dit : nullptr,
                           dstat));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(W, dW, bmm * P * D, hipMemcpyDeviceToHost, st));
  if (Theta) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Theta, dTheta, bmm * P * D, hipMemcpyDeviceToHost, st));
  if (n_iter) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(n_iter, dit, bp * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(status, dstat, bp * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

int elfihip_syn_loglik_glasso_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                                  const double* dWh, const double* alphas, int P, int standardise, double tol, int max_iter,
                                  double* dloglik, int32_t* dstatus, double* dmean, double* dcov) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(gl_loglik_check(ctx, dX, G, n, m, ldx, dy, alphas, P, tol, max_iter, dloglik, dstatus));
  DeviceGuard g(ctx->device);
  return gl_loglik_dev(ctx, dX, G, n, m, ldx, dy, dWh, alphas, P, standardise, tol, max_iter, dloglik, dstatus, dmean, dcov);
}

int elfihip_syn_loglik_glasso(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* y,
                              const double* Wh, const double* alphas, int P, int standardise, double tol, int max_iter,
                              double* loglik, int32_t* status, double* mean, double* cov) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(gl_loglik_check(ctx, X, G, n, m, ldx, y, alphas, P, tol, max_iter, loglik, status));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)G * (size_t)n, md = (size_t)m * sizeof(double), gp = (size_t)G * P, D = sizeof(double);
  // in: [X rows m][y m][Wh m m]; out: [loglik G P][mean G m][cov G P m m][status G P]
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((rows * m + (size_t)m + (size_t)m * m) * D));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((gp + (size_t)G * m + gp * m * m) * D + gp * sizeof(int32_t)));
  double* dX = ctx->in.as<double>();
  double* dy = dX + rows * m;
  double* dWh = dy + m;
  double* dll = ctx->out.as<double>();
  double* dmean = dll + gp;
  double* dcov = dmean + (size_t)G * m;
  int32_t* dstat = reinterpret_cast<int32_t*>(dcov + gp * m * m);
  ELFIHIP_TRY(upload_rows(ctx, dX, X, rows, m, ldx));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dy, y, md, hipMemcpyHostToDevice, st));
  if (Wh) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dWh, Wh, (size_t)m * md, hipMemcpyHostToDevice, st));
  ELFIHIP_TRY(gl_loglik_dev(ctx, dX, G, n, m, m, dy, Wh ? dWh : nullptr, alphas, P, standardise, tol, max_iter, dll, dstat,
                            mean ? dmean : nullptr, cov ? dcov : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(loglik, dll, gp * D, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(status, dstat, gp * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (mean) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(mean, dmean, (size_t)G * md, hipMemcpyDeviceToHost, st));
  if (cov) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(cov, dcov, gp * m * md, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
