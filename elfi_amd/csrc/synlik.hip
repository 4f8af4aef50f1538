// Batched Gaussian synthetic likelihood (BSL) on gfx950.
//
// Replaces, for G groups of n simulated summary rows at once, what elfi/methods/bsl/pdf_methods.py does per call:
//   gaussian_syn_likelihood (:77-135)              mean, np.cov, optional Warton shrinkage (cov_warton.py:6-30), MVN logpdf
//   gaussian_syn_likelihood_ghurye_olkin (:138-176) the unbiased estimator
//   syn_likelihood_misspec (:267-316)              mean- or variance-adjusted
// and what log_SL_stdev / select_penalty (pre_sample_methods.py:102-143, 215-318) loop over: prefixes of the same rows
// and a list of penalties.
//
// One workgroup of 256 threads owns one group.
//   moments    d_i = x_i - c with c the group's first row (a shift taken from the data: the sums stay of the size of the
//              spread, not of the offset).  S1 = sum d_i by plain adds, S2 = sum d_i d_i^T by v_mfma_f64_16x16x4_f64: the
//              four k of one instruction are four consecutive rows, the 16 x 16 tiles of the (padded) m x m matrix are
//              dealt to the four waves.  Rows are staged 32 at a time in LDS; every chunk is summed from zero and then
//              added to the running total (two-level summation: the error grows with n / 32 + 32, not n).
//   prefixes   one pass serves all K prefixes: at a boundary p the sums of the rows before p are snapshotted.  The order of
//              the additions of a row depends on its index alone -- a boundary inside a 4-row MFMA step is served by an
//              extra, masked MFMA into a temporary, the running sums go on with the whole step -- so prefix p of a long
//              group has the bits of a group of p rows.
//   finish     at every boundary, in LDS: covariance, then per penalty the shrunk / adjusted matrix, its Cholesky factor
//              with the residual y - mean as an extra row (the forward solve rides along), the log-determinant and the
//              quadratic form.  A non-positive pivot or a non-finite value gives -inf.
// Whitening (rows -> rows W^T, y -> W y) is a launch of its own in front.
// Determinism: no atomics, fixed order everywhere; a group's result does not depend on G.
// The shape of the LDS buffers, the MFMA step and the factorisation are shared with semibsl.hip and logratio.hip
// (syn_gram.hpp); the check of the lists and their parameter block with semibsl.hip (group_args.hpp).
#include "common.hpp"
#include "syn_gram.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace elfihip {

struct SynArgs {
  const double* X;          // (G n, m), pitch ldx
  int64_t n, ldx;
  int m, variant;
  const double* y;          // (m), whitened
  const double* gamma;      // (m) or NULL (variants 2, 3)
  const int64_t* prefixes;  // (K) ascending, last == n
  const double* penalties;  // (P) or NULL
  const double* konst;      // (K): variant 1, the terms that depend on (m, prefix) alone
  int K, P;
  double* loglik;           // (G, K, max(P, 1))
  double* mean;             // (G, m) or NULL
  double* cov;              // (G, m, m) or NULL
};

template <int T>
struct SynShape : GramShape<T> {
  using GramShape<T>::MP;
  using GramShape<T>::SP;
  using GramShape<T>::LP;
  static constexpr int DOUBLES = SL_RC * SP + MP * LP + (MP + 1) * LP + 6 * MP;
  static_assert(DOUBLES * sizeof(double) <= 160 * 1024);
};

// rows -> rows W^T (sequential k), one output element per thread and step
__global__ __launch_bounds__(256) void synlik_whiten_kernel(const double* X, int64_t rows, int m, int64_t ldx,
                                                            const double* W, const double* y, double* Xw, double* yw) {
  const int64_t total = rows * m;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / m;
    const int j = (int)(e - r * m);
    const double* x = X + r * ldx;
    const double* w = W + (int64_t)j * m;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += x[k] * w[k];
    Xw[e] = s;
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < m) {
    const double* w = W + (int64_t)threadIdx.x * m;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += w[k] * y[k];
    yw[threadIdx.x] = s;
  }
}

// The log-likelihoods of prefix kb (np rows) for every penalty; S holds S2, s1 holds S1 of the shifted rows.  All 256
// threads; ends with a barrier.
template <int T>
__device__ void synlik_finish(const SynArgs& A, int g, int kb, int64_t np, double* S, double* L, const double* cs,
                              const double* s1, const double* yd, double* sd, double* dg, double* ws) {
  constexpr int LP = SynShape<T>::LP;
  const int tid = threadIdx.x, m = A.m;
  const int tx = tid & 15, ty = tid >> 4;
  const double dn = (double)np;
  for (int i = ty; i < m; i += 16)
    for (int j = tx; j < m; j += 16) S[i * LP + j] = (S[i * LP + j] - s1[i] * s1[j] / dn) / (dn - 1.0);
  __syncthreads();
  if (tid < m) sd[tid] = sqrt(S[tid * LP + tid]);
  if (np == A.n) {  // the full group: the moments BSL keeps for the gamma sampler
    if (A.mean && tid < m) A.mean[(int64_t)g * m + tid] = cs[tid] + s1[tid] / dn;
    if (A.cov)
      for (int i = ty; i < m; i += 16)
        for (int j = tx; j < m; j += 16) A.cov[((int64_t)g * m + i) * m + j] = S[i * LP + j];
  }
  const int Pe = A.P > 0 ? A.P : 1;
  for (int pi = 0; pi < Pe; ++pi) {
    __syncthreads();
    // cov_warton(S, 1 - penalty) as written: eps inside both diagonal scalings
    const double gam = A.P > 0 ? 1.0 - A.penalties[pi] : 1.0;
    if (A.P > 0 && tid < m) ws[tid] = sqrt(S[tid * LP + tid] + 1e-5);
    __syncthreads();
    for (int i = ty; i < m; i += 16)
      for (int j = tx; j <= i; j += 16) {
        double v = S[i * LP + j];
        if (A.P > 0) {
          const double d1i = 1.0 / ws[i], d1j = 1.0 / ws[j];
          const double r = (d1i * v) * d1j;
          const double rg = gam * r + (i == j ? (1.0 - gam) : 0.0);
          v = (ws[i] * rg) * ws[j];
        }
        if (A.variant == 3 && i == j) {
          const double a = sd[i] * A.gamma[i];
          v += a * a;
        }
        L[i * LP + j] = v;
      }
    if (tid < m) {  // the residual y - mean as row m of the factor: its forward solve is the factorisation's own update
      double v = yd[tid] - s1[tid] / dn;
      if (A.variant == 2) v -= sd[tid] * A.gamma[tid];
      L[m * LP + tid] = v;
    }
    __syncthreads();
    const bool ok = chol_extra_row<LP>(L, dg, m);
    if (tid == 0) {
      double ll = -INFINITY;
      if (ok) {
        double quad = 0.0, logdet = 0.0;
        for (int j = 0; j < m; ++j) {
          const double z = L[m * LP + j];
          quad += z * z;
          logdet += log(dg[j]);
        }
        logdet *= 2.0;
        if (A.variant == 1) {
          // psi = (n - 1) S - v v^T / (1 - 1/n): det psi = (n - 1)^m det S (1 - v^T S^-1 v / ((n - 1)(1 - 1/n)))
          const double t = 1.0 - quad / ((dn - 1.0) * (1.0 - 1.0 / dn));
          if (t > 0.0) {
            const double logdet_psi = m * log(dn - 1.0) + logdet + log(t);
            const double B = -0.5 * (dn - m - 2.0) * (log(dn - 1.0) + logdet);
            const double C = 0.5 * (dn - m - 3.0) * logdet_psi;
            ll = A.konst[kb] + B + C;
          }
        } else {
          ll = -0.5 * (m * 1.8378770664093453 + logdet + quad);
        }
        if (!(fabs(ll) <= 1.7976931348623157e308)) ll = -INFINITY;   // NaN or an infinity of either sign
      }
      A.loglik[((int64_t)g * A.K + kb) * Pe + pi] = ll;
    }
  }
  __syncthreads();
}

template <int T>
__global__ __launch_bounds__(256) void synlik_kernel(SynArgs A) {
  using Sh = SynShape<T>;
  constexpr int MP = Sh::MP, SP = Sh::SP, LP = Sh::LP, NT = Sh::NT;
  extern __shared__ __align__(16) double lds[];
  double* stage = lds;                  // (SL_RC, SP) shifted rows, zero beyond n and beyond m
  double* S = stage + SL_RC * SP;       // (MP, LP) snapshot of S2, then the covariance
  double* L = S + MP * LP;              // (MP + 1, LP) the matrix being factorised + the residual row
  double* cs = L + (MP + 1) * LP;       // shift
  double* s1 = cs + MP;                 // snapshot of S1
  double* yd = s1 + MP;                 // y - shift
  double* sd = yd + MP;                 // sqrt(diag cov)
  double* dg = sd + MP;                 // diagonal of the factor
  double* ws = dg + MP;                 // Warton's diagonal scaling
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = A.m;
  const int g = blockIdx.x;
  const double* Xg = A.X + (int64_t)g * A.n * A.ldx;
  if (tid < MP) cs[tid] = tid < m ? Xg[tid] : 0.0;
  __syncthreads();
  if (tid < MP) yd[tid] = tid < m ? A.y[tid] - cs[tid] : 0.0;

  v4d tot[NT], chk[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) tot[i] = (v4d){0.0, 0.0, 0.0, 0.0};
  double s1tot = 0.0, s1chk = 0.0;
  const int lr = lane >> 4, lc = lane & 15;
  int kb = 0;  // next boundary
  int64_t nextp = A.prefixes[0];
  for (int64_t r0 = 0; r0 < A.n; r0 += SL_RC) {
    __syncthreads();  // the previous chunk is consumed
    for (int e = tid; e < SL_RC * MP; e += 256) {
      const int rr = e / MP, c = e - rr * MP;
      const int64_t r = r0 + rr;
      double v = 0.0;
      if (r < A.n && c < m) v = Xg[r * A.ldx + c] - cs[c];
      stage[rr * SP + c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NT; ++i) chk[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    s1chk = 0.0;
    const int nr = (int)(A.n - r0 < SL_RC ? A.n - r0 : SL_RC);
    for (int s = 0; 4 * s < nr; ++s) {
      const int64_t g0 = r0 + 4 * s;
      const double* row = stage + (4 * s + lr) * SP + lc;
      // boundaries in (g0, g0 + 4]: the sums of the rows before the boundary, without disturbing the running ones
      while (kb < A.K && nextp <= g0 + 4) {
        const int64_t np = nextp;
        const int cut = (int)(np - g0);   // rows of this step that count: 1 .. 4
#pragma unroll
        for (int i = 0; i < NT; ++i) {
          const int q = wv + 4 * i;
          if (q < T * T) {
            const int ti = q / T, tj = q - ti * T;
            const double a = lr < cut ? row[16 * ti] : 0.0;
            const double b = lr < cut ? row[16 * tj] : 0.0;
            const v4d tmp = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, chk[i], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(16 * ti + lr + 4 * r) * LP + 16 * tj + lc] = tot[i][r] + tmp[r];
          }
        }
        if (tid < MP) {
          double t1 = s1chk;
          for (int rr = 0; rr < cut; ++rr) t1 += stage[(4 * s + rr) * SP + tid];
          s1[tid] = s1tot + t1;
        }
        __syncthreads();
        synlik_finish<T>(A, g, kb, np, S, L, cs, s1, yd, sd, dg, ws);
        ++kb;
        nextp = kb < A.K ? A.prefixes[kb] : 0;
      }
      gram_step<T>(chk, row, wv);
      if (tid < MP)
        for (int rr = 0; rr < 4; ++rr) s1chk += stage[(4 * s + rr) * SP + tid];
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) tot[i] += chk[i];
    s1tot += s1chk;
  }
}

// log c(d, n - 2) - log c(d, n - 1) - d/2 log(1 - 1/n) - d/2 log(2 pi) of Ghurye & Olkin's unbiased estimator
// (pdf_methods.py:168-171, wcon :319-341); NaN where a gamma function's argument is not positive (n <= d + 1)
static double unbiased_const(int d, int64_t n) {
  if (n <= (int64_t)d + 1) return NAN;
  long double a = 0.5L * d * logl(2.0L);
  for (int x = 0; x < d; ++x) a -= lgammal(0.5L * (long double)(n - 2 - x)) - lgammal(0.5L * (long double)(n - 1 - x));
  a -= 0.5L * d * logl(1.0L - 1.0L / (long double)n);
  a -= 0.5L * d * logl(2.0L * 3.14159265358979323846264338327950288L);
  return (double)a;
}

static int synlik_check(elfihip_ctx* ctx, const void* X, int64_t G, int64_t n, int m, int64_t ldx, const void* y,
                        int variant, const void* gamma_adj, const int64_t* prefixes, int K, const double* penalties, int P,
                        const void* loglik) {
  ELFIHIP_REQUIRE(ctx, m >= 1 && m <= SL_MAX_M, "synthetic likelihood: %d summaries; 1 to %d are supported", m, SL_MAX_M);
  ELFIHIP_REQUIRE(ctx, G >= 1 && G <= 0x7fffffff && n >= 2 && ldx >= m, "bad shape G=%lld n=%lld m=%d ldx=%lld",
                  (long long)G, (long long)n, m, (long long)ldx);
  ELFIHIP_REQUIRE(ctx, X && y && loglik, "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, variant >= 0 && variant <= 3, "unknown variant %d", variant);
  ELFIHIP_REQUIRE(ctx, variant < 2 || gamma_adj, "variant %d needs gamma_adj", variant);
  ELFIHIP_REQUIRE(ctx, !(penalties && P >= 1) || variant == 0, "penalties go with the standard variant only (variant %d)",
                  variant);
  const std::string bad = group_lists_error(prefixes, K, penalties, P, n);
  ELFIHIP_REQUIRE(ctx, bad.empty(), "%s", bad.c_str());
  return ELFIHIP_OK;
}

// Device rows, y, W, gamma and outputs; host prefixes and penalties (checked above).
static int synlik_dev_impl(elfihip_ctx* ctx, const double* dX, int G, int64_t n, int m, int64_t ldx, const double* dy,
                           const double* dW, int variant, const double* dgamma, const int64_t* prefixes, int K,
                           const double* penalties, int P, double* dll, double* dmean, double* dcov) {
  hipStream_t st = ctx->stream;
  const int Ke = prefixes ? K : 1;
  std::vector<double> konst(Ke);
  for (int k = 0; k < Ke; ++k) konst[k] = variant == 1 ? unbiased_const(m, prefixes ? prefixes[k] : n) : 0.0;
  // parameter block: [prefixes Ke][konst Ke][penalties P], and behind it on the device [yw m]
  const GroupParams B = group_params(prefixes, K, n, konst.data(), penalties, P);
  ELFIHIP_CHECK_HIP(ctx, ctx->par.reserve((B.words.size() + m) * sizeof(double)));
  double* dpar = ctx->par.as<double>();
  // pageable host memory: the copy is done with it when hipMemcpyAsync returns (common.hpp: pageable uploads)
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar, B.words.data(), B.words.size() * sizeof(double), hipMemcpyHostToDevice, st));
  SynArgs A;
  A.X = dX;
  A.n = n;
  A.ldx = ldx;
  A.m = m;
  A.variant = variant;
  A.y = dy;
  A.gamma = dgamma;
  A.prefixes = reinterpret_cast<const int64_t*>(dpar);
  A.konst = dpar + B.konst;
  A.penalties = P > 0 ? dpar + B.pen : nullptr;
  A.K = Ke;
  A.P = P;
  A.loglik = dll;
  A.mean = dmean;
  A.cov = dcov;
  if (dW) {
    const int64_t rows = (int64_t)G * n;
    ELFIHIP_CHECK_HIP(ctx, ctx->scratch.reserve((size_t)rows * m * sizeof(double)));
    double* dXw = ctx->scratch.as<double>();
    double* dyw = dpar + B.words.size();
    const int64_t want = (rows * m + 255) / 256;
    const int grid = (int)std::min<int64_t>(std::max<int64_t>(want, 1), (int64_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(synlik_whiten_kernel, dim3(grid), dim3(256), 0, st, dX, rows, m, ldx, dW, dy, dXw, dyw);
    ELFIHIP_TRY(launch_status(ctx, "whitening kernel"));
    A.X = dXw;
    A.ldx = m;
    A.y = dyw;
  }
  return launch_by_tiles(
      ctx, m, (unsigned)G, "synthetic likelihood kernel", [](auto T) { return synlik_kernel<decltype(T)::value>; },
      [](auto T) { return (size_t)SynShape<decltype(T)::value>::DOUBLES * sizeof(double); }, A);
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_syn_loglik_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                           const double* dW, int variant, const double* dgamma_adj, const int64_t* prefixes, int K,
                           const double* penalties, int P, double* dloglik, double* dmean, double* dcov) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(synlik_check(ctx, dX, G, n, m, ldx, dy, variant, dgamma_adj, prefixes, K, penalties, P, dloglik));
  DeviceGuard g(ctx->device);
  return synlik_dev_impl(ctx, dX, (int)G, n, m, ldx, dy, dW, variant, dgamma_adj, prefixes, K, penalties, P, dloglik,
                         dmean, dcov);
}

int elfihip_syn_loglik(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* y,
                       const double* W, int variant, const double* gamma_adj, const int64_t* prefixes, int K,
                       const double* penalties, int P, double* loglik, double* mean, double* cov) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(synlik_check(ctx, X, G, n, m, ldx, y, variant, gamma_adj, prefixes, K, penalties, P, loglik));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)G * (size_t)n, md = (size_t)m * sizeof(double);
  const size_t nll = (size_t)G * (prefixes ? K : 1) * (P > 0 ? P : 1);
  // in: [X rows m][y m][gamma m][W m m]; out: [loglik][mean G m][cov G m m]
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((rows * m + 2 * (size_t)m + (size_t)m * m) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((nll + (size_t)G * m + (size_t)G * m * m) * sizeof(double)));
  double* dX = ctx->in.as<double>();
  double* dy = dX + rows * m;
  double* dgam = dy + m;
  double* dW = dgam + m;
  double* dll = ctx->out.as<double>();
  double* dmean = dll + nll;
  double* dcov = dmean + (size_t)G * m;
  ELFIHIP_TRY(upload_rows(ctx, dX, X, rows, m, ldx));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dy, y, md, hipMemcpyHostToDevice, st));
  if (gamma_adj) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dgam, gamma_adj, md, hipMemcpyHostToDevice, st));
  if (W) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dW, W, (size_t)m * md, hipMemcpyHostToDevice, st));
  ELFIHIP_TRY(synlik_dev_impl(ctx, dX, (int)G, n, m, m, dy, W ? dW : nullptr, variant, gamma_adj ? dgam : nullptr, prefixes,
                              K, penalties, P, dll, mean ? dmean : nullptr, cov ? dcov : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(loglik, dll, nll * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mean) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(mean, dmean, (size_t)G * md, hipMemcpyDeviceToHost, st));
  if (cov) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(cov, dcov, (size_t)G * m * md, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
