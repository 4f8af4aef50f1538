// KLIEP density-ratio estimation (Sugiyama et al. 2008) on gfx950, batched over basis scales and cross-validation folds.
//
// Replaces what elfi/methods/density_ratio_estimation.py does per scale in Python: the basis matrices built with a call
// per entry (_compute_A, _compute_b, _weighted_basis_sum -- the last at every convergence check), the projected
// gradient iteration (_KLIEP, :183-202) and the likelihood cross-validation that repeats it per fold (_KLIEP_lcv,
// :157-181).  One call serves S scales; with F > 0 folds also the S x F leave-fold-out fits.  A "problem" is one
// (scale, held-out fold or none).
//
// Five launches, no host synchronisation between them.
//   basis    one wave per row of x: A[i, j] = exp(-0.5 |x_i - theta_j|^2 / sigma / sigma) (divided by sigma twice, as the
//            reference does), theta = x[:n], into scratch (S, Nx, n); the row's flag "some A[i, j] > 1e-64".
//   b        one workgroup per (scale, centre): b_j = sum_t basis(theta_j, y_t) wy_t.
//   index    one workgroup per scale: the filtered index of a non-null row is the number of non-null rows in front of it,
//            L their count; the row's fold is that of np.array_split(arange(L), F) (the first L % F folds have one more).
//   solve    ONE workgroup of 1024 threads per problem loops over all its steps inside the launch: alpha, b and
//            b_normalized = b / (b . b) sit in LDS, A streams from L2 / HBM once per step -- a wave takes a row, its
//            lanes the columns j = lane + 64 k: the row's product with alpha is a per-lane sum and a fixed tree over the
//            lanes, r_i = w_i / (A_i . alpha), and the same registers give the lane's share of A^T r.  No workgroup waits
//            for another: no grid-wide barrier, no cooperative launch, no spin.
//   lcv      S threads: the mean of a scale's fold scores; +inf when L = 0.
// The iteration mirrors _KLIEP: alpha = 1 / n; prev = A alpha over ALL rows (null and held-out ones included); per step
//   alpha += epsilon A_tr^T (w_tr / (A_tr alpha)) over the training rows (non-null, not held out),
//   alpha = max(0, alpha + (1 - b . alpha) b_normalized), alpha /= b . alpha,
// and when i % interval == 0 (step 0 included) t = A alpha over all rows, stop if |t - prev|_2 < abs_tol, else prev = t.
// NaN and inf propagate as in NumPy (max(0, NaN) is NaN) and never end the loop early: max_iter bounds it.
// The full fit of a scale takes the caller's weights as they are (the reference hands _KLIEP the raw weights_x, :133), the
// fold fits and the scores the normalised ones (_KLIEP_lcv uses self.weights_x).
// Every sum is a per-thread (per-lane) strided sum followed by a fixed tree: no float atomics, and a problem's bits do not
// depend on S, on F or on the other problems of the call.
#include "common.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace elfihip {

constexpr int KL_MAX_D = 64;
constexpr int KL_MAX_N = 256;
constexpr int KL_MAX_ROWS = 65536;
constexpr int KL_MAX_S = 16;
constexpr int KL_MAX_F = 16;
constexpr int KL_THREADS = 1024;              // of the solve kernel
constexpr int KL_WAVES = KL_THREADS / 64;
constexpr int KL_SLOTS = KL_MAX_N / 64;       // columns per lane
constexpr double KL_NULL_LEVEL = 1e-64;

struct KliepArgs {
  const double* x;       // (Nx, d), pitch ldx; the centres are its first n rows
  const double* y;       // (Ny, d), pitch ldy
  const double* wx;      // (Nx) as the caller has them: the full fits
  const double* wxn;     // (Nx) normalised: the fold fits and the scores (F > 0)
  const double* wyn;     // (Ny) normalised
  int64_t ldx, ldy;
  int Nx, Ny, d, n, S, F, max_iter, interval;
  double epsilon, abs_tol;
  double sigma[KL_MAX_S];
  double* A;             // scratch (S, Nx, n)
  double* b;             // scratch (S, n)
  double* t;             // scratch (S (F + 1), 2, Nx): A alpha of the last two convergence checks
  double* fold_scores;   // scratch (S, F)
  int* fold;             // scratch (S, Nx): the basis kernel's flag, then the row's fold (-1: a null row)
  int* L;                // scratch (S)
  double* alpha;         // (S, n) or NULL
  double* w;             // (S, Nx) or NULL
  int64_t* iters;        // (S) or NULL
  double* scores;        // (S, F) or NULL
  double* lcv;           // (S) or NULL
};

__device__ __forceinline__ double kl_basis(const double* p, const double* c, int d, double sigma) {
  double s = 0.0;
  for (int k = 0; k < d; ++k) {
    const double v = p[k] - c[k];
    s += v * v;
  }
  return exp(-0.5 * s / sigma / sigma);
}

// every lane gets the sum over the wave's 64 lanes, in a fixed tree
__device__ __forceinline__ double wave_sum(double q) {
  q = lanes16_sum(q);
  q += __shfl_xor(q, 16);
  q += __shfl_xor(q, 32);
  return q;
}

// The sum over the workgroup of one value per thread, in a fixed tree; every thread gets it.  NT a power of two.
template <int NT>
__device__ __forceinline__ double kl_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void kliep_basis_kernel(KliepArgs P) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int s = blockIdx.y;
  const int i = blockIdx.x * 4 + wv;
  if (i >= P.Nx) return;   // (whole waves leave; nothing below synchronises the workgroup)
  const double sigma = P.sigma[s];
  const double* xi = P.x + (int64_t)i * P.ldx;
  double* Ai = P.A + ((int64_t)s * P.Nx + i) * P.n;
  bool some = false;
  for (int j = lane; j < P.n; j += 64) {
    const double a = kl_basis(xi, P.x + (int64_t)j * P.ldx, P.d, sigma);
    Ai[j] = a;
    some = some || a > KL_NULL_LEVEL;
  }
  const bool any = __any(some);
  if (lane == 0) P.fold[(int64_t)s * P.Nx + i] = any ? 1 : 0;
}

__global__ __launch_bounds__(256) void kliep_b_kernel(KliepArgs P) {
  __shared__ double red[256];
  const int j = blockIdx.x, s = blockIdx.y;
  const double* cj = P.x + (int64_t)j * P.ldx;
  const double sigma = P.sigma[s];
  double acc = 0.0;
  for (int t = threadIdx.x; t < P.Ny; t += 256) acc += kl_basis(cj, P.y + (int64_t)t * P.ldy, P.d, sigma) * P.wyn[t];
  acc = kl_block_sum<256>(acc, red);
  if (threadIdx.x == 0) P.b[s * P.n + j] = acc;
}

__global__ __launch_bounds__(256) void kliep_index_kernel(KliepArgs P) {
  __shared__ int cnt[256];
  __shared__ int total;
  const int tid = threadIdx.x, s = blockIdx.x;
  int* fold = P.fold + (int64_t)s * P.Nx;
  // thread t owns the rows [lo, hi): it alone reads and rewrites their entries of `fold`
  const int chunk = (P.Nx + 255) / 256;
  const int lo = tid * chunk < P.Nx ? tid * chunk : P.Nx;
  const int hi = lo + chunk < P.Nx ? lo + chunk : P.Nx;
  int c = 0;
  for (int i = lo; i < hi; ++i) c += fold[i];
  cnt[tid] = c;
  __syncthreads();
  if (tid == 0) {
    int run = 0;
    for (int k = 0; k < 256; ++k) {
      const int v = cnt[k];
      cnt[k] = run;   // the number of non-null rows in front of thread k's rows
      run += v;
    }
    total = run;
    P.L[s] = run;
  }
  __syncthreads();
  const int L = total;
  const int F = P.F;
  const int q = F > 0 ? L / F : 0, r = F > 0 ? L % F : 0;
  int idx = cnt[tid];
  for (int i = lo; i < hi; ++i) {
    if (!fold[i]) {
      fold[i] = -1;
      continue;
    }
    int f = 0;
    if (F > 0) f = idx < r * (q + 1) ? idx / (q + 1) : r + (idx - r * (q + 1)) / q;   // (q > 0 here: idx >= r = L otherwise)
    fold[i] = f;
    ++idx;
  }
}

// t[i] = A_i . alpha for every row i of the scale: a wave per row, lanes over the columns
__device__ __forceinline__ void kl_all_rows(const double* A, const double* alpha, int Nx, int n, double* t) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = wv; i < Nx; i += KL_WAVES) {
    const double* Ai = A + (int64_t)i * n;
    double p = 0.0;
#pragma unroll
    for (int k = 0; k < KL_SLOTS; ++k) {
      const int j = lane + 64 * k;
      if (j < n) p += Ai[j] * alpha[j];
    }
    p = wave_sum(p);
    if (lane == 0) t[i] = p;
  }
}

__global__ __launch_bounds__(KL_THREADS) void kliep_solve_kernel(KliepArgs P) {
  __shared__ double red[KL_THREADS];
  __shared__ double alpha[KL_MAX_N], b[KL_MAX_N], bn[KL_MAX_N];
  __shared__ double gpart[KL_WAVES][KL_MAX_N];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = P.n, Nx = P.Nx;
  const int s = blockIdx.x / (P.F + 1), h = blockIdx.x % (P.F + 1);   // h = 0: the full fit; else fold h - 1 is held out
  const int held = h - 1;
  const int L = P.L[s];
  if (h > 0 && L == 0) {   // the reference returns before any fit; the lcv kernel writes +inf
    if (tid == 0) P.fold_scores[s * P.F + held] = NAN;
    return;
  }
  const double* A = P.A + (int64_t)s * Nx * n;
  const int* fold = P.fold + (int64_t)s * Nx;
  const double* wt = h == 0 ? P.wx : P.wxn;
  double* tprev = P.t + (int64_t)blockIdx.x * 2 * Nx;
  double* tcur = tprev + Nx;

  // b, b_normalized, alpha = 1 / n
  double bj = 0.0;
  if (tid < n) {
    bj = P.b[s * n + tid];
    b[tid] = bj;
    alpha[tid] = 1.0 / (double)n;
  }
  const double bb = kl_block_sum<KL_THREADS>(tid < n ? bj * bj : 0.0, red);
  if (tid < n) bn[tid] = bj / bb;
  __syncthreads();
  kl_all_rows(A, alpha, Nx, n, tprev);

  int it = 0;
  for (int i = 0; i < P.max_iter; ++i) {
    it = i;
    // the lane's share of A_tr^T (w_tr / (A_tr alpha)) over the wave's training rows
    double g[KL_SLOTS];
#pragma unroll
    for (int k = 0; k < KL_SLOTS; ++k) g[k] = 0.0;
    for (int r = wv; r < Nx; r += KL_WAVES) {
      const int f = fold[r];
      if (f < 0 || f == held) continue;   // (held = -1 in the full fit: never equal to a fold)
      const double* Ar = A + (int64_t)r * n;
      double a[KL_SLOTS];
      double p = 0.0;
#pragma unroll
      for (int k = 0; k < KL_SLOTS; ++k) {
        const int j = lane + 64 * k;
        a[k] = j < n ? Ar[j] : 0.0;
        if (j < n) p += a[k] * alpha[j];
      }
      p = wave_sum(p);
      const double q = wt[r] / p;
#pragma unroll
      for (int k = 0; k < KL_SLOTS; ++k) g[k] += a[k] * q;
    }
#pragma unroll
    for (int k = 0; k < KL_SLOTS; ++k) gpart[wv][lane + 64 * k] = g[k];
    __syncthreads();
    double aj = 0.0;
    if (tid < n) {
      double v[KL_WAVES];
#pragma unroll
      for (int k = 0; k < KL_WAVES; ++k) v[k] = gpart[k][tid];
#pragma unroll
      for (int st = KL_WAVES / 2; st > 0; st >>= 1)
#pragma unroll
        for (int k = 0; k < st; ++k) v[k] += v[k + st];
      aj = alpha[tid] + P.epsilon * v[0];
    }
    const double ba = kl_block_sum<KL_THREADS>(tid < n ? b[tid] * aj : 0.0, red);
    if (tid < n) {
      const double v = aj + (1.0 - ba) * bn[tid];
      aj = v > 0.0 ? v : (v != v ? v : 0.0);   // np.maximum(0, v): a NaN stays
    }
    const double ba2 = kl_block_sum<KL_THREADS>(tid < n ? b[tid] * aj : 0.0, red);
    if (tid < n) alpha[tid] = aj / ba2;
    __syncthreads();
    if (i % P.interval == 0) {
      kl_all_rows(A, alpha, Nx, n, tcur);
      __syncthreads();   // the waves' stores to global memory are visible to the workgroup
      double acc = 0.0;
      for (int r = tid; r < Nx; r += KL_THREADS) {
        const double dv = tcur[r] - tprev[r];
        acc += dv * dv;
      }
      const double diff = sqrt(kl_block_sum<KL_THREADS>(acc, red));
      if (diff < P.abs_tol) break;   // (the same value in every thread; false for a NaN)
      double* sw = tprev;
      tprev = tcur;
      tcur = sw;
    }
  }

  // w = A alpha of the final alpha
  __syncthreads();
  kl_all_rows(A, alpha, Nx, n, tcur);
  __syncthreads();
  if (h == 0) {
    if (P.alpha && tid < n) P.alpha[s * n + tid] = alpha[tid];
    if (P.w)
      for (int r = tid; r < Nx; r += KL_THREADS) P.w[(int64_t)s * Nx + r] = tcur[r];
    if (P.iters && tid == 0) P.iters[s] = it;
    return;
  }
  // the weighted mean of log w over the held-out rows (np.average with weights)
  double num = 0.0, den = 0.0;
  for (int r = tid; r < Nx; r += KL_THREADS)
    if (fold[r] == held) {
      num += log(tcur[r]) * P.wxn[r];
      den += P.wxn[r];
    }
  num = kl_block_sum<KL_THREADS>(num, red);
  den = kl_block_sum<KL_THREADS>(den, red);
  if (tid == 0) P.fold_scores[s * P.F + held] = num / den;
}

__global__ void kliep_lcv_kernel(KliepArgs P) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= P.S) return;
  double sum = 0.0;
  for (int f = 0; f < P.F; ++f) {
    const double v = P.fold_scores[s * P.F + f];
    if (P.scores) P.scores[s * P.F + f] = v;
    sum += v;
  }
  if (P.lcv) P.lcv[s] = P.L[s] == 0 ? INFINITY : sum / (double)P.F;
}

// out[i] = sum_j basis(points_i, centres_j) alpha_j: a wave per point, in the order of the fit's A alpha
__global__ __launch_bounds__(256) void kliep_ratio_kernel(const double* pts, int64_t M, int d, int64_t ldp, const double* cen,
                                                          int n, int64_t ldc, const double* alpha, double sigma,
                                                          double* out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 4 + wv;
  if (i >= M) return;
  const double* pi = pts + i * ldp;
  double p = 0.0;
#pragma unroll
  for (int k = 0; k < KL_SLOTS; ++k) {
    const int j = lane + 64 * k;
    if (j < n) p += kl_basis(pi, cen + (int64_t)j * ldc, d, sigma) * alpha[j];
  }
  p = wave_sum(p);
  if (lane == 0) out[i] = p;
}

static bool kl_sigma_ok(double s) { return s > 0.0 && s <= 1.7976931348623157e308; }

static int kliep_fit_check(elfihip_ctx* ctx, const void* x, int64_t Nx, int d, int64_t ldx, const void* y, int64_t Ny,
                           int64_t ldy, const void* wx, const void* wxn, const void* wyn, const double* sigmas, int S, int n,
                           int max_iter, int interval, int F) {
  ELFIHIP_REQUIRE(ctx, d >= 1 && d <= KL_MAX_D, "KLIEP: %d dimensions; 1 to %d are supported", d, KL_MAX_D);
  ELFIHIP_REQUIRE(ctx, n >= 1 && n <= KL_MAX_N, "KLIEP: %d basis functions; 1 to %d are supported", n, KL_MAX_N);
  ELFIHIP_REQUIRE(ctx, Nx >= n && Nx <= KL_MAX_ROWS, "KLIEP: %lld numerator rows; n = %d to %d are supported", (long long)Nx,
                  n, KL_MAX_ROWS);
  ELFIHIP_REQUIRE(ctx, Ny >= 1 && Ny <= KL_MAX_ROWS, "KLIEP: %lld denominator rows; 1 to %d are supported", (long long)Ny,
                  KL_MAX_ROWS);
  ELFIHIP_REQUIRE(ctx, ldx >= d && ldy >= d, "bad pitch ldx=%lld ldy=%lld d=%d", (long long)ldx, (long long)ldy, d);
  ELFIHIP_REQUIRE(ctx, S >= 1 && S <= KL_MAX_S, "KLIEP: %d scales; 1 to %d are supported", S, KL_MAX_S);
  ELFIHIP_REQUIRE(ctx, F >= 0 && F <= KL_MAX_F, "KLIEP: %d folds; 0 to %d are supported", F, KL_MAX_F);
  ELFIHIP_REQUIRE(ctx, max_iter >= 1 && interval >= 1, "KLIEP: max_iter=%d conv_check_interval=%d must be at least 1",
                  max_iter, interval);
  ELFIHIP_REQUIRE(ctx, x && y && wx && wyn && sigmas && (F == 0 || wxn), "NULL data pointer");
  for (int s = 0; s < S; ++s)
    ELFIHIP_REQUIRE(ctx, kl_sigma_ok(sigmas[s]), "KLIEP: sigma[%d] = %g must be positive and finite", s, sigmas[s]);
  return ELFIHIP_OK;
}

static size_t kl_up(size_t v) { return (v + 1) & ~(size_t)1; }

static int kliep_fit_impl(elfihip_ctx* ctx, const double* dx, int64_t Nx, int d, int64_t ldx, const double* dy, int64_t Ny,
                          int64_t ldy, const double* dwx, const double* dwxn, const double* dwyn, const double* sigmas,
                          int S, int n, double epsilon, int max_iter, double abs_tol, int interval, int F, double* dalpha,
                          double* dw, int64_t* diters, double* dscores, double* dlcv) {
  hipStream_t st = ctx->stream;
  const size_t nA = (size_t)S * Nx * n, nb = (size_t)S * n, nt = (size_t)S * (F + 1) * 2 * Nx, nsc = (size_t)S * F + 1;
  const size_t nfold = kl_up((size_t)S * Nx), nL = kl_up((size_t)S);   // ints
  ELFIHIP_CHECK_HIP(ctx, ctx->scratch.reserve((nA + nb + nt + nsc) * sizeof(double) + (nfold + nL) * sizeof(int)));
  KliepArgs P;
  P.x = dx;
  P.y = dy;
  P.wx = dwx;
  P.wxn = dwxn;
  P.wyn = dwyn;
  P.ldx = ldx;
  P.ldy = ldy;
  P.Nx = (int)Nx;
  P.Ny = (int)Ny;
  P.d = d;
  P.n = n;
  P.S = S;
  P.F = F;
  P.max_iter = max_iter;
  P.interval = interval;
  P.epsilon = epsilon;
  P.abs_tol = abs_tol;
  for (int s = 0; s < KL_MAX_S; ++s) P.sigma[s] = s < S ? sigmas[s] : 1.0;
  P.A = ctx->scratch.as<double>();
  P.b = P.A + nA;
  P.t = P.b + nb;
  P.fold_scores = P.t + nt;
  P.fold = reinterpret_cast<int*>(P.fold_scores + nsc);
  P.L = P.fold + nfold;
  P.alpha = dalpha;
  P.w = dw;
  P.iters = diters;
  P.scores = dscores;
  P.lcv = dlcv;
  hipLaunchKernelGGL(kliep_basis_kernel, dim3((unsigned)((Nx + 3) / 4), (unsigned)S), dim3(256), 0, st, P);
  ELFIHIP_TRY(launch_status(ctx, "KLIEP basis kernel"));
  hipLaunchKernelGGL(kliep_b_kernel, dim3((unsigned)n, (unsigned)S), dim3(256), 0, st, P);
  ELFIHIP_TRY(launch_status(ctx, "KLIEP b kernel"));
  hipLaunchKernelGGL(kliep_index_kernel, dim3((unsigned)S), dim3(256), 0, st, P);
  ELFIHIP_TRY(launch_status(ctx, "KLIEP index kernel"));
  hipLaunchKernelGGL(kliep_solve_kernel, dim3((unsigned)(S * (F + 1))), dim3(KL_THREADS), 0, st, P);
  ELFIHIP_TRY(launch_status(ctx, "KLIEP solve kernel"));
  if (F > 0 && (dscores || dlcv)) {
    hipLaunchKernelGGL(kliep_lcv_kernel, dim3(1), dim3(64), 0, st, P);
    ELFIHIP_TRY(launch_status(ctx, "KLIEP lcv kernel"));
  }
  return ELFIHIP_OK;
}

static int kliep_ratio_check(elfihip_ctx* ctx, const void* pts, int64_t M, int d, int64_t ldp, const void* cen, int n,
                             int64_t ldc, const void* alpha, double sigma, const void* out) {
  ELFIHIP_REQUIRE(ctx, d >= 1 && d <= KL_MAX_D, "KLIEP: %d dimensions; 1 to %d are supported", d, KL_MAX_D);
  ELFIHIP_REQUIRE(ctx, n >= 1 && n <= KL_MAX_N, "KLIEP: %d basis functions; 1 to %d are supported", n, KL_MAX_N);
  ELFIHIP_REQUIRE(ctx, M >= 0 && (M + 3) / 4 <= 0x7fffffff, "KLIEP: bad number of points %lld", (long long)M);
  ELFIHIP_REQUIRE(ctx, ldp >= d && ldc >= d, "bad pitch ldp=%lld ldc=%lld d=%d", (long long)ldp, (long long)ldc, d);
  ELFIHIP_REQUIRE(ctx, kl_sigma_ok(sigma), "KLIEP: sigma = %g must be positive and finite", sigma);
  ELFIHIP_REQUIRE(ctx, cen && alpha && (M == 0 || (pts && out)), "NULL data pointer");
  return ELFIHIP_OK;
}

static int kliep_ratio_impl(elfihip_ctx* ctx, const double* dpts, int64_t M, int d, int64_t ldp, const double* dcen, int n,
                            int64_t ldc, const double* dalpha, double sigma, double* dout) {
  if (M == 0) return ELFIHIP_OK;
  hipLaunchKernelGGL(kliep_ratio_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, ctx->stream, dpts, M, d, ldp, dcen, n,
                     ldc, dalpha, sigma, dout);
  return launch_status(ctx, "KLIEP ratio kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_kliep_fit_dev(elfihip_ctx* ctx, const double* dx, int64_t Nx, int d, int64_t ldx, const double* dy, int64_t Ny,
                          int64_t ldy, const double* dwx, const double* dwx_norm, const double* dwy_norm,
                          const double* sigmas, int S, int n, double epsilon, int max_iter, double abs_tol,
                          int conv_check_interval, int F, double* dalpha, double* dw, int64_t* diters, double* dscores,
                          double* dlcv) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(kliep_fit_check(ctx, dx, Nx, d, ldx, dy, Ny, ldy, dwx, dwx_norm, dwy_norm, sigmas, S, n, max_iter,
                              conv_check_interval, F));
  DeviceGuard g(ctx->device);
  return kliep_fit_impl(ctx, dx, Nx, d, ldx, dy, Ny, ldy, dwx, dwx_norm, dwy_norm, sigmas, S, n, epsilon, max_iter, abs_tol,
                        conv_check_interval, F, dalpha, dw, diters, dscores, dlcv);
}

int elfihip_kliep_fit(elfihip_ctx* ctx, const double* x, int64_t Nx, int d, int64_t ldx, const double* y, int64_t Ny,
                      int64_t ldy, const double* wx, const double* wx_norm, const double* wy_norm, const double* sigmas,
                      int S, int n, double epsilon, int max_iter, double abs_tol, int conv_check_interval, int F,
                      double* alpha, double* w, int64_t* iters, double* scores, double* lcv) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(kliep_fit_check(ctx, x, Nx, d, ldx, y, Ny, ldy, wx, wx_norm, wy_norm, sigmas, S, n, max_iter,
                              conv_check_interval, F));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t sx = (size_t)Nx * d, sy = (size_t)Ny * d, D = sizeof(double);
  // in: [x Nx d][y Ny d][wx Nx][wx_norm Nx][wy_norm Ny]; out: [alpha S n][w S Nx][iters S][scores S F][lcv S]
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((sx + sy + 2 * (size_t)Nx + (size_t)Ny) * D));
  const size_t na = (size_t)S * n, nw = (size_t)S * Nx, nsc = (size_t)S * F;
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((na + nw + 2 * (size_t)S + nsc) * D));
  double* dx = ctx->in.as<double>();
  double* dy = dx + sx;
  double* dwx = dy + sy;
  double* dwxn = dwx + Nx;
  double* dwyn = dwxn + Nx;
  double* da = ctx->out.as<double>();
  double* dw = da + na;
  int64_t* dit = reinterpret_cast<int64_t*>(dw + nw);
  double* dsc = reinterpret_cast<double*>(dit + S);
  double* dl = dsc + nsc;
  ELFIHIP_TRY(upload_rows(ctx, dx, x, (size_t)Nx, d, ldx));
  ELFIHIP_TRY(upload_rows(ctx, dy, y, (size_t)Ny, d, ldy));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dwx, wx, (size_t)Nx * D, hipMemcpyHostToDevice, st));
  if (F > 0) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dwxn, wx_norm, (size_t)Nx * D, hipMemcpyHostToDevice, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dwyn, wy_norm, (size_t)Ny * D, hipMemcpyHostToDevice, st));
  const bool cv = F > 0;
  ELFIHIP_TRY(kliep_fit_impl(ctx, dx, Nx, d, d, dy, Ny, d, dwx, cv ? dwxn : nullptr, dwyn, sigmas, S, n, epsilon, max_iter,
                             abs_tol, conv_check_interval, F, alpha ? da : nullptr, w ? dw : nullptr, iters ? dit : nullptr,
                             cv && scores ? dsc : nullptr, cv && lcv ? dl : nullptr));
  if (alpha) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(alpha, da, na * D, hipMemcpyDeviceToHost, st));
  if (w) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(w, dw, nw * D, hipMemcpyDeviceToHost, st));
  if (iters) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(iters, dit, (size_t)S * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (cv && scores) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(scores, dsc, nsc * D, hipMemcpyDeviceToHost, st));
  if (cv && lcv) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(lcv, dl, (size_t)S * D, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

int elfihip_kliep_ratio_dev(elfihip_ctx* ctx, const double* dpoints, int64_t M, int d, int64_t ldp, const double* dcentres,
                            int n, int64_t ldc, const double* dalpha, double sigma, double* dout) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(kliep_ratio_check(ctx, dpoints, M, d, ldp, dcentres, n, ldc, dalpha, sigma, dout));
  DeviceGuard g(ctx->device);
  return kliep_ratio_impl(ctx, dpoints, M, d, ldp, dcentres, n, ldc, dalpha, sigma, dout);
}

int elfihip_kliep_ratio(elfihip_ctx* ctx, const double* points, int64_t M, int d, int64_t ldp, const double* centres, int n,
                        int64_t ldc, const double* alpha, double sigma, double* out) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(kliep_ratio_check(ctx, points, M, d, ldp, centres, n, ldc, alpha, sigma, out));
  if (M == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t sp = (size_t)M * d, sc = (size_t)n * d, D = sizeof(double);
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((sp + sc + (size_t)n) * D));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((size_t)M * D));
  double* dp = ctx->in.as<double>();
  double* dc = dp + sp;
  double* da = dc + sc;
  double* dout = ctx->out.as<double>();
  ELFIHIP_TRY(upload_rows(ctx, dp, points, (size_t)M, d, ldp));
  ELFIHIP_TRY(upload_rows(ctx, dc, centres, (size_t)n, d, ldc));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(da, alpha, (size_t)n * D, hipMemcpyHostToDevice, st));
  ELFIHIP_TRY(kliep_ratio_impl(ctx, dp, M, d, d, dc, n, d, da, sigma, dout));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(out, dout, (size_t)M * D, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
