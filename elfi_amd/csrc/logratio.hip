// Batched logistic-regression ratio estimation (the classifier of BOLFIRE) on gfx950.
//
// Replaces, for G groups of n simulated summary rows at once, what elfi/methods/classifier.py:72-121 does per call:
// StandardScaler on the n likelihood rows (label +1) stacked on the nm marginal rows (label -1), scikit-learn's
// LogisticRegression(penalty='l1', solver='liblinear') on the standardised rows, and the log-odds at the observed rows.
// The marginal rows are shared by every group.
//
// One workgroup of 256 threads owns one group (the form of synlik.hip).
//   scaler     two passes over the N = n + nm rows: column sums, then sums of squared deviations, both compensated
//              (TwoSum: the result is the rounded exact sum for all practical N), so mean and scale do not depend on the
//              order of the rows beyond the last bit.  A column StandardScaler treats as constant gets scale 1.
//   objective  f(v) = ||v||_1 + C sum_i log(1 + exp(-y_i v.z_i)), z_i = (x~_i, 1), v = (w, b): liblinear's L1R_LR with a
//              penalised intercept.
//   outer step proximal Newton (newGLMNET): one pass over the rows, staged 32 at a time in LDS, gives the margins, the
//              loss, the gradient and the (m + 1)^2 weighted Gram matrix: the m x m block  sum_i D_i x~_i x~_i^T  by
//              v_mfma_f64_16x16x4_f64 on the rows scaled by sqrt(D_i) (tiles dealt to the four waves, syn_gram.hpp), the
//              intercept row  sum_i D_i x~_i, sum_i D_i  by plain sums, so m = 64 still fits the 64-wide tiles.  Every
//              chunk is summed from zero and added to the running total (two-level summation).
//   inner      coordinate descent with soft-thresholding on the quadratic model, by one wave: lane j holds coordinate j's
//              gradient, diagonal, value and (H d)_j in registers (coordinate 64 is replicated), a coordinate's update
//              is computed by every lane from broadcast values; sweeps in index order until the model's own optimality
//              violation is <= 0.1 min(0.1, V) V (V: the outer violation; floor 1e-14), which keeps the outer
//              iteration superlinear.  A coordinate inside the threshold is set to exactly zero.
//   line search backtracking (1, 1/2, 1/4, ...) on the true objective: one loss-only pass per trial; sufficient decrease
//              0.01 lambda Delta (Delta = g.d + ||v + d||_1 - ||v||_1) plus 64 eps |f|, the rounding of f itself.
//   stopping   V = max_j |g_j + sign(v_j)| (v_j != 0), max(|g_j| - 1, 0) (v_j == 0) with g the gradient of the smooth
//              part; stop when V <= tol or after max_iter outer steps.
// Determinism: no atomics, fixed order everywhere; a group's result does not depend on G.
#include "common.hpp"
#include "syn_gram.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace elfihip {

struct LrArgs {
  const double* X;   // (G n, m), pitch ldx
  const double* M;   // (nm, m), pitch ldm
  const double* Y;   // (k, m) contiguous
  int64_t n, ldx, nm, ldm;
  int m, k, max_iter;
  double C, class_min, tol;
  double floor_value;  // log(class_min / (1 - class_min)), taken on the host
  double* logratio;  // (G, k)
  double* coef;      // (G, m) or NULL
  double* intercept; // (G) or NULL
  double* mean;      // (G, m) or NULL
  double* scale;     // (G, m) or NULL
  int* n_iter;       // (G) or NULL
  int* status;       // (G) or NULL
};

constexpr int LR_VP = 72;          // pitch of the coordinate vectors (m + 1 <= 65)
constexpr int LR_MAX_SWEEPS = 1000;
constexpr int LR_MAX_HALVINGS = 40;

template <int T>
struct LrShape : GramShape<T> {
  using GramShape<T>::MP;
  using GramShape<T>::SP;
  using GramShape<T>::LP;
  // staged rows (also the 4 x 64 x 2 partial sums of the scaler: 512 <= 32 SP), the Gram matrix with the intercept row,
  // mean, scale, v, v + d, trial point, gradient; per staged row: gradient coefficient, weight, loss; 8 scalars
  static constexpr int DOUBLES = SL_RC * SP + (MP + 1) * LP + 6 * LR_VP + 3 * SL_RC + 8;
  static_assert(DOUBLES * sizeof(double) <= 160 * 1024);
};

// s + e is the running sum: TwoSum keeps what the addition rounds away
__device__ __forceinline__ void two_sum(double& s, double& e, double x) {
  const double t = s + x;
  const double bp = t - s;
  e += (s - (t - bp)) + (x - bp);
  s = t;
}

__device__ __forceinline__ const double* lr_row(const LrArgs& A, const double* Xg, int64_t r) {
  return r < A.n ? Xg + r * A.ldx : A.M + (r - A.n) * A.ldm;
}

// Column sums of f(x[r][c]) over the N stacked rows for c = tid & 63: (0) x, (1) (x - mu[c])^2.  Rows r = part mod 4 go
// to part tid >> 6; the four parts are combined in order.  res[c] receives the rounded sum; returns (to every thread)
// whether a value was not finite.
template <int SQ>
__device__ int lr_column_sums(const LrArgs& A, const double* Xg, const double* mu, double* part, double* res) {
  const int tid = threadIdx.x, c = tid & 63, p = tid >> 6, m = A.m;
  const int64_t N = A.n + A.nm;
  double s = 0.0, e = 0.0;
  int bad = 0;
  if (c < m) {
    const double shift = SQ ? mu[c] : 0.0;
    for (int64_t r = p; r < N; r += 4) {
      double x = lr_row(A, Xg, r)[c];
      if (!(fabs(x) <= 1.7976931348623157e308)) bad = 1;
      if (SQ) {
        x = x - shift;
        x = x * x;
      }
      two_sum(s, e, x);
    }
  }
  part[2 * tid] = s;
  part[2 * tid + 1] = e;
  bad = __syncthreads_or(bad);
  if (tid < m) {
    double ts = part[2 * tid], te = part[2 * tid + 1];
    for (int q = 1; q < 4; ++q) {
      two_sum(ts, te, part[2 * (64 * q + tid)]);
      te += part[2 * (64 * q + tid) + 1];
    }
    res[tid] = ts + te;
  }
  __syncthreads();
  return bad;
}

// One pass over the group's N rows at the coefficients w (LDS; w[m] the intercept): the loss sum_i log(1 + exp(-y_i t_i))
// goes to sc8[0].  FULL: also H <- C (Gram matrix of the rows weighted by D_i, with the intercept as row and column m),
// gv <- C (gradient of the loss).  All 256 threads; ends with a barrier.
template <int T, bool FULL>
__device__ void lr_pass(const LrArgs& A, const double* Xg, double* stage, const double* mu, const double* sc,
                        const double* w, double* cr, double* dr, double* fr, double* H, double* gv, double* sc8) {
  using Sh = LrShape<T>;
  constexpr int MP = Sh::MP, SP = Sh::SP, LP = Sh::LP, NT = Sh::NT;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = A.m;
  const int lr = lane >> 4, lc = lane & 15;
  const int64_t N = A.n + A.nm;
  v4d tot[NT], chk[NT];
  if (FULL) {
#pragma unroll
    for (int i = 0; i < NT; ++i) tot[i] = (v4d){0.0, 0.0, 0.0, 0.0};
  }
  double gtot = 0.0, htot = 0.0;             // thread j < m: gradient and intercept-row entry j
  double ftot = 0.0, ctot = 0.0, dtot = 0.0; // thread 255: loss, intercept gradient, H[m][m]
  for (int64_t r0 = 0; r0 < N; r0 += SL_RC) {
    __syncthreads();  // the previous chunk is consumed
    for (int e = tid; e < SL_RC * MP; e += 256) {
      const int rr = e / MP, c = e - rr * MP;
      const int64_t r = r0 + rr;
      double v = 0.0;
      if (r < N && c < m) v = (lr_row(A, Xg, r)[c] - mu[c]) / sc[c];
      stage[rr * SP + c] = v;
    }
    __syncthreads();
    {  // margins: 8 lanes per row
      const int rr = tid >> 3, p = tid & 7;
      double part = 0.0;
      for (int c = p; c < m; c += 8) part += stage[rr * SP + c] * w[c];
      const double t = lanes8_sum(part) + w[m];
      if (p == 0) {
        const int64_t r = r0 + rr;
        const double y = r < A.n ? 1.0 : -1.0;
        const double s = y * t;
        const double ex = exp(-fabs(s));
        const double pm = s >= 0.0 ? ex / (1.0 + ex) : 1.0 / (1.0 + ex);   // sigma(-s)
        const bool in = r < N;
        fr[rr] = in ? (s > 0.0 ? 0.0 : -s) + log1p(ex) : 0.0;
        cr[rr] = in ? -y * pm : 0.0;
        dr[rr] = in ? ex / ((1.0 + ex) * (1.0 + ex)) : 0.0;
      }
    }
    __syncthreads();
    if (FULL && tid < m) {
      double gs = 0.0, hs = 0.0;
      for (int rr = 0; rr < SL_RC; ++rr) {
        const double x = stage[rr * SP + tid];
        gs += cr[rr] * x;
        hs += dr[rr] * x;
      }
      gtot += gs;
      htot += hs;
    }
    if (tid == 255) {
      double fs = 0.0, cs = 0.0, ds = 0.0;
      for (int rr = 0; rr < SL_RC; ++rr) {
        fs += fr[rr];
        cs += cr[rr];
        ds += dr[rr];
      }
      ftot += fs;
      ctot += cs;
      dtot += ds;
    }
    if (FULL) {
      __syncthreads();  // the unscaled rows are consumed
      for (int e = tid; e < SL_RC * MP; e += 256) {
        const int rr = e / MP, c = e - rr * MP;
        stage[rr * SP + c] *= sqrt(dr[rr]);
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < NT; ++i) chk[i] = (v4d){0.0, 0.0, 0.0, 0.0};
      const int nr = (int)(N - r0 < SL_RC ? N - r0 : SL_RC);
      for (int s = 0; 4 * s < nr; ++s) gram_step<T>(chk, stage + (4 * s + lr) * SP + lc, wv);
#pragma unroll
      for (int i = 0; i < NT; ++i) tot[i] += chk[i];
    }
  }
  if (FULL) {
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int q = wv + 4 * i;
      if (q < T * T) {
        const int ti = q / T, tj = q - ti * T;
#pragma unroll
        for (int r = 0; r < 4; ++r) H[(16 * ti + lr + 4 * r) * LP + 16 * tj + lc] = A.C * tot[i][r];
      }
    }
    __syncthreads();  // row and column m of the tiles (zeros of the padding, m < MP) give way to the intercept
    if (tid < m) {
      H[m * LP + tid] = A.C * htot;
      H[tid * LP + m] = A.C * htot;
      gv[tid] = A.C * gtot;
    }
  }
  if (tid == 255) {
    sc8[0] = ftot;
    if (FULL) {
      H[m * LP + m] = A.C * dtot;
      gv[m] = A.C * ctot;
    }
  }
  __syncthreads();
}

// Coordinate descent on  g.d + d.H d / 2 + ||v + d||_1  by wave 0: un <- v + d.  D = m + 1 coordinates.
template <int LP>
__device__ void lr_descend(const double* H, const double* gv, const double* v, double* un, int D, double inner_tol) {
  const int lane = threadIdx.x & 63;
  const bool own = lane < D, has64 = D == 65;
  const double gl = own ? gv[lane] : 0.0, hl = own ? H[lane * LP + lane] + 1e-12 : 1.0;
  double ul = own ? v[lane] : 0.0, hd = 0.0;
  const double g64 = has64 ? gv[64] : 0.0, h64 = has64 ? H[64 * LP + 64] + 1e-12 : 1.0;
  double u64 = has64 ? v[64] : 0.0, hd64 = 0.0;
  for (int sweep = 0; sweep < LR_MAX_SWEEPS; ++sweep) {
    double worst = 0.0;
    for (int j = 0; j < D; ++j) {
      double a, b, c;
      if (j < 64) {
        a = __shfl(hl, j);
        b = __shfl(gl, j) + __shfl(hd, j);
        c = __shfl(ul, j);
      } else {
        a = h64;
        b = g64 + hd64;
        c = u64;
      }
      const double viol = c > 0.0 ? fabs(b + 1.0) : c < 0.0 ? fabs(b - 1.0) : fmax(fabs(b) - 1.0, 0.0);
      worst = fmax(worst, viol);
      double nu = 0.0;
      if (b + 1.0 <= a * c)
        nu = c - (b + 1.0) / a;
      else if (b - 1.0 >= a * c)
        nu = c - (b - 1.0) / a;
      if (nu != c) {   // the same values in every lane: uniform
        const double dl = nu - c;
        if (own) hd += dl * H[j * LP + lane];
        if (has64) hd64 += dl * H[j * LP + 64];
        if (j < 64) {
          if (lane == j) ul = nu;
        } else {
          u64 = nu;
        }
      }
    }
    if (worst <= inner_tol) break;
  }
  if (own) un[lane] = ul;
  if (has64 && lane == 0) un[64] = u64;
}

template <int T>
__global__ __launch_bounds__(256) void logratio_kernel(LrArgs A) {
  using Sh = LrShape<T>;
  constexpr int MP = Sh::MP, SP = Sh::SP, LP = Sh::LP;
  extern __shared__ __align__(16) double lds[];
  double* stage = lds;                   // (SL_RC, SP) standardised rows, zero beyond N and beyond m
  double* H = stage + SL_RC * SP;        // (MP + 1, LP) C x weighted Gram matrix, the intercept as coordinate m
  double* mu = H + (MP + 1) * LP;        // column means
  double* sc = mu + LR_VP;               // column scales
  double* v = sc + LR_VP;                // (w, b)
  double* un = v + LR_VP;                // v + d of the quadratic model
  double* vt = un + LR_VP;               // trial point of the line search
  double* gv = vt + LR_VP;               // gradient of the smooth part
  double* cr = gv + LR_VP;               // per staged row: -y sigma(-y t)
  double* dr = cr + SL_RC;               //                 sigma (1 - sigma)
  double* fr = dr + SL_RC;               //                 log(1 + exp(-y t))
  double* sc8 = fr + SL_RC;              // [0] loss, [1] violation, [2] Delta, [3] ||v||_1, [4] ||trial||_1
  const int tid = threadIdx.x, m = A.m, D = A.m + 1;
  const int g = blockIdx.x;
  const int64_t N = A.n + A.nm;
  const double* Xg = A.X + (int64_t)g * A.n * A.ldx;
  const double dN = (double)N, eps = 2.220446049250313e-16;

  // ---- scaler -----------------------------------------------------------------------------------------------------
  int bad = lr_column_sums<0>(A, Xg, mu, stage, mu);
  if (tid < m) mu[tid] = mu[tid] / dN;
  __syncthreads();
  bad |= lr_column_sums<1>(A, Xg, mu, stage, sc);
  int fin = 1;
  if (tid < m) {
    const double var = sc[tid] / dN, mean = mu[tid];
    fin = fabs(mean) <= 1.7976931348623157e308 && fabs(var) <= 1.7976931348623157e308;
    const double t = dN * mean * eps;
    sc[tid] = var <= dN * eps * var + t * t ? 1.0 : sqrt(var);
  }
  if (tid < LR_VP) v[tid] = 0.0;
  bad |= __syncthreads_or(!fin);
  int n_iter = 0, status = 0;
  if (bad) {
    status = 2;
  } else {
    // ---- proximal Newton ------------------------------------------------------------------------------------------
    for (int it = 0;; ++it) {
      lr_pass<T, true>(A, Xg, stage, mu, sc, v, cr, dr, fr, H, gv, sc8);
      if (tid == 0) {
        double viol = 0.0, l1 = 0.0;
        for (int j = 0; j < D; ++j) {
          const double vj = v[j], gj = gv[j];
          viol = fmax(viol, vj > 0.0 ? fabs(gj + 1.0) : vj < 0.0 ? fabs(gj - 1.0) : fmax(fabs(gj) - 1.0, 0.0));
          l1 += fabs(vj);
        }
        sc8[1] = viol;
        sc8[3] = l1;
      }
      __syncthreads();
      const double viol = sc8[1];
      if (!(viol > A.tol)) {
        if (!(viol <= A.tol)) status = 2;   // NaN: a non-finite value on the way
        break;
      }
      if (it >= A.max_iter) {
        status = 1;
        break;
      }
      const double f_old = A.C * sc8[0] + sc8[3];
      if (tid < 64) lr_descend<LP>(H, gv, v, un, D, fmax(0.1 * fmin(0.1, viol) * viol, 1e-14));
      __syncthreads();
      if (tid == 0) {
        double gd = 0.0, l1 = 0.0;
        for (int j = 0; j < D; ++j) {
          gd += gv[j] * (un[j] - v[j]);
          l1 += fabs(un[j]);
        }
        sc8[2] = gd + l1 - sc8[3];
      }
      __syncthreads();
      const double delta = sc8[2];
      double lam = 1.0;
      bool accepted = false;
      for (int h = 0; h < LR_MAX_HALVINGS; ++h) {
        if (tid < D) vt[tid] = lam == 1.0 ? un[tid] : v[tid] + lam * (un[tid] - v[tid]);
        __syncthreads();
        lr_pass<T, false>(A, Xg, stage, mu, sc, vt, cr, dr, fr, H, gv, sc8);
        if (tid == 0) {
          double l1 = 0.0;
          for (int j = 0; j < D; ++j) l1 += fabs(vt[j]);
          sc8[4] = l1;
        }
        __syncthreads();
        const double f_new = A.C * sc8[0] + sc8[4];
        if (f_new - f_old <= 0.01 * lam * delta + 64.0 * eps * fabs(f_old)) {
          accepted = true;
          break;
        }
        lam *= 0.5;
      }
      if (!accepted) {   // no step reduces the objective: the rounding level of f is reached before tol
        status = 4;
        break;
      }
      if (tid < D) v[tid] = vt[tid];
      n_iter = it + 1;
      __syncthreads();
    }
  }

  // ---- outputs ------------------------------------------------------------------------------------------------------
  const bool nan_out = status == 2;
  if (tid < m) {
    if (A.coef) A.coef[(int64_t)g * m + tid] = nan_out ? NAN : v[tid];
    if (A.mean) A.mean[(int64_t)g * m + tid] = nan_out ? NAN : mu[tid];
    if (A.scale) A.scale[(int64_t)g * m + tid] = nan_out ? NAN : sc[tid];
  }
  if (tid == 0) {
    if (A.intercept) A.intercept[g] = nan_out ? NAN : v[m];
    if (A.n_iter) A.n_iter[g] = n_iter;
    if (A.status) A.status[g] = status;
  }
  for (int q = tid; q < A.k; q += 256) {
    double t = NAN;
    if (!nan_out) {
      const double* yq = A.Y + (int64_t)q * m;
      t = 0.0;
      for (int j = 0; j < m; ++j) t += v[j] * ((yq[j] - mu[j]) / sc[j]);
      t += v[m];
      if (A.class_min > 0.0) {
        const double ex = exp(-fabs(t));
        const double p = t >= 0.0 ? 1.0 / (1.0 + ex) : ex / (1.0 + ex);
        if (p < A.class_min) t = A.floor_value;
      }
    }
    A.logratio[(int64_t)g * A.k + q] = t;
  }
}

static int logratio_check(elfihip_ctx* ctx, const void* X, int64_t G, int64_t n, int m, int64_t ldx, const void* M,
                          int64_t nm, int64_t ldm, const void* Yobs, int64_t k, double C, double class_min, double tol,
                          int max_iter, const void* logratio) {
  ELFIHIP_REQUIRE(ctx, m >= 1 && m <= SL_MAX_M, "log ratio: %d summaries; 1 to %d are supported", m, SL_MAX_M);
  ELFIHIP_REQUIRE(ctx, G >= 1 && G <= 0x7fffffff && n >= 1 && nm >= 1 && ldx >= m && ldm >= m && k >= 1 && k <= 0x7fffffff,
                  "bad shape G=%lld n=%lld nm=%lld m=%d ldx=%lld ldm=%lld k=%lld", (long long)G, (long long)n,
                  (long long)nm, m, (long long)ldx, (long long)ldm, (long long)k);
  ELFIHIP_REQUIRE(ctx, X && M && Yobs && logratio, "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, C > 0.0 && C <= 1.7976931348623157e308, "C must be positive and finite");
  ELFIHIP_REQUIRE(ctx, class_min >= 0.0 && class_min < 1.0, "class_min must lie in [0, 1)");
  ELFIHIP_REQUIRE(ctx, tol >= 0.0, "tol must not be negative");
  ELFIHIP_REQUIRE(ctx, max_iter >= 0, "max_iter must not be negative");
  return ELFIHIP_OK;
}

static int logratio_dev_impl(elfihip_ctx* ctx, const double* dX, int G, int64_t n, int m, int64_t ldx, const double* dM,
                             int64_t nm, int64_t ldm, const double* dY, int k, double C, double class_min, double tol,
                             int max_iter, double* dlr, double* dcoef, double* dicpt, double* dmean, double* dscale,
                             int* dniter, int* dstatus) {
  LrArgs A;
  A.X = dX;
  A.M = dM;
  A.Y = dY;
  A.n = n;
  A.ldx = ldx;
  A.nm = nm;
  A.ldm = ldm;
  A.m = m;
  A.k = k;
  A.max_iter = max_iter;
  A.C = C;
  A.class_min = class_min;
  A.tol = tol;
  A.floor_value = class_min > 0.0 ? std::log(class_min / (1.0 - class_min)) : 0.0;
  A.logratio = dlr;
  A.coef = dcoef;
  A.intercept = dicpt;
  A.mean = dmean;
  A.scale = dscale;
  A.n_iter = dniter;
  A.status = dstatus;
  return launch_by_tiles(
      ctx, m, (unsigned)G, "log-ratio kernel", [](auto T) { return logratio_kernel<decltype(T)::value>; },
      [](auto T) { return (size_t)LrShape<decltype(T)::value>::DOUBLES * sizeof(double); }, A);
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_log_ratio_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dM,
                          int64_t nm, int64_t ldm, const double* dYobs, int64_t k, double C, double class_min, double tol,
                          int max_iter, double* dlogratio, double* dcoef, double* dintercept, double* dmean,
                          double* dscale, int* dn_iter, int* dstatus) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(logratio_check(ctx, dX, G, n, m, ldx, dM, nm, ldm, dYobs, k, C, class_min, tol, max_iter, dlogratio));
  DeviceGuard g(ctx->device);
  return logratio_dev_impl(ctx, dX, (int)G, n, m, ldx, dM, nm, ldm, dYobs, (int)k, C, class_min, tol, max_iter, dlogratio,
                           dcoef, dintercept, dmean, dscale, dn_iter, dstatus);
}

int elfihip_log_ratio(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* M,
                      int64_t nm, int64_t ldm, const double* Yobs, int64_t k, double C, double class_min, double tol,
                      int max_iter, double* logratio, double* coef, double* intercept, double* mean, double* scale,
                      int* n_iter, int* status) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(logratio_check(ctx, X, G, n, m, ldx, M, nm, ldm, Yobs, k, C, class_min, tol, max_iter, logratio));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)G * (size_t)n, md = (size_t)m * sizeof(double), Gs = (size_t)G;
  // in: [X rows m][M nm m][Yobs k m]; out: [logratio G k][coef G m][mean G m][scale G m][intercept G][n_iter G][status G]
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((rows + (size_t)nm + (size_t)k) * md));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((Gs * (size_t)k + 3 * Gs * m + Gs) * sizeof(double) + 2 * Gs * sizeof(int)));
  double* dX = ctx->in.as<double>();
  double* dM = dX + rows * m;
  double* dY = dM + (size_t)nm * m;
  double* dlr = ctx->out.as<double>();
  double* dcoef = dlr + Gs * (size_t)k;
  double* dmean = dcoef + Gs * m;
  double* dscale = dmean + Gs * m;
  double* dicpt = dscale + Gs * m;
  int* dniter = reinterpret_cast<int*>(dicpt + Gs);
  int* dstatus = dniter + Gs;
  ELFIHIP_TRY(upload_rows(ctx, dX, X, rows, m, ldx));
  ELFIHIP_TRY(upload_rows(ctx, dM, M, (size_t)nm, m, ldm));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dY, Yobs, (size_t)k * md, hipMemcpyHostToDevice, st));
  ELFIHIP_TRY(logratio_dev_impl(ctx, dX, (int)G, n, m, m, dM, nm, m, dY, (int)k, C, class_min, tol, max_iter, dlr,
                                coef ? dcoef : nullptr, intercept ? dicpt : nullptr, mean ? dmean : nullptr,
                                scale ? dscale : nullptr, n_iter ? dniter : nullptr, status ? dstatus : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(logratio, dlr, Gs * (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
  if (coef) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(coef, dcoef, Gs * md, hipMemcpyDeviceToHost, st));
  if (mean) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(mean, dmean, Gs * md, hipMemcpyDeviceToHost, st));
  if (scale) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(scale, dscale, Gs * md, hipMemcpyDeviceToHost, st));
  if (intercept) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(intercept, dicpt, Gs * sizeof(double), hipMemcpyDeviceToHost, st));
  if (n_iter) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(n_iter, dniter, Gs * sizeof(int), hipMemcpyDeviceToHost, st));
  if (status) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(status, dstatus, Gs * sizeof(int), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
