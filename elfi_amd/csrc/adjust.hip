// Batched linear regression adjustment (elfi/methods/post_processing.py:195-209, LinearAdjustment) on gfx950.
//
// A job is one (group g, prefix k) pair: the first p_k rows of group g of the regressors X (the summaries minus the
// observed ones, m columns) and of the responses Y (the parameters, q columns).  Per job, per response y:
//     b = argmin ||Yc - Xc b||_2 over the centred rows,  intercept = ybar - xbar.b,  adjusted_i = y_i - x_i.b
// (the reference fits scikit-learn's LinearRegression, an SVD of the centred regressors, and adjusts with the uncentred
// ones).  Here the fit is a Householder QR of the centred [Xc | Yc], which does not depend on how the columns are scaled;
// no Gram matrix is formed.  W = m + q.
//
//   column sums   one workgroup per tile of TR rows: thread c adds column c row by row, and keeps the minimum and maximum
//                 of a regressor column and whether a value was not finite.  A second launch adds a job's tile sums in
//                 tile order and divides by p_k.
//   tile QR       one workgroup per tile: the centred rows [Xc | Yc] (TR x W) in LDS, reduced column by column to the
//                 upper-triangular factor by Householder reflections; the W x W triangle goes to the context's scratch.
//                 A reflection is three steps: the products of column j with every trailing column (each thread adds a
//                 fixed slice of rows, the slices are added in order), the coefficients, the rank-one update.
//                 TR depends on (m, q) alone: 256 rows up to W = 40, 128 beyond (at most 85 KiB of LDS).
//   combine       a fixed binary tree over the job's tiles: at stride s = 1, 2, 4, ... the triangles of tiles t and t + s
//                 (t a multiple of 2 s) are stacked (2 W x W, at most 104 KiB), reduced the same way and written back
//                 to t.  The tree depends on the number of tiles, that is on p_k, alone.
//   solve         one workgroup per job: R11 b = R12 by back-substitution per response, the intercept, and
//                 rss = the squared norm of the response's column of R22.  Column j is dependent when
//                 |R_jj| <= max(p_k, m) eps ||centred column j||_2, the norm taken from R (an orthogonal factor keeps
//                 it); a column whose minimum equals its maximum is constant, hence dependent.
//   adjust        adjusted[i] = Y[i] - X[i].b with the UNCENTRED X, the product summed left to right; rows at or beyond
//                 p_k, and every row of a job whose status is not 0, are NaN.
// Every job works on its own rows from its own means, so prefix p_k has the bits of a group of p_k rows and nothing
// depends on G or on the other jobs.  No atomics, no arrival counters; fp contraction is off.
#include "common.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace elfihip {

constexpr int ADJ_MAX_M = 64;
constexpr int ADJ_MAX_Q = 16;
constexpr int ADJ_NT = 256;          // threads per workgroup
constexpr int ADJ_MAX_PARTS = 16;    // row slices of a column product
constexpr double ADJ_EPS = 2.220446049250313e-16;
constexpr double ADJ_DBL_MAX = 1.7976931348623157e308;

// rows of a tile: a function of (m, q) alone
inline int adj_tile_rows(int m, int q) { return m + q <= 40 ? 256 : 128; }
// slices of a column product over `rows` rows of W columns: (number, rows per slice)
__host__ __device__ inline int adj_parts(int W) { return ADJ_NT / W < ADJ_MAX_PARTS ? ADJ_NT / W : ADJ_MAX_PARTS; }
// doubles of LDS for `rows` x W in reduction: the matrix at pitch W | 1, the slices' partial products, the coefficients,
// two scalars
inline size_t adj_lds_doubles(int rows, int W) { return (size_t)rows * (W | 1) + ADJ_NT + W + 2; }

struct AdjArgs {
  const double* X;          // (G n, m), pitch ldx
  const double* Y;          // (G n, q), pitch ldy
  int64_t n, ldx, ldy;
  int m, q, K, TR;
  const int64_t* prefixes;  // (K)
  const double* toff;       // (K): tiles of the group's jobs before job k (whole numbers)
  int64_t sumT;             // tiles of one group's jobs
  double* rec;              // per tile: [W column sums][m minima][m maxima][not finite]
  double* mean;             // (J, W)
  int* jflag;               // (J): 1 a value is not finite, 2 a regressor column is constant
  double* tri;              // per tile: (W, W) upper-triangular factor
  double* beta;             // (J, q, m): the coefficients the adjust pass reads
  int* jstatus;             // (J)
  double* adjusted;         // (J, n, q)
  double* coef;             // (J, q, m) or NULL
  double* intercept;        // (J, q) or NULL
  double* rss;              // (J, q) or NULL
  int* status;              // (J) or NULL
};

struct AdjTile {
  int64_t g, t, p, job, row0;
  int k, cnt;
  int64_t tiles;   // of the job
};

// block b = g sumT + toff[k] + t: tile t of job (g, k); b is also the tile's slot in rec and tri
__device__ __forceinline__ AdjTile adj_locate(const AdjArgs& A, int64_t b) {
  AdjTile L;
  L.g = b / A.sumT;
  const int64_t rem = b - L.g * A.sumT;
  int k = 0;
  while (k + 1 < A.K && (int64_t)A.toff[k + 1] <= rem) ++k;
  L.k = k;
  L.t = rem - (int64_t)A.toff[k];
  L.p = A.prefixes[k];
  L.job = L.g * A.K + k;
  L.row0 = L.t * A.TR;
  const int64_t left = L.p - L.row0;
  L.cnt = (int)(left < A.TR ? left : A.TR);
  L.tiles = (L.p + A.TR - 1) / A.TR;
  return L;
}

__device__ __forceinline__ double adj_value(const AdjArgs& A, int64_t row, int c) {
  return c < A.m ? A.X[row * A.ldx + c] : A.Y[row * A.ldy + (c - A.m)];
}

__global__ __launch_bounds__(128) void adj_colsum_kernel(AdjArgs A) {
  const AdjTile L = adj_locate(A, blockIdx.x);
  const int c = threadIdx.x, m = A.m, W = A.m + A.q;
  const int rec_len = W + 2 * m + 1;
  double s = 0.0, lo = INFINITY, hi = -INFINITY;
  int bad = 0;
  if (c < W) {
    const int64_t row = L.g * A.n + L.row0;
#pragma unroll 4
    for (int r = 0; r < L.cnt; ++r) {
      const double x = adj_value(A, row + r, c);
      if (!(fabs(x) <= ADJ_DBL_MAX)) bad = 1;
      lo = x < lo ? x : lo;
      hi = x > hi ? x : hi;
      s = s + x;
    }
  }
  bad = __syncthreads_or(bad);
  double* rec = A.rec + (int64_t)blockIdx.x * rec_len;
  if (c < W) rec[c] = s;
  if (c < m) {
    rec[W + c] = lo;
    rec[W + m + c] = hi;
  }
  if (c == 0) rec[W + 2 * m] = bad ? 1.0 : 0.0;
}

// one workgroup per job: the tile sums in tile order
__global__ __launch_bounds__(128) void adj_mean_kernel(AdjArgs A) {
  const int64_t job = blockIdx.x;
  const int64_t g = job / A.K;
  const int k = (int)(job - g * A.K);
  const int64_t p = A.prefixes[k];
  const int64_t tiles = (p + A.TR - 1) / A.TR;
  const int c = threadIdx.x, m = A.m, W = A.m + A.q;
  const int rec_len = W + 2 * m + 1;
  const double* rec = A.rec + (g * A.sumT + (int64_t)A.toff[k]) * rec_len;
  int flag = 0;
  if (c < W) {
    double s = 0.0, lo = INFINITY, hi = -INFINITY;
    for (int64_t t = 0; t < tiles; ++t) {
      const double* rt = rec + t * rec_len;
      s = s + rt[c];
      if (c < m) {
        lo = rt[W + c] < lo ? rt[W + c] : lo;
        hi = rt[W + m + c] > hi ? rt[W + m + c] : hi;
      }
      if (c == 0 && rt[W + 2 * m] != 0.0) flag |= 1;
    }
    A.mean[job * W + c] = s / (double)p;
    if (c < m && lo == hi) flag |= 2;
  }
  const int f1 = __syncthreads_or(flag & 1), f2 = __syncthreads_or(flag & 2);
  if (c == 0) A.jflag[job] = (f1 ? 1 : 0) | (f2 ? 2 : 0);
}

// The matrix M (cnt rows, W columns, pitch WP) in LDS to upper-triangular form by Householder reflections, in place; what
// is left below the diagonal is not meaningful.  RS: rows per slice of a column product (fixed by the caller's shape).
// part: ADJ_NT doubles, f: W doubles, sc: 2 doubles.  All 256 threads call; ends with a barrier.
__device__ void adj_house(double* M, int cnt, int W, int WP, int RS, double* part, double* f, double* sc) {
  const int tid = threadIdx.x;
  const int NP = adj_parts(W);
  const int pc = tid / W, cc = tid - pc * W;
  const int steps = W < cnt - 1 ? W : cnt - 1;
  for (int j = 0; j < steps; ++j) {
    // products of column j with the columns c >= j over the rows r >= j, slice by slice
    if (pc < NP) {
      double s = 0.0;
      if (cc >= j) {
        const int lo = pc * RS > j ? pc * RS : j;
        const int hi = (pc + 1) * RS < cnt ? (pc + 1) * RS : cnt;
        for (int r = lo; r < hi; ++r) s = s + M[r * WP + j] * M[r * WP + cc];
      }
      part[pc * W + cc] = s;
    }
    __syncthreads();
    // v = x - beta e_j with beta = -sign(x_j) ||x||: v.v = 2 beta (beta - x_j), v.a_c = x.a_c - beta a_jc;
    // f_c = 2 (v.a_c) / (v.v)
    if (tid < W && tid >= j) {
      double dj = 0.0, dc = 0.0;
      for (int k = 0; k < NP; ++k) {
        dj = dj + part[k * W + j];
        dc = dc + part[k * W + tid];
      }
      const double alpha = M[j * WP + j];
      const double norm = sqrt(dj);
      const double beta = alpha >= 0.0 ? -norm : norm;
      double fc = 0.0;
      if (dj > 0.0) fc = (dc - beta * M[j * WP + tid]) / (beta * (beta - alpha));
      f[tid] = fc;
      if (tid == j) {
        sc[0] = alpha - beta;
        sc[1] = dj > 0.0 ? beta : alpha;
      }
    }
    __syncthreads();
    const int ncol = W - j - 1, nrow = cnt - j;
    const double vj = sc[0];
    for (int e = tid; e < nrow * ncol; e += ADJ_NT) {
      const int rr = e / ncol;
      const int r = j + rr, c = j + 1 + (e - rr * ncol);
      const double vr = rr == 0 ? vj : M[r * WP + j];
      M[r * WP + c] = M[r * WP + c] - vr * f[c];
    }
    if (tid == 0) M[j * WP + j] = sc[1];   // rows below j alone are read from here on
    __syncthreads();
  }
  __syncthreads();
}

// the triangle of the reduced M (cnt rows) to a (W, W) slot, zeros below the diagonal and from row cnt on
__device__ __forceinline__ void adj_store_triangle(const double* M, int cnt, int W, int WP, double* slot) {
  for (int e = threadIdx.x; e < W * W; e += ADJ_NT) {
    const int i = e / W, c = e - i * W;
    slot[e] = (i < cnt && c >= i) ? M[i * WP + c] : 0.0;
  }
}

__global__ __launch_bounds__(ADJ_NT) void adj_tile_qr_kernel(AdjArgs A) {
  extern __shared__ __align__(16) double lds[];
  const AdjTile L = adj_locate(A, blockIdx.x);
  const int W = A.m + A.q, WP = W | 1;
  double* M = lds;
  double* part = M + A.TR * WP;
  double* f = part + ADJ_NT;
  double* sc = f + W;
  const double* mean = A.mean + L.job * W;
  const int64_t row = L.g * A.n + L.row0;
  for (int e = threadIdx.x; e < L.cnt * W; e += ADJ_NT) {
    const int r = e / W, c = e - r * W;
    M[r * WP + c] = adj_value(A, row + r, c) - mean[c];
  }
  __syncthreads();
  const int NP = adj_parts(W);
  adj_house(M, L.cnt, W, WP, (A.TR + NP - 1) / NP, part, f, sc);
  adj_store_triangle(M, L.cnt, W, WP, A.tri + (int64_t)blockIdx.x * W * W);
}

// stride s of the tree: tiles t (a multiple of 2 s) and t + s of a job -> t
__global__ __launch_bounds__(ADJ_NT) void adj_combine_kernel(AdjArgs A, int64_t s) {
  extern __shared__ __align__(16) double lds[];
  const AdjTile L = adj_locate(A, blockIdx.x);
  if (L.t % (2 * s) != 0 || L.t + s >= L.tiles) return;   // the whole workgroup
  const int W = A.m + A.q, WP = W | 1;
  double* M = lds;
  double* part = M + 2 * W * WP;
  double* f = part + ADJ_NT;
  double* sc = f + W;
  double* top = A.tri + (int64_t)blockIdx.x * W * W;
  const double* bottom = top + s * W * W;
  for (int e = threadIdx.x; e < W * W; e += ADJ_NT) {
    const int i = e / W, c = e - i * W;
    M[i * WP + c] = top[e];
    M[(W + i) * WP + c] = bottom[e];
  }
  __syncthreads();
  const int NP = adj_parts(W);
  adj_house(M, 2 * W, W, WP, (2 * W + NP - 1) / NP, part, f, sc);
  adj_store_triangle(M, 2 * W, W, WP, top);
}

__global__ __launch_bounds__(ADJ_NT) void adj_solve_kernel(AdjArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int tid = threadIdx.x, m = A.m, q = A.q, W = m + q, WP = W | 1;
  const int64_t job = blockIdx.x;
  const int64_t g = job / A.K;
  const int k = (int)(job - g * A.K);
  const int64_t p = A.prefixes[k];
  const double* slot = A.tri + (g * A.sumT + (int64_t)A.toff[k]) * W * W;
  double* R = lds;                 // (W, WP)
  double* bv = R + W * WP;         // (q, m)
  for (int e = tid; e < W * W; e += ADJ_NT) {
    const int i = e / W, c = e - i * W;
    R[i * WP + c] = slot[e];
  }
  __syncthreads();
  int dep = 0;
  if (tid < m) {
    double s = 0.0;
    for (int i = 0; i <= tid; ++i) s = s + R[i * WP + tid] * R[i * WP + tid];
    const double scale = (double)(p > m ? p : (int64_t)m) * ADJ_EPS * sqrt(s);
    dep = !(fabs(R[tid * WP + tid]) > scale);
  }
  dep = __syncthreads_or(dep);
  const int flag = A.jflag[job];
  const int status = (flag & 1) ? 2 : ((flag & 2) || p - 1 < (int64_t)m || dep) ? 3 : 0;
  if (tid < q) {
    const int t = tid;
    const double* mean = A.mean + job * W;
    double* b = bv + t * m;
    double icpt = NAN, rs = NAN;
    if (status == 0) {
      for (int j = m - 1; j >= 0; --j) {
        double s = R[j * WP + m + t];
        for (int i = j + 1; i < m; ++i) s = s - R[j * WP + i] * b[i];
        b[j] = s / R[j * WP + j];
      }
      double d = 0.0;
      for (int j = 0; j < m; ++j) d = d + mean[j] * b[j];
      icpt = mean[m + t] - d;
      rs = 0.0;
      for (int i = m; i <= m + t; ++i) rs = rs + R[i * WP + m + t] * R[i * WP + m + t];
    } else {
      for (int j = 0; j < m; ++j) b[j] = NAN;
    }
    for (int j = 0; j < m; ++j) {
      A.beta[(job * q + t) * m + j] = b[j];
      if (A.coef) A.coef[(job * q + t) * m + j] = b[j];
    }
    if (A.intercept) A.intercept[job * q + t] = icpt;
    if (A.rss) A.rss[job * q + t] = rs;
  }
  if (tid == 0) {
    A.jstatus[job] = status;
    if (A.status) A.status[job] = status;
  }
}

// grid: J x nb workgroups, nb = ceil(n q / 256); one output element per thread
__global__ __launch_bounds__(ADJ_NT) void adj_apply_kernel(AdjArgs A, int64_t nb) {
  __shared__ double b[ADJ_MAX_Q * ADJ_MAX_M];
  const int tid = threadIdx.x, m = A.m, q = A.q;
  const int64_t job = (int64_t)blockIdx.x / nb, chunk = (int64_t)blockIdx.x - job * nb;
  const int64_t g = job / A.K;
  const int k = (int)(job - g * A.K);
  const int64_t p = A.prefixes[k];
  const int st = A.jstatus[job];
  for (int e = tid; e < q * m; e += ADJ_NT) b[e] = A.beta[job * q * m + e];
  __syncthreads();
  const int64_t e = chunk * ADJ_NT + tid;
  if (e >= A.n * q) return;
  const int64_t i = e / q;
  const int t = (int)(e - i * q);
  double val = NAN;
  if (st == 0 && i < p) {
    const int64_t row = g * A.n + i;
    const double* x = A.X + row * A.ldx;
    const double* bt = b + t * m;
    double s = 0.0;
    for (int c = 0; c < m; ++c) s = s + x[c] * bt[c];
    val = A.Y[row * A.ldy + t] - s;
  }
  A.adjusted[job * A.n * q + e] = val;
}

// tiles of the jobs of one group: toff[k] before job k; returns their sum
static int64_t adj_tile_offsets(const int64_t* prefixes, int Ke, int64_t n, int TR, std::vector<double>& toff) {
  toff.resize(Ke);
  int64_t sum = 0;
  for (int k = 0; k < Ke; ++k) {
    toff[k] = (double)sum;
    const int64_t p = prefixes ? prefixes[k] : n;
    sum += (p + TR - 1) / TR;
  }
  return sum;
}

// prefixes is a host array in both forms: it is checked here, before anything is launched
static int adjust_check(elfihip_ctx* ctx, const void* X, int64_t G, int64_t n, int m, int64_t ldx, const void* Y, int q,
                        int64_t ldy, const int64_t* prefixes, int K, const void* adjusted) {
  ELFIHIP_REQUIRE(ctx, m >= 1 && m <= ADJ_MAX_M, "linear adjustment: %d summaries; 1 to %d are supported", m, ADJ_MAX_M);
  ELFIHIP_REQUIRE(ctx, q >= 1 && q <= ADJ_MAX_Q, "linear adjustment: %d parameters; 1 to %d are supported", q, ADJ_MAX_Q);
  ELFIHIP_REQUIRE(ctx, G >= 1 && G <= 0x7fffffff && n >= 2 && ldx >= m && ldy >= q,
                  "bad shape G=%lld n=%lld m=%d ldx=%lld q=%d ldy=%lld", (long long)G, (long long)n, m, (long long)ldx, q,
                  (long long)ldy);
  ELFIHIP_REQUIRE(ctx, X && Y && adjusted, "NULL data pointer");
  const std::string bad = group_lists_error(prefixes, K, nullptr, 0, n);
  ELFIHIP_REQUIRE(ctx, bad.empty(), "%s", bad.c_str());
  const int Ke = prefixes ? K : 1;
  std::vector<double> toff;
  const int64_t sumT = adj_tile_offsets(prefixes, Ke, n, adj_tile_rows(m, q), toff);
  const int64_t nb = (n * q + ADJ_NT - 1) / ADJ_NT;
  ELFIHIP_REQUIRE(ctx, sumT <= 0x7fffffff / G && nb <= 0x7fffffff / (G * Ke),
                  "linear adjustment: G=%lld groups of n=%lld rows at %d prefixes are more than one launch takes",
                  (long long)G, (long long)n, Ke);
  return ELFIHIP_OK;
}

static int adjust_dev_impl(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dY,
                           int q, int64_t ldy, const int64_t* prefixes, int K, double* dadj, double* dcoef, double* dicpt,
                           double* drss, int* dstatus) {
  hipStream_t st = ctx->stream;
  const int Ke = prefixes ? K : 1, W = m + q, TR = adj_tile_rows(m, q);
  std::vector<double> toff;
  const int64_t sumT = adj_tile_offsets(prefixes, Ke, n, TR, toff);
  // parameter block: [prefixes Ke][tile offsets Ke]
  const GroupParams B = group_params(prefixes, K, n, toff.data(), nullptr, 0);
  ELFIHIP_CHECK_HIP(ctx, ctx->par.reserve(B.words.size() * sizeof(double)));
  double* dpar = ctx->par.as<double>();
  // pageable host memory: the copy is done with it when hipMemcpyAsync returns (common.hpp: pageable uploads)
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar, B.words.data(), B.words.size() * sizeof(double), hipMemcpyHostToDevice, st));
  const size_t J = (size_t)G * Ke, tiles = (size_t)G * (size_t)sumT, rec_len = (size_t)W + 2 * m + 1;
  // scratch: [tri tiles W W][rec tiles rec_len][mean J W][beta J q m][jflag J][jstatus J]
  const size_t doubles = tiles * W * W + tiles * rec_len + J * W + J * q * m;
  ELFIHIP_CHECK_HIP(ctx, ctx->sel.reserve(doubles * sizeof(double) + 2 * J * sizeof(int)));
  AdjArgs A;
  A.X = dX;
  A.Y = dY;
  A.n = n;
  A.ldx = ldx;
  A.ldy = ldy;
  A.m = m;
  A.q = q;
  A.K = Ke;
  A.TR = TR;
  A.prefixes = reinterpret_cast<const int64_t*>(dpar);
  A.toff = dpar + B.konst;
  A.sumT = sumT;
  A.tri = ctx->sel.as<double>();
  A.rec = A.tri + tiles * W * W;
  A.mean = A.rec + tiles * rec_len;
  A.beta = A.mean + J * W;
  A.jflag = reinterpret_cast<int*>(A.beta + J * q * m);
  A.jstatus = A.jflag + J;
  A.adjusted = dadj;
  A.coef = dcoef;
  A.intercept = dicpt;
  A.rss = drss;
  A.status = dstatus;
  hipLaunchKernelGGL(adj_colsum_kernel, dim3((unsigned)tiles), dim3(128), 0, st, A);
  ELFIHIP_TRY(launch_status(ctx, "adjustment column-sum kernel"));
  hipLaunchKernelGGL(adj_mean_kernel, dim3((unsigned)J), dim3(128), 0, st, A);
  ELFIHIP_TRY(launch_status(ctx, "adjustment mean kernel"));
  const size_t lds_tile = adj_lds_doubles(TR, W) * sizeof(double), lds_pair = adj_lds_doubles(2 * W, W) * sizeof(double);
  ELFIHIP_TRY(set_lds(ctx, adj_tile_qr_kernel, lds_tile, 48 * 1024));
  hipLaunchKernelGGL(adj_tile_qr_kernel, dim3((unsigned)tiles), dim3(ADJ_NT), lds_tile, st, A);
  ELFIHIP_TRY(launch_status(ctx, "adjustment tile QR kernel"));
  const int64_t most = (n + TR - 1) / TR;
  if (most > 1) ELFIHIP_TRY(set_lds(ctx, adj_combine_kernel, lds_pair, 48 * 1024));
  for (int64_t s = 1; s < most; s <<= 1) {
    hipLaunchKernelGGL(adj_combine_kernel, dim3((unsigned)tiles), dim3(ADJ_NT), lds_pair, st, A, s);
    ELFIHIP_TRY(launch_status(ctx, "adjustment combine kernel"));
  }
  const size_t lds_solve = ((size_t)W * (W | 1) + (size_t)q * m) * sizeof(double);
  ELFIHIP_TRY(set_lds(ctx, adj_solve_kernel, lds_solve, 48 * 1024));
  hipLaunchKernelGGL(adj_solve_kernel, dim3((unsigned)J), dim3(ADJ_NT), lds_solve, st, A);
  ELFIHIP_TRY(launch_status(ctx, "adjustment solve kernel"));
  const int64_t nb = (n * q + ADJ_NT - 1) / ADJ_NT;
  hipLaunchKernelGGL(adj_apply_kernel, dim3((unsigned)(J * (size_t)nb)), dim3(ADJ_NT), 0, st, A, nb);
  return launch_status(ctx, "adjustment apply kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_linear_adjust_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx,
                              const double* dY, int q, int64_t ldy, const int64_t* prefixes, int K, double* dadjusted,
                              double* dcoef, double* dintercept, double* drss, int* dstatus) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(adjust_check(ctx, dX, G, n, m, ldx, dY, q, ldy, prefixes, K, dadjusted));
  DeviceGuard g(ctx->device);
  return adjust_dev_impl(ctx, dX, G, n, m, ldx, dY, q, ldy, prefixes, K, dadjusted, dcoef, dintercept, drss, dstatus);
}

int elfihip_linear_adjust(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* Y,
                          int q, int64_t ldy, const int64_t* prefixes, int K, double* adjusted, double* coef,
                          double* intercept, double* rss, int* status) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(adjust_check(ctx, X, G, n, m, ldx, Y, q, ldy, prefixes, K, adjusted));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)G * (size_t)n, J = (size_t)G * (prefixes ? K : 1);
  const size_t nadj = J * (size_t)n * q, ncoef = J * (size_t)q * m, nq = J * (size_t)q;
  // in: [X rows m][Y rows q]; out: [adjusted J n q][coef J q m][intercept J q][rss J q][status J]
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(rows * (size_t)(m + q) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((nadj + ncoef + 2 * nq) * sizeof(double) + J * sizeof(int)));
  double* dX = ctx->in.as<double>();
  double* dY = dX + rows * m;
  double* dadj = ctx->out.as<double>();
  double* dcoef = dadj + nadj;
  double* dicpt = dcoef + ncoef;
  double* drss = dicpt + nq;
  int* dstatus = reinterpret_cast<int*>(drss + nq);
  ELFIHIP_TRY(upload_rows(ctx, dX, X, rows, m, ldx));
  ELFIHIP_TRY(upload_rows(ctx, dY, Y, rows, q, ldy));
  ELFIHIP_TRY(adjust_dev_impl(ctx, dX, G, n, m, m, dY, q, q, prefixes, K, dadj, coef ? dcoef : nullptr,
                              intercept ? dicpt : nullptr, rss ? drss : nullptr, status ? dstatus : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(adjusted, dadj, nadj * sizeof(double), hipMemcpyDeviceToHost, st));
  if (coef) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(coef, dcoef, ncoef * sizeof(double), hipMemcpyDeviceToHost, st));
  if (intercept) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(intercept, dicpt, nq * sizeof(double), hipMemcpyDeviceToHost, st));
  if (rss) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(rss, drss, nq * sizeof(double), hipMemcpyDeviceToHost, st));
  if (status) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(status, dstatus, J * sizeof(int), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
