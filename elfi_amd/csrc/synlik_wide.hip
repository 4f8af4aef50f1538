// The wide Gaussian synthetic likelihood on gfx950: 65 to 256 summaries, variants 0 (standard, optionally Warton
// shrinkage) and 1 (unbiased, Ghurye-Olkin) of synlik.hip, whose semantics it keeps.
//
// synlik.hip holds the padded m x m matrix, its factor and a staged chunk of rows in the LDS of one workgroup; at 145
// summaries the two matrices alone are 412 KB.  Here the work is split in two kernels with a global workspace between them.
//
//   moments   grid (lower-triangle pairs of 64-column blocks, G), 256 threads.  A workgroup owns one 64 x 64 block
//             (bi, bj <= bi) of S2 = sum d_i d_i^T of one group, d_i = x_i - c with c the group's first row.  It streams
//             the n rows, 32 at a time: its two 64-column slabs are staged in LDS at a pitch of 80 doubles (pitch mod 32 ==
//             16: the two rows a half-wave reads fall into different banks).  The 16 tiles of the block are dealt four to
//             a wave (wave w: column tile w, the four row tiles), one v_mfma_f64_16x16x4_f64 per tile and 4 rows.  Every
//             chunk is summed from zero and then added to the running total.  The diagonal-block workgroups also sum S1.
//             At a prefix boundary p the sums of the rows before p are written to the workspace; a boundary inside a
//             4-row step goes through an extra, masked MFMA into a temporary, the running sums go on with the whole
//             step, so prefix p of a long group has the bits of a group of p rows.
//   finish    one workgroup of 256 threads per (group, prefix, penalty).  Left-looking blocked Cholesky factorisation
//             (wide_chol.hpp: wide_panel_chol, shared with semibsl_wide.hip) on
//             the job's own slab of the workspace, the residual y - mean riding along as row m (its forward solve is the
//             factorisation's update).  Per 32-column panel: the update sum_k L[i][k] L[j][k] over the panels already
//             factored is accumulated by MFMA from the slab (each lane loads four consecutive k of one row, 32 bytes;
//             the slab is L2-resident), the panel's own entries -- covariance from S1 and S2, Warton for the job's
//             penalty -- are formed in the same lane and the difference goes to LDS (at most 257 x 32 at pitch 33);
//             the 32 x 32 diagonal block is factored there and the rows below solved, column by column; the panel is
//             written back once.  The unfactored matrix is never stored: every word of the slab is written exactly once
//             and nothing in global memory is read, modified and written.  Left-looking for that reason: a right-looking
//             sweep would read and write the trailing matrix, up to 526 KB, once per panel.
//             log|S| and the quadratic form are summed by one thread in index order.
// Whitening is the launch of syn_gauss.hpp in front.  No atomics, fixed order everywhere: one (group, prefix, penalty)
// result depends neither on G, K, P nor on how the host cuts the launches into chunks to keep the workspace under its cap.
#include "syn_gauss.hpp"
#include "wide_chol.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace elfihip {

constexpr int SW_RC = 32;              // rows per staged chunk (8 MFMA steps)
constexpr int SW_SP = SW_BLK + 16;     // pitch of a staged slab

// doubles of one (group, prefix) snapshot: the padded S2 (lower blocks) and S1 behind it
inline size_t wide_snap(int m) { return (size_t)wide_mpad(m) * wide_mpad(m) + wide_mpad(m); }

struct WideMomArgs {
  const double* X;          // (Gc n, m), pitch ldx: the groups of this launch
  int64_t n, ldx;
  int m, mpad, K;
  const int64_t* prefixes;  // (K) ascending, last == n
  double* snap;             // (Gc, K) snapshots
};

__global__ __launch_bounds__(256) void synlik_wide_moments_kernel(WideMomArgs A) {
  __shared__ __align__(16) double stage[2 * SW_RC * SW_SP];
  __shared__ double cs[2 * SW_BLK];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = A.m;
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.x) ++bi;
  const int bj = (int)blockIdx.x - bi * (bi + 1) / 2;
  const bool diag = bi == bj;
  const int g = blockIdx.y;
  const double* Xg = A.X + (int64_t)g * A.n * A.ldx;
  double* snap_g = A.snap + (size_t)g * A.K * ((size_t)A.mpad * A.mpad + A.mpad);
  if (tid < 2 * SW_BLK) {
    const int col = SW_BLK * (tid < SW_BLK ? bi : bj) + (tid & (SW_BLK - 1));
    cs[tid] = col < m ? Xg[col] : 0.0;
  }
  double* stA = stage;
  double* stB = diag ? stage : stage + SW_RC * SW_SP;
  const int slabs = diag ? 1 : 2;

  v4d tot[4], chk[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) tot[i] = (v4d){0.0, 0.0, 0.0, 0.0};
  double s1tot = 0.0, s1chk = 0.0;
  const int lr = lane >> 4, lc = lane & 15;
  int kb = 0;  // next boundary
  int64_t nextp = A.prefixes[0];
  for (int64_t r0 = 0; r0 < A.n; r0 += SW_RC) {
    __syncthreads();  // the previous chunk is consumed (first pass: cs is written)
    for (int e = tid; e < slabs * SW_RC * SW_BLK; e += 256) {
      const int sl = e / (SW_RC * SW_BLK), f = e - sl * (SW_RC * SW_BLK);
      const int rr = f / SW_BLK, c = f - rr * SW_BLK;
      const int col = SW_BLK * (sl ? bj : bi) + c;
      const int64_t r = r0 + rr;
      double v = 0.0;
      if (r < A.n && col < m) v = Xg[r * A.ldx + col] - cs[sl * SW_BLK + c];
      stage[(sl * SW_RC + rr) * SW_SP + c] = v;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) chk[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    s1chk = 0.0;
    const int nr = (int)(A.n - r0 < SW_RC ? A.n - r0 : SW_RC);
    for (int s = 0; 4 * s < nr; ++s) {
      const int64_t g0 = r0 + 4 * s;
      const double* rowA = stA + (4 * s + lr) * SW_SP + lc;
      const double* rowB = stB + (4 * s + lr) * SW_SP + 16 * wv + lc;
      // boundaries in (g0, g0 + 4]: the sums of the rows before the boundary, without disturbing the running ones
      while (kb < A.K && nextp <= g0 + 4) {
        const int cut = (int)(nextp - g0);   // rows of this step that count: 1 .. 4
        double* S2 = snap_g + (size_t)kb * ((size_t)A.mpad * A.mpad + A.mpad);
        const double b = lr < cut ? rowB[0] : 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const double a = lr < cut ? rowA[16 * i] : 0.0;
          const v4d tmp = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, chk[i], 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; ++r)
            S2[(size_t)(SW_BLK * bi + 16 * i + lr + 4 * r) * A.mpad + SW_BLK * bj + 16 * wv + lc] = tot[i][r] + tmp[r];
        }
        if (diag && tid < SW_BLK) {
          double t1 = s1chk;
          for (int rr = 0; rr < cut; ++rr) t1 += stA[(4 * s + rr) * SW_SP + tid];
          S2[(size_t)A.mpad * A.mpad + SW_BLK * bi + tid] = s1tot + t1;
        }
        ++kb;
        nextp = kb < A.K ? A.prefixes[kb] : 0;
      }
      const double b = rowB[0];
#pragma unroll
      for (int i = 0; i < 4; ++i) chk[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(rowA[16 * i], b, chk[i], 0, 0, 0);
      if (diag && tid < SW_BLK)
        for (int rr = 0; rr < 4; ++rr) s1chk += stA[(4 * s + rr) * SW_SP + tid];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) tot[i] += chk[i];
    s1tot += s1chk;
  }
}

struct WideFinArgs {
  const double* X;          // (Gc n, m), pitch ldx: the groups of this launch (the shift is their first row)
  int64_t n, ldx;
  int m, mpad, pw, variant;
  const double* y;          // (m), whitened
  const int64_t* prefixes;  // (K)
  const double* penalties;  // (P) or NULL
  const double* konst;      // (K): variant 1
  int K, P;
  const double* snap;       // (Gc, K) snapshots of this launch's groups
  double* slabs;            // one per workgroup
  int64_t job0;             // first job of the launch, counted from the launch's first group: job = (g K + k) Pe + p
  int64_t group0;           // the launch's first group in the call
  double* loglik;           // (G, K, max(P, 1))
  double* mean;             // (G, m) or NULL
  double* cov;              // (G, m, m) or NULL
};

__global__ __launch_bounds__(256) void synlik_wide_finish_kernel(WideFinArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int m = A.m, mpad = A.mpad, pw = A.pw;
  double* P = lds;                         // (m + 1, SW_PP) the panel
  double* s1 = P + (size_t)(m + 1) * SW_PP;   // S1 of the shifted rows
  double* rs = s1 + mpad;                  // y - mean
  double* ws = rs + mpad;                  // Warton's diagonal scaling
  double* dg = ws + mpad;                  // diagonal of the factor
  double* z = dg + mpad;                   // the solved residual
  const int tid = threadIdx.x;
  const int Pe = A.P > 0 ? A.P : 1;
  const int64_t job = A.job0 + blockIdx.x;
  const int pi = (int)(job % Pe);
  const int kb = (int)((job / Pe) % A.K);
  const int64_t gl = job / Pe / A.K;       // group within the launch
  const int64_t g = A.group0 + gl;
  const int64_t np = A.prefixes[kb];
  const double dn = (double)np;
  const double* S2 = A.snap + (size_t)(gl * A.K + kb) * ((size_t)mpad * mpad + mpad);
  const double* Xg = A.X + gl * A.n * A.ldx;
  double* L = A.slabs + (size_t)blockIdx.x * (size_t)(m + 1) * pw;
  double* out = A.loglik + ((g * A.K + kb) * Pe + pi);

  if (tid < m) {
    const double c = Xg[tid], t1 = S2[(size_t)mpad * mpad + tid];
    s1[tid] = t1;
    rs[tid] = (A.y[tid] - c) - t1 / dn;
    const double d = (S2[(size_t)tid * mpad + tid] - t1 * t1 / dn) / (dn - 1.0);
    ws[tid] = sqrt(d + 1e-5);
    if (np == A.n && pi == 0 && A.mean) A.mean[g * m + tid] = c + t1 / dn;
  }
  __syncthreads();
  if (np == A.n && pi == 0 && A.cov) {  // the full group: one value for (i, j) and (j, i)
    double* C = A.cov + g * m * m;
    for (int i = tid >> 4; i < m; i += 16)
      for (int j = tid & 15; j <= i; j += 16) {
        const double v = (S2[(size_t)i * mpad + j] - s1[i] * s1[j] / dn) / (dn - 1.0);
        C[(size_t)i * m + j] = v;
        C[(size_t)j * m + i] = v;
      }
  }
  const double gam = A.P > 0 ? 1.0 - A.penalties[pi] : 1.0;
  // entry (i, j <= i) of the matrix to factor, row m the residual; cov_warton(S, 1 - penalty) as written: eps inside
  // both diagonal scalings
  const auto entry = [&](int i, int j) -> double {
    if (j >= m || j > i) return 0.0;
    if (i == m) return rs[j];
    double v = (S2[(size_t)i * mpad + j] - s1[i] * s1[j] / dn) / (dn - 1.0);
    if (A.P > 0) {
      const double d1i = 1.0 / ws[i], d1j = 1.0 / ws[j];
      const double r = (d1i * v) * d1j;
      const double rg = gam * r + (i == j ? (1.0 - gam) : 0.0);
      v = (ws[i] * rg) * ws[j];
    }
    return v;
  };

  if (!wide_panel_chol(L, pw, m, P, dg, z, entry)) {
    if (tid == 0) *out = -INFINITY;
    return;
  }

  if (tid == 0) {
    double ll = -INFINITY;
    double quad = 0.0, logdet = 0.0;
    for (int j = 0; j < m; ++j) {
      quad += z[j] * z[j];
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
    *out = ll;
  }
}

static int wide_check(elfihip_ctx* ctx, const void* X, int64_t G, int64_t n, int m, int64_t ldx, const void* y, int variant,
                      const int64_t* prefixes, int K, const double* penalties, int P, const void* loglik) {
  ELFIHIP_REQUIRE(ctx, m >= SW_MIN_M && m <= SW_MAX_M,
                  "wide synthetic likelihood: %d summaries; %d to %d are supported (elfihip_syn_loglik takes 1 to %d)", m,
                  SW_MIN_M, SW_MAX_M, SW_MIN_M - 1);
  ELFIHIP_REQUIRE(ctx, G >= 1 && G <= 0x7fffffff && n >= 2 && ldx >= m, "bad shape G=%lld n=%lld m=%d ldx=%lld",
                  (long long)G, (long long)n, m, (long long)ldx);
  ELFIHIP_REQUIRE(ctx, X && y && loglik, "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, variant == 0 || variant == 1,
                  "wide synthetic likelihood: variant %d; 0 (standard) and 1 (unbiased) are supported above %d summaries",
                  variant, SW_MIN_M - 1);
  ELFIHIP_REQUIRE(ctx, !(penalties && P >= 1) || variant == 0, "penalties go with the standard variant only (variant %d)",
                  variant);
  const std::string bad = group_lists_error(prefixes, K, penalties, P, n);
  ELFIHIP_REQUIRE(ctx, bad.empty(), "%s", bad.c_str());
  return ELFIHIP_OK;
}

// Device rows, y, W and outputs; host prefixes and penalties (checked above).
static int wide_dev_impl(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                         const double* dW, int variant, const int64_t* prefixes, int K, const double* penalties, int P,
                         double* dll, double* dmean, double* dcov) {
  hipStream_t st = ctx->stream;
  const int Ke = prefixes ? K : 1, Pe = P > 0 ? P : 1;
  std::vector<double> konst(Ke);
  for (int k = 0; k < Ke; ++k) konst[k] = variant == 1 ? unbiased_const(m, prefixes ? prefixes[k] : n) : 0.0;
  // parameter block: [prefixes Ke][konst Ke][penalties P], and behind it on the device [yw m]
  const GroupParams B = group_params(prefixes, K, n, konst.data(), penalties, P);
  double* dpar;
  ELFIHIP_TRY(upload_group_params(ctx, B, m, &dpar));
  double* dyw = dpar + B.words.size();

  // The workspace, in doubles: [whitened rows of Gc groups][their Gc Ke snapshots][Jc slabs].  Half the cap bounds the
  // first two, half the slabs; one group and one slab are the least a launch needs.
  const size_t cap = (ctx->wide_cap ? ctx->wide_cap : SW_SCRATCH_CAP) / sizeof(double);
  const size_t xw_group = dW ? ((size_t)n * m + 3) / 4 * 4 : 0;
  const size_t snap = wide_snap(m), slab = wide_slab(m);
  const size_t per_group = xw_group + (size_t)Ke * snap;
  const int64_t Gc = (int64_t)std::min<size_t>(std::min<size_t>((size_t)G, 65535), std::max<size_t>(1, cap / 2 / per_group));   // (grid.y)
  const int64_t group_jobs = (int64_t)Ke * Pe;
  const int64_t Jc = (int64_t)std::min<size_t>((size_t)(Gc * group_jobs), std::max<size_t>(1, cap / 2 / slab));
  ELFIHIP_CHECK_HIP(ctx, ctx->scratch.reserve(((size_t)Gc * per_group + (size_t)Jc * slab) * sizeof(double)));
  double* dXw = ctx->scratch.as<double>();
  double* dsnap = dXw + (size_t)Gc * xw_group;
  double* dslab = dsnap + (size_t)Gc * Ke * snap;

  const int nb = wide_mpad(m) / SW_BLK;
  const size_t fin_lds = ((size_t)(m + 1) * SW_PP + 5 * (size_t)wide_mpad(m)) * sizeof(double);
  ELFIHIP_TRY(set_lds(ctx, synlik_wide_finish_kernel, fin_lds, 48 * 1024));
  for (int64_t g0 = 0; g0 < G; g0 += Gc) {
    const int64_t gc = std::min<int64_t>(Gc, G - g0);
    const double* Xc = dX + g0 * n * ldx;
    int64_t ldc = ldx;
    if (dW) {
      const int64_t rows = gc * n;
      const int64_t want = (rows * m + 255) / 256;
      const int grid = (int)std::min<int64_t>(std::max<int64_t>(want, 1), (int64_t)ctx->cu_count * 8);
      hipLaunchKernelGGL(synlik_whiten_kernel, dim3(grid), dim3(256), 0, st, Xc, rows, m, ldx, dW, dy, dXw, dyw);
      ELFIHIP_TRY(launch_status(ctx, "whitening kernel"));
      Xc = dXw;
      ldc = m;
    }
    WideMomArgs M;
    M.X = Xc;
    M.n = n;
    M.ldx = ldc;
    M.m = m;
    M.mpad = wide_mpad(m);
    M.K = Ke;
    M.prefixes = reinterpret_cast<const int64_t*>(dpar);
    M.snap = dsnap;
    hipLaunchKernelGGL(synlik_wide_moments_kernel, dim3(nb * (nb + 1) / 2, (unsigned)gc), dim3(256), 0, st, M);
    ELFIHIP_TRY(launch_status(ctx, "wide synthetic likelihood moments kernel"));
    WideFinArgs F;
    F.X = Xc;
    F.n = n;
    F.ldx = ldc;
    F.m = m;
    F.mpad = wide_mpad(m);
    F.pw = wide_pitch(m);
    F.variant = variant;
    F.y = dW ? dyw : dy;
    F.prefixes = M.prefixes;
    F.penalties = P > 0 ? dpar + B.pen : nullptr;
    F.konst = dpar + B.konst;
    F.K = Ke;
    F.P = P;
    F.snap = dsnap;
    F.slabs = dslab;
    F.group0 = g0;
    F.loglik = dll;
    F.mean = dmean;
    F.cov = dcov;
    for (int64_t j0 = 0; j0 < gc * group_jobs; j0 += Jc) {
      F.job0 = j0;
      const int64_t jc = std::min<int64_t>(Jc, gc * group_jobs - j0);
      hipLaunchKernelGGL(synlik_wide_finish_kernel, dim3((unsigned)jc), dim3(256), fin_lds, st, F);
      ELFIHIP_TRY(launch_status(ctx, "wide synthetic likelihood finish kernel"));
    }
  }
  return ELFIHIP_OK;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_syn_wide_set_cap(elfihip_ctx* ctx, int64_t bytes) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, bytes >= 0, "workspace cap %lld is negative", (long long)bytes);
  ctx->wide_cap = (size_t)bytes;
  return ELFIHIP_OK;
}

int elfihip_syn_loglik_wide_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx,
                                const double* dy, const double* dW, int variant, const int64_t* prefixes, int K,
                                const double* penalties, int P, double* dloglik, double* dmean, double* dcov) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(wide_check(ctx, dX, G, n, m, ldx, dy, variant, prefixes, K, penalties, P, dloglik));
  DeviceGuard g(ctx->device);
  return wide_dev_impl(ctx, dX, G, n, m, ldx, dy, dW, variant, prefixes, K, penalties, P, dloglik, dmean, dcov);
}

int elfihip_syn_loglik_wide(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* y,
                            const double* W, int variant, const int64_t* prefixes, int K, const double* penalties, int P,
                            double* loglik, double* mean, double* cov) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(wide_check(ctx, X, G, n, m, ldx, y, variant, prefixes, K, penalties, P, loglik));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)G * (size_t)n, md = (size_t)m * sizeof(double);
  const size_t nll = group_results(G, prefixes, K, P);
  // in: [X rows m][y m][W m m]; out: [loglik][mean G m][cov G m m]
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((rows * m + (size_t)m + (size_t)m * m) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((nll + (size_t)G * m + (size_t)G * m * m) * sizeof(double)));
  double* dX = ctx->in.as<double>();
  double* dy = dX + rows * m;
  double* dW = dy + m;
  double* dll = ctx->out.as<double>();
  double* dmean = dll + nll;
  double* dcov = dmean + (size_t)G * m;
  ELFIHIP_TRY(upload_rows(ctx, dX, X, rows, m, ldx));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dy, y, md, hipMemcpyHostToDevice, st));
  if (W) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dW, W, (size_t)m * md, hipMemcpyHostToDevice, st));
  ELFIHIP_TRY(wide_dev_impl(ctx, dX, G, n, m, m, dy, W ? dW : nullptr, variant, prefixes, K, penalties, P, dll,
                            mean ? dmean : nullptr, cov ? dcov : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(loglik, dll, nll * sizeof(double), hipMemcpyDeviceToHost, st));
  if (mean) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(mean, dmean, (size_t)G * md, hipMemcpyDeviceToHost, st));
  if (cov) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(cov, dcov, (size_t)G * m * md, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
