// The wide whitened semiparametric synthetic likelihood (wsemiBSL) on gfx950: 65 to 256 summaries, with the semantics of
// wsemibsl.hip.
//
// wsemibsl.hip keeps W, Q^T Q, rho and the factor in the LDS of one workgroup, which ends at 64 columns.  Here neither W (up
// to 512 KB) nor a covariance fits, so the work is cut as in semibsl_wide.hip -- the unit is the (group, prefix) job, with a
// global workspace between the kernels -- and the two products with W walk their inner index in slabs.
//
//   column     semibsl.hip's kernel in its wide layout: scores Q[job][column][row] at the padded row pitch NP, eta and logpdf
//              to the job's statistics.
//   transform  T[job][c][r] = sum_k Q[job][k][r] W[c][k] by v_mfma_f64_16x16x4_f64: one workgroup of 256 threads per (job,
//              chunk of 64 rows, block of 64 columns of T); a chunk that begins at or behind p returns at once.  k is walked
//              in slabs of 32: 32 columns of Q x 64 rows (each column a run of 64 consecutive doubles in global memory) and
//              the 64 x 32 piece of the W block are staged, then consumed.  A wave owns 16 rows x the block's four column
//              tiles.  Every element of T is ONE accumulator chain over k = 0, 4, 8, ... carried across the slabs, the same
//              chain for every row: a row of T depends on that row of Q and on W alone, so equal rows of Q give equal rows
//              of T wherever they sit (ties stay ties).  Columns >= m and rows >= p are staged as exact zeros.  The tile is
//              turned in LDS and stored in Q's layout, so the next kernel reads a column contiguously.
//   re-rank    wsemibsl.hip's kernel in the wide layout (semi_wide.hpp): one workgroup per (job, column), the column of T in
//              LDS, semi_rank.hpp's counting ranks; q' overwrites T in place, and goes to the caller's scores for the full
//              group.
//   gram       semibsl_wide.hip's kernel twice: on Q' it writes rho (and the caller's), on Q the covariance
//              C_ab = ((Q^T Q)_ab - s_a s_b / p) / (p - 1), symmetric to the bit, zero beyond m.
//   scale      one workgroup per (job, block of 64 rows of W), so C comes from L2 once per block and not once per row.  Per
//              block of 64 columns c: V = W C by MFMA (V_ac = sum_b W_ab C_cb, the chain b = 0, 4, 8, ... in slabs of 32 as
//              above; the row block of W is staged row-major), the tile turned in LDS, and a thread per row a carries
//              d_a^2 += W_ac V_ac and eta_w,a += W_ac eta_c over c in index order across the blocks.  d = sqrt(d^2) and
//              eta_w go to the job's whitened statistics, d of the full group to the caller's scale.
//   finish     semibsl_wide.hip's kernel with the scaled entry d_i ((1 - l) rho_ij + l [i == j]) d_j and eta_w as row m;
//              -inf before the factorisation if a d is not positive and finite, or p = 2.
//
// LDS pitches, reasoned on the 64-bank model (64 banks of 4 bytes; a 64-bit access is served 32 lanes at a time, free of
// conflicts when the 32 words fall into 32 different 8-byte bank pairs, i.e. are different mod 32) -- reasoning, not a
// measurement:
//   Q slab [k][row], pitch 80.   Staging: 32 consecutive lanes write 32 consecutive rows of one column.  A operand of lane
//                                (lr = lane >> 4, lc = lane & 15): word 80 (4 s + lr) + 16 wave + lc; a half-wave has two
//                                lr, i.e. two runs of 16 words 80 = 16 mod 32 apart.
//   W / C slab [c][k], pitch 34. Staging: a half-wave writes the 32 k of one row.  B operand: word 34 (16 tj + lc) + 4 s +
//                                lr = 2 lc + lr mod 32, all different over a half-wave.  The scale kernel's A operand (the
//                                row block of W, [a][k]) reads the same way.
//   turned tile [c][row], pitch 66.  Accumulator element r of a lane goes to word 66 (16 tj + lc) + 16 wave + lr + 4 r =
//                                2 lc + lr + const mod 32; it is read back along the rows, consecutive words.
// 4 736 doubles (37 888 bytes) of static LDS per workgroup: the two slabs, and the turned tile (4 224) in their place.
//
// Everything is f64, no atomics, every sum in a fixed order: one (group, prefix, penalty) result depends neither on G, K, P
// nor on how the host cuts the jobs into launches to keep the workspace under the context's cap; prefix p of a long group
// has the bits of a group of p rows.  -inf with the status left at ELFIHIP_OK: as wsemibsl.hip.
#include "semi_wide.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace elfihip {

constexpr int WW_ROWS = 64;    // rows of Q per workgroup of the transform, rows of W per workgroup of the scale: 16 per wave
constexpr int WW_KS = 32;      // k per slab (8 MFMA steps)
constexpr int WW_QP = 80;      // pitch of the Q slab [k][row]
constexpr int WW_WP = 34;      // pitch of a [row][k] slab
constexpr int WW_TP = 66;      // pitch of the turned tile [column][row]
constexpr int WW_LDS = WW_KS * WW_QP + SW_BLK * WW_WP;
static_assert(SW_BLK * WW_TP <= WW_LDS && 2 * SW_BLK * WW_WP <= WW_LDS);

// `steps` MFMA steps of a staged slab: acc[tj] += A (this wave's 16 rows x 4 steps k) B^T (column tile tj).  A element
// (row, k) is As[row AR + k AK]; B element (column, k) is Bs[column WW_WP + k].
template <int AR, int AK>
__device__ __forceinline__ void slab_mfma(v4d (&acc)[4], const double* As, const double* Bs, int steps, int wv, int lr, int lc) {
  const double* a = As + (16 * wv + lc) * AR + lr * AK;
  const double* b = Bs + lc * WW_WP + lr;
  for (int s = 0; s < steps; ++s) {
    const double av = a[4 * s * AK];
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[16 * tj * WW_WP + 4 * s], acc[tj], 0, 0, 0);
  }
}

// The wave's 16 x 64 accumulators into the turned tile Ts[column][row]: D[row lr + 4 r][column lc] of tile tj.
__device__ __forceinline__ void turn_tile(const v4d (&acc)[4], double* Ts, int wv, int lr, int lc) {
#pragma unroll
  for (int tj = 0; tj < 4; ++tj)
#pragma unroll
    for (int r = 0; r < 4; ++r) Ts[(16 * tj + lc) * WW_TP + 16 * wv + lr + 4 * r] = acc[tj][r];
}

// A 64 x 32 piece of a row-major matrix (rows row0 .., columns k0 .., pitch ld) into a [row][k] slab; zero from row `rows`
// and column `cols` on.
__device__ __forceinline__ void stage_rows(double* S, const double* M, int ld, int row0, int rows, int k0, int cols) {
  for (int e = threadIdx.x; e < SW_BLK * WW_KS; e += 256) {
    const int rr = e / WW_KS, kk = e - rr * WW_KS;
    const int row = row0 + rr, k = k0 + kk;
    S[rr * WW_WP + kk] = (row < rows && k < cols) ? M[(size_t)row * ld + k] : 0.0;
  }
}

__global__ __launch_bounds__(256) void wsemi_wide_transform_kernel(WsemiWideArgs A) {
  __shared__ __align__(16) double lds[WW_LDS];
  double* Qs = lds;                    // (WW_KS, WW_QP) columns k0 .. of Q, this chunk's rows
  double* Ws = lds + WW_KS * WW_QP;    // (64, WW_WP) rows 64 cb .. of W, columns k0 ..
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = A.S.m, NP = A.S.NP;
  const int lr = lane >> 4, lc = lane & 15;
  unsigned b = blockIdx.x;
  const int cb = (int)(b % (unsigned)A.nb);
  b /= (unsigned)A.nb;
  const int chunk = (int)(b % (unsigned)A.chunks);
  const int64_t lj = b / (unsigned)A.chunks;
  const int64_t gk = A.S.job0 + lj;
  const int p = (int)A.S.prefixes[gk % A.S.K];
  const int r0 = chunk * WW_ROWS;
  if (r0 >= p) return;   // the same for every thread
  const double* Qj = A.S.Q + lj * m * NP;
  v4d acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = (v4d){0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < m; k0 += WW_KS) {
    __syncthreads();  // the previous slab is consumed
    for (int e = tid; e < WW_KS * WW_ROWS; e += 256) {
      const int kk = e / WW_ROWS, rr = e - kk * WW_ROWS;
      const int k = k0 + kk, r = r0 + rr;
      Qs[kk * WW_QP + rr] = (k < m && r < p) ? Qj[(int64_t)k * NP + r] : 0.0;
    }
    stage_rows(Ws, A.W, m, SW_BLK * cb, m, k0, m);
    __syncthreads();
    const int left = (m - k0 + 3) / 4;
    slab_mfma<1, WW_QP>(acc, Qs, Ws, left < WW_KS / 4 ? left : WW_KS / 4, wv, lr, lc);
  }
  __syncthreads();   // the slabs are consumed: the turned tile takes their place
  turn_tile(acc, lds, wv, lr, lc);
  __syncthreads();
  double* Tj = A.T + lj * m * NP;
  for (int e = tid; e < SW_BLK * WW_ROWS; e += 256) {
    const int cc = e / WW_ROWS, rr = e - cc * WW_ROWS;
    const int c = SW_BLK * cb + cc, r = r0 + rr;
    if (c < m && r < p) Tj[(int64_t)c * NP + r] = lds[cc * WW_TP + rr];
  }
}

__global__ __launch_bounds__(256) void wsemi_wide_scale_kernel(WsemiWideArgs A) {
  __shared__ __align__(16) double lds[WW_LDS];
  __shared__ double eta[SEMI_WIDE_M];
  double* As = lds;                     // (64, WW_WP) rows 64 rb .. of W, columns k0 ..
  double* Bs = lds + SW_BLK * WW_WP;    // (64, WW_WP) rows 64 cb .. of C, columns k0 ..
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = A.S.m, mpad = A.mpad;
  const int lr = lane >> 4, lc = lane & 15;
  const int rb = (int)(blockIdx.x % (unsigned)A.nb);
  const int64_t lj = blockIdx.x / (unsigned)A.nb;
  const int64_t gk = A.S.job0 + lj;
  const int p = (int)A.S.prefixes[gk % A.S.K];
  const double* Cj = A.C + (size_t)lj * mpad * mpad;
  if (tid < m) eta[tid] = A.S.stats[lj * SEMI_WIDE_STATS + tid];
  const int a = SW_BLK * rb + tid;   // the row of the threads that carry the sums
  const bool mine = tid < SW_BLK && a < m;
  double d2 = 0.0, ew = 0.0;
  for (int cb = 0; cb < A.nb; ++cb) {
    v4d acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < m; k0 += WW_KS) {
      __syncthreads();  // the previous slab, or the turned tile, is consumed
      stage_rows(As, A.W, m, SW_BLK * rb, m, k0, m);
      stage_rows(Bs, Cj, mpad, SW_BLK * cb, mpad, k0, m);
      __syncthreads();
      const int left = (m - k0 + 3) / 4;
      slab_mfma<WW_WP, 1>(acc, As, Bs, left < WW_KS / 4 ? left : WW_KS / 4, wv, lr, lc);
    }
    __syncthreads();
    turn_tile(acc, lds, wv, lr, lc);   // V[a][c] at lds[c][a]
    __syncthreads();
    if (mine) {
      const int c1 = m - SW_BLK * cb < SW_BLK ? m - SW_BLK * cb : SW_BLK;
      const double* wa = A.W + (size_t)a * m + SW_BLK * cb;
      for (int cc = 0; cc < c1; ++cc) {
        const double w = wa[cc];
        d2 += w * lds[cc * WW_TP + tid];
        ew += w * eta[SW_BLK * cb + cc];
      }
    }
  }
  if (mine) {
    const double d = sqrt(d2);
    double* ws = A.wst + lj * WSEMI_WIDE_STATS;
    ws[a] = d;
    ws[SEMI_WIDE_M + a] = ew;
    if (A.scale && p == A.S.n) A.scale[(gk / A.S.K) * m + a] = d;
  }
}

static int wsemi_wide_check(elfihip_ctx* ctx, const void* X, int64_t G, int64_t n, int m, int64_t ldx, const void* y,
                            const void* W, const int64_t* prefixes, int K, const double* penalties, int P, const void* loglik) {
  ELFIHIP_REQUIRE(ctx, m >= SW_MIN_M && m <= SW_MAX_M,
                  "wide whitened semiparametric likelihood: %d summaries; %d to %d are supported (elfihip_wsemi_loglik takes 1 to %d)",
                  m, SW_MIN_M, SW_MAX_M, SW_MIN_M - 1);
  ELFIHIP_REQUIRE(ctx, n >= 2 && n <= SEMI_MAX_N,
                  "wide whitened semiparametric likelihood: %lld rows per group; 2 to %d are supported", (long long)n, SEMI_MAX_N);
  ELFIHIP_REQUIRE(ctx, G >= 1 && G <= 0x7fffffff && ldx >= m, "bad shape G=%lld n=%lld m=%d ldx=%lld", (long long)G,
                  (long long)n, m, (long long)ldx);
  ELFIHIP_REQUIRE(ctx, X && y && loglik, "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, W, "the whitening matrix is NULL");
  const std::string bad = group_lists_error(prefixes, K, penalties, P, n);
  ELFIHIP_REQUIRE(ctx, bad.empty(), "%s", bad.c_str());
  return ELFIHIP_OK;
}

// Device rows, y, W and outputs; host prefixes and penalties (checked above).
static int wsemi_wide_dev_impl(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                               const double* dW, const int64_t* prefixes, int K, const double* penalties, int P, double* dll,
                               double* du, double* drho, double* dscale, double* dscores) {
  hipStream_t st = ctx->stream;
  const GroupParams B = group_params(prefixes, K, n, nullptr, penalties, P);
  double* dpar;
  ELFIHIP_TRY(upload_group_params(ctx, B, 0, &dpar));
  const int Ke = B.Ke, Pe = P > 0 ? P : 1;
  const int mpad = wide_mpad(m), pw = wide_pitch(m), NP = (int)((n + SMW_RC - 1) / SMW_RC * SMW_RC);
  const int nb = mpad / SW_BLK, pairs = nb * (nb + 1) / 2, chunks = (int)((n + WW_ROWS - 1) / WW_ROWS);

  // The workspace, in doubles: [Q of Jc jobs][their T, then Q'][rho][C][statistics][whitened statistics][Fc slabs].  Half the
  // cap bounds the jobs' part, half the slabs; one job and one slab are the least a launch needs.  A launch has at most
  // 2^31 - 1 workgroups: Jc m of the column and re-rank kernels, Jc chunks nb of the transform (pairs < m and nb < m, so the
  // gram and scale kernels fit as well) and Fc of the finish kernel.
  const size_t cap = (ctx->wide_cap ? ctx->wide_cap : SW_SCRATCH_CAP) / sizeof(double);
  const size_t qd = (size_t)m * NP, rd = (size_t)mpad * mpad, slab = wide_slab(m);
  const size_t per_job = 2 * qd + 2 * rd + SEMI_WIDE_STATS + WSEMI_WIDE_STATS;
  const int64_t J = G * Ke;
  const size_t most = (size_t)(0x7fffffff / std::max(m, chunks * nb));
  const int64_t Jc = (int64_t)std::min<size_t>(std::min<size_t>((size_t)J, most), std::max<size_t>(1, cap / 2 / per_job));
  const int64_t Fc = (int64_t)std::min<size_t>(std::min<size_t>((size_t)Jc * Pe, 0x7fffffff), std::max<size_t>(1, cap / 2 / slab));
  ELFIHIP_CHECK_HIP(ctx, ctx->scratch.reserve(((size_t)Jc * per_job + (size_t)Fc * slab) * sizeof(double)));

  WsemiWideArgs A;
  SemiWideArgs& C = A.S;
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
  double* dT = C.Q + (size_t)Jc * qd;
  double* dR = dT + (size_t)Jc * qd;
  double* dC = dR + (size_t)Jc * rd;
  C.stats = dC + (size_t)Jc * rd;
  C.loglik = dll;
  C.u = du;
  C.rho = nullptr;      // the gram kernel's
  C.scores = nullptr;   // the re-rank kernel's
  C.NP = NP;
  A.W = dW;
  A.T = A.Q2 = dT;
  A.C = dC;
  A.wst = C.stats + (size_t)Jc * SEMI_WIDE_STATS;
  A.scale = dscale;
  A.scores = dscores;
  A.chunks = chunks;
  A.nb = nb;
  A.mpad = mpad;
  SemiGramArgs M;
  M.Q = dT;
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
  SemiCovArgs V;
  static_cast<SemiGramArgs&>(V) = M;
  V.Q = C.Q;
  V.R = dC;
  V.rho = nullptr;
  WsemiWideFinArgs F;
  F.R = dR;
  F.stats = C.stats;
  F.wst = A.wst;
  F.slabs = A.wst + (size_t)Jc * WSEMI_WIDE_STATS;
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
    C.job0 = M.job0 = V.job0 = F.job0 = j0;
    ELFIHIP_TRY(semibsl_launch_column_wide(ctx, C, jc));
    hipLaunchKernelGGL(wsemi_wide_transform_kernel, dim3((unsigned)(jc * chunks * nb)), dim3(256), 0, st, A);
    ELFIHIP_TRY(launch_status(ctx, "wide whitened semiparametric likelihood transform kernel"));
    ELFIHIP_TRY(wsemi_launch_rerank_wide(ctx, A, jc));
    ELFIHIP_TRY(semibsl_wide_launch_gram(ctx, M, jc));
    ELFIHIP_TRY(semibsl_wide_launch_cov(ctx, V, jc));
    hipLaunchKernelGGL(wsemi_wide_scale_kernel, dim3((unsigned)(jc * nb)), dim3(256), 0, st, A);
    ELFIHIP_TRY(launch_status(ctx, "wide whitened semiparametric likelihood scale kernel"));
    for (int64_t f0 = 0; f0 < jc * Pe; f0 += Fc) {
      F.fjob0 = f0;
      ELFIHIP_TRY(semibsl_wide_launch_finish_scaled(ctx, F, std::min<int64_t>(Fc, jc * Pe - f0)));
    }
  }
  return ELFIHIP_OK;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_wsemi_loglik_wide_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx,
                                  const double* dy, const double* dW, const int64_t* prefixes, int K, const double* penalties,
                                  int P, double* dloglik, double* du, double* drho, double* dscale, double* dscores) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(wsemi_wide_check(ctx, dX, G, n, m, ldx, dy, dW, prefixes, K, penalties, P, dloglik));
  DeviceGuard g(ctx->device);
  return wsemi_wide_dev_impl(ctx, dX, G, n, m, ldx, dy, dW, prefixes, K, penalties, P, dloglik, du, drho, dscale, dscores);
}

int elfihip_wsemi_loglik_wide(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* y,
                              const double* W, const int64_t* prefixes, int K, const double* penalties, int P, double* loglik,
                              double* u, double* rho, double* scale, double* scores) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(wsemi_wide_check(ctx, X, G, n, m, ldx, y, W, prefixes, K, penalties, P, loglik));
  for (int e = 0; e < m * m; ++e)
    ELFIHIP_REQUIRE(ctx, std::isfinite(W[e]), "the whitening matrix has a non-finite entry (row %d, column %d)", e / m, e % m);
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)G * (size_t)n, md = (size_t)m * sizeof(double);
  const size_t nll = group_results(G, prefixes, K, P);
  // in: [X rows m][y m][W m m]; out: [loglik][u G m][rho G m m][scale G m][scores G n m]
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((rows * m + (size_t)m + (size_t)m * m) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((nll + 2 * (size_t)G * m + (size_t)G * m * m + (scores ? rows * m : 0)) * sizeof(double)));
  double* dX = ctx->in.as<double>();
  double* dy = dX + rows * m;
  double* dW = dy + m;
  double* dll = ctx->out.as<double>();
  double* du = dll + nll;
  double* drho = du + (size_t)G * m;
  double* dsc = drho + (size_t)G * m * m;
  double* dsco = dsc + (size_t)G * m;
  ELFIHIP_TRY(upload_rows(ctx, dX, X, rows, m, ldx));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dy, y, md, hipMemcpyHostToDevice, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dW, W, (size_t)m * md, hipMemcpyHostToDevice, st));
  ELFIHIP_TRY(wsemi_wide_dev_impl(ctx, dX, G, n, m, m, dy, dW, prefixes, K, penalties, P, dll, u ? du : nullptr,
                                  rho ? drho : nullptr, scale ? dsc : nullptr, scores ? dsco : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(loglik, dll, nll * sizeof(double), hipMemcpyDeviceToHost, st));
  if (u) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(u, du, (size_t)G * md, hipMemcpyDeviceToHost, st));
  if (rho) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(rho, drho, (size_t)G * m * md, hipMemcpyDeviceToHost, st));
  if (scale) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(scale, dsc, (size_t)G * md, hipMemcpyDeviceToHost, st));
  if (scores) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(scores, dsco, rows * md, hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
