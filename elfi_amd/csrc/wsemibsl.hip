// Batched whitened semiparametric synthetic likelihood (wsemiBSL; Priddle, Sisson, Frazier, Turner & Drovandi 2021) on
// gfx950: the semiparametric likelihood of semibsl.hip with the normal scores decorrelated by a whitening matrix W, so
// that heavy shrinkage of the rank correlation costs little.
//
// Replaces, for G groups x K prefixes x P penalties at once, the whitening branch of
// elfi/methods/bsl/pdf_methods.py:213-264 (semi_param_kernel_estimate) and gaussian_copula_density.py:33-60.  For the
// first p rows of a group, observed y, W (m x m) and a Warton penalty l:
//   column     (semibsl.hip's kernel, unchanged) per column j the KDE logpdf_j at y_j, u_j = min(1, mean_i Phi(z_ij)),
//              eta_j = Phi^-1(u_j), the normal scores q_ij = Phi^-1(rank_ij / (p + 1)) and the denominator
//              sum_{i=1..p} Phi^-1(i / (p + 1))^2.
//   transform  T = Q W^T by v_mfma_f64_16x16x4_f64.  One workgroup of 256 threads per (group, prefix, chunk of 64 rows):
//              a group of 16384 rows is 256 workgroups.  W sits in LDS once per workgroup, the 64 rows of Q next to it,
//              both at a pitch = 2 mod 32 doubles: the 32 lanes of an operand read (16 rows x 2 neighbouring k) fall
//              into 32 different 8-byte banks.  A wave owns 16 rows: it keeps their operands in registers (16 tj-loops
//              reuse them), and every element of T is the accumulator chain over k = 0, 4, 8 ... of one MFMA lane
//              position -- the same chain for every row, so a row of T depends on that row of Q and on W alone and
//              two equal rows of Q give equal rows of T wherever they sit (ties stay ties).  Columns >= m and rows >= p
//              are staged as exact zeros.  The tile is turned in LDS and stored column-major, T (G K, m, n): the next
//              kernel reads a column contiguously.
//   re-rank    one workgroup per (group, prefix, column): the column of T in LDS (at most 128 KB), ranks by counting
//              with ties at the average rank (semi_rank.hpp: the code of the column kernel), q'_ij = Phi^-1(rank'_ij /
//              (p + 1)) into a second score matrix laid out as Q.
//   finish     one workgroup per (group, prefix), templated on the tile count.  One pass of 32-row chunks stages Q' and Q
//              side by side: Q'^T Q' and Q^T Q by MFMA with the two-level summation of syn_gram.hpp, the column sums
//              s of Q by the same two levels (a thread per column: the 32 staged rows in order, then the total).  Then
//                rho_ab = (Q'^T Q')_ab / denominator, rho_aa = 1
//                C_ab   = ((Q^T Q)_ab - s_a s_b / p) / (p - 1)                 (cov(Q), ddof 1; the means are not zero
//                                                                               once there are ties)
//                d_a^2  = w_a^T C w_a   (four threads per a take 16 rows of C each, summed b ascending, c ascending;
//                                        the four parts are added in order), eta_w = W eta (b ascending)
//              and per penalty  M = diag(d) ((1 - l) rho + l I) diag(d)  (the shrinkage before the scaling, as the
//              reference orders it), its Cholesky factor with eta_w as the extra row, and
//                loglik = -(log|M| + eta_w^T M^-1 eta_w - eta_w^T eta_w) / 2 + sum_j logpdf_j.
//              LDS at four tiles: the stage of both chunks (40 KB; W moves into it once the sums are done), rho, and
//              the buffer of the factor (C sits in it until d is known): 111 KB.
// Every sum is a fixed order: no atomics, nothing depends on G, on the other prefixes or on the other penalties -- prefix
// p of a long group has the bits of a group of p rows.
// -inf, with the status left at ELFIHIP_OK: semibsl.hip's list (a u_j of 0 or 1, a column without spread, a non-positive
// pivot, a non-finite value, two rows and m > 1) and a d_a that is not positive and finite.  A decided divergence: the
// reference lets W eta turn an infinite eta_j (u_j of 0 or 1) into NaN where W has a zero, and returns NaN; here it is -inf.
#include "semi_wide.hpp"

#include <algorithm>
#include <cmath>
#include <type_traits>

#pragma clang fp contract(off)

namespace elfihip {

constexpr int WS_ROWS = 64;   // rows of Q per workgroup of the transform: 16 per wave

struct WsemiArgs {
  SemiArgs S;        // the column kernel's arguments (its rho and scores NULL: the outputs below are of the transformed scores)
  const double* W;   // (m, m) row-major, pitch m
  double* T;         // scratch (G K, m, n): the transformed scores, column-major
  double* Q2;        // scratch (G K, n, MP): the scores of T's columns
  int chunks;        // 64-row chunks of n rows
  double* rho;       // (G, m, m) or NULL
  double* scale;     // (G, m) or NULL
  double* scores;    // (G, n, m) or NULL
};

template <int T>
struct TransformShape {
  static constexpr int MP = 16 * T;
  static constexpr int WP = MP + 2;      // pitch of W and of the staged rows: 2 mod 32 or 18 mod 32
  static constexpr int TP = WS_ROWS + 1; // pitch of the turned tile (a column of 64 rows)
  static constexpr int DOUBLES = (MP + WS_ROWS) * WP;
  static_assert(MP * TP <= WS_ROWS * WP);   // the turned tile fits where the rows were
};

template <int T>
__global__ __launch_bounds__(256) void wsemi_transform_kernel(WsemiArgs A) {
  using Sh = TransformShape<T>;
  constexpr int MP = Sh::MP, WP = Sh::WP, TP = Sh::TP;
  extern __shared__ __align__(16) double lds[];
  double* Ws = lds;             // (MP, WP) W, zero beyond m
  double* Qs = lds + MP * WP;   // (WS_ROWS, WP) rows of Q, zero beyond p and beyond m; then the turned tile (MP, TP)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = A.S.m;
  const int lr = lane >> 4, lc = lane & 15;
  const int chunk = (int)(blockIdx.x % (unsigned)A.chunks);
  const int64_t gk = blockIdx.x / (unsigned)A.chunks;
  const int p = (int)A.S.prefixes[gk % A.S.K];
  const int r0 = chunk * WS_ROWS;
  if (r0 >= p) return;   // the same for every thread
  const int64_t n = A.S.n;
  const double* Qg = A.S.Q + gk * n * MP;
  for (int e = tid; e < MP * MP; e += 256) {
    const int a = e / MP, b = e - a * MP;
    Ws[a * WP + b] = (a < m && b < m) ? A.W[a * m + b] : 0.0;
  }
  for (int e = tid; e < WS_ROWS * MP; e += 256) {
    const int rr = e / MP, c = e - rr * MP;
    const int r = r0 + rr;
    Qs[rr * WP + c] = (r < p && c < m) ? Qg[(int64_t)r * MP + c] : 0.0;
  }
  __syncthreads();
  // A operand: lane holds Q[row lc of the wave's 16][k = 4 s + lr]; B operand: W^T[k][j] = W[j = lc of tile tj][k]
  double a[4 * T];
#pragma unroll
  for (int s = 0; s < 4 * T; ++s) a[s] = Qs[(16 * wv + lc) * WP + 4 * s + lr];
  __syncthreads();   // every wave has its rows: the buffer is free for the turned tile
#pragma unroll
  for (int tj = 0; tj < T; ++tj) {
    v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4 * T; ++s)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], Ws[(16 * tj + lc) * WP + 4 * s + lr], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) Qs[(16 * tj + lc) * TP + 16 * wv + lr + 4 * r] = acc[r];   // D[row lr + 4 r][col lc]
  }
  __syncthreads();
  double* Tg = A.T + gk * m * n;
  for (int e = tid; e < MP * WS_ROWS; e += 256) {
    const int c = e / WS_ROWS, rr = e - c * WS_ROWS;
    const int r = r0 + rr;
    if (c < m && r < p) Tg[(int64_t)c * n + r] = Qs[c * TP + rr];
  }
}

// Args picks the layout: WsemiArgs T (G K, m, n) and Q2 row-major at pitch MP; WsemiWideArgs (semi_wide.hpp) the wide one
// of wsemibsl_wide.hip, T and Q2 (jobs, m, NP) of a launch that holds a part of the call's jobs.  Q2 may be T there: a
// workgroup has read its column before it writes it.
template <class Args>
__global__ __launch_bounds__(256) void wsemi_rerank_kernel(Args A) {
  constexpr bool WIDE = std::is_same<Args, WsemiWideArgs>::value;
  extern __shared__ __align__(16) double lds[];
  double* col = lds;   // the column of T, NaN up to a multiple of 4
  const int tid = threadIdx.x, m = A.S.m;
  const int j = (int)(blockIdx.x % (unsigned)m);
  const int64_t lj = blockIdx.x / (unsigned)m;   // the job within the launch
  int64_t gk = lj;
  if constexpr (WIDE) gk += A.S.job0;
  const int64_t g = gk / A.S.K, n = A.S.n;
  const int p = (int)A.S.prefixes[gk % A.S.K];
  const int pp = (p + 3) & ~3;
  const bool full = p == n;
  const double* Tc;
  if constexpr (WIDE)
    Tc = A.T + (lj * m + j) * A.S.NP;
  else
    Tc = A.T + (gk * m + j) * n;
  for (int i = tid; i < pp; i += 256) col[i] = i < p ? Tc[i] : NAN;
  __syncthreads();
  const double np1 = (double)p + 1.0;
  double* Qg;
  int64_t qp = 1;   // pitch of consecutive rows
  if constexpr (WIDE) {
    Qg = A.Q2 + (lj * m + j) * A.S.NP;
  } else {
    Qg = A.Q2 + gk * n * A.S.MP + j;
    qp = A.S.MP;
  }
  const double2* col2 = reinterpret_cast<const double2*>(col);
  for (int i = tid; i < p; i += 256) {
    const double q = rank_score(col2, pp, col[i], np1);
    Qg[(int64_t)i * qp] = q;
    if (A.scores && full) A.scores[(g * n + i) * m + j] = q;
  }
}

template <class Args>
static int launch_rerank(elfihip_ctx* ctx, const Args& A, int64_t jobs, const char* name) {
  const size_t bytes = (size_t)((A.S.n + 3) & ~(int64_t)3) * sizeof(double);
  ELFIHIP_TRY(set_lds(ctx, wsemi_rerank_kernel<Args>, bytes, 48 * 1024));
  hipLaunchKernelGGL(wsemi_rerank_kernel<Args>, dim3((unsigned)(jobs * A.S.m)), dim3(256), bytes, ctx->stream, A);
  return launch_status(ctx, name);
}

int wsemi_launch_rerank_wide(elfihip_ctx* ctx, const WsemiWideArgs& A, int64_t jobs) {
  return launch_rerank(ctx, A, jobs, "wide whitened semiparametric likelihood re-rank kernel");
}

template <int T>
struct WsemiShape : GramShape<T> {
  using GramShape<T>::MP;
  using GramShape<T>::SP;
  using GramShape<T>::LP;
  static constexpr int STAGE = 2 * SL_RC * SP;   // a chunk of Q' and a chunk of Q; afterwards W (MP, LP)
  static constexpr int VECS = 6 * MP + 4 * SL_MAX_M + 8;
  static constexpr int DOUBLES = STAGE + MP * LP + (MP + 1) * LP + VECS;
  static_assert(MP * LP <= STAGE);
  static_assert(DOUBLES * sizeof(double) <= 160 * 1024);
};

template <int T>
__global__ __launch_bounds__(256) void wsemi_finish_kernel(WsemiArgs A) {
  using Sh = WsemiShape<T>;
  constexpr int MP = Sh::MP, SP = Sh::SP, LP = Sh::LP, NT = Sh::NT;
  extern __shared__ __align__(16) double lds[];
  double* stage2 = lds;                  // (SL_RC, SP) transformed scores Q', zero beyond p and beyond m
  double* stage1 = lds + SL_RC * SP;     // (SL_RC, SP) scores Q
  double* Wl = lds;                      // (MP, LP) W, once the sums are done
  double* S = lds + Sh::STAGE;           // (MP, LP) Q'^T Q', then rho
  double* L = S + MP * LP;               // (MP + 1, LP) Q^T Q, then C; then the matrix being factorised + eta_w
  double* eta = L + (MP + 1) * LP;
  double* lpv = eta + MP;                // logpdf of the columns
  double* dg = lpv + MP;                 // diagonal of the factor
  double* csum = dg + MP;                // column sums of Q
  double* dsc = csum + MP;               // d
  double* etw = dsc + MP;                // W eta
  double* part = etw + MP;               // (4, SL_MAX_M) the four parts of d^2
  double* flag = part + 4 * SL_MAX_M;    // not 0: a d_a that is not positive and finite
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = A.S.m;
  const int tx = tid & 15, ty = tid >> 4;
  const int64_t gk = blockIdx.x;
  const int k = (int)(gk % A.S.K);
  const int64_t g = gk / A.S.K;
  const int p = (int)A.S.prefixes[k];
  const bool full = p == A.S.n;
  const double* Q1 = A.S.Q + gk * A.S.n * MP;
  const double* Q2 = A.Q2 + gk * A.S.n * MP;
  const double* st = A.S.stats + gk * SEMI_STATS;
  if (tid < MP) {
    eta[tid] = tid < m ? st[tid] : 0.0;
    lpv[tid] = tid < m ? st[SL_MAX_M + tid] : 0.0;
  }
  if (tid == 0) flag[0] = 0.0;
  const double den = st[2 * SL_MAX_M];

  v4d tot2[NT], tot1[NT], chk[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) tot2[i] = tot1[i] = (v4d){0.0, 0.0, 0.0, 0.0};
  double stot = 0.0;
  const int lr = lane >> 4, lc = lane & 15;
  for (int r0 = 0; r0 < p; r0 += SL_RC) {
    __syncthreads();  // the previous chunk is consumed
    for (int e = tid; e < SL_RC * MP; e += 256) {
      const int rr = e / MP, c = e - rr * MP;
      const int r = r0 + rr;
      const bool in = r < p && c < m;
      stage2[rr * SP + c] = in ? Q2[(int64_t)r * MP + c] : 0.0;
      stage1[rr * SP + c] = in ? Q1[(int64_t)r * MP + c] : 0.0;
    }
    __syncthreads();
    const int nr = p - r0 < SL_RC ? p - r0 : SL_RC;
#pragma unroll
    for (int i = 0; i < NT; ++i) chk[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int s = 0; 4 * s < nr; ++s) gram_step<T>(chk, stage2 + (4 * s + lr) * SP + lc, wv);
#pragma unroll
    for (int i = 0; i < NT; ++i) tot2[i] += chk[i];
#pragma unroll
    for (int i = 0; i < NT; ++i) chk[i] = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int s = 0; 4 * s < nr; ++s) gram_step<T>(chk, stage1 + (4 * s + lr) * SP + lc, wv);
#pragma unroll
    for (int i = 0; i < NT; ++i) tot1[i] += chk[i];
    if (tid < MP) {
      double sc = 0.0;
      for (int rr = 0; rr < SL_RC; ++rr) sc += stage1[rr * SP + tid];   // rows beyond p are zeros
      stot += sc;
    }
  }
  __syncthreads();   // the stage is consumed: W takes its place
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int q = wv + 4 * i;
    if (q < T * T) {
      const int ti = q / T, tj = q - ti * T;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        S[(16 * ti + lr + 4 * r) * LP + 16 * tj + lc] = tot2[i][r];
        L[(16 * ti + lr + 4 * r) * LP + 16 * tj + lc] = tot1[i][r];
      }
    }
  }
  if (tid < MP) csum[tid] = stot;
  for (int e = tid; e < m * m; e += 256) {
    const int a = e / m, b = e - a * m;
    Wl[a * LP + b] = A.W[e];
  }
  __syncthreads();
  const double dp = (double)p;
  for (int i = ty; i < m; i += 16)
    for (int j = tx; j < m; j += 16) {
      const double v = i == j ? 1.0 : S[i * LP + j] / den;
      S[i * LP + j] = v;
      if (A.rho && full) A.rho[(g * m + i) * m + j] = v;
      L[i * LP + j] = (L[i * LP + j] - csum[i] * csum[j] / dp) / (dp - 1.0);   // C
    }
  __syncthreads();
  // d_a^2 = w_a^T C w_a: thread (a, part) sums rows b = 16 part ... of C
  {
    const int a = tid & 63, pt = tid >> 6;
    double acc = 0.0;
    if (a < m) {
      const int b1 = 16 * pt + 16 < m ? 16 * pt + 16 : m;
      for (int b = 16 * pt; b < b1; ++b) {
        double t = 0.0;
        for (int c = 0; c < m; ++c) t += L[b * LP + c] * Wl[a * LP + c];
        acc += Wl[a * LP + b] * t;
      }
    }
    part[pt * SL_MAX_M + a] = acc;
  }
  __syncthreads();
  if (tid < m) {
    const double d2 = ((part[tid] + part[SL_MAX_M + tid]) + part[2 * SL_MAX_M + tid]) + part[3 * SL_MAX_M + tid];
    const double d = sqrt(d2);
    if (!(d2 > 0.0 && d2 <= 1.7976931348623157e308)) flag[0] = 1.0;   // every writer writes the same value
    dsc[tid] = d;
    if (A.scale && full) A.scale[g * m + tid] = d;
    double ew = 0.0;
    for (int b = 0; b < m; ++b) ew += Wl[tid * LP + b] * eta[b];
    etw[tid] = ew;
  }
  const int Pe = A.S.P > 0 ? A.S.P : 1;
  for (int pi = 0; pi < Pe; ++pi) {
    __syncthreads();
    const double lam = A.S.P > 0 ? A.S.penalties[pi] : 0.0;
    const double gam = 1.0 - lam;
    for (int i = ty; i < m; i += 16)
      for (int j = tx; j <= i; j += 16) L[i * LP + j] = dsc[i] * ((i == j ? gam + lam : gam * S[i * LP + j]) * dsc[j]);
    if (tid < m) L[m * LP + tid] = etw[tid];   // eta_w as row m of the factor: its forward solve is the factorisation's own update
    __syncthreads();
    const bool ok = flag[0] == 0.0 && chol_extra_row<LP>(L, dg, m);
    if (tid == 0) {
      double ll = -INFINITY;
      if (ok && !(p == 2 && m > 1)) {
        double quad = 0.0, ee = 0.0, logdet = 0.0, lps = 0.0;
        for (int j = 0; j < m; ++j) {
          const double z = L[m * LP + j];
          quad += z * z;
          ee += etw[j] * etw[j];
          logdet += log(dg[j]);
          lps += lpv[j];
        }
        ll = -0.5 * (2.0 * logdet + (quad - ee)) + lps;
        if (!(fabs(ll) <= 1.7976931348623157e308)) ll = -INFINITY;   // NaN or an infinity of either sign
      }
      A.S.loglik[(gk * Pe) + pi] = ll;
    }
  }
}

static int wsemi_check(elfihip_ctx* ctx, const void* X, int64_t G, int64_t n, int m, int64_t ldx, const void* y,
                       const void* W, const int64_t* prefixes, int K, const double* penalties, int P, const void* loglik) {
  ELFIHIP_TRY(semi_check(ctx, "whitened semiparametric likelihood", X, G, n, m, ldx, y, loglik));
  ELFIHIP_REQUIRE(ctx, W, "the whitening matrix is NULL");
  const int64_t Ke = prefixes ? K : 1, chunks = (n + WS_ROWS - 1) / WS_ROWS;
  ELFIHIP_REQUIRE(ctx, G * Ke * std::max<int64_t>(m, chunks) <= 0x7fffffff, "G K = %lld x %d: the workgroups are too many",
                  (long long)G, (int)Ke);
  const std::string bad = group_lists_error(prefixes, K, penalties, P, n);
  ELFIHIP_REQUIRE(ctx, bad.empty(), "%s", bad.c_str());
  return ELFIHIP_OK;
}

// Device rows, y, W and outputs; host prefixes and penalties (checked above).
static int wsemi_dev_impl(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                          const double* dW, const int64_t* prefixes, int K, const double* penalties, int P, double* dll,
                          double* du, double* drho, double* dscale, double* dscores) {
  const int64_t GK = G * (prefixes ? K : 1);
  // scratch: [Q][Q'][T][stats], Q' and T between semi_setup's two
  const size_t qd = (size_t)GK * (size_t)n * (16 * group_tiles(m)), td = (size_t)GK * (size_t)n * m;
  WsemiArgs A;
  ELFIHIP_TRY(semi_setup(ctx, A.S, dX, G, n, m, ldx, dy, prefixes, K, penalties, P, qd + td, dll, du, nullptr, nullptr));
  A.Q2 = A.S.Q + qd;
  A.T = A.Q2 + qd;
  A.W = dW;
  A.chunks = (int)((n + WS_ROWS - 1) / WS_ROWS);
  A.rho = drho;
  A.scale = dscale;
  A.scores = dscores;
  ELFIHIP_TRY(semibsl_launch_column(ctx, A.S, GK));
  ELFIHIP_TRY(launch_by_tiles(
      ctx, m, (unsigned)(GK * A.chunks), "whitened semiparametric likelihood transform kernel",
      [](auto T) { return wsemi_transform_kernel<decltype(T)::value>; },
      [](auto T) { return (size_t)TransformShape<decltype(T)::value>::DOUBLES * sizeof(double); }, A));
  ELFIHIP_TRY(launch_rerank(ctx, A, GK, "whitened semiparametric likelihood re-rank kernel"));
  return launch_by_tiles(
      ctx, m, (unsigned)GK, "whitened semiparametric likelihood finish kernel",
      [](auto T) { return wsemi_finish_kernel<decltype(T)::value>; },
      [](auto T) { return (size_t)WsemiShape<decltype(T)::value>::DOUBLES * sizeof(double); }, A);
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_wsemi_loglik_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                             const double* dW, const int64_t* prefixes, int K, const double* penalties, int P,
                             double* dloglik, double* du, double* drho, double* dscale, double* dscores) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(wsemi_check(ctx, dX, G, n, m, ldx, dy, dW, prefixes, K, penalties, P, dloglik));
  DeviceGuard g(ctx->device);
  return wsemi_dev_impl(ctx, dX, G, n, m, ldx, dy, dW, prefixes, K, penalties, P, dloglik, du, drho, dscale, dscores);
}

int elfihip_wsemi_loglik(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* y,
                         const double* W, const int64_t* prefixes, int K, const double* penalties, int P, double* loglik,
                         double* u, double* rho, double* scale, double* scores) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(wsemi_check(ctx, X, G, n, m, ldx, y, W, prefixes, K, penalties, P, loglik));
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
  ELFIHIP_TRY(wsemi_dev_impl(ctx, dX, G, n, m, m, dy, dW, prefixes, K, penalties, P, dll, u ? du : nullptr,
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
