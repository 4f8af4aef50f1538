// ELFI's stochastic Lorenz-96 forecast model on gfx950 -- draws, the Runge-Kutta recurrence of every simulation, the six
// summaries and the distance in one pass.
//
// Replaces, for elfi/examples/lorenz.py:
//     forecast_lorenz:  per step i = 1 .. T - 1   e = normal(0, 1, (batch, K));  eta = phi * eta + e * sqrt(1 - phi^2)
//                       y = runge_kutta_ode_solver(_lorenz_ode, total_duration / T, y, (eta, theta1, theta2, f))   lorenz.py:94-163
//     _lorenz_ode:      dy_k = -y[k-2] y[k-1] + y[k-1] y[k+1] - y[k] + f - (theta1 + y[k] theta2) + eta[k], cyclic    lorenz.py:18-55
//     mean, var, autocov, cov, xcov(prev), xcov(next) -- six Summary nodes that walk the (batch, T, K) series eleven
//     times                                                                                                        lorenz.py:231-320
//
// The recurrence runs along time and couples neighbouring variables, so a simulation belongs to ONE wavefront (a workgroup
// is one wavefront) and lane k owns variable k: eta, y, the Runge-Kutta stages and the three time-sequential column sums
// stay in registers, the neighbours k - 2, k - 1, k + 1 come by cross-lane reads, and every finished row leaves as one
// coalesced store (to the caller's Y when asked for) and into the simulation's (T, K) image in LDS.  The arithmetic is
// + - * / by constants only, FMA contraction off, in the reference's operation order: the series is the reference's BIT FOR
// BIT on the same draws.  So are the summaries, given NumPy's reduction orders:
//     column sums along time (np.mean / np.var over axis 1 of a (batch, T, K) array) are plain left-to-right sums -- one
//     lane per column;
//     np.mean over the flattened (T, K) or (T - 1, K) terms is NumPy's pairwise sum (np_sum.hpp): the split tree's leaves
//     (at most 128 terms, at most 65 leaves for the 8192 terms of NumPy's reduction buffer) are summed one per lane with the
//     eight interleaved accumulators, and combined in the tree's order;
//     np.mean over the K column values is one such leaf.
// The centred products need the column means first, so the series is read twice: it stays in LDS -- T K doubles, 51 KB for
// the example's 160 x 40, three wavefronts per CU.  No atomics; no result depends on the grid.
//
// Draws made here are the library's counter-based stream (philox.hpp): element e of the row-major (n, T - 1, K) array is
// normal number e of (seed, stream), what elfihip_randn_dev writes.
#include "common.hpp"

#include <algorithm>

#include "dist_metrics.hpp"
#include "philox.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int LZ_THREADS = 64;                 // one wavefront: lane = variable
constexpr int LZ_MAX_VARS = ELFIHIP_LORENZ_MAX_VARS;
constexpr int LZ_MAX_TERMS = ELFIHIP_LORENZ_MAX_TERMS;
constexpr int LZ_LEAF = 128;                   // NumPy's PW_BLOCKSIZE
constexpr int LZ_MAX_LEAVES = 65;              // of the split tree of any n <= 8192 (its depth is at most 7)
constexpr int LZ_TAB = 68;                     // leaf table: LZ_MAX_LEAVES entries, entry 66 the leaf count
constexpr int LZ_DEPTH = 8;
constexpr size_t LZ_LDS_PER_CU = 160 * 1024;
constexpr size_t LZ_LDS_GRANULE = 1280;

struct LorenzArgs {
  const double* E;      // (n, ldE): the (T - 1, K) draws of a simulation, or NULL: drawn here
  int64_t ldE;
  uint64_t seed, stream;
  const double* t1;     // (n)
  const double* t2;     // (n)
  const double* y0;     // (K), or (n, ldy0)
  int64_t ldy0;         // 0: one shared row
  int64_t n;
  int K, T;
  double f, c, phi, h;
  double* S;            // (n, lds): Mean, Var, Autocov, Cov, CrosscovPrev, CrosscovNext
  int64_t lds;
  double* Y;            // optional (n, ldy): the (T, K) series
  int64_t ldy;
  double* D;            // optional (n): euclidean distance to obs
  double obs[6];
};

// One leaf of NumPy's pairwise sum, NV sums at once: next(t) yields the NV terms of the following element (the leaf's
// elements are asked for in order).  Fewer than 8 terms in order; else eight interleaved accumulators, the tail in order.
template <int NV, class F>
__device__ __forceinline__ void leaf_sum(F& next, int n, double (&res)[NV]) {
  double t[NV];
  if (n < 8) {
#pragma unroll
    for (int v = 0; v < NV; ++v) res[v] = 0.0;
    for (int i = 0; i < n; ++i) {
      next(t);
#pragma unroll
      for (int v = 0; v < NV; ++v) res[v] += t[v];
    }
    return;
  }
  double r[8][NV];
#pragma unroll
  for (int j = 0; j < 8; ++j) next(r[j]);
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      next(t);
#pragma unroll
      for (int v = 0; v < NV; ++v) r[j][v] += t[v];
    }
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) res[v] = ((r[0][v] + r[1][v]) + (r[2][v] + r[3][v])) + ((r[4][v] + r[5][v]) + (r[6][v] + r[7][v]));
  for (; i < n; ++i) {
    next(t);
#pragma unroll
    for (int v = 0; v < NV; ++v) res[v] += t[v];
  }
}

// The split tree of NumPy's pairwise sum of n terms (more than 128: split at n / 2 rounded down to a multiple of 8), as
// the list of its leaves from left to right: offset | length << 13 | merges << 21, where `merges` is the number of
// inner nodes complete once that leaf is -- a leaf that ends the right subtree of a node completes it, and whatever that
// node ends in turn.  One lane; `stk` is scratch for at most LZ_DEPTH pending right subtrees.
__device__ void leaf_table(int n, uint32_t* tab, int* stk) {
  int sp = 0, nleaf = 0;
  stk[0] = 0;
  stk[1] = n;
  stk[2] = 0;
  sp = 1;
  while (sp > 0) {
    --sp;
    int lo = stk[3 * sp], len = stk[3 * sp + 1], r = stk[3 * sp + 2];
    while (len > LZ_LEAF) {
      int n2 = len / 2;
      n2 -= n2 % 8;
      stk[3 * sp] = lo + n2;
      stk[3 * sp + 1] = len - n2;
      stk[3 * sp + 2] = r + 1;
      ++sp;
      len = n2;
      r = 0;
    }
    if (nleaf < LZ_MAX_LEAVES) tab[nleaf] = (uint32_t)lo | ((uint32_t)len << 13) | ((uint32_t)r << 21);
    ++nleaf;
  }
  tab[LZ_TAB - 2] = (uint32_t)nleaf;
}

// Combines the leaves' sums in the tree's order.  val[r][v]: sum v of leaf (lane + 64 r), one leaf per lane; every lane
// runs the same stack machine on values read across the wavefront and ends with the same totals.
template <int NV>
__device__ __forceinline__ void combine_leaves(const uint32_t* tab, const double (&val)[2][NV], double (&out)[NV]) {
  const int nleaf = (int)tab[LZ_TAB - 2];
  double st[LZ_DEPTH][NV];
#pragma unroll
  for (int d = 0; d < LZ_DEPTH; ++d)
#pragma unroll
    for (int v = 0; v < NV; ++v) st[d][v] = 0.0;
  for (int l = 0; l < nleaf; ++l) {
#pragma unroll
    for (int d = LZ_DEPTH - 1; d > 0; --d)
#pragma unroll
      for (int v = 0; v < NV; ++v) st[d][v] = st[d - 1][v];
#pragma unroll
    for (int v = 0; v < NV; ++v) st[0][v] = __shfl(l < LZ_THREADS ? val[0][v] : val[1][v], l & (LZ_THREADS - 1));
    const int merges = (int)(tab[l] >> 21);
    for (int m = 0; m < merges; ++m) {
#pragma unroll
      for (int v = 0; v < NV; ++v) st[0][v] = st[1][v] + st[0][v];
#pragma unroll
      for (int d = 1; d < LZ_DEPTH - 1; ++d)
#pragma unroll
        for (int v = 0; v < NV; ++v) st[d][v] = st[d + 1][v];
    }
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) out[v] = st[0][v];
}

__global__ __launch_bounds__(LZ_THREADS) void lorenz_kernel(LorenzArgs A) {
  extern __shared__ __align__(16) double lz_lds[];
  const int lane = threadIdx.x, K = A.K, T = A.T;
  const int N = T * K, N1 = (T - 1) * K;
  double* x = lz_lds;                 // (T, K): the series of the simulation at hand
  double* am = x + N;                 // (K): mean over t < T - 1
  double* bm = am + LZ_MAX_VARS;      // (K): mean over t >= 1
  uint32_t* tabN = reinterpret_cast<uint32_t*>(bm + LZ_MAX_VARS);   // leaves of the sum over T K terms
  uint32_t* tabN1 = tabN + LZ_TAB;                                   // ... over (T - 1) K terms
  if (lane == 0) {
    leaf_table(N, tabN, reinterpret_cast<int*>(x));
    leaf_table(N1, tabN1, reinterpret_cast<int*>(x));
  }
  __syncthreads();
  // lanes beyond K shadow variable lane mod K (their values are never stored): every cross-lane read finds a live value
  const int k = lane % K;
  const bool own = lane < K;
  const int km1 = k == 0 ? K - 1 : k - 1, km2 = km1 == 0 ? K - 1 : km1 - 1, kp1 = k + 1 == K ? 0 : k + 1;
  const double f = A.f, c = A.c, phi = A.phi, h = A.h;
  for (int64_t s = blockIdx.x; s < A.n; s += gridDim.x) {
    const double th1 = A.t1[s], th2 = A.t2[s];
    double y = A.y0[s * A.ldy0 + k];
    const double* e_row = A.E ? A.E + s * A.ldE : nullptr;
    const int64_t e_base = s * (int64_t)N1;      // the drawn form: element e_base + (i - 1) K + k of the stream
    double* y_row = A.Y ? A.Y + s * A.ldy : nullptr;
    __syncthreads();                             // the previous simulation's LDS image is done with
    if (own) {
      x[k] = y;
      if (y_row) y_row[k] = y;
    }
    double eta = 0.0, sm = y, sa = y, sb = 0.0;  // column sums over all t, t < T - 1, t >= 1
    double e_next = e_row ? e_row[k] : 0.0;
    for (int i = 1; i < T; ++i) {
      double e;
      if (e_row) {
        e = e_next;
        if (i + 1 < T) e_next = e_row[(int64_t)i * K + k];
      } else {
        const uint64_t el = (uint64_t)(e_base + (int64_t)(i - 1) * K + k);
        double z0, z1;
        normal_pair(A.seed, A.stream, el >> 1, z0, z1);
        e = (el & 1) ? z1 : z0;
      }
      eta = phi * eta + e * c;
      auto ode = [&](double u) {
        const double um1 = __shfl(u, km1), um2 = __shfl(u, km2), up1 = __shfl(u, kp1);
        const double g = th1 + u * th2;
        return ((((-um2 * um1 + um1 * up1) - u) + f) - g) + eta;
      };
      const double k1 = h * ode(y);
      const double k2 = h * ode(y + k1 / 2);
      const double k3 = h * ode(y + k2 / 2);
      const double k4 = h * ode(y + k3);
      y = y + (((k1 + 2 * k2) + 2 * k3) + k4) / 6;
      sm += y;
      if (i < T - 1) sa += y;
      sb += y;
      if (own) {
        x[i * K + k] = y;
        if (y_row) y_row[(int64_t)i * K + k] = y;
      }
    }
    const double m = sm / (double)T, a = sa / (double)(T - 1), b = sb / (double)(T - 1);
    if (own) {
      am[k] = a;
      bm[k] = b;
    }
    __syncthreads();
    // Var and Cov: the centred squares and neighbour products summed along time by the column's lane, then over the columns
    const double mn = __shfl(m, kp1);
    double sv = 0.0, sq = 0.0;
    for (int t = 0; t < T; ++t) {
      const double d = x[t * K + k] - m, dn = x[t * K + kp1] - mn;
      sv += d * d;
      sq += d * dn;
    }
    sv = sv / (double)T;
    sq = sq / (double)T;
    double vc[2];
    {
      int i = 0;
      auto next = [&](double (&t)[2]) {
        t[0] = __shfl(sv, i);
        t[1] = __shfl(sq, i);
        ++i;
      };
      leaf_sum<2>(next, K, vc);
    }
    // Mean: the pairwise sum over the T K values, a leaf per lane
    double mv[2][1] = {{0.0}, {0.0}};
    {
      const int nleaf = (int)tabN[LZ_TAB - 2];
      for (int l = lane, r = 0; l < nleaf; l += LZ_THREADS, ++r) {
        const uint32_t e = tabN[l];
        const double* p = x + (e & 8191u);
        auto next = [&](double (&t)[1]) { t[0] = *p++; };
        double res[1];
        leaf_sum<1>(next, (int)((e >> 13) & 255u), res);
        if (r == 0)
          mv[0][0] = res[0];
        else
          mv[1][0] = res[0];
      }
    }
    double mean[1];
    combine_leaves<1>(tabN, mv, mean);
    // Autocov, CrosscovPrev, CrosscovNext: pairwise sums over the (T - 1) K products (x[t, k] - a_k) (x[t + 1, k'] - b_k'),
    // k' = k, k - 1, k + 1
    double lv[2][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    {
      const int nleaf = (int)tabN1[LZ_TAB - 2];
      for (int l = lane, r = 0; l < nleaf; l += LZ_THREADS, ++r) {
        const uint32_t e = tabN1[l];
        int idx = (int)(e & 8191u), kk = idx % K;
        auto next = [&](double (&t)[3]) {
          const int kp = kk + 1 == K ? 0 : kk + 1, km = kk == 0 ? K - 1 : kk - 1;
          const double xa = x[idx] - am[kk];
          const double* nx = x + (idx - kk + K);      // row t + 1
          t[0] = xa * (nx[kk] - bm[kk]);
          t[1] = xa * (nx[km] - bm[km]);
          t[2] = xa * (nx[kp] - bm[kp]);
          ++idx;
          kk = kp;
        };
        double res[3];
        leaf_sum<3>(next, (int)((e >> 13) & 255u), res);
#pragma unroll
        for (int v = 0; v < 3; ++v) {
          if (r == 0)
            lv[0][v] = res[v];
          else
            lv[1][v] = res[v];
        }
      }
    }
    double lag[3];
    combine_leaves<3>(tabN1, lv, lag);
    if (lane == 0) {
      const double out[6] = {mean[0] / (double)N,   vc[0] / (double)K,   lag[0] / (double)N1,
                             vc[1] / (double)K,     lag[1] / (double)N1, lag[2] / (double)N1};
      double* sr = A.S + s * A.lds;
      using Euclid = Op<ELFIHIP_EUCLIDEAN, false>;   // cdist's euclidean, the distance kernels' own row arithmetic
      double acc = Euclid::init();
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        sr[j] = out[j];
        acc = Euclid::step(acc, out[j], A.obs[j], 1.0, 2.0);
      }
      if (A.D) A.D[s] = Euclid::finish(acc, 0.5);
    }
  }
}

static size_t lorenz_lds_bytes(int K, int T) {
  return ((size_t)T * K + 2 * LZ_MAX_VARS) * sizeof(double) + 2 * LZ_TAB * sizeof(uint32_t);
}

static int lorenz_dev_impl(elfihip_ctx* ctx, const double* dE, int64_t ldE, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                           int n_timestep, const double* dt1, const double* dt2, double f, double c, double phi, double h,
                           const double* dy0, int64_t ldy0, const double* obs, double* dS, int64_t lds, double* dY, int64_t ldy,
                           double* dD) {
  ELFIHIP_REQUIRE(ctx, n >= 0, "bad batch n=%lld", (long long)n);
  ELFIHIP_REQUIRE(ctx, n_obs >= 4 && n_obs <= LZ_MAX_VARS, "n_obs %d outside [4, %d]", n_obs, LZ_MAX_VARS);
  ELFIHIP_REQUIRE(ctx, n_timestep >= 2, "n_timestep %d: at least 2", n_timestep);
  ELFIHIP_REQUIRE(ctx, (int64_t)n_timestep * n_obs <= LZ_MAX_TERMS, "n_timestep * n_obs = %lld: at most %d",
                  (long long)n_timestep * n_obs, LZ_MAX_TERMS);
  const int64_t series = (int64_t)n_timestep * n_obs, draws = series - n_obs;
  ELFIHIP_REQUIRE(ctx, (!dE || ldE >= draws) && lds >= 6 && (!dY || ldy >= series) && (ldy0 == 0 || ldy0 >= n_obs),
                  "leading dimension below the row length");
  ELFIHIP_REQUIRE(ctx, !dD || obs, "a distance needs the observed summaries");
  ELFIHIP_REQUIRE(ctx, n == 0 || (dt1 && dt2 && dy0 && dS), "NULL data pointer");
  if (n == 0) return ELFIHIP_OK;
  LorenzArgs A;
  A.E = dE;
  A.ldE = ldE;
  A.seed = seed;
  A.stream = stream;
  A.t1 = dt1;
  A.t2 = dt2;
  A.y0 = dy0;
  A.ldy0 = ldy0;
  A.n = n;
  A.K = n_obs;
  A.T = n_timestep;
  A.f = f;
  A.c = c;
  A.phi = phi;
  A.h = h;
  A.S = dS;
  A.lds = lds;
  A.Y = dY;
  A.ldy = ldy;
  A.D = dD;
  for (int j = 0; j < 6; ++j) A.obs[j] = obs ? obs[j] : 0.0;
  const size_t bytes = lorenz_lds_bytes(n_obs, n_timestep);
  const size_t held = (bytes + LZ_LDS_GRANULE - 1) / LZ_LDS_GRANULE * LZ_LDS_GRANULE;
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(16, (int64_t)(LZ_LDS_PER_CU / held)));
  const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)ctx->cu_count * per_cu);
  ELFIHIP_TRY(set_lds(ctx, lorenz_kernel, bytes));
  hipLaunchKernelGGL(lorenz_kernel, dim3(grid), dim3(LZ_THREADS), bytes, ctx->stream, A);
  return launch_status(ctx, "lorenz_kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_lorenz_summaries_dev(elfihip_ctx* ctx, const double* dE, int64_t ldE, uint64_t seed, uint64_t stream, int64_t n,
                                 int n_obs, int n_timestep, const double* dt1, const double* dt2, double f, double c, double phi,
                                 double h, const double* dy0, int64_t ldy0, const double* obs, double* dS, int64_t lds,
                                 double* dY, int64_t ldy, double* dD) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return lorenz_dev_impl(ctx, dE, ldE, seed, stream, n, n_obs, n_timestep, dt1, dt2, f, c, phi, h, dy0, ldy0, obs, dS, lds, dY,
                         ldy, dD);
}

int elfihip_lorenz_summaries(elfihip_ctx* ctx, const double* E, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                             int n_timestep, const double* t1, const double* t2, double f, double c, double phi, double h,
                             const double* y0, int y0_per_simulation, const double* obs, double* S, double* Y, double* D) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 0, "bad batch n=%lld", (long long)n);
  ELFIHIP_REQUIRE(ctx, n_obs >= 4 && n_obs <= LZ_MAX_VARS, "n_obs %d outside [4, %d]", n_obs, LZ_MAX_VARS);
  ELFIHIP_REQUIRE(ctx, n_timestep >= 2, "n_timestep %d: at least 2", n_timestep);
  ELFIHIP_REQUIRE(ctx, (int64_t)n_timestep * n_obs <= LZ_MAX_TERMS, "n_timestep * n_obs = %lld: at most %d",
                  (long long)n_timestep * n_obs, LZ_MAX_TERMS);
  ELFIHIP_REQUIRE(ctx, n == 0 || (t1 && t2 && y0 && S), "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, !D || obs, "a distance needs the observed summaries");
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const size_t series = (size_t)n_timestep * n_obs, draws = series - n_obs;
  const size_t ne = E ? (size_t)n * draws : 0, ny0 = y0_per_simulation ? (size_t)n * n_obs : (size_t)n_obs;
  const size_t ns = (size_t)n * 6, ny = Y ? (size_t)n * series : 0;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((ne + 2 * (size_t)n + ny0) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((ns + (size_t)n + ny) * sizeof(double)));
  double* dE = ctx->in.as<double>();
  double* dt1 = dE + ne;
  double* dt2 = dt1 + n;
  double* dy0 = dt2 + n;
  double* dS = ctx->out.as<double>();
  double* dD = dS + ns;
  double* dY = dD + n;
  if (E) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dE, E, ne * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dt1, t1, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dt2, t2, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dy0, y0, ny0 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(lorenz_dev_impl(ctx, E ? dE : nullptr, (int64_t)draws, seed, stream, n, n_obs, n_timestep, dt1, dt2, f, c, phi, h,
                              dy0, y0_per_simulation ? n_obs : 0, obs, dS, 6, Y ? dY : nullptr, (int64_t)series,
                              D ? dD : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(S, dS, ns * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (D) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(D, dD, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (Y) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Y, dY, ny * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
