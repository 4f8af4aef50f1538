// ELFI's g-and-k example models on gfx950: the univariate (elfi/examples/gnk.py) and the bivariate one
// (elfi/examples/bignk.py) -- draws, the quantile function, the per-column sort, the octiles, the robust statistics and the
// distance in one pass.
//
// Replaces:
//     GNK:     z = ss.norm.rvs(size=(batch, n_obs))
//              y = A + B * (1 + c * ((1 - np.exp(-g * z)) / (1 + np.exp(-g * z)))) * (1 + z**2)**k * z       gnk.py:61-64
//     BiGNK:   z[i] = ss.multivariate_normal.rvs(cov=[[1, rho_i], [rho_i, 1]], size=n_obs) in a Python loop over the
//              batch, then the same quantile function per dimension                                          bignk.py:83-108
//     ss_order = np.sort(y) (the trailing axis: the series as it is), ss_octile = np.percentile(y, linspace(12.5, 87.5, 7),
//     axis=1), ss_robust from the same seven octiles, euclidean_multiss                                      gnk.py:115-248
//
// Unlike the time-series models of series.hip nothing here is a recurrence: every element of a series is one exp, one pow
// and a division away from its draw.  So the 64 lanes of the one-wavefront workgroup take ELEMENTS of the tile while the
// work is transcendental -- lane l draws (or loads, coalesced) element l, l + 64, ... of the tile's row-major block,
// evaluates the quantile function in the reference's order of operations and puts the value into its column in LDS --
// and COLUMNS only once there is something to sort: one lane owns one (simulation, dimension) column, 64 simulations per
// tile at dim = 1 and 32 at dim = 2 (fewer only where that many columns exceed the LDS), Shell-sorts it in place with NaNs
// last (lane_sort.hpp), reads the seven octiles at the host's (lo, hi, t) positions (np.percentile's linear rule, as mg1_kernel reads its
// quantiles) and forms the robust statistics from them.  Columns have the odd pitch of series.hip: the 32 lanes of a
// ds_read_b64 group touch 32 different bank pairs at every step of the sort.  FMA contraction is off: everything after the
// series is bit-identical to NumPy on the same series; the series itself goes through the device's exp and pow and is
// within a few units eps (|A| + |y - A|) of the reference's (include/elfihip.h).
//
// The draws made here are the library's counter-based stream (philox.hpp): element e of the row-major (n, n_obs, dim) array
// is normal number e of (seed, stream), as elfihip_randn_dev writes them; at dim = 2 the pair (e0, e1) of an observation
// -- one Philox counter -- becomes z0 = e0, z1 = rho e0 + sqrt(1 - rho rho) e1.
#include "common.hpp"

#include <algorithm>
#include <cmath>

#include "dist_launch.hpp"
#include "dist_metrics.hpp"
#include "lane_sort.hpp"
#include "philox.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int GNK_THREADS = 64;                 // one wavefront
constexpr size_t GNK_LDS = 160 * 1024;
constexpr int GNK_NOCT = 7;
constexpr int GNK_OBS_INLINE = 64;              // observed rows up to this length travel in the kernel arguments

struct GnkArgs {
  const double* Z;      // (n, ldz) the normals, a row = (n_obs, dim) row-major, already correlated; or NULL: drawn here
  int64_t ldz;
  uint64_t seed, stream;
  const double* P;      // (n, ldp): A, B, g, k | A1, A2, B1, B2, g1, g2, k1, k2, rho
  int64_t ldp;
  double c;
  int64_t n;
  int n_obs, dim;
  int Lp, rows;         // LDS column pitch (odd), simulations per tile
  double* Y;            // optional (n, ldy): the series, (n_obs, dim) row-major per simulation
  double* Zo;           // optional (n, ldzo): the draws used
  double* Ys;           // optional (n, ldys): every column sorted, same layout
  double* O;            // optional (n, ldo): 7 dim octiles
  double* R;            // optional (n, ldr): 4 dim robust statistics
  double* D;            // optional (n)
  int64_t ldy, ldzo, ldys, ldo, ldr;
  int which;            // the row D is taken on: ELFIHIP_GNK_ORDER / SORTED / OCTILE / ROBUST
  int sort, read;       // (uniform) the tile is sorted; the octiles are read
  const double* dobs;   // observed row on the device (rows longer than GNK_OBS_INLINE), else NULL: obs below
  int lo[GNK_NOCT], hi[GNK_NOCT];
  double t[GNK_NOCT];
  double obs[GNK_OBS_INLINE];
};

__global__ __launch_bounds__(GNK_THREADS) void gnk_kernel(GnkArgs A) {
  extern __shared__ __align__(16) double tile[];
  using Euclid = Op<ELFIHIP_EUCLIDEAN, false>;   // cdist's euclidean, the distance kernels' own row arithmetic
  const int tid = threadIdx.x, nobs = A.n_obs, dim = A.dim, sh = dim - 1, Lp = A.Lp, Rt = A.rows;
  const int Lrow = nobs * dim;                // doubles of a simulation's row in Z, Y, Zo, Ys
  double* par = tile + (size_t)Rt * dim * Lp;   // per column: A, B, g, k
  double* cor = par + (size_t)Rt * dim * 4;     // per simulation: rho, sqrt(1 - rho rho)
  auto ob = [&](int j) { return A.dobs ? A.dobs[j] : A.obs[j]; };
  // the distance of the (n_obs, dim) row-major rows in LDS to the observed row, summed as elfihip_dist_rows sums a row of
  // that length: left to right by the lane of the simulation, or, from kMaxTileM + 1 values on, by the whole wavefront
  // with lane-strided partial sums and its butterfly
  auto row_distance = [&](int64_t row0, int rows) {
    if (Lrow <= kMaxTileM) {
      if (tid < rows) {
        double acc = Euclid::init();
        for (int j = 0; j < Lrow; ++j) acc = Euclid::step(acc, tile[(tid * dim + (j & sh)) * Lp + (j >> sh)], ob(j), 1.0, 2.0);
        A.D[row0 + tid] = Euclid::finish(acc, 0.5);
      }
    } else {
      for (int r = 0; r < rows; ++r) {
        double acc = Euclid::init();
        for (int j = tid; j < Lrow; j += GNK_THREADS)
          acc = Euclid::step(acc, tile[(r * dim + (j & sh)) * Lp + (j >> sh)], A.dobs[j], 1.0, 2.0);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc = Euclid::combine(acc, __shfl_xor(acc, off, 64));
        if (tid == 0) A.D[row0 + r] = Euclid::finish(acc, 0.5);
      }
    }
  };
  const int64_t ntiles = (A.n + Rt - 1) / Rt;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * Rt;
    const int rows = (int)((A.n - row0) < Rt ? (A.n - row0) : Rt);
    const int cols = rows * dim;
    __syncthreads();
    for (int e = tid; e < cols * 4; e += GNK_THREADS) {
      const int col = e >> 2, q = e & 3;
      par[e] = A.P[(row0 + (col >> sh)) * A.ldp + q * dim + (col & sh)];
    }
    if (dim == 2 && !A.Z && tid < rows) {
      const double rho = A.P[(row0 + tid) * A.ldp + 8];
      cor[2 * tid] = rho;
      cor[2 * tid + 1] = sqrt(1.0 - rho * rho);
    }
    __syncthreads();
    // ---- fill and transform: lanes take elements ----
    // element j of simulation r, normal z: the quantile function in the reference's order, into column (r, j mod dim)
    auto put = [&](int r, int j, double z) {
      const int col = r * dim + (j & sh);
      const double* p = par + 4 * col;
      const double ex = exp(-(p[2] * z));
      const double br = 1.0 + A.c * ((1.0 - ex) / (1.0 + ex));
      const double y = p[0] + ((p[1] * br) * pow(1.0 + z * z, p[3])) * z;
      tile[col * Lp + (j >> sh)] = y;
      if (A.Y) A.Y[(row0 + r) * A.ldy + j] = y;
      if (A.Zo) A.Zo[(row0 + r) * A.ldzo + j] = z;
    };
    if (A.Z) {
      for (int e = tid; e < rows * Lrow; e += GNK_THREADS) {
        const int r = e / Lrow, j = e - r * Lrow;
        put(r, j, A.Z[(row0 + r) * A.ldz + j]);
      }
    } else {
      // elements [e0, e1) of the row-major (n, n_obs dim) matrix; a pair that straddles the tile's end is drawn by both
      // tiles.  At dim = 2 a row holds an even number of elements, so a pair is one observation of one simulation.
      const int64_t e0 = row0 * Lrow, e1 = e0 + (int64_t)rows * Lrow;
      for (int64_t p = e0 / 2 + tid; 2 * p < e1; p += GNK_THREADS) {
        double z[2];
        normal_pair(A.seed, A.stream, (uint64_t)p, z[0], z[1]);
        if (dim == 2) {
          const int r = (int)((2 * p - e0) / Lrow);
          z[1] = (cor[2 * r] * z[0]) + (cor[2 * r + 1] * z[1]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t e = 2 * p + h;
          if (e >= e0 && e < e1) {
            const int off = (int)(e - e0), r = off / Lrow;
            put(r, off - r * Lrow, z[h]);
          }
        }
      }
    }
    __syncthreads();
    if (A.D && A.which == ELFIHIP_GNK_ORDER) row_distance(row0, rows);
    if (!A.sort) continue;   // (uniform)
    __syncthreads();
    // ---- sort and read: lanes take columns ----
    double* y = tile + (size_t)(tid < cols ? tid : 0) * Lp;
    if (tid < cols) shell_sort(y, nobs, nan_last_after);   // NaNs last, as np.sort leaves them
    if (A.Ys || (A.D && A.which == ELFIHIP_GNK_SORTED)) {   // (uniform) the sorted columns leave in whole rows, coalesced
      __syncthreads();
      if (A.Ys)
        for (int e = tid; e < rows * Lrow; e += GNK_THREADS) {
          const int r = e / Lrow, j = e - r * Lrow;
          A.Ys[(row0 + r) * A.ldys + j] = tile[(r * dim + (j & sh)) * Lp + (j >> sh)];
        }
      if (A.D && A.which == ELFIHIP_GNK_SORTED) row_distance(row0, rows);
    }
    if (!A.read) continue;   // (uniform)
    const bool mine = tid < cols;
    const int64_t gi = row0 + (tid >> sh);
    const int d = tid & sh;
    double o[GNK_NOCT], rb[4];
    {
      // np.percentile's _lerp: a + (b - a) t, and b - (b - a) (1 - t) where t >= 0.5; a column with a NaN (sorted last) is
      // NaN throughout
      const bool has_nan = y[nobs - 1] != y[nobs - 1];
#pragma unroll
      for (int k = 0; k < GNK_NOCT; ++k) {
        const double lo = y[A.lo[k]], hi = y[A.hi[k]], diff = hi - lo, tk = A.t[k];
        double val = tk >= 0.5 ? hi - diff * (1.0 - tk) : lo + diff * tk;
        if (has_nan) val = __builtin_nan("");
        o[k] = val;
      }
      // ss_robust (gnk.py:216-248): E2, E4, E6 are the quartiles; an exactly zero ss_B becomes 0 + eps
      double sB = o[5] - o[1];
      if (sB == 0.0) sB = sB + 0x1.0p-52;
      rb[0] = o[3];
      rb[1] = sB;
      rb[2] = ((o[5] + o[1]) - 2.0 * o[3]) / sB;
      rb[3] = (((o[6] - o[4]) + o[2]) - o[0]) / sB;
    }
    if (mine && A.O) {
#pragma unroll
      for (int k = 0; k < GNK_NOCT; ++k) A.O[gi * A.ldo + k * dim + d] = o[k];
    }
    if (mine && A.R) {
#pragma unroll
      for (int k = 0; k < 4; ++k) A.R[gi * A.ldr + k * dim + d] = rb[k];
    }
    if (A.D && A.which >= ELFIHIP_GNK_OCTILE) {   // (uniform) the row [v_d0, v_d1, ...] lies across the simulation's lanes
      const int base = tid & ~sh;
      double acc = Euclid::init();
      if (A.which == ELFIHIP_GNK_OCTILE) {
#pragma unroll
        for (int k = 0; k < GNK_NOCT; ++k)
          for (int dd = 0; dd < dim; ++dd) acc = Euclid::step(acc, __shfl(o[k], base + dd, 64), A.obs[k * dim + dd], 1.0, 2.0);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          for (int dd = 0; dd < dim; ++dd) acc = Euclid::step(acc, __shfl(rb[k], base + dd, 64), A.obs[k * dim + dd], 1.0, 2.0);
      }
      if (mine && d == 0) A.D[gi] = Euclid::finish(acc, 0.5);
    }
  }
}

// ---- launch -------------------------------------------------------------------------------------------------------------
static int gnk_obs_length(int which, int n_obs, int dim) {
  return which == ELFIHIP_GNK_OCTILE ? GNK_NOCT * dim : (which == ELFIHIP_GNK_ROBUST ? 4 * dim : n_obs * dim);
}

static int gnk_dev_impl(elfihip_ctx* ctx, const double* dZ, int64_t ldz, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                        int dim, const double* dP, int64_t ldp, double c, const int* lo, const int* hi, const double* t,
                        const double* obs, int which, double* dY, int64_t ldy, double* dZo, int64_t ldzo, double* dYs,
                        int64_t ldys, double* dO, int64_t ldo, double* dR, int64_t ldr, double* dD) {
  ELFIHIP_REQUIRE(ctx, dim == 1 || dim == 2, "dim %d: the univariate (1) or the bivariate (2) model", dim);
  ELFIHIP_REQUIRE(ctx, n >= 0 && n_obs >= 2, "bad shape n=%lld n_obs=%d (at least 2)", (long long)n, n_obs);
  ELFIHIP_REQUIRE(ctx, (int64_t)n_obs * dim <= ELFIHIP_SERIES_MAX_OBS, "series of %d x %d values: at most %d", n_obs, dim,
                  ELFIHIP_SERIES_MAX_OBS);
  const int Lrow = n_obs * dim, np = dim == 1 ? 4 : 9;
  ELFIHIP_REQUIRE(ctx, which >= ELFIHIP_GNK_ORDER && which <= ELFIHIP_GNK_ROBUST, "unknown distance row %d", which);
  ELFIHIP_REQUIRE(ctx, (!dZ || ldz >= Lrow) && ldp >= np && (!dY || ldy >= Lrow) && (!dZo || ldzo >= Lrow) &&
                           (!dYs || ldys >= Lrow) && (!dO || ldo >= GNK_NOCT * dim) && (!dR || ldr >= 4 * dim),
                  "leading dimension below the row length");
  ELFIHIP_REQUIRE(ctx, !dD || obs, "a distance needs the observed row");
  const bool read = dO || dR || (dD && which >= ELFIHIP_GNK_OCTILE);
  ELFIHIP_REQUIRE(ctx, !read || (lo && hi && t), "octiles need their %d percentile positions", GNK_NOCT);
  if (read)
    for (int k = 0; k < GNK_NOCT; ++k)
      ELFIHIP_REQUIRE(ctx, lo[k] >= 0 && lo[k] < n_obs && hi[k] >= 0 && hi[k] < n_obs, "percentile position %d outside the series", k);
  ELFIHIP_REQUIRE(ctx, n == 0 || dP, "NULL data pointer");
  if (n == 0) return ELFIHIP_OK;
  GnkArgs A;
  A.Z = dZ;
  A.ldz = ldz;
  A.seed = seed;
  A.stream = stream;
  A.P = dP;
  A.ldp = ldp;
  A.c = c;
  A.n = n;
  A.n_obs = n_obs;
  A.dim = dim;
  A.Lp = n_obs | 1;
  A.Y = dY;
  A.Zo = dZo;
  A.Ys = dYs;
  A.O = dO;
  A.R = dR;
  A.D = dD;
  A.ldy = ldy;
  A.ldzo = ldzo;
  A.ldys = ldys;
  A.ldo = ldo;
  A.ldr = ldr;
  A.which = which;
  A.read = read;
  A.sort = read || dYs || (dD && which == ELFIHIP_GNK_SORTED);
  A.dobs = nullptr;
  const int mobs = dD ? gnk_obs_length(which, n_obs, dim) : 0;
  for (int k = 0; k < GNK_NOCT; ++k) {
    A.lo[k] = read ? lo[k] : 0;
    A.hi[k] = read ? hi[k] : 0;
    A.t[k] = read ? t[k] : 0.0;
  }
  for (int j = 0; j < GNK_OBS_INLINE; ++j) A.obs[j] = (mobs <= GNK_OBS_INLINE && j < mobs) ? obs[j] : 0.0;
  if (mobs > GNK_OBS_INLINE) {   // a long observed row (the series itself) goes to the device on the stream
    ELFIHIP_CHECK_HIP(ctx, ctx->par.reserve((size_t)mobs * sizeof(double)));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(ctx->par.p, obs, (size_t)mobs * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    A.dobs = ctx->par.as<double>();
  }
  // simulations per tile: a lane per column, fewer only where that many columns exceed the LDS (series.hip: tile_rows)
  const size_t row_bytes = ((size_t)dim * (A.Lp + 4) + 2) * sizeof(double);
  A.rows = (int)std::min<size_t>(GNK_LDS / row_bytes, GNK_THREADS / dim);
  ELFIHIP_REQUIRE(ctx, A.rows >= 1, "series of %d observations do not fit the LDS tile", n_obs);
  // ... and halved while no more than four tiles -- one wavefront per SIMD, nothing to hide a wait behind -- would be
  // resident on a CU, down to 16 columns: the element phase deals elements, not columns, to the lanes and stays 64 wide;
  // the sort has half its lanes idle in twice the wavefronts, which costs where the SIMDs were busy already (measured on
  // both sides: DESIGN.md)
  while (A.rows * dim > 16 && GNK_LDS / ((size_t)A.rows * row_bytes) < 5) A.rows = (A.rows + 1) / 2;
  const size_t bytes = (size_t)A.rows * row_bytes;
  const int64_t ntiles = (n + A.rows - 1) / A.rows;
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(16, (int64_t)(GNK_LDS / bytes)));
  const unsigned grid = (unsigned)std::min<int64_t>(ntiles, (int64_t)ctx->cu_count * per_cu);
  ELFIHIP_TRY(set_lds(ctx, gnk_kernel, bytes));
  hipLaunchKernelGGL(gnk_kernel, dim3(grid), dim3(GNK_THREADS), bytes, ctx->stream, A);
  return launch_status(ctx, "gnk_kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_gnk_summaries_dev(elfihip_ctx* ctx, const double* dZ, int64_t ldz, uint64_t seed, uint64_t stream, int64_t n,
                              int n_obs, int dim, const double* dP, int64_t ldp, double c, const int* lo, const int* hi,
                              const double* t, const double* obs, int which, double* dY, int64_t ldy, double* dZo,
                              int64_t ldzo, double* dYs, int64_t ldys, double* dO, int64_t ldo, double* dR, int64_t ldr,
                              double* dD) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return gnk_dev_impl(ctx, dZ, ldz, seed, stream, n, n_obs, dim, dP, ldp, c, lo, hi, t, obs, which, dY, ldy, dZo, ldzo, dYs,
                      ldys, dO, ldo, dR, ldr, dD);
}

int elfihip_gnk_summaries(elfihip_ctx* ctx, const double* Z, uint64_t seed, uint64_t stream, int64_t n, int n_obs, int dim,
                          const double* P, double c, const int* lo, const int* hi, const double* t, const double* obs,
                          int which, double* Y, double* Zo, double* Ys, double* O, double* R, double* D) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, dim == 1 || dim == 2, "dim %d: the univariate (1) or the bivariate (2) model", dim);
  ELFIHIP_REQUIRE(ctx, n >= 0 && n_obs >= 2 && (int64_t)n_obs * dim <= ELFIHIP_SERIES_MAX_OBS, "bad shape n=%lld n_obs=%d",
                  (long long)n, n_obs);
  ELFIHIP_REQUIRE(ctx, n == 0 || P, "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, !D || obs, "a distance needs the observed row");
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const int np = dim == 1 ? 4 : 9, mo = GNK_NOCT * dim, mr = 4 * dim;
  const size_t nn = (size_t)n * n_obs * dim, nz = Z ? nn : 0;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((nz + (size_t)n * np) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(((Y ? nn : 0) + (Zo ? nn : 0) + (Ys ? nn : 0) + (size_t)n * (mo + mr + 1)) * sizeof(double)));
  double* dZ = ctx->in.as<double>();
  double* dP = dZ + nz;
  double* dO = ctx->out.as<double>();
  double* dR = dO + (size_t)n * mo;
  double* dD = dR + (size_t)n * mr;
  double* dY = dD + n;
  double* dZo = dY + (Y ? nn : 0);
  double* dYs = dZo + (Zo ? nn : 0);
  if (Z) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dZ, Z, nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dP, P, (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(gnk_dev_impl(ctx, Z ? dZ : nullptr, (int64_t)n_obs * dim, seed, stream, n, n_obs, dim, dP, np, c, lo, hi, t, obs,
                           which, Y ? dY : nullptr, (int64_t)n_obs * dim, Zo ? dZo : nullptr, (int64_t)n_obs * dim,
                           Ys ? dYs : nullptr, (int64_t)n_obs * dim, O ? dO : nullptr, mo, R ? dR : nullptr, mr,
                           D ? dD : nullptr));
  if (O) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(O, dO, (size_t)n * mo * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (R) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(R, dR, (size_t)n * mr * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (D) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(D, dD, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (Y) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Y, dY, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (Zo) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Zo, dZo, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (Ys) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Ys, dYs, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
