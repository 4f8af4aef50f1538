// ELFI's time-series example models on gfx950: ARCH(1), the M/G/1 queue and the Ricker model -- draws, the serial
// recurrence of every simulation, the summaries and the distance in one pass each.
//
// Replaces, for elfi/examples/arch.py:
//     E(t2):   xi = normal((batch, n_obs + 1)); e[:, 0] = normal(batch)
//              e[:, i] = xi[:, i] * np.sqrt(0.2 + t2 * np.power(e[:, i - 1], 2))                     arch.py:127-131
//     arch:    y[:, i] = t1 * y[:, i - 1] + e[:, i],  y[:, 0] = 0,  returns y[:, 1:]                 arch.py:100-105
//     sample_mean, sample_variance (ddof 1), autocorr(lag) of the standardised series, pairwise_autocorr -- 2 + L +
//     L (L - 1) / 2 Summary nodes that each standardise the series again                             arch.py:135-208
// and for elfi/examples/mg1.py:
//     W = exponential(1 / t3), U = uniform(t1, t2), sum_w += W[i]; y[i] = U[i] + max(0, sum_w - sum_x); sum_x += y[i]
//     log_identity = np.log(y), quantiles = np.quantile(y, q, axis=1)                                 mg1.py:40-64
// and for elfi/examples/ricker.py:
//     stock = stock_prev * np.exp(log_rate - stock_prev + std * randn(batch)); stock_obs[:, ii] = poisson(scale * stock)
//     np.mean, np.var, num_zeros, chi_squared -- 2 n_obs small NumPy calls per batch                  ricker.py:11-167
// and for elfi/examples/ar1.py:
//     w = randn(batch, n_obs + 1); x[:, i] = phi * x_prev + w[:, i]  -- n_obs small NumPy calls        ar1.py:28-38
//     and the euclidean distance on the raw series
//
// All four simulators have a recurrence along the series (ARCH: a chain of dependent square roots; M/G/1: two running sums
// and a maximum; Ricker: a chain of dependent exponentials; AR(1): a chain of multiply-adds, each rounded twice), so a simulation belongs to ONE lane from its first step to
// its distance.  A workgroup is one wavefront and a tile is 64 simulations (fewer when 64 rows do not fit the LDS, and 32
// for the stochastic Ricker model, see its launch): the 64 lanes first fill the tile's draws together
// -- coalesced loads of the caller's draws, or Philox4x32-10 pairs, every lane drawing -- then each lane runs its row's
// recurrence in place in LDS, and stays with the row for the reductions: NumPy's pairwise sums (np_sum.hpp) with their
// eight independent accumulators per lane, FMA contraction off, so that series, summaries and quantiles are BIT-IDENTICAL to
// the reference's NumPy on the same draws.  LDS rows have an odd pitch: the 32 lanes of a read group touch 32 different
// 8-byte banks at every step.  What bounds the lanes in flight is LDS -- a simulation keeps its whole series there (it is
// reduced twice and, for M/G/1, sorted: lane_sort.hpp) -- so at n_obs = 100 three tiles are resident per CU; they are independent
// workgroups, and one fills its draws (ALU-bound) while another walks its recurrence (latency-bound).
//
// Draws made here are the library's counter-based stream (philox.hpp): the ARCH noise matrix (n, n_obs + 2) holds, row-major,
// the normals elfihip_randn_dev writes for (seed, stream) -- columns 0 .. n_obs are the reference's xi (column 0 drawn and
// unused, as there), column n_obs + 1 its e[:, 0]; M/G/1 takes element e of its (n, n_obs) standard exponentials as -log u,
// u the 53-bit uniform in (0, 1] of word e of `stream` (the word + 1, as normal_pair forms its u1), and element e of its
// uniforms in [0, 1) as word e of `stream + 1` (gauss.hip: uniform_pair); Ricker's (n, n_obs) normals are the normals of
// (seed, stream) again and its Poisson count e is poisson_draw(.., seed, stream + 1, e) (poisson.hpp).
#include "common.hpp"

#include <algorithm>
#include <cmath>

#include "dist_launch.hpp"
#include "dist_metrics.hpp"
#include "lane_sort.hpp"
#include "np_sum.hpp"
#include "philox.hpp"
#include "poisson.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int SERIES_THREADS = 64;                  // one wavefront: lane = simulation
constexpr size_t SERIES_LDS = 160 * 1024;
constexpr int ARCH_MAX_LAGS = ELFIHIP_ARCH_MAX_LAGS;
constexpr int ARCH_MAX_M = 2 + ARCH_MAX_LAGS + ARCH_MAX_LAGS * (ARCH_MAX_LAGS - 1) / 2;
constexpr int MG1_MAX_Q = ELFIHIP_MG1_MAX_QUANTILES;

// NumPy's sum of n terms by the lane that owns the row; rows of more than 128 terms take the recursive form
template <bool WIDE, class F>
__device__ __forceinline__ double row_sum(F f, int n) {
  if constexpr (WIDE)
    return np_pairwise(f, 0, n);
  else
    return np_pairwise_block(f, 0, n);
}

// ---- ARCH(1) --------------------------------------------------------------------------------------------------------
struct ArchArgs {
  const double* W;      // (n, ldw) noise, or NULL: drawn here
  int64_t ldw;
  uint64_t seed, stream;
  const double* t1;     // (n)
  const double* t2;     // (n)
  int64_t n;
  int n_obs, lags, m;
  int Lp, rows;         // LDS row pitch (odd), rows per tile
  double* S;            // (n, lds): MU, VAR, AC_1 .. AC_L, PW_i_j
  int64_t lds;
  double* Y;            // optional (n, ldy): the series
  int64_t ldy;
  double* D;            // optional (n): euclidean distance to obs
  double obs[ARCH_MAX_M];
};

template <bool WIDE>
__global__ __launch_bounds__(SERIES_THREADS) void arch_kernel(ArchArgs A) {
  extern __shared__ __align__(16) double tile[];
  const int tid = threadIdx.x, nobs = A.n_obs, Lw = A.n_obs + 2, Lp = A.Lp, Rt = A.rows;
  const int64_t ntiles = (A.n + Rt - 1) / Rt;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * Rt;
    const int rows = (int)((A.n - row0) < Rt ? (A.n - row0) : Rt);
    __syncthreads();
    if (A.W) {
      for (int e = tid; e < rows * Lw; e += SERIES_THREADS) {
        const int r = e / Lw, i = e - r * Lw;
        tile[r * Lp + i] = A.W[(row0 + r) * A.ldw + i];
      }
    } else {
      // elements [e0, e1) of the row-major (n, n_obs + 2) matrix; a pair that straddles the tile's end is drawn by both tiles
      const int64_t e0 = row0 * Lw, e1 = e0 + (int64_t)rows * Lw;
      for (int64_t p = e0 / 2 + tid; 2 * p < e1; p += SERIES_THREADS) {
        double z[2];
        normal_pair(A.seed, A.stream, (uint64_t)p, z[0], z[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t e = 2 * p + h;
          if (e >= e0 && e < e1) {
            const int off = (int)(e - e0), r = off / Lw, i = off - r * Lw;
            tile[r * Lp + i] = z[h];
          }
        }
      }
    }
    __syncthreads();
    double* w = tile + (size_t)(tid < rows ? tid : 0) * Lp;
    const int64_t gi = row0 + tid;
    if (tid < rows) {
      // the chain: y_i takes the place of the noise it has consumed (position i - 1 < i)
      const double a = A.t1[gi], b = A.t2[gi];
      double e = w[nobs + 1], y = 0.0;
      for (int i = 1; i <= nobs; ++i) {
        e = w[i] * sqrt(0.2 + b * (e * e));
        y = a * y + e;
        w[i - 1] = y;
      }
    }
    if (A.Y) {   // (uniform) the series leaves in whole rows, coalesced, before it is standardised in place
      __syncthreads();
      for (int e = tid; e < rows * nobs; e += SERIES_THREADS) {
        const int r = e / nobs, i = e - r * nobs;
        A.Y[(row0 + r) * A.ldy + i] = tile[r * Lp + i];
      }
      __syncthreads();
    }
    if (tid < rows) {
      const double mu = row_sum<WIDE>([&](int i) { return w[i]; }, nobs) / (double)nobs;
      const double var = row_sum<WIDE>([&](int i) { const double d = w[i] - mu; return d * d; }, nobs) / (double)(nobs - 1);
      const double sd = sqrt(var);
      for (int i = 0; i < nobs; ++i) w[i] = (w[i] - mu) / sd;
      double ac[ARCH_MAX_LAGS];
#pragma unroll
      for (int l = 1; l <= ARCH_MAX_LAGS; ++l) {
        ac[l - 1] = 0.0;
        if (l <= A.lags) ac[l - 1] = row_sum<WIDE>([&](int i) { return w[i + l] * w[i]; }, nobs - l) / (double)(nobs - l);
      }
      double* s = A.S + gi * A.lds;
      using Euclid = Op<ELFIHIP_EUCLIDEAN, false>;   // cdist's euclidean, the distance kernels' own row arithmetic
      double acc = Euclid::init();
      int k = 0;
      auto put = [&](double v) {
        s[k] = v;
        acc = Euclid::step(acc, v, A.obs[k], 1.0, 2.0);
        ++k;
      };
      put(mu);
      put(var);
#pragma unroll
      for (int l = 0; l < ARCH_MAX_LAGS; ++l)
        if (l < A.lags) put(ac[l]);
#pragma unroll
      for (int i = 0; i < ARCH_MAX_LAGS; ++i)
#pragma unroll
        for (int j = i + 1; j < ARCH_MAX_LAGS; ++j)
          if (j < A.lags) put(ac[i] * ac[j]);
      if (A.D) A.D[gi] = Euclid::finish(acc, 0.5);
    }
  }
}

// ---- AR(1) ----------------------------------------------------------------------------------------------------------
struct Ar1Args {
  const double* W;      // (n, ldw) noise, or NULL: drawn here
  int64_t ldw;
  uint64_t seed, stream;
  const double* phi;    // (n)
  int64_t n;
  int n_obs;
  int Lp, rows;         // LDS row pitch (odd), rows per tile
  double* X;            // optional (n, ldx): the series
  int64_t ldx;
  double* D;            // optional (n): euclidean distance to obs
  const double* dobs;   // (n_obs) observed series on the device, with D
};

__global__ __launch_bounds__(SERIES_THREADS) void ar1_kernel(Ar1Args A) {
  extern __shared__ __align__(16) double tile[];
  using Euclid = Op<ELFIHIP_EUCLIDEAN, false>;   // cdist's euclidean, the distance kernels' own row arithmetic
  const int tid = threadIdx.x, nobs = A.n_obs, Lw = A.n_obs + 1, Lp = A.Lp, Rt = A.rows;
  const int64_t ntiles = (A.n + Rt - 1) / Rt;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * Rt;
    const int rows = (int)((A.n - row0) < Rt ? (A.n - row0) : Rt);
    __syncthreads();
    if (A.W) {
      for (int e = tid; e < rows * Lw; e += SERIES_THREADS) {
        const int r = e / Lw, i = e - r * Lw;
        tile[r * Lp + i] = A.W[(row0 + r) * A.ldw + i];
      }
    } else {
      // elements [e0, e1) of the row-major (n, n_obs + 1) matrix; a pair that straddles the tile's end is drawn by both tiles
      const int64_t e0 = row0 * Lw, e1 = e0 + (int64_t)rows * Lw;
      for (int64_t p = e0 / 2 + tid; 2 * p < e1; p += SERIES_THREADS) {
        double z[2];
        normal_pair(A.seed, A.stream, (uint64_t)p, z[0], z[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t e = 2 * p + h;
          if (e >= e0 && e < e1) {
            const int off = (int)(e - e0), r = off / Lw, i = off - r * Lw;
            tile[r * Lp + i] = z[h];
          }
        }
      }
    }
    __syncthreads();
    if (tid < rows) {
      // the chain: x_i takes the place of the noise before the one it has consumed (position i - 1 < i)
      double* w = tile + (size_t)tid * Lp;
      const double phi = A.phi[row0 + tid];
      double x = 0.0;
      for (int i = 1; i <= nobs; ++i) {
        x = phi * x + w[i];
        w[i - 1] = x;
      }
    }
    __syncthreads();
    if (A.X)     // (uniform) the series leaves in whole rows, coalesced
      for (int e = tid; e < rows * nobs; e += SERIES_THREADS) {
        const int r = e / nobs, i = e - r * nobs;
        A.X[(row0 + r) * A.ldx + i] = tile[r * Lp + i];
      }
    if (!A.D) continue;   // (uniform)
    // summed as elfihip_dist_rows sums a row of that length: left to right by the lane of the simulation, or, from
    // kMaxTileM + 1 values on, by the whole wavefront with lane-strided partial sums and its butterfly (as gnk.hip)
    if (nobs <= kMaxTileM) {
      if (tid < rows) {
        double acc = Euclid::init();
        for (int j = 0; j < nobs; ++j) acc = Euclid::step(acc, tile[tid * Lp + j], A.dobs[j], 1.0, 2.0);
        A.D[row0 + tid] = Euclid::finish(acc, 0.5);
      }
    } else {
      for (int r = 0; r < rows; ++r) {
        double acc = Euclid::init();
        for (int j = tid; j < nobs; j += SERIES_THREADS) acc = Euclid::step(acc, tile[r * Lp + j], A.dobs[j], 1.0, 2.0);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc = Euclid::combine(acc, __shfl_xor(acc, off, 64));
        if (tid == 0) A.D[row0 + r] = Euclid::finish(acc, 0.5);
      }
    }
  }
}

// ---- M/G/1 ----------------------------------------------------------------------------------------------------------
struct Mg1Args {
  const double* E;      // (n, lde) standard exponentials, or NULL: both drawn here
  const double* V;      // (n, ldv) uniforms in [0, 1)
  int64_t lde, ldv;
  uint64_t seed, stream;
  const double* t1;
  const double* t2;
  const double* t3;
  int64_t n;
  int n_obs, nq;
  int Lp, rows;
  double* logY;         // (n, ldl)
  double* Q;            // (n, ldq)
  double* Y;            // optional (n, ldy)
  double* Eo;           // optional (n, ldeo): the draws used
  double* Vo;           // optional (n, ldvo)
  double* D;            // optional (n)
  int64_t ldl, ldq, ldy, ldeo, ldvo;
  int weighted;
  int lo[MG1_MAX_Q], hi[MG1_MAX_Q];
  double t[MG1_MAX_Q], obs[MG1_MAX_Q], w[MG1_MAX_Q];
};

__global__ __launch_bounds__(SERIES_THREADS) void mg1_kernel(Mg1Args A) {
  extern __shared__ __align__(16) double tile[];
  const int tid = threadIdx.x, nobs = A.n_obs, Lp = A.Lp, Rt = A.rows;
  double* te = tile;                        // exponentials, then the series, then the sorted series
  double* tv = tile + (size_t)Rt * Lp;      // uniforms
  const int64_t ntiles = (A.n + Rt - 1) / Rt;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * Rt;
    const int rows = (int)((A.n - row0) < Rt ? (A.n - row0) : Rt);
    __syncthreads();
    if (A.E) {
      for (int e = tid; e < rows * nobs; e += SERIES_THREADS) {
        const int r = e / nobs, i = e - r * nobs;
        const double ex = A.E[(row0 + r) * A.lde + i], un = A.V[(row0 + r) * A.ldv + i];
        te[r * Lp + i] = ex;
        tv[r * Lp + i] = un;
        if (A.Eo) A.Eo[(row0 + r) * A.ldeo + i] = ex;
        if (A.Vo) A.Vo[(row0 + r) * A.ldvo + i] = un;
      }
    } else {
      const int64_t e0 = row0 * nobs, e1 = e0 + (int64_t)rows * nobs;
      for (int64_t p = e0 / 2 + tid; 2 * p < e1; p += SERIES_THREADS) {
        uint64_t we[2], wv[2];
        words53(A.seed, A.stream, (uint64_t)p, we[0], we[1]);
        words53(A.seed, A.stream + 1, (uint64_t)p, wv[0], wv[1]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int64_t e = 2 * p + h;
          if (e >= e0 && e < e1) {
            const int off = (int)(e - e0), r = off / nobs, i = off - r * nobs;
            const double ex = unit_exponential(we[h]), un = unit_co(wv[h]);
            te[r * Lp + i] = ex;
            tv[r * Lp + i] = un;
            if (A.Eo) A.Eo[(row0 + r) * A.ldeo + i] = ex;
            if (A.Vo) A.Vo[(row0 + r) * A.ldvo + i] = un;
          }
        }
      }
    }
    __syncthreads();
    double* y = te + (size_t)(tid < rows ? tid : 0) * Lp;
    const double* v = tv + (size_t)(tid < rows ? tid : 0) * Lp;
    const int64_t gi = row0 + tid;
    bool has_nan = false;
    if (tid < rows) {
      const double a = A.t1[gi], beta = 1.0 / A.t3[gi], span = A.t2[gi] - a;
      double sum_w = 0.0, sum_x = 0.0;
      for (int i = 0; i < nobs; ++i) {
        const double wi = beta * y[i], ui = a + span * v[i];
        sum_w = sum_w + wi;
        const double d = sum_w - sum_x;
        const double yi = ui + (d > 0.0 ? d : (d != d ? d : 0.0));   // np.maximum(0, d): a NaN stays
        sum_x = sum_x + yi;
        y[i] = yi;
        has_nan |= yi != yi;
      }
    }
    __syncthreads();
    // the series and its logarithm leave in whole rows, every lane taking logarithms
    for (int e = tid; e < rows * nobs; e += SERIES_THREADS) {
      const int r = e / nobs, i = e - r * nobs;
      const double yi = te[r * Lp + i];
      A.logY[(row0 + r) * A.ldl + i] = log(yi);
      if (A.Y) A.Y[(row0 + r) * A.ldy + i] = yi;
    }
    __syncthreads();
    if (tid < rows) {
      // sorted in place (lane_sort.hpp): the sorted values are what np.quantile's partition leaves at the positions it reads;
      // the plain comparison, a row with a NaN is overwritten below
      shell_sort(y, nobs, [](double a, double b) { return a > b; });
      double* q = A.Q + gi * A.ldq;
      double acc = 0.0;   // (Op<ELFIHIP_EUCLIDEAN, W>::init())
      for (int k = 0; k < A.nq; ++k) {
        // np.quantile's _lerp: a + (b - a) t, and b - (b - a) (1 - t) where t >= 0.5; a row with a NaN is NaN throughout
        const double lo = y[A.lo[k]], hi = y[A.hi[k]], diff = hi - lo, tk = A.t[k];
        double val = tk >= 0.5 ? hi - diff * (1.0 - tk) : lo + diff * tk;
        if (has_nan) val = __builtin_nan("");
        q[k] = val;
        // cdist's (weighted) euclidean, the distance kernels' own row arithmetic: s += w (d d)
        acc = A.weighted ? Op<ELFIHIP_EUCLIDEAN, true>::step(acc, val, A.obs[k], A.w[k], 2.0)
                         : Op<ELFIHIP_EUCLIDEAN, false>::step(acc, val, A.obs[k], 1.0, 2.0);
      }
      if (A.D) A.D[gi] = Op<ELFIHIP_EUCLIDEAN, false>::finish(acc, 0.5);
    }
  }
}

// ---- Ricker ---------------------------------------------------------------------------------------------------------
// The stock recurrence s_i = s_{i-1} exp((log_rate - s_{i-1}) + sd z_i) is serial, one lane per simulation as in ARCH; the
// stock takes the place of the normal it has consumed.  The Poisson observation of step i does not feed step i + 1, so
// it is made AFTER the recurrence, element by element over the tile's rows, as the normals were drawn: all 64 lanes draw
// whatever the number of rows in the tile, stock and counts leave in whole rows, and neighbouring lanes hold neighbouring
// steps of one simulation (the same scale, stocks of one trajectory) -- which the sampler's branches (poisson.hpp) turn
// out to care little about: 4 % between that order and unrelated simulations side by side.  The counts
// replace the stock in LDS and the lane of the row reduces them.
struct RickerArgs {
  const double* Z;      // (n, ldz) normals, or NULL: drawn here
  int64_t ldz;
  uint64_t seed, stream;
  const double* t1;     // (n) log_rate
  const double* t2;     // (n) sd, NULL with t3: the deterministic form
  const double* t3;     // (n) scale
  double stock_init;
  int64_t n;
  int n_obs;
  int Lp, rows;         // LDS row pitch (odd), rows per tile
  double* S;            // (n, lds): Mean, Var, #0
  double* Y;            // optional (n, ldy): counts (deterministic form: the stock)
  double* St;           // optional (n, ldst): the latent stock
  double* Zo;           // optional (n, ldzo): the normals used
  double* D;            // optional (n)
  int64_t lds, ldy, ldst, ldzo;
  int which;
  double obs[3];
};

template <bool WIDE>
__global__ __launch_bounds__(SERIES_THREADS) void ricker_kernel(RickerArgs A) {
  extern __shared__ __align__(16) double tile[];
  const int tid = threadIdx.x, nobs = A.n_obs, Lp = A.Lp, Rt = A.rows;
  const bool stochastic = A.t2 != nullptr;
  double* sc = tile + (size_t)Rt * Lp;      // the tile's scales, for the element pass
  const int64_t ntiles = (A.n + Rt - 1) / Rt;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * Rt;
    const int rows = (int)((A.n - row0) < Rt ? (A.n - row0) : Rt);
    __syncthreads();
    if (stochastic) {
      if (A.Z) {
        for (int e = tid; e < rows * nobs; e += SERIES_THREADS) {
          const int r = e / nobs, i = e - r * nobs;
          const double z = A.Z[(row0 + r) * A.ldz + i];
          tile[r * Lp + i] = z;
          if (A.Zo) A.Zo[(row0 + r) * A.ldzo + i] = z;
        }
      } else {
        // elements [e0, e1) of the row-major (n, n_obs) matrix; a pair that straddles the tile's end is drawn by both tiles
        const int64_t e0 = row0 * nobs, e1 = e0 + (int64_t)rows * nobs;
        for (int64_t p = e0 / 2 + tid; 2 * p < e1; p += SERIES_THREADS) {
          double z[2];
          normal_pair(A.seed, A.stream, (uint64_t)p, z[0], z[1]);
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int64_t e = 2 * p + h;
            if (e >= e0 && e < e1) {
              const int off = (int)(e - e0), r = off / nobs, i = off - r * nobs;
              tile[r * Lp + i] = z[h];
              if (A.Zo) A.Zo[(row0 + r) * A.ldzo + i] = z[h];
            }
          }
        }
      }
      if (tid < rows) sc[tid] = A.t3[row0 + tid];
      __syncthreads();
    }
    double* w = tile + (size_t)(tid < rows ? tid : 0) * Lp;
    const int64_t gi = row0 + tid;
    if (tid < rows) {
      const double a = A.t1[gi];
      double s = A.stock_init;
      if (stochastic) {
        const double b = A.t2[gi];
        for (int i = 0; i < nobs; ++i) {
          s = s * exp((a - s) + b * w[i]);
          w[i] = s;
        }
      } else {
        w[0] = s;
        for (int i = 1; i < nobs; ++i) {
          s = s * exp((a - s));
          w[i] = s;
        }
      }
    }
    if (stochastic || A.Y || A.St) {   // (uniform) the element pass: stock out, the Poisson draw, counts out, whole rows
      __syncthreads();
      for (int e = tid; e < rows * nobs; e += SERIES_THREADS) {
        const int r = e / nobs, i = e - r * nobs;
        double v = tile[r * Lp + i];
        if (A.St) A.St[(row0 + r) * A.ldst + i] = v;
        if (stochastic) {
          v = poisson_draw(sc[r] * v, A.seed, A.stream + 1, (uint64_t)((row0 + r) * nobs + i));
          tile[r * Lp + i] = v;
        }
        if (A.Y) A.Y[(row0 + r) * A.ldy + i] = v;
      }
      __syncthreads();
    }
    if (tid < rows) {
      const double mean = row_sum<WIDE>([&](int i) { return w[i]; }, nobs) / (double)nobs;
      const double var = row_sum<WIDE>([&](int i) { const double d = w[i] - mean; return d * d; }, nobs) / (double)nobs;
      int zeros = 0;
      for (int i = 0; i < nobs; ++i) zeros += w[i] == 0.0;
      double* s = A.S + gi * A.lds;
      const double nz = (double)zeros;
      s[0] = mean;
      s[1] = var;
      s[2] = nz;
      if (A.D) {
        if (A.which == ELFIHIP_RICKER_CHI2) {
          const double d0 = mean - A.obs[0], d1 = var - A.obs[1], d2 = nz - A.obs[2];
          A.D[gi] = (((d0 * d0) / A.obs[0]) + ((d1 * d1) / A.obs[1])) + ((d2 * d2) / A.obs[2]);
        } else {
          using Euclid = Op<ELFIHIP_EUCLIDEAN, false>;
          A.D[gi] = Euclid::finish(Euclid::step(Euclid::init(), mean, A.obs[0], 1.0, 2.0), 0.5);
        }
      }
    }
  }
}

// ---- launches ---------------------------------------------------------------------------------------------------------
// rows per tile: one per lane, fewer only where 64 rows of `row_bytes` exceed the LDS; 0: not even one row fits
static int tile_rows(size_t row_bytes) {
  const size_t fit = SERIES_LDS / row_bytes;
  return (int)std::min<size_t>(fit, SERIES_THREADS);
}

static unsigned series_grid(const elfihip_ctx* ctx, int64_t n, int rows, size_t lds) {
  const int64_t ntiles = (n + rows - 1) / rows;
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(16, (int64_t)(SERIES_LDS / lds)));
  return (unsigned)std::min<int64_t>(ntiles, (int64_t)ctx->cu_count * per_cu);
}

static int arch_dev_impl(elfihip_ctx* ctx, const double* dW, int64_t ldw, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                         int n_lags, const double* dt1, const double* dt2, const double* obs, double* dS, int64_t lds,
                         double* dY, int64_t ldy, double* dD) {
  ELFIHIP_REQUIRE(ctx, n_lags >= 1 && n_lags <= ARCH_MAX_LAGS, "n_lags %d outside [1, %d]", n_lags, ARCH_MAX_LAGS);
  ELFIHIP_REQUIRE(ctx, n >= 0 && n_obs >= n_lags + 2, "bad shape n=%lld n_obs=%d (at least n_lags + 2 = %d)", (long long)n,
                  n_obs, n_lags + 2);
  ELFIHIP_REQUIRE(ctx, n_obs <= ELFIHIP_SERIES_MAX_OBS, "series of %d observations: at most %d", n_obs, ELFIHIP_SERIES_MAX_OBS);
  const int m = 2 + n_lags + n_lags * (n_lags - 1) / 2;
  ELFIHIP_REQUIRE(ctx, (!dW || ldw >= n_obs + 2) && lds >= m && (!dY || ldy >= n_obs), "leading dimension below the row length");
  ELFIHIP_REQUIRE(ctx, !dD || obs, "a distance needs the observed summaries");
  ELFIHIP_REQUIRE(ctx, n == 0 || (dt1 && dt2 && dS), "NULL data pointer");
  if (n == 0) return ELFIHIP_OK;
  ArchArgs A;
  A.W = dW;
  A.ldw = ldw;
  A.seed = seed;
  A.stream = stream;
  A.t1 = dt1;
  A.t2 = dt2;
  A.n = n;
  A.n_obs = n_obs;
  A.lags = n_lags;
  A.m = m;
  A.Lp = (n_obs + 2) | 1;
  A.S = dS;
  A.lds = lds;
  A.Y = dY;
  A.ldy = ldy;
  A.D = dD;
  for (int j = 0; j < ARCH_MAX_M; ++j) A.obs[j] = (obs && j < m) ? obs[j] : 0.0;
  const size_t row_bytes = (size_t)A.Lp * sizeof(double);
  A.rows = tile_rows(row_bytes);
  ELFIHIP_REQUIRE(ctx, A.rows >= 1, "series of %d observations do not fit the LDS tile", n_obs);
  const size_t bytes = (size_t)A.rows * row_bytes;
  const unsigned grid = series_grid(ctx, n, A.rows, bytes);
  if (n_obs > 128) {
    ELFIHIP_TRY(set_lds(ctx, arch_kernel<true>, bytes));
    hipLaunchKernelGGL(arch_kernel<true>, dim3(grid), dim3(SERIES_THREADS), bytes, ctx->stream, A);
  } else {
    ELFIHIP_TRY(set_lds(ctx, arch_kernel<false>, bytes));
    hipLaunchKernelGGL(arch_kernel<false>, dim3(grid), dim3(SERIES_THREADS), bytes, ctx->stream, A);
  }
  return launch_status(ctx, "arch_kernel");
}

static int ar1_dev_impl(elfihip_ctx* ctx, const double* dW, int64_t ldw, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                        const double* dphi, const double* obs, double* dX, int64_t ldx, double* dD) {
  ELFIHIP_REQUIRE(ctx, n >= 0 && n_obs >= 1, "bad shape n=%lld n_obs=%d (at least 1)", (long long)n, n_obs);
  ELFIHIP_REQUIRE(ctx, n_obs <= ELFIHIP_SERIES_MAX_OBS, "series of %d observations: at most %d", n_obs, ELFIHIP_SERIES_MAX_OBS);
  ELFIHIP_REQUIRE(ctx, (!dW || ldw >= n_obs + 1) && (!dX || ldx >= n_obs), "leading dimension below the row length");
  ELFIHIP_REQUIRE(ctx, !dD || obs, "a distance needs the observed series");
  ELFIHIP_REQUIRE(ctx, n == 0 || dphi, "NULL data pointer");
  if (n == 0) return ELFIHIP_OK;
  Ar1Args A;
  A.W = dW;
  A.ldw = ldw;
  A.seed = seed;
  A.stream = stream;
  A.phi = dphi;
  A.n = n;
  A.n_obs = n_obs;
  A.Lp = (n_obs + 1) | 1;
  A.X = dX;
  A.ldx = ldx;
  A.D = dD;
  A.dobs = nullptr;
  if (dD) {   // the observed series goes to the device on the stream
    ELFIHIP_CHECK_HIP(ctx, ctx->par.reserve((size_t)n_obs * sizeof(double)));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(ctx->par.p, obs, (size_t)n_obs * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    A.dobs = ctx->par.as<double>();
  }
  const size_t row_bytes = (size_t)A.Lp * sizeof(double);
  A.rows = tile_rows(row_bytes);
  ELFIHIP_REQUIRE(ctx, A.rows >= 1, "series of %d observations do not fit the LDS tile", n_obs);
  const size_t bytes = (size_t)A.rows * row_bytes;
  const unsigned grid = series_grid(ctx, n, A.rows, bytes);
  ELFIHIP_TRY(set_lds(ctx, ar1_kernel, bytes));
  hipLaunchKernelGGL(ar1_kernel, dim3(grid), dim3(SERIES_THREADS), bytes, ctx->stream, A);
  return launch_status(ctx, "ar1_kernel");
}

static int mg1_dev_impl(elfihip_ctx* ctx, const double* dE, int64_t lde, const double* dV, int64_t ldv, uint64_t seed,
                        uint64_t stream, int64_t n, int n_obs, const double* dt1, const double* dt2, const double* dt3, int nq,
                        const int* lo, const int* hi, const double* t, const double* obs, const double* w, double* dLogY,
                        int64_t ldl, double* dQ, int64_t ldq, double* dY, int64_t ldy, double* dEo, int64_t ldeo, double* dVo,
                        int64_t ldvo, double* dD) {
  ELFIHIP_REQUIRE(ctx, n >= 0 && n_obs >= 2, "bad shape n=%lld n_obs=%d (at least 2)", (long long)n, n_obs);
  ELFIHIP_REQUIRE(ctx, n_obs <= ELFIHIP_SERIES_MAX_OBS, "series of %d observations: at most %d", n_obs, ELFIHIP_SERIES_MAX_OBS);
  ELFIHIP_REQUIRE(ctx, nq >= 1 && nq <= MG1_MAX_Q && lo && hi && t, "1 to %d quantile positions", MG1_MAX_Q);
  ELFIHIP_REQUIRE(ctx, (dE == nullptr) == (dV == nullptr), "exponentials and uniforms are given together or not at all");
  ELFIHIP_REQUIRE(ctx, (!dE || (lde >= n_obs && ldv >= n_obs)) && ldl >= n_obs && ldq >= nq && (!dY || ldy >= n_obs) &&
                           (!dEo || ldeo >= n_obs) && (!dVo || ldvo >= n_obs),
                  "leading dimension below the row length");
  ELFIHIP_REQUIRE(ctx, !dD || obs, "a distance needs the observed quantiles");
  ELFIHIP_REQUIRE(ctx, !w || obs, "weights without observed quantiles");
  for (int k = 0; k < nq; ++k)
    ELFIHIP_REQUIRE(ctx, lo[k] >= 0 && lo[k] < n_obs && hi[k] >= 0 && hi[k] < n_obs, "quantile position %d outside the series", k);
  ELFIHIP_REQUIRE(ctx, n == 0 || (dt1 && dt2 && dt3 && dLogY && dQ), "NULL data pointer");
  if (n == 0) return ELFIHIP_OK;
  Mg1Args A;
  A.E = dE;
  A.V = dV;
  A.lde = lde;
  A.ldv = ldv;
  A.seed = seed;
  A.stream = stream;
  A.t1 = dt1;
  A.t2 = dt2;
  A.t3 = dt3;
  A.n = n;
  A.n_obs = n_obs;
  A.nq = nq;
  A.Lp = n_obs | 1;
  A.logY = dLogY;
  A.Q = dQ;
  A.Y = dY;
  A.Eo = dEo;
  A.Vo = dVo;
  A.D = dD;
  A.ldl = ldl;
  A.ldq = ldq;
  A.ldy = ldy;
  A.ldeo = ldeo;
  A.ldvo = ldvo;
  A.weighted = w != nullptr;
  for (int k = 0; k < MG1_MAX_Q; ++k) {
    const bool in = k < nq;
    A.lo[k] = in ? lo[k] : 0;
    A.hi[k] = in ? hi[k] : 0;
    A.t[k] = in ? t[k] : 0.0;
    A.obs[k] = (in && obs) ? obs[k] : 0.0;
    A.w[k] = (in && w) ? w[k] : 1.0;
  }
  const size_t row_bytes = 2 * (size_t)A.Lp * sizeof(double);   // exponentials and uniforms
  A.rows = tile_rows(row_bytes);
  ELFIHIP_REQUIRE(ctx, A.rows >= 1, "series of %d observations do not fit the LDS tile", n_obs);
  const size_t bytes = (size_t)A.rows * row_bytes;
  const unsigned grid = series_grid(ctx, n, A.rows, bytes);
  ELFIHIP_TRY(set_lds(ctx, mg1_kernel, bytes));
  hipLaunchKernelGGL(mg1_kernel, dim3(grid), dim3(SERIES_THREADS), bytes, ctx->stream, A);
  return launch_status(ctx, "mg1_kernel");
}

static int ricker_dev_impl(elfihip_ctx* ctx, const double* dZ, int64_t ldz, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                           const double* dt1, const double* dt2, const double* dt3, double stock_init, const double* obs,
                           int which, double* dS, int64_t lds, double* dY, int64_t ldy, double* dSt, int64_t ldst, double* dZo,
                           int64_t ldzo, double* dD) {
  ELFIHIP_REQUIRE(ctx, n >= 1 && n_obs >= 1, "bad shape n=%lld n_obs=%d (at least 1 each)", (long long)n, n_obs);
  ELFIHIP_REQUIRE(ctx, n_obs <= ELFIHIP_SERIES_MAX_OBS, "series of %d observations: at most %d", n_obs, ELFIHIP_SERIES_MAX_OBS);
  ELFIHIP_REQUIRE(ctx, (dt2 == nullptr) == (dt3 == nullptr), "std and scale are given together or not at all");
  ELFIHIP_REQUIRE(ctx, dt2 || (!dZ && !dZo), "the deterministic form takes and returns no normals");
  ELFIHIP_REQUIRE(ctx, which == ELFIHIP_RICKER_CHI2 || which == ELFIHIP_RICKER_EUCLID_MEAN, "unknown distance %d", which);
  ELFIHIP_REQUIRE(ctx, (!dZ || ldz >= n_obs) && lds >= 3 && (!dY || ldy >= n_obs) && (!dSt || ldst >= n_obs) &&
                           (!dZo || ldzo >= n_obs),
                  "leading dimension below the row length");
  ELFIHIP_REQUIRE(ctx, !dD || obs, "a distance needs the observed summaries");
  ELFIHIP_REQUIRE(ctx, dt1 && dS, "NULL data pointer");
  RickerArgs A;
  A.Z = dZ;
  A.ldz = ldz;
  A.seed = seed;
  A.stream = stream;
  A.t1 = dt1;
  A.t2 = dt2;
  A.t3 = dt3;
  A.stock_init = stock_init;
  A.n = n;
  A.n_obs = n_obs;
  A.Lp = n_obs | 1;
  A.S = dS;
  A.Y = dY;
  A.St = dSt;
  A.Zo = dZo;
  A.D = dD;
  A.lds = lds;
  A.ldy = ldy;
  A.ldst = ldst;
  A.ldzo = ldzo;
  A.which = which;
  for (int j = 0; j < 3; ++j) A.obs[j] = obs ? obs[j] : 0.0;
  const size_t row_bytes = ((size_t)A.Lp + 1) * sizeof(double);   // the series and the row's scale
  // the stochastic form spends its time in the Poisson pass, which wants wavefronts more than full ones: at 238 VGPRs a CU
  // runs eight, and eight 64-row tiles of a short series do not fit its LDS, eight 32-row tiles do (n_obs 50, batch 10^6:
  // 3.68 -> 2.82 ms; the recurrence then runs with half its lanes, which the deterministic form would only lose by)
  A.rows = dt2 ? std::min(tile_rows(row_bytes), 32) : tile_rows(row_bytes);
  ELFIHIP_REQUIRE(ctx, A.rows >= 1, "series of %d observations do not fit the LDS tile", n_obs);
  const size_t bytes = (size_t)A.rows * row_bytes;
  const unsigned grid = series_grid(ctx, n, A.rows, bytes);
  if (n_obs > 128) {
    ELFIHIP_TRY(set_lds(ctx, ricker_kernel<true>, bytes));
    hipLaunchKernelGGL(ricker_kernel<true>, dim3(grid), dim3(SERIES_THREADS), bytes, ctx->stream, A);
  } else {
    ELFIHIP_TRY(set_lds(ctx, ricker_kernel<false>, bytes));
    hipLaunchKernelGGL(ricker_kernel<false>, dim3(grid), dim3(SERIES_THREADS), bytes, ctx->stream, A);
  }
  return launch_status(ctx, "ricker_kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_arch_summaries_dev(elfihip_ctx* ctx, const double* dW, int64_t ldw, uint64_t seed, uint64_t stream, int64_t n,
                               int n_obs, int n_lags, const double* dt1, const double* dt2, const double* obs, double* dS,
                               int64_t lds, double* dY, int64_t ldy, double* dD) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return arch_dev_impl(ctx, dW, ldw, seed, stream, n, n_obs, n_lags, dt1, dt2, obs, dS, lds, dY, ldy, dD);
}

int elfihip_arch_summaries(elfihip_ctx* ctx, const double* W, uint64_t seed, uint64_t stream, int64_t n, int n_obs, int n_lags,
                           const double* t1, const double* t2, const double* obs, double* S, double* Y, double* D) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n_lags >= 1 && n_lags <= ARCH_MAX_LAGS, "n_lags %d outside [1, %d]", n_lags, ARCH_MAX_LAGS);
  ELFIHIP_REQUIRE(ctx, n >= 0 && n_obs >= n_lags + 2 && n_obs <= ELFIHIP_SERIES_MAX_OBS, "bad shape n=%lld n_obs=%d",
                  (long long)n, n_obs);
  ELFIHIP_REQUIRE(ctx, n == 0 || (t1 && t2 && S), "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, !D || obs, "a distance needs the observed summaries");
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const int L = n_obs + 2, m = 2 + n_lags + n_lags * (n_lags - 1) / 2;
  const size_t nw = W ? (size_t)n * L : 0, ny = Y ? (size_t)n * n_obs : 0, ns = (size_t)n * m;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((nw + 2 * (size_t)n) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((ns + (size_t)n + ny) * sizeof(double)));
  double* dW = ctx->in.as<double>();
  double* dt1 = dW + nw;
  double* dt2 = dt1 + n;
  double* dS = ctx->out.as<double>();
  double* dD = dS + ns;
  double* dY = dD + n;
  if (W) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dW, W, nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dt1, t1, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dt2, t2, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(arch_dev_impl(ctx, W ? dW : nullptr, L, seed, stream, n, n_obs, n_lags, dt1, dt2, obs, dS, m, Y ? dY : nullptr,
                            n_obs, D ? dD : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(S, dS, ns * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (D) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(D, dD, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (Y) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Y, dY, ny * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_ar1_series_dev(elfihip_ctx* ctx, const double* dW, int64_t ldw, uint64_t seed, uint64_t stream, int64_t n,
                           int n_obs, const double* dphi, const double* obs, double* dX, int64_t ldx, double* dD) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return ar1_dev_impl(ctx, dW, ldw, seed, stream, n, n_obs, dphi, obs, dX, ldx, dD);
}

int elfihip_ar1_series(elfihip_ctx* ctx, const double* W, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                       const double* phi, const double* obs, double* X, double* D) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 0 && n_obs >= 1 && n_obs <= ELFIHIP_SERIES_MAX_OBS, "bad shape n=%lld n_obs=%d", (long long)n, n_obs);
  ELFIHIP_REQUIRE(ctx, n == 0 || phi, "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, !D || obs, "a distance needs the observed series");
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const int L = n_obs + 1;
  const size_t nw = W ? (size_t)n * L : 0, nx = X ? (size_t)n * n_obs : 0;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((nw + (size_t)n) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(((size_t)n + nx) * sizeof(double)));
  double* dW = ctx->in.as<double>();
  double* dphi = dW + nw;
  double* dD = ctx->out.as<double>();
  double* dX = dD + n;
  if (W) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dW, W, nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dphi, phi, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(ar1_dev_impl(ctx, W ? dW : nullptr, L, seed, stream, n, n_obs, dphi, obs, X ? dX : nullptr, n_obs, D ? dD : nullptr));
  if (X) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(X, dX, nx * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (D) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(D, dD, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_mg1_summaries_dev(elfihip_ctx* ctx, const double* dE, int64_t lde, const double* dV, int64_t ldv, uint64_t seed,
                              uint64_t stream, int64_t n, int n_obs, const double* dt1, const double* dt2, const double* dt3,
                              int nq, const int* lo, const int* hi, const double* t, const double* obs, const double* w,
                              double* dLogY, int64_t ldl, double* dQ, int64_t ldq, double* dY, int64_t ldy, double* dEo,
                              int64_t ldeo, double* dVo, int64_t ldvo, double* dD) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return mg1_dev_impl(ctx, dE, lde, dV, ldv, seed, stream, n, n_obs, dt1, dt2, dt3, nq, lo, hi, t, obs, w, dLogY, ldl, dQ, ldq,
                      dY, ldy, dEo, ldeo, dVo, ldvo, dD);
}

int elfihip_mg1_summaries(elfihip_ctx* ctx, const double* E, const double* V, uint64_t seed, uint64_t stream, int64_t n,
                          int n_obs, const double* t1, const double* t2, const double* t3, int nq, const int* lo, const int* hi,
                          const double* t, const double* obs, const double* w, double* logY, double* Q, double* Y, double* Eo,
                          double* Vo, double* D) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 0 && n_obs >= 2 && n_obs <= ELFIHIP_SERIES_MAX_OBS, "bad shape n=%lld n_obs=%d", (long long)n, n_obs);
  ELFIHIP_REQUIRE(ctx, nq >= 1 && nq <= MG1_MAX_Q, "1 to %d quantile positions", MG1_MAX_Q);
  ELFIHIP_REQUIRE(ctx, (E == nullptr) == (V == nullptr), "exponentials and uniforms are given together or not at all");
  ELFIHIP_REQUIRE(ctx, n == 0 || (t1 && t2 && t3 && logY && Q), "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, !D || obs, "a distance needs the observed quantiles");
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const size_t nn = (size_t)n * n_obs, nd = E ? nn : 0, nqn = (size_t)n * nq;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((2 * nd + 3 * (size_t)n) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((nn + nqn + (size_t)n + (Y ? nn : 0) + (Eo ? nn : 0) + (Vo ? nn : 0)) * sizeof(double)));
  double* dE = ctx->in.as<double>();
  double* dV = dE + nd;
  double* dt1 = dV + nd;
  double* dt2 = dt1 + n;
  double* dt3 = dt2 + n;
  double* dL = ctx->out.as<double>();
  double* dQ = dL + nn;
  double* dD = dQ + nqn;
  double* dY = dD + n;
  double* dEo = dY + (Y ? nn : 0);
  double* dVo = dEo + (Eo ? nn : 0);
  if (E) {
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dE, E, nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dV, V, nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dt1, t1, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dt2, t2, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dt3, t3, (size_t)n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(mg1_dev_impl(ctx, E ? dE : nullptr, n_obs, E ? dV : nullptr, n_obs, seed, stream, n, n_obs, dt1, dt2, dt3, nq, lo,
                           hi, t, obs, w, dL, n_obs, dQ, nq, Y ? dY : nullptr, n_obs, Eo ? dEo : nullptr, n_obs,
                           Vo ? dVo : nullptr, n_obs, D ? dD : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(logY, dL, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Q, dQ, nqn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (D) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(D, dD, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (Y) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Y, dY, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (Eo) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Eo, dEo, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (Vo) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Vo, dVo, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_ricker_summaries_dev(elfihip_ctx* ctx, const double* dZ, int64_t ldz, uint64_t seed, uint64_t stream, int64_t n,
                                 int n_obs, const double* dlog_rate, const double* dsd, const double* dscale,
                                 double stock_init, const double* obs, int which, double* dS, int64_t lds, double* dY,
                                 int64_t ldy, double* dSt, int64_t ldst, double* dZo, int64_t ldzo, double* dD) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return ricker_dev_impl(ctx, dZ, ldz, seed, stream, n, n_obs, dlog_rate, dsd, dscale, stock_init, obs, which, dS, lds, dY, ldy,
                         dSt, ldst, dZo, ldzo, dD);
}

int elfihip_ricker_summaries(elfihip_ctx* ctx, const double* Z, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                             const double* log_rate, const double* sd, const double* scale, double stock_init,
                             const double* obs, int which, double* S, double* Y, double* St, double* Zo, double* D) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 1 && n_obs >= 1 && n_obs <= ELFIHIP_SERIES_MAX_OBS, "bad shape n=%lld n_obs=%d", (long long)n, n_obs);
  ELFIHIP_REQUIRE(ctx, (sd == nullptr) == (scale == nullptr), "std and scale are given together or not at all");
  ELFIHIP_REQUIRE(ctx, sd || (!Z && !Zo), "the deterministic form takes and returns no normals");
  ELFIHIP_REQUIRE(ctx, log_rate && S, "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, !D || obs, "a distance needs the observed summaries");
  DeviceGuard g(ctx->device);
  const size_t nn = (size_t)n * n_obs, nz = Z ? nn : 0, np_ = sd ? 3 * (size_t)n : (size_t)n;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((nz + np_) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((4 * (size_t)n + (Y ? nn : 0) + (St ? nn : 0) + (Zo ? nn : 0)) * sizeof(double)));
  double* dZ = ctx->in.as<double>();
  double* dt1 = dZ + nz;
  double* dt2 = dt1 + n;
  double* dt3 = dt2 + n;
  double* dS = ctx->out.as<double>();
  double* dD = dS + 3 * (size_t)n;
  double* dY = dD + n;
  double* dSt = dY + (Y ? nn : 0);
  double* dZo = dSt + (St ? nn : 0);
  const size_t pb = (size_t)n * sizeof(double);
  if (Z) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dZ, Z, nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dt1, log_rate, pb, hipMemcpyHostToDevice, ctx->stream));
  if (sd) {
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dt2, sd, pb, hipMemcpyHostToDevice, ctx->stream));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dt3, scale, pb, hipMemcpyHostToDevice, ctx->stream));
  }
  ELFIHIP_TRY(ricker_dev_impl(ctx, Z ? dZ : nullptr, n_obs, seed, stream, n, n_obs, dt1, sd ? dt2 : nullptr, sd ? dt3 : nullptr,
                              stock_init, obs, which, dS, 3, Y ? dY : nullptr, n_obs, St ? dSt : nullptr, n_obs,
                              Zo ? dZo : nullptr, n_obs, D ? dD : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(S, dS, 3 * pb, hipMemcpyDeviceToHost, ctx->stream));
  if (D) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(D, dD, pb, hipMemcpyDeviceToHost, ctx->stream));
  if (Y) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Y, dY, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (St) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(St, dSt, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (Zo) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Zo, dZo, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
