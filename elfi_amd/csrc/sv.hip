// The alpha-stable stochastic-volatility model (elfi/examples/stochastic_volatility_model.py) and its two quantile
// summaries, fused: one workgroup per simulation keeps the series and one sort buffer in LDS.
//
//   phase A  every lane takes cells t: the three draws of the cell (given, or from the generator -- include/elfihip.h has the
//            rule) and the shock v[t], the general stable transform in S0 (stable.hpp).  This is the Philox and
//            transcendental work, about ten calls per cell, and does not depend on the state.  The normal waits in the
//            cell's slot of the series, the shock in the cell's slot of the (still unused) sort buffer.
//   phase B  the AR(1) chain of log-volatilities x[t] = z[t] sigma + (mu + phi (x[t - 1] - mu)): five dependent operations
//            per step, walked through LDS by lane 0 -- a loop of n_obs trips that guards nothing; the workgroup meets it at
//            the barrier behind.
//   phase C  every lane forms y[t] = exp(x[t] / 2) v[t] and its sort key: the bits of y with the sign bit flipped for y >= 0
//            and all bits flipped below, which orders signed doubles as unsigned integers (-0 and +0 become neighbours,
//            which NumPy's _lerp does not tell apart).  A NaN makes both summaries NaN, as np.quantile does, and nothing is
//            sorted; otherwise the keys are padded to a power of two with the largest key and sorted by the workgroup
//            (wg_sort.hpp), seven lanes read np.quantile's positions (method 'linear', NumPy's _lerp, as toad.hip does) and
//            lane 0 forms (q95 - q05) / (q75 - q25) and ((q95 - q50) - (q50 - q05)) / (q95 - q05).
//
// The workgroup is one wavefront while n_obs <= 1024 -- the sort's 16 keys per lane then cover the series in one trip -- and
// 256 threads above.  LDS: 8 n_obs bytes of series + the buffer (n_obs rounded up to a power of two, and a seventeenth word
// per sixteen, 8 bytes each): 944 bytes at n_obs = 50, 16.9 KB at 1000, 66 KB at the limit 4096.
//
// Every expression keeps NumPy's operation order, FMA contraction off: on given normals x is NumPy's bit for bit, and on y
// so are the two summaries; v and y differ through the device's transcendentals.
#include "common.hpp"

#include <algorithm>

#include "stable.hpp"
#include "wg_sort.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int SV_WAVE_MAX_OBS = 1024;     // up to here one wavefront per simulation
constexpr int SV_NQ = 7;                  // four probabilities of kurt, three of skew
constexpr double SV_PHI_SQUARE_CAP = 0.99999;

struct SvArgs {
  const double* Z;      // (n, ldd) given draws, or NULL: drawn here
  const double* TH;
  const double* W;
  int64_t ldd;
  uint64_t seed, stream;
  uint32_t first;
  int64_t n;
  int n_obs;
  double q[SV_NQ];
  const double* alpha;
  const double* beta;
  const double* kappa;
  const double* eta;
  const double* mu;
  const double* phi;
  const double* sigma;
  const double* x0;     // (n) or NULL: the stationary start
  double* S;            // (n, lds) kurt, skew
  int64_t lds;
  double* Y;            // (n, ldy) returns, or NULL
  int64_t ldy;
  double* X;            // (n, ldx) log-volatilities, or NULL
  int64_t ldx;
  double* V;            // (n, ldv) shocks, or NULL
  int64_t ldv;
  double* Zo;           // (n, ldo) the draws used, or NULL (all three or none)
  double* THo;
  double* Wo;
  int64_t ldo;
};

__device__ __forceinline__ unsigned long long sv_key(double y) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(y);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double sv_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// kept out of line: inlined, the transform's registers add to the sort's and one wavefront per SIMD is left; so, two are
__device__ __noinline__ double sv_shock(double alpha, double beta, double eta, double kappa, double TH, double W) {
  return stable_general(alpha, beta, eta, kappa, true, TH, W);
}

__global__ __launch_bounds__(256) void sv_kernel(const SvArgs A) {
  extern __shared__ double sv_lds[];
  __shared__ double qv[SV_NQ];
  const int tid = threadIdx.x, T = blockDim.x;
  const int n_obs = A.n_obs, P = wg_sort_padded(n_obs);
  double* xs = sv_lds;
  unsigned long long* key = reinterpret_cast<unsigned long long*>(sv_lds + n_obs);

  for (int64_t row = blockIdx.x; row < A.n; row += gridDim.x) {
    const double alpha = A.alpha[row], beta = A.beta[row], kappa = A.kappa[row], eta = A.eta[row];
    const double mu = A.mu[row], phi = A.phi[row], sigma = A.sigma[row], x0 = A.x0 ? A.x0[row] : 0.0;
    const bool valid = stable_valid_general(alpha, beta, kappa) && sigma >= 0.0 && eta == eta && mu == mu && phi == phi && x0 == x0;
    const uint64_t g = (uint64_t)A.first + (uint64_t)row;

    // ---- phase A: draws and shocks of every cell
    for (int t = tid; t < n_obs; t += T) {
      double z, TH, W;
      if (A.Z) {
        const int64_t o = row * A.ldd + t;
        z = A.Z[o];
        TH = A.TH[o];
        W = A.W[o];
      } else {
        const uint64_t e = (g << 32) | (uint64_t)t;
        stable_angle_expo(A.seed, A.stream, e, TH, W);
        double z1;
        normal_pair(A.seed, A.stream + 1, e, z, z1);
      }
      const double v = valid ? sv_shock(alpha, beta, eta, kappa, TH, W) : __builtin_nan("");
      if (A.V) A.V[row * A.ldv + t] = v;
      if (A.Zo) {
        const int64_t o = row * A.ldo + t;
        A.Zo[o] = z;
        A.THo[o] = TH;
        A.Wo[o] = W;
      }
      xs[t] = z;
      key[wg_sort_slot(t)] = (unsigned long long)__double_as_longlong(v);
    }
    __syncthreads();

    if (!valid) {
      // an invalid parameter row: NaN throughout; the neighbours are other rows
      if (tid < 2) A.S[row * A.lds + tid] = __builtin_nan("");
      for (int t = tid; t < n_obs; t += T) {
        if (A.Y) A.Y[row * A.ldy + t] = __builtin_nan("");
        if (A.X) A.X[row * A.ldx + t] = __builtin_nan("");
      }
      __syncthreads();
      continue;
    }

    // ---- phase B: lane 0 walks the chain
    if (tid == 0) {
      double x = A.x0 ? xs[0] * sigma + (mu + phi * (x0 - mu)) : xs[0] * (sigma / sqrt(1.0 - fmin(phi * phi, SV_PHI_SQUARE_CAP))) + mu;
      xs[0] = x;
      int t = 1;
      for (; t + 4 <= n_obs; t += 4) {
        const double z0 = xs[t], z1 = xs[t + 1], z2 = xs[t + 2], z3 = xs[t + 3];
        const double a = z0 * sigma + (mu + phi * (x - mu));
        const double b = z1 * sigma + (mu + phi * (a - mu));
        const double c = z2 * sigma + (mu + phi * (b - mu));
        x = z3 * sigma + (mu + phi * (c - mu));
        xs[t] = a, xs[t + 1] = b, xs[t + 2] = c, xs[t + 3] = x;
      }
      for (; t < n_obs; ++t) {
        x = xs[t] * sigma + (mu + phi * (x - mu));
        xs[t] = x;
      }
    }
    __syncthreads();

    // ---- phase C: returns, keys, the sort and the two summaries
    int nan_here = 0;
    for (int t = tid; t < n_obs; t += T) {
      const double x = xs[t], v = __longlong_as_double((long long)key[wg_sort_slot(t)]);
      const double y = exp(0.5 * x) * v;
      if (A.X) A.X[row * A.ldx + t] = x;
      if (A.Y) A.Y[row * A.ldy + t] = y;
      nan_here |= (y != y);
      key[wg_sort_slot(t)] = sv_key(y);
    }
    for (int e = n_obs + tid; e < P; e += T) key[wg_sort_slot(e)] = ~0ull;
    const int any_nan = __syncthreads_or(nan_here);
    if (any_nan) {
      if (tid < 2) A.S[row * A.lds + tid] = __builtin_nan("");
    } else {
      wg_sort_u64(key, P, tid, T);
      if (tid < SV_NQ) {
        // np.quantile, method 'linear': virtual index (n - 1) p, its two neighbours and _lerp; at the upper end NumPy names
        // both neighbours -1 and measures the weight from that name
        const double virt = (double)(n_obs - 1) * A.q[tid];
        int lo, hi;
        double w;
        if (virt >= (double)(n_obs - 1)) {
          lo = hi = n_obs - 1;
          w = virt - (-1.0);
        } else {
          const double prev = floor(virt);
          lo = (int)prev;
          hi = lo + 1;
          w = virt - prev;
        }
        const double a = sv_unkey(key[wg_sort_slot(lo)]), b = sv_unkey(key[wg_sort_slot(hi)]), diff = b - a;
        qv[tid] = w >= 0.5 ? b - diff * (1.0 - w) : a + diff * w;
      }
      __syncthreads();
      if (tid == 0) {
        A.S[row * A.lds] = (qv[3] - qv[0]) / (qv[2] - qv[1]);
        A.S[row * A.lds + 1] = ((qv[6] - qv[5]) - (qv[5] - qv[4])) / (qv[6] - qv[4]);
      }
    }
    __syncthreads();
  }
}

static size_t sv_lds_bytes(int n_obs) {
  return ((size_t)n_obs + (size_t)std::max(1, wg_sort_words(wg_sort_padded(n_obs)))) * sizeof(double);
}

static int sv_check(elfihip_ctx* ctx, int64_t first_index, int64_t n, int n_obs, const double* q) {
  ELFIHIP_REQUIRE(ctx, n >= 1, "need at least one simulation");
  ELFIHIP_REQUIRE(ctx, first_index >= 0 && first_index <= (int64_t)0x100000000ll - n,
                  "simulation indices first_index .. first_index + n - 1 must lie in [0, 2^32)");
  ELFIHIP_REQUIRE(ctx, n_obs >= 1 && n_obs <= ELFIHIP_SV_MAX_OBS, "need 1 <= n_obs <= %d", ELFIHIP_SV_MAX_OBS);
  ELFIHIP_REQUIRE(ctx, q, "the seven quantile probabilities are needed");
  for (int k = 0; k < SV_NQ; ++k) ELFIHIP_REQUIRE(ctx, q[k] >= 0.0 && q[k] <= 1.0, "quantile probabilities must lie in [0, 1]");
  return ELFIHIP_OK;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_sv_summaries_dev(elfihip_ctx* ctx, const double* dZ, const double* dTH, const double* dW, int64_t ldd, uint64_t seed,
                             uint64_t stream, int64_t first_index, int64_t n, int n_obs, const double* q, const double* dalpha,
                             const double* dbeta, const double* dkappa, const double* deta, const double* dmu, const double* dphi,
                             const double* dsigma, const double* dx0, double* dS, int64_t lds, double* dY, int64_t ldy, double* dX,
                             int64_t ldx, double* dV, int64_t ldv, double* dZo, double* dTHo, double* dWo, int64_t ldo) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(sv_check(ctx, first_index, n, n_obs, q));
  const bool given = dZ || dTH || dW, echo = dZo || dTHo || dWo;
  ELFIHIP_REQUIRE(ctx, !given || (dZ && dTH && dW && ldd >= n_obs), "the three draw arrays are given together, at a pitch of at least n_obs");
  ELFIHIP_REQUIRE(ctx, !echo || (dZo && dTHo && dWo && ldo >= n_obs), "the three draw outputs are asked for together, at a pitch of at least n_obs");
  ELFIHIP_REQUIRE(ctx, dalpha && dbeta && dkappa && deta && dmu && dphi && dsigma && dS && lds >= 2,
                  "parameters and summaries are needed, the summaries at a pitch of at least 2");
  ELFIHIP_REQUIRE(ctx, (!dY || ldy >= n_obs) && (!dX || ldx >= n_obs) && (!dV || ldv >= n_obs), "an output pitch is shorter than its row");
  DeviceGuard g(ctx->device);
  SvArgs A;
  A.Z = dZ, A.TH = dTH, A.W = dW, A.ldd = ldd;
  A.seed = seed, A.stream = stream, A.first = (uint32_t)first_index, A.n = n, A.n_obs = n_obs;
  for (int k = 0; k < SV_NQ; ++k) A.q[k] = q[k];
  A.alpha = dalpha, A.beta = dbeta, A.kappa = dkappa, A.eta = deta, A.mu = dmu, A.phi = dphi, A.sigma = dsigma, A.x0 = dx0;
  A.S = dS, A.lds = lds, A.Y = dY, A.ldy = ldy, A.X = dX, A.ldx = ldx, A.V = dV, A.ldv = ldv;
  A.Zo = dZo, A.THo = dTHo, A.Wo = dWo, A.ldo = ldo;
  const size_t lds_bytes = sv_lds_bytes(n_obs);
  ELFIHIP_TRY(set_lds(ctx, sv_kernel, lds_bytes, 48 * 1024));
  const int threads = n_obs <= SV_WAVE_MAX_OBS ? 64 : 256;
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(threads == 64 ? 16 : 4, (size_t)(150 * 1024) / (lds_bytes + 1024)));
  const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)ctx->cu_count * per_cu);
  hipLaunchKernelGGL(sv_kernel, dim3(grid), dim3(threads), lds_bytes, ctx->stream, A);
  return launch_status(ctx, "sv_kernel");
}

int elfihip_sv_summaries(elfihip_ctx* ctx, const double* Z, const double* TH, const double* W, uint64_t seed, uint64_t stream,
                         int64_t first_index, int64_t n, int n_obs, const double* q, const double* alpha, const double* beta,
                         const double* kappa, const double* eta, const double* mu, const double* phi, const double* sigma,
                         const double* x0, double* S, double* Y, double* X, double* V, double* Zo, double* THo, double* Wo) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(sv_check(ctx, first_index, n, n_obs, q));
  const bool given = Z || TH || W, echo = Zo || THo || Wo;
  ELFIHIP_REQUIRE(ctx, !given || (Z && TH && W), "the three draw arrays are given together");
  ELFIHIP_REQUIRE(ctx, !echo || (Zo && THo && Wo), "the three draw outputs are asked for together");
  ELFIHIP_REQUIRE(ctx, alpha && beta && kappa && eta && mu && phi && sigma && S, "parameters and summaries are needed");
  DeviceGuard g(ctx->device);
  const size_t N = (size_t)n, cells = (size_t)n_obs, d8 = sizeof(double);
  // staging: parameters | given draws | outputs
  ELFIHIP_CHECK_HIP(ctx, ctx->par.reserve(8 * N * d8));
  double* dpar = ctx->par.as<double>();
  const double* hp[8] = {alpha, beta, kappa, eta, mu, phi, sigma, x0};
  for (int k = 0; k < (x0 ? 8 : 7); ++k)
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar + k * N, hp[k], N * d8, hipMemcpyHostToDevice, ctx->stream));
  double* dd[3] = {nullptr, nullptr, nullptr};
  if (given) {
    ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(3 * N * cells * d8));
    const double* hd[3] = {Z, TH, W};
    for (int k = 0; k < 3; ++k) {
      dd[k] = ctx->in.as<double>() + k * N * cells;
      ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dd[k], hd[k], N * cells * d8, hipMemcpyHostToDevice, ctx->stream));
    }
  }
  double* ho[7] = {S, Y, X, V, Zo, THo, Wo};
  double* dop[7];
  size_t width[7] = {2, cells, cells, cells, cells, cells, cells}, total = 0;
  for (int k = 0; k < 7; ++k) total += ho[k] ? N * width[k] : 0;
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(total * d8));
  double* o = ctx->out.as<double>();
  for (int k = 0; k < 7; ++k) {
    dop[k] = ho[k] ? o : nullptr;
    o += ho[k] ? N * width[k] : 0;
  }
  ELFIHIP_TRY(elfihip_sv_summaries_dev(ctx, dd[0], dd[1], dd[2], (int64_t)cells, seed, stream, first_index, n, n_obs, q, dpar,
                                       dpar + N, dpar + 2 * N, dpar + 3 * N, dpar + 4 * N, dpar + 5 * N, dpar + 6 * N,
                                       x0 ? dpar + 7 * N : nullptr, dop[0], 2, dop[1], (int64_t)cells, dop[2], (int64_t)cells,
                                       dop[3], (int64_t)cells, dop[4], dop[5], dop[6], (int64_t)cells));
  for (int k = 0; k < 7; ++k)
    if (ho[k]) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(ho[k], dop[k], N * width[k] * d8, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
