// ELFI's stochastic Lotka-Volterra example on gfx950: an exact event-driven (Gillespie, direct method) simulator whose work
// per simulation is not known in advance, the observation of its trajectory at n_obs evenly spaced times, the nine summaries
// and the distance.
//
// Replaces, for elfi/examples/lotka_volterra.py:
//     while any(times < time_end): hazards, 1 / sum, exponential, cumsum, uniform, stoichiometry   -- about 20 NumPy calls
//         per EVENT of the slowest simulation of the batch, the whole batch in lock-step             lotka_volterra.py:85-120
//     np.where / np.unique per observation time, linear interpolation, int32 store                lotka_volterra.py:125-138
//     stock_mean, stock_log_variance, stock_autocorr (lag 1, 2), stock_crosscorr, euclidean        lotka_volterra.py:226-277
//
// lv_sim_kernel: one lane per simulation, persistent wavefronts.  The number of events of a simulation under the model's
// priors has a median near 180 and a 99 % point near 50 000, so 64 simulations dealt to 64 lanes once would leave the
// wavefront waiting for its slowest lane at a few percent occupancy.  Instead a lane whose simulation ends writes its
// marks and takes the NEXT simulation index from a counter in device memory: per wavefront the finished lanes are
// balloted, one lane adds their number to the counter with one vector atomic and every finished lane takes base + its rank
// among them.  A lane that draws an index >= n retires; the wavefront leaves when all 64 have.  No wavefront waits for
// another, every loop is bounded (events by max_events, observations by n_obs, refills by the counter), and which lane ran
// a simulation when does not enter its result: the draws of event k of simulation i are Philox counter (i << 32) | k.
// The state of a simulation is three rates, two stocks, the time and two counters; nothing of the trajectory is kept --
// observation i is emitted by the first event at or past its time, from that event and the state before it, straight to
// device memory (a few hundred bytes per simulation against thousands of events of arithmetic).  The launch -- a persistent
// grid sized by the instance's occupancy, the counter zeroed -- is event_sim.hpp's, the draws are philox.hpp's.
// lv_summary_kernel: one lane per simulation over the observations written, NumPy's pairwise sums (np_sum.hpp), FMA
// contraction off: bit-identical to the reference's summary functions except for the device's log in the two log-variance
// columns.  The two are separate launches because their shapes differ: the simulation is latency-bound, wants every
// wavefront a SIMD can hold and has no use for the summaries' registers (eight accumulators per sum).
//
// The statement of the model is in include/elfihip.h (elfihip_lv_summaries) and, in NumPy, in tests/lv_ref.py.
#include "common.hpp"

#include <algorithm>
#include <cmath>

#include "dist_metrics.hpp"
#include "event_sim.hpp"
#include "np_sum.hpp"
#include "philox.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int LV_THREADS = SIM_THREADS;
constexpr int LV_SUMMARIES = ELFIHIP_LV_SUMMARIES;
constexpr double LV_INT_LIMIT = 2147483648.0;

struct LvArgs {
  const double* E;      // (n, lde) unit exponentials, or NULL with U: drawn here
  const double* U;      // (n, ldu) uniforms in [0, 1)
  const double* Z;      // (n, ldz) normals of the observation noise, or NULL: drawn here (if sigma)
  int64_t lde, ldu, ldz;
  uint64_t seed, stream, first;
  const double *r1, *r2, *r3, *prey, *pred, *sigma;   // (n) each; sigma NULL: no noise
  int64_t n;
  int n_obs, max_events;
  double time_end, step;
  double* Y;            // (n, ldy): n_obs pairs (prey, predator)
  int64_t ldy;
  double* T;            // optional (n): the time of the last event
  int* status;          // optional (n)
  long long* events;    // optional (n)
  unsigned long long* counter;   // the next simulation index, zero at launch
};

// what an int32 slot keeps of v: truncated toward zero, -0 as +0; NaN where the cast is undefined
__device__ __forceinline__ double lv_store(double v) { return fabs(v) < LV_INT_LIMIT ? trunc(v) + 0.0 : NAN; }

template <bool DRAWN, bool NOISE>
__global__ __launch_bounds__(LV_THREADS) void lv_sim_kernel(LvArgs A) {
  const int lane = threadIdx.x, n_obs = A.n_obs;
  const double time_end = A.time_end;
  bool active = false, retired = false;
  int64_t idx = 0;
  double r1 = 0.0, r2 = 0.0, r3 = 0.0, sg = 0.0, x = 0.0, y = 0.0, t = 0.0;
  int k = 0, io = 1;     // events made, the next observation to emit
  double* yrow = A.Y;
  for (;;) {
    // ---- refill: every idle lane takes the next simulation index ----
    const bool idle = !active && !retired;
    const unsigned long long need = __ballot(idle);
    if (need) {
      const int leader = __ffsll((long long)need) - 1;
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(A.counter, (unsigned long long)__popcll(need));
      const unsigned lo = __shfl((unsigned)base, leader), hi = __shfl((unsigned)(base >> 32), leader);
      base = ((unsigned long long)hi << 32) | lo;
      if (idle) {
        const unsigned long long i = base + (unsigned long long)__popcll(need & ((1ull << lane) - 1ull));
        if (i >= (unsigned long long)A.n) {
          retired = true;
        } else {
          idx = (int64_t)i;
          r1 = A.r1[idx];
          r2 = A.r2[idx];
          r3 = A.r3[idx];
          sg = NOISE ? A.sigma[idx] : 0.0;
          x = floor(A.prey[idx]);
          y = floor(A.pred[idx]);
          t = 0.0;
          k = 0;
          io = 1;
          yrow = A.Y + idx * A.ldy;
          const bool valid = rate_ok(r1) && rate_ok(r2) && rate_ok(r3) && rate_ok(sg) && x >= 0.0 &&
                             x < LV_INT_LIMIT && y >= 0.0 && y < LV_INT_LIMIT;
          if (valid) {
            yrow[0] = x;
            yrow[1] = y;
            active = true;
          } else {            // status 3: the whole row is NaN, the lane stays idle
            for (int j = 0; j < 2 * n_obs; ++j) yrow[j] = NAN;
            if (A.T) A.T[idx] = NAN;
            if (A.status) A.status[idx] = ELFIHIP_LV_INVALID;
            if (A.events) A.events[idx] = 0;
          }
        }
      }
    }
    if (__ballot(active) == 0ull) {
      if (need == 0ull) break;     // nobody runs, nobody asked: all 64 lanes have retired
      continue;                    // the lanes that asked retired or met invalid rows: ask again
    }
    // ---- one event of every running lane ----
    if (active) {
      ++k;
      double e, u;
      if constexpr (DRAWN) {
        uint64_t a, b;
        words53(A.seed, A.stream, (uint32_t)k, (uint32_t)(A.first + (uint64_t)idx), a, b);   // counter (i << 32) | k
        e = unit_exponential(a);
        u = unit_co(b);
      } else {
        e = A.E[idx * A.lde + (k - 1)];
        u = A.U[idx * A.ldu + (k - 1)];
      }
      const double h0 = r1 * x, h1 = (r2 * x) * y, h2 = r3 * y;
      const double s = (h0 + h1) + h2;
      const double inv = 1.0 / s;
      double tn = t + inv * e;
      const double p0 = h0 * inv, p1 = h1 * inv;
      const double c1 = p0 + p1;
      int reaction = (int)(u >= p0) + (int)(u >= c1);
      if (isinf(inv)) reaction = 3;
      const double xn = x + (reaction == 0 ? 1.0 : reaction == 1 ? -1.0 : 0.0);
      const double yn = y + (reaction == 1 ? 1.0 : reaction == 2 ? -1.0 : 0.0);
      if (yn == 0.0) tn = time_end;
      // observations this event passes: between the state before it and the state after it
      while (io < n_obs) {
        const double to = io == n_obs - 1 ? time_end : (double)io * A.step;
        if (!(tn >= to)) break;
        const double term = (to - t) / (tn - t);
        double vx = (xn - x) * term + x, vy = (yn - y) * term + y;
        if constexpr (NOISE) {
          double z0, z1;
          if (A.Z) {
            z0 = A.Z[idx * A.ldz + 2 * (io - 1)];
            z1 = A.Z[idx * A.ldz + 2 * (io - 1) + 1];
          } else {
            normal_pair(A.seed, A.stream + 1, (A.first + (uint64_t)idx) * (uint64_t)(n_obs - 1) + (uint64_t)(io - 1), z0, z1);
          }
          vx = vx + sg * z0;
          vy = vy + sg * z1;
        }
        yrow[2 * io] = lv_store(vx);
        yrow[2 * io + 1] = lv_store(vy);
        ++io;
      }
      x = xn;
      y = yn;
      t = tn;
      const bool reached = t >= time_end;
      if (reached || k >= A.max_events) {
        for (; io < n_obs; ++io) {       // only when the events ran out: what was not observed is NaN
          yrow[2 * io] = NAN;
          yrow[2 * io + 1] = NAN;
        }
        if (A.T) A.T[idx] = t;
        if (A.status) A.status[idx] = !reached ? ELFIHIP_LV_OUT_OF_EVENTS : y == 0.0 ? ELFIHIP_LV_EXTINCT : ELFIHIP_LV_REACHED_END;
        if (A.events) A.events[idx] = k;
        active = false;
      }
    }
  }
}

// the draws of the drawn form, into memory: E, U (n, n_events) -- what the given form takes
__global__ __launch_bounds__(256) void lv_draws_kernel(uint64_t seed, uint64_t stream, uint64_t first, int64_t n, int n_events,
                                                       double* __restrict__ E, int64_t lde, double* __restrict__ U,
                                                       int64_t ldu) {
  const int64_t total = n * n_events, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t el = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; el < total; el += stride) {
    const int64_t i = el / n_events;
    const int k = (int)(el - i * n_events) + 1;
    uint64_t a, b;
    words53(seed, stream, (uint32_t)k, (uint32_t)(first + (uint64_t)i), a, b);
    E[i * lde + (k - 1)] = unit_exponential(a);
    U[i * ldu + (k - 1)] = unit_co(b);
  }
}

// ---- summaries --------------------------------------------------------------------------------------------------------
struct LvSumArgs {
  const double* Y;
  int64_t ldy, n;
  int n_obs;
  double* S;        // optional (n, lds)
  int64_t lds;
  double* D;        // optional (n)
  double obs[LV_SUMMARIES];
};

template <bool WIDE, class F>
__device__ __forceinline__ double lv_row_sum(F f, int n) {
  if constexpr (WIDE)
    return np_pairwise(f, 0, n);
  else
    return np_pairwise_block(f, 0, n);
}

// The reference's functions on one series pair, each in its own operation order:
//   stock_mean          np.mean: the pairwise sum / n_obs
//   stock_log_variance  log(np.var(ddof=1) + 1): d = y - mean, sum(d d) / (n_obs - 1)
//   stock_autocorr      sx = (y - mean) / np.std(ddof=1); sum(sx[lag:] sx[:-lag]) / (n_obs - 1)
//   stock_crosscorr     s = (y - mean) / np.std(ddof=0) per species; sum(s_prey s_pred) / (n_obs - 1) -- ddof 0 in the standard
//                       deviations but n_obs - 1 in the mean of products, as the reference has it
// A constant series has standard deviation 0 and its correlations are 0 / 0 = NaN, as there.
template <bool WIDE>
__global__ __launch_bounds__(LV_THREADS) void lv_summary_kernel(LvSumArgs A) {
  const int n = A.n_obs;
  const int64_t stride = (int64_t)gridDim.x * LV_THREADS;
  for (int64_t gi = (int64_t)blockIdx.x * LV_THREADS + threadIdx.x; gi < A.n; gi += stride) {
    const double* w = A.Y + gi * A.ldy;
    double mean[2], lvar[2], ac1[2], ac2[2], sd0[2];
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
      const double mu = lv_row_sum<WIDE>([&](int i) { return w[2 * i + sp]; }, n) / (double)n;
      const double ss = lv_row_sum<WIDE>([&](int i) { const double d = w[2 * i + sp] - mu; return d * d; }, n);
      const double var1 = ss / (double)(n - 1);
      const double sd1 = sqrt(var1);
      mean[sp] = mu;
      lvar[sp] = log(var1 + 1.0);
      sd0[sp] = sqrt(ss / (double)n);
      ac1[sp] = lv_row_sum<WIDE>([&](int i) { return ((w[2 * (i + 1) + sp] - mu) / sd1) * ((w[2 * i + sp] - mu) / sd1); }, n - 1) /
                (double)(n - 1);
      ac2[sp] = lv_row_sum<WIDE>([&](int i) { return ((w[2 * (i + 2) + sp] - mu) / sd1) * ((w[2 * i + sp] - mu) / sd1); }, n - 2) /
                (double)(n - 1);
    }
    const double cc = lv_row_sum<WIDE>([&](int i) { return ((w[2 * i] - mean[0]) / sd0[0]) * ((w[2 * i + 1] - mean[1]) / sd0[1]); }, n) /
                      (double)(n - 1);
    const double s[LV_SUMMARIES] = {mean[0], mean[1], lvar[0], lvar[1], ac1[0], ac1[1], ac2[0], ac2[1], cc};
    if (A.S) {
#pragma unroll
      for (int j = 0; j < LV_SUMMARIES; ++j) A.S[gi * A.lds + j] = s[j];
    }
    if (A.D) {
      using Euclid = Op<ELFIHIP_EUCLIDEAN, false>;   // cdist's euclidean, the distance kernels' own row arithmetic
      double acc = Euclid::init();
#pragma unroll
      for (int j = 0; j < LV_SUMMARIES; ++j) acc = Euclid::step(acc, s[j], A.obs[j], 1.0, 2.0);
      A.D[gi] = Euclid::finish(acc, 0.5);
    }
  }
}

// ---- launches -----------------------------------------------------------------------------------------------------------
static int lv_dev_impl(elfihip_ctx* ctx, const double* dE, int64_t lde, const double* dU, int64_t ldu, const double* dZ,
                       int64_t ldz, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_obs, double time_end,
                       int64_t max_events, const double* dr1, const double* dr2, const double* dr3, const double* dprey,
                       const double* dpred, const double* dsigma, const double* obs, double* dY, int64_t ldy, double* dT,
                       int32_t* dstatus, int64_t* devents, double* dS, int64_t lds, double* dD) {
  ELFIHIP_REQUIRE(ctx, n >= 1, "bad batch n=%lld (at least 1)", (long long)n);
  ELFIHIP_REQUIRE(ctx, n_obs >= 3 && n_obs <= ELFIHIP_SERIES_MAX_OBS, "series of %d observations: 3 to %d", n_obs,
                  ELFIHIP_SERIES_MAX_OBS);
  ELFIHIP_REQUIRE(ctx, max_events >= 1 && max_events <= ELFIHIP_LV_MAX_EVENTS, "max_events %lld: 1 to 2^30", (long long)max_events);
  ELFIHIP_REQUIRE(ctx, std::isfinite(time_end) && time_end > 0.0, "time_end must be finite and positive");
  ELFIHIP_TRY(check_sim_indices(ctx, first, n));
  ELFIHIP_REQUIRE(ctx, (dE == nullptr) == (dU == nullptr), "E and U are given together or not at all");
  ELFIHIP_REQUIRE(ctx, !dZ || dsigma, "noise draws without sigma");
  ELFIHIP_REQUIRE(ctx, !dD || obs, "a distance needs the observed summaries");
  ELFIHIP_REQUIRE(ctx, dr1 && dr2 && dr3 && dprey && dpred, "NULL parameter pointer");
  ELFIHIP_REQUIRE(ctx, (!dE || (lde >= max_events && ldu >= max_events)) && (!dZ || ldz >= 2 * (n_obs - 1)) &&
                           (!dY || ldy >= 2 * n_obs) && (!dS || lds >= LV_SUMMARIES),
                  "leading dimension below the row length");
  // the counter, and the observations when the caller does not want them but the summaries need them
  const size_t ybytes = dY ? 0 : (size_t)n * 2 * n_obs * sizeof(double);
  ELFIHIP_CHECK_HIP(ctx, ctx->sim.reserve(SIM_HEAD + ybytes));
  LvArgs A;
  A.E = dE;
  A.U = dU;
  A.Z = dZ;
  A.lde = lde;
  A.ldu = ldu;
  A.ldz = ldz;
  A.seed = seed;
  A.stream = stream;
  A.first = (uint64_t)first;
  A.r1 = dr1;
  A.r2 = dr2;
  A.r3 = dr3;
  A.prey = dprey;
  A.pred = dpred;
  A.sigma = dsigma;
  A.n = n;
  A.n_obs = n_obs;
  A.max_events = (int)max_events;
  A.time_end = time_end;
  A.step = time_end / (double)(n_obs - 1);      // np.linspace's step
  A.Y = dY ? dY : reinterpret_cast<double*>(ctx->sim.as<char>() + SIM_HEAD);
  A.ldy = dY ? ldy : 2 * (int64_t)n_obs;
  A.T = dT;
  A.status = dstatus;
  A.events = reinterpret_cast<long long*>(devents);
  A.counter = ctx->sim.as<unsigned long long>();
  // a lane per simulation: never more wavefronts than there are groups of 64 simulations
  const int64_t groups = (n + LV_THREADS - 1) / LV_THREADS;
  if (dE) {
    if (dsigma)
      ELFIHIP_TRY(launch_persistent(ctx, lv_sim_kernel<false, true>, "lv_sim_kernel", groups, A));
    else
      ELFIHIP_TRY(launch_persistent(ctx, lv_sim_kernel<false, false>, "lv_sim_kernel", groups, A));
  } else {
    if (dsigma)
      ELFIHIP_TRY(launch_persistent(ctx, lv_sim_kernel<true, true>, "lv_sim_kernel", groups, A));
    else
      ELFIHIP_TRY(launch_persistent(ctx, lv_sim_kernel<true, false>, "lv_sim_kernel", groups, A));
  }
  if (!dS && !dD) return ELFIHIP_OK;
  LvSumArgs B;
  B.Y = A.Y;
  B.ldy = A.ldy;
  B.n = n;
  B.n_obs = n_obs;
  B.S = dS;
  B.lds = lds;
  B.D = dD;
  for (int j = 0; j < LV_SUMMARIES; ++j) B.obs[j] = obs ? obs[j] : 0.0;
  const unsigned grid = (unsigned)std::min<int64_t>((n + LV_THREADS - 1) / LV_THREADS, (int64_t)ctx->cu_count * 32);
  if (n_obs > 128)
    hipLaunchKernelGGL(lv_summary_kernel<true>, dim3(grid), dim3(LV_THREADS), 0, ctx->stream, B);
  else
    hipLaunchKernelGGL(lv_summary_kernel<false>, dim3(grid), dim3(LV_THREADS), 0, ctx->stream, B);
  return launch_status(ctx, "lv_summary_kernel");
}

static int lv_draws_impl(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int64_t n_events,
                         double* dE, int64_t lde, double* dU, int64_t ldu) {
  ELFIHIP_REQUIRE(ctx, n >= 1 && n_events >= 1 && n_events <= ELFIHIP_LV_MAX_EVENTS, "bad shape n=%lld n_events=%lld",
                  (long long)n, (long long)n_events);
  ELFIHIP_TRY(check_sim_indices(ctx, first, n));
  ELFIHIP_REQUIRE(ctx, dE && dU && lde >= n_events && ldu >= n_events, "NULL pointer or leading dimension below the row length");
  const unsigned grid = (unsigned)std::min<int64_t>((n * n_events + 255) / 256, (int64_t)ctx->cu_count * 16);
  hipLaunchKernelGGL(lv_draws_kernel, dim3(grid), dim3(256), 0, ctx->stream, seed, stream, (uint64_t)first, n, (int)n_events, dE,
                     lde, dU, ldu);
  return launch_status(ctx, "lv_draws_kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_lv_summaries_dev(elfihip_ctx* ctx, const double* dE, int64_t lde, const double* dU, int64_t ldu, const double* dZ,
                             int64_t ldz, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_obs, double time_end,
                             int64_t max_events, const double* dr1, const double* dr2, const double* dr3, const double* dprey,
                             const double* dpred, const double* dsigma, const double* obs, double* dY, int64_t ldy, double* dT,
                             int32_t* dstatus, int64_t* devents, double* dS, int64_t lds, double* dD) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return lv_dev_impl(ctx, dE, lde, dU, ldu, dZ, ldz, seed, stream, first, n, n_obs, time_end, max_events, dr1, dr2, dr3, dprey,
                     dpred, dsigma, obs, dY, ldy, dT, dstatus, devents, dS, lds, dD);
}

int elfihip_lv_summaries(elfihip_ctx* ctx, const double* E, const double* U, const double* Z, uint64_t seed, uint64_t stream,
                         int64_t first, int64_t n, int n_obs, double time_end, int64_t max_events, const double* r1,
                         const double* r2, const double* r3, const double* prey, const double* pred, const double* sigma,
                         const double* obs, double* Y, double* T, int32_t* status, int64_t* events, double* S, double* D) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 1 && n_obs >= 3 && n_obs <= ELFIHIP_SERIES_MAX_OBS, "bad shape n=%lld n_obs=%d", (long long)n, n_obs);
  ELFIHIP_REQUIRE(ctx, max_events >= 1 && max_events <= ELFIHIP_LV_MAX_EVENTS, "max_events %lld: 1 to 2^30", (long long)max_events);
  ELFIHIP_REQUIRE(ctx, (E == nullptr) == (U == nullptr), "E and U are given together or not at all");
  ELFIHIP_REQUIRE(ctx, !Z || sigma, "noise draws without sigma");
  ELFIHIP_REQUIRE(ctx, r1 && r2 && r3 && prey && pred, "NULL parameter pointer");
  ELFIHIP_REQUIRE(ctx, !D || obs, "a distance needs the observed summaries");
  DeviceGuard g(ctx->device);
  const size_t nn = (size_t)n, ne = E ? nn * (size_t)max_events : 0, nz = Z ? nn * 2 * (size_t)(n_obs - 1) : 0;
  const size_t ny = Y ? nn * 2 * (size_t)n_obs : 0;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((2 * ne + nz + 6 * nn) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((ny + (LV_SUMMARIES + 3) * nn) * sizeof(double) + nn * sizeof(int32_t)));
  double* dE = ctx->in.as<double>();
  double* dU = dE + ne;
  double* dZ = dU + ne;
  double* dpar = dZ + nz;
  double* dY = ctx->out.as<double>();
  double* dS = dY + ny;
  double* dD = dS + LV_SUMMARIES * nn;
  double* dT = dD + nn;
  int64_t* dev = reinterpret_cast<int64_t*>(dT + nn);
  int32_t* dst = reinterpret_cast<int32_t*>(dev + nn);
  const size_t pb = nn * sizeof(double);
  if (E) {
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dE, E, ne * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dU, U, ne * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  if (Z) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dZ, Z, nz * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const double* par[6] = {r1, r2, r3, prey, pred, sigma};
  for (int j = 0; j < 6; ++j)
    if (par[j]) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar + j * nn, par[j], pb, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(lv_dev_impl(ctx, E ? dE : nullptr, max_events, E ? dU : nullptr, max_events, Z ? dZ : nullptr, 2 * (int64_t)(n_obs - 1),
                          seed, stream, first, n, n_obs, time_end, max_events, dpar, dpar + nn, dpar + 2 * nn, dpar + 3 * nn,
                          dpar + 4 * nn, sigma ? dpar + 5 * nn : nullptr, obs, Y ? dY : nullptr, 2 * (int64_t)n_obs,
                          T ? dT : nullptr, status ? dst : nullptr, events ? dev : nullptr, S ? dS : nullptr, LV_SUMMARIES,
                          D ? dD : nullptr));
  if (Y) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Y, dY, ny * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (S) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(S, dS, LV_SUMMARIES * pb, hipMemcpyDeviceToHost, ctx->stream));
  if (D) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(D, dD, pb, hipMemcpyDeviceToHost, ctx->stream));
  if (T) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(T, dT, pb, hipMemcpyDeviceToHost, ctx->stream));
  if (events) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(events, dev, nn * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (status) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(status, dst, nn * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_lv_draws_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int64_t n_events,
                         double* dE, int64_t lde, double* dU, int64_t ldu) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return lv_draws_impl(ctx, seed, stream, first, n, n_events, dE, lde, dU, ldu);
}

int elfihip_lv_draws(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int64_t n_events, double* E,
                     double* U) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 1 && n_events >= 1 && n_events <= ELFIHIP_LV_MAX_EVENTS && E && U, "bad arguments");
  DeviceGuard g(ctx->device);
  const size_t ne = (size_t)n * (size_t)n_events;
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(2 * ne * sizeof(double)));
  double* dE = ctx->out.as<double>();
  double* dU = dE + ne;
  ELFIHIP_TRY(lv_draws_impl(ctx, seed, stream, first, n, n_events, dE, n_events, dU, n_events));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(E, dE, ne * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(U, dU, ne * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
