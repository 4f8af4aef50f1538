// ELFI's day-care-centre transmission example (Numminen et al. 2013; Gutmann and Corander 2016) on gfx950: an exact
// event-driven (Gillespie, direct method) simulator of the carriage of n_strains strains by the n_ind individuals of a
// centre, the four summaries over the first n_obs individuals and the example's sorted L1 distance.
//
// Replaces, for elfi/examples/daycare.py:
//     while any(time < time_end): state / sum, tile, where, hazards[state] = 1, 1 / sum, exponential, cumsum over all
//         n_ind n_strains hazards, uniform, unravel_index, flip  -- about 20 NumPy calls per EVENT over every centre of
//         every simulation of the batch, in lock-step until the slowest has passed time_end            daycare.py:99-136
//     ss_shannon, ss_strains, ss_prevalence, ss_prevalence_multi, distance                             daycare.py:199-312
//
// dc_sim_kernel: one wavefront per (simulation, centre) pair, persistent: a wavefront whose pair ends takes the NEXT pair
// from a counter in device memory (event_sim.hpp: one atomic per pair; event counts under the priors range from tens to over 10^4).  A
// lane is individual `lane` (its strains as the bits of `mask`) AND strain `lane` (its carriers as the bits of `car`):
// n_ind, n_strains <= 64.  The hazard of (i, s) is 1 where i carries s and c_i g_s elsewhere, so an event costs a lane
// n_ind + n_strains + n_ind + n_strains steps instead of n_ind n_strains hazards: the strain lanes sum P_s over the carriers'
// 1 / k_i (LDS broadcast reads) and form g_s, the individual lanes sum their row over the strains, every lane runs the prefix
// over the rows (the same values in the same order: the total, the chosen individual and the time stay wave-uniform), then
// the scan over the chosen individual's strains, one bit flips.  Each centre stops at ITS first event at or past time_end (the
// reference keeps all of a batch jumping until the slowest is done, so its result depends on the batch).  Every loop is
// bounded (events by max_events, pairs by the counter), no wavefront waits for another, and which wavefront ran a pair when
// does not enter its result: the draws of event k of centre c of simulation i are Philox counter ((c << 22) | k, i).
// dc_summary_kernel: one wavefront per pair over the masks written; Shannon's sum in NumPy's pairwise order (np_sum.hpp).
// dc_dist_kernel: rows of k summaries x m centres divided by the observed maxima, one lane Shell-sorts one row in LDS
// (lane_sort.hpp), |x - y| against the sorted observed row summed left to right.
// FMA contraction is off.  The statement of the model is in include/elfihip.h (elfihip_daycare_summaries) and, in NumPy, in
// tests/daycare_ref.py.
#include "common.hpp"

#include <algorithm>
#include <cmath>

#include "event_sim.hpp"
#include "lane_sort.hpp"
#include "np_sum.hpp"
#include "philox.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int DC_THREADS = SIM_THREADS;
constexpr int DC_EVENT_BITS = 22;     // Philox counter word 0: (centre << 22) | event;  max_events <= 2^21, n_dcc <= 2^10
constexpr int DC_SUMMARIES = ELFIHIP_DAYCARE_SUMMARIES;
constexpr size_t DC_DIST_LDS = 48 * 1024;

struct DcArgs {
  const double* E;      // (n n_dcc, lde) unit exponentials, or NULL with U: drawn here
  const double* U;      // (n n_dcc, ldu) uniforms in [0, 1)
  int64_t lde, ldu;
  uint64_t seed, stream, first;
  const double *t1, *t2, *t3;   // (n) each
  int64_t n;
  int n_dcc, n_ind, n_strains, n_obs, max_events;
  double time_end, nf;  // nf = 1 / (n_ind - 1)
  unsigned long long* M;   // (n n_dcc, ldm): the strain masks of the first n_obs individuals
  int64_t ldm;
  double* T;            // optional (n n_dcc): the time of the last event
  int* status;          // (n n_dcc)
  long long* events;    // optional (n n_dcc)
  unsigned long long* counter;   // the next pair, zero at launch
  double f[ELFIHIP_DAYCARE_MAX_STRAINS];   // the strains' prevalence in the community
};

template <bool DRAWN>
__global__ __launch_bounds__(DC_THREADS) void dc_sim_kernel(DcArgs A) {
  __shared__ double s_invk[DC_THREADS], s_g[DC_THREADS], s_r[DC_THREADS];
  __shared__ unsigned long long s_msk[DC_THREADS];
  const int lane = threadIdx.x, n_ind = A.n_ind, n_strains = A.n_strains;
  const unsigned long long pairs = (unsigned long long)A.n * (unsigned long long)A.n_dcc;
  const double fs = lane < n_strains ? A.f[lane] : 0.0;
  for (;;) {
    const unsigned long long p = wave_fetch(A.counter, lane, 1ull);   // the next pair, a scalar
    if (p >= pairs) break;
    const int64_t sim = (int64_t)(p / (unsigned)A.n_dcc);
    const uint32_t centre = (uint32_t)(p - (unsigned long long)sim * (unsigned)A.n_dcc);
    const double t1 = A.t1[sim], t2 = A.t2[sim], t3 = A.t3[sim];
    unsigned long long mask = 0ull, car = 0ull;
    double t = 0.0;
    int k = 0;
    bool reached = false;
    if (!(rate_ok(t1) && rate_ok(t2) && rate_ok(t3))) {    // (uniform) the whole simulation is invalid
      if (lane < A.n_obs) A.M[p * A.ldm + lane] = 0ull;
      if (lane == 0) {
        A.status[p] = ELFIHIP_DAYCARE_INVALID;
        if (A.T) A.T[p] = NAN;
        if (A.events) A.events[p] = 0;
      }
      continue;
    }
    const double t2f = t2 * fs;
    while (k < A.max_events) {       // every value that decides the control flow is the same in all 64 lanes
      ++k;
      double e, u;
      if constexpr (DRAWN) {
        const uint64_t g = A.first + (uint64_t)sim;
        uint64_t a, b;
        words53(A.seed, A.stream, (centre << DC_EVENT_BITS) | (uint32_t)k, (uint32_t)g, a, b);
        e = unit_exponential(a);
        u = unit_co(b);
      } else {
        e = A.E[p * A.lde + (k - 1)];
        u = A.U[p * A.ldu + (k - 1)];
      }
      const int cnt = __popcll(mask);
      s_invk[lane] = cnt ? 1.0 / (double)cnt : 0.0;
      s_msk[lane] = mask;
      __syncthreads();
      // strain `lane`: P = the carriers' 1 / k_i, individuals ascending
      double P = 0.0;
      for (int i = 0; i < n_ind; ++i) P += ((car >> i) & 1ull) ? s_invk[i] : 0.0;
      s_g[lane] = ((t1 * P) * A.nf + 1e-9) + t2f;
      __syncthreads();
      // individual `lane`: the row of hazards, strains ascending
      const double c = cnt ? t3 : 1.0;
      double r = 0.0;
      for (int s = 0; s < n_strains; ++s) r += ((mask >> s) & 1ull) ? 1.0 : c * s_g[s];
      s_r[lane] = r;
      __syncthreads();
      // the prefix over the rows: lane j keeps cum_j, all lanes the total
      double acc = 0.0, mycum = 0.0;
      for (int j = 0; j < n_ind; ++j) {
        acc += s_r[j];
        if (j == lane) mycum = acc;
      }
      const double total = acc, target = u * total;
      const int is = __popcll(__ballot(lane < n_ind - 1 && target >= mycum));
      const double before = __shfl(mycum, is > 0 ? is - 1 : 0);
      const double rem = target - (is > 0 ? before : 0.0);
      // the scan over the chosen individual's strains
      const unsigned long long m_sel = s_msk[is];
      const double c_sel = m_sel ? t3 : 1.0;
      double part = 0.0;
      int ss = 0;
      for (int s = 0; s < n_strains; ++s) {
        part += ((m_sel >> s) & 1ull) ? 1.0 : c_sel * s_g[s];
        ss += (int)(s < n_strains - 1 && rem >= part);
      }
      if (lane == is) mask ^= 1ull << ss;
      if (lane == ss) car ^= 1ull << is;
      t = t + e / total;
      __syncthreads();          // the next event overwrites what this one read
      if (__builtin_amdgcn_readfirstlane((int)(t >= A.time_end))) {      // the same in all lanes: said so
        reached = true;
        break;
      }
    }
    if (lane < A.n_obs) A.M[p * A.ldm + lane] = mask;
    if (lane == 0) {
      A.status[p] = reached ? ELFIHIP_DAYCARE_REACHED_END : ELFIHIP_DAYCARE_OUT_OF_EVENTS;
      if (A.T) A.T[p] = t;
      if (A.events) A.events[p] = k;
    }
  }
}

// the draws of the drawn form, into memory: E, U (n n_dcc, n_events) -- what the given form takes
__global__ __launch_bounds__(256) void dc_draws_kernel(uint64_t seed, uint64_t stream, uint64_t first, int64_t n, int n_dcc,
                                                       int n_events, double* __restrict__ E, int64_t lde,
                                                       double* __restrict__ U, int64_t ldu) {
  const int64_t total = n * n_dcc * n_events, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t el = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; el < total; el += stride) {
    const int64_t p = el / n_events, i = p / n_dcc;
    const int k = (int)(el - p * n_events) + 1;
    const uint64_t g = first + (uint64_t)i;
    uint64_t a, b;
    words53(seed, stream, ((uint32_t)(p - i * n_dcc) << DC_EVENT_BITS) | (uint32_t)k, (uint32_t)g, a, b);
    E[p * lde + (k - 1)] = unit_exponential(a);
    U[p * ldu + (k - 1)] = unit_co(b);
  }
}

// ---- summaries --------------------------------------------------------------------------------------------------------
struct DcSumArgs {
  const unsigned long long* M;
  int64_t ldm, n;
  const int* status;
  int n_dcc, n_strains, n_obs;
  double* S;        // (n, lds): summary j of centre c at j n_dcc + c
  int64_t lds;
};

// The reference's functions on the observed individuals of one centre:
//   ss_shannon           p_s = (carriers of s) / (all carriages), 0 / 0 -> 0, then 0 -> 1;  -(pairwise sum of p log p)
//   ss_strains           the number of strains somebody carries
//   ss_prevalence        (individuals who carry anything) / n_obs
//   ss_prevalence_multi  (individuals who carry more than one strain) / n_obs
__global__ __launch_bounds__(DC_THREADS) void dc_summary_kernel(DcSumArgs A) {
  __shared__ unsigned long long s_msk[DC_THREADS];
  __shared__ double s_term[DC_THREADS];
  const int lane = threadIdx.x;
  const int64_t pairs = A.n * A.n_dcc;
  for (int64_t p = blockIdx.x; p < pairs; p += gridDim.x) {
    const unsigned long long mask = lane < A.n_obs ? A.M[p * A.ldm + lane] : 0ull;
    s_msk[lane] = mask;
    __syncthreads();
    int cnt = 0, total = 0;
    for (int i = 0; i < A.n_obs; ++i) {
      const unsigned long long mi = s_msk[i];
      cnt += (int)((mi >> lane) & 1ull);
      total += __popcll(mi);
    }
    if (lane >= A.n_strains) cnt = 0;
    const double prop = cnt == 0 ? 1.0 : (double)cnt / (double)total;
    s_term[lane] = prop * log(prop);
    const int seen = __popcll(__ballot(cnt > 0));
    const int infected = __popcll(__ballot(mask != 0ull)), multi = __popcll(__ballot(__popcll(mask) > 1));
    __syncthreads();
    if (lane == 0) {
      const int64_t sim = p / A.n_dcc;
      double* out = A.S + sim * A.lds + (p - sim * A.n_dcc);
      const bool ok = A.status[p] == ELFIHIP_DAYCARE_REACHED_END;
      const double shannon = -np_pairwise_block([&](int s) { return s_term[s]; }, 0, A.n_strains);
      out[0] = ok ? shannon : NAN;
      out[A.n_dcc] = ok ? (double)seen : NAN;
      out[2 * (int64_t)A.n_dcc] = ok ? (double)infected / (double)A.n_obs : NAN;
      out[3 * (int64_t)A.n_dcc] = ok ? (double)multi / (double)A.n_obs : NAN;
    }
    __syncthreads();
  }
}

// ---- the distance -------------------------------------------------------------------------------------------------------
// the observed rows, once per call: one workgroup per summary: the row's maximum (1 where it is 0), the row divided by it, sorted
__global__ __launch_bounds__(DC_THREADS) void dc_obs_kernel(const double* __restrict__ obs, int m, double* __restrict__ ys,
                                                            double* __restrict__ om) {
  extern __shared__ __align__(16) double tile[];
  const int tid = threadIdx.x;
  const double* row = obs + (int64_t)blockIdx.x * m;
  double mx = -INFINITY;
  for (int c = tid; c < m; c += DC_THREADS) mx = fmax(mx, row[c]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  const double o = mx == 0.0 ? 1.0 : mx;
  for (int c = tid; c < m; c += DC_THREADS) tile[c] = row[c] / o;
  __syncthreads();
  if (tid == 0) {
    shell_sort(tile, m, nan_last_after);
    om[blockIdx.x] = o;
  }
  __syncthreads();
  for (int c = tid; c < m; c += DC_THREADS) ys[(int64_t)blockIdx.x * m + c] = tile[c];
}

// X (n, ldx): summary j of column c of simulation i at i ldx + j m + c.  A tile is Rt simulations = Rt k rows of pitch Lp in LDS.
__global__ __launch_bounds__(DC_THREADS) void dc_dist_kernel(const double* __restrict__ X, int64_t ldx, int64_t n, int k, int m,
                                                             int Lp, int Rt, const double* __restrict__ ys,
                                                             const double* __restrict__ om, double* __restrict__ D) {
  extern __shared__ __align__(16) double tile[];
  double* rowsum = tile + (size_t)Rt * k * Lp;
  const int tid = threadIdx.x;
  for (int64_t s0 = (int64_t)blockIdx.x * Rt; s0 < n; s0 += (int64_t)gridDim.x * Rt) {
    const int sims = n - s0 < Rt ? (int)(n - s0) : Rt, rows = sims * k, km = k * m;
    for (int idx = tid; idx < sims * km; idx += DC_THREADS) {
      const int sim = idx / km, rest = idx - sim * km, j = rest / m, c = rest - j * m;
      tile[(sim * k + j) * Lp + c] = X[(s0 + sim) * ldx + rest] / om[j];
    }
    __syncthreads();
    if (tid < rows) {
      double* y = tile + (size_t)tid * Lp;
      shell_sort(y, m, nan_last_after);
      const double* yo = ys + (size_t)(tid % k) * m;
      double acc = 0.0;
      for (int c = 0; c < m; ++c) acc += fabs(y[c] - yo[c]);
      rowsum[tid] = acc;
    }
    __syncthreads();
    if (tid < sims) {
      double acc = 0.0;
      for (int j = 0; j < k; ++j) acc += rowsum[tid * k + j];
      D[s0 + tid] = acc / (double)km;
    }
    __syncthreads();
  }
}

// ---- launches -----------------------------------------------------------------------------------------------------------
// obs (k, m) host values -> the sorted, normalised rows and the maxima at `work` (device: raw k m, sorted k m, maxima k),
// then D (n) of the rows of dX
static int dc_distance_launch(elfihip_ctx* ctx, const double* dX, int64_t ldx, int64_t n, int k, int m, const double* obs,
                              double* work, double* dD) {
  const size_t km = (size_t)k * m;
  double *raw = work, *ys = work + km, *om = ys + km;
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(raw, obs, km * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(dc_obs_kernel, dim3(k), dim3(DC_THREADS), (size_t)m * sizeof(double), ctx->stream, raw, m, ys, om);
  ELFIHIP_TRY(launch_status(ctx, "dc_obs_kernel"));
  const int Lp = m | 1;        // an odd pitch: the lanes' rows start on different banks
  const size_t per_sim = ((size_t)k * Lp + k) * sizeof(double);
  const int Rt = (int)std::max<size_t>(1, std::min<size_t>(DC_THREADS / k, DC_DIST_LDS / per_sim));
  const unsigned grid = (unsigned)std::min<int64_t>((n + Rt - 1) / Rt, (int64_t)ctx->cu_count * 16);
  hipLaunchKernelGGL(dc_dist_kernel, dim3(grid), dim3(DC_THREADS), Rt * per_sim, ctx->stream, dX, ldx, n, k, m, Lp, Rt, ys, om, dD);
  return launch_status(ctx, "dc_dist_kernel");
}

static int dc_distance_check(elfihip_ctx* ctx, int64_t n, int k, int m, const double* obs) {
  ELFIHIP_REQUIRE(ctx, n >= 1, "bad batch n=%lld (at least 1)", (long long)n);
  ELFIHIP_REQUIRE(ctx, k >= 1 && k <= ELFIHIP_DAYCARE_DIST_MAX_SUMMARIES && m >= 1 && m <= ELFIHIP_DAYCARE_MAX_DCC &&
                           (int64_t)k * m <= ELFIHIP_DAYCARE_DIST_MAX_TERMS,
                  "distance over %d summaries of %d columns: 1 to %d summaries, 1 to %d columns, at most %d values", k, m,
                  ELFIHIP_DAYCARE_DIST_MAX_SUMMARIES, ELFIHIP_DAYCARE_MAX_DCC, ELFIHIP_DAYCARE_DIST_MAX_TERMS);
  ELFIHIP_REQUIRE(ctx, obs, "the distance needs the observed summaries");
  for (int64_t j = 0; j < (int64_t)k * m; ++j) ELFIHIP_REQUIRE(ctx, std::isfinite(obs[j]), "observed summary %lld is not finite", (long long)j);
  return ELFIHIP_OK;
}

static int dc_distance_dev_impl(elfihip_ctx* ctx, const double* dX, int64_t ldx, int64_t n, int k, int m, const double* obs,
                                double* dD) {
  ELFIHIP_TRY(dc_distance_check(ctx, n, k, m, obs));
  ELFIHIP_REQUIRE(ctx, dX && dD && ldx >= (int64_t)k * m, "NULL pointer or leading dimension below the row length");
  ELFIHIP_CHECK_HIP(ctx, ctx->sim.reserve(SIM_HEAD + (2 * (size_t)k * m + k) * sizeof(double)));
  return dc_distance_launch(ctx, dX, ldx, n, k, m, obs, reinterpret_cast<double*>(ctx->sim.as<char>() + SIM_HEAD), dD);
}

static int dc_shape_check(elfihip_ctx* ctx, int64_t first, int64_t n, int n_dcc, int64_t n_events) {
  ELFIHIP_REQUIRE(ctx, n >= 1 && n <= ELFIHIP_DAYCARE_MAX_BATCH, "bad batch n=%lld: 1 to 2^31 - 1", (long long)n);
  ELFIHIP_REQUIRE(ctx, n_dcc >= 1 && n_dcc <= ELFIHIP_DAYCARE_MAX_DCC, "%d centres: 1 to %d", n_dcc, ELFIHIP_DAYCARE_MAX_DCC);
  ELFIHIP_REQUIRE(ctx, n_events >= 1 && n_events <= ELFIHIP_DAYCARE_MAX_EVENTS, "max_events %lld: 1 to 2^21", (long long)n_events);
  return check_sim_indices(ctx, first, n);
}

static int dc_dev_impl(elfihip_ctx* ctx, const double* dE, int64_t lde, const double* dU, int64_t ldu, uint64_t seed,
                       uint64_t stream, int64_t first, int64_t n, int n_dcc, int n_ind, int n_strains, int n_obs, double time_end,
                       int64_t max_events, const double* dt1, const double* dt2, const double* dt3, const double* freq,
                       const double* obs, uint64_t* dM, int64_t ldm, double* dT, int32_t* dstatus, int64_t* devents, double* dS,
                       int64_t lds, double* dD) {
  ELFIHIP_TRY(dc_shape_check(ctx, first, n, n_dcc, max_events));
  ELFIHIP_REQUIRE(ctx, n_ind >= 2 && n_ind <= ELFIHIP_DAYCARE_MAX_IND, "%d individuals: 2 to %d", n_ind, ELFIHIP_DAYCARE_MAX_IND);
  ELFIHIP_REQUIRE(ctx, n_strains >= 1 && n_strains <= ELFIHIP_DAYCARE_MAX_STRAINS, "%d strains: 1 to %d", n_strains,
                  ELFIHIP_DAYCARE_MAX_STRAINS);
  ELFIHIP_REQUIRE(ctx, n_obs >= 1 && n_obs <= n_ind, "%d observed individuals: 1 to n_ind = %d", n_obs, n_ind);
  ELFIHIP_REQUIRE(ctx, std::isfinite(time_end) && time_end > 0.0, "time_end must be finite and positive");
  ELFIHIP_REQUIRE(ctx, (dE == nullptr) == (dU == nullptr), "E and U are given together or not at all");
  ELFIHIP_REQUIRE(ctx, dt1 && dt2 && dt3, "NULL parameter pointer");
  for (int s = 0; freq && s < n_strains; ++s)
    ELFIHIP_REQUIRE(ctx, std::isfinite(freq[s]) && freq[s] >= 0.0, "freq_strains_commun[%d] must be finite and not negative", s);
  ELFIHIP_REQUIRE(ctx, !dD || obs, "a distance needs the observed summaries");
  ELFIHIP_REQUIRE(ctx, (!dE || (lde >= max_events && ldu >= max_events)) && (!dM || ldm >= n_obs) &&
                           (!dS || lds >= (int64_t)DC_SUMMARIES * n_dcc),
                  "leading dimension below the row length");
  if (dD) ELFIHIP_TRY(dc_distance_check(ctx, n, DC_SUMMARIES, n_dcc, obs));
  // the counter, the observed rows' work space, and whatever the kernels hand each other that the caller does not keep
  const size_t pairs = (size_t)n * n_dcc, km = (size_t)DC_SUMMARIES * n_dcc;
  const bool want_s = dS || dD;
  const size_t o_obs = SIM_HEAD, o_st = o_obs + align256((2 * km + DC_SUMMARIES) * sizeof(double));
  const size_t o_m = o_st + (dstatus ? 0 : align256(pairs * sizeof(int32_t)));
  const size_t o_s = o_m + (dM ? 0 : align256(pairs * n_obs * sizeof(uint64_t)));
  const size_t end = o_s + (dS || !dD ? 0 : align256((size_t)n * km * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->sim.reserve(end));
  char* base = ctx->sim.as<char>();
  DcArgs A;
  A.E = dE;
  A.U = dU;
  A.lde = lde;
  A.ldu = ldu;
  A.seed = seed;
  A.stream = stream;
  A.first = (uint64_t)first;
  A.t1 = dt1;
  A.t2 = dt2;
  A.t3 = dt3;
  A.n = n;
  A.n_dcc = n_dcc;
  A.n_ind = n_ind;
  A.n_strains = n_strains;
  A.n_obs = n_obs;
  A.max_events = (int)max_events;
  A.time_end = time_end;
  A.nf = 1.0 / (double)(n_ind - 1);
  A.M = dM ? reinterpret_cast<unsigned long long*>(dM) : reinterpret_cast<unsigned long long*>(base + o_m);
  A.ldm = dM ? ldm : n_obs;
  A.T = dT;
  A.status = dstatus ? dstatus : reinterpret_cast<int*>(base + o_st);
  A.events = reinterpret_cast<long long*>(devents);
  A.counter = ctx->sim.as<unsigned long long>();
  for (int s = 0; s < ELFIHIP_DAYCARE_MAX_STRAINS; ++s) A.f[s] = s < n_strains ? (freq ? freq[s] : 0.1) : 0.0;
  if (dE)
    ELFIHIP_TRY(launch_persistent(ctx, dc_sim_kernel<false>, "dc_sim_kernel", (int64_t)pairs, A));
  else
    ELFIHIP_TRY(launch_persistent(ctx, dc_sim_kernel<true>, "dc_sim_kernel", (int64_t)pairs, A));
  if (!want_s) return ELFIHIP_OK;
  DcSumArgs B;
  B.M = A.M;
  B.ldm = A.ldm;
  B.n = n;
  B.status = A.status;
  B.n_dcc = n_dcc;
  B.n_strains = n_strains;
  B.n_obs = n_obs;
  B.S = dS ? dS : reinterpret_cast<double*>(base + o_s);
  B.lds = dS ? lds : (int64_t)km;
  const unsigned grid = (unsigned)std::min<int64_t>((int64_t)pairs, (int64_t)ctx->cu_count * 32);
  hipLaunchKernelGGL(dc_summary_kernel, dim3(grid), dim3(DC_THREADS), 0, ctx->stream, B);
  ELFIHIP_TRY(launch_status(ctx, "dc_summary_kernel"));
  if (!dD) return ELFIHIP_OK;
  return dc_distance_launch(ctx, B.S, B.lds, n, DC_SUMMARIES, n_dcc, obs, reinterpret_cast<double*>(base + o_obs), dD);
}

static int dc_draws_impl(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_dcc, int64_t n_events,
                         double* dE, int64_t lde, double* dU, int64_t ldu) {
  ELFIHIP_TRY(dc_shape_check(ctx, first, n, n_dcc, n_events));
  ELFIHIP_REQUIRE(ctx, dE && dU && lde >= n_events && ldu >= n_events, "NULL pointer or leading dimension below the row length");
  const int64_t total = n * n_dcc * n_events;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)ctx->cu_count * 16);
  hipLaunchKernelGGL(dc_draws_kernel, dim3(grid), dim3(256), 0, ctx->stream, seed, stream, (uint64_t)first, n, n_dcc, (int)n_events,
                     dE, lde, dU, ldu);
  return launch_status(ctx, "dc_draws_kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_daycare_summaries_dev(elfihip_ctx* ctx, const double* dE, int64_t lde, const double* dU, int64_t ldu, uint64_t seed,
                                  uint64_t stream, int64_t first, int64_t n, int n_dcc, int n_ind, int n_strains, int n_obs,
                                  double time_end, int64_t max_events, const double* dt1, const double* dt2, const double* dt3,
                                  const double* freq, const double* obs, uint64_t* dM, int64_t ldm, double* dT, int32_t* dstatus,
                                  int64_t* devents, double* dS, int64_t lds, double* dD) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return dc_dev_impl(ctx, dE, lde, dU, ldu, seed, stream, first, n, n_dcc, n_ind, n_strains, n_obs, time_end, max_events, dt1, dt2,
                     dt3, freq, obs, dM, ldm, dT, dstatus, devents, dS, lds, dD);
}

int elfihip_daycare_summaries(elfihip_ctx* ctx, const double* E, const double* U, uint64_t seed, uint64_t stream, int64_t first,
                              int64_t n, int n_dcc, int n_ind, int n_strains, int n_obs, double time_end, int64_t max_events,
                              const double* t1, const double* t2, const double* t3, const double* freq, const double* obs,
                              uint64_t* M, double* T, int32_t* status, int64_t* events, double* S, double* D) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(dc_shape_check(ctx, first, n, n_dcc, max_events));
  ELFIHIP_REQUIRE(ctx, n_obs >= 1 && n_obs <= ELFIHIP_DAYCARE_MAX_IND, "%d observed individuals: 1 to n_ind", n_obs);
  ELFIHIP_REQUIRE(ctx, (E == nullptr) == (U == nullptr), "E and U are given together or not at all");
  ELFIHIP_REQUIRE(ctx, t1 && t2 && t3, "NULL parameter pointer");
  DeviceGuard g(ctx->device);
  const size_t nn = (size_t)n, pairs = nn * (size_t)n_dcc, ne = E ? pairs * (size_t)max_events : 0;
  const size_t nm = M ? pairs * (size_t)n_obs : 0, ns = S ? nn * DC_SUMMARIES * (size_t)n_dcc : 0;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((2 * ne + 3 * nn) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((nm + ns + nn + 2 * pairs) * sizeof(double) + pairs * sizeof(int32_t)));
  double* dE = ctx->in.as<double>();
  double* dU = dE + ne;
  double* dpar = dU + ne;
  uint64_t* dM = ctx->out.as<uint64_t>();
  double* dS = reinterpret_cast<double*>(dM + nm);
  double* dD = dS + ns;
  double* dT = dD + nn;
  int64_t* dev = reinterpret_cast<int64_t*>(dT + pairs);
  int32_t* dst = reinterpret_cast<int32_t*>(dev + pairs);
  if (E) {
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dE, E, ne * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dU, U, ne * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  const double* par[3] = {t1, t2, t3};
  for (int j = 0; j < 3; ++j)
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar + j * nn, par[j], nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(dc_dev_impl(ctx, E ? dE : nullptr, max_events, E ? dU : nullptr, max_events, seed, stream, first, n, n_dcc, n_ind,
                          n_strains, n_obs, time_end, max_events, dpar, dpar + nn, dpar + 2 * nn, freq, obs, M ? dM : nullptr, n_obs,
                          T ? dT : nullptr, status ? dst : nullptr, events ? dev : nullptr, S ? dS : nullptr,
                          (int64_t)DC_SUMMARIES * n_dcc, D ? dD : nullptr));
  if (M) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(M, dM, nm * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (S) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(S, dS, ns * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (D) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(D, dD, nn * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (T) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(T, dT, pairs * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (events) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(events, dev, pairs * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (status) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(status, dst, pairs * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_daycare_draws_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_dcc,
                              int64_t n_events, double* dE, int64_t lde, double* dU, int64_t ldu) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return dc_draws_impl(ctx, seed, stream, first, n, n_dcc, n_events, dE, lde, dU, ldu);
}

int elfihip_daycare_draws(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_dcc, int64_t n_events,
                          double* E, double* U) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(dc_shape_check(ctx, first, n, n_dcc, n_events));
  ELFIHIP_REQUIRE(ctx, E && U, "NULL pointer");
  DeviceGuard g(ctx->device);
  const size_t ne = (size_t)n * (size_t)n_dcc * (size_t)n_events;
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(2 * ne * sizeof(double)));
  double* dE = ctx->out.as<double>();
  double* dU = dE + ne;
  ELFIHIP_TRY(dc_draws_impl(ctx, seed, stream, first, n, n_dcc, n_events, dE, n_events, dU, n_events));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(E, dE, ne * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(U, dU, ne * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_daycare_distance_dev(elfihip_ctx* ctx, const double* dX, int64_t ldx, int64_t n, int k, int m, const double* obs,
                                 double* dD) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return dc_distance_dev_impl(ctx, dX, ldx, n, k, m, obs, dD);
}

int elfihip_daycare_distance(elfihip_ctx* ctx, const double* X, int64_t n, int k, int m, const double* obs, double* D) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(dc_distance_check(ctx, n, k, m, obs));
  ELFIHIP_REQUIRE(ctx, X && D, "NULL pointer");
  DeviceGuard g(ctx->device);
  const size_t nx = (size_t)n * k * m;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(nx * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((size_t)n * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(ctx->in.p, X, nx * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(dc_distance_dev_impl(ctx, ctx->in.as<double>(), (int64_t)k * m, n, k, m, obs, ctx->out.as<double>()));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(D, ctx->out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
