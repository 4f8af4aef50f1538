// ELFI's birth-death-mutation example (Tanaka et al. 2006, the model of Lintusaari et al. 2017) on gfx950: a jump chain over
// up to 4096 cluster counts, its two summaries and the example's distance.
//
// Replaces, for elfi/examples/bdm.py:
//     per batch: np.savetxt of the parameters (4 decimals), a `bdm` executable compiled by hand as a subprocess, np.loadtxt
//         of its standard output, two os.remove                                                          bdm.py:19-68
//     T1, T2                                                                                            bdm.py:71-80
// and the simulator itself, elfi/examples/cpp/bdm.cpp: per event two uniforms, a search over three cumulative rates and a
// linear search over the cumulative cluster sizes.
//
// bd_sim_kernel: one wavefront per simulation, persistent: a wavefront takes its NEXT simulation from a counter in device
// memory (the events per simulation vary 40-fold over the prior), by one atomic of the whole wavefront read back as a scalar
// (event_sim.hpp: wave_fetch, and its reason).  Everything that decides the control flow -- pop, cluster_end, the event, the chosen
// cluster, the event count -- is the same in all 64 lanes, so the event loop has no divergent exit.
//   N <= 64: lane l holds clusters[l] in a register, and with it the INCLUSIVE cumulative sum up to l.  An event changes one or
//   two clusters by one, so the cumulative sums are kept, not recomputed: the lanes at or past the cluster add the change.  The
//   cluster search is one ballot of (double)cum > uc pop below cluster_end, the first empty slot one ballot of clusters == 0.
//   64 < N <= 4096: lane l owns the contiguous block [l B, (l + 1) B), B = ceil(N / 64), in LDS (16 KB), and keeps in registers
//   the block's sum, the inclusive cumulative sum of the block sums (kept up to date the same way) and the number of empty slots
//   of the block.  An event ballots the 64 cumulative block sums, then the one owning lane walks its block; the first empty slot
//   is the lowest lane that has one, then that lane's first.
//   N <= 32 and a batch of at least two full grids: bd_pair_kernel, two simulations per wavefront (its own comment below).
// The uniforms are fetched a wavefront at a time -- the given form loads 64 consecutive doubles (32 events) with one coalesced
// load, the drawn form makes 64 Philox calls (64 events), a lane each -- and handed out by readlane.  A given uniform is checked
// before it is used.  A search that finds nothing takes its last candidate; no index leaves [0, N).  Every loop is bounded: events
// by max_events, walks by the block, simulations by the counter; no wavefront waits for another, and which wavefront ran a
// simulation does not enter its result: event k of simulation g is Philox counter (g << 32) | k.
// The summaries are made in the same kernel from the clusters in LDS: the counts by a wave sum of integers, T2's sum in
// NumPy's pairwise order (np_sum.hpp) -- the lanes fill a leaf of at most 128 terms together, divide and square a lane each,
// and every lane adds the leaf up in NumPy's order, so the result is uniform.  FMA contraction is off.  The statement of the
// model is in include/elfihip.h (elfihip_bdm_clusters) and, in NumPy, in tests/bdm_ref.py.
#include "common.hpp"

#include <algorithm>
#include <cmath>

#include "dist_metrics.hpp"
#include "event_sim.hpp"
#include "np_sum.hpp"
#include "philox.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int BD_THREADS = SIM_THREADS;
constexpr int BD_MAX_N = ELFIHIP_BDM_MAX_N;      // 4096 = 64 lanes x 64 slots
constexpr int BD_LEAF = 128;                     // NumPy's pairwise leaf
constexpr int BD_PAIR_GRIDS = 2;                 // bd_pair_kernel from this many full grids (32 wavefronts per CU) of simulations on

struct BdArgs {
  const double* U;      // (n, ldu) uniforms, or NULL: drawn here
  int64_t ldu;
  uint64_t seed, stream, first;
  const double *alpha, *delta, *tau;   // (n) each
  int64_t n;
  int N, mode, B;       // B = ceil(N / 64): slots per lane of the wide form
  unsigned max_events;
  double t2n, obs;
  int32_t* Cl;          // optional (n, ldc)
  int64_t ldc;
  int* status;          // optional (n)
  long long* events;    // optional (n)
  double* T;            // optional (n, ldt): T1, T2
  int64_t ldt;
  double* D;            // optional (n)
  unsigned long long* counter;   // the next simulation, zero at launch
};

// the value lane `src` holds (src the same in every lane), as a scalar
__device__ __forceinline__ int bd_lane_int(int v, int src) {
  return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(src));
}
__device__ __forceinline__ double bd_lane_double(double v, int src) {
  const int s = __builtin_amdgcn_readfirstlane(src);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), s), __builtin_amdgcn_readlane(__double2loint(v), s));
}

// NumPy's pairwise sum of term(lo) .. term(lo + n - 1), by the whole wavefront: every call and every barrier is reached by all
// 64 lanes, the lanes fill a leaf together and each adds it up in NumPy's order
template <class F>
__device__ __forceinline__ double bd_leaf_sum(F term, double* leaf, int lo, int n, int lane) {
  __syncthreads();                 // the leaf before this one has been read
  for (int i = lane; i < n; i += BD_THREADS) leaf[i] = term(lo + i);
  __syncthreads();
  return np_pairwise_block([&](int i) { return leaf[i]; }, 0, n);
}

template <class F>
__device__ double bd_pairwise(F term, double* leaf, int lo, int n, int lane) {
  if (n <= BD_LEAF) return bd_leaf_sum(term, leaf, lo, n, lane);
  int n2 = n / 2;
  n2 -= n2 % 8;
  const double a = bd_pairwise(term, leaf, lo, n2, lane);
  const double b = bd_pairwise(term, leaf, lo + n2, n - n2, lane);
  return a + b;
}

template <bool DRAWN, bool WIDE>
__global__ __launch_bounds__(BD_THREADS) void bd_sim_kernel(BdArgs A) {
  __shared__ unsigned s_cl[WIDE ? BD_MAX_N : BD_THREADS];
  __shared__ double s_leaf[BD_LEAF];
  const int lane = threadIdx.x, N = A.N, B = WIDE ? A.B : 1;
  const int cap = N + (A.mode == 1);
  const int blk_lo = lane * B, blk_hi = blk_lo + B < N ? blk_lo + B : N;   // this lane's slots [blk_lo, blk_hi), empty past N
  for (;;) {
    const unsigned long long sim = wave_fetch(A.counter, lane, 1ull);   // the next simulation, a scalar
    if (sim >= (unsigned long long)A.n) break;
    const double alpha = A.alpha[sim], delta = A.delta[sim], tau = A.tau[sim];
    const double c0 = 0.0 + alpha, c1 = c0 + delta, c2 = c1 + tau, tot = c2;
    const bool rates_ok = rate_ok(alpha) && rate_ok(delta) && rate_ok(tau) && tot > 0.0 && tot < INFINITY;
    const uint64_t g = A.first + sim;
    const double* urow = DRAWN ? nullptr : A.U + (int64_t)sim * A.ldu;
    // the state: own (small form: this lane's cluster; wide form: this lane's block sum), cum (the inclusive cumulative sum
    // of own over the lanes), nz (wide form: empty slots of the block)
    int own = lane == 0 ? 1 : 0, cum = 1, nz = 0;
    if constexpr (WIDE) {
      for (int i = blk_lo; i < blk_lo + B; ++i) s_cl[i] = 0u;   // (64 B <= 4096: the whole array where N is no multiple of B)
      __syncthreads();
      if (lane == 0) s_cl[0] = 1u;
      nz = (blk_hi > blk_lo ? blk_hi - blk_lo : 0) - (lane == 0 ? 1 : 0);
      __syncthreads();
    }
    int pop = 1, cend = 1, cl = 0, st = rates_ok ? ELFIHIP_BDM_REACHED_N : ELFIHIP_BDM_INVALID;
    unsigned k = 0;                 // events made
    double bue = 0.0, buc = 0.0;    // this lane's share of the uniforms fetched last
    if (rates_ok) {
      while (pop > 0 && pop < cap) {      // (every value that decides the control flow is the same in all 64 lanes)
        if (k == A.max_events) {
          st = ELFIHIP_BDM_OUT_OF_EVENTS;
          break;
        }
        double ue, uc;
        if constexpr (DRAWN) {
          const int slot = (int)(k & 63u);
          if (slot == 0) uniform53_pair(A.seed, A.stream, k + 1u + (unsigned)lane, (uint32_t)g, bue, buc);   // (g << 32) | event
          ue = bd_lane_double(bue, slot);
          uc = bd_lane_double(buc, slot);
        } else {
          const int slot = (int)(k & 31u);
          if (slot == 0) {
            const uint64_t at = 2ull * k + (unsigned)lane;
            bue = at < 2ull * A.max_events ? urow[at] : 0.0;
          }
          ue = bd_lane_double(bue, 2 * slot);
          uc = bd_lane_double(bue, 2 * slot + 1);
          if (!(ue >= 0.0 && ue < 1.0) || !(uc >= 0.0 && uc < 1.0)) {   // nothing is indexed by an unchecked value
            st = ELFIHIP_BDM_INVALID;
            break;
          }
        }
        ++k;
        const double te = ue * tot, thr = uc * (double)pop;
        const int ev = c0 > te ? 0 : (c1 > te ? 1 : 2);
        const unsigned long long hit = __ballot((double)cum > thr && blk_lo < cend);
        int owner;                  // the lane that holds cluster cl
        unsigned cv;                // clusters[cl]
        if constexpr (WIDE) {
          if (hit) {
            owner = __ffsll((long long)hit) - 1;
            int found = blk_hi - 1;
            if (lane == owner) {
              unsigned run = (unsigned)(cum - own);
              for (int i = blk_lo; i < blk_hi; ++i) {
                run += s_cl[i];
                if ((double)run > thr) {
                  found = i;
                  break;
                }
              }
            }
            cl = bd_lane_int(found, owner);
          } else {
            cl = cend - 1;
            owner = cl / B;
          }
          cl = __builtin_amdgcn_readfirstlane(cl < 0 ? 0 : (cl >= N ? N - 1 : cl));
          cv = s_cl[cl];
        } else {
          cl = hit ? __ffsll((long long)hit) - 1 : cend - 1;
          owner = cl;
          cv = (unsigned)bd_lane_int(own, cl);
        }
        const bool split = ev == 2 && cv > 1u;
        const int change = ev == 0 ? 1 : ((ev == 1 || split) ? -1 : 0);
        pop += ev == 0 ? 1 : (ev == 1 ? -1 : 0);
        if constexpr (WIDE) {
          if (lane == owner) {
            const unsigned nv = cv + (unsigned)change;
            s_cl[cl] = nv;
            own += change;
            nz += (nv == 0u && cv != 0u ? 1 : 0) - (cv == 0u && nv != 0u ? 1 : 0);
          }
        } else {
          if (lane == owner) own += change;
        }
        if (lane >= owner) cum += change;
        if (split) {                // the first empty slot of [0, N) opens a cluster
          int j = -1, jl = 0;
          if constexpr (WIDE) {
            const unsigned long long has = __ballot(nz > 0);
            if (has) {
              jl = __ffsll((long long)has) - 1;
              int found = -1;
              if (lane == jl) {
                for (int i = blk_lo; i < blk_hi; ++i)
                  if (s_cl[i] == 0u) {
                    found = i;
                    break;
                  }
                if (found >= 0) {
                  s_cl[found] = 1u;
                  own += 1;
                  nz -= 1;
                }
              }
              j = bd_lane_int(found, jl);
            }
          } else {
            const unsigned long long has = __ballot(own == 0 && lane < N);
            if (has) {
              j = jl = __ffsll((long long)has) - 1;
              if (lane == j) own = 1;
            }
          }
          if (j >= 0) {
            if (lane >= jl) cum += 1;
            cend = cend > j + 1 ? cend : j + 1;
          }
        }
      }
    }
    if (st == ELFIHIP_BDM_REACHED_N) {
      if (pop == 0) {
        st = ELFIHIP_BDM_EXTINCT;
      } else if (A.mode == 1 && k > 0u) {   // Stadler's rule: the birth that reached N + 1 is taken back
        if constexpr (WIDE) {
          if (lane == cl / B) s_cl[cl] -= 1u;
        } else {
          if (lane == cl) own -= 1;
        }
        pop -= 1;
      }
    }
    if constexpr (WIDE) {
      if (st == ELFIHIP_BDM_INVALID)
        for (int i = blk_lo; i < blk_lo + B; ++i) s_cl[i] = 0u;
    } else {
      s_cl[lane] = st == ELFIHIP_BDM_INVALID ? 0u : (unsigned)own;
    }
    __syncthreads();
    if (A.Cl)
      for (int i = lane; i < N; i += BD_THREADS) A.Cl[(int64_t)sim * A.ldc + i] = (int32_t)s_cl[i];
    if (A.T || A.D) {               // (uniform)
      int cnt = 0, sum = 0;
      for (int i = lane; i < N; i += BD_THREADS) {
        const unsigned v = s_cl[i];
        cnt += v > 0u ? 1 : 0;
        sum += (int)v;
      }
      cnt = wave_sum(cnt);
      sum = wave_sum(sum);
      const double t2n = A.t2n;
      auto term = [&](int i) {
        const double q = (double)s_cl[i] / t2n;
        return q * q;
      };
      const double sq = WIDE ? bd_pairwise(term, s_leaf, 0, N, lane) : bd_leaf_sum(term, s_leaf, 0, N, lane);   // (N <= 64: one leaf)
      double t1 = (double)cnt / (double)sum, t2 = 1.0 - sq;
      if (st >= ELFIHIP_BDM_OUT_OF_EVENTS) t1 = t2 = NAN;
      if (lane == 0) {
        if (A.T) {
          A.T[(int64_t)sim * A.ldt] = t1;
          A.T[(int64_t)sim * A.ldt + 1] = t2;
        }
        using City = Op<ELFIHIP_CITYBLOCK, false>;   // the example's minkowski p = 1, the distance kernels' own row arithmetic
        if (A.D) A.D[sim] = City::finish(City::step(City::init(), t1, A.obs, 1.0, 1.0), 1.0);
      }
    }
    if (lane == 0) {
      if (A.status) A.status[sim] = st;
      if (A.events) A.events[sim] = (long long)k;
    }
    __syncthreads();                // the next simulation overwrites the clusters and the leaf
  }
}

// bd_pair_kernel: N <= 32, TWO simulations per wavefront, lanes 0 .. 31 and 32 .. 63 a simulation each.  What is a scalar in
// bd_sim_kernel is here a value the 32 lanes of a half share: ballots are read by halves, the uniforms and the chosen cluster's
// size come by ds_bpermute, and a half that has finished idles until the other has.  Slower for a lone wavefront, faster once
// the device is full (DESIGN.md has the numbers): the launch takes it from two full grids of simulations on.  The same
// counters, the same operations: a simulation's result is the one of bd_sim_kernel, bit for bit.
template <bool DRAWN>
__global__ __launch_bounds__(BD_THREADS) void bd_pair_kernel(BdArgs A) {
  __shared__ double s_leaf[BD_THREADS];
  const int lane = threadIdx.x, half = lane >> 5, l = lane & 31, h0 = half * 32, N = A.N;
  const int cap = N + (A.mode == 1);
  for (;;) {
    const unsigned long long base = wave_fetch(A.counter, lane, 2ull);   // the next two simulations, a scalar
    if (base >= (unsigned long long)A.n) break;
    const bool valid = base + half < (unsigned long long)A.n;       // (an odd batch: the last wavefront's upper half is idle)
    const unsigned long long sim = valid ? base + half : base;
    const double alpha = A.alpha[sim], delta = A.delta[sim], tau = A.tau[sim];
    const double c0 = 0.0 + alpha, c1 = c0 + delta, c2 = c1 + tau, tot = c2;
    const bool rates_ok = rate_ok(alpha) && rate_ok(delta) && rate_ok(tau) && tot > 0.0 && tot < INFINITY;
    const uint64_t g = A.first + sim;
    const double* urow = DRAWN ? nullptr : A.U + (int64_t)sim * A.ldu;
    int own = l == 0 ? 1 : 0, cum = 1, pop = 1, cend = 1, last = 0, st = rates_ok ? ELFIHIP_BDM_REACHED_N : ELFIHIP_BDM_INVALID;
    unsigned k = 0, made = 0;       // events the wavefront has stepped through, events this half has made
    double bue = 0.0, buc = 0.0;
    bool active = valid && rates_ok && pop < cap;
    while (__ballot(active) != 0ull) {
      if (k == A.max_events) {
        if (active) st = ELFIHIP_BDM_OUT_OF_EVENTS;
        break;
      }
      double ue, uc;
      if constexpr (DRAWN) {
        const int slot = (int)(k & 31u);
        if (slot == 0) uniform53_pair(A.seed, A.stream, k + 1u + (unsigned)l, (uint32_t)g, bue, buc);
        ue = __shfl(bue, h0 + slot, 64);
        uc = __shfl(buc, h0 + slot, 64);
      } else {
        const int slot = (int)(k & 15u);
        if (slot == 0) {
          const uint64_t at = 2ull * k + (unsigned)l;
          bue = at < 2ull * A.max_events ? urow[at] : 0.0;
        }
        ue = __shfl(bue, h0 + 2 * slot, 64);
        uc = __shfl(bue, h0 + 2 * slot + 1, 64);
        if (active && (!(ue >= 0.0 && ue < 1.0) || !(uc >= 0.0 && uc < 1.0))) {   // nothing is indexed by an unchecked value
          st = ELFIHIP_BDM_INVALID;
          active = false;
        }
      }
      ++k;
      made += active ? 1u : 0u;
      const double te = ue * tot, thr = uc * (double)pop;
      const int ev = c0 > te ? 0 : (c1 > te ? 1 : 2);
      const unsigned hit = (unsigned)(__ballot(active && (double)cum > thr && l < cend) >> h0);
      const int cl = hit ? __ffs((int)hit) - 1 : cend - 1;          // in [0, N): cend <= N <= 32
      const unsigned cv = (unsigned)__shfl(own, h0 + cl, 64);
      const bool split = active && ev == 2 && cv > 1u;
      const int change = !active ? 0 : (ev == 0 ? 1 : ((ev == 1 || split) ? -1 : 0));
      pop += !active ? 0 : (ev == 0 ? 1 : (ev == 1 ? -1 : 0));
      if (l == cl) own += change;
      if (l >= cl) cum += change;
      if (active) last = cl;
      if (__ballot(split) != 0ull) {                                // the first empty slot of [0, N) opens a cluster
        const unsigned has = (unsigned)(__ballot(own == 0 && l < N) >> h0);
        if (split && has) {
          const int j = __ffs((int)has) - 1;
          if (l == j) own = 1;
          if (l >= j) cum += 1;
          cend = cend > j + 1 ? cend : j + 1;
        }
      }
      active = active && pop > 0 && pop < cap;
    }
    if (st == ELFIHIP_BDM_REACHED_N) {
      if (pop == 0) {
        st = ELFIHIP_BDM_EXTINCT;
      } else if (A.mode == 1 && made > 0u) {   // Stadler's rule: the birth that reached N + 1 is taken back
        if (l == last) own -= 1;
        pop -= 1;
      }
    }
    if (st == ELFIHIP_BDM_INVALID) own = 0;
    if (A.Cl && valid && l < N) A.Cl[(int64_t)sim * A.ldc + l] = own;
    if (A.T || A.D) {               // (uniform)
      const int cnt = __popc((unsigned)(__ballot(own > 0 && l < N) >> h0));
      int sum = l < N ? own : 0;
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);    // (stays inside the half)
      const double q = (double)(unsigned)own / A.t2n;
      __syncthreads();              // the leaves of the pair before have been read
      s_leaf[lane] = q * q;
      __syncthreads();
      const double sq = np_pairwise_block([&](int i) { return s_leaf[h0 + i]; }, 0, N);
      double t1 = (double)cnt / (double)sum, t2 = 1.0 - sq;
      if (st >= ELFIHIP_BDM_OUT_OF_EVENTS) t1 = t2 = NAN;
      if (valid && l == 0) {
        if (A.T) {
          A.T[(int64_t)sim * A.ldt] = t1;
          A.T[(int64_t)sim * A.ldt + 1] = t2;
        }
        using City = Op<ELFIHIP_CITYBLOCK, false>;
        if (A.D) A.D[sim] = City::finish(City::step(City::init(), t1, A.obs, 1.0, 1.0), 1.0);
      }
    }
    if (valid && l == 0) {
      if (A.status) A.status[sim] = st;
      if (A.events) A.events[sim] = (long long)made;
    }
  }
}

// the uniforms of the drawn form, into memory: U (n, ldu), columns 2 (k - 1) and 2 (k - 1) + 1 of row i for event k
__global__ __launch_bounds__(256) void bd_draws_kernel(uint64_t seed, uint64_t stream, uint64_t first, int64_t n, int64_t n_events,
                                                       double* __restrict__ U, int64_t ldu) {
  const int64_t total = n * n_events, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t el = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; el < total; el += stride) {
    const int64_t i = el / n_events, e = el - i * n_events;
    double ue, uc;
    uniform53_pair(seed, stream, (uint32_t)(e + 1), (uint32_t)(first + (uint64_t)i), ue, uc);
    U[i * ldu + 2 * e] = ue;
    U[i * ldu + 2 * e + 1] = uc;
  }
}

// ---- launches -----------------------------------------------------------------------------------------------------------
static int bd_shape_check(elfihip_ctx* ctx, int64_t first, int64_t n, int64_t n_events) {
  ELFIHIP_REQUIRE(ctx, n >= 1, "bad batch n=%lld: at least 1", (long long)n);
  ELFIHIP_REQUIRE(ctx, n_events >= 1 && n_events <= ELFIHIP_BDM_MAX_EVENTS, "%lld events: 1 to 2^30", (long long)n_events);
  return check_sim_indices(ctx, first, n);
}

static int bd_model_check(elfihip_ctx* ctx, int64_t first, int64_t n, int N, int mode, int64_t max_events, const void* alpha,
                          const void* delta, const void* tau, const double* obs, const void* D) {
  ELFIHIP_TRY(bd_shape_check(ctx, first, n, max_events));
  ELFIHIP_REQUIRE(ctx, N >= 1 && N <= ELFIHIP_BDM_MAX_N, "population size N=%d: 1 to %d", N, ELFIHIP_BDM_MAX_N);
  ELFIHIP_REQUIRE(ctx, mode == 0 || mode == 1, "stopping mode %d: 0 or 1", mode);
  ELFIHIP_REQUIRE(ctx, alpha && delta && tau, "NULL pointer");
  ELFIHIP_REQUIRE(ctx, !D || obs, "a distance needs the observed summary");
  return ELFIHIP_OK;
}

static int bd_dev_impl(elfihip_ctx* ctx, const double* dU, int64_t ldu, uint64_t seed, uint64_t stream, int64_t first, int64_t n,
                       int N, int mode, int64_t max_events, const double* dalpha, const double* ddelta, const double* dtau,
                       double t2_n, const double* obs, int32_t* dCl, int64_t ldc, int32_t* dstatus, int64_t* devents, double* dT,
                       int64_t ldt, double* dD) {
  ELFIHIP_TRY(bd_model_check(ctx, first, n, N, mode, max_events, dalpha, ddelta, dtau, obs, dD));
  ELFIHIP_REQUIRE(ctx, (!dU || ldu >= 2 * max_events) && (!dCl || ldc >= N) && (!dT || ldt >= 2), "leading dimension below the row length");
  ELFIHIP_CHECK_HIP(ctx, ctx->sim.reserve(SIM_HEAD));
  BdArgs A;
  A.U = dU;
  A.ldu = ldu;
  A.seed = seed;
  A.stream = stream;
  A.first = (uint64_t)first;
  A.alpha = dalpha;
  A.delta = ddelta;
  A.tau = dtau;
  A.n = n;
  A.N = N;
  A.mode = mode;
  A.B = (N + BD_THREADS - 1) / BD_THREADS;
  A.max_events = (unsigned)max_events;
  A.t2n = t2_n;
  A.obs = obs ? obs[0] : 0.0;
  A.Cl = dCl;
  A.ldc = ldc;
  A.status = dstatus;
  A.events = reinterpret_cast<long long*>(devents);
  A.T = dT;
  A.ldt = ldt;
  A.D = dD;
  A.counter = ctx->sim.as<unsigned long long>();
  // two simulations per wavefront pay off once the device is full and lose before (N = 20, truth: 0.56 x the time at 10^5
  // simulations, 0.61 x at 10^4, 1.21 x at 500; from the prior 0.65 x, 1.17 x, 1.52 x -- DESIGN.md): from two full grids on
  if (N <= 32 && n >= BD_PAIR_GRIDS * (int64_t)ctx->cu_count * 32)
    return dU ? launch_persistent(ctx, bd_pair_kernel<false>, "bd_pair_kernel", (n + 1) / 2, A)
              : launch_persistent(ctx, bd_pair_kernel<true>, "bd_pair_kernel", (n + 1) / 2, A);
  if (N <= BD_THREADS)
    return dU ? launch_persistent(ctx, bd_sim_kernel<false, false>, "bd_sim_kernel", n, A)
              : launch_persistent(ctx, bd_sim_kernel<true, false>, "bd_sim_kernel", n, A);
  return dU ? launch_persistent(ctx, bd_sim_kernel<false, true>, "bd_sim_kernel", n, A)
            : launch_persistent(ctx, bd_sim_kernel<true, true>, "bd_sim_kernel", n, A);
}

static int bd_draws_impl(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int64_t n_events, double* dU,
                         int64_t ldu) {
  ELFIHIP_TRY(bd_shape_check(ctx, first, n, n_events));
  ELFIHIP_REQUIRE(ctx, dU, "NULL pointer");
  ELFIHIP_REQUIRE(ctx, ldu >= 2 * n_events, "leading dimension below the row length");
  const int64_t total = n * n_events;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)ctx->cu_count * 16);
  hipLaunchKernelGGL(bd_draws_kernel, dim3(grid), dim3(256), 0, ctx->stream, seed, stream, (uint64_t)first, n, n_events, dU, ldu);
  return launch_status(ctx, "bd_draws_kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_bdm_clusters_dev(elfihip_ctx* ctx, const double* dU, int64_t ldu, uint64_t seed, uint64_t stream, int64_t first,
                             int64_t n, int N, int mode, int64_t max_events, const double* dalpha, const double* ddelta,
                             const double* dtau, double t2_n, const double* obs, int32_t* dCl, int64_t ldc, int32_t* dstatus,
                             int64_t* devents, double* dT, int64_t ldt, double* dD) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return bd_dev_impl(ctx, dU, ldu, seed, stream, first, n, N, mode, max_events, dalpha, ddelta, dtau, t2_n, obs, dCl, ldc, dstatus,
                     devents, dT, ldt, dD);
}

int elfihip_bdm_clusters(elfihip_ctx* ctx, const double* U, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int N,
                         int mode, int64_t max_events, const double* alpha, const double* delta, const double* tau, double t2_n,
                         const double* obs, int32_t* Cl, int32_t* status, int64_t* events, double* T, double* D) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(bd_model_check(ctx, first, n, N, mode, max_events, alpha, delta, tau, obs, D));
  DeviceGuard g(ctx->device);
  const size_t nn = (size_t)n, nu = U ? nn * 2 * (size_t)max_events : 0, pb = nn * sizeof(double);
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((nu + 3 * nn) * sizeof(double)));
  const size_t o_d = align256(2 * pb), o_e = o_d + align256(pb), o_c = o_e + align256(nn * sizeof(int64_t));
  const size_t o_s = o_c + align256(nn * (size_t)N * sizeof(int32_t));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(o_s + nn * sizeof(int32_t)));
  char* out = ctx->out.as<char>();
  double *dU = ctx->in.as<double>(), *dpar = dU + nu;
  double* dT = ctx->out.as<double>();
  double* dD = reinterpret_cast<double*>(out + o_d);
  int64_t* dev = reinterpret_cast<int64_t*>(out + o_e);
  int32_t* dCl = reinterpret_cast<int32_t*>(out + o_c);
  int32_t* dst = reinterpret_cast<int32_t*>(out + o_s);
  if (U) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dU, U, nu * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar, alpha, pb, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar + nn, delta, pb, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar + 2 * nn, tau, pb, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(bd_dev_impl(ctx, U ? dU : nullptr, 2 * max_events, seed, stream, first, n, N, mode, max_events, dpar, dpar + nn,
                          dpar + 2 * nn, t2_n, obs, Cl ? dCl : nullptr, N, status ? dst : nullptr, events ? dev : nullptr,
                          T ? dT : nullptr, 2, D ? dD : nullptr));
  if (Cl) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Cl, dCl, nn * (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (status) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(status, dst, nn * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (events) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(events, dev, nn * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (T) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(T, dT, 2 * pb, hipMemcpyDeviceToHost, ctx->stream));
  if (D) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(D, dD, pb, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_bdm_draws_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int64_t n_events,
                          double* dU, int64_t ldu) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return bd_draws_impl(ctx, seed, stream, first, n, n_events, dU, ldu);
}

int elfihip_bdm_draws(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int64_t n_events, double* U) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(bd_shape_check(ctx, first, n, n_events));
  ELFIHIP_REQUIRE(ctx, U, "NULL pointer");
  DeviceGuard g(ctx->device);
  const size_t nu = (size_t)n * 2 * (size_t)n_events;
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(nu * sizeof(double)));
  ELFIHIP_TRY(bd_draws_impl(ctx, seed, stream, first, n, n_events, ctx->out.as<double>(), 2 * n_events));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(U, ctx->out.p, nu * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
