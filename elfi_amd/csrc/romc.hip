// Robust Optimisation Monte Carlo (Ikonomov & Gutmann 2019) for the MA2 example on gfx950: the frozen-noise objectives
// f_i(theta) = d_i(theta)^2, their Nelder-Mead minima and difference Hessians, the bounding boxes around the minima, the
// weighted samples and the indicator counts of the density.
//
// Replaces, for elfi/methods/inference/romc.py and RomcPosterior (elfi/methods/posteriors.py:393-800) on the MA2 model:
//     _det_generator: one model.generate(batch_size=1, seed=nuisance) per evaluation                     romc.py:562-574
//     OptimisationProblem.solve_gradients: scipy.optimize.minimize(method='Nelder-Mead') + a Hessian     romc.py:1397-1444
//     RegionConstructor.build / line_search                                                              romc.py:1910-2015
//     NDimBoundingBox.sample + the n1 n2 weight evaluations of RomcPosterior.sample                      posteriors.py:694-772
//     _sum_over_indicators / _sum_over_regions_indicators, BS n1 evaluations per density call            posteriors.py:498-554
//
// The objective.  Problem i is one row w (n_obs + 2 normals) of the handle's noise matrix, given by the caller or drawn
// here from the (seed, stream) pair of the problem: normals 0 .. n_obs + 1 of that stream, what
// elfihip_ma2_draw_distance_dev(seed, stream, n = 1) simulates from.  f_i(theta) = D D with D the distance of the fused MA2
// path (summaries.hip): x_k = (w[k+2] + t1 w[k+1]) + t2 w[k], S1 and S2 the lag-1 and lag-2 means in NumPy's pairwise order,
// D = sqrt((S1 - o1)^2 + (S2 - o2)^2), FMA contraction off -- bit for bit the square of what elfihip_ma2_distance_dev returns.
// The rule is D D, not pow(D, 2): the reference's float(d) ** 2 goes through libm's pow, which differs from d d
// in about one value of a thousand.
//
// One wavefront evaluates one objective: the row is loaded once into LDS and stays there for all of the wavefront's
// evaluations; per evaluation the 64 lanes form the n_obs values of x together, then each aligned group of eight lanes adds
// NumPy's eight interleaved accumulators a lane each (DPP combine), so every lane ends with the same bits.  The value is
// then read as a scalar, and everything that decides control flow -- the simplex, the function values, the counters of the
// line search -- is the same in all 64 lanes: the loops have no divergent exit.  A workgroup is one wavefront, so the
// barriers around the LDS row cost nothing and cannot wait for a wavefront that took another path.  Every loop is bounded:
// Nelder-Mead by maxiter and maxfev, the line search by K (rep_lim + 2) evaluations, the walks by their counts.
//
// The algorithms are stated in include/elfihip.h and, in NumPy, in tests/romc_ref.py.
#include "common.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <new>

#include "philox.hpp"

#pragma clang fp contract(off)

struct elfihip_romc {
  elfihip_ctx* ctx = nullptr;
  int model = 0;
  int64_t n1 = 0;
  int n_obs = 0;
  double obs1 = 0.0, obs2 = 0.0;
  double* W = nullptr;   // (n1, n_obs + 2) on the device, contiguous
};

namespace elfihip {

constexpr int RO_THREADS = 64;                            // one wavefront
constexpr int RO_MAX_L = ELFIHIP_ROMC_MAX_OBS + 2;        // 128: the longest row
constexpr int RO_MAX_K = 64;                              // refinements of the line search
constexpr int RO_MAX_REP = 1 << 20;                       // repetitions of one refinement
constexpr int RO_MAX_EVAL = 1 << 20;                      // the smaller of maxiter and maxfev

struct RoModel {
  const double* W;   // (n1, n_obs + 2)
  int64_t n1;
  int nobs;
  double o1, o2;
};

// the value lane 0 holds, as a scalar (every lane holds the same bits where this is used)
__device__ __forceinline__ double ro_uniform(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// the value lane `src` holds (src the same in every lane), as a scalar
__device__ __forceinline__ double ro_lane_double(double v, int src) {
  const int s = __builtin_amdgcn_readfirstlane(src);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), s), __builtin_amdgcn_readlane(__double2loint(v), s));
}
__device__ __forceinline__ int ro_lane_int(int v, int src) {
  return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(src));
}

__device__ __forceinline__ bool ro_finite(double v) { return v - v == 0.0; }

__device__ __forceinline__ void ro_load_row(const RoModel& M, int64_t i, double* s_w, int lane) {
  const int L = M.nobs + 2;
  __syncthreads();
  for (int k = lane; k < L; k += RO_THREADS) s_w[k] = M.W[i * L + k];
  __syncthreads();
}

// NumPy's pairwise sum of n <= 128 terms by an aligned group of eight lanes, lane j of it one accumulator (np_sum.hpp,
// summaries.hip's np_pairwise8): every lane of the group returns the same bits
template <class F>
__device__ __forceinline__ double ro_pairwise8(F f, int n, int j) {
  if (n < 8) {
    double r = 0.0;
    for (int i = 0; i < n; ++i) r += f(i);
    return r;
  }
  const int nfull = n - (n % 8);
  double r = f(j);
  for (int i = 8 + j; i < nfull; i += 8) r += f(i);
  r = lanes8_sum(r);
  for (int i = nfull; i < n; ++i) r += f(i);
  return r;
}

// f(theta) of the row in s_w, by the whole wavefront; s_x is its scratch
__device__ __forceinline__ double ro_objective(const RoModel& M, const double* s_w, double* s_x, double t1, double t2, int lane) {
  const int nobs = M.nobs;
  __syncthreads();                  // the x of the evaluation before has been read
  for (int i = lane; i < nobs; i += RO_THREADS) s_x[i] = (s_w[i + 2] + t1 * s_w[i + 1]) + t2 * s_w[i];
  __syncthreads();
  const int j = lane & 7;
  const double s1 = ro_pairwise8([&](int i) { return s_x[i + 1] * s_x[i]; }, nobs - 1, j) / (double)(nobs - 1);
  const double s2 = ro_pairwise8([&](int i) { return s_x[i + 2] * s_x[i]; }, nobs - 2, j) / (double)(nobs - 2);
  const double d1 = s1 - M.o1, d2 = s2 - M.o2;
  const double D = sqrt(d1 * d1 + d2 * d2);
  return ro_uniform(D * D);
}

// ---- the noise matrix from (seed, stream) pairs ---------------------------------------------------------------------------
__global__ __launch_bounds__(RO_THREADS) void ro_draw_kernel(const unsigned long long* __restrict__ seeds,
                                                             const unsigned long long* __restrict__ streams, int L,
                                                             double* __restrict__ W) {
  const int64_t i = blockIdx.x;
  const int p = threadIdx.x;
  if (2 * p >= L) return;
  double z0, z1;
  normal_pair(seeds[i], streams[i], (uint64_t)p, z0, z1);
  W[i * L + 2 * p] = z0;
  if (2 * p + 1 < L) W[i * L + 2 * p + 1] = z1;
}

// ---- objective: P pairs (theta, problem) ------------------------------------------------------------------------------------
struct RoObjArgs {
  RoModel M;
  int64_t P;
  const double* theta;   // (P, ldt)
  int64_t ldt;
  const long long* prob;  // (P)
  double* f;             // (P)
};

// wavefront i < n1 walks the pairs of problem i; wavefront n1 answers NaN for the pairs whose problem does not exist
__global__ __launch_bounds__(RO_THREADS) void ro_objective_kernel(RoObjArgs A) {
  __shared__ double s_w[RO_MAX_L], s_x[RO_MAX_L];
  const int lane = threadIdx.x;
  const int64_t me = blockIdx.x;
  if (me == A.M.n1) {
    for (int64_t p = lane; p < A.P; p += RO_THREADS) {
      const long long q = A.prob[p];
      if (q < 0 || q >= (long long)A.M.n1) A.f[p] = NAN;
    }
    return;
  }
  ro_load_row(A.M, me, s_w, lane);
  for (int64_t base = 0; base < A.P; base += RO_THREADS) {
    const int64_t p = base + lane;
    const bool mine = p < A.P && A.prob[p] == (long long)me;
    unsigned long long todo = __ballot(mine);
    if (todo == 0ull) continue;
    const double a = mine ? A.theta[p * A.ldt] : 0.0, b = mine ? A.theta[p * A.ldt + 1] : 0.0;
    double fv = 0.0;
    while (todo != 0ull) {
      const int k = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const double v = ro_objective(A.M, s_w, s_x, ro_lane_double(a, k), ro_lane_double(b, k), lane);
      if (lane == k) fv = v;
    }
    if (mine) A.f[p] = fv;
  }
}

// ---- solve: Nelder-Mead as scipy.optimize.minimize(method='Nelder-Mead') runs it, then the difference Hessian --------------
struct RoSolveArgs {
  RoModel M;
  const double* x0;   // (n1, ldx0)
  int64_t ldx0;
  int maxiter, maxfev;
  double* x_min;      // (n1, ldx)
  int64_t ldx;
  double* f_min;      // (n1)
  double* hess;       // (n1, 2, 2)
  int32_t *nfev, *nit, *status;
};

#define RO_SWAP(i, j)                        \
  do {                                       \
    double t_;                               \
    t_ = sa[i], sa[i] = sa[j], sa[j] = t_;   \
    t_ = sb[i], sb[i] = sb[j], sb[j] = t_;   \
    t_ = sf[i], sf[i] = sf[j], sf[j] = t_;   \
  } while (0)
// ascending, ties in order (an insertion sort of three)
#define RO_SORT3()                           \
  do {                                       \
    if (sf[1] < sf[0]) RO_SWAP(0, 1);        \
    if (sf[2] < sf[1]) {                     \
      RO_SWAP(1, 2);                         \
      if (sf[1] < sf[0]) RO_SWAP(0, 1);      \
    }                                        \
  } while (0)

__global__ __launch_bounds__(RO_THREADS) void ro_solve_kernel(RoSolveArgs A) {
  __shared__ double s_w[RO_MAX_L], s_x[RO_MAX_L];
  const int lane = threadIdx.x;
  const int64_t me = blockIdx.x;
  ro_load_row(A.M, me, s_w, lane);
  const double xa = ro_uniform(A.x0[me * A.ldx0]), xb = ro_uniform(A.x0[me * A.ldx0 + 1]);
  const double xatol = 1e-4, fatol = 1e-4;
  // the simplex (coordinates sa, sb) and its values, the same in every lane
  double sa[3] = {xa, xa != 0.0 ? (1.0 + 0.05) * xa : 0.00025, xa};
  double sb[3] = {xb, xb, xb != 0.0 ? (1.0 + 0.05) * xb : 0.00025};
  double sf[3] = {INFINITY, INFINITY, INFINITY};
  int fev = 0, it = 1;
  bool bad = false;          // a value that is not finite: the problem ends
  // an evaluation SciPy's wrapper would refuse (maxfev reached) returns false and leaves `out` alone
  auto eval = [&](double a, double b, double& out) -> bool {
    if (fev >= A.maxfev) return false;
    ++fev;
    out = ro_objective(A.M, s_w, s_x, a, b, lane);
    if (!ro_finite(out)) bad = true;
    return true;
  };
  bool go = eval(sa[0], sb[0], sf[0]);
  if (go && !bad) go = eval(sa[1], sb[1], sf[1]);
  if (go && !bad) go = eval(sa[2], sb[2], sf[2]);
  RO_SORT3();
  while (!bad && fev < A.maxfev && it < A.maxiter) {
    const double dx = fmax(fmax(fabs(sa[1] - sa[0]), fabs(sb[1] - sb[0])), fmax(fabs(sa[2] - sa[0]), fabs(sb[2] - sb[0])));
    const double df = fmax(fabs(sf[0] - sf[1]), fabs(sf[0] - sf[2]));
    if (dx <= xatol && df <= fatol) break;
    bool done = false;        // the iteration ran to its end (no evaluation was refused)
    do {
      const double ca = (sa[0] + sa[1]) / 2.0, cb = (sb[0] + sb[1]) / 2.0;     // the centroid of all but the worst
      const double ra = 2.0 * ca - 1.0 * sa[2], rb = 2.0 * cb - 1.0 * sb[2];   // reflection
      double fr = 0.0;
      if (!eval(ra, rb, fr) || bad) break;
      if (fr < sf[0]) {
        const double ea = 3.0 * ca - 2.0 * sa[2], eb = 3.0 * cb - 2.0 * sb[2];   // expansion
        double fe = 0.0;
        if (!eval(ea, eb, fe) || bad) break;
        if (fe < fr) {
          sa[2] = ea, sb[2] = eb, sf[2] = fe;
        } else {
          sa[2] = ra, sb[2] = rb, sf[2] = fr;
        }
      } else if (fr < sf[1]) {
        sa[2] = ra, sb[2] = rb, sf[2] = fr;
      } else {
        bool shrink = false;
        if (fr < sf[2]) {                                                        // contraction
          const double qa = 1.5 * ca - 0.5 * sa[2], qb = 1.5 * cb - 0.5 * sb[2];
          double fq = 0.0;
          if (!eval(qa, qb, fq) || bad) break;
          if (fq <= fr) {
            sa[2] = qa, sb[2] = qb, sf[2] = fq;
          } else {
            shrink = true;
          }
        } else {                                                                 // inside contraction
          const double qa = 0.5 * ca + 0.5 * sa[2], qb = 0.5 * cb + 0.5 * sb[2];
          double fq = 0.0;
          if (!eval(qa, qb, fq) || bad) break;
          if (fq < sf[2]) {
            sa[2] = qa, sb[2] = qb, sf[2] = fq;
          } else {
            shrink = true;
          }
        }
        if (shrink) {
          // (SciPy moves the vertex first and evaluates it then: a refused evaluation leaves the moved vertex with its old value)
          sa[1] = sa[0] + 0.5 * (sa[1] - sa[0]), sb[1] = sb[0] + 0.5 * (sb[1] - sb[0]);
          if (!eval(sa[1], sb[1], sf[1]) || bad) break;
          sa[2] = sa[0] + 0.5 * (sa[2] - sa[0]), sb[2] = sb[0] + 0.5 * (sb[2] - sb[0]);
          if (!eval(sa[2], sb[2], sf[2]) || bad) break;
        }
      }
      done = true;
    } while (false);
    if (done) ++it;
    RO_SORT3();
  }
  int st = ELFIHIP_ROMC_SOLVED;
  if (bad)
    st = ELFIHIP_ROMC_NONFINITE;
  else if (fev >= A.maxfev)
    st = ELFIHIP_ROMC_MAXFEV;
  else if (it >= A.maxiter)
    st = ELFIHIP_ROMC_MAXITER;
  double ma = sa[0], mb = sb[0], f0 = sf[0];
  double h00 = NAN, h01 = NAN, h11 = NAN;
  if (st == ELFIHIP_ROMC_SOLVED) {
    // central second differences with the steps h_k = 2^-13 max(1, |x_k|)
    const double ha = 0x1.0p-13 * fmax(1.0, fabs(ma)), hb = 0x1.0p-13 * fmax(1.0, fabs(mb));
    const double fpa = ro_objective(A.M, s_w, s_x, ma + ha, mb, lane), fma_ = ro_objective(A.M, s_w, s_x, ma - ha, mb, lane);
    const double fpb = ro_objective(A.M, s_w, s_x, ma, mb + hb, lane), fmb = ro_objective(A.M, s_w, s_x, ma, mb - hb, lane);
    const double fpp = ro_objective(A.M, s_w, s_x, ma + ha, mb + hb, lane), fpm = ro_objective(A.M, s_w, s_x, ma + ha, mb - hb, lane);
    const double fmp = ro_objective(A.M, s_w, s_x, ma - ha, mb + hb, lane), fmm = ro_objective(A.M, s_w, s_x, ma - ha, mb - hb, lane);
    h00 = ((fpa - f0) + (fma_ - f0)) / (ha * ha);
    h11 = ((fpb - f0) + (fmb - f0)) / (hb * hb);
    h01 = ((fpp - fpm) - (fmp - fmm)) / ((4.0 * ha) * hb);
  } else if (st == ELFIHIP_ROMC_NONFINITE) {
    ma = mb = f0 = NAN;
  }
  if (lane == 0) {
    A.x_min[me * A.ldx] = ma;
    A.x_min[me * A.ldx + 1] = mb;
    A.f_min[me] = f0;
    A.hess[me * 4] = h00;
    A.hess[me * 4 + 1] = h01;
    A.hess[me * 4 + 2] = h01;
    A.hess[me * 4 + 3] = h11;
    A.nfev[me] = fev;
    A.nit[me] = it;
    A.status[me] = st;
  }
}

// ---- regions: the rotation from the Hessian, one line search per (region, direction, side) ---------------------------------
// One cyclic Jacobi sweep of the symmetric part of H -- for two dimensions one rotation, which annihilates the off-diagonal
// entry -- with + - x / sqrt only; the columns of V are the eigenvectors.  The identity when H is not finite or has no full
// rank by NumPy's matrix_rank rule, min |lambda| <= max |lambda| D eps.
__device__ __forceinline__ void ro_rotation(double h00, double h01, double h10, double h11, double V[4]) {
  const bool fin = ro_finite(h00) && ro_finite(h01) && ro_finite(h10) && ro_finite(h11);
  double a = h00, d = h11;
  const double b = (h01 + h10) * 0.5;
  double v00 = 1.0, v01 = 0.0, v10 = 0.0, v11 = 1.0;
  if (fin && b != 0.0) {
    const double tau = (d - a) / (2.0 * b);
    const double root = sqrt(1.0 + tau * tau);
    const double t = tau >= 0.0 ? 1.0 / (tau + root) : -1.0 / (-tau + root);
    const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
    a = a - t * b;
    d = d + t * b;
    v00 = c, v10 = -s, v01 = s, v11 = c;
  }
  const double la = fabs(a), ld = fabs(d);
  const double mn = la < ld ? la : ld, mx = la < ld ? ld : la;
  if (!fin || !ro_finite(a) || !ro_finite(d) || mn <= mx * (double)ELFIHIP_ROMC_DIM * DBL_EPSILON) v00 = 1.0, v01 = 0.0, v10 = 0.0, v11 = 1.0;
  V[0] = v00, V[1] = v01, V[2] = v10, V[3] = v11;
}

struct RoRegionArgs {
  RoModel M;
  int64_t R;
  const long long* prob;   // (R)
  const double* centre;    // (R, 2)
  const double* hess;      // (R, 2, 2)
  double eps, eta;
  int K, rep_lim;
  double* rotation;        // (R, 2, 2)
  double* limits;          // (R, 2, 2): [direction][left, right]
  int32_t* nfev;           // (R, 2, 2)
};

__global__ __launch_bounds__(RO_THREADS) void ro_region_kernel(RoRegionArgs A) {
  __shared__ double s_w[RO_MAX_L], s_x[RO_MAX_L];
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x >> 2;
  const int d = (blockIdx.x >> 1) & 1, side = blockIdx.x & 1;
  const long long q = A.prob[r];
  const int64_t slot = r * 4 + d * 2 + side;
  if (q < 0 || q >= (long long)A.M.n1) {       // (the same in every lane)
    if (lane == 0) {
      A.limits[slot] = NAN;
      A.nfev[slot] = 0;
      if (d == 0 && side == 0)
        for (int k = 0; k < 4; ++k) A.rotation[r * 4 + k] = NAN;
    }
    return;
  }
  ro_load_row(A.M, q, s_w, lane);
  double V[4];
  ro_rotation(ro_uniform(A.hess[r * 4]), ro_uniform(A.hess[r * 4 + 1]), ro_uniform(A.hess[r * 4 + 2]), ro_uniform(A.hess[r * 4 + 3]), V);
  if (lane == 0 && d == 0 && side == 0)
    for (int k = 0; k < 4; ++k) A.rotation[r * 4 + k] = V[k];
  // the reference's line_search (romc.py:1971-2015), operation for operation, along +- column d
  const double va = side ? V[d] : -V[d], vb = side ? V[2 + d] : -V[2 + d];
  double ta = ro_uniform(A.centre[r * 2]), tb = ro_uniform(A.centre[r * 2 + 1]);
  double offset = 0.0, eta = A.eta;
  int evals = 0;
  for (int i = 0; i < A.K; ++i) {
    int rep = 0;
    for (;;) {                      // (at most rep_lim + 2 evaluations)
      const double fv = ro_objective(A.M, s_w, s_x, ta, tb, lane);
      ++evals;
      if (!(fv < A.eps && rep <= A.rep_lim)) break;
      ta += eta * va;
      tb += eta * vb;
      offset += eta;
      ++rep;
    }
    ta -= eta * va;
    tb -= eta * vb;
    offset -= eta;
    if (rep > A.rep_lim) break;
    eta = eta / 2.0;
  }
  if (offset <= 0.0) offset = eta;
  if (lane == 0) {
    A.limits[slot] = side ? offset : -offset;
    A.nfev[slot] = evals;
  }
}

// ---- sample: n2 points per region, uniform in its box ------------------------------------------------------------------------
struct RoSampleArgs {
  RoModel M;
  int64_t R, n2;
  const long long* prob;
  const double *centre, *rotation, *limits;
  uint64_t seed, stream;
  double* theta;   // (R, n2, ldth)
  int64_t ldth;
  double* f;       // (R, n2)
};

__global__ __launch_bounds__(RO_THREADS) void ro_sample_kernel(RoSampleArgs A) {
  __shared__ double s_w[RO_MAX_L], s_x[RO_MAX_L];
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x;
  const long long q = A.prob[r];
  const bool exists = q >= 0 && q < (long long)A.M.n1;    // (the same in every lane)
  if (exists) ro_load_row(A.M, q, s_w, lane);
  const double c0 = A.centre[r * 2], c1 = A.centre[r * 2 + 1];
  const double r00 = A.rotation[r * 4], r01 = A.rotation[r * 4 + 1], r10 = A.rotation[r * 4 + 2], r11 = A.rotation[r * 4 + 3];
  const double l0 = A.limits[r * 4], w0 = A.limits[r * 4 + 1] - l0, l1 = A.limits[r * 4 + 2], w1 = A.limits[r * 4 + 3] - l1;
  for (int64_t base = 0; base < A.n2; base += RO_THREADS) {
    const int64_t j = base + lane;
    const double t0 = uniform53_first(A.seed, A.stream + (uint64_t)r, 2ull * (uint64_t)j) * w0 + l0;
    const double t1 = uniform53_first(A.seed, A.stream + (uint64_t)r, 2ull * (uint64_t)j + 1ull) * w1 + l1;
    const double a = (r00 * t0 + r01 * t1) + c0, b = (r10 * t0 + r11 * t1) + c1;
    const int cnt = (int)(A.n2 - base < RO_THREADS ? A.n2 - base : RO_THREADS);
    double fv = NAN;
    if (exists)
      for (int k = 0; k < cnt; ++k) {
        const double v = ro_objective(A.M, s_w, s_x, ro_lane_double(a, k), ro_lane_double(b, k), lane);
        if (lane == k) fv = v;
      }
    if (j < A.n2) {
      double* out = A.theta + (r * A.n2 + j) * A.ldth;
      out[0] = a;
      out[1] = b;
      A.f[r * A.n2 + j] = fv;
    }
  }
}

// ---- count: count[b] = sum over the regions of 1[f_r(theta_b) <= eps] (and theta_b in box r) -----------------------------------
struct RoCountArgs {
  RoModel M;
  int64_t BS, R, chunks;
  const double* theta;   // (BS, ldt)
  int64_t ldt;
  const long long* prob;
  double eps;
  int contain;
  const double *centre, *rotation_inv, *limits;
  int32_t* count;        // (BS), zero at launch
};

// one wavefront per (region, 64 points): the integer adds of the wavefronts commute, the counts do not depend on scheduling
__global__ __launch_bounds__(RO_THREADS) void ro_count_kernel(RoCountArgs A) {
  __shared__ double s_w[RO_MAX_L], s_x[RO_MAX_L];
  const int lane = threadIdx.x;
  const int64_t r = blockIdx.x / A.chunks, base = (blockIdx.x - r * A.chunks) * RO_THREADS;
  const long long q = A.prob[r];
  if (q < 0 || q >= (long long)A.M.n1) return;      // (the same in every lane)
  ro_load_row(A.M, q, s_w, lane);
  const int64_t p = base + lane;
  const bool live = p < A.BS;
  const double a = live ? A.theta[p * A.ldt] : 0.0, b = live ? A.theta[p * A.ldt + 1] : 0.0;
  int inside = live ? 1 : 0;
  if (A.contain) {
    // NDimBoundingBox.contains: R^-1 p + R^-1 (-c) within the limits, both ends included
    const double c0 = A.centre[r * 2], c1 = A.centre[r * 2 + 1];
    const double* ri = A.rotation_inv + r * 4;
    const double* lim = A.limits + r * 4;
    const double y0 = (ri[0] * a + ri[1] * b) + (ri[0] * -c0 + ri[1] * -c1);
    const double y1 = (ri[2] * a + ri[3] * b) + (ri[2] * -c0 + ri[3] * -c1);
    if (y0 < lim[0] || y0 > lim[1] || y1 < lim[2] || y1 > lim[3]) inside = 0;
  }
  const int cnt = (int)(A.BS - base < RO_THREADS ? A.BS - base : RO_THREADS);
  int hit = 0;
  for (int k = 0; k < cnt; ++k) {
    if (ro_lane_int(inside, k) == 0) continue;      // (a scalar: outside the box, no evaluation)
    const double v = ro_objective(A.M, s_w, s_x, ro_lane_double(a, k), ro_lane_double(b, k), lane);
    if (lane == k && v <= A.eps) hit = 1;
  }
  if (hit) atomicAdd(&A.count[p], 1);
}

// ---- launches -----------------------------------------------------------------------------------------------------------------
static inline RoModel ro_model(const elfihip_romc* h) {
  RoModel M;
  M.W = h->W;
  M.n1 = h->n1;
  M.nobs = h->n_obs;
  M.o1 = h->obs1;
  M.o2 = h->obs2;
  return M;
}

static int ro_objective_impl(elfihip_romc* h, int64_t P, const double* dtheta, int64_t ldt, const int64_t* dprob, double* df) {
  elfihip_ctx* ctx = h->ctx;
  ELFIHIP_REQUIRE(ctx, P >= 0, "bad number of pairs P=%lld", (long long)P);
  if (P == 0) return ELFIHIP_OK;
  ELFIHIP_REQUIRE(ctx, dtheta && dprob && df, "NULL pointer");
  ELFIHIP_REQUIRE(ctx, ldt >= ELFIHIP_ROMC_DIM, "leading dimension below the row length");
  RoObjArgs A;
  A.M = ro_model(h);
  A.P = P;
  A.theta = dtheta;
  A.ldt = ldt;
  A.prob = reinterpret_cast<const long long*>(dprob);
  A.f = df;
  hipLaunchKernelGGL(ro_objective_kernel, dim3((unsigned)(h->n1 + 1)), dim3(RO_THREADS), 0, ctx->stream, A);
  return launch_status(ctx, "ro_objective_kernel");
}

static int ro_limits_check(elfihip_ctx* ctx, int maxiter, int maxfev) {
  ELFIHIP_REQUIRE(ctx, maxiter >= 1 && maxfev >= 1, "maxiter=%d, maxfev=%d: at least 1 each", maxiter, maxfev);
  ELFIHIP_REQUIRE(ctx, std::min(maxiter, maxfev) <= RO_MAX_EVAL, "the smaller of maxiter=%d and maxfev=%d bounds the search: up to %d",
                  maxiter, maxfev, RO_MAX_EVAL);
  return ELFIHIP_OK;
}

static int ro_solve_impl(elfihip_romc* h, const double* dx0, int64_t ldx0, int maxiter, int maxfev, double* dx_min, int64_t ldx,
                         double* df_min, double* dhess, int32_t* dnfev, int32_t* dnit, int32_t* dstatus) {
  elfihip_ctx* ctx = h->ctx;
  ELFIHIP_TRY(ro_limits_check(ctx, maxiter, maxfev));
  ELFIHIP_REQUIRE(ctx, dx0 && dx_min && df_min && dhess && dnfev && dnit && dstatus, "NULL pointer");
  ELFIHIP_REQUIRE(ctx, ldx0 >= ELFIHIP_ROMC_DIM && ldx >= ELFIHIP_ROMC_DIM, "leading dimension below the row length");
  RoSolveArgs A;
  A.M = ro_model(h);
  A.x0 = dx0;
  A.ldx0 = ldx0;
  A.maxiter = maxiter;
  A.maxfev = maxfev;
  A.x_min = dx_min;
  A.ldx = ldx;
  A.f_min = df_min;
  A.hess = dhess;
  A.nfev = dnfev;
  A.nit = dnit;
  A.status = dstatus;
  hipLaunchKernelGGL(ro_solve_kernel, dim3((unsigned)h->n1), dim3(RO_THREADS), 0, ctx->stream, A);
  return launch_status(ctx, "ro_solve_kernel");
}

static int ro_region_check(elfihip_ctx* ctx, int64_t R) {
  ELFIHIP_REQUIRE(ctx, R >= 0 && R <= ELFIHIP_ROMC_MAX_PROBLEMS, "bad number of regions R=%lld: up to %d", (long long)R,
                  ELFIHIP_ROMC_MAX_PROBLEMS);
  return ELFIHIP_OK;
}

static int ro_search_check(elfihip_ctx* ctx, double eps_region, int K, double eta, int rep_lim) {
  ELFIHIP_REQUIRE(ctx, K >= 1 && K <= RO_MAX_K, "K=%d refinements: 1 to %d", K, RO_MAX_K);
  ELFIHIP_REQUIRE(ctx, rep_lim >= 0 && rep_lim <= RO_MAX_REP, "rep_lim=%d: 0 to %d", rep_lim, RO_MAX_REP);
  ELFIHIP_REQUIRE(ctx, eta > 0.0 && eta < INFINITY, "the step eta must be positive and finite");
  ELFIHIP_REQUIRE(ctx, eps_region == eps_region, "eps_region is NaN");
  return ELFIHIP_OK;
}

static int ro_regions_impl(elfihip_romc* h, int64_t R, const int64_t* dprob, const double* dcentre, const double* dhess,
                           double eps_region, int K, double eta, int rep_lim, double* drotation, double* dlimits, int32_t* dnfev) {
  elfihip_ctx* ctx = h->ctx;
  ELFIHIP_TRY(ro_region_check(ctx, R));
  ELFIHIP_TRY(ro_search_check(ctx, eps_region, K, eta, rep_lim));
  if (R == 0) return ELFIHIP_OK;
  ELFIHIP_REQUIRE(ctx, dprob && dcentre && dhess && drotation && dlimits && dnfev, "NULL pointer");
  RoRegionArgs A;
  A.M = ro_model(h);
  A.R = R;
  A.prob = reinterpret_cast<const long long*>(dprob);
  A.centre = dcentre;
  A.hess = dhess;
  A.eps = eps_region;
  A.eta = eta;
  A.K = K;
  A.rep_lim = rep_lim;
  A.rotation = drotation;
  A.limits = dlimits;
  A.nfev = dnfev;
  hipLaunchKernelGGL(ro_region_kernel, dim3((unsigned)(R * 4)), dim3(RO_THREADS), 0, ctx->stream, A);
  return launch_status(ctx, "ro_region_kernel");
}

static int ro_sample_impl(elfihip_romc* h, int64_t R, const int64_t* dprob, const double* dcentre, const double* drotation,
                          const double* dlimits, int64_t n2, uint64_t seed, uint64_t stream, double* dtheta, int64_t ldth, double* df) {
  elfihip_ctx* ctx = h->ctx;
  ELFIHIP_TRY(ro_region_check(ctx, R));
  ELFIHIP_REQUIRE(ctx, n2 >= 0 && n2 <= ELFIHIP_ROMC_MAX_POINTS, "n2=%lld points per region: up to %d", (long long)n2, ELFIHIP_ROMC_MAX_POINTS);
  if (R == 0 || n2 == 0) return ELFIHIP_OK;
  ELFIHIP_REQUIRE(ctx, dprob && dcentre && drotation && dlimits && dtheta && df, "NULL pointer");
  ELFIHIP_REQUIRE(ctx, ldth >= ELFIHIP_ROMC_DIM, "leading dimension below the row length");
  RoSampleArgs A;
  A.M = ro_model(h);
  A.R = R;
  A.n2 = n2;
  A.prob = reinterpret_cast<const long long*>(dprob);
  A.centre = dcentre;
  A.rotation = drotation;
  A.limits = dlimits;
  A.seed = seed;
  A.stream = stream;
  A.theta = dtheta;
  A.ldth = ldth;
  A.f = df;
  hipLaunchKernelGGL(ro_sample_kernel, dim3((unsigned)R), dim3(RO_THREADS), 0, ctx->stream, A);
  return launch_status(ctx, "ro_sample_kernel");
}

static int ro_count_impl(elfihip_romc* h, int64_t BS, const double* dtheta, int64_t ldt, int64_t R, const int64_t* dprob, double eps,
                         int contain, const double* dcentre, const double* drotation_inv, const double* dlimits, int32_t* dcount) {
  elfihip_ctx* ctx = h->ctx;
  ELFIHIP_TRY(ro_region_check(ctx, R));
  ELFIHIP_REQUIRE(ctx, BS >= 0 && BS <= ELFIHIP_ROMC_MAX_POINTS, "BS=%lld points: up to %d", (long long)BS, ELFIHIP_ROMC_MAX_POINTS);
  ELFIHIP_REQUIRE(ctx, contain == 0 || contain == 1, "the containment flag is 0 or 1");
  if (BS == 0) return ELFIHIP_OK;
  ELFIHIP_REQUIRE(ctx, dtheta && dcount && (R == 0 || dprob), "NULL pointer");
  ELFIHIP_REQUIRE(ctx, !contain || R == 0 || (dcentre && drotation_inv && dlimits), "containment needs the boxes");
  ELFIHIP_REQUIRE(ctx, ldt >= ELFIHIP_ROMC_DIM, "leading dimension below the row length");
  ELFIHIP_CHECK_HIP(ctx, hipMemsetAsync(dcount, 0, (size_t)BS * sizeof(int32_t), ctx->stream));
  if (R == 0) return ELFIHIP_OK;
  RoCountArgs A;
  A.M = ro_model(h);
  A.BS = BS;
  A.R = R;
  A.chunks = (BS + RO_THREADS - 1) / RO_THREADS;
  ELFIHIP_REQUIRE(ctx, A.chunks * R <= (int64_t)0x7fffffff, "%lld points x %lld regions: too many for one launch", (long long)BS, (long long)R);
  A.theta = dtheta;
  A.ldt = ldt;
  A.prob = reinterpret_cast<const long long*>(dprob);
  A.eps = eps;
  A.contain = contain;
  A.centre = dcentre;
  A.rotation_inv = drotation_inv;
  A.limits = dlimits;
  A.count = dcount;
  hipLaunchKernelGGL(ro_count_kernel, dim3((unsigned)(A.chunks * R)), dim3(RO_THREADS), 0, ctx->stream, A);
  return launch_status(ctx, "ro_count_kernel");
}

// the host forms answer a problem index that does not exist with an error (the _dev forms, which cannot look, with NaN)
static int ro_index_check(elfihip_romc* h, const int64_t* prob, int64_t n) {
  for (int64_t k = 0; k < n; ++k)
    ELFIHIP_REQUIRE(h->ctx, prob[k] >= 0 && prob[k] < h->n1, "problem index %lld at position %lld: the handle has %lld problems",
                    (long long)prob[k], (long long)k, (long long)h->n1);
  return ELFIHIP_OK;
}

// staging: pieces of one device buffer, each aligned to 256 bytes
struct RoCarve {
  char* base = nullptr;
  size_t used = 0;
  size_t add(size_t bytes) {
    const size_t at = used;
    used += (bytes + 255) & ~(size_t)255;
    return at;
  }
  template <class T>
  T* at(size_t off) const {
    return reinterpret_cast<T*>(base + off);
  }
};

static int ro_create_check(elfihip_ctx* ctx, int model, int64_t n1, int n_obs, double obs1, double obs2, bool given, bool drawn) {
  ELFIHIP_REQUIRE(ctx, model == ELFIHIP_ROMC_MA2, "model %d: ELFIHIP_ROMC_MA2 is the one model", model);
  ELFIHIP_REQUIRE(ctx, n1 >= 1 && n1 <= ELFIHIP_ROMC_MAX_PROBLEMS, "n1=%lld problems: 1 to %d", (long long)n1, ELFIHIP_ROMC_MAX_PROBLEMS);
  ELFIHIP_REQUIRE(ctx, n_obs >= 3 && n_obs <= ELFIHIP_ROMC_MAX_OBS, "n_obs=%d: 3 to %d", n_obs, ELFIHIP_ROMC_MAX_OBS);
  ELFIHIP_REQUIRE(ctx, obs1 - obs1 == 0.0 && obs2 - obs2 == 0.0, "the observed summaries must be finite");
  ELFIHIP_REQUIRE(ctx, given != drawn, "give either the noise matrix or the (seed, stream) pairs");
  return ELFIHIP_OK;
}

static int ro_alloc(elfihip_ctx* ctx, int model, int64_t n1, int n_obs, double obs1, double obs2, elfihip_romc** out) {
  elfihip_romc* h = new (std::nothrow) elfihip_romc();
  if (!h) return fail(ctx, ELFIHIP_ERR_NOMEM, "out of host memory");
  h->ctx = ctx;
  h->model = model;
  h->n1 = n1;
  h->n_obs = n_obs;
  h->obs1 = obs1;
  h->obs2 = obs2;
  void* p = nullptr;
  const hipError_t e = hipMalloc(&p, (size_t)n1 * (size_t)(n_obs + 2) * sizeof(double));
  if (e != hipSuccess) {
    delete h;
    return fail(ctx, ELFIHIP_ERR_NOMEM, "the noise matrix could not be allocated: %s", hipGetErrorString(e));
  }
  h->W = reinterpret_cast<double*>(p);
  *out = h;
  return ELFIHIP_OK;
}

static int ro_draw(elfihip_romc* h, const uint64_t* dseeds, const uint64_t* dstreams) {
  elfihip_ctx* ctx = h->ctx;
  hipLaunchKernelGGL(ro_draw_kernel, dim3((unsigned)h->n1), dim3(RO_THREADS), 0, ctx->stream,
                     reinterpret_cast<const unsigned long long*>(dseeds), reinterpret_cast<const unsigned long long*>(dstreams),
                     h->n_obs + 2, h->W);
  return launch_status(ctx, "ro_draw_kernel");
}

static void ro_release(elfihip_romc* h) {
  if (h->W) (void)hipFree(h->W);
  delete h;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_romc_create_dev(elfihip_ctx* ctx, int model, int64_t n1, int n_obs, double obs1, double obs2, const double* dW,
                            int64_t ldw, const uint64_t* dseeds, const uint64_t* dstreams, elfihip_romc** out) {
  if (!ctx || !out) return fail(ctx, ELFIHIP_ERR_ARG, "NULL argument");
  *out = nullptr;
  ELFIHIP_TRY(ro_create_check(ctx, model, n1, n_obs, obs1, obs2, dW != nullptr, dseeds != nullptr && dstreams != nullptr));
  ELFIHIP_REQUIRE(ctx, !dW || (!dseeds && !dstreams), "give either the noise matrix or the (seed, stream) pairs");
  ELFIHIP_REQUIRE(ctx, !dW || ldw >= n_obs + 2, "leading dimension below the row length");
  DeviceGuard g(ctx->device);
  elfihip_romc* h = nullptr;
  ELFIHIP_TRY(ro_alloc(ctx, model, n1, n_obs, obs1, obs2, &h));
  const size_t row = (size_t)(n_obs + 2) * sizeof(double);
  int rc = ELFIHIP_OK;
  if (dW) {
    const hipError_t e = hipMemcpy2DAsync(h->W, row, dW, (size_t)ldw * sizeof(double), row, (size_t)n1, hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) rc = fail(ctx, ELFIHIP_ERR_HIP, "the copy of the noise matrix failed: %s", hipGetErrorString(e));
  } else {
    rc = ro_draw(h, dseeds, dstreams);
  }
  if (rc != ELFIHIP_OK) {
    ro_release(h);
    return rc;
  }
  *out = h;
  return ELFIHIP_OK;
}

int elfihip_romc_create(elfihip_ctx* ctx, int model, int64_t n1, int n_obs, double obs1, double obs2, const double* W,
                        const uint64_t* seeds, const uint64_t* streams, elfihip_romc** out) {
  if (!ctx || !out) return fail(ctx, ELFIHIP_ERR_ARG, "NULL argument");
  *out = nullptr;
  ELFIHIP_TRY(ro_create_check(ctx, model, n1, n_obs, obs1, obs2, W != nullptr, seeds != nullptr && streams != nullptr));
  ELFIHIP_REQUIRE(ctx, !W || (!seeds && !streams), "give either the noise matrix or the (seed, stream) pairs");
  DeviceGuard g(ctx->device);
  elfihip_romc* h = nullptr;
  ELFIHIP_TRY(ro_alloc(ctx, model, n1, n_obs, obs1, obs2, &h));
  auto body = [&]() -> int {
    if (W) {
      ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(h->W, W, (size_t)n1 * (size_t)(n_obs + 2) * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    } else {
      const size_t nb = (size_t)n1 * sizeof(uint64_t);
      RoCarve in;
      const size_t o_seed = in.add(nb), o_stream = in.add(nb);
      ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(in.used));
      in.base = ctx->in.as<char>();
      ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<uint64_t>(o_seed), seeds, nb, hipMemcpyHostToDevice, ctx->stream));
      ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<uint64_t>(o_stream), streams, nb, hipMemcpyHostToDevice, ctx->stream));
      ELFIHIP_TRY(ro_draw(h, in.at<uint64_t>(o_seed), in.at<uint64_t>(o_stream)));
    }
    ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ELFIHIP_OK;
  };
  const int rc = body();
  if (rc != ELFIHIP_OK) {
    ro_release(h);
    return rc;
  }
  *out = h;
  return ELFIHIP_OK;
}

int elfihip_romc_free(elfihip_romc* h) {
  if (!h) return ELFIHIP_OK;
  DeviceGuard g(h->ctx->device);
  (void)hipStreamSynchronize(h->ctx->stream);
  ro_release(h);
  return ELFIHIP_OK;
}

int elfihip_romc_objective_dev(elfihip_romc* h, int64_t P, const double* dtheta, int64_t ldt, const int64_t* dprob, double* df) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "the handle is NULL");
  DeviceGuard g(h->ctx->device);
  return ro_objective_impl(h, P, dtheta, ldt, dprob, df);
}

int elfihip_romc_objective(elfihip_romc* h, int64_t P, const double* theta, const int64_t* prob, double* f) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "the handle is NULL");
  elfihip_ctx* ctx = h->ctx;
  ELFIHIP_REQUIRE(ctx, P >= 0, "bad number of pairs P=%lld", (long long)P);
  if (P == 0) return ELFIHIP_OK;
  ELFIHIP_REQUIRE(ctx, theta && prob && f, "NULL pointer");
  ELFIHIP_TRY(ro_index_check(h, prob, P));
  DeviceGuard g(ctx->device);
  const size_t n = (size_t)P;
  RoCarve in, out;
  const size_t o_t = in.add(n * 2 * sizeof(double)), o_p = in.add(n * sizeof(int64_t));
  const size_t o_f = out.add(n * sizeof(double));
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(in.used));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(out.used));
  in.base = ctx->in.as<char>();
  out.base = ctx->out.as<char>();
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_t), theta, n * 2 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<int64_t>(o_p), prob, n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(ro_objective_impl(h, P, in.at<double>(o_t), 2, in.at<int64_t>(o_p), out.at<double>(o_f)));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(f, out.at<double>(o_f), n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_romc_solve_dev(elfihip_romc* h, const double* dx0, int64_t ldx0, int maxiter, int maxfev, double* dx_min, int64_t ldx,
                           double* df_min, double* dhess, int32_t* dnfev, int32_t* dnit, int32_t* dstatus) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "the handle is NULL");
  DeviceGuard g(h->ctx->device);
  return ro_solve_impl(h, dx0, ldx0, maxiter, maxfev, dx_min, ldx, df_min, dhess, dnfev, dnit, dstatus);
}

int elfihip_romc_solve(elfihip_romc* h, const double* x0, int maxiter, int maxfev, double* x_min, double* f_min, double* hess,
                       int32_t* nfev, int32_t* nit, int32_t* status) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "the handle is NULL");
  elfihip_ctx* ctx = h->ctx;
  ELFIHIP_TRY(ro_limits_check(ctx, maxiter, maxfev));
  ELFIHIP_REQUIRE(ctx, x0 && x_min && f_min && hess && nfev && nit && status, "NULL pointer");
  DeviceGuard g(ctx->device);
  const size_t n = (size_t)h->n1, pd = sizeof(double), pi = sizeof(int32_t);
  RoCarve in, out;
  const size_t o_x0 = in.add(n * 2 * pd);
  const size_t o_x = out.add(n * 2 * pd), o_f = out.add(n * pd), o_h = out.add(n * 4 * pd), o_e = out.add(n * pi), o_i = out.add(n * pi),
               o_s = out.add(n * pi);
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(in.used));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(out.used));
  in.base = ctx->in.as<char>();
  out.base = ctx->out.as<char>();
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_x0), x0, n * 2 * pd, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(ro_solve_impl(h, in.at<double>(o_x0), 2, maxiter, maxfev, out.at<double>(o_x), 2, out.at<double>(o_f), out.at<double>(o_h),
                            out.at<int32_t>(o_e), out.at<int32_t>(o_i), out.at<int32_t>(o_s)));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(x_min, out.at<double>(o_x), n * 2 * pd, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(f_min, out.at<double>(o_f), n * pd, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(hess, out.at<double>(o_h), n * 4 * pd, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(nfev, out.at<int32_t>(o_e), n * pi, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(nit, out.at<int32_t>(o_i), n * pi, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(status, out.at<int32_t>(o_s), n * pi, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_romc_regions_dev(elfihip_romc* h, int64_t R, const int64_t* dprob, const double* dcentre, const double* dhess,
                             double eps_region, int K, double eta, int rep_lim, double* drotation, double* dlimits, int32_t* dnfev) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "the handle is NULL");
  DeviceGuard g(h->ctx->device);
  return ro_regions_impl(h, R, dprob, dcentre, dhess, eps_region, K, eta, rep_lim, drotation, dlimits, dnfev);
}

int elfihip_romc_regions(elfihip_romc* h, int64_t R, const int64_t* prob, const double* centre, const double* hess, double eps_region,
                         int K, double eta, int rep_lim, double* rotation, double* limits, int32_t* nfev) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "the handle is NULL");
  elfihip_ctx* ctx = h->ctx;
  ELFIHIP_TRY(ro_region_check(ctx, R));
  ELFIHIP_TRY(ro_search_check(ctx, eps_region, K, eta, rep_lim));
  if (R == 0) return ELFIHIP_OK;
  ELFIHIP_REQUIRE(ctx, prob && centre && hess && rotation && limits && nfev, "NULL pointer");
  ELFIHIP_TRY(ro_index_check(h, prob, R));
  DeviceGuard g(ctx->device);
  const size_t n = (size_t)R, pd = sizeof(double);
  RoCarve in, out;
  const size_t o_p = in.add(n * sizeof(int64_t)), o_c = in.add(n * 2 * pd), o_h = in.add(n * 4 * pd);
  const size_t o_r = out.add(n * 4 * pd), o_l = out.add(n * 4 * pd), o_e = out.add(n * 4 * sizeof(int32_t));
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(in.used));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(out.used));
  in.base = ctx->in.as<char>();
  out.base = ctx->out.as<char>();
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<int64_t>(o_p), prob, n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_c), centre, n * 2 * pd, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_h), hess, n * 4 * pd, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(ro_regions_impl(h, R, in.at<int64_t>(o_p), in.at<double>(o_c), in.at<double>(o_h), eps_region, K, eta, rep_lim,
                              out.at<double>(o_r), out.at<double>(o_l), out.at<int32_t>(o_e)));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(rotation, out.at<double>(o_r), n * 4 * pd, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(limits, out.at<double>(o_l), n * 4 * pd, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(nfev, out.at<int32_t>(o_e), n * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_romc_sample_dev(elfihip_romc* h, int64_t R, const int64_t* dprob, const double* dcentre, const double* drotation,
                            const double* dlimits, int64_t n2, uint64_t seed, uint64_t stream, double* dtheta, int64_t ldth, double* df) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "the handle is NULL");
  DeviceGuard g(h->ctx->device);
  return ro_sample_impl(h, R, dprob, dcentre, drotation, dlimits, n2, seed, stream, dtheta, ldth, df);
}

int elfihip_romc_sample(elfihip_romc* h, int64_t R, const int64_t* prob, const double* centre, const double* rotation,
                        const double* limits, int64_t n2, uint64_t seed, uint64_t stream, double* theta, double* f) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "the handle is NULL");
  elfihip_ctx* ctx = h->ctx;
  ELFIHIP_TRY(ro_region_check(ctx, R));
  ELFIHIP_REQUIRE(ctx, n2 >= 0 && n2 <= ELFIHIP_ROMC_MAX_POINTS, "n2=%lld points per region: up to %d", (long long)n2, ELFIHIP_ROMC_MAX_POINTS);
  if (R == 0 || n2 == 0) return ELFIHIP_OK;
  ELFIHIP_REQUIRE(ctx, prob && centre && rotation && limits && theta && f, "NULL pointer");
  ELFIHIP_TRY(ro_index_check(h, prob, R));
  DeviceGuard g(ctx->device);
  const size_t n = (size_t)R, m = n * (size_t)n2, pd = sizeof(double);
  RoCarve in, out;
  const size_t o_p = in.add(n * sizeof(int64_t)), o_c = in.add(n * 2 * pd), o_r = in.add(n * 4 * pd), o_l = in.add(n * 4 * pd);
  const size_t o_t = out.add(m * 2 * pd), o_f = out.add(m * pd);
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(in.used));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(out.used));
  in.base = ctx->in.as<char>();
  out.base = ctx->out.as<char>();
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<int64_t>(o_p), prob, n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_c), centre, n * 2 * pd, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_r), rotation, n * 4 * pd, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_l), limits, n * 4 * pd, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(ro_sample_impl(h, R, in.at<int64_t>(o_p), in.at<double>(o_c), in.at<double>(o_r), in.at<double>(o_l), n2, seed, stream,
                             out.at<double>(o_t), 2, out.at<double>(o_f)));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(theta, out.at<double>(o_t), m * 2 * pd, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(f, out.at<double>(o_f), m * pd, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_romc_count_dev(elfihip_romc* h, int64_t BS, const double* dtheta, int64_t ldt, int64_t R, const int64_t* dprob, double eps,
                           int contain, const double* dcentre, const double* drotation_inv, const double* dlimits, int32_t* dcount) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "the handle is NULL");
  DeviceGuard g(h->ctx->device);
  return ro_count_impl(h, BS, dtheta, ldt, R, dprob, eps, contain, dcentre, drotation_inv, dlimits, dcount);
}

int elfihip_romc_count(elfihip_romc* h, int64_t BS, const double* theta, int64_t R, const int64_t* prob, double eps, int contain,
                       const double* centre, const double* rotation_inv, const double* limits, int32_t* count) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "the handle is NULL");
  elfihip_ctx* ctx = h->ctx;
  ELFIHIP_TRY(ro_region_check(ctx, R));
  ELFIHIP_REQUIRE(ctx, BS >= 0 && BS <= ELFIHIP_ROMC_MAX_POINTS, "BS=%lld points: up to %d", (long long)BS, ELFIHIP_ROMC_MAX_POINTS);
  ELFIHIP_REQUIRE(ctx, contain == 0 || contain == 1, "the containment flag is 0 or 1");
  if (BS == 0) return ELFIHIP_OK;
  ELFIHIP_REQUIRE(ctx, theta && count && (R == 0 || prob), "NULL pointer");
  ELFIHIP_REQUIRE(ctx, !contain || R == 0 || (centre && rotation_inv && limits), "containment needs the boxes");
  if (R > 0) ELFIHIP_TRY(ro_index_check(h, prob, R));
  DeviceGuard g(ctx->device);
  const size_t n = (size_t)R, b = (size_t)BS, pd = sizeof(double);
  const bool boxes = contain && R > 0;
  RoCarve in, out;
  const size_t o_t = in.add(b * 2 * pd), o_p = in.add(n * sizeof(int64_t)), o_c = in.add(n * 2 * pd), o_r = in.add(n * 4 * pd),
               o_l = in.add(n * 4 * pd);
  const size_t o_n = out.add(b * sizeof(int32_t));
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(in.used));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(out.used));
  in.base = ctx->in.as<char>();
  out.base = ctx->out.as<char>();
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_t), theta, b * 2 * pd, hipMemcpyHostToDevice, ctx->stream));
  if (R > 0) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<int64_t>(o_p), prob, n * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
  if (boxes) {
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_c), centre, n * 2 * pd, hipMemcpyHostToDevice, ctx->stream));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_r), rotation_inv, n * 4 * pd, hipMemcpyHostToDevice, ctx->stream));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(in.at<double>(o_l), limits, n * 4 * pd, hipMemcpyHostToDevice, ctx->stream));
  }
  ELFIHIP_TRY(ro_count_impl(h, BS, in.at<double>(o_t), 2, R, in.at<int64_t>(o_p), eps, contain, in.at<double>(o_c), in.at<double>(o_r),
                            in.at<double>(o_l), out.at<int32_t>(o_n)));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(count, out.at<int32_t>(o_n), b * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
