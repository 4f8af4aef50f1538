// The GP mean alone at many points, and a differential-evolution search for its minimiser that stays on the device.
//
// Replaces stochastic_optimization (elfi/methods/bo/utils.py:9-37) as BayesianOptimization.extract_result calls it
// (elfi/methods/inference/bolfi.py:180-199): SciPy's differential_evolution over target_model.predict_mean, one full
// GP prediction (mean AND variance: a pass over the factor) per trial vector.  The mean needs only k(x, X) alpha, O(n d)
// per point; here one generation of the search is ONE launch -- workgroup i makes member i's trial vector, evaluates the
// mean at it and selects -- and the host reads a converged flag once per chunk of generations.  The statement of the
// algorithm is in include/elfihip.h (elfihip_gp_minimize_mean) and, in NumPy, in tests/de_ref.py.
#include <cmath>
#include <vector>

#include "gp.hpp"
#include "philox.hpp"

namespace elfihip {

constexpr int DE_MAX_NP = 3840;       // population limit: 15 members per dimension at the largest accepted dimension
constexpr int DE_DEFAULT_CHUNK = 8;   // generations enqueued between two reads of the converged flag
constexpr double DE_CR = 0.7;         // SciPy's recombination constant

// ---- the mean at the point held in LDS ---------------------------------------------------------------------------------
// Terms as kstar_kernel (gp_predict.hip) forms them: r2 = (|x|^2 + |X_i|^2) - 2 x.X_i clipped at 0, k = CovFn<KIND>::k(r2) (rbf: s_f exp(r2 (-1/2l^2))),
// term_i = (k + s_b) alpha_i.  Summation order (fixed; it depends on n alone): thread t of the 256 adds the terms
// i = t, t + 256, t + 512, ... in ascending order; the 64 lanes of a wave are then added by the xor
// butterfly 32, 16, 8, 4, 2, 1; the four waves as ((w0 + w1) + w2) + w3.  Every thread returns the sum.
template <int KIND>
__device__ __forceinline__ double mean_at(const double* __restrict__ X, const double* __restrict__ x2,
                                          const double* __restrict__ alpha, int64_t n, int dp, double var,
                                          double neg_half_inv_ls2, double bias, const double* sx, double sx2, double* red) {
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    double dot = 0.0;
    for (int c = 0; c < dp; ++c) dot += sx[c] * X[i * dp + c];
    double r2 = (sx2 + x2[i]) + (-2.0 * dot);
    r2 = r2 < 0.0 ? 0.0 : r2;
    const double k = CovFn<KIND>(var, neg_half_inv_ls2).k(r2);
    const double contrib = (k + bias) * alpha[i];
    {
#pragma clang fp contract(off)
      acc = acc + contrib;   // an addition of the rounded term, as the prediction's sum has it
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  __syncthreads();   // red may still be read from an earlier use
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// mu[s] for the points xs (S, dp) zero padded, with their squared norms: one workgroup per point
template <int KIND>
__global__ __launch_bounds__(256) void mean_kernel(const double* X, const double* x2, const double* alpha, const double* xs,
                                                   const double* xs2, int64_t n, int dp, double var,
                                                   double neg_half_inv_ls2, double bias, double* mu) {
  __shared__ double sx[256];
  __shared__ double red[4];
  const int64_t s = blockIdx.x;
  if ((int)threadIdx.x < dp) sx[threadIdx.x] = xs[s * dp + threadIdx.x];
  __syncthreads();
  const double m = mean_at<KIND>(X, x2, alpha, n, dp, var, neg_half_inv_ls2, bias, sx, xs2[s], red);
  if (threadIdx.x == 0) mu[s] = m;
}

// ---- the search's random numbers ------------------------------------------------------------------------------------------
// Draw (generation g, member i, slot s) is the first 53-bit uniform of Philox counter (c0 = i (2 d + 4) + s, c1 = g) of
// (seed, stream).  Slots: 0, 1 the two indices; 2 the fill point; 3 + j the crossover of dimension j; 3 + d + j its redraw;
// 3 + 2 d the dither (member 0's is the generation's).  Generation 0 is the start population: slot 3 + j of member i is the
// uniform that dimension j is ordered by, slot 3 + d + j the member's place inside its stratum.
__device__ __forceinline__ double de_draw(uint64_t seed, uint64_t stream, int g, int i, int slot, int d) {
  const uint32_t c0 = (uint32_t)i * (uint32_t)(2 * d + 4) + (uint32_t)slot;
  uint64_t a, b;
  words53(seed, stream, c0, (uint32_t)g, a, b);
  return unit_co(a);
}

struct DeState {
  int converged;   // the stop test held after generation `gens`
  int gens;        // generations made
  int nonfinite;   // an energy was not finite
  int pad;
};

struct DeArgs {
  const double *X, *x2, *alpha;
  int64_t n;
  int dp, d, NP;
  double var, neg_half_inv_ls2, bias;
  const double *lo, *hi;   // (d) each
  uint64_t seed, stream;
  double tol;
  int maxiter;
  DeState* st;
};

// Start population in unit coordinates: workgroup j orders the members by their uniforms of dimension j (stable: ties by
// index) and member i takes (perm_j(i) + u_ij) / NP, perm_j the stable argsort.
__global__ __launch_bounds__(256) void de_start_kernel(DeArgs A, double* pop) {
  __shared__ double su[DE_MAX_NP];
  __shared__ int sperm[DE_MAX_NP];
  const int j = blockIdx.x, NP = A.NP, d = A.d;
  for (int i = threadIdx.x; i < NP; i += 256) su[i] = de_draw(A.seed, A.stream, 0, i, 3 + j, d);
  __syncthreads();
  for (int i = threadIdx.x; i < NP; i += 256) {
    const double u = su[i];
    int rank = 0;
    for (int k = 0; k < NP; ++k) rank += (su[k] < u || (su[k] == u && k < i)) ? 1 : 0;
    sperm[rank] = i;   // a permutation: every rank is written once
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NP; i += 256) {
#pragma clang fp contract(off)
    pop[(int64_t)i * d + j] = ((double)sperm[i] + de_draw(A.seed, A.stream, 0, i, 3 + d + j, d)) / (double)NP;
  }
}

// Generation g (g = 0: the energies of the start population).  Workgroup i reads the whole previous generation (pin, Ein)
// and writes member i of the next (pout, Eout): no workgroup reads what another writes in the same launch.  Every workgroup
// forms the stop test and the best member from Ein by itself, in the same fixed order, so all take the same decision.
template <int KIND>
__global__ __launch_bounds__(256) void de_generation_kernel(DeArgs A, int g, const double* pin, const double* Ein,
                                                            double* pout, double* Eout) {
  __shared__ double sx[256];
  __shared__ double strial[256];
  __shared__ double red[4];
  __shared__ double sred[256];
  __shared__ int sidx[256];
  const int i = blockIdx.x, NP = A.NP, d = A.d, t = threadIdx.x;
  __shared__ int sflag;
  bool stop = false;
  int best = 0;
  if (g > 0) {
    // The two flags are written by workgroup 0 alone, from the very energies every workgroup tests below, so reading one
    // early or late changes no decision; thread 0 reads them ONCE for the workgroup, so that all its waves take the same
    // branch around the barriers below whenever workgroup 0's store of this launch becomes visible.
    if (t == 0) sflag = (A.st->converged != 0 || A.st->nonfinite != 0) ? 1 : 0;
    __syncthreads();
    stop = sflag != 0;
    if (!stop) {
      // mean, standard deviation and arg-min of Ein: thread t takes t, t + 256, ... in order; then a halving tree
      double s = 0.0, bv = INFINITY;
      int bi = NP;
      bool bad = false;
      for (int k = t; k < NP; k += 256) {
        const double e = Ein[k];
        s += e;
        bad |= !isfinite(e);
        if (e < bv) bv = e, bi = k;
      }
      sred[t] = s;
      __syncthreads();
      for (int w = 128; w > 0; w >>= 1) {
        if (t < w) sred[t] += sred[t + w];
        __syncthreads();
      }
      const double mean = sred[0] / (double)NP;
      __syncthreads();
      double q = 0.0;
      for (int k = t; k < NP; k += 256) {
        const double dlt = Ein[k] - mean;
        q += dlt * dlt;
      }
      sred[t] = q;
      __syncthreads();
      for (int w = 128; w > 0; w >>= 1) {
        if (t < w) sred[t] += sred[t + w];
        __syncthreads();
      }
      const double sd = sqrt(sred[0] / (double)NP);
      __syncthreads();
      sred[t] = bv;
      sidx[t] = bad ? -1 : bi;
      __syncthreads();
      for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
          const double ov = sred[t + w];
          const int oi = sidx[t + w];
          if (oi < 0 || sidx[t] < 0) sidx[t] = -1;
          else if (ov < sred[t] || (ov == sred[t] && oi < sidx[t])) sred[t] = ov, sidx[t] = oi;
        }
        __syncthreads();
      }
      best = sidx[0];
      __syncthreads();
      if (best < 0) {
        stop = true;
        if (i == 0 && t == 0) A.st->nonfinite = 1;
      } else if (g > 1 && sd <= A.tol * fabs(mean)) {   // the test follows a generation, as SciPy's solve() has it
        stop = true;
        if (i == 0 && t == 0) A.st->converged = 1;
      } else if (g > A.maxiter) {   // the launch after the last generation only tests
        stop = true;
      }
    }
    if (stop) {   // the member passes through unchanged
      if (t < d) pout[(int64_t)i * d + t] = pin[(int64_t)i * d + t];
      if (t == 0) Eout[i] = Ein[i];
      return;
    }
    if (i == 0 && t == 0) A.st->gens = g;
  }
  // the trial vector (unit coordinates), one thread per dimension
  if (t < d) {
    double v = pin[(int64_t)i * d + t];
    if (g > 0) {
      const double F = 0.5 + 0.5 * de_draw(A.seed, A.stream, g, 0, 3 + 2 * d, d);
      int r0 = (int)(de_draw(A.seed, A.stream, g, i, 0, d) * (double)(NP - 1));
      r0 = r0 > NP - 2 ? NP - 2 : r0;
      r0 += r0 >= i ? 1 : 0;
      int r1 = (int)(de_draw(A.seed, A.stream, g, i, 1, d) * (double)(NP - 2));
      r1 = r1 > NP - 3 ? NP - 3 : r1;
      const int lo2 = i < r0 ? i : r0, hi2 = i < r0 ? r0 : i;
      r1 += r1 >= lo2 ? 1 : 0;
      r1 += r1 >= hi2 ? 1 : 0;
      int fill = (int)(de_draw(A.seed, A.stream, g, i, 2, d) * (double)d);
      fill = fill > d - 1 ? d - 1 : fill;
      if (t == fill || de_draw(A.seed, A.stream, g, i, 3 + t, d) < DE_CR) {
#pragma clang fp contract(off)
        const double diff = pin[(int64_t)r0 * d + t] - pin[(int64_t)r1 * d + t];
        v = pin[(int64_t)best * d + t] + F * diff;
      }
      if (v < 0.0 || v > 1.0) v = de_draw(A.seed, A.stream, g, i, 3 + d + t, d);   // SciPy's _ensure_constraint
    }
    strial[t] = v;
    {
#pragma clang fp contract(off)
      const double l = A.lo[t], h = A.hi[t];
      sx[t] = 0.5 * (l + h) + (v - 0.5) * fabs(h - l);
    }
  } else if (t < A.dp) {
    sx[t] = 0.0;
  }
  __syncthreads();
  double q = 0.0;   // |x|^2 in ascending order of the dimension, as the host forms it for a prediction call
  {
#pragma clang fp contract(off)
    for (int c = 0; c < d; ++c) q = q + sx[c] * sx[c];
  }
  const double e = mean_at<KIND>(A.X, A.x2, A.alpha, A.n, A.dp, A.var, A.neg_half_inv_ls2, A.bias, sx, q, red);
  // an energy that is not finite is kept with its trial: the next launch (there always is one) finds it in Ein, in every
  // workgroup alike, and ends the search with the error -- no flag is written here, where other workgroups might read it
  const bool take = g == 0 || e <= Ein[i] || !isfinite(e);
  if (t < d) pout[(int64_t)i * d + t] = take ? strial[t] : pin[(int64_t)i * d + t];
  if (t == 0) Eout[i] = take ? e : Ein[i];
}

// mean-only evaluation of S host points (one upload, one launch, one download)
static int predict_mean_impl(elfihip_gp* gp, const double* Xs, int64_t S, double* mu) {
  elfihip_ctx* ctx = gp->ctx;
  const int d = gp->d, dp = gp->dp;
  std::vector<double> h((size_t)S * (dp + 1), 0.0);
  double* hx2 = h.data() + (size_t)S * dp;
  for (int64_t s = 0; s < S; ++s) {
    double q = 0.0;
    for (int c = 0; c < d; ++c) {
      const double x = Xs[s * d + c];
      h[(size_t)s * dp + c] = x;
      q += x * x;
    }
    hx2[s] = q;
  }
  ELFIHIP_CHECK_HIP(ctx, gp->ws_min.reserve(((size_t)S * (dp + 2)) * sizeof(double)));
  double* dx = gp->ws_min.as<double>();
  double* dmu = dx + (size_t)S * (dp + 1);
  hipStream_t st = ctx->stream;
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dx, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, st));
  dispatch_kernel(gp->kernel, [&](auto kind) {
    hipLaunchKernelGGL(mean_kernel<decltype(kind)::value>, dim3((unsigned)S), dim3(256), 0, st, gp->X, gp->x2, gp->alpha, dx,
                       dx + (size_t)S * dp, gp->n, dp, gp->var, -0.5 / (gp->ls * gp->ls), gp->bias, dmu);
  });
  ELFIHIP_TRY(launch_status(ctx, "mean_kernel"));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(mu, dmu, (size_t)S * sizeof(double), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

static int minimize_mean_impl(elfihip_gp* gp, const double* lower, const double* upper, uint64_t seed, uint64_t stream,
                              int popsize, int maxiter, double tol, int polish, double* x_out, double* f_out,
                              int64_t* info_out, double* pop_out, double* energies_out) {
  elfihip_ctx* ctx = gp->ctx;
  const int d = gp->d;
  const int NP = std::max(5, popsize * d);
  const size_t npd = (size_t)NP * d;
  // device: lo, hi (d each) | two populations | two energy vectors | the state
  const size_t n_dbl = 2 * (size_t)d + 2 * npd + 2 * (size_t)NP;
  ELFIHIP_CHECK_HIP(ctx, gp->ws_de.reserve(n_dbl * sizeof(double) + sizeof(DeState)));
  double* dlo = gp->ws_de.as<double>();
  double* dhi = dlo + d;
  double* pop[2] = {dhi + d, dhi + d + npd};
  double* E[2] = {pop[1] + npd, pop[1] + npd + NP};
  DeState* dst = reinterpret_cast<DeState*>(E[1] + NP);
  hipStream_t st = ctx->stream;
  std::vector<double> hb(2 * (size_t)d);
  std::copy(lower, lower + d, hb.begin());
  std::copy(upper, upper + d, hb.begin() + d);
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dlo, hb.data(), hb.size() * sizeof(double), hipMemcpyHostToDevice, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemsetAsync(dst, 0, sizeof(DeState), st));
  DeArgs A;
  A.X = gp->X, A.x2 = gp->x2, A.alpha = gp->alpha;
  A.n = gp->n, A.dp = gp->dp, A.d = d, A.NP = NP;
  A.var = gp->var, A.neg_half_inv_ls2 = -0.5 / (gp->ls * gp->ls), A.bias = gp->bias;
  A.lo = dlo, A.hi = dhi;
  A.seed = seed, A.stream = stream, A.tol = tol, A.maxiter = maxiter, A.st = dst;
  hipLaunchKernelGGL(de_start_kernel, dim3((unsigned)d), dim3(256), 0, st, A, pop[1]);
  ELFIHIP_TRY(launch_status(ctx, "de_start_kernel"));
  // generation g reads buffer (g + 1) & 1 and writes buffer g & 1
  dispatch_kernel(gp->kernel, [&](auto kind) {
    hipLaunchKernelGGL(de_generation_kernel<decltype(kind)::value>, dim3((unsigned)NP), dim3(256), 0, st, A, 0, pop[1], E[1], pop[0],
                       E[0]);
  });
  ELFIHIP_TRY(launch_status(ctx, "de_generation_kernel"));
  const int chunk = gp->min_chunk > 0 ? gp->min_chunk : DE_DEFAULT_CHUNK;
  int g = 0, converged = 0, gens = 0, nonfinite = 0;
  for (;;) {
    // one more launch than generations: the stop test on generation maxiter's energies is the next launch's
    const int g_end = std::min(g + chunk, maxiter + 1);
    for (; g < g_end; ++g) {
      dispatch_kernel(gp->kernel, [&](auto kind) {
        hipLaunchKernelGGL(de_generation_kernel<decltype(kind)::value>, dim3((unsigned)NP), dim3(256), 0, st, A, g + 1, pop[g & 1],
                           E[g & 1], pop[(g + 1) & 1], E[(g + 1) & 1]);
      });
      ELFIHIP_TRY(launch_status(ctx, "de_generation_kernel"));
    }
    MailSrc M;
    M.p[0] = &dst->converged, M.p[1] = &dst->gens, M.p[2] = &dst->nonfinite, M.p[3] = nullptr;
    M.bytes[0] = M.bytes[1] = M.bytes[2] = 4, M.bytes[3] = 0;
    M.n = 3;
    ELFIHIP_TRY(mail_post(ctx, M));
    ELFIHIP_TRY(mail_wait(ctx));
    converged = (int)mail_read(ctx, 0), gens = (int)mail_read(ctx, 1), nonfinite = (int)mail_read(ctx, 2);
    if (converged || nonfinite || g > maxiter) break;
  }
  if (nonfinite)
    return fail(ctx, ELFIHIP_ERR_STATE, "the GP mean is not finite at a trial point of generation %d", gens);
  std::vector<double> hp(npd), he((size_t)NP);
  const int cur = g & 1;
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(hp.data(), pop[cur], npd * sizeof(double), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(he.data(), E[cur], (size_t)NP * sizeof(double), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  int best = 0;
  for (int i = 1; i < NP; ++i)
    if (he[(size_t)i] < he[(size_t)best]) best = i;
  std::vector<double> x((size_t)d);
  for (int c = 0; c < d; ++c) {
    const double v = 0.5 * (lower[c] + upper[c]) + (hp[(size_t)best * d + c] - 0.5) * std::fabs(upper[c] - lower[c]);
    x[(size_t)c] = std::min(std::max(v, lower[c]), upper[c]);
  }
  double f = he[(size_t)best];
  int64_t nfev = (int64_t)NP * (gens + 1);
  int accepted = 0;
  if (polish) {
    std::vector<double> xp((size_t)d);
    double fp = 0.0, fm = 0.0;
    int64_t ne = 0;
    ELFIHIP_TRY(elfihip_gp_lcb_minimize(gp, x.data(), 1, lower, upper, 0.0, 1000, xp.data(), &fp, nullptr, &ne));
    ELFIHIP_TRY(predict_mean_impl(gp, xp.data(), 1, &fm));
    nfev += ne + 1;
    if (fm < f) {
      x = xp;
      f = fm;
      accepted = 1;
    }
  }
  std::copy(x.begin(), x.end(), x_out);
  if (f_out) *f_out = f;
  if (info_out) info_out[0] = gens, info_out[1] = nfev, info_out[2] = converged, info_out[3] = accepted;
  if (pop_out) std::copy(hp.begin(), hp.end(), pop_out);
  if (energies_out) std::copy(he.begin(), he.end(), energies_out);
  return ELFIHIP_OK;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_gp_predict_mean(elfihip_gp* gp, const double* Xs, int64_t S, double* mu) {
  if (!gp) return fail(nullptr, ELFIHIP_ERR_ARG, "gp is NULL");
  elfihip_ctx* ctx = gp->ctx;
  ELFIHIP_REQUIRE(ctx, S >= 0 && (S == 0 || (Xs && mu)), "bad arguments");
  ELFIHIP_REQUIRE(ctx, S <= 0x7fffffff, "%lld points exceed one launch (2^31 - 1 workgroups)", (long long)S);
  if (!gp->factored || gp->n < 1)
    return fail(ctx, ELFIHIP_ERR_STATE, "GP is not factorised (call elfihip_gp_factorize first)");
  if (S == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  try {
    return predict_mean_impl(gp, Xs, S, mu);
  } catch (const std::bad_alloc&) {
    return fail(ctx, ELFIHIP_ERR_NOMEM, "out of host memory staging %lld points", (long long)S);
  }
}

int elfihip_gp_minimize_mean(elfihip_gp* gp, const double* lower, const double* upper, uint64_t seed, uint64_t stream,
                             int popsize, int maxiter, double tol, int polish, double* x_out, double* f_out,
                             int64_t* info_out, double* pop_out, double* energies_out) {
  if (!gp) return fail(nullptr, ELFIHIP_ERR_ARG, "gp is NULL");
  elfihip_ctx* ctx = gp->ctx;
  ELFIHIP_REQUIRE(ctx, lower && upper && x_out, "bad arguments");
  ELFIHIP_REQUIRE(ctx, popsize >= 1 && maxiter >= 0 && tol >= 0.0, "popsize >= 1, maxiter >= 0 and tol >= 0 are required");
  for (int c = 0; c < gp->d; ++c)
    ELFIHIP_REQUIRE(ctx, std::isfinite(lower[c]) && std::isfinite(upper[c]) && lower[c] < upper[c],
                    "bounds of dimension %d are not finite with lower < upper", c);
  ELFIHIP_REQUIRE(ctx, (int64_t)popsize * gp->d <= DE_MAX_NP, "population %lld exceeds the limit %d (popsize x dimension)",
                  (long long)popsize * gp->d, DE_MAX_NP);
  if (!gp->factored || gp->n < 1)
    return fail(ctx, ELFIHIP_ERR_STATE, "GP is not factorised (call elfihip_gp_factorize first)");
  DeviceGuard g(ctx->device);
  try {
    return minimize_mean_impl(gp, lower, upper, seed, stream, popsize, maxiter, tol, polish, x_out, f_out, info_out, pop_out,
                              energies_out);
  } catch (const std::bad_alloc&) {
    return fail(ctx, ELFIHIP_ERR_NOMEM, "out of host memory in the search for the mean's minimiser");
  }
}

int elfihip_gp_set_minimize_chunk(elfihip_gp* gp, int generations) {
  if (!gp) return fail(nullptr, ELFIHIP_ERR_ARG, "gp is NULL");
  ELFIHIP_REQUIRE(gp->ctx, generations >= 0 && generations <= 1024, "generations per chunk in [0, 1024]");
  gp->min_chunk = generations;
  return ELFIHIP_OK;
}

}  // extern "C"
