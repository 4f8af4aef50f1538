// Per-metric arithmetic of the distance kernels (device only): Op for the metrics that are one left-to-right accumulator,
// Row for canberra, braycurtis, cosine and correlation.  Both sum in SciPy's order, so the results are bit-identical to cdist.
// FMA contraction is off from here to the end of the including file: a fused d*d+s would round differently from the
// reference's separate multiply and add.  (The headers below are included first: they keep the default.)
#pragma once

#include "common.hpp"
#include "tile_stream.hpp"
#include "np_sum.hpp"

#pragma clang fp contract(off)

namespace elfihip {

// Cube root for the order-3 Minkowski distance: exponent split by frexp, a single-precision seed (exp2 / log2, ~1e-6) and
// ONE Halley step (cubic: ~1e-18) -- some sixty instructions against the several hundred of pow(s, 1.0 / 3.0); within
// 1 ulp of the correctly rounded root, inside the 1e-14 the general orders are held to against SciPy's pow().
// (The device library's cbrt() measured SLOWER than pow() here: 1.25 10^6 x 64 rows 0.128 -> 0.205 ms.)
__device__ __forceinline__ double cbrt_halley(double s) {
  if (!(s > 0.0) || !(s < __builtin_huge_val())) return s;   // 0, NaN, +inf (negative sums do not occur)
  int e;
  double mant = frexp(s, &e);                 // s = mant 2^e, mant in [0.5, 1)
  int q = e / 3, r = e - 3 * q;
  if (r < 0) {
    r += 3;
    q -= 1;
  }
  mant = ldexp(mant, r);                      // in [0.5, 4)
  double y = (double)__builtin_exp2f(__builtin_log2f((float)mant) * (1.0f / 3.0f));
  const double y3 = y * y * y;
  y = y * ((y3 + 2.0 * mant) / (2.0 * y3 + mant));
  return ldexp(y, q);
}

// ---- per-metric term / finish --------------------------------------------------
template <int METRIC, bool W>
struct Op {
  __device__ static __forceinline__ double init() { return 0.0; }
  __device__ static __forceinline__ double step(double s, double x, double y, double a, double p) {
    double d = x - y;
    if constexpr (METRIC == ELFIHIP_EUCLIDEAN) {
      double t = d * d;
      if constexpr (W) t = a * t;  // SciPy: w * (d*d)
      return s + t;
    } else if constexpr (METRIC == ELFIHIP_SQEUCLIDEAN) {
      if constexpr (W) return s + (a * d) * d;  // SciPy associates the other way here
      return s + d * d;
    } else if constexpr (METRIC == ELFIHIP_CITYBLOCK) {
      double t = fabs(d);
      if constexpr (W) t = a * t;
      return s + t;
    } else if constexpr (METRIC == ELFIHIP_CHEBYSHEV) {
      double t = fabs(d);
      if constexpr (W) t = (a == 0.0) ? 0.0 : t;  // SciPy: zero-weight columns are ignored
      return t > s ? t : s;
    } else if constexpr (METRIC == ELFIHIP_MINKOWSKI) {
      // p = 3 and p = 4 (the integer orders the repository's examples use beyond 1 and 2) by multiplication:
      // within 1 ulp of pow() per term and several times cheaper; any other order through pow()
      const double ad = fabs(d);
      double t;
      if (p == 3.0)
        t = (ad * ad) * ad;
      else if (p == 4.0)
        t = (ad * ad) * (ad * ad);
      else
        t = pow(ad, p);
      if constexpr (W) t = a * t;
      return s + t;
    } else {  // ELFIHIP_SEUCLIDEAN, a = V_j
      return s + (d * d) / a;
    }
  }
  __device__ static __forceinline__ double combine(double a, double b) {
    if constexpr (METRIC == ELFIHIP_CHEBYSHEV)
      return a > b ? a : b;
    else
      return a + b;
  }
  __device__ static __forceinline__ double finish(double s, double inv_p) {
    if constexpr (METRIC == ELFIHIP_EUCLIDEAN || METRIC == ELFIHIP_SEUCLIDEAN)
      return sqrt(s);
    else if constexpr (METRIC == ELFIHIP_MINKOWSKI) {
      // the root of the integer orders 3 and 4 without pow() (SciPy takes pow(s, 1.0 / p), whose exponent is itself
      // rounded: the roots below agree with it to 1-2 ulp, inside the 1e-14 the general orders are held to); at
      // m = 2 the pow() per ROW was what the kernel spent its time on (4 10^6 rows: 0.058 ms against 0.018 for euclidean)
      if (inv_p == 1.0 / 3.0) return cbrt_halley(s);
      if (inv_p == 0.25) return sqrt(sqrt(s));
      return pow(s, inv_p);
    } else
      return s;
  }
};

// ---- canberra, braycurtis, cosine, correlation ----------------------------------------------------------------------
// These do not fit Op's one left-to-right accumulator: braycurtis keeps two sums, cosine forms its dot products in SciPy's
// two lanes (even j, odd j, then the odd last term), correlation first takes the row mean in NumPy's pairwise order.  A
// kernel hands Row<METRIC, W>::dist its row as accessors -- x(j) (LDS, registers or global), y(j), a(j) -- and Row sums
// in exactly the order SciPy does, so the unweighted forms (and weighted canberra / braycurtis) are bit-identical to
// cdist.  Weighted cosine / correlation follow SciPy's Python correlation(u, v, w, centered): wn = w / sum w, means
// x.wn, dots x.(y wn), 1 - uv / sqrt(uu vv) clipped to [0, 2]; SciPy's np.dot order is its BLAS's (held to 1e-13).
// What depends on the observed row alone (Obs) is formed once per workgroup inside the kernel, from y and aux.
template <int METRIC>
constexpr bool kRowMetric = METRIC >= ELFIHIP_CANBERRA;

struct Obs {
  double sw;     // weighted cosine / correlation: sum w (the kernels keep wn_j = w_j / sw in place of w_j)
  double ymu;    // correlation: mean of y (weighted: y.wn)
  double ynorm;  // unweighted: |y| (correlation: |y - ymu|); weighted: (y - ymu).((y - ymu) wn)
};

template <int METRIC, bool W>
struct Row {
  static constexpr bool kCentered = METRIC == ELFIHIP_CORRELATION;
  static constexpr bool kNormW = W && (METRIC == ELFIHIP_COSINE || METRIC == ELFIHIP_CORRELATION);

  // the observed row's constants; y(j), w(j) are the raw observed row and weights
  template <class YF, class WF>
  __device__ static __forceinline__ Obs obs(YF y, WF w, int m) {
    Obs o{1.0, 0.0, 0.0};
    if constexpr (METRIC == ELFIHIP_COSINE || METRIC == ELFIHIP_CORRELATION) {
      if constexpr (W) {
        o.sw = np_pairwise_bounded<2>(w, 0, m);   // w.sum()
        if constexpr (kCentered) {
          double mu = 0.0;
          for (int j = 0; j < m; ++j) mu += y(j) * (w(j) / o.sw);
          o.ymu = mu;
        }
        double vv = 0.0;
        for (int j = 0; j < m; ++j) {
          const double yc = y(j) - o.ymu;
          vv += yc * (yc * (w(j) / o.sw));
        }
        o.ynorm = vv;
      } else {
        if constexpr (kCentered) o.ymu = np_pairwise_bounded<2>(y, 0, m) / (double)m;
        auto cy = [&](int j) { return kCentered ? y(j) - o.ymu : y(j); };
        o.ynorm = sqrt(dot2(cy, cy, m));
      }
    }
    return o;
  }

  // SciPy's dot_product: two lanes (even and odd j), added, then the last term of an odd length
  template <class UF, class VF>
  __device__ static __forceinline__ double dot2(UF u, VF v, int m) {
    double s0 = 0.0, s1 = 0.0;
    int j = 0;
#pragma unroll 4
    for (; j + 1 < m; j += 2) {
      s0 += u(j) * v(j);
      s1 += u(j + 1) * v(j + 1);
    }
    double s = s0 + s1;
    if (m & 1) s += u(m - 1) * v(m - 1);
    return s;
  }

  // x(j), y(j) the row and the observed row, a(j) the weight the kernel keeps (w_j, or wn_j for cosine / correlation)
  template <class XF, class YF, class AF>
  __device__ static __forceinline__ double dist(XF x, YF y, AF a, int m, const Obs& o) {
    if constexpr (METRIC == ELFIHIP_CANBERRA) {
      double s = 0.0;
#pragma unroll 4
      for (int j = 0; j < m; ++j) {
        const double xj = x(j), yj = y(j);
        double num = fabs(xj - yj);
        const double den = fabs(xj) + fabs(yj);
        if constexpr (W) num = a(j) * num;
        s += num / (den + (den == 0.0 ? 1.0 : 0.0));
      }
      return s;
    } else if constexpr (METRIC == ELFIHIP_BRAYCURTIS) {
      double sn = 0.0, sd = 0.0;
#pragma unroll 4
      for (int j = 0; j < m; ++j) {
        const double xj = x(j), yj = y(j);
        double dn = fabs(xj - yj), dd = fabs(xj + yj);
        if constexpr (W) {
          dn = a(j) * dn;
          dd = a(j) * dd;
        }
        sn += dn;
        sd += dd;
      }
      return sn / sd;
    } else if constexpr (W) {   // weighted cosine / correlation
      double xmu = 0.0;
      if constexpr (kCentered) {
#pragma unroll 4
        for (int j = 0; j < m; ++j) xmu += x(j) * a(j);
      }
      double uv = 0.0, uu = 0.0;
#pragma unroll 4
      for (int j = 0; j < m; ++j) {
        const double xc = kCentered ? x(j) - xmu : x(j);
        const double yc = kCentered ? y(j) - o.ymu : y(j);
        uv += xc * (yc * a(j));
        uu += xc * (xc * a(j));
      }
      return clip02(1.0 - uv / sqrt(uu * o.ynorm));
    } else {                    // cosine / correlation
      double xmu = 0.0;
      if constexpr (kCentered) xmu = np_pairwise_bounded<2>(x, 0, m) / (double)m;
      auto cx = [&](int j) { return kCentered ? x(j) - xmu : x(j); };
      auto cy = [&](int j) { return kCentered ? y(j) - o.ymu : y(j); };
      double s0 = 0.0, s1 = 0.0, q0 = 0.0, q1 = 0.0;
      int j = 0;
#pragma unroll 4
      for (; j + 1 < m; j += 2) {
        const double x0 = cx(j), x1 = cx(j + 1);
        s0 += x0 * cy(j);
        s1 += x1 * cy(j + 1);
        q0 += x0 * x0;
        q1 += x1 * x1;
      }
      double s = s0 + s1, q = q0 + q1;
      if (m & 1) {
        const double xl = cx(m - 1);
        s += xl * cy(m - 1);
        q += xl * xl;
      }
      return cos_finish(s, sqrt(q), o.ynorm);
    }
  }

  // SciPy's cosine_distance_double: clip the cosine to [-1, 1], then 1 - c (NaN stays NaN)
  __device__ static __forceinline__ double cos_finish(double dot, double nx, double ny) {
    double c = dot / (nx * ny);
    if (fabs(c) > 1.0) c = copysign(1.0, c);
    return 1.0 - c;
  }
  // np.clip(d, 0, 2), NaN stays NaN
  __device__ static __forceinline__ double clip02(double d) { return d < 0.0 ? 0.0 : (d > 2.0 ? 2.0 : d); }

  // wide rows (one wavefront per row, lane-strided partial sums, butterfly): x, y, w raw pointers
  __device__ static __forceinline__ double wide(const double* __restrict__ x, const double* __restrict__ y,
                                                const double* __restrict__ w, int m, int lane, const Obs& o) {
    auto wsum = [](double v) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      return v;
    };
    auto wn = [&](int j) { return kNormW ? w[j] / o.sw : (W ? w[j] : 1.0); };
    if constexpr (METRIC == ELFIHIP_CANBERRA || METRIC == ELFIHIP_BRAYCURTIS) {
      double s0 = 0.0, s1 = 0.0;
      for (int j = lane; j < m; j += 64) {
        const double xj = x[j], yj = y[j];
        if constexpr (METRIC == ELFIHIP_CANBERRA) {
          double num = fabs(xj - yj);
          const double den = fabs(xj) + fabs(yj);
          if constexpr (W) num = w[j] * num;
          s0 += num / (den + (den == 0.0 ? 1.0 : 0.0));
        } else {
          double dn = fabs(xj - yj), dd = fabs(xj + yj);
          if constexpr (W) {
            dn = w[j] * dn;
            dd = w[j] * dd;
          }
          s0 += dn;
          s1 += dd;
        }
      }
      s0 = wsum(s0);
      if constexpr (METRIC == ELFIHIP_CANBERRA) return s0;
      return s0 / wsum(s1);
    } else {
      double xmu = 0.0;
      if constexpr (kCentered) {
        for (int j = lane; j < m; j += 64) xmu += W ? x[j] * wn(j) : x[j];
        xmu = wsum(xmu);
        if constexpr (!W) xmu = xmu / (double)m;
      }
      double uv = 0.0, uu = 0.0;
      for (int j = lane; j < m; j += 64) {
        const double xc = x[j] - xmu, yc = y[j] - o.ymu;
        if constexpr (W) {
          uv += xc * (yc * wn(j));
          uu += xc * (xc * wn(j));
        } else {
          uv += xc * yc;
          uu += xc * xc;
        }
      }
      uv = wsum(uv);
      uu = wsum(uu);
      if constexpr (W) return clip02(1.0 - uv / sqrt(uu * o.ynorm));
      return cos_finish(uv, sqrt(uu), o.ynorm);
    }
  }
};

// the weight a kernel keeps for metric METRIC: w_j as given, wn_j = w_j / sum w for weighted cosine / correlation
template <int METRIC, bool W>
__device__ __forceinline__ double kept_aux(double w, const Obs& o) {
  if constexpr (kRowMetric<METRIC> && Row<METRIC, W>::kNormW) return w / o.sw;
  return w;
}

// the observed row's constants from global y / aux (every lane forms the same values; uniform loads)
template <int METRIC, bool W>
__device__ __forceinline__ Obs obs_of(const double* __restrict__ y, const double* __restrict__ aux, int m) {
  if constexpr (kRowMetric<METRIC>)
    return Row<METRIC, W>::obs([&](int j) { return y[j]; }, [&](int j) { return W ? aux[j] : 1.0; }, m);
  return Obs{1.0, 0.0, 0.0};
}

}  // namespace elfihip
