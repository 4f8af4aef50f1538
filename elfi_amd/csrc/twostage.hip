// Summary-statistic selection (Nunes & Balding 2010; elfi/methods/diagnostics.py:15-289, TwoStageSelection) on gfx950.
//
// Three pieces, each for all candidate combinations at once:
//   subset_best   the k best rows of every 0/1 column mask under the euclidean distance -- what the reference gets from
//                 one elfi.Rejection per combination (:172-212).  Composed: dist_multiw_dev_impl (multiw.hip) with the
//                 masks as weights (w * d2 with w in {0, 1} sums the subset with the same bits) into a block of at most
//                 kMaxK columns, topk_dev_impl (topk.hip) per column with the block's width as stride, then a bitonic
//                 sort of the survivors by (distance, row), NaN last.  Only the (C, k) results leave the device.
//   knn_entropy   E = log(pi^(q/2) / Gamma(q/2 + 1)) - psi(k) + log n + (q / n) sum_i log R_ik (:214-253) with R_ik the
//                 distance from point i to its k-th nearest neighbour, the point itself counting as the first (what
//                 cKDTree.query(theta_i, k)[0][-1] returns).  One query point per thread: its coordinates and an
//                 ascending list of the k smallest squared distances sit in registers (lengths 4 / 8 / 16), the
//                 candidates pass through LDS in tiles of 256 points and every thread visits them in index order
//                 (broadcast reads).  A squared distance is summed left to right; only R_ik gets a sqrt.  Coordinates are
//                 padded with zeros up to the instance's width: adding 0 * 0 leaves a sum's bits alone.
//   mrsse         (1 / J) sum_j sqrt(sum_{i,d} (theta_gid - closest_jd)^2) (:255-289): one workgroup per (g, j).
// Determinism: no atomics, no arrival counters; every workgroup reduces in a fixed tree and writes one partial, a second
// launch adds the partials in index order.  A group's result does not depend on G.
// fp contraction is off, as in the distance kernels whose bits subset_best has to reproduce.
#include "internal.hpp"
#include "dist_launch.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

#pragma clang fp contract(off)

namespace elfihip {

constexpr int TS_NT = 256;          // threads per workgroup = query points per workgroup = points per LDS tile
constexpr int TS_MAX_Q = 32;
constexpr int TS_MAX_K = 16;
constexpr int TS_SORT_CH = 2048;    // keys a workgroup sorts in LDS
constexpr size_t TS_BLOCK_BYTES = (size_t)1 << 30;

// Sum of the 256 values of a workgroup, every thread's `v` at red[tid]: ((0 + 128) + (64 + 192)) + ... in a fixed tree.
// All threads call; the sum is at red[0] after the last barrier.
__device__ __forceinline__ void ts_tree_sum(double* red, int tid, double v) {
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = TS_NT / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = red[tid] + red[tid + s];
    __syncthreads();
  }
}

struct KnnArgs {
  const double* T;   // (G n, q), pitch ldt
  int64_t n, ldt;
  int q, k;
  double* part;      // (G, nb): sum of log R over the workgroup's points
  double* kth;       // (G, n) or NULL
};

template <int KC, int QC>
__global__ __launch_bounds__(TS_NT) void knn_kernel(KnnArgs A) {
  extern __shared__ __align__(16) double lds[];
  double* tile = lds;                 // (256, QC)
  double* red = lds + TS_NT * QC;     // (256)
  const int tid = threadIdx.x, q = A.q;
  const int64_t g = blockIdx.x, nb = gridDim.y;
  const int64_t i = (int64_t)blockIdx.y * TS_NT + tid;
  const double* Tg = A.T + g * A.n * A.ldt;
  double a[QC], best[KC];
#pragma unroll
  for (int d = 0; d < QC; ++d) a[d] = (i < A.n && d < q) ? Tg[i * A.ldt + d] : 0.0;
#pragma unroll
  for (int t = 0; t < KC; ++t) best[t] = INFINITY;
  for (int64_t j0 = 0; j0 < A.n; j0 += TS_NT) {
    const int cnt = (int)(A.n - j0 < TS_NT ? A.n - j0 : TS_NT);
    __syncthreads();   // the previous tile is consumed
    for (int e = tid; e < cnt * QC; e += TS_NT) {
      const int jj = e / QC, d = e - jj * QC;
      tile[e] = d < q ? Tg[(j0 + jj) * A.ldt + d] : 0.0;
    }
    __syncthreads();
    for (int jj = 0; jj < cnt; ++jj) {
      const double* b = tile + jj * QC;
      double s = 0.0;
#pragma unroll
      for (int d = 0; d < QC; ++d) {
        const double df = a[d] - b[d];
        s = s + df * df;
      }
      if (s < best[KC - 1]) {   // (a NaN never enters)
#pragma unroll
        for (int t = KC - 1; t > 0; --t) best[t] = s < best[t - 1] ? best[t - 1] : (s < best[t] ? s : best[t]);
        best[0] = s < best[0] ? s : best[0];
      }
    }
  }
  double r2 = best[0];
#pragma unroll
  for (int t = 1; t < KC; ++t) r2 = (t == A.k - 1) ? best[t] : r2;
  const double R = sqrt(r2);
  if (A.kth && i < A.n) A.kth[g * A.n + i] = R;
  ts_tree_sum(red, tid, i < A.n ? log(R) : 0.0);
  if (tid == 0) A.part[g * nb + blockIdx.y] = red[0];
}

// entropy[g] = base + (q / n) (part[g][0] + part[g][1] + ...), the partials in index order
__global__ void knn_finish_kernel(const double* part, int64_t G, int64_t nb, double base, double qn, double* entropy) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  double s = 0.0;
  for (int64_t b = 0; b < nb; ++b) s = s + part[g * nb + b];
  entropy[g] = base + qn * s;
}

// root[g][j] = sqrt(sum_{i, d} (theta[g][i][d] - closest[j][d])^2): thread t sums the elements t, t + 256, ... of the
// flattened (i, d) index, then the tree
__global__ __launch_bounds__(TS_NT) void mrsse_root_kernel(const double* T, int64_t n, int q, int64_t ldt,
                                                           const double* Cl, int64_t ldc, double* root) {
  __shared__ double red[TS_NT];
  __shared__ double cj[TS_MAX_Q];
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x, j = blockIdx.y, J = gridDim.y;
  if (tid < q) cj[tid] = Cl[j * ldc + tid];
  __syncthreads();
  const double* Tg = T + g * n * ldt;
  const int64_t total = n * q;
  double s = 0.0;
  for (int64_t e = tid; e < total; e += TS_NT) {
    const int64_t i = e / q;
    const int d = (int)(e - i * q);
    const double df = Tg[i * ldt + d] - cj[d];
    s = s + df * df;
  }
  ts_tree_sum(red, tid, s);
  if (tid == 0) root[g * J + j] = sqrt(red[0]);
}

__global__ void mrsse_finish_kernel(const double* root, int64_t G, int64_t J, double* out) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  double s = 0.0;
  for (int64_t j = 0; j < J; ++j) s = s + root[g * J + j];
  out[g] = s / (double)J;
}

// ---- the survivors of a selection in order: (distance, row) ascending, NaN last ---------------------------------------

__device__ __forceinline__ bool ts_before(double va, int64_t ia, double vb, int64_t ib) {
  const bool na = va != va, nb = vb != vb;
  if (na != nb) return nb;
  if (!na && va != vb) return va < vb;
  return ia < ib;
}

// entries k .. P - 1 of every column's (P) list: NaN with the largest row number, behind every survivor
__global__ void ts_pad_kernel(double* v, int64_t* ix, int64_t cols, int64_t P, int64_t k) {
  const int64_t w = P - k, total = cols * w;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = e / w, t = k + (e - c * w);
    v[c * P + t] = __builtin_nan("");
    ix[c * P + t] = std::numeric_limits<int64_t>::max();
  }
}

// The bitonic network's steps that stay inside an aligned chunk of min(P, 2048) entries: merge sizes size_lo .. size_hi,
// of each the strides below the chunk length.  Grid (chunks, columns).
__global__ __launch_bounds__(TS_NT) void ts_sort_local_kernel(double* v, int64_t* ix, int64_t P, int64_t size_lo,
                                                              int64_t size_hi) {
  __shared__ double sv[TS_SORT_CH];
  __shared__ int64_t si[TS_SORT_CH];
  const int tid = threadIdx.x;
  const int len = (int)(P < TS_SORT_CH ? P : TS_SORT_CH);
  const int64_t base = (int64_t)blockIdx.x * len;
  double* vc = v + (int64_t)blockIdx.y * P + base;
  int64_t* ic = ix + (int64_t)blockIdx.y * P + base;
  for (int e = tid; e < len; e += TS_NT) {
    sv[e] = vc[e];
    si[e] = ic[e];
  }
  __syncthreads();
  for (int64_t size = size_lo; size <= size_hi; size <<= 1) {
    for (int j = (int)(size >> 1 < len >> 1 ? size >> 1 : len >> 1); j > 0; j >>= 1) {
      for (int t = tid; t < len / 2; t += TS_NT) {
        const int lo = (t & (j - 1)) + ((t & ~(j - 1)) << 1), hi = lo + j;
        const bool asc = ((base + lo) & size) == 0;
        const double vl = sv[lo], vh = sv[hi];
        const int64_t il = si[lo], ih = si[hi];
        if (ts_before(vh, ih, vl, il) == asc) {
          sv[lo] = vh;
          sv[hi] = vl;
          si[lo] = ih;
          si[hi] = il;
        }
      }
      __syncthreads();
    }
  }
  for (int e = tid; e < len; e += TS_NT) {
    vc[e] = sv[e];
    ic[e] = si[e];
  }
}

// One step of the network with a stride of at least a chunk: a pair per thread.  Grid (pairs / 256, columns).
__global__ __launch_bounds__(TS_NT) void ts_sort_step_kernel(double* v, int64_t* ix, int64_t P, int64_t size, int64_t j) {
  const int64_t t = (int64_t)blockIdx.x * TS_NT + threadIdx.x;
  if (t >= P / 2) return;
  double* vc = v + (int64_t)blockIdx.y * P;
  int64_t* ic = ix + (int64_t)blockIdx.y * P;
  const int64_t lo = (t & (j - 1)) + ((t & ~(j - 1)) << 1), hi = lo + j;
  const bool asc = (lo & size) == 0;
  const double vl = vc[lo], vh = vc[hi];
  const int64_t il = ic[lo], ih = ic[hi];
  if (ts_before(vh, ih, vl, il) == asc) {
    vc[lo] = vh;
    vc[hi] = vl;
    ic[lo] = ih;
    ic[hi] = il;
  }
}

// the first k of every sorted list to the caller's (C, k) arrays
__global__ void ts_emit_kernel(const double* v, const int64_t* ix, int64_t cols, int64_t P, int64_t k, double* vals,
                               int64_t* rows) {
  const int64_t total = cols * k;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = e / k, t = e - c * k;
    vals[e] = v[c * P + t];
    rows[e] = ix[c * P + t];
  }
}

static int ts_grid(const elfihip_ctx* ctx, int64_t work) {
  const int64_t want = (work + TS_NT - 1) / TS_NT;
  return (int)std::min<int64_t>(std::max<int64_t>(want, 1), (int64_t)std::max(ctx->cu_count, 1) * 8);
}

static int ts_sort(elfihip_ctx* ctx, double* v, int64_t* ix, int cols, int64_t P) {
  hipStream_t st = ctx->stream;
  const int64_t len = std::min<int64_t>(P, TS_SORT_CH);
  const dim3 lgrid((unsigned)(P / len), (unsigned)cols);
  hipLaunchKernelGGL(ts_sort_local_kernel, lgrid, dim3(TS_NT), 0, st, v, ix, P, (int64_t)2, len);
  for (int64_t size = 2 * len; size <= P; size <<= 1) {
    for (int64_t j = size >> 1; j >= len; j >>= 1)
      hipLaunchKernelGGL(ts_sort_step_kernel, dim3((unsigned)((P / 2 + TS_NT - 1) / TS_NT), (unsigned)cols), dim3(TS_NT), 0,
                         st, v, ix, P, size, j);
    hipLaunchKernelGGL(ts_sort_local_kernel, lgrid, dim3(TS_NT), 0, st, v, ix, P, size, size);
  }
  return launch_status(ctx, "survivor sort kernels");
}

static int knn_check(elfihip_ctx* ctx, const void* T, int64_t G, int64_t n, int q, int64_t ldt, int k,
                     const void* entropy) {
  ELFIHIP_REQUIRE(ctx, q >= 1 && q <= TS_MAX_Q, "k-NN entropy: %d dimensions; 1 to %d are supported", q, TS_MAX_Q);
  ELFIHIP_REQUIRE(ctx, k >= 1 && k <= TS_MAX_K, "k-NN entropy: k=%d; 1 to %d are supported", k, TS_MAX_K);
  ELFIHIP_REQUIRE(ctx, G >= 1 && G <= 0x7fffffff && n >= 1 && ldt >= q && (n + TS_NT - 1) / TS_NT <= 65535,
                  "bad shape G=%lld n=%lld q=%d ldt=%lld", (long long)G, (long long)n, q, (long long)ldt);
  ELFIHIP_REQUIRE(ctx, T && entropy, "NULL data pointer");
  return ELFIHIP_OK;
}

// log(pi^(q/2) / Gamma(q/2 + 1)) - psi(k) + log n: the terms that depend on (q, k, n) alone; psi(k) = -gamma + sum_{j<k} 1/j
static double knn_base(int q, int k, int64_t n) {
  long double b = 0.5L * q * logl(3.14159265358979323846264338327950288L) - lgammal(0.5L * q + 1.0L);
  long double psi = -0.57721566490153286060651209008240243L;
  for (int j = 1; j < k; ++j) psi += 1.0L / j;
  return (double)(b - psi + logl((long double)n));
}

static int knn_dev_impl(elfihip_ctx* ctx, const double* dT, int64_t G, int64_t n, int q, int64_t ldt, int k,
                        double* dentropy, double* dkth) {
  const int64_t nb = (n + TS_NT - 1) / TS_NT;
  ELFIHIP_CHECK_HIP(ctx, ctx->sel.reserve((size_t)G * nb * sizeof(double)));
  KnnArgs A;
  A.T = dT;
  A.n = n;
  A.ldt = ldt;
  A.q = q;
  A.k = k;
  A.part = ctx->sel.as<double>();
  A.kth = dkth;
  int rc = ELFIHIP_OK;
  with_constant<4, 8, 16>(k <= 4 ? 4 : (k <= 8 ? 8 : 16), [&](auto KC) {
    with_constant<2, 4, 8, 16, 32>(q <= 2 ? 2 : (q <= 4 ? 4 : (q <= 8 ? 8 : (q <= 16 ? 16 : 32))), [&](auto QC) {
      constexpr int kc = decltype(KC)::value, qc = decltype(QC)::value;
      const size_t lds = (size_t)TS_NT * (qc + 1) * sizeof(double);
      if ((rc = set_lds(ctx, knn_kernel<kc, qc>, lds)) != ELFIHIP_OK) return;
      hipLaunchKernelGGL((knn_kernel<kc, qc>), dim3((unsigned)G, (unsigned)nb), dim3(TS_NT), lds, ctx->stream, A);
    });
  });
  ELFIHIP_TRY(rc);
  ELFIHIP_TRY(launch_status(ctx, "k-NN entropy kernel"));
  hipLaunchKernelGGL(knn_finish_kernel, dim3((unsigned)((G + TS_NT - 1) / TS_NT)), dim3(TS_NT), 0, ctx->stream,
                     (const double*)A.part, G, nb, knn_base(q, k, n), (double)q / (double)n, dentropy);
  return launch_status(ctx, "k-NN entropy finish kernel");
}

static int mrsse_check(elfihip_ctx* ctx, const void* T, int64_t G, int64_t n, int q, int64_t ldt, const void* Cl,
                       int64_t J, int64_t ldc, const void* out) {
  ELFIHIP_REQUIRE(ctx, q >= 1 && q <= TS_MAX_Q, "MRSSE: %d dimensions; 1 to %d are supported", q, TS_MAX_Q);
  ELFIHIP_REQUIRE(ctx, G >= 1 && G <= 0x7fffffff && n >= 1 && J >= 1 && J <= 65535 && ldt >= q && ldc >= q,
                  "bad shape G=%lld n=%lld J=%lld q=%d ldt=%lld ldc=%lld", (long long)G, (long long)n, (long long)J, q,
                  (long long)ldt, (long long)ldc);
  ELFIHIP_REQUIRE(ctx, T && Cl && out, "NULL data pointer");
  return ELFIHIP_OK;
}

static int mrsse_dev_impl(elfihip_ctx* ctx, const double* dT, int64_t G, int64_t n, int q, int64_t ldt, const double* dC,
                          int64_t J, int64_t ldc, double* dout) {
  ELFIHIP_CHECK_HIP(ctx, ctx->sel.reserve((size_t)G * J * sizeof(double)));
  double* root = ctx->sel.as<double>();
  hipLaunchKernelGGL(mrsse_root_kernel, dim3((unsigned)G, (unsigned)J), dim3(TS_NT), 0, ctx->stream, dT, n, q, ldt, dC, ldc,
                     root);
  ELFIHIP_TRY(launch_status(ctx, "MRSSE kernel"));
  hipLaunchKernelGGL(mrsse_finish_kernel, dim3((unsigned)((G + TS_NT - 1) / TS_NT)), dim3(TS_NT), 0, ctx->stream,
                     (const double*)root, G, J, dout);
  return launch_status(ctx, "MRSSE finish kernel");
}

// masks is a host array in both forms: it is checked here, before anything is launched
static int subset_check(elfihip_ctx* ctx, const void* X, int64_t n, int m, int64_t ldx, const void* y, const double* masks,
                        int64_t C, int64_t k, const void* vals, const void* rows) {
  ELFIHIP_REQUIRE(ctx, n >= 1 && m >= 1 && ldx >= m && C >= 1 && C <= 0x7fffffff && k >= 1,
                  "bad shape n=%lld m=%d ldx=%lld C=%lld k=%lld", (long long)n, m, (long long)ldx, (long long)C,
                  (long long)k);
  ELFIHIP_REQUIRE(ctx, X && y && masks && vals && rows, "NULL data pointer");
  for (int64_t c = 0; c < C; ++c) {
    bool any = false;
    for (int j = 0; j < m; ++j) {
      const double w = masks[c * m + j];
      ELFIHIP_REQUIRE(ctx, w == 0.0 || w == 1.0, "mask %lld, entry %d is %g: a mask holds 0 and 1", (long long)c, j, w);
      any = any || w == 1.0;
    }
    ELFIHIP_REQUIRE(ctx, any, "mask %lld selects no column", (long long)c);
  }
  return ELFIHIP_OK;
}

// dX, dy, dvals, drows on the device; masks on the host (checked).  Synchronises once per block of combinations: the
// resident selection reports a timed-out grid barrier through a flag (topk.hip), and a column whose flag is set is
// selected again by the nine-launch form before the block is sorted.
static int subset_dev_impl(elfihip_ctx* ctx, const double* dX, int64_t n, int m, int64_t ldx, const double* dy,
                           const double* masks, int64_t C, int64_t k, double* dvals, int64_t* drows) {
  hipStream_t st = ctx->stream;
  if (k > n) k = n;
  int64_t P = 2;
  while (P < k) P <<= 1;
  // a block: (n, Cb) distances, (Cb, P) survivors and rows, Cb time-out flags
  const size_t per_col = (size_t)n * sizeof(double) + (size_t)P * (sizeof(double) + sizeof(int64_t)) + 8;
  const int Cmax = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(kMaxK, C), (int64_t)(TS_BLOCK_BYTES / per_col)));
  ELFIHIP_CHECK_HIP(ctx, ctx->par.reserve((size_t)C * m * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->sel.reserve((size_t)Cmax * per_col));
  double* dM = ctx->par.as<double>();
  // pageable host memory: the copy is done with it when hipMemcpyAsync returns (common.hpp: pageable uploads)
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dM, masks, (size_t)C * m * sizeof(double), hipMemcpyHostToDevice, st));
  double* dD = ctx->sel.as<double>();
  double* sv = dD + (size_t)n * Cmax;
  int64_t* si = reinterpret_cast<int64_t*>(sv + (size_t)Cmax * P);
  unsigned* flags = reinterpret_cast<unsigned*>(si + (size_t)Cmax * P);
  std::vector<unsigned> hflags((size_t)Cmax);
  for (int64_t c0 = 0; c0 < C; c0 += Cmax) {
    const int Cb = (int)std::min<int64_t>(Cmax, C - c0);
    ELFIHIP_TRY(dist_multiw_dev_impl(ctx, dX, n, m, ldx, dy, dM + c0 * m, Cb, dD, nullptr, nullptr));
    if (P > k) {
      hipLaunchKernelGGL(ts_pad_kernel, dim3(ts_grid(ctx, Cb * (P - k))), dim3(TS_NT), 0, st, sv, si, (int64_t)Cb, P, k);
      ELFIHIP_TRY(launch_status(ctx, "survivor padding kernel"));
    }
    ELFIHIP_CHECK_HIP(ctx, hipMemsetAsync(flags, 0, (size_t)Cb * sizeof(unsigned), st));
    bool resident = false;
    for (int c = 0; c < Cb; ++c) {
      ELFIHIP_TRY(topk_dev_impl(ctx, dD + c, n, Cb, k, sv + (size_t)c * P, si + (size_t)c * P, false));
      if (const void* err = topk_resident_err_dev(ctx)) {
        resident = true;
        ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(flags + c, err, sizeof(unsigned), hipMemcpyDeviceToDevice, st));
      }
    }
    if (resident) {
      ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(hflags.data(), flags, (size_t)Cb * sizeof(unsigned), hipMemcpyDeviceToHost, st));
      ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
      for (int c = 0; c < Cb; ++c)
        if (hflags[(size_t)c])
          ELFIHIP_TRY(topk_dev_impl(ctx, dD + c, n, Cb, k, sv + (size_t)c * P, si + (size_t)c * P, true));
    }
    ELFIHIP_TRY(ts_sort(ctx, sv, si, Cb, P));
    hipLaunchKernelGGL(ts_emit_kernel, dim3(ts_grid(ctx, Cb * k)), dim3(TS_NT), 0, st, (const double*)sv,
                       (const int64_t*)si, (int64_t)Cb, P, k, dvals + c0 * k, drows + c0 * k);
    ELFIHIP_TRY(launch_status(ctx, "survivor emit kernel"));
  }
  return ELFIHIP_OK;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_knn_entropy_dev(elfihip_ctx* ctx, const double* dT, int64_t G, int64_t n, int q, int64_t ldt, int k,
                            double* dentropy, double* dkth) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(knn_check(ctx, dT, G, n, q, ldt, k, dentropy));
  DeviceGuard g(ctx->device);
  return knn_dev_impl(ctx, dT, G, n, q, ldt, k, dentropy, dkth);
}

int elfihip_knn_entropy(elfihip_ctx* ctx, const double* T, int64_t G, int64_t n, int q, int64_t ldt, int k,
                        double* entropy, double* kth) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(knn_check(ctx, T, G, n, q, ldt, k, entropy));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)G * (size_t)n;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(rows * q * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(((size_t)G + rows) * sizeof(double)));
  double* dT = ctx->in.as<double>();
  double* dE = ctx->out.as<double>();
  double* dK = dE + G;
  ELFIHIP_TRY(upload_rows(ctx, dT, T, rows, q, ldt));
  ELFIHIP_TRY(knn_dev_impl(ctx, dT, G, n, q, q, k, dE, kth ? dK : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(entropy, dE, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, st));
  if (kth) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(kth, dK, rows * sizeof(double), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

int elfihip_mrsse_dev(elfihip_ctx* ctx, const double* dT, int64_t G, int64_t n, int q, int64_t ldt,
                      const double* dclosest, int64_t J, int64_t ldc, double* dmrsse) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(mrsse_check(ctx, dT, G, n, q, ldt, dclosest, J, ldc, dmrsse));
  DeviceGuard g(ctx->device);
  return mrsse_dev_impl(ctx, dT, G, n, q, ldt, dclosest, J, ldc, dmrsse);
}

int elfihip_mrsse(elfihip_ctx* ctx, const double* T, int64_t G, int64_t n, int q, int64_t ldt, const double* closest,
                  int64_t J, int64_t ldc, double* mrsse) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(mrsse_check(ctx, T, G, n, q, ldt, closest, J, ldc, mrsse));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const size_t rows = (size_t)G * (size_t)n;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((rows + (size_t)J) * q * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((size_t)G * sizeof(double)));
  double* dT = ctx->in.as<double>();
  double* dC = dT + rows * q;
  double* dO = ctx->out.as<double>();
  ELFIHIP_TRY(upload_rows(ctx, dT, T, rows, q, ldt));
  ELFIHIP_TRY(upload_rows(ctx, dC, closest, (size_t)J, q, ldc));
  ELFIHIP_TRY(mrsse_dev_impl(ctx, dT, G, n, q, q, dC, J, q, dO));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(mrsse, dO, (size_t)G * sizeof(double), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

int elfihip_subset_best_dev(elfihip_ctx* ctx, const double* dX, int64_t n, int m, int64_t ldx, const double* dy,
                            const double* masks, int64_t C, int64_t k, double* dvals, int64_t* drows) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(subset_check(ctx, dX, n, m, ldx, dy, masks, C, k, dvals, drows));
  DeviceGuard g(ctx->device);
  return subset_dev_impl(ctx, dX, n, m, ldx, dy, masks, C, k, dvals, drows);
}

int elfihip_subset_best(elfihip_ctx* ctx, const double* X, int64_t n, int m, int64_t ldx, const double* y,
                        const double* masks, int64_t C, int64_t k, double* vals, int64_t* rows) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(subset_check(ctx, X, n, m, ldx, y, masks, C, k, vals, rows));
  DeviceGuard g(ctx->device);
  hipStream_t st = ctx->stream;
  const int64_t ke = k > n ? n : k;
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(((size_t)n * m + (size_t)m) * sizeof(double)));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((size_t)C * ke * (sizeof(double) + sizeof(int64_t))));
  double* dX = ctx->in.as<double>();
  double* dy = dX + (size_t)n * m;
  double* dv = ctx->out.as<double>();
  int64_t* dr = reinterpret_cast<int64_t*>(dv + (size_t)C * ke);
  ELFIHIP_TRY(upload_rows(ctx, dX, X, (size_t)n, m, ldx));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dy, y, (size_t)m * sizeof(double), hipMemcpyHostToDevice, st));
  ELFIHIP_TRY(subset_dev_impl(ctx, dX, n, m, m, dy, masks, C, k, dv, dr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(vals, dv, (size_t)C * ke * sizeof(double), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(rows, dr, (size_t)C * ke * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(st));
  return ELFIHIP_OK;
}

}  // extern "C"
