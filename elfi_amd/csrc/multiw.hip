// K weighted euclidean distances per row (AdaptiveDistance.nested_distance) for gfx950 (MI355X): one pass over the rows
// for all K weight vectors, out (n, K).  Three forms: narrow rows in registers, the pipelined tile, the plain tile.
// FMA contraction is off in this file, as in the other distance kernels (distance.hip).
#include "internal.hpp"
#include "dist_launch.hpp"

#pragma clang fp contract(off)

namespace elfihip {

// Pipelined K-weight form (AdaptiveDistance.nested_distance).
template <int U>
__global__ __launch_bounds__(256) void dist_multiw_pipe_kernel(RowArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int T = blockDim.x, tid = threadIdx.x, m = A.m, K = A.K;
  double* tile = lds;
  const int R = A.R;
  double* ys = tile + (size_t)R * A.mp;
  double* ws = ys + m;  // (K, m)
  for (int j = tid; j < m; j += T) ys[j] = A.y[j];
  for (int j = tid; j < K * m; j += T) ws[j] = A.aux[j];
  const int64_t ntiles = (A.n + R - 1) / R;
  const double thr = A.F.thr ? *A.F.thr : 0.0;   // fused selection, by the LAST nested distance (samplers.py:233)
  double2 v[U];
  int64_t t = blockIdx.x;
  if (t < ntiles) tile_fetch<U>(A, t * R, (int)((A.n - t * R) < R ? (A.n - t * R) : R), v);
  for (; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * R;
    const int rows = (int)((A.n - row0) < R ? (A.n - row0) : R);
    __syncthreads();
    tile_commit<U>(A, tile, rows, v);
    const int64_t tn = t + gridDim.x;
    if (tn < ntiles) tile_fetch<U>(A, tn * R, (int)((A.n - tn * R) < R ? (A.n - tn * R) : R), v);
    __syncthreads();
    double dlast = 0.0;
    if (tid < rows) {
      const double* row = tile + (size_t)tid * A.mp;
      // four weight vectors per sweep over the row: (x-y)^2 is formed once per element and feeds four
      // independent left-to-right sums (each still in cdist's order)
      for (int k0 = 0; k0 < K; k0 += 4) {
        const int kn = K - k0 < 4 ? K - k0 : 4;
        const double* w0 = ws + (size_t)k0 * m;
        const double* w1 = ws + (size_t)(k0 + (kn > 1 ? 1 : 0)) * m;
        const double* w2 = ws + (size_t)(k0 + (kn > 2 ? 2 : 0)) * m;
        const double* w3 = ws + (size_t)(k0 + (kn > 3 ? 3 : 0)) * m;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
          const double d = row[j] - ys[j];
          const double d2 = d * d;
          s0 = s0 + w0[j] * d2;
          s1 = s1 + w1[j] * d2;
          s2 = s2 + w2[j] * d2;
          s3 = s3 + w3[j] * d2;
        }
        double* o = A.out + (row0 + tid) * K + k0;
        const double r0 = sqrt(s0), r1 = sqrt(s1), r2 = sqrt(s2), r3 = sqrt(s3);
        o[0] = r0;
        if (kn > 1) o[1] = r1;
        if (kn > 2) o[2] = r2;
        if (kn > 3) o[3] = r3;
        dlast = kn > 3 ? r3 : (kn > 2 ? r2 : (kn > 1 ? r1 : r0));
      }
    }
    if (A.F.thr) reject_offer(A.F, tid < rows && dlast < thr, dlast, A.F.row_base + row0 + tid);
  }
}

// K weighted euclidean distances per row (AdaptiveDistance.nested_distance); out (n,K).
template <int U>
__global__ void dist_multiw_kernel(RowArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int T = blockDim.x, tid = threadIdx.x, m = A.m, K = A.K;
  double* tile = lds;
  double* ys = tile + (size_t)T * A.mp;
  double* ws = ys + m;  // (K, m)
  for (int j = tid; j < m; j += T) ys[j] = A.y[j];
  for (int j = tid; j < K * m; j += T) ws[j] = A.aux[j];
  const int64_t ntiles = (A.n + T - 1) / T;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * T;
    const int rows = (int)((A.n - row0) < T ? (A.n - row0) : T);
    __syncthreads();
    load_tile<U>(A, tile, row0, rows);
    __syncthreads();
    if (tid < rows) {
      const double* row = tile + (size_t)tid * A.mp;
      // four weight vectors per sweep over the row: (x-y)^2 is formed once per element and feeds four
      // independent left-to-right sums (each still in cdist's order)
      for (int k0 = 0; k0 < K; k0 += 4) {
        const int kn = K - k0 < 4 ? K - k0 : 4;
        const double* w0 = ws + (size_t)k0 * m;
        const double* w1 = ws + (size_t)(k0 + (kn > 1 ? 1 : 0)) * m;
        const double* w2 = ws + (size_t)(k0 + (kn > 2 ? 2 : 0)) * m;
        const double* w3 = ws + (size_t)(k0 + (kn > 3 ? 3 : 0)) * m;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 4
        for (int j = 0; j < m; ++j) {
          const double d = row[j] - ys[j];
          const double d2 = d * d;
          s0 = s0 + w0[j] * d2;
          s1 = s1 + w1[j] * d2;
          s2 = s2 + w2[j] * d2;
          s3 = s3 + w3[j] * d2;
        }
        double* o = A.out + (row0 + tid) * K + k0;
        o[0] = sqrt(s0);
        if (kn > 1) o[1] = sqrt(s1);
        if (kn > 2) o[2] = sqrt(s2);
        if (kn > 3) o[3] = sqrt(s3);
      }
    }
  }
}

// K weighted euclidean distances per narrow row (AdaptiveDistance.nested_distance): the weights of up to 8 vectors in
// registers, every sum left to right as dist_multiw_pipe_kernel forms it (bit-identical); the K results of a row are
// adjacent in `out` (a wave writes 512 K contiguous bytes).
template <int M, int U>
__global__ __launch_bounds__(256) void dist_multiw_narrow_kernel(RowArgs A) {
  constexpr int KMAX = 8;
  __shared__ __align__(16) double stage_all[4 * 64 * KMAX];   // per wave: the K results of 64 rows on their way to contiguous stores
  const int tid = threadIdx.x, K = A.K;
  double* stage = stage_all + (tid >> 6) * 64 * KMAX;
  const bool staged = (reinterpret_cast<uintptr_t>(A.out) & 15u) == 0;
  double yv[M], wv[KMAX][M];
#pragma unroll
  for (int j = 0; j < M; ++j) yv[j] = A.y[j];
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int j = 0; j < M; ++j) wv[k][j] = k < K ? A.aux[k * M + j] : 0.0;
  const double thr = A.F.thr ? *A.F.thr : 0.0;   // fused selection, by the LAST nested distance (samplers.py:233)
  const int64_t per = 256 * U;
  for (int64_t base = (int64_t)blockIdx.x * per; base < A.n; base += (int64_t)gridDim.x * per) {
    double x[U][M];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = base + u * 256 + tid;
      narrow_load<M>(A, r < A.n ? r : A.n - 1, x[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = base + u * 256 + tid;
      double d2[M];
#pragma unroll
      for (int j = 0; j < M; ++j) {
        const double d = x[u][j] - yv[j];
        d2[j] = d * d;
      }
      double dlast = 0.0, dk[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        dk[k] = 0.0;
        if (k < K) {
          double sk = 0.0;
#pragma unroll
          for (int j = 0; j < M; ++j) sk = sk + wv[k][j] * d2[j];
          dlast = sqrt(sk);
          dk[k] = dlast;
          if (!staged && r < A.n) A.out[r * K + k] = dlast;
        }
      }
      if (staged) {
        const int64_t r0 = base + u * 256 + (tid & ~63);   // first row of this wave's 64
        const int64_t left = A.n - r0;
        if (left > 0) wave_store_rows<KMAX>(stage, A.out + r0 * K, dk, K, tid & 63, left < 64 ? (int)left : 64);
      }
      if (A.F.thr) reject_offer(A.F, r < A.n && dlast < thr, dlast, A.F.row_base + r);
    }
  }
}

int dist_multiw_dev_impl(elfihip_ctx* ctx, const double* dX, int64_t n, int m, int64_t ldx, const double* dy,
                         const double* dW, int K, double* dout, const RejectFilter* F, bool* filtered) {
  if (filtered) *filtered = false;
  ELFIHIP_REQUIRE(ctx, n >= 0 && m >= 1, "bad shape n=%lld m=%d", (long long)n, m);
  ELFIHIP_REQUIRE(ctx, K >= 1 && K <= kMaxK, "K=%d outside [1,%d]", K, kMaxK);
  ELFIHIP_REQUIRE(ctx, ldx >= m, "ldx (%lld) < m (%d)", (long long)ldx, m);
  ELFIHIP_REQUIRE(ctx, n == 0 || (dX && dy && dW && dout), "NULL data pointer");
  if (n == 0) return ELFIHIP_OK;
  RowArgs A = make_row_args(ctx, dX, n, m, ldx, dy, dW, 2.0, dout);
  A.K = K;
  if (F) A.F = *F;
  if (narrow_rows(ctx, A) && K <= 8) {
    if (filtered) *filtered = A.F.thr != nullptr;
    return launch_narrow(ctx, A, "dist_multiw_narrow_kernel",
                         [](auto M) { return dist_multiw_narrow_kernel<decltype(M)::value, kNarrowU>; });
  }
  size_t lds;
  int T = pick_block(m, (size_t)m + (size_t)K * m, &lds);
  ELFIHIP_REQUIRE(ctx, lds <= 160 * 1024, "m=%d with K=%d weight vectors does not fit LDS", m, K);
  const int g = grid_for(ctx, (n + T - 1) / T, lds, T);
  if (A.vec2 && m <= 128) {
    const int Tp = 128, U = 16;
    int R = 2 * Tp * U / m;
    if (R > Tp) R = Tp;
    A.R = R;
    const size_t ldsp = ((size_t)R * A.mp + (size_t)m + (size_t)K * m) * sizeof(double);
    if (ldsp <= 64 * 1024) {
      const int gp = grid_for(ctx, (n + R - 1) / R, ldsp, Tp);
      hipLaunchKernelGGL((dist_multiw_pipe_kernel<16>), dim3(gp), dim3(Tp), ldsp, ctx->stream, A);
      if (filtered) *filtered = A.F.thr != nullptr;
      return launch_status(ctx, "dist_multiw_pipe_kernel");
    }
  }
  ELFIHIP_TRY(set_lds(ctx, dist_multiw_kernel<8>, lds));
  hipLaunchKernelGGL((dist_multiw_kernel<8>), dim3(g), dim3(T), lds, ctx->stream, A);
  return launch_status(ctx, "dist_multiw_kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_dist_multiw_dev(elfihip_ctx* ctx, const double* dX, int64_t n, int m, int64_t ldx,
                            const double* dy, const double* dW, int K, double* dout) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return dist_multiw_dev_impl(ctx, dX, n, m, ldx, dy, dW, K, dout, nullptr, nullptr);
}

int elfihip_dist_multiw(elfihip_ctx* ctx, const double* X, int64_t n, int m, int64_t ldx, const double* y,
                        const double* W, int K, double* out) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 0 && m >= 1 && ldx >= m, "bad shape n=%lld m=%d ldx=%lld", (long long)n, m,
                  (long long)ldx);
  ELFIHIP_REQUIRE(ctx, K >= 1 && K <= kMaxK, "K=%d outside [1,%d]", K, kMaxK);
  ELFIHIP_REQUIRE(ctx, y && W && (n == 0 || (X && out)), "NULL data pointer");
  DeviceGuard g(ctx->device);
  double *dX, *dy, *dW;
  ELFIHIP_TRY(stage_row_call(ctx, X, n, m, ldx, y, W, (size_t)K * m, K, &dX, &dy, &dW));
  ELFIHIP_TRY(dist_multiw_dev_impl(ctx, dX, n, m, m, dy, dW, K, ctx->out.as<double>(), nullptr, nullptr));
  return finish_host_call(ctx, out, n, K, true);
}

}  // extern "C"
