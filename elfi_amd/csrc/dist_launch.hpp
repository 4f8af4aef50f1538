// What the distance translation units (distance.hip, mahalanobis.hip, multiw.hip) share on the host side: launch shapes,
// the argument constructors, the narrow-row form's loader and selection, and the host-pointer entry points' staging and tail.
#pragma once

#include <algorithm>

#include "common.hpp"
#include "tile_stream.hpp"

namespace elfihip {

constexpr int kMaxTileM = 299;  // widest row the LDS-tile kernel takes (64 rows * 301 * 8 B < 160 KiB)
constexpr int kMaxK = 64;

static inline int pick_block(int m, size_t extra_doubles, size_t* lds_bytes) {
  const int mp = m | 1;
  const int cand[3] = {256, 128, 64};
  for (int c = 0; c < 3; ++c) {
    size_t b = ((size_t)cand[c] * mp + extra_doubles) * sizeof(double);
    if (b <= 41 * 1024 || cand[c] == 64) {
      *lds_bytes = b;
      return cand[c];
    }
  }
  return 64;
}

static inline int grid_for(const elfihip_ctx* ctx, int64_t ntiles, size_t lds_bytes, int T) {
  int per_cu = (int)((160 * 1024) / (lds_bytes ? lds_bytes : 1));
  int by_waves = 32 / (T / 64);
  if (per_cu > by_waves) per_cu = by_waves;
  if (per_cu > 8) per_cu = 8;
  if (per_cu < 1) per_cu = 1;
  int64_t g = (int64_t)ctx->cu_count * per_cu;
  if (g > ntiles) g = ntiles;
  if (g < 1) g = 1;
  return (int)g;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// RowArgs / ColArgs nt: non-temporal loads of rows and columns that are read once (form 1: plain loads, for comparison)
static inline int stream_nt(const elfihip_ctx* ctx) { return ctx->dist_form != 1; }

static inline RowArgs make_row_args(const elfihip_ctx* ctx, const double* dX, int64_t n, int m, int64_t ldx,
                                    const double* dy, const double* daux, double p, double* dout) {
  RowArgs A;
  A.X = dX;
  A.n = n;
  A.ldx = ldx;
  A.y = dy;
  A.aux = daux;
  A.out = dout;
  A.p = p;
  A.inv_p = p != 0.0 ? 1.0 / p : 0.0;
  A.m = m;
  A.mp = m | 1;
  A.K = A.R = 0;
  A.nt = stream_nt(ctx);
  A.F = RejectFilter{nullptr, nullptr, nullptr, nullptr, 0u, 0ll};
  A.M = RejectMergeJob{};
  A.vec2 = (m % 2 == 0) && (ldx % 2 == 0) && aligned16(dX);
  A.div_h = make_fastdiv((uint32_t)(A.vec2 ? m / 2 : m));
  return A;
}

// ---- narrow rows (round 6): m = 2 or 4 summaries, 16-byte aligned ----------------------------------------------------------
// A row is one or two 16-byte granules: nothing to stage.  The tile kernels put 128 rows (2 KiB at m = 2) through LDS
// per pair of barriers with one lane in four idle and were launch- and barrier-bound at configs[0]'s own shape (4 10^6 x 2:
// minkowski 0.23, mahalanobis 0.28, the K-weight form 0.26 of HBM -- profiles/r05_kernel_table.md).  Here lane r of a
// 256-thread workgroup OWNS rows r, r + 256, ...: U rows (U 16- or 32-byte non-temporal loads) in flight per lane,
// consecutive lanes on consecutive rows (a wave-instruction covers 1 KiB of contiguous rows), the row summed left to right in
// registers exactly as the tile kernels sum it (bit-identical), one 8-byte store per row (512 contiguous bytes per wave).
#if defined(__HIPCC__)
template <int M>
__device__ __forceinline__ void narrow_load(const RowArgs& A, int64_t r, double (&x)[M]) {
  typedef double v2d_nt __attribute__((ext_vector_type(2)));
  const v2d_nt* src = reinterpret_cast<const v2d_nt*>(A.X + r * A.ldx);
#pragma unroll
  for (int h = 0; h < M / 2; ++h) {
    const v2d_nt t = __builtin_nontemporal_load(src + h);
    x[2 * h] = t.x;
    x[2 * h + 1] = t.y;
  }
}
#endif

constexpr int kNarrowU = 4;   // rows in flight per lane

static inline bool narrow_rows(const elfihip_ctx* ctx, const RowArgs& A) {
  return A.vec2 && (A.m == 2 || A.m == 4) && ctx->dist_form != 1;   // (form 1: the tile kernels of rounds 1-5, for comparison)
}
static inline unsigned narrow_grid(const elfihip_ctx* ctx, int64_t n, int U) {
  int64_t g = (n + 256 * U - 1) / (256 * U), cap = (int64_t)ctx->cu_count * 8;
  if (g > cap) g = cap;
  return (unsigned)(g < 1 ? 1 : g);
}
// Launches the narrow form of a kernel family: kernel_of(M) is the instance for rows of M = 2 or 4 doubles.
template <class KernelOf>
static inline int launch_narrow(elfihip_ctx* ctx, const RowArgs& A, const char* name, KernelOf kernel_of) {
  with_constant<2, 4>(A.m, [&](auto M) {
    hipLaunchKernelGGL(kernel_of(M), dim3(narrow_grid(ctx, A.n, kNarrowU)), dim3(256), 0, ctx->stream, A);
  });
  return launch_status(ctx, name);
}

// ---- host-pointer entry points: stage, launch, copy back, synchronise ---------------
static inline int stage_params(elfihip_ctx* ctx, const double* y, const double* aux, int m, size_t naux,
                               double** dy, double** daux) {
  ELFIHIP_CHECK_HIP(ctx, ctx->par.reserve(((size_t)m + naux) * sizeof(double)));
  *dy = ctx->par.as<double>();
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(*dy, y, (size_t)m * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  *daux = nullptr;
  if (aux) {
    *daux = *dy + m;
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(*daux, aux, naux * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  }
  return ELFIHIP_OK;
}

static inline int stage_rows(elfihip_ctx* ctx, const double* X, int64_t n, int m, int64_t ldx, double** dX) {
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((size_t)n * m * sizeof(double)));
  *dX = ctx->in.as<double>();
  if (n == 0) return ELFIHIP_OK;
  return upload_rows(ctx, *dX, X, (size_t)n, m, ldx);
}

// The row-major host entry points' preamble: y, aux (naux doubles, or NULL), the rows at pitch m, room for n x cols results
static inline int stage_row_call(elfihip_ctx* ctx, const double* X, int64_t n, int m, int64_t ldx, const double* y,
                                 const double* aux, size_t naux, int cols, double** dX, double** dy, double** daux) {
  ELFIHIP_TRY(stage_params(ctx, y, aux, m, aux ? naux : 0, dy, daux));
  ELFIHIP_TRY(stage_rows(ctx, X, n, m, ldx, dX));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((size_t)(n ? n : 1) * cols * sizeof(double)));
  return ELFIHIP_OK;
}

// The tail of every host entry point: the n x cols results in ctx->out are kept on the device for the sampler (keep;
// see keep_distances), copied to `out` (unless NULL) and the stream is synchronised.
static inline int finish_host_call(elfihip_ctx* ctx, double* out, int64_t n, int cols, bool keep) {
  if (keep) ELFIHIP_TRY(keep_distances(ctx, ctx->out.as<double>(), n, cols));
  if (n && out)
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(out, ctx->out.p, (size_t)n * cols * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // namespace elfihip
