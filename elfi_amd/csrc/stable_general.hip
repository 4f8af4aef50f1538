// General alpha-stable variates into memory: out[e] = stable_general(alpha[e], beta[e], loc[e], scale[e], s0, TH, W) with TH
// and W of Philox counter e of (seed, stream) -- stable_angle_expo, the draw of the symmetric sampler -- or a caller's angles
// and exponentials (stable.hpp holds the rule).  One element per lane.
#include "common.hpp"

#include <algorithm>

#include "stable.hpp"

#pragma clang fp contract(off)

namespace elfihip {

__global__ __launch_bounds__(256) void stable_general_kernel(uint64_t seed, uint64_t stream, int64_t n, int s0,
                                                             const double* __restrict__ alpha, const double* __restrict__ beta,
                                                             const double* __restrict__ loc, const double* __restrict__ scale,
                                                             const double* __restrict__ angle, const double* __restrict__ expo,
                                                             double* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += step) {
    double TH, W;
    if (angle) {
      TH = angle[e];
      W = expo[e];
    } else {
      stable_angle_expo(seed, stream, (uint64_t)e, TH, W);
    }
    out[e] = stable_general(alpha[e], beta[e], loc[e], scale[e], s0 != 0, TH, W);
  }
}

static int stable_general_check(elfihip_ctx* ctx, int64_t n, int s0, const void* alpha, const void* beta, const void* loc,
                                const void* scale, const void* angle, const void* expo, const void* out) {
  ELFIHIP_REQUIRE(ctx, n >= 0 && (n == 0 || (alpha && beta && loc && scale && out)), "bad arguments");
  ELFIHIP_REQUIRE(ctx, s0 == 0 || s0 == 1, "the parameterisation is 0 (S1) or 1 (S0)");
  ELFIHIP_REQUIRE(ctx, (angle == nullptr) == (expo == nullptr), "angles and exponentials are given together or not at all");
  return ELFIHIP_OK;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_stable_general_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, int s0, const double* dalpha,
                               const double* dbeta, const double* dloc, const double* dscale, const double* dangle,
                               const double* dexpo, double* dout) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(stable_general_check(ctx, n, s0, dalpha, dbeta, dloc, dscale, dangle, dexpo, dout));
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->cu_count * 16);
  hipLaunchKernelGGL(stable_general_kernel, dim3(grid), dim3(256), 0, ctx->stream, seed, stream, n, s0, dalpha, dbeta, dloc,
                     dscale, dangle, dexpo, dout);
  return launch_status(ctx, "stable_general_kernel");
}

int elfihip_stable_general(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, int s0, const double* alpha,
                           const double* beta, const double* loc, const double* scale, const double* angle, const double* expo,
                           double* out) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(stable_general_check(ctx, n, s0, alpha, beta, loc, scale, angle, expo, out));
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const size_t bytes = (size_t)n * sizeof(double);
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(6 * bytes));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(bytes));
  double* din = ctx->in.as<double>();
  double* dout = ctx->out.as<double>();
  const double* src[6] = {alpha, beta, loc, scale, angle, expo};
  for (int k = 0; k < (angle ? 6 : 4); ++k)
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(din + (size_t)k * n, src[k], bytes, hipMemcpyHostToDevice, ctx->stream));
  const size_t N = (size_t)n;
  ELFIHIP_TRY(elfihip_stable_general_dev(ctx, seed, stream, n, s0, din, din + N, din + 2 * N, din + 3 * N,
                                         angle ? din + 4 * N : nullptr, angle ? din + 5 * N : nullptr, dout));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
