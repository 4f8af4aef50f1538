// Symmetric alpha-stable variates into memory: out[e] = stable_draw(alpha[e], scale[e], seed, stream, e), or the transform
// alone on a caller's angles and exponentials (stable.hpp holds the rule).  One element per lane.
#include "common.hpp"

#include <algorithm>

#include "stable.hpp"

#pragma clang fp contract(off)

namespace elfihip {

__global__ __launch_bounds__(256) void stable_kernel(uint64_t seed, uint64_t stream, int64_t n, const double* __restrict__ alpha,
                                                     const double* __restrict__ scale, const double* __restrict__ angle,
                                                     const double* __restrict__ expo, double* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += step)
    out[e] = angle ? stable_transform(alpha[e], scale[e], angle[e], expo[e]) : stable_draw(alpha[e], scale[e], seed, stream, (uint64_t)e);
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_stable_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, const double* dalpha, const double* dscale,
                       const double* dangle, const double* dexpo, double* dout) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 0 && (n == 0 || (dalpha && dscale && dout)), "bad arguments");
  ELFIHIP_REQUIRE(ctx, (dangle == nullptr) == (dexpo == nullptr), "angles and exponentials are given together or not at all");
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->cu_count * 16);
  hipLaunchKernelGGL(stable_kernel, dim3(grid), dim3(256), 0, ctx->stream, seed, stream, n, dalpha, dscale, dangle, dexpo, dout);
  return launch_status(ctx, "stable_kernel");
}

int elfihip_stable(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, const double* alpha, const double* scale,
                   const double* angle, const double* expo, double* out) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 0 && (n == 0 || (alpha && scale && out)), "bad arguments");
  ELFIHIP_REQUIRE(ctx, (angle == nullptr) == (expo == nullptr), "angles and exponentials are given together or not at all");
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const size_t bytes = (size_t)n * sizeof(double);
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(4 * bytes));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(bytes));
  double* din = ctx->in.as<double>();
  double* dout = ctx->out.as<double>();
  const double* src[4] = {alpha, scale, angle, expo};
  for (int k = 0; k < (angle ? 4 : 2); ++k)
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(din + (size_t)k * n, src[k], bytes, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(elfihip_stable_dev(ctx, seed, stream, n, din, din + n, angle ? din + 2 * (size_t)n : nullptr,
                                 angle ? din + 3 * (size_t)n : nullptr, dout));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
