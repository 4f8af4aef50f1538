// Poisson variates into memory: out[e] = poisson_draw(lam[e], seed, stream, e) (poisson.hpp holds the rule and its bounds).
// One element per lane; a wavefront's lanes hold 64 unrelated intensities here, so they wait for the slowest branch among
// them -- the fused Ricker kernel (series.hip) orders its elements so that neighbours share a branch.
#include "common.hpp"

#include <algorithm>

#include "poisson.hpp"

#pragma clang fp contract(off)

namespace elfihip {

__global__ __launch_bounds__(256) void poisson_kernel(uint64_t seed, uint64_t stream, int64_t n, const double* __restrict__ lam,
                                                      double* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += step)
    out[e] = poisson_draw(lam[e], seed, stream, (uint64_t)e);
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_poisson_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, const double* dlam, double* dout) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 0 && (n == 0 || (dlam && dout)), "bad arguments");
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, (int64_t)ctx->cu_count * 16);
  hipLaunchKernelGGL(poisson_kernel, dim3(grid), dim3(256), 0, ctx->stream, seed, stream, n, dlam, dout);
  return launch_status(ctx, "poisson_kernel");
}

int elfihip_poisson(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, const double* lam, double* out) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 0 && (n == 0 || (lam && out)), "bad arguments");
  if (n == 0) return ELFIHIP_OK;
  DeviceGuard g(ctx->device);
  const size_t bytes = (size_t)n * sizeof(double);
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(bytes));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(bytes));
  double* dlam = ctx->in.as<double>();
  double* dout = ctx->out.as<double>();
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dlam, lam, bytes, hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(elfihip_poisson_dev(ctx, seed, stream, n, dlam, dout));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
