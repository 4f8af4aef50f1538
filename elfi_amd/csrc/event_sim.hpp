// What the event-driven simulators share (gillespie.hip, daycare.hip, scratch_assay.hip, bdm.hip): a persistent grid of
// one-wavefront workgroups that take their work units from a counter in device memory, because the events of a unit are not
// known in advance.  The counter is the first word of the context's `sim` buffer; a model's own work space follows its
// 256-byte head.
#pragma once

#include <algorithm>
#include <cmath>

#include "common.hpp"

namespace elfihip {

constexpr int SIM_THREADS = 64;       // one wavefront
constexpr size_t SIM_HEAD = 256;      // the counter's share of ctx->sim

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// word 1 of a draw's Philox counter is the simulation's index
static inline int check_sim_indices(elfihip_ctx* ctx, int64_t first, int64_t n) {
  ELFIHIP_REQUIRE(ctx, first >= 0 && first <= (int64_t)0xffffffffLL && n <= (int64_t)0x100000000LL - first,
                  "simulation indices first .. first + n - 1 must stay below 2^32");
  return ELFIHIP_OK;
}

// Launches `kernel` (named `name`) over `units` work units dealt from A.counter: as many workgroups as the device holds at
// once (the kernel's registers and LDS decide), never more than there are units.  The occupancy of a kernel instance is asked
// for once per context and kept under the instance's address.
template <class KernelT, class Args>
static int launch_persistent(elfihip_ctx* ctx, KernelT kernel, const char* name, int64_t units, const Args& A) {
  const void* key = reinterpret_cast<const void*>(kernel);
  int per_cu = 0;
  for (const auto& seen : ctx->sim_per_cu)
    if (seen.first == key) per_cu = seen.second;
  if (per_cu == 0) {
    int q = 0;
    ELFIHIP_CHECK_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&q, kernel, SIM_THREADS, 0));
    per_cu = std::max(1, std::min(q, 32));
    ctx->sim_per_cu.emplace_back(key, per_cu);
  }
  const unsigned grid = (unsigned)std::min<int64_t>(units, (int64_t)ctx->cu_count * per_cu);
  ELFIHIP_CHECK_HIP(ctx, hipMemsetAsync(A.counter, 0, sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SIM_THREADS), 0, ctx->stream, A);
  return launch_status(ctx, name);
}

#if defined(__HIPCC__)
// The wavefront's next `step` units: the counter's value before, the same in every lane.
// Every lane takes part in the one atomic (lane 0 adds `step`, the others 0: the compiler folds them into one instruction)
// and the answer is read back from lane 0 as a scalar, so that every branch on it -- the caller's loop exit, an invalid
// unit's `continue` -- is a branch of the whole wavefront.  With `if (lane == 0)` around the atomic the compiler joins
// that test to the `if (lane == 0)` of the marks a simulator writes at the end of a unit and sends the other 63 lanes round
// the loop without lane 0: a broadcast from lane 0 then reads nothing, they take unit 0 again and the loop never ends.
__device__ __forceinline__ unsigned long long wave_fetch(unsigned long long* counter, int lane, unsigned long long step) {
  const unsigned long long got = atomicAdd(counter, lane == 0 ? step : 0ull);
  return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(got >> 32)) << 32) |
         (unsigned)__builtin_amdgcn_readfirstlane((int)got);
}

// a rate, or a standard deviation: not negative, finite, no NaN
__device__ __forceinline__ bool rate_ok(double r) { return r >= 0.0 && r < INFINITY; }

// every lane gets the sum over the wavefront
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
#endif

}  // namespace elfihip
