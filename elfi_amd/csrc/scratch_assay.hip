// ELFI's scratch-assay example (the cell-motility model of Johnston et al. 2014 with the summaries of Price et al. 2018, the test
// problem of the BSL paper) on gfx950: a lattice random walk of up to 1024 cells, its n_obs + 1 summaries.
//
// Replaces, for elfi/examples/scratch_assay.py:
//     per iteration: sum, where, choice, uniform, a Python loop over the events with choice(4), array arithmetic and two
//         clamps per event -- 10^4 to 2 10^5 events per simulation, 0.1 to 1.6 s each               scratch_assay.py:79-117
//     cell_summaries                                                                                 scratch_assay.py:122-141
//
// The model, iteration t = 0 .. n_iter - 1 of a binary grid of nrows x ncols cells:
//   1. num_cells = the cell count; the list = the occupied cells in row-major order.
//   2. a full grid: nothing happens, no draw is consumed.
//   3. motility: slots k < num_cells have a candidate C[k] in [0, num_cells), a uniform P[k], a direction M[k]; the slots with
//      P[k] < pm are events, in slot order: the cell list[C[k]] looks at its neighbour (M 0: row + 1, 1: row - 1, 2: col + 1,
//      3: col - 1, clamped to the grid) and moves there if that is empty; list[C[k]] follows.
//   4. proliferation: fresh draws over the same num_cells slots against pp, on the list as motility left it; the clamped
//      neighbour is set, whatever it was.
//   5. (t + 1) % obs_every == 0: the grid is frame (t + 1) / obs_every; frame 0 is the initial grid.
// Summaries: ds[j] = the cells that differ between frames j and j + 1, then the cell count of frame n_obs.
//
// sa_sim_kernel: one wavefront per simulation, persistent: a wavefront takes its NEXT simulation from a counter in device memory
// (the events per simulation vary 20-fold over the prior), by one atomic of the whole wavefront read back as a scalar
// (event_sim.hpp: wave_fetch, and its reason).  The grid lies in LDS as one BYTE per cell (1 KB), lane l owns cells 16 l .. 16 l + 15:
// every iteration it packs them to 16 bits, a wave prefix sum of the popcounts places its cells in the row-major list (LDS,
// 16-bit linear indices, 2 KB).  The draw pass is parallel -- lane takes slots lane + 64 j over a wave-uniform trip count (at most
// 16), checks what it read, and the selected slots are compacted IN SLOT ORDER into a queue (LDS, candidate | direction << 10, 2
// KB) by ballot and popcount-below-lane.  The event walk is serial: exactly queue-length trips, every lane makes every trip
// and does the same reads and writes, so no lane depends on another inside it and it holds no barrier, no atomic and no exit:
// queue[e] -> list[c] -> grid[target] -> three stores.  A byte per cell instead of a bit: the event ends in plain stores, not
// in read-modify-writes of mask words (two more dependent round trips, and a case of its own when cell and target share a
// word).  Measured at 200 ns per event for a lone wavefront; reading the queue one event ahead with the event's arithmetic made
// scalar (readfirstlane) took 5 % off that and added 5-8 % to a full device's batch, so it is not kept.  Frames are kept as 16 bits per lane; ds is a wave sum of popcount(prev ^ cur).  No global memory is touched
// inside the loop but the given draws.  Every loop is bounded: iterations by n_iter, slots by 16 trips, events by the queue
// (at most 1023), simulations by the counter; no wavefront waits for another, and which wavefront ran a simulation does not
// enter its result: slot k of phase f of iteration t of simulation g is Philox counter (((2 t + f) << 10) | k, g).
// FMA contraction is off.  The statement of the model is in include/elfihip.h (elfihip_assay_summaries) and, in NumPy, in
// tests/assay_ref.py.
#include "common.hpp"

#include <algorithm>
#include <cmath>

#include "event_sim.hpp"
#include "philox.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int SA_THREADS = SIM_THREADS;
constexpr int SA_MAX = ELFIHIP_ASSAY_MAX_CELLS;         // 1024 = 64 lanes x 16 cells
constexpr int SA_WORDS = SA_MAX / 32;
constexpr int SA_SLOT_BITS = 10;                        // Philox counter word 0: ((2 t + f) << 10) | slot

struct SaArgs {
  const int32_t* C;     // (n, n_iter, 2, cells), or NULL with P and M: drawn here
  const double* P;
  const uint8_t* M;
  uint64_t seed, stream, first;
  const double *pm, *pp;   // (n) each
  int64_t n;
  int nrows, ncols, cells, n_iter, obs_every, n_obs;
  unsigned row_magic;   // (pos row_magic) >> 20 == pos / ncols for pos < 1024
  double* S;            // (n, lds)
  int64_t lds;
  int* status;          // optional (n)
  long long* events;    // optional (n, 2)
  unsigned* frames;     // optional (n, n_obs + 1, 32): cell c at bit c % 32 of word c / 32
  unsigned long long* counter;   // the next simulation, zero at launch
  unsigned init[SA_WORDS];       // the initial grid in the frames' layout
};

// the draws of slot k of phase f of iteration t of simulation g for num_cells slots
__device__ __forceinline__ void sa_draw(uint64_t seed, uint64_t stream, uint64_t g, int t, int f, int k, int num_cells, int& c,
                                        double& p, unsigned& m) {
  uint32_t r[4];
  philox4x32_10(((uint32_t)(2 * t + f) << SA_SLOT_BITS) | (uint32_t)k, (uint32_t)g, (uint32_t)stream, (uint32_t)(stream >> 32),
                (uint32_t)seed, (uint32_t)(seed >> 32), r);
  c = (int)__umulhi(r[0], (uint32_t)num_cells);
  p = unit_co(word53(r[1], r[2]));
  m = r[3] >> 30;
}

// four cells, one byte each (0 or 1) <-> four bits
__device__ __forceinline__ unsigned sa_pack4(unsigned w) { return ((w * 0x01020408u) >> 24) & 0xFu; }
__device__ __forceinline__ unsigned sa_spread4(unsigned b) { return (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21); }

template <bool DRAWN>
__global__ __launch_bounds__(SA_THREADS) void sa_sim_kernel(SaArgs A) {
  __shared__ __align__(16) unsigned char s_grid[SA_MAX];
  __shared__ unsigned short s_list[SA_MAX], s_queue[SA_MAX];
  const int lane = threadIdx.x, cells = A.cells, nrows = A.nrows, ncols = A.ncols, n_obs = A.n_obs;
  const unsigned init16 = (A.init[lane >> 1] >> ((lane & 1) * 16)) & 0xFFFFu;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (;;) {
    const unsigned long long sim = wave_fetch(A.counter, lane, 1ull);   // the next simulation, a scalar
    if (sim >= (unsigned long long)A.n) break;
    const double pm = A.pm[sim], pp = A.pp[sim];
    const uint64_t g = A.first + sim;
    double* S = A.S + (int64_t)sim * A.lds;
    unsigned* frames = A.frames ? A.frames + (int64_t)sim * (n_obs + 1) * SA_WORDS : nullptr;
    reinterpret_cast<uint4*>(s_grid)[lane] = make_uint4(sa_spread4(init16), sa_spread4(init16 >> 4), sa_spread4(init16 >> 8),
                                                        sa_spread4(init16 >> 12));
    if (frames && lane < SA_WORDS) frames[lane] = A.init[lane];
    __syncthreads();
    unsigned prev = init16;
    long long made[2] = {0, 0};
    int next_obs = A.obs_every, frame = 0;
    bool bad = false;
    for (int t = 0;; ++t) {            // (every value that decides the control flow is the same in all 64 lanes)
      const uint4 w = reinterpret_cast<const uint4*>(s_grid)[lane];
      const unsigned cur = sa_pack4(w.x) | (sa_pack4(w.y) << 4) | (sa_pack4(w.z) << 8) | (sa_pack4(w.w) << 12);
      if (t == next_obs) {             // the grid after iteration t - 1 is frame t / obs_every
        ++frame;
        next_obs += A.obs_every;
        const int ds = wave_sum(__popc(prev ^ cur));
        if (lane == 0) S[frame - 1] = (double)ds;
        const unsigned up = (unsigned)__shfl_down((int)cur, 1, 64);
        if (frames && !(lane & 1)) frames[frame * SA_WORDS + (lane >> 1)] = cur | (up << 16);
        prev = cur;
      }
      if (t == A.n_iter) break;
      // the row-major list: an inclusive prefix sum of the lanes' cell counts
      const int cnt = __popc(cur);
      int incl = cnt;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(incl, off, 64);
        if (lane >= off) incl += v;
      }
      const int nc = __builtin_amdgcn_readlane(incl, 63);
      if (nc == cells) continue;       // a full grid: nothing happens, nothing is drawn
      int o = incl - cnt;
#pragma unroll
      for (int b = 0; b < 16; ++b)
        if ((cur >> b) & 1u) s_list[o++] = (unsigned short)(16 * lane + b);
      const int trips = (nc + 63) >> 6;
      for (int f = 0; f < 2; ++f) {
        const double thr = f ? pp : pm;
        int qlen = 0;
        for (int j = 0; j < trips; ++j) {
          const int k = lane + 64 * j;
          const bool valid = k < nc;
          int c = 0;
          double p = 0.0;
          unsigned m = 0;
          if (valid) {
            if constexpr (DRAWN) {
              sa_draw(A.seed, A.stream, g, t, f, k, nc, c, p, m);
            } else {
              const int64_t at = ((((int64_t)sim * A.n_iter + t) * 2 + f) * cells) + k;
              c = A.C[at];
              p = A.P[at];
              m = A.M[at];
            }
          }
          const bool wrong = valid && ((unsigned)c >= (unsigned)nc || m > 3u);   // nothing is indexed by an unchecked value
          if (wrong) c = 0, m = 0;
          bad = bad || __ballot(wrong) != 0ull;
          const bool sel = valid && p < thr;                                     // NaN selects nothing
          const unsigned long long bal = __ballot(sel);
          if (sel) s_queue[qlen + __popcll(bal & below)] = (unsigned short)((unsigned)c | (m << SA_SLOT_BITS));
          qlen += __popcll(bal);
        }
        if (bad) break;
        __syncthreads();               // the list and the queue are written
        for (int e = 0; e < qlen; ++e) {
          const unsigned q = s_queue[e], c = q & (SA_MAX - 1), d = q >> SA_SLOT_BITS;
          const unsigned pos = s_list[c];
          const unsigned row = (pos * A.row_magic) >> 20, col = pos - row * ncols;
          unsigned tgt = pos;
          if (d == 0u)
            tgt = row + 1 < (unsigned)nrows ? pos + ncols : pos;
          else if (d == 1u)
            tgt = row > 0u ? pos - ncols : pos;
          else if (d == 2u)
            tgt = col + 1 < (unsigned)ncols ? pos + 1 : pos;
          else
            tgt = col > 0u ? pos - 1 : pos;
          if (f) {
            s_grid[tgt] = 1;
          } else if (s_grid[tgt] == 0) {
            s_grid[pos] = 0;
            s_grid[tgt] = 1;
            s_list[c] = (unsigned short)tgt;
          }
        }
        made[f] += qlen;
        __syncthreads();               // the next draw pass overwrites the queue, the next iteration reads the grid by lanes
      }
      if (bad) break;
    }
    if (bad) {                         // (uniform) a draw that is no draw: the simulation has no result
      for (int j = lane; j <= n_obs; j += SA_THREADS) S[j] = NAN;
      if (frames)
        for (int j = lane; j < (n_obs + 1) * SA_WORDS; j += SA_THREADS) frames[j] = 0u;
      made[0] = made[1] = 0;
    } else {
      const int count = wave_sum(__popc(prev));
      if (lane == 0) S[n_obs] = (double)count;
    }
    if (lane == 0) {
      if (A.status) A.status[sim] = bad ? ELFIHIP_ASSAY_BAD_DRAW : ELFIHIP_ASSAY_OK;
      if (A.events) {
        A.events[2 * sim] = made[0];
        A.events[2 * sim + 1] = made[1];
      }
    }
    __syncthreads();                   // the next simulation overwrites the grid
  }
}

// the draws of the drawn form, into memory: C, P, M (n, n_iter, 2, cells) for num_cells (n, n_iter, 2) slots per row, zero
// past them -- what the given form takes
__global__ __launch_bounds__(256) void sa_draws_kernel(uint64_t seed, uint64_t stream, uint64_t first, int64_t n, int n_iter, int cells,
                                                       const int32_t* __restrict__ num_cells, int32_t* __restrict__ C,
                                                       double* __restrict__ P, uint8_t* __restrict__ M) {
  const int64_t total = n * n_iter * 2 * cells, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t el = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; el < total; el += stride) {
    const int64_t row = el / cells, it = row >> 1, i = it / n_iter;
    const int k = (int)(el - row * cells), f = (int)(row & 1), t = (int)(it - i * n_iter);
    const int nc = std::min(std::max(num_cells[row], 0), cells);
    int c = 0;
    double p = 0.0;
    unsigned m = 0;
    if (k < nc) sa_draw(seed, stream, first + (uint64_t)i, t, f, k, nc, c, p, m);
    C[el] = c;
    P[el] = p;
    M[el] = (uint8_t)m;
  }
}

// ---- launches -----------------------------------------------------------------------------------------------------------
static int sa_shape_check(elfihip_ctx* ctx, int64_t first, int64_t n, int n_iter, int64_t cells) {
  ELFIHIP_REQUIRE(ctx, n >= 1 && n <= ELFIHIP_ASSAY_MAX_BATCH, "bad batch n=%lld: 1 to 2^31 - 1", (long long)n);
  ELFIHIP_REQUIRE(ctx, cells >= 1 && cells <= ELFIHIP_ASSAY_MAX_CELLS, "%lld cells: 1 to %d", (long long)cells, ELFIHIP_ASSAY_MAX_CELLS);
  ELFIHIP_REQUIRE(ctx, n_iter >= 1 && n_iter <= ELFIHIP_ASSAY_MAX_ITER, "%d iterations: 1 to 2^21", n_iter);
  return check_sim_indices(ctx, first, n);
}

static int sa_model_check(elfihip_ctx* ctx, int64_t first, int64_t n, int nrows, int ncols, int n_iter, int obs_every,
                          const uint8_t* init, const void* C, const void* P, const void* M, const void* pm, const void* pp,
                          const void* S) {
  ELFIHIP_REQUIRE(ctx, nrows >= 1 && ncols >= 1, "a grid of %d x %d", nrows, ncols);
  ELFIHIP_TRY(sa_shape_check(ctx, first, n, n_iter, (int64_t)nrows * ncols));
  ELFIHIP_REQUIRE(ctx, obs_every >= 1 && obs_every <= n_iter, "an observation every %d of %d iterations: 1 to n_iter", obs_every, n_iter);
  ELFIHIP_REQUIRE(ctx, (C == nullptr) == (P == nullptr) && (C == nullptr) == (M == nullptr), "C, P and M are given together or not at all");
  ELFIHIP_REQUIRE(ctx, init && pm && pp && S, "NULL pointer");
  for (int c = 0; c < nrows * ncols; ++c) ELFIHIP_REQUIRE(ctx, init[c] <= 1, "cell %d of the initial grid is neither 0 nor 1", c);
  return ELFIHIP_OK;
}

static int sa_dev_impl(elfihip_ctx* ctx, const int32_t* dC, const double* dP, const uint8_t* dM, uint64_t seed, uint64_t stream,
                       int64_t first, int64_t n, int nrows, int ncols, int n_iter, int obs_every, const uint8_t* init,
                       const double* dpm, const double* dpp, double* dS, int64_t lds, int32_t* dstatus, int64_t* devents,
                       uint32_t* dframes) {
  ELFIHIP_TRY(sa_model_check(ctx, first, n, nrows, ncols, n_iter, obs_every, init, dC, dP, dM, dpm, dpp, dS));
  const int n_obs = n_iter / obs_every;
  ELFIHIP_REQUIRE(ctx, lds >= n_obs + 1, "leading dimension below the row length");
  ELFIHIP_CHECK_HIP(ctx, ctx->sim.reserve(SIM_HEAD));
  SaArgs A;
  A.C = dC;
  A.P = dP;
  A.M = dM;
  A.seed = seed;
  A.stream = stream;
  A.first = (uint64_t)first;
  A.pm = dpm;
  A.pp = dpp;
  A.n = n;
  A.nrows = nrows;
  A.ncols = ncols;
  A.cells = nrows * ncols;
  A.n_iter = n_iter;
  A.obs_every = obs_every;
  A.n_obs = n_obs;
  A.row_magic = (1u << 20) / (unsigned)ncols + 1u;
  A.S = dS;
  A.lds = lds;
  A.status = dstatus;
  A.events = reinterpret_cast<long long*>(devents);
  A.frames = dframes;
  A.counter = ctx->sim.as<unsigned long long>();
  for (int w = 0; w < SA_WORDS; ++w) A.init[w] = 0u;
  for (int c = 0; c < A.cells; ++c) A.init[c >> 5] |= (unsigned)init[c] << (c & 31);
  return dC ? launch_persistent(ctx, sa_sim_kernel<false>, "sa_sim_kernel", n, A)
            : launch_persistent(ctx, sa_sim_kernel<true>, "sa_sim_kernel", n, A);
}

static int sa_draws_impl(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_iter, int cells,
                         const int32_t* dnum, int32_t* dC, double* dP, uint8_t* dM) {
  ELFIHIP_TRY(sa_shape_check(ctx, first, n, n_iter, cells));
  ELFIHIP_REQUIRE(ctx, dnum && dC && dP && dM, "NULL pointer");
  const int64_t total = n * n_iter * 2 * cells;
  const unsigned grid = (unsigned)std::min<int64_t>((total + 255) / 256, (int64_t)ctx->cu_count * 16);
  hipLaunchKernelGGL(sa_draws_kernel, dim3(grid), dim3(256), 0, ctx->stream, seed, stream, (uint64_t)first, n, n_iter, cells, dnum, dC,
                     dP, dM);
  return launch_status(ctx, "sa_draws_kernel");
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_assay_summaries_dev(elfihip_ctx* ctx, const int32_t* dC, const double* dP, const uint8_t* dM, uint64_t seed,
                                uint64_t stream, int64_t first, int64_t n, int nrows, int ncols, int n_iter, int obs_every,
                                const uint8_t* init, const double* dpm, const double* dpp, double* dS, int64_t lds,
                                int32_t* dstatus, int64_t* devents, uint32_t* dframes) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return sa_dev_impl(ctx, dC, dP, dM, seed, stream, first, n, nrows, ncols, n_iter, obs_every, init, dpm, dpp, dS, lds, dstatus,
                     devents, dframes);
}

int elfihip_assay_summaries(elfihip_ctx* ctx, const int32_t* C, const double* P, const uint8_t* M, uint64_t seed, uint64_t stream,
                            int64_t first, int64_t n, int nrows, int ncols, int n_iter, int obs_every, const uint8_t* init,
                            const double* pm, const double* pp, double* S, int32_t* status, int64_t* events, uint32_t* frames) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(sa_model_check(ctx, first, n, nrows, ncols, n_iter, obs_every, init, C, P, M, pm, pp, S));
  DeviceGuard g(ctx->device);
  const size_t nn = (size_t)n, nd = C ? nn * (size_t)n_iter * 2 * (size_t)(nrows * ncols) : 0, ns = nn * (size_t)(n_iter / obs_every + 1);
  const size_t nf = frames ? ns * SA_WORDS : 0;
  const size_t i_c = align256((nd + 2 * nn) * sizeof(double)), i_m = i_c + align256(nd * sizeof(int32_t));
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(i_m + nd));
  const size_t o_e = align256(ns * sizeof(double)), o_f = o_e + align256(2 * nn * sizeof(int64_t));
  const size_t o_s = o_f + align256(nf * sizeof(uint32_t));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(o_s + nn * sizeof(int32_t)));
  char *in = ctx->in.as<char>(), *out = ctx->out.as<char>();
  double *dP = ctx->in.as<double>(), *dpar = dP + nd;
  int32_t* dC = reinterpret_cast<int32_t*>(in + i_c);
  uint8_t* dM = reinterpret_cast<uint8_t*>(in + i_m);
  double* dS = ctx->out.as<double>();
  int64_t* dev = reinterpret_cast<int64_t*>(out + o_e);
  uint32_t* dfr = reinterpret_cast<uint32_t*>(out + o_f);
  int32_t* dst = reinterpret_cast<int32_t*>(out + o_s);
  if (C) {
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dP, P, nd * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dC, C, nd * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dM, M, nd, hipMemcpyHostToDevice, ctx->stream));
  }
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar, pm, nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar + nn, pp, nn * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(sa_dev_impl(ctx, C ? dC : nullptr, C ? dP : nullptr, C ? dM : nullptr, seed, stream, first, n, nrows, ncols, n_iter,
                          obs_every, init, dpar, dpar + nn, dS, n_iter / obs_every + 1, status ? dst : nullptr,
                          events ? dev : nullptr, frames ? dfr : nullptr));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(S, dS, ns * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (status) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(status, dst, nn * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  if (events) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(events, dev, 2 * nn * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
  if (frames) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(frames, dfr, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

int elfihip_assay_draws_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_iter, int cells,
                            const int32_t* dnum_cells, int32_t* dC, double* dP, uint8_t* dM) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return sa_draws_impl(ctx, seed, stream, first, n, n_iter, cells, dnum_cells, dC, dP, dM);
}

int elfihip_assay_draws(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_iter, int cells,
                        const int32_t* num_cells, int32_t* C, double* P, uint8_t* M) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(sa_shape_check(ctx, first, n, n_iter, cells));
  ELFIHIP_REQUIRE(ctx, num_cells && C && P && M, "NULL pointer");
  const size_t rows = (size_t)n * (size_t)n_iter * 2, nd = rows * (size_t)cells;
  for (size_t r = 0; r < rows; ++r)
    ELFIHIP_REQUIRE(ctx, num_cells[r] >= 0 && num_cells[r] <= cells, "num_cells[%lld] = %d: 0 to %d", (long long)r, num_cells[r], cells);
  DeviceGuard g(ctx->device);
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(rows * sizeof(int32_t)));
  const size_t o_c = align256(nd * sizeof(double)), o_m = o_c + align256(nd * sizeof(int32_t));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(o_m + nd));
  char* out = ctx->out.as<char>();
  double* dP = ctx->out.as<double>();
  int32_t* dC = reinterpret_cast<int32_t*>(out + o_c);
  uint8_t* dM = reinterpret_cast<uint8_t*>(out + o_m);
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(ctx->in.p, num_cells, rows * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  ELFIHIP_TRY(sa_draws_impl(ctx, seed, stream, first, n, n_iter, cells, ctx->in.as<int32_t>(), dC, dP, dM));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(C, dC, nd * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(P, dP, nd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(M, dM, nd, hipMemcpyDeviceToHost, ctx->stream));
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
