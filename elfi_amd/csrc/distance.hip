// Batched row-vs-observed distances for gfx950 (MI355X).
//
// Replaces the scipy.spatial.distance.cdist(X (n,m), Y (1,m), ...) call that
// elfi.Distance / AdaptiveDistance make once per batch
// (elfi/model/elfi_model.py:1037,1084 via elfi/model/utils.py:37-52).
//
// These kernels are HBM-bound: 8*m bytes in and 8 bytes out per distance, 2-3 flops
// per byte.  Design:
//   * row-major input (the np.column_stack layout): a workgroup streams a tile of
//     R = blockDim rows as ONE contiguous span with 16-byte loads per lane (fully
//     coalesced), drops it into LDS with an odd row pitch (m|1 doubles, so a
//     column walk by 64 lanes is bank-conflict free for ds_read_b64), and then lane r
//     sums row r left to right.  The LDS transpose is what lets every lane own a
//     whole row, so the accumulation order is exactly SciPy's (sequential over j) and
//     the result is bit-identical to cdist for the +,*,abs,max metrics.
//   * column-major input (ELFI's separate summary arrays, before column_stack): lane
//     i walks column j at row i -- coalesced by construction, no LDS needed.
//   * very wide rows (m >= 300): one wavefront per row with a shuffle tree (order
//     differs from SciPy by a few ulp; documented tolerance).
//   * canberra, braycurtis, cosine and correlation go through the same forms with
//     their row sums in Row<METRIC, W> (dist_metrics.hpp): SciPy's order again, so bit-identical
//     up to m = 299 except weighted cosine / correlation (SciPy's np.dot order).
// FMA contraction is off in this file (dist_metrics.hpp): a fused d*d+s would round differently from the reference's
// separate multiply and add.
// Mahalanobis has its own kernels (mahalanobis.hip), and so have the K weighted distances of AdaptiveDistance (multiw.hip).
#include "common.hpp"
#include "tile_stream.hpp"
#include "internal.hpp"
#include "dist_launch.hpp"
#include "dist_metrics.hpp"

namespace elfihip {

// Pipelined form of dist_rows_kernel: requires vec2 and T * U >= T * m / 2 (whole tile per batch).
template <int METRIC, bool W, int U>
__global__ __launch_bounds__(256) void dist_rows_pipe_kernel(RowArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int T = blockDim.x, tid = threadIdx.x, m = A.m;
  double* tile = lds;
  const int R = A.R;
  double* ys = tile + (size_t)R * A.mp;
  double* as = ys + m;
  const Obs o = obs_of<METRIC, W>(A.y, A.aux, m);
  for (int j = tid; j < m; j += T) {
    ys[j] = A.y[j];
    if constexpr (W) as[j] = kept_aux<METRIC, W>(A.aux[j], o);
  }
  const int64_t ntiles = (A.n + R - 1) / R;
  const double thr = A.F.thr ? *A.F.thr : 0.0;   // fused selection: the sampler state's current k-th best distance
  double2 v[U];
  int64_t t = blockIdx.x;
  if (t < ntiles) tile_fetch<U>(A, t * R, (int)((A.n - t * R) < R ? (A.n - t * R) : R), v);
  for (; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * R;
    const int rows = (int)((A.n - row0) < R ? (A.n - row0) : R);
    __syncthreads();  // tile free (previous readers done); ys/as visible on the first trip
    tile_commit<U>(A, tile, rows, v);
    const int64_t tn = t + gridDim.x;
    if (tn < ntiles) tile_fetch<U>(A, tn * R, (int)((A.n - tn * R) < R ? (A.n - tn * R) : R), v);
    __syncthreads();
    double dist = 0.0;
    if (tid < rows) {
      const double* row = tile + (size_t)tid * A.mp;
      if constexpr (kRowMetric<METRIC>) {
        dist = Row<METRIC, W>::dist([&](int j) { return row[j]; }, [&](int j) { return ys[j]; },
                                    [&](int j) { return as[j]; }, m, o);
      } else {
        double s = Op<METRIC, W>::init();
#pragma unroll 8
        for (int j = 0; j < m; ++j) s = Op<METRIC, W>::step(s, row[j], ys[j], W ? as[j] : 1.0, A.p);
        dist = Op<METRIC, W>::finish(s, A.inv_p);
      }
      A.out[row0 + tid] = dist;
    }
    if (A.F.thr) reject_offer(A.F, tid < rows && dist < thr, dist, A.F.row_base + row0 + tid);
  }
}

// ---- LDS-DMA form of the row stream (round 5; m = 16 / 32 / 64 with 16-byte aligned rows) -----------------------------------
// The tile no longer passes through registers: `global_load_lds_dwordx4` writes 1 KiB per wave-instruction straight into
// LDS, so a wave can keep a RING of D slots (16 KiB each) in flight at no register cost and without any workgroup barrier --
// a wave only ever reads slots it issued itself, behind its own counted `s_waitcnt vmcnt` (MI355X_MICROARCH.md: nothing
// else orders a ds_read behind an LDS-DMA).  The DMA image is lane-linear (base + lane * 16), i.e. rows at pitch m with no
// padding; the bank conflicts of "lane r reads row r" are removed by an XOR swizzle of the 16-byte granules that is applied
// to the SOURCE address when the slot is filled and again when the row is read (cdna_hip_programming.md rule 21).  Lane r
// still sums row r left to right, so the results stay bit-identical to cdist.  Non-temporal loads: the rows are read once.
// Measured on 10^6 x 32 (scripts/native/glds_probe.hip, profiles/r05_glds_probe.md): 41.8-42.1 us = 6.3 TB/s (40.7 on the
// best box), against 46.5-47.2 us for the register-staged pipeline in the same binary.
// MERGE: workgroup 0 folds the sampler state's sealed candidate list A.M into the state (reject_merge_wave, in the ring's
// LDS) and streams nothing; the other gridDim.x - 1 workgroups stream the slots.  The stream reads the threshold once, with
// an atomic load: the k-th distance before this merge and the one after it are both upper bounds of the state's k-th
// distance, so either keeps the filter exact.  Nothing waits across workgroups.
template <int METRIC, bool W, int MM, int ROWS, int D, bool MERGE>
__global__ __launch_bounds__(64) void dist_rows_dma_kernel(RowArgs A) {
  extern __shared__ __align__(16) double lds[];
  constexpr int SLOT = ROWS * MM;                // doubles
  constexpr int H = MM / 2;
  constexpr int PIECES = ROWS * H / 64;
  static_assert(ROWS <= 64 && (ROWS * H) % 64 == 0, "a slot is a whole number of 1 KiB DMA pieces, one row per lane");
  static_assert(D * SLOT * 8 >= REJ_FUSED_LDS, "the merge role works in the slot ring");
  if constexpr (MERGE) {
    if (blockIdx.x == 0) {
      reject_merge_wave(A.M, lds);
      return;
    }
  }
  const int lane = threadIdx.x;
  double* ring = lds;
  double* ys = lds + (size_t)D * SLOT;
  double* as = ys + MM;
  const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)ring);
  const Obs o = obs_of<METRIC, W>(A.y, A.aux, MM);
  if (lane < MM) {
    ys[lane] = A.y[lane];
    if constexpr (W) as[lane] = kept_aux<METRIC, W>(A.aux[lane], o);
  }
  const int64_t nslots = (A.n + ROWS - 1) / ROWS;
  const int64_t stride = MERGE ? gridDim.x - 1 : gridDim.x;
  double thr = 0.0;   // fused selection: the sampler state's current k-th best distance
  if (A.F.thr) {
    if constexpr (MERGE)
      thr = __hip_atomic_load(A.F.thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (workgroup 0 may be rewriting it)
    else
      thr = *A.F.thr;
  }
  unsigned off[PIECES];   // byte offset of this lane's granule of piece i from the slot's first row (the launcher checks
#pragma unroll            // that 64 rows of pitch ldx stay below 2^31 bytes)
  for (int i = 0; i < PIECES; ++i) {
    const int G = i * 64 + lane;
    const int row = G / H, g = G % H;
    off[i] = (unsigned)(((int64_t)row * A.ldx + 2 * (g ^ dma_swizzle_key<MM>(row))) * 8);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // nothing of the prologue is outstanding: the counted
  int64_t t = MERGE ? blockIdx.x - 1 : blockIdx.x;               // waits below see the DMA pieces and the stores only
#pragma unroll
  for (int k = 0; k < D - 1; ++k) {
    const int64_t tk = t + k * stride;
    if (tk < nslots) dma_issue_slot<MM, ROWS>(A, off, tk * ROWS, lds_base + (unsigned)(k * SLOT * 8), lane);
  }
  int cur = 0;
  for (; t < nslots; t += stride) {
    // keep the ring full: the slot read in the previous trip is free (its reads were waited for at the trip's end)
    const int64_t tn = t + (int64_t)(D - 1) * stride;
    int nxt = cur + D - 1;
    if (nxt >= D) nxt -= D;
    if (tn < nslots) {
      dma_issue_slot<MM, ROWS>(A, off, tn * ROWS, lds_base + (unsigned)(nxt * SLOT * 8), lane);
      // loads return in order: once at most the D - 1 younger slots' pieces are outstanding, slot `cur` has landed (a
      // store of an earlier trip still in flight only makes this wait longer, never shorter)
      wait_vmcnt<PIECES * (D - 1)>();
    } else {
      wait_vmcnt<0>();
    }
    const int64_t row0 = t * ROWS;
    double dist = 0.0;
    const bool mine = (ROWS == 64 || lane < ROWS) && row0 + lane < A.n;
    if (ROWS == 64 || lane < ROWS) {
      const double* row = ring + (size_t)cur * SLOT + (size_t)lane * MM;
      const int key = dma_swizzle_key<MM>(lane);
      if constexpr (kRowMetric<METRIC>) {
        dist = Row<METRIC, W>::dist([&](int j) { return row[2 * ((j >> 1) ^ key) + (j & 1)]; },
                                    [&](int j) { return ys[j]; }, [&](int j) { return as[j]; }, MM, o);
      } else {
        double s = Op<METRIC, W>::init();
#pragma unroll
        for (int c = 0; c < H; ++c) {
          const double2 v = *reinterpret_cast<const double2*>(row + 2 * (c ^ key));
          const double2 yv = *reinterpret_cast<const double2*>(ys + 2 * c);
          double2 av = make_double2(1.0, 1.0);
          if constexpr (W) av = *reinterpret_cast<const double2*>(as + 2 * c);
          s = Op<METRIC, W>::step(s, v.x, yv.x, av.x, A.p);
          s = Op<METRIC, W>::step(s, v.y, yv.y, av.y, A.p);
        }
        dist = Op<METRIC, W>::finish(s, A.inv_p);
      }
      if (mine) A.out[row0 + lane] = dist;
    }
    if (A.F.thr) reject_offer(A.F, mine && dist < thr, dist, A.F.row_base + row0 + lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the slot's reads are done before it is refilled
    cur = cur + 1 == D ? 0 : cur + 1;
  }
}

// One distance per row, SciPy accumulation order.
template <int METRIC, bool W, int U>
__global__ void dist_rows_kernel(RowArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int T = blockDim.x, tid = threadIdx.x, m = A.m;
  double* tile = lds;
  double* ys = tile + (size_t)T * A.mp;
  double* as = ys + m;
  const Obs o = obs_of<METRIC, W>(A.y, A.aux, m);
  for (int j = tid; j < m; j += T) {
    ys[j] = A.y[j];
    if constexpr (W) as[j] = kept_aux<METRIC, W>(A.aux[j], o);
  }
  const int64_t ntiles = (A.n + T - 1) / T;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * T;
    const int rows = (int)((A.n - row0) < T ? (A.n - row0) : T);
    __syncthreads();  // tile free (previous readers done); ys/as visible on the first trip
    load_tile<U>(A, tile, row0, rows);
    __syncthreads();
    if (tid < rows) {
      const double* row = tile + (size_t)tid * A.mp;
      if constexpr (kRowMetric<METRIC>) {
        A.out[row0 + tid] = Row<METRIC, W>::dist([&](int j) { return row[j]; }, [&](int j) { return ys[j]; },
                                                 [&](int j) { return as[j]; }, m, o);
      } else {
        double s = Op<METRIC, W>::init();
#pragma unroll 4
        for (int j = 0; j < m; ++j) s = Op<METRIC, W>::step(s, row[j], ys[j], W ? as[j] : 1.0, A.p);
        A.out[row0 + tid] = Op<METRIC, W>::finish(s, A.inv_p);
      }
    }
  }
}

// Column-major input: lane i reads C[j*ldc + i]; two rows per lane when aligned.
struct ColArgs {
  const double* C;
  int64_t n, ldc;
  const double* y;
  const double* aux;
  double* out;
  double p, inv_p;
  int m;
  int vec2;
  int nt;   // non-temporal loads of the columns (each element is read once)
};

typedef double v2d_cols __attribute__((ext_vector_type(2)));

template <int METRIC, bool W>
__global__ void dist_cols_kernel(ColArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int m = A.m;
  double* ys = lds;
  double* as = ys + m;
  const Obs o = obs_of<METRIC, W>(A.y, A.aux, m);
  for (int j = threadIdx.x; j < m; j += blockDim.x) {
    ys[j] = A.y[j];
    if constexpr (W) as[j] = kept_aux<METRIC, W>(A.aux[j], o);
  }
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if constexpr (kRowMetric<METRIC>) {
    // lane i owns row i (8-byte loads, consecutive lanes on consecutive rows); correlation reads its columns twice, for
    // the mean and for the dot products (the second read is served by the caches for the rows a wave has in flight)
    for (int64_t i = gid; i < A.n; i += stride) {
      const double* __restrict__ c = A.C + i;
      A.out[i] = Row<METRIC, W>::dist([&](int j) { return c[(int64_t)j * A.ldc]; }, [&](int j) { return ys[j]; },
                                      [&](int j) { return as[j]; }, m, o);
    }
  } else if (A.vec2) {
    const int64_t npair = A.n >> 1;
    for (int64_t i2 = gid; i2 < npair; i2 += stride) {
      double s0 = Op<METRIC, W>::init(), s1 = s0;
      const double* __restrict__ c = A.C + 2 * i2;
      int j = 0;
      for (; j + 8 <= m; j += 8) {
        double2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const double* src = c + (int64_t)(j + u) * A.ldc;
          if (A.nt) {
            const v2d_cols t = __builtin_nontemporal_load(reinterpret_cast<const v2d_cols*>(src));
            v[u] = make_double2(t.x, t.y);
          } else {
            v[u] = *reinterpret_cast<const double2*>(src);
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          s0 = Op<METRIC, W>::step(s0, v[u].x, ys[j + u], W ? as[j + u] : 1.0, A.p);
          s1 = Op<METRIC, W>::step(s1, v[u].y, ys[j + u], W ? as[j + u] : 1.0, A.p);
        }
      }
      for (; j < m; ++j) {
        double2 v = *reinterpret_cast<const double2*>(c + (int64_t)j * A.ldc);
        s0 = Op<METRIC, W>::step(s0, v.x, ys[j], W ? as[j] : 1.0, A.p);
        s1 = Op<METRIC, W>::step(s1, v.y, ys[j], W ? as[j] : 1.0, A.p);
      }
      double2 o;
      o.x = Op<METRIC, W>::finish(s0, A.inv_p);
      o.y = Op<METRIC, W>::finish(s1, A.inv_p);
      *reinterpret_cast<double2*>(A.out + 2 * i2) = o;
    }
    if ((A.n & 1) && gid == 0) {  // odd tail row
      const int64_t i = A.n - 1;
      double s = Op<METRIC, W>::init();
      for (int j = 0; j < m; ++j)
        s = Op<METRIC, W>::step(s, A.C[(int64_t)j * A.ldc + i], ys[j], W ? as[j] : 1.0, A.p);
      A.out[i] = Op<METRIC, W>::finish(s, A.inv_p);
    }
  } else {
    for (int64_t i = gid; i < A.n; i += stride) {
      double s = Op<METRIC, W>::init();
      const double* __restrict__ c = A.C + i;
      int j = 0;
      for (; j + 8 <= m; j += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = c[(int64_t)(j + u) * A.ldc];
#pragma unroll
        for (int u = 0; u < 8; ++u) s = Op<METRIC, W>::step(s, v[u], ys[j + u], W ? as[j + u] : 1.0, A.p);
      }
      for (; j < m; ++j) s = Op<METRIC, W>::step(s, c[(int64_t)j * A.ldc], ys[j], W ? as[j] : 1.0, A.p);
      A.out[i] = Op<METRIC, W>::finish(s, A.inv_p);
    }
  }
}

// Very wide rows: one wavefront per row, lanes stride over the columns, butterfly combine.
template <int METRIC, bool W>
__global__ void dist_rows_wide_kernel(RowArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  if constexpr (kRowMetric<METRIC>) {
    const Obs o = obs_of<METRIC, W>(A.y, A.aux, A.m);
    for (int64_t r = wave; r < A.n; r += nwaves) {
      const double d = Row<METRIC, W>::wide(A.X + r * A.ldx, A.y, A.aux, A.m, lane, o);
      if (lane == 0) A.out[r] = d;
    }
    return;
  }
  for (int64_t r = wave; r < A.n; r += nwaves) {
    const double* __restrict__ x = A.X + r * A.ldx;
    double s = Op<METRIC, W>::init();
    for (int j = lane; j < A.m; j += 64) s = Op<METRIC, W>::step(s, x[j], A.y[j], W ? A.aux[j] : 1.0, A.p);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = Op<METRIC, W>::combine(s, __shfl_xor(s, off, 64));
    if (lane == 0) A.out[r] = Op<METRIC, W>::finish(s, A.inv_p);
  }
}

template <int METRIC, bool W, int M, int U>
__global__ __launch_bounds__(256) void dist_rows_narrow_kernel(RowArgs A) {
  const int tid = threadIdx.x;
  double yv[M], av[M];
  const Obs o = obs_of<METRIC, W>(A.y, A.aux, M);
#pragma unroll
  for (int j = 0; j < M; ++j) {
    yv[j] = A.y[j];
    av[j] = W ? kept_aux<METRIC, W>(A.aux[j], o) : 1.0;
  }
  const double thr = A.F.thr ? *A.F.thr : 0.0;   // fused selection: the sampler state's current k-th best distance
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
      double dist;
      if constexpr (kRowMetric<METRIC>) {
        dist = Row<METRIC, W>::dist([&](int j) { return x[u][j]; }, [&](int j) { return yv[j]; },
                                    [&](int j) { return av[j]; }, M, o);
      } else {
        double s = Op<METRIC, W>::init();
#pragma unroll
        for (int j = 0; j < M; ++j) s = Op<METRIC, W>::step(s, x[u][j], yv[j], av[j], A.p);
        dist = Op<METRIC, W>::finish(s, A.inv_p);
      }
      if (r < A.n) A.out[r] = dist;
      if (A.F.thr) reject_offer(A.F, r < A.n && dist < thr, dist, A.F.row_base + r);
    }
  }
}

// 16-byte loads per thread of the pipelined row kernels.  Rows that cost a few flops per element (everything but
// general Minkowski and the K-weight sums) stream best in tiles of 32 to 64 rows (8 to 16 KiB per workgroup); the
// heavier per-row work wants all 128 lanes of the workgroup on rows (tiles of 128 rows).
static int pipe_unroll(int m, bool light) {
  if (!light) return m <= 16 ? 8 : 16;
  return m <= 32 ? 4 : (m <= 64 ? 8 : 16);
}

// Where the LDS-DMA form is used for the Row metrics: where it was measured faster than the register-staged pipeline
// (scripts/time_metrics.py, profiles/distance_metrics.md).  Canberra's division per element makes it VALU-bound in the DMA form's
// one-wave workgroups except at 32 summaries (2 10^6 x 16: 55.0 us against 49.3; 10^6 x 32: 54.0 against 64.2;
// 1.25 10^6 x 64: 175 against 152).  At 64 summaries the slots hold 32 rows -- half the lanes sum rows -- and weighted
// correlation (three sums per element) loses there too (166 against 151 us).  Everything else streams faster by DMA.
template <int METRIC, bool W, int MM>
constexpr bool kDma = MM == 16   ? METRIC != ELFIHIP_CANBERRA
                      : MM == 64 ? !(METRIC == ELFIHIP_CANBERRA || (METRIC == ELFIHIP_CORRELATION && W))
                                 : true;

// The LDS-DMA form's shapes, summaries per row -> rows per slot and slots in the ring: one-wave workgroups, each with a ring
// of two 16 KiB slots (64 rows of 32 summaries, 32 rows of 64; four 8 KiB slots of 64 rows at 16 summaries), four
// workgroups per CU.  Measured on 10^6 x 32 / 5 10^5 x 64, plain | weighted (scripts/native/glds_probe.hip,
// profiles/r05_glds_probe.md): ring of 2 x 4 per CU 41.9 | 42.0 and 40.7 | 41.1 us; ring of 4 x 2 per CU 41.8 | 42.6 and
// 40.0 | 51.2 (two waves per CU cannot hide the weighted 64-column row sums); 8 KiB slots 42.3-43.7; without `nt` 46-48; the
// register-staged pipeline 46.6-47.2.
template <int MM> struct DmaShape;
template <> struct DmaShape<16> { static constexpr int ROWS = 64, D = 4; };
template <> struct DmaShape<32> { static constexpr int ROWS = 64, D = 2; };
template <> struct DmaShape<64> { static constexpr int ROWS = 32, D = 2; };

// Launches the LDS-DMA form if the rows have MM summaries and the metric takes the form at that width; says whether it did.
template <int METRIC, bool W, int MM>
static bool launch_dma(elfihip_ctx* ctx, const RowArgs& A, bool* merged) {
  if constexpr (kDma<METRIC, W, MM>) {
    if (A.m != MM) return false;
    constexpr int ROWS = DmaShape<MM>::ROWS, D = DmaShape<MM>::D;
    const size_t lds = ((size_t)D * ROWS * MM + 2 * (size_t)MM) * sizeof(double);
    // a sealed candidate list of the sampler state: workgroup 0 of the same grid merges it (the other 4 x CUs - 1 stream:
    // 15 625 slots of 10^6 x 32 still take 16 trips at most)
    const bool merge = A.M.k > 0 && A.F.thr != nullptr;
    int64_t g = (int64_t)ctx->cu_count * 4;
    const int64_t nslots = (A.n + ROWS - 1) / ROWS;
    if (g > nslots + (merge ? 1 : 0)) g = nslots + (merge ? 1 : 0);
    if (g < 1) g = 1;
    auto kernel = merge ? dist_rows_dma_kernel<METRIC, W, MM, ROWS, D, true> : dist_rows_dma_kernel<METRIC, W, MM, ROWS, D, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)g), dim3(64), lds, ctx->stream, A);
    if (merge && merged) *merged = true;
    return true;
  }
  return false;
}

template <int METRIC, bool W>
static int launch_rows(elfihip_ctx* ctx, RowArgs A, bool* filtered, bool* merged) {
  if (A.m > kMaxTileM) {
    const int64_t g = std::min<int64_t>((A.n + 3) / 4, (int64_t)ctx->cu_count * 8);   // four rows (waves) per workgroup
    hipLaunchKernelGGL((dist_rows_wide_kernel<METRIC, W>), dim3((unsigned)g), dim3(256), 0, ctx->stream, A);
    return launch_status(ctx, "dist_rows_wide_kernel");
  }
  if (narrow_rows(ctx, A)) {
    if (filtered) *filtered = A.F.thr != nullptr;   // this form offers its candidates itself, too
    return launch_narrow(ctx, A, "dist_rows_narrow_kernel",
                         [](auto M) { return dist_rows_narrow_kernel<METRIC, W, decltype(M)::value, kNarrowU>; });
  }
  // Metrics with a division or pow() per element (seuclidean, general Minkowski) keep the register-staged form below: they
  // want all lanes of more waves.
  if (A.vec2 && ctx->dist_form != 1 && METRIC != ELFIHIP_MINKOWSKI && METRIC != ELFIHIP_SEUCLIDEAN && A.ldx <= (1 << 21) &&
      (launch_dma<METRIC, W, 16>(ctx, A, merged) || launch_dma<METRIC, W, 32>(ctx, A, merged) ||
       launch_dma<METRIC, W, 64>(ctx, A, merged))) {
    if (filtered) *filtered = A.F.thr != nullptr;   // this form offers its candidates itself, too
    return launch_status(ctx, "dist_rows_dma_kernel");
  }
  if (A.vec2 && A.m <= 128) {
    // pipelined form: 128 threads, U register pairs each = one whole tile of R rows.  Small tiles win: 8 KiB in
    // flight per workgroup (32 rows of 32) with 8 workgroups per CU streams 10^6 x 32 in 47.5 us, the 32 KiB tile
    // (U = 16) in 49.6 us, 4 KiB (U = 2) in 59 us; a pure read of the buffer takes 42.5 us
    // (scripts/native/stream_probe.hip).  Also measured: 256-thread tiles and non-temporal loads, no gain.
    const int Tp = 128, U = pipe_unroll(A.m, METRIC != ELFIHIP_MINKOWSKI);
    int R = 2 * Tp * U / A.m;
    if (R > Tp) R = Tp;
    A.R = R;
    const size_t ldsp = ((size_t)R * A.mp + 2 * (size_t)A.m) * sizeof(double);
    const int gp = grid_for(ctx, (A.n + R - 1) / R, ldsp, Tp);
    with_constant<4, 8, 16>(U, [&](auto UC) {
      hipLaunchKernelGGL((dist_rows_pipe_kernel<METRIC, W, decltype(UC)::value>), dim3(gp), dim3(Tp), ldsp, ctx->stream, A);
    });
    if (filtered) *filtered = A.F.thr != nullptr;   // the pipelined form offers its candidates itself
    return launch_status(ctx, "dist_rows_pipe_kernel");
  }
  size_t lds;
  const int T = pick_block(A.m, 2 * (size_t)A.m, &lds);
  const int g = grid_for(ctx, (A.n + T - 1) / T, lds, T);
  if (T == 64) {
    ELFIHIP_TRY(set_lds(ctx, dist_rows_kernel<METRIC, W, 16>, lds));
    hipLaunchKernelGGL((dist_rows_kernel<METRIC, W, 16>), dim3(g), dim3(T), lds, ctx->stream, A);
  } else {
    hipLaunchKernelGGL((dist_rows_kernel<METRIC, W, 8>), dim3(g), dim3(T), lds, ctx->stream, A);
  }
  return launch_status(ctx, "dist_rows_kernel");
}

template <int METRIC, bool W>
static int launch_cols(elfihip_ctx* ctx, ColArgs A) {
  const int T = 256;
  int64_t work = (A.vec2 && !kRowMetric<METRIC>) ? ((A.n + 1) >> 1) : A.n;   // (the Row metrics take one row per lane)
  const int64_t g = std::max<int64_t>(1, std::min<int64_t>((work + T - 1) / T, (int64_t)ctx->cu_count * 8));
  size_t lds = 2 * (size_t)A.m * sizeof(double);
  hipLaunchKernelGGL((dist_cols_kernel<METRIC, W>), dim3((unsigned)g), dim3(T), lds, ctx->stream, A);
  return launch_status(ctx, "dist_cols_kernel");
}

// SciPy folds minkowski p=1 / p=2 / p=inf into cityblock / euclidean / chebyshev.
static int canonical_metric(elfihip_ctx* ctx, int metric, double p, const double* aux, int* out_metric) {
  *out_metric = metric;
  switch (metric) {
    case ELFIHIP_EUCLIDEAN:
    case ELFIHIP_SQEUCLIDEAN:
    case ELFIHIP_CITYBLOCK:
    case ELFIHIP_CHEBYSHEV:
    case ELFIHIP_CANBERRA:
    case ELFIHIP_BRAYCURTIS:
    case ELFIHIP_COSINE:
    case ELFIHIP_CORRELATION:
      return ELFIHIP_OK;
    case ELFIHIP_MINKOWSKI:
      if (!(p > 0.0)) return fail(ctx, ELFIHIP_ERR_ARG, "minkowski needs p > 0 (got %g)", p);
      if (p == 1.0) *out_metric = ELFIHIP_CITYBLOCK;
      if (p == 2.0) *out_metric = ELFIHIP_EUCLIDEAN;
      if (p > 1.7e308) *out_metric = ELFIHIP_CHEBYSHEV;
      return ELFIHIP_OK;
    case ELFIHIP_SEUCLIDEAN:
      return aux ? ELFIHIP_OK : fail(ctx, ELFIHIP_ERR_ARG, "seuclidean needs V");
    case ELFIHIP_MAHALANOBIS:
      return aux ? ELFIHIP_OK : fail(ctx, ELFIHIP_ERR_ARG, "mahalanobis needs VI");
    default:
      return fail(ctx, ELFIHIP_ERR_ARG, "unknown metric id %d", metric);
  }
}

// The canonical metric as a compile-time constant: f(std::integral_constant<int, METRIC>{}, std::bool_constant<W>{}).
// seuclidean always carries its V in aux: it exists in the weighted form only.
template <class F>
static int with_metric(elfihip_ctx* ctx, int cm, bool weighted, F f) {
  auto either = [&](auto M) { return weighted ? f(M, std::true_type{}) : f(M, std::false_type{}); };
  switch (cm) {
    case ELFIHIP_EUCLIDEAN: return either(std::integral_constant<int, ELFIHIP_EUCLIDEAN>{});
    case ELFIHIP_SQEUCLIDEAN: return either(std::integral_constant<int, ELFIHIP_SQEUCLIDEAN>{});
    case ELFIHIP_CITYBLOCK: return either(std::integral_constant<int, ELFIHIP_CITYBLOCK>{});
    case ELFIHIP_CHEBYSHEV: return either(std::integral_constant<int, ELFIHIP_CHEBYSHEV>{});
    case ELFIHIP_MINKOWSKI: return either(std::integral_constant<int, ELFIHIP_MINKOWSKI>{});
    case ELFIHIP_CANBERRA: return either(std::integral_constant<int, ELFIHIP_CANBERRA>{});
    case ELFIHIP_BRAYCURTIS: return either(std::integral_constant<int, ELFIHIP_BRAYCURTIS>{});
    case ELFIHIP_COSINE: return either(std::integral_constant<int, ELFIHIP_COSINE>{});
    case ELFIHIP_CORRELATION: return either(std::integral_constant<int, ELFIHIP_CORRELATION>{});
    case ELFIHIP_SEUCLIDEAN: return f(std::integral_constant<int, ELFIHIP_SEUCLIDEAN>{}, std::true_type{});
  }
  return fail(ctx, ELFIHIP_ERR_ARG, "unhandled metric %d", cm);
}

// F / filtered: fused selection (reject.hip).  *filtered tells the caller whether the kernel that ran offered the
// candidates itself; otherwise the caller filters dout in a separate pass.  M / merged: a sealed candidate list to merge
// beside the pass (with F only); *merged tells whether the launch took it (the DMA row form), otherwise the caller merges it.
int dist_rows_dev_impl(elfihip_ctx* ctx, int metric, const double* dX, int64_t n, int m, int64_t ldx, const double* dy,
                       const double* daux, double p, double* dout, const RejectFilter* F, bool* filtered,
                       const RejectMergeJob* M, bool* merged) {
  if (filtered) *filtered = false;
  if (merged) *merged = false;
  ELFIHIP_REQUIRE(ctx, n >= 0 && m >= 1, "bad shape n=%lld m=%d", (long long)n, m);
  ELFIHIP_REQUIRE(ctx, ldx >= m, "ldx (%lld) < m (%d)", (long long)ldx, m);
  ELFIHIP_REQUIRE(ctx, n == 0 || (dX && dy && dout), "NULL data pointer");
  int cm;
  ELFIHIP_TRY(canonical_metric(ctx, metric, p, daux, &cm));
  if (n == 0) return ELFIHIP_OK;
  RowArgs A = make_row_args(ctx, dX, n, m, ldx, dy, daux, p, dout);
  if (F) A.F = *F;
  if (F && M && M->k > 0 && M->k <= REJ_FUSED_MAX_K) A.M = *M;
  if (cm == ELFIHIP_MAHALANOBIS) return launch_mahalanobis(ctx, A);
  return with_metric(ctx, cm, daux != nullptr, [&](auto MC, auto WC) {
    return launch_rows<decltype(MC)::value, decltype(WC)::value>(ctx, A, filtered, merged);
  });
}

static ColArgs make_col_args(const elfihip_ctx* ctx, const double* dC, int64_t n, int m, int64_t ldc, const double* dy,
                             const double* daux, double p, double* dout) {
  return ColArgs{dC, n, ldc, dy, daux, dout, p, p != 0.0 ? 1.0 / p : 0.0, m,
                 (ldc % 2 == 0) && aligned16(dC) && aligned16(dout), stream_nt(ctx)};
}

static int dist_cols_dev_impl(elfihip_ctx* ctx, int metric, const double* dC, int64_t n, int m,
                              int64_t ldc, const double* dy, const double* daux, double p, double* dout) {
  ELFIHIP_REQUIRE(ctx, n >= 0 && m >= 1, "bad shape n=%lld m=%d", (long long)n, m);
  ELFIHIP_REQUIRE(ctx, ldc >= n, "ldc (%lld) < n (%lld)", (long long)ldc, (long long)n);
  ELFIHIP_REQUIRE(ctx, n == 0 || (dC && dy && dout), "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, metric != ELFIHIP_MAHALANOBIS, "mahalanobis needs the row-major entry point");
  int cm;
  ELFIHIP_TRY(canonical_metric(ctx, metric, p, daux, &cm));
  if (n == 0) return ELFIHIP_OK;
  const ColArgs A = make_col_args(ctx, dC, n, m, ldc, dy, daux, p, dout);
  return with_metric(ctx, cm, daux != nullptr, [&](auto MC, auto WC) {
    return launch_cols<decltype(MC)::value, decltype(WC)::value>(ctx, A);
  });
}

static size_t aux_len(int metric, int m) {
  return metric == ELFIHIP_MAHALANOBIS ? (size_t)m * m : (size_t)m;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_dist_rows_dev(elfihip_ctx* ctx, int metric, const double* dX, int64_t n, int m, int64_t ldx,
                          const double* dy, const double* daux, double p, double* dout) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return dist_rows_dev_impl(ctx, metric, dX, n, m, ldx, dy, daux, p, dout, nullptr, nullptr);
}

int elfihip_dist_cols_dev(elfihip_ctx* ctx, int metric, const double* dC, int64_t n, int m, int64_t ldc,
                          const double* dy, const double* daux, double p, double* dout) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  DeviceGuard g(ctx->device);
  return dist_cols_dev_impl(ctx, metric, dC, n, m, ldc, dy, daux, p, dout);
}

// ---- host-pointer entry points: stage, launch, copy back, synchronise (dist_launch.hpp) ---------------
int elfihip_dist_rows(elfihip_ctx* ctx, int metric, const double* X, int64_t n, int m, int64_t ldx,
                      const double* y, const double* aux, double p, double* out) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 0 && m >= 1 && ldx >= m, "bad shape n=%lld m=%d ldx=%lld", (long long)n, m,
                  (long long)ldx);
  ELFIHIP_REQUIRE(ctx, y && (n == 0 || (X && out)), "NULL data pointer");
  DeviceGuard g(ctx->device);
  double *dX, *dy, *daux;
  ELFIHIP_TRY(stage_row_call(ctx, X, n, m, ldx, y, aux, aux_len(metric, m), 1, &dX, &dy, &daux));
  ELFIHIP_TRY(dist_rows_dev_impl(ctx, metric, dX, n, m, m, dy, daux, p, ctx->out.as<double>(), nullptr, nullptr));
  return finish_host_call(ctx, out, n, 1, true);
}

// Host-pointer form of the fused distance + selection step (reject.hip): one ABC batch in, its distances out, the
// sampler state updated on the way.
int elfihip_reject_push_rows(elfihip_reject* h, int metric, const double* X, int64_t n, int m, int64_t ldx,
                             const double* y, const double* aux, double p, double* out, int64_t row_base) {
  if (!h) return fail(nullptr, ELFIHIP_ERR_ARG, "state is NULL");
  elfihip_ctx* ctx = reject_ctx(h);
  ELFIHIP_REQUIRE(ctx, n >= 0 && m >= 1 && ldx >= m, "bad shape n=%lld m=%d ldx=%lld", (long long)n, m,
                  (long long)ldx);
  ELFIHIP_REQUIRE(ctx, y && (n == 0 || X), "NULL data pointer");   // out == NULL: the distances stay on the device
  DeviceGuard g(ctx->device);
  double *dX, *dy, *daux;
  ELFIHIP_TRY(stage_row_call(ctx, X, n, m, ldx, y, aux, aux_len(metric, m), 1, &dX, &dy, &daux));
  ELFIHIP_TRY(reject_push_rows_impl(h, metric, dX, n, m, m, dy, daux, p, ctx->out.as<double>(), row_base));
  return finish_host_call(ctx, out, n, 1, false);   // (the sampler state has taken what it keeps)
}

int elfihip_dist_cols(elfihip_ctx* ctx, int metric, const double* const* cols, int m, int64_t n,
                      const double* y, const double* aux, double p, double* out) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_REQUIRE(ctx, n >= 0 && m >= 1, "bad shape n=%lld m=%d", (long long)n, m);
  ELFIHIP_REQUIRE(ctx, y && cols && (n == 0 || out), "NULL data pointer");
  ELFIHIP_REQUIRE(ctx, metric != ELFIHIP_MAHALANOBIS, "mahalanobis needs the row-major entry point");
  DeviceGuard g(ctx->device);
  double *dy, *daux;
  ELFIHIP_TRY(stage_params(ctx, y, aux, m, aux ? (size_t)m : 0, &dy, &daux));
  const int64_t ldc = (n + 1) & ~(int64_t)1;  // even pitch keeps every column 16-byte aligned
  ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve((size_t)(ldc ? ldc : 2) * m * sizeof(double)));
  double* dC = ctx->in.as<double>();
  for (int j = 0; j < m && n; ++j) {
    ELFIHIP_REQUIRE(ctx, cols[j] != nullptr, "column %d is NULL", j);
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dC + (size_t)j * ldc, cols[j], (size_t)n * sizeof(double),
                                          hipMemcpyHostToDevice, ctx->stream));
  }
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve((size_t)(ldc ? ldc : 2) * sizeof(double)));
  ELFIHIP_TRY(dist_cols_dev_impl(ctx, metric, dC, n, m, ldc ? ldc : 2, dy, daux, p, ctx->out.as<double>()));
  return finish_host_call(ctx, out, n, 1, true);
}

}  // extern "C"
