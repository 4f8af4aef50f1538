// Mahalanobis distances of rows to the observed row, sqrt(d' VI d), for gfx950 (MI355X): five kernel forms by row width,
// and launch_mahalanobis() at the end of the file, the one place that says which m takes which.
// FMA contraction is off in this file, as in the other distance kernels (distance.hip).
#include "internal.hpp"
#include "dist_launch.hpp"

#pragma clang fp contract(off)

namespace elfihip {

// The lane-per-row form: VI (m*m, row-major) is read through the scalar/L1 path.
template <int U>
__global__ void dist_rows_mahalanobis_kernel(RowArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int T = blockDim.x, tid = threadIdx.x, m = A.m;
  double* tile = lds;
  double* ys = tile + (size_t)T * A.mp;
  for (int j = tid; j < m; j += T) ys[j] = A.y[j];
  const double* __restrict__ VI = A.aux;
  const int64_t ntiles = (A.n + T - 1) / T;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * T;
    const int rows = (int)((A.n - row0) < T ? (A.n - row0) : T);
    __syncthreads();
    load_tile<U>(A, tile, row0, rows);
    __syncthreads();
    if (tid < rows) {
      double* row = tile + (size_t)tid * A.mp;
      for (int j = 0; j < m; ++j) row[j] = row[j] - ys[j];  // own row only: no hazard
      double s = 0.0;
      for (int i = 0; i < m; ++i) {
        double ti = 0.0;
        const double* vi = VI + (size_t)i * m;
        for (int k = 0; k < m; ++k) ti += row[k] * vi[k];
        s += row[i] * ti;
      }
      A.out[row0 + tid] = sqrt(s);
    }
  }
}

// Mahalanobis for 8 <= m <= 64 on the matrix cores: 2 m^2 flop per row is GEMM-shaped work (delta (rows x m) times VI) and the
// lane-per-row form above reads m^2 LDS words per row (0.72 ms for 10^6 x 32, 6.3 ms for 1.25 10^6 x 64 -- 0.05 and 0.01
// of the HBM roofline).  Here a wave owns 16 rows of the tile: T = delta VI as v_mfma_f64_16x16x4 tiles (A operand: the
// rows' differences from LDS, B operand: VI from LDS, both zero padded to the MFMA shape), then s_r = sum_c T[r][c]
// delta[r][c] folded in the accumulator layout and reduced over the 16 lanes of a row.  One MFMA per row at m = 32:
// 26 us of matrix-pipe time for 10^6 rows, below the 47 us the rows take to stream.  The order of the additions
// is the matrix core's, not SciPy's BLAS calls' (whose order is unspecified too): compared at 1e-13.
constexpr int MAHA_ROWS = 64;   // rows per tile: 16 per wave, 4 waves
typedef double v4d __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void dist_rows_mahalanobis_mfma_kernel(RowArgs A) {
  extern __shared__ __align__(16) double lds[];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, m = A.m;
  const int mk = (m + 3) & ~3, mc = (m + 15) & ~15;     // k and column extents of the padded product
  const int dp = mc | 1;                                // pitch of the difference rows (>= mc: the fold reads the padding)
  double* dl = lds;                                     // MAHA_ROWS x dp: x - y, zero beyond m
  double* vi = dl + MAHA_ROWS * dp;                     // mk x mc: VI, zero padded
  for (int e = tid; e < mk * mc; e += 256) {
    const int k = e / mc, c = e - k * mc;
    vi[e] = (k < m && c < m) ? A.aux[(size_t)k * m + c] : 0.0;
  }
  const int64_t ntiles = (A.n + MAHA_ROWS - 1) / MAHA_ROWS;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * MAHA_ROWS;
    const int rows = (int)((A.n - row0) < MAHA_ROWS ? (A.n - row0) : MAHA_ROWS);
    __syncthreads();
    for (int e = tid; e < MAHA_ROWS * dp; e += 256) {
      const int r = e / dp, c = e - r * dp;
      dl[e] = (r < rows && c < m) ? A.X[(row0 + r) * A.ldx + c] - A.y[c] : 0.0;
    }
    __syncthreads();
    const double* da = dl + (16 * w + (l & 15)) * dp + (l >> 4);   // A operand: row l & 15, k = 4 s + (l >> 4)
    double part[4] = {0.0, 0.0, 0.0, 0.0};
    for (int ct0 = 0; ct0 < mc / 16; ct0 += 4) {
      v4d acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = (v4d){0.0, 0.0, 0.0, 0.0};
      for (int s_ = 0; s_ < mk / 4; ++s_) {
        const double a = da[4 * s_];
        const double* vb = vi + (4 * s_ + (l >> 4)) * mc + 16 * ct0 + (l & 15);   // B operand: k = 4 s + (l >> 4), column l & 15
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (16 * (ct0 + j) < mc) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, vb[16 * j], acc[j], 0, 0, 0);
      }
      // accumulator element i of lane l is T[row (l >> 4) + 4 i][column 16 ct + (l & 15)]
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (16 * (ct0 + j) < mc) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            part[i] += acc[j][i] * dl[(16 * w + (l >> 4) + 4 * i) * dp + 16 * (ct0 + j) + (l & 15)];
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double v = lanes16_sum(part[i]);
      const int r = 16 * w + (l >> 4) + 4 * i;
      if ((l & 15) == 0 && r < rows) A.out[row0 + r] = sqrt(v);
    }
  }
}

// Mahalanobis on narrow rows: VI (M x M) in registers, the sums in dist_rows_mahalanobis_kernel's order (bit-identical to it).
template <int M, int U>
__global__ __launch_bounds__(256) void dist_rows_mahalanobis_narrow_kernel(RowArgs A) {
  const int tid = threadIdx.x;
  double yv[M], vi[M][M];
#pragma unroll
  for (int j = 0; j < M; ++j) {
    yv[j] = A.y[j];
#pragma unroll
    for (int k = 0; k < M; ++k) vi[j][k] = A.aux[j * M + k];
  }
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
      double d[M];
#pragma unroll
      for (int j = 0; j < M; ++j) d[j] = x[u][j] - yv[j];
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        double ti = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) ti += d[k] * vi[i][k];
        s += d[i] * ti;
      }
      if (r < A.n) A.out[r] = sqrt(s);
    }
  }
}

// The same product with VI in REGISTERS and the rows streamed like the other distance kernels (round 3: the LDS form above
// re-read its B operand from LDS for every MFMA and filled its tile with 8-byte loads behind an integer division --
// 0.59 ms for 1.25 10^6 x 64, 0.14 of the HBM roofline and an eighth of what the matrix pipes allow).  VI does not change
// between tiles: lane l keeps VI[4 s + (l >> 4)][16 j + (l & 15)] for every k step s and column tile j (KC = 4: 64
// doubles) from the first tile to the last; the rows arrive by the software-pipelined 16-byte loads of tile_stream.hpp
// (next tile in flight while this one is multiplied) as RAW x, and x - y is formed when an operand is read.
// KC = 16-column tiles of the padded row (the k extent is padded to the same 16 KC; padded entries are exact zeros).
template <int KC>
__global__ __launch_bounds__(256, 2) void dist_rows_mahalanobis_reg_kernel(RowArgs A) {   // two workgroups per CU: <= 256 registers
  extern __shared__ __align__(16) double lds[];
  constexpr int U = 8;   // 256 threads x 8 x 16 bytes = one 64 x 64 tile
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, m = A.m, mp = A.mp;
  double* tile = lds;    // MAHA_ROWS x mp raw rows (+ 64 doubles of zeros behind: operand reads beyond the last row)
  double* ys = tile + MAHA_ROWS * mp + 64;   // y padded to 16 KC entries (in LDS: 16 KC registers fewer per lane)
  for (int e = tid; e < 64; e += 256) tile[MAHA_ROWS * mp + e] = 0.0;
  for (int e = tid; e < 16 * KC; e += 256) ys[e] = e < m ? A.y[e] : 0.0;
  double b[4 * KC][KC], yc[KC];
#pragma unroll
  for (int s_ = 0; s_ < 4 * KC; ++s_) {
    const int k = 4 * s_ + (l >> 4);
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      const int c = 16 * j + (l & 15);
      b[s_][j] = (k < m && c < m) ? A.aux[(size_t)k * m + c] : 0.0;
    }
  }
#pragma unroll
  for (int j = 0; j < KC; ++j) yc[j] = (16 * j + (l & 15)) < m ? A.y[16 * j + (l & 15)] : 0.0;
  const int64_t ntiles = (A.n + MAHA_ROWS - 1) / MAHA_ROWS;
  double2 v[U];
  int64_t t = blockIdx.x;
  if (t < ntiles) tile_fetch<U>(A, t * MAHA_ROWS, (int)((A.n - t * MAHA_ROWS) < MAHA_ROWS ? (A.n - t * MAHA_ROWS) : MAHA_ROWS), v);
  for (; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * MAHA_ROWS;
    const int rows = (int)((A.n - row0) < MAHA_ROWS ? (A.n - row0) : MAHA_ROWS);
    __syncthreads();   // tile free
    tile_commit<U>(A, tile, rows, v);
    const int64_t tn = t + gridDim.x;
    if (tn < ntiles) tile_fetch<U>(A, tn * MAHA_ROWS, (int)((A.n - tn * MAHA_ROWS) < MAHA_ROWS ? (A.n - tn * MAHA_ROWS) : MAHA_ROWS), v);
    __syncthreads();
    // rows >= `rows` of a short last tile hold the previous tile's values: finite or not, they only reach their own
    // (discarded) results -- every lane's operand is its own row's
    const double* xa = tile + (16 * w + (l & 15)) * mp + (l >> 4);   // A operand: row l & 15, k = 4 s + (l >> 4)
    // one column tile at a time (ONE accumulator tile live: with all KC of them the KC = 4 instance spills beside its 64
    // registers of VI); the A operand is re-read from LDS per column tile, 16 KC ds_read_b64 against 4 KC^2 MFMAs
    double part[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < KC; ++j) {
      v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s_ = 0; s_ < 4 * KC; ++s_) {
        const int k = 4 * s_ + (l >> 4);
        const double a = k < m ? xa[4 * s_] - ys[k] : 0.0;    // (masked: the padding must not carry a neighbour's NaN)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[s_][j], acc, 0, 0, 0);
      }
      // fold with delta: accumulator element i of lane l is T[row (l >> 4) + 4 i][column 16 j + (l & 15)]
      const int c = 16 * j + (l & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double dlt = c < m ? tile[(16 * w + (l >> 4) + 4 * i) * mp + c] - yc[j] : 0.0;
        part[i] += acc[i] * dlt;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double q = lanes16_sum(part[i]);
      const int r = 16 * w + (l >> 4) + 4 * i;
      if ((l & 15) == 0 && r < rows) A.out[row0 + r] = sqrt(q);
    }
  }
}

// ---- 50 <= m <= 64 (four 16-column tiles of VI): the waves SHARE VI instead of each holding all of it ----------------
// The register form above at KC = 4 keeps 64 doubles of VI per lane beside the staging registers of the next tile: the
// compiler spilled the row addresses, and every reload (`scratch_load; s_waitcnt vmcnt(0)`) waited for ALL loads in flight
// -- the eight 16-byte loads of a tile went out one memory round trip after the other, and with the addresses repaired
// the reload moved behind the prefetch and made the MFMA loop wait for it: 12 / 9.5 us per 64-row tile, waves waiting
// 68 % of their cycles, matrix pipes busy 0.28 / 0.36 (profiles/r04_mahalanobis_pmc.md).  Here wave w owns column tile w
// of VI (16 doubles per lane) and multiplies ALL 64 rows of the tile by it -- the same 64 MFMAs per wave and tile -- and
// the four waves' shares of delta^T VI delta meet in LDS: under 128 registers, no scratch, four workgroups per CU.
// Row loads: thread (row t >> 5, column pair t & 31), eight rows apart per step; a lane beyond the row's last pair / the
// tile's last row re-reads the last valid one (no predicated loads; the commit drops it).  The tile holds delta = x - y
// (subtracted at the commit: the operand reads are the MFMA operands themselves).
// KC = column tiles of VI = 1, 2 or 4 (m <= 16, <= 32, 50 .. 64): wave w owns column tile w % KC and the KC row groups
// from (w / KC) KC on -- 4 KC^2 MFMAs per wave and tile whatever KC.  LDS row pitch 16 KC + 2 doubles: lane (row l & 15,
// k-offset l >> 4) of an operand read lands in 8-byte bank (pitch row + k-offset) mod 32, and with pitch = 2 (mod 32) (or 18)
// each half-wave covers the 32 banks once (the odd pitch m | 1 of the other kernels puts row + k-offset there: four lanes
// per bank).
template <int KC>
__global__ __launch_bounds__(256, KC == 4 ? 3 : 4) void dist_rows_mahalanobis_split_kernel(RowArgs A) {   // (KC = 4 at four per CU: 3 spills, 0.282 against 0.274 ms)
  extern __shared__ __align__(16) double lds[];
  const int tid = threadIdx.x, l = tid & 63, w = tid >> 6, m = A.m, h = m >> 1;
  constexpr int P = 16 * KC + 2;     // LDS row pitch
  constexpr int KS = 4 * KC;         // k-steps of four
  constexpr int CPB = 8 * KC;        // column pairs of a padded row: thread (row t / CPB, pair t % CPB), 256 / CPB rows per step
  constexpr int RPS = 256 / CPB, U = MAHA_ROWS / RPS;
  double* tile = lds;                // MAHA_ROWS x P: delta = x - y, zero from column m on (written once, below)
  double* red = tile + MAHA_ROWS * P;   // [column tile][row]: the waves' shares of a row's quadratic form
  for (int e = tid; e < MAHA_ROWS * P; e += 256) tile[e] = 0.0;
  const int jt = w % KC, g0 = (w / KC) * KC;
  const int c = 16 * jt + (l & 15);          // this lane's column of VI
  double b[KS];
#pragma unroll
  for (int s_ = 0; s_ < KS; ++s_) {
    const int k = 4 * s_ + (l >> 4);
    b[s_] = (k < m && c < m) ? A.aux[(size_t)k * m + c] : 0.0;
  }
  const int cp = tid % CPB, r0 = tid / CPB;
  const int cpc = cp < h ? cp : h - 1;
  const uint32_t col = 2u * (uint32_t)cpc;
  const double y0 = A.y[2 * cpc], y1 = A.y[2 * cpc + 1];
  const int64_t ntiles = (A.n + MAHA_ROWS - 1) / MAHA_ROWS;
  double2 v[U];
  // straight-line: no branch around the loads (with the loads of a tile on one of several paths the compiler's wait
  // counters are merged at the join and the first MFMA of the loop waits for the prefetch it should overlap with)
  auto fetch = [&](int64_t tt) {
    const int64_t row0 = tt * MAHA_ROWS;
    const int rows = (int)((A.n - row0) < MAHA_ROWS ? (A.n - row0) : MAHA_ROWS);
    const char* __restrict__ Xt = reinterpret_cast<const char*>(A.X + row0 * A.ldx);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = r0 + RPS * u;
      v[u] = *reinterpret_cast<const double2*>(Xt + ((uint32_t)(r < rows ? r : rows - 1) * (uint32_t)A.ldx + col) * 8u);
    }
  };
  int64_t t = blockIdx.x;
  if (t < ntiles) fetch(t);
  for (; t < ntiles; t += gridDim.x) {
    const int64_t row0 = t * MAHA_ROWS;
    const int rows = (int)((A.n - row0) < MAHA_ROWS ? (A.n - row0) : MAHA_ROWS);
    __syncthreads();   // tile free, red read (and, the first time, the zeros in place)
    if (cp < h) {
#pragma unroll
      for (int u = 0; u < U; ++u)   // (rows beyond a short last tile get copies of its last row: finite, discarded)
        *reinterpret_cast<double2*>(tile + (r0 + RPS * u) * P + 2 * cp) = make_double2(v[u].x - y0, v[u].y - y1);
    }
    const int64_t tn = t + gridDim.x;
    fetch(tn < ntiles ? tn : t);   // (beyond the last tile: this one again, dropped)
    __syncthreads();
    // the wave's KC 16-row groups side by side: independent accumulator chains (one chain of dependent MFMAs leaves the
    // matrix pipe idle between a result and the next issue whenever the SIMD's other waves are waiting too)
    const double* xa = tile + (16 * g0 + (l & 15)) * P + (l >> 4);   // A operand of group g0 + g: row 16 (g0 + g) + (l & 15), k = 4 s + (l >> 4)
    v4d acc[KC];
#pragma unroll
    for (int g = 0; g < KC; ++g) acc[g] = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s_ = 0; s_ < KS; ++s_)
#pragma unroll
      for (int g = 0; g < KC; ++g)
        acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[16 * g * P + 4 * s_], b[s_], acc[g], 0, 0, 0);
    // fold with delta: accumulator element i of lane l is T[row 16 (g0 + g) + (l >> 4) + 4 i][column c] (delta is 0 from column m on)
#pragma unroll
    for (int g = 0; g < KC; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 16 * (g0 + g) + (l >> 4) + 4 * i;
        const double q = lanes16_sum(acc[g][i] * tile[r * P + c]);   // (DPP: common.hpp; __shfl_xor here was a third of a tile's time)
        if ((l & 15) == 0) red[jt * MAHA_ROWS + r] = q;
      }
    __syncthreads();
    if (tid < rows) {
      double q = red[tid];
      if (KC == 2) q += red[MAHA_ROWS + tid];
      if (KC == 4) q = ((q + red[MAHA_ROWS + tid]) + red[2 * MAHA_ROWS + tid]) + red[3 * MAHA_ROWS + tid];
      A.out[row0 + tid] = sqrt(q);
    }
  }
}

// Which m takes which kernel.  A is complete (make_row_args); aux is VI (m x m, row-major).
//   m = 2, 4 (16-byte aligned rows)       lane-owned rows, VI in registers            dist_rows_mahalanobis_narrow_kernel
//   8 <= m <= 64, even, aligned rows      matrix cores, rows by pipelined 16-byte loads:
//       16-column tiles of VI: 1, 2, 4      the waves share VI                        dist_rows_mahalanobis_split_kernel
//       3                                   every wave holds all of VI (a fourth wave would be left without a column
//                                           tile in the split form)                   dist_rows_mahalanobis_reg_kernel
//   8 <= m <= 64 otherwise                matrix cores, operands from LDS             dist_rows_mahalanobis_mfma_kernel
//   every other m <= 299                  lane per row, VI through the scalar / L1 path (below 8 the padding to the
//                                         16-wide tile costs more than this form)     dist_rows_mahalanobis_kernel
int launch_mahalanobis(elfihip_ctx* ctx, const RowArgs& A) {
  const int m = A.m;
  const int64_t ntiles = (A.n + MAHA_ROWS - 1) / MAHA_ROWS;
  ELFIHIP_REQUIRE(ctx, m <= kMaxTileM, "mahalanobis supports m <= %d", kMaxTileM);
  if (narrow_rows(ctx, A))
    return launch_narrow(ctx, A, "dist_rows_mahalanobis_narrow_kernel",
                         [](auto M) { return dist_rows_mahalanobis_narrow_kernel<decltype(M)::value, kNarrowU>; });
  if (m >= 8 && m <= 64 && A.vec2 && A.ldx < (1 << 22)) {
    const int kc = (m + 15) / 16;
    if (kc != 3) {
      const size_t lb = ((size_t)MAHA_ROWS * (16 * kc + 2) + (size_t)kc * MAHA_ROWS) * sizeof(double);
      int g = grid_for(ctx, ntiles, lb, 256);
      const int per_cu = kc == 4 ? 3 : (kc == 2 ? 5 : 8);   // workgroups per CU by registers (measured: m = 32 0.128 ms with 3, 0.075 with 5)
      if (g > per_cu * ctx->cu_count) g = per_cu * ctx->cu_count;
      with_constant<4, 2, 1>(kc, [&](auto KC) {
        hipLaunchKernelGGL((dist_rows_mahalanobis_split_kernel<decltype(KC)::value>), dim3(g), dim3(256), lb, ctx->stream, A);
      });
      return launch_status(ctx, "dist_rows_mahalanobis_split_kernel");
    }
    const size_t lb = ((size_t)MAHA_ROWS * A.mp + 64 + 64) * sizeof(double);
    hipLaunchKernelGGL((dist_rows_mahalanobis_reg_kernel<3>), dim3(grid_for(ctx, ntiles, lb, 256)), dim3(256), lb, ctx->stream, A);
    return launch_status(ctx, "dist_rows_mahalanobis_reg_kernel");
  }
  if (m >= 8 && m <= 64) {
    const int mk = (m + 3) & ~3, mc = (m + 15) & ~15;
    const size_t lb = ((size_t)MAHA_ROWS * (mc | 1) + (size_t)mk * mc) * sizeof(double);
    ELFIHIP_TRY(set_lds(ctx, dist_rows_mahalanobis_mfma_kernel, lb));
    hipLaunchKernelGGL(dist_rows_mahalanobis_mfma_kernel, dim3(grid_for(ctx, ntiles, lb, 256)), dim3(256), lb, ctx->stream, A);
    return launch_status(ctx, "dist_rows_mahalanobis_mfma_kernel");
  }
  size_t lds;
  const int T = pick_block(m, (size_t)m, &lds);
  ELFIHIP_TRY(set_lds(ctx, dist_rows_mahalanobis_kernel<8>, lds));
  hipLaunchKernelGGL((dist_rows_mahalanobis_kernel<8>), dim3(grid_for(ctx, (A.n + T - 1) / T, lds, T)), dim3(T), lds, ctx->stream, A);
  return launch_status(ctx, "dist_rows_mahalanobis_kernel");
}

}  // namespace elfihip
