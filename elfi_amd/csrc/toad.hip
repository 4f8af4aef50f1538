// Marchand's toad movement model (elfi/examples/toad.py) and An, Nott and Drovandi's summaries, fused: one workgroup per
// simulation keeps the (n_days, n_toads) positions and one sort buffer in LDS.
//
//   phase A  every lane takes cells (day i >= 1, toad j): the four draws of the cell (given, or from the generator --
//            include/elfihip.h has the rule), the return decision U < p0 and the alpha-stable step (stable.hpp).  This is
//            the Philox and transcendental work and does not depend on the state.  The step waits in the cell's own slot
//            of X; the decision and the refuge day wait as a 16-bit code in the (still unused) sort buffer.
//   phase B  a lane per toad walks its chain of n_days - 1 cells: X[i] = X[refuge] where the toad returned, X[i - 1] + step
//            otherwise.  Toads do not interact, so the chains need no barrier; only this part is serial.
//   phase C  per lag: all lanes form |X[i + lag] - X[i]|; the returned ones (< thd) are counted, NaN is dropped (as
//            np.nanquantile drops it), the rest are compacted into the buffer -- a ballot and one LDS atomic per wavefront
//            for each of the two counts -- padded to a power of two with +inf and sorted by the workgroup (wg_sort.hpp).
//            Lanes then read the quantile positions of np.nanquantile (method 'linear': NumPy's _lerp, as series.hip does
//            for M/G/1), np.nanmedian's middle and the log differences.
//
// LDS: 8 n_days n_toads bytes of positions + the buffer (the displacement count of the smallest lag rounded up to a power
// of two, and a seventeenth word per sixteen for the sort's bank layout, 8 bytes each; at least 2 bytes per cell for the
// codes) -- 33 264 + 34 816 bytes at 63 x 66, two workgroups on a CU's 160 KB; 64 + 68 KB at the limit n_days n_toads = 8192.
//
// Every expression keeps NumPy's operation order, FMA contraction off: on given steps X is NumPy's bit for bit, and on X
// so are the counts and medians; the log differences differ by the device's log.
#include "common.hpp"

#include <algorithm>

#include "stable.hpp"
#include "wg_sort.hpp"

#pragma clang fp contract(off)

namespace elfihip {

constexpr int TOAD_THREADS = 256;
constexpr double TOAD_EXPM20 = 0x1.1b48655f37267p-29;   // np.exp(-20); np.log of it is -20 exactly
constexpr double TOAD_F64_MAX = 0x1.fffffffffffffp+1023;
constexpr unsigned TOAD_BAD_REFUGE = 0xFFFFu;

struct ToadArgs {
  const double* U;      // (n, ldd) given draws of the cells (day - 1) n_toads + toad, or NULL: drawn here
  const double* TH;
  const double* W;
  const int32_t* R;
  int64_t ldd;
  uint64_t seed, stream;
  uint32_t first;
  int64_t n;
  int nt, nd, nlags, nq;
  int lags[ELFIHIP_TOAD_MAX_LAGS];
  double p[ELFIHIP_TOAD_MAX_QUANTILES];
  double thd;
  const double* alpha;
  const double* gamma;
  const double* p0;
  double* S;            // (n, lds) summaries, (nq + 1) per lag
  int64_t lds;
  double* X;            // (n, ldx) positions, row-major (day, toad), or NULL
  int64_t ldx;
  double* Dx;           // (n, lddx) steps of the cells, or NULL
  int64_t lddx;
  double* Uo;           // (n, ldo) the draws used, or NULL (all four or none)
  double* THo;
  double* Wo;
  int32_t* Ro;
  int64_t ldo;
};

// np.nan_to_num(x, nan=np.inf): NaN -> +inf, and the infinities to the largest finite doubles
__device__ __forceinline__ double toad_fix(double x) {
  if (x != x) return __builtin_inf();
  if (x == __builtin_inf()) return TOAD_F64_MAX;
  if (x == -__builtin_inf()) return -TOAD_F64_MAX;
  return x;
}

__global__ __launch_bounds__(TOAD_THREADS) void toad_kernel(const ToadArgs A) {
  extern __shared__ double toad_lds[];
  __shared__ double qv[ELFIHIP_TOAD_MAX_QUANTILES];
  __shared__ int cnt[2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int nt = A.nt, nd = A.nd, cells = (nd - 1) * nt, ncol = A.nq + 1;
  double* X = toad_lds;
  unsigned long long* key = reinterpret_cast<unsigned long long*>(toad_lds + nd * nt);
  unsigned short* code = reinterpret_cast<unsigned short*>(key);
  const double* sorted = reinterpret_cast<const double*>(key);

  for (int64_t row = blockIdx.x; row < A.n; row += gridDim.x) {
    const double alpha = A.alpha[row], gamma = A.gamma[row], p0 = A.p0[row];
    const bool valid = stable_valid(alpha, gamma) && p0 >= 0.0 && p0 <= 1.0;
    const uint64_t g = (uint64_t)A.first + (uint64_t)row;

    // ---- phase A: draws, decisions and steps of every cell
    for (int c = tid; c < cells; c += TOAD_THREADS) {
      const int i = c / nt + 1, j = c - (i - 1) * nt;
      double U, TH, W;
      int r;
      if (A.U) {
        const int64_t o = row * A.ldd + c;
        U = A.U[o];
        TH = A.TH[o];
        W = A.W[o];
        r = A.R[o];
      } else {
        const uint64_t e = (g << 32) | ((uint64_t)i << 16) | (uint64_t)j;
        stable_angle_expo(A.seed, A.stream, e, TH, W);
        const uint64_t s1 = A.stream + 1;
        uint32_t w[4];
        philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), (uint32_t)s1, (uint32_t)(s1 >> 32), (uint32_t)A.seed,
                      (uint32_t)(A.seed >> 32), w);
        U = unit_co(word53(w[0], w[1]));
        r = (int)__umulhi(w[2], (uint32_t)i);
      }
      const double dx = valid ? stable_transform(alpha, gamma, TH, W) : __builtin_nan("");
      if (A.Dx) A.Dx[row * A.lddx + c] = dx;
      if (A.Uo) {
        const int64_t o = row * A.ldo + c;
        A.Uo[o] = U;
        A.THo[o] = TH;
        A.Wo[o] = W;
        A.Ro[o] = r;
      }
      X[nt + c] = dx;
      code[c] = (unsigned short)(U < p0 ? ((r >= 0 && r < i) ? (unsigned)(r + 1) : TOAD_BAD_REFUGE) : 0u);
    }
    for (int j = tid; j < nt; j += TOAD_THREADS) X[j] = 0.0;
    __syncthreads();

    if (!valid) {
      // an invalid parameter row: NaN summaries and positions; the neighbours are other workgroups' rows
      for (int k = tid; k < ncol * A.nlags; k += TOAD_THREADS) A.S[row * A.lds + k] = __builtin_nan("");
      if (A.X)
        for (int e = tid; e < nd * nt; e += TOAD_THREADS) A.X[row * A.ldx + e] = __builtin_nan("");
      __syncthreads();
      continue;
    }

    // ---- phase B: a lane per toad walks its chain
    for (int j = tid; j < nt; j += TOAD_THREADS) {
      double prev = 0.0;
      for (int i = 1; i < nd; ++i) {
        const unsigned cd = code[(i - 1) * nt + j];
        double x;
        if (cd == 0u)
          x = prev + X[i * nt + j];
        else if (cd == TOAD_BAD_REFUGE)
          x = __builtin_nan("");
        else
          x = X[(int)(cd - 1u) * nt + j];
        X[i * nt + j] = x;
        prev = x;
      }
    }
    __syncthreads();
    if (A.X)
      for (int e = tid; e < nd * nt; e += TOAD_THREADS) A.X[row * A.ldx + e] = X[e];

    // ---- phase C: the summaries of every lag
    for (int l = 0; l < A.nlags; ++l) {
      const int lag = A.lags[l], m = nt * (nd - lag), sh = lag * nt;
      if (tid < 2) cnt[tid] = 0;
      __syncthreads();
      for (int base = 0; base < m; base += TOAD_THREADS) {   // every lane makes every trip: the ballots are whole
        const int e = base + tid;
        bool keep = false, ret = false;
        double d = 0.0;
        if (e < m) {
          d = fabs(X[e + sh] - X[e]);
          ret = d < A.thd;
          keep = !ret && d == d;
        }
        const unsigned long long mk = __ballot(keep), mr = __ballot(ret);
        int b = 0;
        if (lane == 0) {
          if (mr) atomicAdd(&cnt[0], __popcll(mr));
          if (mk) b = atomicAdd(&cnt[1], __popcll(mk));
        }
        b = __builtin_amdgcn_readfirstlane(b);
        if (keep) key[wg_sort_slot(b + __popcll(mk & ((1ull << lane) - 1ull)))] = (unsigned long long)__double_as_longlong(d);
      }
      __syncthreads();
      const int nret = cnt[0], nk = cnt[1];
      const int P = wg_sort_padded(nk);
      for (int e = nk + tid; e < P; e += TOAD_THREADS) key[wg_sort_slot(e)] = ELFIHIP_F64_INF_BITS;
      __syncthreads();
      wg_sort_u64(key, P, tid, TOAD_THREADS);

      if (tid < A.nq) {
        // np.nanquantile, method 'linear': virtual index (nk - 1) p, its two neighbours and _lerp; at the upper end NumPy
        // names both neighbours -1 and measures the weight from that name
        double q = __builtin_nan("");
        if (nk > 0) {
          const double virt = (double)(nk - 1) * A.p[tid];
          int lo, hi;
          double t;
          if (virt >= (double)(nk - 1)) {
            lo = hi = nk - 1;
            t = virt - (-1.0);
          } else {
            const double prev = floor(virt);
            lo = (int)prev;
            hi = lo + 1;
            t = virt - prev;
          }
          const double a = sorted[wg_sort_slot(lo)], b = sorted[wg_sort_slot(hi)], diff = b - a;
          q = t >= 0.5 ? b - diff * (1.0 - t) : a + diff * t;
        }
        qv[tid] = q;
      }
      __syncthreads();
      double* s = A.S + row * A.lds + (int64_t)l * ncol;
      if (tid == 0) s[0] = (double)nret;
      if (tid == 1) {
        // np.nanmedian: the mean of the two middle values; below 600 displacements NumPy's masked-array path also forms
        // (x + x) / 2 of a single middle value
        double med = __builtin_nan("");
        if (nk > 0) {
          const int h = nk >> 1;
          const double hi = sorted[wg_sort_slot(h)], lo = (nk & 1) ? hi : sorted[wg_sort_slot(h - 1)];
          med = ((nk & 1) && m >= 600) ? hi : (lo + hi) / 2.0;
        }
        s[1] = toad_fix(med);
      }
      if (tid >= 2 && tid < ncol) {
        const double d = qv[tid - 1] - qv[tid - 2];
        s[tid] = toad_fix(d != d ? d : (d <= TOAD_EXPM20 ? -20.0 : log(d)));
      }
      __syncthreads();
    }
  }
}

static size_t toad_buffer_doubles(int nt, int nd, int nlags, const int* lags) {
  int minlag = lags[0];
  for (int l = 1; l < nlags; ++l) minlag = std::min(minlag, lags[l]);
  const size_t P = (size_t)wg_sort_words(wg_sort_padded(nt * (nd - minlag))), codes = ((size_t)(nd - 1) * nt + 3) / 4;
  return std::max(P, codes);
}

static int toad_check(elfihip_ctx* ctx, int64_t first_index, int64_t n, int n_toads, int n_days, int n_lags, const int* lags,
                      int nq, const double* p, double thd) {
  ELFIHIP_REQUIRE(ctx, n >= 1, "need at least one simulation");
  ELFIHIP_REQUIRE(ctx, first_index >= 0 && first_index <= (int64_t)0x100000000ll - n,
                  "simulation indices first_index .. first_index + n - 1 must lie in [0, 2^32)");
  ELFIHIP_REQUIRE(ctx, n_days >= 2 && n_toads >= 1 && (int64_t)n_days * n_toads <= ELFIHIP_TOAD_MAX_CELLS,
                  "need n_days >= 2, n_toads >= 1 and n_days n_toads <= %d", ELFIHIP_TOAD_MAX_CELLS);
  ELFIHIP_REQUIRE(ctx, n_lags >= 1 && n_lags <= ELFIHIP_TOAD_MAX_LAGS && lags, "1 to %d lags", ELFIHIP_TOAD_MAX_LAGS);
  for (int l = 0; l < n_lags; ++l)
    ELFIHIP_REQUIRE(ctx, lags[l] >= 1 && lags[l] <= n_days - 1, "lag %d outside [1, n_days - 1]", lags[l]);
  ELFIHIP_REQUIRE(ctx, nq >= 1 && nq <= ELFIHIP_TOAD_MAX_QUANTILES && p, "1 to %d quantiles", ELFIHIP_TOAD_MAX_QUANTILES);
  for (int k = 0; k < nq; ++k)
    ELFIHIP_REQUIRE(ctx, p[k] >= 0.0 && p[k] <= 1.0 && (k == 0 || p[k] > p[k - 1]), "quantiles must increase within [0, 1]");
  ELFIHIP_REQUIRE(ctx, thd == thd, "thd is NaN");
  return ELFIHIP_OK;
}

}  // namespace elfihip

using namespace elfihip;

extern "C" {

int elfihip_toad_summaries_dev(elfihip_ctx* ctx, const double* dU, const double* dTH, const double* dW, const int32_t* dR,
                               int64_t ldd, uint64_t seed, uint64_t stream, int64_t first_index, int64_t n, int n_toads,
                               int n_days, int n_lags, const int* lags, int nq, const double* p, double thd,
                               const double* dalpha, const double* dgamma, const double* dp0, double* dS, int64_t lds,
                               double* dX, int64_t ldx, double* dDx, int64_t lddx, double* dUo, double* dTHo, double* dWo,
                               int32_t* dRo, int64_t ldo) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(toad_check(ctx, first_index, n, n_toads, n_days, n_lags, lags, nq, p, thd));
  const int64_t cells = (int64_t)(n_days - 1) * n_toads;
  const bool given = dU || dTH || dW || dR, echo = dUo || dTHo || dWo || dRo;
  ELFIHIP_REQUIRE(ctx, !given || (dU && dTH && dW && dR && ldd >= cells), "the four draw arrays are given together, at a pitch of at least (n_days - 1) n_toads");
  ELFIHIP_REQUIRE(ctx, !echo || (dUo && dTHo && dWo && dRo && ldo >= cells), "the four draw outputs are asked for together, at a pitch of at least (n_days - 1) n_toads");
  ELFIHIP_REQUIRE(ctx, dalpha && dgamma && dp0 && dS && lds >= (int64_t)(nq + 1) * n_lags, "parameters and summaries are needed, the summaries at a pitch of at least (nq + 1) n_lags");
  ELFIHIP_REQUIRE(ctx, (!dX || ldx >= (int64_t)n_days * n_toads) && (!dDx || lddx >= cells), "an output pitch is shorter than its row");
  DeviceGuard g(ctx->device);
  ToadArgs A;
  A.U = dU, A.TH = dTH, A.W = dW, A.R = dR, A.ldd = ldd;
  A.seed = seed, A.stream = stream, A.first = (uint32_t)first_index, A.n = n;
  A.nt = n_toads, A.nd = n_days, A.nlags = n_lags, A.nq = nq;
  for (int l = 0; l < ELFIHIP_TOAD_MAX_LAGS; ++l) A.lags[l] = l < n_lags ? lags[l] : 1;
  for (int k = 0; k < ELFIHIP_TOAD_MAX_QUANTILES; ++k) A.p[k] = k < nq ? p[k] : 0.0;
  A.thd = thd;
  A.alpha = dalpha, A.gamma = dgamma, A.p0 = dp0;
  A.S = dS, A.lds = lds, A.X = dX, A.ldx = ldx, A.Dx = dDx, A.lddx = lddx;
  A.Uo = dUo, A.THo = dTHo, A.Wo = dWo, A.Ro = dRo, A.ldo = ldo;
  const size_t lds_bytes = ((size_t)n_days * n_toads + toad_buffer_doubles(n_toads, n_days, n_lags, lags)) * sizeof(double);
  ELFIHIP_TRY(set_lds(ctx, toad_kernel, lds_bytes, 48 * 1024));
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (size_t)(150 * 1024) / (lds_bytes + 1024)));
  const unsigned grid = (unsigned)std::min<int64_t>(n, (int64_t)ctx->cu_count * per_cu);
  hipLaunchKernelGGL(toad_kernel, dim3(grid), dim3(TOAD_THREADS), lds_bytes, ctx->stream, A);
  return launch_status(ctx, "toad_kernel");
}

int elfihip_toad_summaries(elfihip_ctx* ctx, const double* U, const double* TH, const double* W, const int32_t* R, uint64_t seed,
                           uint64_t stream, int64_t first_index, int64_t n, int n_toads, int n_days, int n_lags, const int* lags,
                           int nq, const double* p, double thd, const double* alpha, const double* gamma, const double* p0,
                           double* S, double* X, double* Dx, double* Uo, double* THo, double* Wo, int32_t* Ro) {
  if (!ctx) return fail(nullptr, ELFIHIP_ERR_ARG, "ctx is NULL");
  ELFIHIP_TRY(toad_check(ctx, first_index, n, n_toads, n_days, n_lags, lags, nq, p, thd));
  const bool given = U || TH || W || R, echo = Uo || THo || Wo || Ro;
  ELFIHIP_REQUIRE(ctx, !given || (U && TH && W && R), "the four draw arrays are given together");
  ELFIHIP_REQUIRE(ctx, !echo || (Uo && THo && Wo && Ro), "the four draw outputs are asked for together");
  ELFIHIP_REQUIRE(ctx, alpha && gamma && p0 && S, "parameters and summaries are needed");
  DeviceGuard g(ctx->device);
  const size_t cells = (size_t)(n_days - 1) * n_toads, grid_cells = (size_t)n_days * n_toads, ns = (size_t)(nq + 1) * n_lags;
  const size_t N = (size_t)n, d8 = sizeof(double);
  // staging: parameters | given draws (three double arrays and the int32 one) | outputs
  ELFIHIP_CHECK_HIP(ctx, ctx->par.reserve(3 * N * d8));
  double* dpar = ctx->par.as<double>();
  const double* hp[3] = {alpha, gamma, p0};
  for (int k = 0; k < 3; ++k)
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dpar + k * N, hp[k], N * d8, hipMemcpyHostToDevice, ctx->stream));
  double *dU = nullptr, *dTH = nullptr, *dW = nullptr;
  int32_t* dR = nullptr;
  if (given) {
    ELFIHIP_CHECK_HIP(ctx, ctx->in.reserve(N * cells * (3 * d8 + sizeof(int32_t))));
    dU = ctx->in.as<double>(), dTH = dU + N * cells, dW = dTH + N * cells;
    dR = reinterpret_cast<int32_t*>(dW + N * cells);
    const double* hd[3] = {U, TH, W};
    double* dd[3] = {dU, dTH, dW};
    for (int k = 0; k < 3; ++k)
      ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dd[k], hd[k], N * cells * d8, hipMemcpyHostToDevice, ctx->stream));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(dR, R, N * cells * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
  }
  const size_t out_doubles = N * (ns + (X ? grid_cells : 0) + (Dx ? cells : 0) + (echo ? 3 * cells : 0));
  ELFIHIP_CHECK_HIP(ctx, ctx->out.reserve(out_doubles * d8 + (echo ? N * cells * sizeof(int32_t) : 0)));
  double* o = ctx->out.as<double>();
  double* dS = o;
  o += N * ns;
  double* dX = X ? o : nullptr;
  o += X ? N * grid_cells : 0;
  double* dDx = Dx ? o : nullptr;
  o += Dx ? N * cells : 0;
  double *dUo = nullptr, *dTHo = nullptr, *dWo = nullptr;
  int32_t* dRo = nullptr;
  if (echo) {
    dUo = o, dTHo = o + N * cells, dWo = o + 2 * N * cells;
    dRo = reinterpret_cast<int32_t*>(o + 3 * N * cells);
  }
  ELFIHIP_TRY(elfihip_toad_summaries_dev(ctx, dU, dTH, dW, dR, (int64_t)cells, seed, stream, first_index, n, n_toads, n_days,
                                         n_lags, lags, nq, p, thd, dpar, dpar + N, dpar + 2 * N, dS, (int64_t)ns, dX,
                                         (int64_t)grid_cells, dDx, (int64_t)cells, dUo, dTHo, dWo, dRo, (int64_t)cells));
  ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(S, dS, N * ns * d8, hipMemcpyDeviceToHost, ctx->stream));
  if (X) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(X, dX, N * grid_cells * d8, hipMemcpyDeviceToHost, ctx->stream));
  if (Dx) ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Dx, dDx, N * cells * d8, hipMemcpyDeviceToHost, ctx->stream));
  if (echo) {
    double* ho[3] = {Uo, THo, Wo};
    double* dd[3] = {dUo, dTHo, dWo};
    for (int k = 0; k < 3; ++k)
      ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(ho[k], dd[k], N * cells * d8, hipMemcpyDeviceToHost, ctx->stream));
    ELFIHIP_CHECK_HIP(ctx, hipMemcpyAsync(Ro, dRo, N * cells * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  }
  ELFIHIP_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ELFIHIP_OK;
}

}  // extern "C"
