/*
 * elfihip.h -- C ABI of libelfihip.so: the MI355X (gfx950) hot path for ELFI.
 *
 * Drop-in boundary.  Every entry point replaces one piece of
 * arithmetic that reference ELFI (v0.8.7, /root/reference) delegates to SciPy / GPy /
 * NumPy on the host.  The reference site each function stands in for is cited next
 * to its declaration as `elfi/<file>:<lines>`.
 *
 * Conventions
 *  - plain C types only: pointers, sizes, doubles.  No torch / numpy types.
 *  - every function returns an int status (ELFIHIP_OK == 0); the text of the last
 *    failure on a context is available from elfihip_last_error().
 *  - "host" entry points take HOST pointers; the library stages through device
 *    buffers it owns and never keeps a caller pointer after it returns.
 *  - "_dev" twins take DEVICE pointers (every pointer argument, including the small
 *    y / w vectors), enqueue on the context's stream and return without
 *    synchronising; results are ordered with later work on the same stream.  Where a _dev
 *    form takes a small HOST array (it says so below), the array may be overwritten as soon
 *    as the call has returned; the entry points that do wait for the stream say so below
 *    (elfihip_subset_best_dev, elfihip_adaptive_push_dev's first-batch check, and pushes,
 *    elfihip_reject_flush and elfihip_reject_state_dev on host-merge states).
 *    tests/test_stream_order_gpu.py holds every _dev entry point to this
 *    on an adopted stream that is busy.
 *  - a context is bound to one GPU and one HIP stream; it is not thread-safe, but
 *    distinct contexts may be used from distinct threads.
 *  - all floating point is IEEE binary64; row sums are accumulated in the same
 *    left-to-right order SciPy's cdist uses, with FMA contraction disabled, so the
 *    euclidean / cityblock / chebyshev families reproduce cdist bit for bit.
 */
#ifndef ELFIHIP_H
#define ELFIHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ELFIHIP_VERSION 100 /* 0.1.0 */

/* status codes */
enum {
  ELFIHIP_OK = 0,
  ELFIHIP_ERR_ARG = 1,      /* bad argument / shape -> ValueError on the Python side   */
  ELFIHIP_ERR_HIP = 2,      /* HIP runtime failure  -> RuntimeError                      */
  ELFIHIP_ERR_NOT_PD = 3,   /* Cholesky met a non-positive pivot -> np.linalg.LinAlgError */
  ELFIHIP_ERR_STATE = 4,    /* call made in the wrong state (e.g. predict before factor) */
  ELFIHIP_ERR_NOMEM = 5
};

/* metrics of scipy.spatial.distance.cdist that elfi.Distance accepts by name
 * (elfi/model/elfi_model.py:1020-1037). */
enum {
  ELFIHIP_EUCLIDEAN = 0,   /* sqrt(sum w_j (x_j-y_j)^2)            */
  ELFIHIP_SQEUCLIDEAN = 1, /* sum w_j (x_j-y_j)^2                  */
  ELFIHIP_CITYBLOCK = 2,   /* sum w_j |x_j-y_j|                    */
  ELFIHIP_CHEBYSHEV = 3,   /* max_j |x_j-y_j|   (w ignored unless 0: SciPy drops w_j==0 columns) */
  ELFIHIP_MINKOWSKI = 4,   /* (sum w_j |x_j-y_j|^p)^(1/p)          */
  ELFIHIP_SEUCLIDEAN = 5,  /* sqrt(sum (x_j-y_j)^2 / V_j), aux = V */
  ELFIHIP_MAHALANOBIS = 6, /* sqrt(d' VI d), aux = VI (m x m row-major) */
  ELFIHIP_CANBERRA = 7,    /* sum w_j |x_j-y_j| / (|x_j|+|y_j|)   (a 0/0 term counts 0) */
  ELFIHIP_BRAYCURTIS = 8,  /* sum w_j |x_j-y_j| / sum w_j |x_j+y_j| */
  ELFIHIP_COSINE = 9,      /* 1 - x.y / (|x| |y|)   (w: weighted dots with w / sum w) */
  ELFIHIP_CORRELATION = 10 /* cosine of x - mean(x) and y - mean(y)  (w: weighted means and dots) */
};

typedef struct elfihip_ctx elfihip_ctx;
typedef struct elfihip_gp elfihip_gp;

/* ------------------------------------------------------------------ context */
int elfihip_version(void);
int elfihip_device_count(int* count);
/* device < 0: use the current HIP device. */
int elfihip_ctx_create(int device, elfihip_ctx** ctx);
int elfihip_ctx_destroy(elfihip_ctx* ctx);
/* Text of the last error on ctx (or the last context-less error if ctx == NULL). */
const char* elfihip_last_error(const elfihip_ctx* ctx);
/* Adopt an externally owned hipStream_t (e.g. torch's current stream); NULL restores
 * the context's own stream.  The own stream is NON-BLOCKING: it is not ordered against
 * the null stream or any other stream, so a caller that fills device buffers elsewhere
 * (the *_dev entry points) either adopts that stream here or synchronises it before the
 * call; the *_dev entry points themselves are asynchronous on the context's stream.
 * They are not the only ones: elfihip_gp_factorize, elfihip_gp_extend and
 * elfihip_gp_nlml_grad wait for a ticket, not for the stream, and return while rows of
 * alpha are still being written on it.  A caller that switches streams synchronises the
 * old one first (as tests/stream_order.py: adopted_stream does); this call does not. */
int elfihip_ctx_set_stream(elfihip_ctx* ctx, void* hip_stream);
int elfihip_ctx_synchronize(elfihip_ctx* ctx);
/* Device properties the roofline needs: CU count, clock (kHz), memory clock (kHz),
 * bus width (bits), total global memory (bytes).  Any pointer may be NULL. */
/* Page-locked host memory for results that leave the device in bulk (the (n, m) rows of a device-side simulator: a
 * pageable destination takes the copy at ~1 GB/s on first touch, a pinned one at PCIe speed).  Not tied to a context. */
int elfihip_host_alloc(size_t bytes, void** out);
int elfihip_host_free(void* p);
int elfihip_device_info(elfihip_ctx* ctx, int* cu_count, int* clock_khz, int* mem_clock_khz,
                        int* mem_bus_bits, int64_t* total_mem, char* name, int name_len);

/* Kernel timing with HIP events on the context's stream (bench.py's roofline leg). */
int elfihip_timer_start(elfihip_ctx* ctx);
int elfihip_timer_stop(elfihip_ctx* ctx, float* elapsed_ms); /* synchronises on the stop event */

/* ----------------------------------------------------------------- distance
 * Replaces scipy.spatial.distance.cdist(X (n,m), Y (1,m), metric, p=, w=, V=, VI=)
 * as called from distance_as_discrepancy (elfi/model/utils.py:37-52) through
 * elfi.Distance (elfi/model/elfi_model.py:1037) and AdaptiveDistance (:1084).
 * out has n doubles -- the (n,1)->(n,) squeeze of utils.py:50-51 is built in.
 *
 * aux: w (m) for EUCLIDEAN/SQEUCLIDEAN/CITYBLOCK/MINKOWSKI/CHEBYSHEV/CANBERRA/BRAYCURTIS/COSINE/CORRELATION
 *      (NULL = unweighted), V (m) for SEUCLIDEAN, VI (m*m, row-major) for MAHALANOBIS.  p only for MINKOWSKI.
 * Ids 0..10 are the canonical metrics.  The Python layer (elfi_amd/_lib.py: METRIC_NAMES) also takes SciPy's aliases,
 * in any letter case: e eu euclid | sqe sqeuclid | c cb cblock | ch cheb cheby chebychev | m mi pnorm | s se |
 * mah mahal | cos | co (canberra and braycurtis have none).
 * canberra, braycurtis, cosine and correlation sum in SciPy's order (cosine: SciPy's two-lane dot products; correlation:
 * the row mean in NumPy's pairwise order) and match cdist bit for bit up to m = 299, except weighted cosine / correlation
 * (1e-13: SciPy's np.dot order is its BLAS's); wider rows are summed by a butterfly (1e-14).
 */

/* X row-major (n, m) with leading dimension ldx >= m (doubles).
 *
 * Layout contract of the _dev row entry points (elfihip_dist_rows_dev, _dist_multiw_dev, _reject_push_rows_dev,
 * _reject_push_multiw_dev, _adaptive_push_dev, _row_summary_dev, _ma2_distance_dev, _welford_update_dev,
 * _weighted_var_dev): ANY ldx >= m and ANY 8-byte aligned dX are correct -- a view of a wider device matrix needs no
 * copy -- and so is any 8-byte aligned result pointer (dout, and a (n, K) dout at any such address: the kernels that write
 * results in 16-byte pieces test dout themselves and store single doubles otherwise).  The fast paths (16-byte row loads:
 * the narrow, pipelined, LDS-DMA, matrix-core Mahalanobis and fused adaptive kernels) need m even, ldx even and dX 16-byte
 * aligned; every other layout takes the 8-byte-load kernels, whose results are the same up to the documented tolerance of
 * the metric (bit for bit for the exact metrics).  Two forms address a tile's rows with 32-bit offsets and are taken only
 * below a pitch limit: the LDS-DMA row form for ldx <= 2^21, the matrix-core Mahalanobis kernels for ldx < 2^22; above,
 * the register-staged forms run.  elfihip_dist_cols_dev reads and writes two rows per lane when ldc is even and dC and dout
 * are both 16-byte aligned, and one row per lane otherwise.  tests/test_device_layouts_gpu.py runs every one of them at
 * packed, even, odd and offset layouts. */
int elfihip_dist_rows(elfihip_ctx* ctx, int metric, const double* X, int64_t n, int m, int64_t ldx,
                      const double* y, const double* aux, double p, double* out);
int elfihip_dist_rows_dev(elfihip_ctx* ctx, int metric, const double* dX, int64_t n, int m,
                          int64_t ldx, const double* dy, const double* daux, double p,
                          double* dout);

/* How the row-major distance calls stream their matrix (no reference counterpart; results are bit-identical either way):
 * 0 (default) rows of 16 / 32 / 64 summaries with 16-byte aligned rows arrive in LDS by LDS-DMA (global_load_lds, rings
 * of two 16 KiB slots per wave, non-temporal) -- every other shape, and 1 always, takes the register-staged pipeline;
 * any other form is ELFIHIP_ERR_ARG.  An LDS-DMA form of the fused adaptive-distance pass (elfihip_adaptive_push) was
 * built, measured slower than its register-staged form and removed (profiles/r05_adaptive_dma.md). */
int elfihip_dist_set_form(elfihip_ctx* ctx, int form);
/* m separately stored summary columns of length n each (structure of arrays): the
 * form ELFI hands to distance_as_discrepancy BEFORE np.column_stack
 * (elfi/model/utils.py:39) -- lets the caller skip that host-side copy. */
int elfihip_dist_cols(elfihip_ctx* ctx, int metric, const double* const* cols, int m, int64_t n,
                      const double* y, const double* aux, double p, double* out);
/* Column-major device matrix: column j starts at dC + j*ldc, ldc >= n. */
int elfihip_dist_cols_dev(elfihip_ctx* ctx, int metric, const double* dC, int64_t n, int m,
                          int64_t ldc, const double* dy, const double* daux, double p,
                          double* dout);

/* AdaptiveDistance.nested_distance (elfi/model/elfi_model.py:1135-1151): K weighted
 * euclidean distances of the same rows in one pass.  W is (K, m) row-major holding the
 * cdist weights (i.e. (1/scale)^2, elfi_model.py:1132); the unweighted first function
 * (w=None, :1089) is passed as a row of ones, which is bit-identical.  out is (n, K)
 * row-major, as np.column_stack of the K cdist results. */
int elfihip_dist_multiw(elfihip_ctx* ctx, const double* X, int64_t n, int m, int64_t ldx,
                        const double* y, const double* W, int K, double* out);
int elfihip_dist_multiw_dev(elfihip_ctx* ctx, const double* dX, int64_t n, int m, int64_t ldx,
                            const double* dy, const double* dW, int K, double* dout);

/* AdaptiveDistance.add_data (elfi/model/elfi_model.py:1104-1125): one batched
 * Welford/Chan update of the running column statistics with the rows of X (n, m):
 *   N += n; d1 = x - mean; mean += sum(d1)/N; d2 = x - mean; M2 += sum(d1*d2).
 * Host form: count/mean/M2 are host scalars/vectors updated in place.
 * Device form: dstate is a device vector of 1 + 2m doubles [N, mean (m), M2 (m)]
 * updated in place on the context's stream (no host round trip). */
int elfihip_welford_update(elfihip_ctx* ctx, const double* X, int64_t n, int m, int64_t ldx,
                           int64_t* count, double* mean, double* M2);
int elfihip_welford_update_dev(elfihip_ctx* ctx, const double* dX, int64_t n, int m, int64_t ldx,
                               double* dstate);
/* Multi-GPU adaptive distance: merge the `world` rank states (each 1 + 2m doubles: count, mean, M2 -- what
 * elfihip_welford_update_dev maintains) that an all-gather left in device memory, in rank order, with Chan's pairwise
 * formula -- the merge the reference gets for free from seeing all batches in one process (elfi_model.py:1104-1125).
 * dmerged (1 + 2m) receives the global state, dw2 (m, may be NULL) the cdist weights 1 / scale^2 = N / M2
 * (elfi_model.py:1124,1129-1132).  Asynchronous on the context's stream. */
int elfihip_welford_merge_dev(elfihip_ctx* ctx, const double* dstates, int world, int m, double* dmerged, double* dw2);

/* ------------------------------------------------------------------ selection
 * The selection inside Rejection._merge_batch (elfi/methods/inference/samplers.py:209-237): the
 * reference argsorts n_samples + batch_size distances on the host per batch; keeping the k smallest
 * of the batch is equivalent and lets only k rows leave the GPU.  vals (k) / idx (k, row numbers)
 * come back ascending by (distance, row); NaN last; k is clipped to n.  `stride` (in doubles) lets
 * the _dev form read one column of an (n, K) nested-distance matrix in place; the _dev form leaves
 * the k survivors unsorted (row order inside "< k-th" then "== k-th"). */
/* Which implementation serves the selections of this context: 0 (default) the resident single-launch radix select
 * (slices of 16 384 keys held in registers for n <= 2 x 10^6 on MI355X, re-read from memory per phase above that),
 * falling back to the nine-launch form when its grid barrier times out; 1 the nine-launch form always; 2 the resident
 * form without the register variant (measurement and tests). */
int elfihip_topk_set_form(elfihip_ctx* ctx, int form);
int elfihip_topk_smallest(elfihip_ctx* ctx, const double* D, int64_t n, int64_t stride, int64_t k, double* vals,
                          int64_t* idx);
int elfihip_topk_smallest_dev(elfihip_ctx* ctx, const double* dD, int64_t n, int64_t stride, int64_t k,
                              double* dvals, int64_t* didx);

/* ------------------------------------------------------------------- sampler state: running best-k, fused with the distance
 * Replaces Rejection._merge_batch (elfi/methods/inference/samplers.py:209-237: copy the batch behind the n_samples best
 * rows, argsort n_samples + batch_size distances on the host, every batch).  An elfihip_reject keeps the k smallest
 * distances seen so far and their GLOBAL row numbers (row_base + row inside the batch; ties go to the earlier row) in
 * device memory, ascending.  A push computes a batch's distances (written to dout / out, as the Distance node must
 * return them) and folds the batch in during the same pass: once the state is full its k-th distance is a threshold and
 * the distance kernel itself lists the rows below it; a one-workgroup merge keeps the k best.
 * k <= 2048: the state lives on the device, pushes are asynchronous.  2048 < k <= 2^20 ("host-merge" states): the few
 * candidates of every push are merged into a sorted host copy, the k-th distance goes back as the device threshold
 * (a push synchronises).
 * _dev forms are asynchronous (distance pass on the context's stream); elfihip_reject_result synchronises and copies the state out
 * (vals, rows: k entries; *count = how many are real).  A state never fails for valid input: the candidate list holds
 * 8 x the largest batch pushed and is merged every 8th push at the latest; a push that would offer very many
 * candidates (a small first batch, a new SMC round without reset) takes the radix selection of its k best instead.
 * Nested distances (n, K) are ranked by their last column (samplers.py:233). */
typedef struct elfihip_reject elfihip_reject;
int elfihip_reject_create(elfihip_ctx* ctx, int64_t k, elfihip_reject** out);
int elfihip_reject_free(elfihip_reject* h);
int elfihip_reject_reset(elfihip_reject* h);
/* out may be NULL: the batch's distances are not copied back (only the k best rows ever leave the GPU) */
int elfihip_reject_push_rows(elfihip_reject* h, int metric, const double* X, int64_t n, int m, int64_t ldx,
                             const double* y, const double* aux, double p, double* out, int64_t row_base);
int elfihip_reject_push_rows_dev(elfihip_reject* h, int metric, const double* dX, int64_t n, int m, int64_t ldx,
                                 const double* dy, const double* daux, double p, double* dout, int64_t row_base);
int elfihip_reject_push_multiw_dev(elfihip_reject* h, const double* dX, int64_t n, int m, int64_t ldx, const double* dy,
                                   const double* dW, int K, double* dout, int64_t row_base);
/* distances that exist already (any Distance / Discrepancy node): dD[i * stride], i < n */
int elfihip_reject_push_dev(elfihip_reject* h, const double* dD, int64_t n, int64_t stride, int64_t row_base);
/* ... in host memory: D (n, ncols) row-major, ncols >= 1 nested columns, ranked by the last one -- what
 * Rejection._merge_batch receives as batch[discrepancy_name] (samplers.py:209-237).  Synchronises. */
int elfihip_reject_push(elfihip_reject* h, const double* D, int64_t n, int ncols, int64_t row_base);
/* The acceptance condition of a threshold objective (samplers.py:219-225: Rejection.sample(threshold=...)): a row takes
 * part only if EVERY one of its nested columns is <= threshold (pushes of (n, ncols) distances: elfihip_reject_push,
 * _push_multiw_dev; single-column pushes test their one column).  Set before the first push or after a reset;
 * enable = 0 removes it.  Accepted rows are counted on the device (elfihip_reject_meta). */
int elfihip_reject_set_accept(elfihip_reject* h, int enable, double threshold);
/* The same condition with ONE THRESHOLD PER NESTED COLUMN: what AdaptiveDistanceSMC hands its Rejection as `threshold`
 * -- the list [inf, threshold of population 1, ...] (samplers.py:657-660), compared column by column by
 * `batch[d] <= threshold` (samplers.py:222-223).  thresholds: ncols values, +inf allowed; every later push must carry
 * ncols nested columns. */
int elfihip_reject_set_accept_cols(elfihip_reject* h, int ncols, const double* thresholds);
/* What Rejection._update_state_meta / _update_objective_n_batches read after every batch (samplers.py:239-271): the
 * current k-th distance (+inf while fewer than k rows are in; it is the sampler's `threshold` state), rows accepted by
 * the pushes since the previous call and in total (acceptance threshold set).  in_use: entries of a host-merge state
 * (-1 for device states: elfihip_reject_result reports it).  Merges what is pending and synchronises; any output may be NULL. */
int elfihip_reject_meta(elfihip_reject* h, double* kth, int64_t* in_use, int64_t* accepted_last, int64_t* accepted_total);
/* Distances that are still on the device.  Every HOST-form call that returns distances (elfihip_dist_rows, _dist_cols,
 * _dist_multiw, _adaptive_push, _gauss_distance, _ma2_distance, _ma2_draw_distance) leaves a device copy of what it
 * returned in the context -- (n, ncols) row-major -- until the next such call; elfihip_kept_distances names it (epoch: a
 * counter of those calls).  elfihip_reject_push_kept folds that copy into the state as elfihip_reject_push would fold
 * the host array (acceptance, ranking by the last column), without the upload: what Rejection._merge_batch receives as
 * batch[discrepancy_name] (samplers.py:209-237) is the array the Distance node just returned.  Status ELFIHIP_ERR_STATE
 * when a later call has replaced the copy (the caller then pushes the host array). */
int elfihip_kept_distances(elfihip_ctx* ctx, uint64_t* epoch, int64_t* n, int* ncols);
int elfihip_reject_push_kept(elfihip_reject* h, uint64_t epoch, int64_t row_base);
/* device pointers to the state (k values ascending, k rows), e.g. as the send buffers of a gather */
int elfihip_reject_state_dev(elfihip_reject* h, double** dvals, int64_t** drows);
/* From the next merge on, every merge also leaves the state as one packed device buffer at ddst -- k doubles (values)
 * followed by k int64 (rows): the send buffer of a gather -- written by the merges themselves (no extra copy); NULL
 * stops it. */
int elfihip_reject_export_dev(elfihip_reject* h, void* ddst);
/* Candidates are merged into the state after every push at first and, once the threshold has settled, after every 8th
 * (a one-workgroup merge after every distance pass would cost a third of the pass); in between the list keeps growing against the last merged threshold, which still bounds the
 * current k-th distance from above, so nothing is missed.  States with k <= 1024 pushed through the row distances
 * (m = 16 / 32 / 64) SEAL the list at a merge point instead, and the next such push merges it in one workgroup of its own
 * distance launch; every other reader or push form merges a sealed list first.  The export buffer written is the one
 * current when the merge is launched.  elfihip_reject_flush merges what is pending now; _result, _state_dev do so
 * themselves.  On a device state (k <= 2048) _flush and _state_dev only queue that merge on the context's stream and
 * return: work queued behind _state_dev sees every batch merged at the pointers it returns.  On a host-merge state
 * both wait for the stream, as its pushes do. */
int elfihip_reject_flush(elfihip_reject* h);
/* vals / rows: k entries each; *count = entries in use.  A NaN distance never enters the state (the reference's argsort
 * would list such rows last, after every finite distance): while fewer than k finite distances have been seen, count is
 * their number. */
int elfihip_reject_result(elfihip_reject* h, double* vals, int64_t* rows, int64_t* count);

/* ------------------------------------------------------------------ one adaptive-distance batch in one read
 * Everything the reference does with a batch of an AdaptiveDistance round while its rows are read ONCE:
 *   - AdaptiveDistance.nested_distance (elfi/model/elfi_model.py:1135-1151): the K weighted euclidean distances under
 *     the weights of the EARLIER rounds (W (K, m): cdist weights, a row of ones for the unweighted first function) ->
 *     dout / out (n, K), bit-identical to elfihip_dist_multiw; dout / out may be NULL (nothing but the state's k rows
 *     leaves the GPU);
 *   - AdaptiveDistance.add_data (elfi_model.py:1104-1125), which Rejection._merge_batch calls for every batch
 *     (elfi/methods/inference/samplers.py:213-216): the batch folded into the running column statistics [N, mean (m),
 *     M2 (m)] that the NEXT update_distance turns into weights -- dwelford (device, 1 + 2m doubles, in place) or
 *     count / mean / M2 (host, in place); NULL: no statistics.  Tile-local two-pass sums merged with Chan's pairwise
 *     update in a fixed order: equal to the reference's batched Welford update up to rounding, bit-reproducible;
 *   - Rejection._merge_batch (samplers.py:218-237) against `state` (may be NULL): acceptance of every nested column
 *     (elfihip_reject_set_accept / _set_accept_cols), ranking by the last one, rows numbered row_base + row.  A first
 *     batch of >= 2^20 rows is selected against a provisional threshold taken from a prefix of the batch and verified
 *     (see csrc/reject.hip); the result is exact in every case.
 * Rows narrower than 129 doubles with even m / ldx and 16-byte aligned dX take the fused kernel (csrc/adaptive.hip);
 * other shapes run the separate passes (elfihip_welford_update_dev, elfihip_dist_multiw_dev, candidate pass).
 * _dev: asynchronous on the context's stream, except for the first-batch check, which reads four bytes back. */
int elfihip_adaptive_push_dev(elfihip_ctx* ctx, elfihip_reject* state, const double* dX, int64_t n, int m, int64_t ldx,
                              const double* dy, const double* dW, int K, double* dout, double* dwelford,
                              int64_t row_base);
int elfihip_adaptive_push(elfihip_ctx* ctx, elfihip_reject* state, const double* X, int64_t n, int m, int64_t ldx,
                          const double* y, const double* W, int K, double* out, int64_t* count, double* mean,
                          double* M2, int64_t row_base);

/* ... on rows that are still on the device: elfihip_randn_rows (below) leaves a device copy of the rows it returned --
 * elfihip_kept_rows names it -- and elfihip_adaptive_push_kept runs the pass on that copy (no upload of the batch);
 * ELFIHIP_ERR_STATE when a later elfihip_randn_rows call has replaced it. */
int elfihip_kept_rows(elfihip_ctx* ctx, uint64_t* epoch, int64_t* n, int* m);
int elfihip_adaptive_push_kept(elfihip_ctx* ctx, elfihip_reject* state, uint64_t rows_epoch, const double* y,
                               const double* W, int K, double* out, int64_t* count, double* mean, double* M2,
                               int64_t row_base);

/* ------------------------------------------------------------------ SMC proposal density
 * GMDistribution.pdf (elfi/methods/utils.py:142-183): density of a Gaussian mixture with shared
 * covariance at M points, out[r] = sum_i weights[i] * N(x_r; means[i], cov).  The caller passes the
 * covariance in the factored form SciPy's multivariate_normal uses: U (d x d, row-major) with
 * cov^+ = U U^T, and log_norm = rank*log(2 pi) + log pdet(cov); weights already normalised.  d <= 64 (above 16 both point sets are
 * transformed by U once and a pair costs d subtractions). */
int elfihip_gm_pdf(elfihip_ctx* ctx, const double* x, int64_t M, int d, const double* means, int64_t N,
                   const double* weights, const double* U, double log_norm, double* out);
/* n draws from the same mixture -- GMDistribution.rvs (elfi/methods/utils.py:199-262), the proposal of an SMC batch
 * (samplers.py:434-459): draw i picks the component at the inverse of the cumulative weights `cumw` (N values, last 1) at
 * the uniform of Philox counter i of stream (seed, stream) and adds A z_i, A (d, d) row-major with A A^T = cov, z_i the d
 * standard normals of counters i ceil(d / 2) ... of stream (seed, stream + 1) (the generator of elfihip_randn_dev).  The
 * validity check against the prior (prior_logpdf) stays with the caller.  Host pointers; out (n, d). */
int elfihip_gm_rvs(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, int d, const double* means, int64_t N,
                   const double* cumw, const double* A, double* out);

/* ------------------------------------------------------------------ SMC population statistics
 * weighted_var (elfi/methods/utils.py:108-139; caller samplers.py:521-534): unbiased weighted variance of every
 * column of the accepted sample, s2[c] = sum_i w_i (x_ic - xbar_c)^2 / (V1 - V2 / V1), xbar_c = sum_i w_i x_ic / V1,
 * V1 = sum w, V2 = sum w^2.  X (n, m) row-major with pitch ldx; w (n) or NULL for unit weights (the reference's
 * default); s2 (m).  Deterministic (fixed summation order). */
int elfihip_weighted_var(elfihip_ctx* ctx, const double* X, int64_t n, int m, int64_t ldx, const double* w, double* s2);
int elfihip_weighted_var_dev(elfihip_ctx* ctx, const double* dX, int64_t n, int m, int64_t ldx, const double* dw,
                             double* ds2);

/* ------------------------------------------------------------------ Bayesian synthetic likelihood
 * The Gaussian synthetic log-likelihood of G groups of n simulated summary rows in one launch
 * (elfi/methods/bsl/pdf_methods.py:77-176, 267-316; the loops of pre_sample_methods.py:102-143, 215-318).
 * X (G n, m) row-major with pitch ldx, group g = rows g n ... g n + n - 1; m <= 64; n >= 2.  y (m) observed summaries.
 * W (m, m) row-major or NULL: whitening, rows -> rows W^T and y -> W y before the moments (pdf_methods.py:105-108).
 * variant: 0 standard, 1 unbiased (Ghurye-Olkin), 2 mean-adjusted, 3 variance-adjusted (2, 3: gamma_adj (m), else NULL).
 * prefixes: K row counts, ascending, >= 2, the last == n; NULL (K 0 or 1) = {n}.  Prefix k takes the moments of the
 * first prefixes[k] rows of every group, with the bits a group of that many rows has.
 * penalties: P Warton penalties in [0, 1] (cov_warton(S, 1 - penalty), cov_warton.py:6-30); NULL (P 0) = no shrinkage.
 * Variant 0 only: the reference defines no shrinkage for the others, ELFIHIP_ERR_ARG.
 * loglik (G, K, max(P, 1)): -inf where the matrix has a non-positive Cholesky pivot (variant 1: also psi) or a value is
 * not finite -- the status stays ELFIHIP_OK.  mean (G, m), cov (G, m, m) or NULL: sample mean and np.cov(rowvar=False)
 * of the full group after whitening, before shrinkage and adjustment.
 * Host form: host pointers, synchronises.  _dev form: X, y, W, gamma_adj, loglik, mean, cov are device pointers, no
 * synchronisation; prefixes and penalties are host arrays in both forms (they are checked before the launch).
 * Deterministic; a group's result does not depend on G. */
int elfihip_syn_loglik(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* y,
                       const double* W, int variant, const double* gamma_adj, const int64_t* prefixes, int K,
                       const double* penalties, int P, double* loglik, double* mean, double* cov);
int elfihip_syn_loglik_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                           const double* dW, int variant, const double* dgamma_adj, const int64_t* prefixes, int K,
                           const double* penalties, int P, double* dloglik, double* dmean, double* dcov);

/* The semiparametric synthetic log-likelihood (semiBSL: a kernel density estimate per summary and a Gaussian copula with
 * the Gaussian rank correlation; elfi/methods/bsl/pdf_methods.py:179-264, gaussian_rank_corr.py:30-52) of G groups of n
 * rows in one call.  X, y, ldx, prefixes, penalties and loglik (G, K, max(P, 1)) as for elfihip_syn_loglik; m <= 64,
 * 2 <= n <= 16384 (one column of a group is held in LDS).  Per column j of the first p rows: bandwidth
 * h = (3 p / 4)^(-1/5) std (ddof 1), z_i = (y_j - x_ij) / h, logpdf_j = logsumexp_i(-z_i^2 / 2) - log p - log h -
 * log(2 pi) / 2, u_j = min(1, sum_i Phi(z_i) / p), eta_j = Phi^-1(u_j); scores q_ij = Phi^-1(r_ij / (p + 1)) with r the
 * 1-based rank within the column, ties at the average rank; rho_ab = sum_i q_ia q_ib / sum_i Phi^-1(i / (p + 1))^2,
 * rho_aa = 1; penalty l: rho <- (1 - l) rho + l I (corr_warton: no eps);
 * loglik = -(log|rho| + eta^T rho^-1 eta - eta^T eta) / 2 + sum_j logpdf_j.
 * -inf with the status left at ELFIHIP_OK: a u_j of 0 or 1, a non-positive Cholesky pivot, a non-finite value; a column
 * without spread (h = 0 -- the reference raises LinAlgError from scipy's gaussian_kde there); two rows and m > 1 (rho has
 * rank one; the reference returns about -1e16 from rounding noise).
 * u (G, m), rho (G, m, m), scores (G, n, m) or NULL: of the full groups, the integrals u_j, the rank correlation before
 * shrinkage and the normal scores q.
 * Host form: host pointers, synchronises.  _dev form: X, y, loglik, u, rho, scores are device pointers, no
 * synchronisation; prefixes and penalties are host arrays in both forms (they are checked before any launch).
 * Deterministic; a group's result does not depend on G, and prefix p has the bits of a group of p rows. */
int elfihip_semi_loglik(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* y,
                        const int64_t* prefixes, int K, const double* penalties, int P, double* loglik, double* u,
                        double* rho, double* scores);
int elfihip_semi_loglik_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dy,
                            const int64_t* prefixes, int K, const double* penalties, int P, double* dloglik, double* du,
                            double* drho, double* dscores);

/* KLIEP density-ratio estimation (elfi/methods/density_ratio_estimation.py: fit, _KLIEP :183-202, _KLIEP_lcv :157-181) of
 * numerator rows x (Nx, d), pitch ldx, against denominator rows y (Ny, d), pitch ldy, for S basis scales in one call; with
 * F > 0 folds also the S x F leave-fold-out fits of the likelihood cross-validation.
 * Centres theta = x[:n]; A[i, j] = exp(-0.5 |x_i - theta_j|^2 / sigma / sigma); b_j = sum_t basis(theta_j, y_t) wy_norm[t],
 * b_normalized = b / (b . b).  Row i is non-null when some A[i, j] > 1e-64; the filtered index of a non-null row is the
 * number of non-null rows in front of it, L their count; fold f holds the filtered indices
 * np.array_split(arange(L), F)[f].  Per problem (scale, held-out fold or none): alpha = 1 / n, prev = A alpha over all Nx
 * rows; step i = 0 .. max_iter - 1: alpha += epsilon A_tr^T (w_tr / (A_tr alpha)) over the training rows (non-null, not
 * held out), alpha = max(0, alpha + (1 - b . alpha) b_normalized), alpha /= b . alpha; when i % conv_check_interval == 0:
 * t = A alpha over all rows, stop if |t - prev|_2 < abs_tol, else prev = t.  NaN and inf propagate as in NumPy.
 * wx (Nx): the weights of the full fits, as the caller has them (the reference passes them unnormalised); wx_norm (Nx):
 * the normalised weights of the fold fits and the scores (read with F > 0 only, may be NULL otherwise); wy_norm (Ny).
 * sigmas: S scales, a host array in both forms.
 * Outputs, each may be NULL: alpha (S, n), w (S, Nx) = A alpha of the full fit, iters (S) the index i at which its loop
 * ended; with F > 0 scores (S, F), the weighted mean (wx_norm) of log w of the fold's fit over the held-out rows, and
 * lcv (S), their mean over the folds -- +inf when L = 0, as the reference returns; a held-out ratio of 0 gives -inf.
 * Limits (ELFIHIP_ERR_ARG before any launch): 1 <= d <= 64, 1 <= n <= 256, n <= Nx, Nx and Ny <= 65536, 1 <= S <= 16,
 * 0 <= F <= 16, max_iter >= 1, conv_check_interval >= 1, every sigma positive and finite.
 * Host form: host pointers, synchronises.  _dev form: x, y, the weights and the outputs are device pointers, no
 * synchronisation.  Deterministic; a problem's result does not depend on S, on F or on the other problems. */
int elfihip_kliep_fit(elfihip_ctx* ctx, const double* x, int64_t Nx, int d, int64_t ldx, const double* y, int64_t Ny,
                      int64_t ldy, const double* wx, const double* wx_norm, const double* wy_norm, const double* sigmas,
                      int S, int n, double epsilon, int max_iter, double abs_tol, int conv_check_interval, int F,
                      double* alpha, double* w, int64_t* iters, double* scores, double* lcv);
int elfihip_kliep_fit_dev(elfihip_ctx* ctx, const double* dx, int64_t Nx, int d, int64_t ldx, const double* dy, int64_t Ny,
                          int64_t ldy, const double* dwx, const double* dwx_norm, const double* dwy_norm,
                          const double* sigmas, int S, int n, double epsilon, int max_iter, double abs_tol,
                          int conv_check_interval, int F, double* dalpha, double* dw, int64_t* diters, double* dscores,
                          double* dlcv);

/* The fitted ratio at M points (M, d), pitch ldp: out[i] = sum_j exp(-0.5 |p_i - c_j|^2 / sigma / sigma) alpha[j] for the
 * n centres (n, d), pitch ldc (_weighted_basis_sum, :140-143) -- summed in the order of the fit, so the ratio at the
 * fit's own rows has the bits of its w.  1 <= d <= 64, 1 <= n <= 256, sigma positive and finite; M = 0 does nothing. */
int elfihip_kliep_ratio(elfihip_ctx* ctx, const double* points, int64_t M, int d, int64_t ldp, const double* centres, int n,
                        int64_t ldc, const double* alpha, double sigma, double* out);
int elfihip_kliep_ratio_dev(elfihip_ctx* ctx, const double* dpoints, int64_t M, int d, int64_t ldp, const double* dcentres,
                            int n, int64_t ldc, const double* dalpha, double sigma, double* dout);

/* Logistic-regression ratio estimation (the classifier of BOLFIRE; elfi/methods/classifier.py:72-121: StandardScaler,
 * then scikit-learn's LogisticRegression(penalty='l1', solver='liblinear'), then the log-odds) of G groups in one call.
 * X (G n, m) row-major with pitch ldx: the likelihood rows, label +1, group g = rows g n ... g n + n - 1.  M (nm, m) with
 * pitch ldm: the marginal rows, label -1, shared by every group.  Yobs (k, m) contiguous: where the log ratio is read.
 * 1 <= m <= 64, n >= 1, nm >= 1, k >= 1; C > 0 (liblinear's default 1), 0 <= class_min < 1, tol >= 0, max_iter >= 0.
 * Per group, N = n + nm: mean and population standard deviation (ddof 0) of the N stacked rows per column, scale 1 for a
 * column StandardScaler treats as constant (var <= N eps var + (N mean eps)^2); x~ = (x - mean) / scale.  The fit
 * minimises liblinear's L1R_LR objective with fit_intercept=True, intercept_scaling=1,
 *     ||v||_1 + C sum_i log(1 + exp(-y_i v.z_i)),  z_i = (x~_i, 1),  v = (w, b)
 * (the intercept is a penalised coordinate) by proximal Newton steps: coordinate descent with soft-thresholding on the
 * quadratic model, then a backtracking line search on the objective; a coordinate ends exactly zero or not.  With
 * g = C Z^T (-y o sigma(-y o Z v)) the optimality violation is the largest of |g_j + sign(v_j)| (v_j != 0) and
 * max(|g_j| - 1, 0) (v_j == 0); the iteration stops when it is <= tol or after max_iter outer steps.
 * logratio (G, k): t = w.x~_obs + b where expit(t) >= class_min, else log(class_min / (1 - class_min)).  That is the
 * reference's log(p / (1 - p)), p = max(expit(t), class_min), without the rounding of 1 - p, and finite where the
 * reference returns +-inf from an expit that under- or overflows.
 * Each may be NULL: coef (G, m), intercept (G), mean (G, m), scale (G, m), n_iter (G) outer steps taken, status (G):
 * 0 converged, 1 stopped at max_iter, 2 a non-finite value (in the group's rows, in M, or on the way), 4 no step lowers the
 * objective any more (its rounding level is reached before tol).  A group with status 2 has NaN outputs.  None of these
 * is an error return: the call gives ELFIHIP_OK.
 * Host form: host pointers, synchronises.  _dev form: X, M, Yobs and every output are device pointers, no
 * synchronisation; the scalars are host values in both forms.
 * Deterministic; a group's result does not depend on G or on the other groups of the call. */
int elfihip_log_ratio(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* M,
                      int64_t nm, int64_t ldm, const double* Yobs, int64_t k, double C, double class_min, double tol,
                      int max_iter, double* logratio, double* coef, double* intercept, double* mean, double* scale,
                      int* n_iter, int* status);
int elfihip_log_ratio_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx, const double* dM,
                          int64_t nm, int64_t ldm, const double* dYobs, int64_t k, double C, double class_min, double tol,
                          int max_iter, double* dlogratio, double* dcoef, double* dintercept, double* dmean,
                          double* dscale, int* dn_iter, int* dstatus);

/* ------------------------------------------------------------------ summary-statistic selection
 * The data-parallel steps of TwoStageSelection (Nunes & Balding 2010; elfi/methods/diagnostics.py:15-289), each for all
 * candidate combinations in one call (csrc/twostage.hip).  Deterministic: fixed-order sums, no atomics; a group's result
 * does not depend on G.  Every argument is checked before anything is launched; on ELFIHIP_ERR_ARG no output is touched.
 *
 * elfihip_knn_entropy (diagnostics.py:214-253): T holds G groups of n points in q dimensions, row-major with pitch ldt,
 * group g = rows g n ... g n + n - 1.  entropy (G):
 *   E = log(pi^(q/2) / Gamma(q/2 + 1)) - psi(k) + log n + (q / n) sum_i log R_ik,
 * R_ik = the euclidean distance from point i to its k-th nearest neighbour where the point itself is the first, at
 * distance 0 (cKDTree.query(theta_i, k)[0][-1]): k = 4 is the third other point; k = 1, or k coincident points, give -inf;
 * k > n gives +inf (the tree pads with inf).  kth (G, n) or NULL: the R_ik.  A squared distance is summed left to right over
 * the dimensions.  1 <= q <= 32, 1 <= k <= 16, n >= 1 (at most 65535 * 256 points per group).
 *
 * elfihip_mrsse (:255-289): mrsse (G) = (1 / J) sum_j sqrt(sum_{i,d} (T[g][i][d] - closest[j][d])^2) with closest (J, q) at
 * pitch ldc, J <= 65535, the mean over j taken in index order.
 *
 * elfihip_subset_best: what one elfi.Rejection per combination selects (:172-212) from ONE pool of simulations.  X (n, m)
 * with pitch ldx are the summaries, y (m) the observed ones, masks (C, m) hold 0.0 / 1.0 (any other entry and an all-zero
 * mask are argument errors).  vals (C, min(k, n)) and rows (C, min(k, n)): the k smallest euclidean distances of every
 * combination over its selected columns, with their row numbers, ascending by (distance, row), NaN last.  The distances
 * are elfihip_dist_multiw's with the masks as weights, bit for bit, so a non-finite value in an UNSELECTED column makes
 * the row's distance 0 * inf = NaN and ranks it last.  Composed on the device from elfihip_dist_multiw_dev (blocks of at
 * most 64 combinations and 1 GiB), elfihip_topk_smallest_dev per column and a sort of the survivors; no (n, C) matrix
 * reaches the host.
 *
 * Host forms: host pointers, synchronise.  _dev forms: device pointers and the context's stream; masks is a HOST array in
 * both forms (it is checked before the launch).  elfihip_knn_entropy_dev and elfihip_mrsse_dev do not synchronise;
 * elfihip_subset_best_dev synchronises once per block of combinations (it reads the selection's time-out flags). */
int elfihip_knn_entropy(elfihip_ctx* ctx, const double* T, int64_t G, int64_t n, int q, int64_t ldt, int k,
                        double* entropy, double* kth);
int elfihip_knn_entropy_dev(elfihip_ctx* ctx, const double* dT, int64_t G, int64_t n, int q, int64_t ldt, int k,
                            double* dentropy, double* dkth);
int elfihip_mrsse(elfihip_ctx* ctx, const double* T, int64_t G, int64_t n, int q, int64_t ldt, const double* closest,
                  int64_t J, int64_t ldc, double* mrsse);
int elfihip_mrsse_dev(elfihip_ctx* ctx, const double* dT, int64_t G, int64_t n, int q, int64_t ldt,
                      const double* dclosest, int64_t J, int64_t ldc, double* dmrsse);
int elfihip_subset_best(elfihip_ctx* ctx, const double* X, int64_t n, int m, int64_t ldx, const double* y,
                        const double* masks, int64_t C, int64_t k, double* vals, int64_t* rows);
int elfihip_subset_best_dev(elfihip_ctx* ctx, const double* dX, int64_t n, int m, int64_t ldx, const double* dy,
                            const double* masks, int64_t C, int64_t k, double* dvals, int64_t* drows);

/* ------------------------------------------------------------------ regression adjustment
 * elfi.LinearAdjustment / elfi.adjust_posterior (elfi/methods/post_processing.py:195-253) for G groups of n accepted rows
 * and K nested prefixes of every group in one call (csrc/adjust.hip).  X (G n, m) row-major with pitch ldx: the summaries
 * minus the observed summaries; Y (G n, q) with pitch ldy: the parameters, one column each; group g = rows g n ...
 * g n + n - 1 of both.  1 <= m <= 64, 1 <= q <= 16, n >= 2.  prefixes (K) as for elfihip_syn_loglik: ascending, >= 2, the
 * last == n; NULL = {n} (Ke = 1, else Ke = K).  A job is one (g, k): the first p_k rows of group g.  Per job and response:
 *     b = argmin || (y - ybar) - (X - xbar) b ||_2,   intercept = ybar - xbar.b,   rss = the minimum (a sum of squares),
 *     adjusted_i = y_i - x_i.b   with the UNCENTRED x_i, summed left to right (what LinearAdjustment._adjust computes)
 * by a Householder QR of the centred [X | Y] in float64: tiles of 256 rows (128 when m + q > 40), the tile factors folded
 * pairwise in a fixed binary tree; no Gram matrix is formed, so the result does not depend on the columns' scales (the
 * reference's SVD does).  rss is the squared norm of the response's column of R22.
 * adjusted (G, Ke, n, q), required: rows at or beyond p_k are NaN.  Each may be NULL: coef (G, Ke, q, m), intercept
 * (G, Ke, q), rss (G, Ke, q), status (G, Ke), per job:
 *   0 ok;
 *   2 a non-finite value in the job's rows;
 *   3 rank-deficient: p_k - 1 < m, a constant column (minimum == maximum), or a column j with
 *     |R_jj| <= max(p_k, m) eps ||centred column j||_2 (scale-invariant).  The reference returns the minimum-norm
 *     solution there; the device does not.
 * A job with status 2 or 3 has NaN outputs.  None of these is an error return: the call gives ELFIHIP_OK.
 * Every argument is checked before anything is launched; on ELFIHIP_ERR_ARG no output is touched.
 * Host form: host pointers, synchronises.  _dev form: X, Y and every output are device pointers on the context's stream,
 * no synchronisation; prefixes is a host array in both forms.
 * Deterministic: fixed-order sums, no atomics; a job's result does not depend on G or on the other jobs, and prefix p has
 * the bits of a group of p rows. */
int elfihip_linear_adjust(elfihip_ctx* ctx, const double* X, int64_t G, int64_t n, int m, int64_t ldx, const double* Y,
                          int q, int64_t ldy, const int64_t* prefixes, int K, double* adjusted, double* coef,
                          double* intercept, double* rss, int* status);
int elfihip_linear_adjust_dev(elfihip_ctx* ctx, const double* dX, int64_t G, int64_t n, int m, int64_t ldx,
                              const double* dY, int q, int64_t ldy, const int64_t* prefixes, int K, double* dadjusted,
                              double* dcoef, double* dintercept, double* drss, int* dstatus);

/* ------------------------------------------------------------------ summaries
 * Row-wise summary statistics that ELFI's example models install as elfi.Summary operations, with
 * NumPy's exact (pairwise) summation order, i.e. bit-identical results:
 *   ELFIHIP_SUM_MEAN     np.mean(y, axis=1)                           elfi/examples/gauss.py:142-156
 *   ELFIHIP_SUM_VAR      np.var(y, axis=1)                            elfi/examples/gauss.py:159-173
 *   ELFIHIP_SUM_AUTOCOV  np.mean(x[:, lag:] * x[:, :-lag], axis=1)    elfi/examples/ma2.py:40-59
 * X is row-major (n, L) with leading dimension ldx; out has n doubles; lag only for AUTOCOV.  A row takes one LDS tile:
 * L <= 20479 ((L | 1) * 8 bytes <= 160 KiB), ELFIHIP_ERR_ARG beyond.  Rows longer than NumPy's reduction buffer (8192
 * elements) are summed as NumPy sums them: pairwise inside pieces of 8192, the pieces added in order. */
enum { ELFIHIP_SUM_MEAN = 0, ELFIHIP_SUM_VAR = 1, ELFIHIP_SUM_AUTOCOV = 2 };
int elfihip_row_summary(elfihip_ctx* ctx, int kind, const double* X, int64_t n, int L, int64_t ldx, int lag,
                        double* out);
int elfihip_row_summary_dev(elfihip_ctx* ctx, int kind, const double* dX, int64_t n, int L, int64_t ldx, int lag,
                            double* dout);
/* The whole MA2 example path after the random draw, fused (elfi/examples/ma2.py:11-59,62-92 +
 * elfi.Distance('euclidean', S1, S2)): from the white noise W (n, n_obs + 2) -- drawn by the caller
 * from the reference's MT19937 stream, random_state.randn(batch_size, n_obs + 2) -- and per-row
 * parameters t1, t2 (n): x = w[:, 2:] + t1 w[:, 1:-1] + t2 w[:, :-2], S1 = autocov(x, 1),
 * S2 = autocov(x, 2), D = sqrt((S1 - obs1)^2 + (S2 - obs2)^2), bit-identical to the reference's
 * NumPy/SciPy results, in one pass over W. */
int elfihip_ma2_distance(elfihip_ctx* ctx, const double* W, int64_t n, int n_obs, const double* t1, const double* t2,
                         double obs1, double obs2, double* S1, double* S2, double* D);
/* ... with the white noise drawn inside the kernel (Philox4x32-10, key `seed`, counter stream `stream`: the draws of
 * elfihip_randn_dev), host parameters in, host results out: the whole example as ONE node operation. */
int elfihip_ma2_draw_distance(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, int n_obs, const double* t1,
                              const double* t2, double obs1, double obs2, double* S1, double* S2, double* D);
int elfihip_ma2_distance_dev(elfihip_ctx* ctx, const double* dW, int64_t n, int n_obs, int64_t ldw, const double* dt1,
                             const double* dt2, double obs1, double obs2, double* dS1, double* dS2, double* dD);
/* The same with the white noise DRAWN IN THE KERNEL (synthetic-throughput runs; the reference draws it from MT19937 on the
 * host, examples/ma2.py:31-33: bit parity with a reference run needs that stream, so parity runs hand W in): element e
 * of the row-major (n, n_obs + 2) noise matrix is normal number e of the stream (seed, stream) of elfihip_randn_dev, so
 * the results equal elfihip_randn_dev + elfihip_ma2_distance_dev bit for bit while the noise never exists in memory.
 * n_obs <= 126. */
int elfihip_ma2_draw_distance_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, int n_obs, const double* dt1,
                                  const double* dt2, double obs1, double obs2, double* dS1, double* dS2, double* dD);

/* The Gaussian example model, fused (elfi/examples/gauss.py:11-35 gauss, :142-173 ss_mean / ss_var, :133
 * elfi.Distance('euclidean', ss_mean, ss_var)): y = z * sigma + mu for n simulations of n_obs observations (what
 * ss.norm.rvs(loc, scale) computes from standard normals z), S1 = np.mean(y, axis=1), S2 = np.var(y, axis=1),
 * D = sqrt((S1 - obs_mean)^2 + (S2 - obs_var)^2) -- bit-identical to NumPy / SciPy on the same z -- in one pass.
 * Z (n, n_obs) holds the standard normals (drawn by the caller from the reference's MT19937 stream when results must
 * match the reference); Z == NULL draws them on the device: Philox4x32-10, counter = (pair index, stream), key = seed,
 * Box-Muller, element e of the row-major (n, n_obs) matrix from pair e / 2 -- a pure function of (seed, stream, e).
 * Y (optional, (n, n_obs)) receives the simulator output.  mu, sigma: n values each. */
int elfihip_gauss_distance(elfihip_ctx* ctx, const double* Z, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                           const double* mu, const double* sigma, double obs_mean, double obs_var, double* Y, double* S1,
                           double* S2, double* D);
int elfihip_gauss_distance_dev(elfihip_ctx* ctx, const double* dZ, int64_t ldz, uint64_t seed, uint64_t stream, int64_t n,
                               int n_obs, const double* dmu, const double* dsigma, double obs_mean, double obs_var,
                               double* dY, double* dS1, double* dS2, double* dD);
/* Device-resident synthetic inputs from the same generator: dout[e] = z_e * scale + loc, e < n (the simulator
 * outputs of BASELINE configs[1] / configs[3]); the raw Philox4x32-10 blocks (4 x uint32 per block, counter =
 * (block, stream), key = seed) for known-answer tests. */
int elfihip_randn_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, double loc, double scale, double* dout);
/* The synthetic Gaussian simulator of BASELINE configs[1] / [3] as ONE host-form node operation: out (n, m) row-major,
 * out[i][j] = loc[i] + scale[j] z, z = the draws of elfihip_randn_dev(seed, stream) in row-major order (m even).  The rows
 * also stay on the device for the distance call that follows (elfihip_kept_rows, elfihip_adaptive_push_kept). */
int elfihip_randn_rows(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, int m, const double* loc,
                       const double* scale, double* out);
int elfihip_random_bits_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t nblocks, uint32_t* dout);
/* Prior draws on the device.  Replaces the draws behind elfi.Prior nodes -- rvs_from_distribution
 * (elfi/model/utils.py:6-35) -> scipy.stats rvs on the host, 64 % of the reference loop's time per batch of 10^6 once
 * simulator and distance run on the GPU.  U_e = the 53-bit uniform in [0, 1) made of the first
 * (e even) / second (e odd) pair of words of Philox counter e / 2 of stream (seed, stream) -- the generator of
 * elfihip_randn_dev -- transformed in the reference's own operation order:
 *   ELFIHIP_PRIOR_UNIFORM: out = U * a[1] + a[0]                  ss.uniform.rvs(loc = a[0], scale = a[1])
 *   ELFIHIP_PRIOR_MA2_T1:  CustomPrior1.rvs(b = a[0])             elfi/examples/ma2.py:102-118
 *   ELFIHIP_PRIOR_MA2_T2:  CustomPrior2.rvs(t1 = cond, a = a[0])  elfi/examples/ma2.py:147-166 (cond: n values)
 * a: host scalars.  Host form: cond / out host pointers; _dev form: device pointers, no synchronisation. */
#define ELFIHIP_PRIOR_UNIFORM 0
#define ELFIHIP_PRIOR_MA2_T1 1
#define ELFIHIP_PRIOR_MA2_T2 2
int elfihip_prior_draw(elfihip_ctx* ctx, int kind, uint64_t seed, uint64_t stream, int64_t n, const double* a,
                       const double* cond, double* out);
int elfihip_prior_draw_dev(elfihip_ctx* ctx, int kind, uint64_t seed, uint64_t stream, int64_t n, const double* a,
                           const double* dcond, double* dout);

/* The time-series example models, fused: draws, the serial recurrence of every simulation, summaries and distance in one
 * pass; series, summaries and quantiles bit-identical to the reference's NumPy on the same draws.  Series of at most
 * ELFIHIP_SERIES_MAX_OBS observations (a simulation keeps its series in LDS).  Draw matrices given as NULL are drawn
 * in the kernel from the stream (seed, stream) of elfihip_randn_dev.  Optional outputs may be NULL.  obs, w and the
 * quantile positions are HOST arrays in both forms; in the _dev forms every other pointer is a device pointer and every
 * matrix comes with the caller's leading dimension (in doubles); no synchronisation.  The host forms synchronise.
 *
 * ARCH(1) (elfi/examples/arch.py): W (n, n_obs + 2) standard normals -- columns 0 .. n_obs the reference's xi =
 * normal((batch, n_obs + 1)), column n_obs + 1 its e[:, 0] = normal(batch); W == NULL: element e of the row-major matrix
 * is normal number e of (seed, stream).  e_i = xi_i sqrt(0.2 + t2 e_{i-1}^2), y_0 = 0, y_i = t1 y_{i-1} + e_i, i = 1 ..
 * n_obs.  S (n, m), m = 2 + L + L (L - 1) / 2 for L = n_lags in 1 .. ELFIHIP_ARCH_MAX_LAGS, n_obs >= L + 2: sample_mean,
 * sample_variance, autocorr(lag 1 .. L), pairwise_autocorr(i, j) for i < j in itertools.combinations order.  Y (n, n_obs):
 * the series.  D (n): euclidean distance of the row of S to obs (m values), bit-identical to elfihip_dist_rows on S. */
#define ELFIHIP_SERIES_MAX_OBS 2048
#define ELFIHIP_ARCH_MAX_LAGS 8
int elfihip_arch_summaries(elfihip_ctx* ctx, const double* W, uint64_t seed, uint64_t stream, int64_t n, int n_obs, int n_lags,
                           const double* t1, const double* t2, const double* obs, double* S, double* Y, double* D);
int elfihip_arch_summaries_dev(elfihip_ctx* ctx, const double* dW, int64_t ldw, uint64_t seed, uint64_t stream, int64_t n,
                               int n_obs, int n_lags, const double* dt1, const double* dt2, const double* obs, double* dS,
                               int64_t lds, double* dY, int64_t ldy, double* dD);
/* AR(1) (elfi/examples/ar1.py): W (n, n_obs + 1) standard normals, the reference's randn(batch, n_obs + 1) -- column 0 is
 * drawn and unused, as there; W == NULL: element e of the row-major matrix is normal number e of (seed, stream).  x_0 = 0,
 * x_i = phi x_{i-1} + w_i for i = 1 .. n_obs: the product is rounded, then the sum (contraction off).  NaN and infinite phi
 * propagate as NumPy's do (inf * 0 = NaN at i = 1).  X (n, n_obs): the series x_1 .. x_n_obs.  D (n): euclidean distance of
 * the row of X to obs (n_obs host values), bit-identical to elfihip_dist_rows 'euclidean' on X.  X and D may each be NULL.
 * 1 <= n_obs <= ELFIHIP_SERIES_MAX_OBS, n >= 0; anything else is ELFIHIP_ERR_ARG, and so is a distance without obs. */
int elfihip_ar1_series(elfihip_ctx* ctx, const double* W, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                       const double* phi, const double* obs, double* X, double* D);
int elfihip_ar1_series_dev(elfihip_ctx* ctx, const double* dW, int64_t ldw, uint64_t seed, uint64_t stream, int64_t n,
                           int n_obs, const double* dphi, const double* obs, double* dX, int64_t ldx, double* dD);
/* M/G/1 (elfi/examples/mg1.py): E (n, n_obs) standard exponentials and V (n, n_obs) uniforms in [0, 1) -- the reference's
 * standard_exponential((n_obs, batch)) and random_sample((n_obs, batch)), transposed; both NULL: E_e = -log u with u the
 * 53-bit uniform in (0, 1] made of word e of (seed, stream) (the word + 1, as the normals' radius takes it), V_e = word e of
 * (seed, stream + 1) as elfihip_prior_draw forms its uniforms.  W = (1 / t3) E, U = t1 + (t2 - t1) V, sum_w += W_i,
 * y_i = U_i + max(0, sum_w - sum_x), sum_x += y_i.  logY (n, n_obs) = log y (the device logarithm: within a few ulp of
 * np.log).  Q (n, nq), 1 <= nq <= ELFIHIP_MG1_MAX_QUANTILES: np.quantile(y, q, axis=1, method='linear') from the positions
 * the host computed by NumPy's virtual-index rule -- for quantile k the sorted neighbours a = s[lo[k]], b = s[hi[k]] and the
 * weight t[k]: a + (b - a) t[k] if t[k] < 0.5, else b - (b - a) (1 - t[k]).  Y: the series; Eo, Vo: the draws used.
 * D (n): euclidean distance of the row of Q to obs (nq values), weighted by w (nq values) when w is given; bit-identical
 * to elfihip_dist_rows on Q. */
#define ELFIHIP_MG1_MAX_QUANTILES 64
int elfihip_mg1_summaries(elfihip_ctx* ctx, const double* E, const double* V, uint64_t seed, uint64_t stream, int64_t n,
                          int n_obs, const double* t1, const double* t2, const double* t3, int nq, const int* lo, const int* hi,
                          const double* t, const double* obs, const double* w, double* logY, double* Q, double* Y, double* Eo,
                          double* Vo, double* D);
int elfihip_mg1_summaries_dev(elfihip_ctx* ctx, const double* dE, int64_t lde, const double* dV, int64_t ldv, uint64_t seed,
                              uint64_t stream, int64_t n, int n_obs, const double* dt1, const double* dt2, const double* dt3,
                              int nq, const int* lo, const int* hi, const double* t, const double* obs, const double* w,
                              double* dLogY, int64_t ldl, double* dQ, int64_t ldq, double* dY, int64_t ldy, double* dEo,
                              int64_t ldeo, double* dVo, int64_t ldvo, double* dD);

/* Counter-based Poisson variates: out[e] = poisson_draw(lam[e], seed, stream, e), e < n, a deterministic function of lam[e]
 * and the generator's words, so element e does not depend on n or on where it is drawn (csrc/poisson.hpp; the NumPy
 * statement is tests/ricker_ref.py: poisson_ref).  Attempt j = 0, 1, .. of element e reads Philox counter e of stream
 * (seed, stream + j): u1 = ((r0 << 21) | (r1 >> 11)) 2^-53, u2 the same of words 2, 3, both in [0, 1).  The result is a double:
 *   lam NaN, lam < 0 or lam > 2^53: NaN.  (RandomState.poisson raises ValueError for the whole batch; here the element
 *     is marked and the batch goes on.)
 *   lam == 0: 0, no draw.
 *   0 < lam < 10: inversion on u1 of attempt 0 -- p = F = exp(-lam), k = 0; while u1 > F and k < ELFIHIP_POISSON_MAX_K:
 *     k += 1, p = p (lam / k), F = F + p; the result is k.
 *   lam >= 10: Hoermann's PTRS, the algorithm of NumPy's legacy poisson.  slam = sqrt(lam), loglam = log(lam), b = 0.931 +
 *     2.53 slam, a = -0.059 + 0.02483 b, invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2).  Per
 *     attempt: U = u1 - 0.5, V = u2, us = 0.5 - |U|, k = floor((2 a / us + b) U + lam + 0.43); accept k if us >= 0.07 and
 *     V <= vr; else reject if k < 0 or (us < 0.013 and V > us); else accept iff log(V) + log(invalpha) - log(a / (us us) + b)
 *     <= -lam + k loglam - lgamma(k + 1).  After ELFIHIP_POISSON_MAX_ATTEMPTS rejections (an attempt rejects with
 *     probability 0.25 at lam = 10, below 0.14 at large lam: probability below 1e-38; the bound only makes the loop finite)
 *     the result is floor(lam).
 * The device's exp, log and lgamma differ from the host's in the last places, so a draw whose u1 lies within 2^-44 of a
 * cumulative probability, or whose PTRS test is decided in the last bits, may differ from the NumPy statement by one
 * acceptance decision; above lam = 10^6 only the distribution is claimed.  Host form: host pointers, synchronises; _dev
 * form: device pointers, no synchronisation. */
#define ELFIHIP_POISSON_MAX_K 128
#define ELFIHIP_POISSON_MAX_ATTEMPTS 64
int elfihip_poisson(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, const double* lam, double* out);
int elfihip_poisson_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, const double* dlam, double* dout);

/* The Ricker model (elfi/examples/ricker.py), fused as the time-series models above: draws, the stock recurrence of every
 * simulation, the Poisson observation of every step, the three summaries and the distance in one pass.  1 <= n_obs <=
 * ELFIHIP_SERIES_MAX_OBS and n >= 1; anything else is ELFIHIP_ERR_ARG, and so is a distance without obs.
 * Stochastic form (stochastic_ricker): log_rate, sd (the reference's std), scale (n each), stock_init a host scalar.  Z (n, n_obs) standard
 * normals -- the reference's randn(batch) of step i in column i - 1; Z == NULL: element e of the row-major matrix is normal
 * number e of (seed, stream), as elfihip_randn_dev writes it.  With s_0 = stock_init, for i = 1 .. n_obs, the device's exp:
 *     s_i = s_{i-1} exp((log_rate - s_{i-1}) + sd z_i)           y_i = poisson_draw(scale s_i, seed, stream + 1, e)
 * with e = row n_obs + i - 1 (attempt j of that element reads stream + 1 + j; the normals keep `stream` to themselves).  A
 * stock that has underflowed to 0 is observed as 0; one that has overflowed (s = inf, then NaN) as NaN.
 * Deterministic form (ricker), selected by sd == scale == NULL (one without the other is ELFIHIP_ERR_ARG; Z and Zo must
 * be NULL): y_0 = stock_init, y_i = y_{i-1} exp((log_rate - y_{i-1})), i = 1 .. n_obs - 1; no draws.
 * Each step is within an ulp or two of NumPy's on the same s_{i-1} (the exponential's argument is formed identically);
 * the map is chaotic, so whole trajectories are not comparable.  Everything after the series is exact arithmetic on it,
 * bit-identical to NumPy: S (n, 3) = Mean np.mean(y, axis=1), Var np.var(y, axis=1) (ddof 0), #0 np.sum(y == 0, axis=1) as a
 * double.  Optional outputs, each may be NULL: Y (n, n_obs) the observed counts (deterministic form: the stock), St (n,
 * n_obs) the latent stock s_1 .. s_n_obs (deterministic form: the same series as Y), Zo (n, n_obs) the normals used, D (n)
 * the distance of the row of S to obs (3 host values) named by `which`:
 *   ELFIHIP_RICKER_CHI2         (((S0 - o0)^2 / o0) + ((S1 - o1)^2 / o1)) + ((S2 - o2)^2 / o2), the reference's chi_squared; an
 *                               observed 0 gives inf or NaN as there
 *   ELFIHIP_RICKER_EUCLID_MEAN  sqrt((S0 - o0)^2), bit-identical to elfihip_dist_rows 'euclidean' on the Mean column
 * Host form: contiguous host arrays, synchronises.  _dev form: device pointers, Z, S, Y, St, Zo with the caller's leading
 * dimension (in doubles), no synchronisation.  obs is a host array in both. */
#define ELFIHIP_RICKER_CHI2 0
#define ELFIHIP_RICKER_EUCLID_MEAN 1
int elfihip_ricker_summaries(elfihip_ctx* ctx, const double* Z, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                             const double* log_rate, const double* sd, const double* scale, double stock_init,
                             const double* obs, int which, double* S, double* Y, double* St, double* Zo, double* D);
int elfihip_ricker_summaries_dev(elfihip_ctx* ctx, const double* dZ, int64_t ldz, uint64_t seed, uint64_t stream, int64_t n,
                                 int n_obs, const double* dlog_rate, const double* dsd, const double* dscale,
                                 double stock_init, const double* obs, int which, double* dS, int64_t lds, double* dY,
                                 int64_t ldy, double* dSt, int64_t ldst, double* dZo, int64_t ldzo, double* dD);

/* The stochastic Lotka-Volterra model (elfi/examples/lotka_volterra.py; Owen, Wilkinson and Gillespie 2015): Gillespie's
 * direct method for prey x and predators y, observed at n_obs evenly spaced times, the nine summaries and the distance
 * (csrc/gillespie.hip; the NumPy statement is tests/lv_ref.py).  Per simulation: r1, r2, r3, prey_init, predator_init and
 * optionally sigma (n each); host scalars n_obs, time_end, max_events.  x = floor(prey_init), y = floor(predator_init), t = 0,
 * kept as doubles (exact; the reference's int32 stock would wrap past 2^31).  Event k = 1, 2, .. in fp64, FMA contraction off:
 *     h0 = r1 x;  h1 = (r2 x) y;  h2 = r3 y;  s = (h0 + h1) + h2;  inv = 1.0 / s
 *     t_new = t + inv e_k                                  e_k a unit exponential
 *     p0 = h0 inv;  p1 = h1 inv;  c0 = p0;  c1 = p0 + p1
 *     reaction = (u_k >= c0) + (u_k >= c1)                 0: x + 1    1: x - 1, y + 1    2: y - 1;   isinf(inv): none
 *     apply;  if y == 0: t_new = time_end
 * Observation times t_out are np.linspace(0, time_end, n_obs): i (time_end / (n_obs - 1)), the last one time_end itself.
 * Observation 0 is the initial state, without noise.  Observation i >= 1 belongs to the first event j >= 1 with t_j >=
 * t_out[i]; its value is, per species with stock s,
 *     v = ((s_j - s_{j-1}) ((t_out[i] - t_{j-1}) / (t_j - t_{j-1})) + s_{j-1}) + sigma z
 * (the reference's linear interpolation between events; without sigma nothing is added), stored as the reference's int32
 * slot keeps it: truncated toward zero, -0 as +0, as a double; |v| >= 2^31 or NaN is stored as NaN (the reference's cast is
 * undefined there).  The simulation stops at the first event with t >= time_end, the y == 0 case included.  IEEE
 * arithmetic carries the degenerate cases as NumPy does: with both species at 0, inv = inf, no reaction, y == 0 ends the
 * simulation and every observation is 0.
 * Randomness.  Given form: E and U (n, n_events) unit exponentials and uniforms in [0, 1), column k - 1 feeds event k and
 * max_events = n_events; Z (n, 2 (n_obs - 1)) standard normals with sigma, observation i's prey at column 2 (i - 1), its
 * predator next to it (the reference's draw order).  Drawn form (E == U == NULL): event k of simulation i reads Philox
 * counter p = ((first + i) << 32) | k of (seed, stream) (csrc/philox.hpp's layout with p in place of the pair index):
 * e_k = -log((((w0 << 21) | (w1 >> 11)) + 1) 2^-53), u_k = ((w2 << 21) | (w3 >> 11)) 2^-53.  Z == NULL with sigma: noise normal
 * number (first + i) 2 (n_obs - 1) + q is that normal of (seed, stream + 1), as elfihip_randn_dev writes it.  `first` shifts the
 * simulation indices of a call (first + n <= 2^32): simulation i of one call is simulation 0 of a call with first = i.  So
 * a simulation's result is a function of its own parameters, (seed, stream, first + i), n_obs and time_end alone: not of n,
 * of the grid, of max_events short of reaching it, or of the lane that ran it.  elfihip_lv_draws writes the E and U of the
 * drawn form into memory: the drawn form IS the given form on them.
 * Limits: 3 <= n_obs <= ELFIHIP_SERIES_MAX_OBS, 1 <= max_events <= ELFIHIP_LV_MAX_EVENTS, n >= 1, time_end finite and > 0;
 * anything else is ELFIHIP_ERR_ARG, and so are a distance without obs, E without U and Z without sigma.
 * Marks per simulation, status (int32) and the number of events made (int64):
 *   ELFIHIP_LV_REACHED_END    an event reached time_end
 *   ELFIHIP_LV_EXTINCT        the predators died out (the time is set to time_end)
 *   ELFIHIP_LV_OUT_OF_EVENTS  max_events used up before time_end: the observations not yet emitted are NaN, and so are the
 *                             row's summaries and distance.  The reference has no such bound: it doubles its arrays and
 *                             goes on for as long as the slowest simulation of the batch takes.
 *   ELFIHIP_LV_INVALID        a rate or sigma NaN, negative or infinite, or a floored initial stock NaN, negative or >= 2^31:
 *                             every output of the row is NaN, 0 events
 * Outputs, each may be NULL: Y (n, n_obs, 2) the observations (prey, predator), T (n) the time of the last event, status,
 * events, S (n, 9) the summaries in the reference's order -- prey / predator mean, log-variance log(var(ddof 1) + 1),
 * autocorrelation lag 1 and lag 2 ((y - mean) / std(ddof 1), products summed and divided by n_obs - 1), the
 * cross-correlation (std with ddof 0, divided by n_obs - 1 as the reference has it) -- with NumPy's pairwise sums,
 * bit-identical to the reference's functions except for the device's log in the log-variances (within 4 ulp); a constant
 * series gives 0 / 0 = NaN in its correlations as there.  D (n): euclidean distance of the row of S to obs (9 host values),
 * bit-identical to elfihip_dist_rows 'euclidean'.
 * Host form: contiguous host arrays, synchronises.  _dev form: device pointers, E, U, Z, Y, S with the caller's leading
 * dimension (in doubles; Y's per simulation), no synchronisation.  obs is a host array in both. */
#define ELFIHIP_LV_SUMMARIES 9
#define ELFIHIP_LV_MAX_EVENTS (1LL << 30)
#define ELFIHIP_LV_REACHED_END 0
#define ELFIHIP_LV_EXTINCT 1
#define ELFIHIP_LV_OUT_OF_EVENTS 2
#define ELFIHIP_LV_INVALID 3
int elfihip_lv_summaries(elfihip_ctx* ctx, const double* E, const double* U, const double* Z, uint64_t seed, uint64_t stream,
                         int64_t first, int64_t n, int n_obs, double time_end, int64_t max_events, const double* r1,
                         const double* r2, const double* r3, const double* prey, const double* pred, const double* sigma,
                         const double* obs, double* Y, double* T, int32_t* status, int64_t* events, double* S, double* D);
int elfihip_lv_summaries_dev(elfihip_ctx* ctx, const double* dE, int64_t lde, const double* dU, int64_t ldu, const double* dZ,
                             int64_t ldz, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_obs, double time_end,
                             int64_t max_events, const double* dr1, const double* dr2, const double* dr3, const double* dprey,
                             const double* dpred, const double* dsigma, const double* obs, double* dY, int64_t ldy, double* dT,
                             int32_t* dstatus, int64_t* devents, double* dS, int64_t lds, double* dD);
int elfihip_lv_draws(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int64_t n_events, double* E,
                     double* U);
int elfihip_lv_draws_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int64_t n_events,
                         double* dE, int64_t lde, double* dU, int64_t ldu);

/* The day-care-centre transmission model (elfi/examples/daycare.py; Numminen, Cheng, Gyllenberg and Corander 2013; the model
 * BOLFI was introduced on, Gutmann and Corander 2016): Gillespie's direct method for the carriage I_is of n_strains strains by the
 * n_ind individuals of each of n_dcc centres, the four summaries over the first n_obs individuals of every centre and the
 * example's distance (csrc/daycare.hip; the NumPy statement is tests/daycare_ref.py).  Per simulation: t1, t2, t3 (n each);
 * host scalars n_dcc, n_ind, n_strains, n_obs, time_end, max_events and freq (n_strains host values, NULL: 0.1 each).  Every
 * (simulation, centre) pair is simulated on its own from I = 0, t = 0.  Event k = 1, 2, .. in fp64, FMA contraction off, every
 * sum from 0 in ascending index order:
 *     k_i = sum_s I_is;  P_s = sum_i (I_is ? 1.0 / k_i : 0);  g_s = ((t1 P_s) nf + 1e-9) + t2 freq_s;  nf = 1.0 / (n_ind - 1)
 *     c_i = k_i > 0 ? t3 : 1;  hazard h_is = I_is ? 1 : c_i g_s  (recovery at rate 1, infection scaled by t3 for carriers)
 *     r_i = sum_s h_is;  cum_i = r_0 + .. + r_i;  total = cum_{n_ind - 1}
 *     t = t + e_k / total                                   e_k a unit exponential
 *     target = u_k total;  i* = #{i < n_ind - 1: target >= cum_i};  rem = target - (i* > 0 ? cum_{i* - 1} : 0)
 *     s* = #{s < n_strains - 1: rem >= h_{i* 0} + .. + h_{i* s}};  I_{i* s*} flips
 * -- the reference's choice among its row-major (individual-major) hazards, which it sums pairwise and compares as
 * probabilities: the same event unless u_k lies within rounding of a boundary.  A pair stops at ITS first event with t >=
 * time_end and the state after that event is its result: what the reference returns for batch_size = 1, n_dcc = 1.  (With
 * more it keeps every centre of every simulation of the batch jumping until the slowest has passed time_end, so that a result
 * depends on what else is in the batch; that is not reproduced.)
 * Randomness.  Given form: E and U (n, n_dcc, n_events) unit exponentials and uniforms in [0, 1), column k - 1 feeds event k
 * and max_events = n_events.  Drawn form (E == U == NULL): event k of centre c of simulation i reads the Philox counter words
 * ((c << 22) | k, first + i, stream low, stream high) under key seed: e_k = -log((((w0 << 21) | (w1 >> 11)) + 1) 2^-53), u_k =
 * ((w2 << 21) | (w3 >> 11)) 2^-53.  `first` shifts the simulation indices of a call (first + n <= 2^32).  So a pair's result is a
 * function of its simulation's parameters, (seed, stream, first + i, c) and the shape alone: not of n, of the grid, of
 * max_events short of reaching it, or of the wavefront that ran it.  elfihip_daycare_draws writes the E and U of the drawn form
 * into memory: the drawn form IS the given form on them.
 * Limits: 2 <= n_ind <= ELFIHIP_DAYCARE_MAX_IND, 1 <= n_strains <= ELFIHIP_DAYCARE_MAX_STRAINS, 1 <= n_obs <= n_ind, 1 <= n_dcc
 * <= ELFIHIP_DAYCARE_MAX_DCC, 1 <= n <= ELFIHIP_DAYCARE_MAX_BATCH, time_end finite and > 0, freq finite and >= 0, 1 <=
 * max_events <= ELFIHIP_DAYCARE_MAX_EVENTS; anything else is ELFIHIP_ERR_ARG, and so are a distance without obs and E without U.
 * Marks per pair, status (int32), the number of events made (int64) and the time of the last one:
 *   ELFIHIP_DAYCARE_REACHED_END    an event reached time_end
 *   ELFIHIP_DAYCARE_OUT_OF_EVENTS  max_events used up before time_end: the centre's summaries and the simulation's distance
 *                                  are NaN; the masks are the state reached
 *   ELFIHIP_DAYCARE_INVALID        t1, t2 or t3 NaN, negative or infinite: every centre of the simulation has this mark, 0
 *                                  events, time NaN, empty masks, NaN summaries and distance
 * Outputs, each may be NULL: M (n, n_dcc, n_obs) the observed state, bit s of a word = that individual carries strain s; T,
 * status, events (n, n_dcc); S (n, 4, n_dcc) the summaries of every centre in the reference's order --
 *   Shannon index  p_s = (observed carriers of s) / (observed carriages), 0 / 0 -> 0 and then 0 -> 1; -(sum_s p_s log p_s) in
 *                  NumPy's pairwise order: the reference's bit for bit except for the device's log (within 4 ulp)
 *   the number of strains observed;  (individuals carrying anything) / n_obs;  (individuals carrying two or more) / n_obs
 * D (n): the example's distance of S to obs (4, n_dcc host values), as elfihip_daycare_distance gives it.
 * elfihip_daycare_distance: X (n, k, m), obs (k, m) finite host values.  o_j = max_c obs_jc, 1 where that is 0; x = X / o_j and y =
 * obs / o_j, each row sorted over c (NaN last, as np.sort); D_i = (sum_j (sum_c |x_ijc - y_jc|)) / (k m), the inner sums left to
 * right and then the outer one: the reference's sum up to its order.  A NaN in X makes D_i NaN.  1 <= k <=
 * ELFIHIP_DAYCARE_DIST_MAX_SUMMARIES, 1 <= m <= ELFIHIP_DAYCARE_MAX_DCC, k m <= ELFIHIP_DAYCARE_DIST_MAX_TERMS.
 * Host forms: contiguous host arrays, synchronise.  _dev forms: device pointers and the caller's leading dimensions -- E and U
 * per (simulation, centre) row in doubles, M per (simulation, centre) row in words, S and X per simulation in doubles -- no
 * synchronisation.  freq and obs are host arrays in both. */
#define ELFIHIP_DAYCARE_SUMMARIES 4
#define ELFIHIP_DAYCARE_MAX_IND 64
#define ELFIHIP_DAYCARE_MAX_STRAINS 64
#define ELFIHIP_DAYCARE_MAX_DCC 1024
#define ELFIHIP_DAYCARE_MAX_BATCH 2147483647LL
#define ELFIHIP_DAYCARE_MAX_EVENTS (1LL << 21)
#define ELFIHIP_DAYCARE_DIST_MAX_SUMMARIES 16
#define ELFIHIP_DAYCARE_DIST_MAX_TERMS 4096
#define ELFIHIP_DAYCARE_REACHED_END 0
#define ELFIHIP_DAYCARE_OUT_OF_EVENTS 1
#define ELFIHIP_DAYCARE_INVALID 2
int elfihip_daycare_summaries(elfihip_ctx* ctx, const double* E, const double* U, uint64_t seed, uint64_t stream, int64_t first,
                              int64_t n, int n_dcc, int n_ind, int n_strains, int n_obs, double time_end, int64_t max_events,
                              const double* t1, const double* t2, const double* t3, const double* freq, const double* obs,
                              uint64_t* M, double* T, int32_t* status, int64_t* events, double* S, double* D);
int elfihip_daycare_summaries_dev(elfihip_ctx* ctx, const double* dE, int64_t lde, const double* dU, int64_t ldu, uint64_t seed,
                                  uint64_t stream, int64_t first, int64_t n, int n_dcc, int n_ind, int n_strains, int n_obs,
                                  double time_end, int64_t max_events, const double* dt1, const double* dt2, const double* dt3,
                                  const double* freq, const double* obs, uint64_t* dM, int64_t ldm, double* dT, int32_t* dstatus,
                                  int64_t* devents, double* dS, int64_t lds, double* dD);
int elfihip_daycare_draws(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_dcc, int64_t n_events,
                          double* E, double* U);
int elfihip_daycare_draws_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_dcc,
                              int64_t n_events, double* dE, int64_t lde, double* dU, int64_t ldu);
int elfihip_daycare_distance(elfihip_ctx* ctx, const double* X, int64_t n, int k, int m, const double* obs, double* D);
int elfihip_daycare_distance_dev(elfihip_ctx* ctx, const double* dX, int64_t ldx, int64_t n, int k, int m, const double* obs,
                                 double* dD);

/* The scratch-assay model (elfi/examples/scratch_assay.py; the cell-motility model of Johnston et al. 2014 with the summaries of
 * Price et al. 2018, the test problem of the BSL paper): a random walk with proliferation of the cells of a binary grid of nrows
 * x ncols cells, and its n_obs + 1 summaries (csrc/scratch_assay.hip; the NumPy statement is tests/assay_ref.py).  Per
 * simulation: pm, pp (n each).  Host scalars nrows, ncols, n_iter, obs_every -- the caller computes n_iter = int(obs_period /
 * tau) and obs_every = int(obs_interval / tau) as the example does; n_obs = n_iter / obs_every (integer division) -- and init
 * (nrows ncols host bytes, each 0 or 1, row-major): the initial grid, shared by the batch.  Iteration t = 0 .. n_iter - 1:
 *   1. num_cells = the cell count; the list = the occupied cells in row-major order (np.where).
 *   2. A full grid: the iteration does nothing and consumes no draw.
 *   3. Motility.  Slots k = 0 .. num_cells - 1 each have a candidate C[k] in [0, num_cells), a uniform P[k] and a direction
 *      M[k].  The slots with P[k] < pm are events, executed in slot order.  The event's cell is list[C[k]]; its target is the
 *      neighbour M 0: row + 1, 1: row - 1, 2: col + 1, 3: col - 1, clamped to the grid (at an edge: the cell itself).  An empty
 *      target: the cell moves there and list[C[k]] becomes the target.  A candidate may occur, and move, several times.
 *   4. Proliferation.  Fresh C, P, M over the same num_cells slots, against pp, on the list as motility left it (a cell born
 *      here is in no list before the next iteration).  The clamped target is set to 1 whether or not it was empty.
 *   5. (t + 1) % obs_every == 0: the grid is frame (t + 1) / obs_every.  Frame 0 is the initial grid.
 * P[k] < pm is evaluated as it stands: a NaN selects nothing, values outside [0, 1] are legal, no parameter value is invalid.
 * An empty grid stays empty (the reference runs it too and returns zeros).
 * S (n, n_obs + 1): ds[j] = the number of cells that differ between frames j and j + 1, j = 0 .. n_obs - 1, then the cell count
 * of frame n_obs; all integers, exact.  status (n) int32; events (n, 2) int64: the motility and the proliferation events
 * executed (the slots selected); frames (n, n_obs + 1, 32) uint32: cell c = row ncols + col at bit c % 32 of word c / 32.
 * status, events and frames may be NULL.
 * Randomness.  Given form: C int32, P float64, M uint8, each (n, n_iter, 2, nrows ncols), contiguous: row (t, f) feeds phase f
 * (0 motility, 1 proliferation) of iteration t.  Entries at k >= num_cells are never read; every entry read is checked before
 * anything is indexed by it: a C[k] outside [0, num_cells) or an M[k] above 3 ends that simulation with status
 * ELFIHIP_ASSAY_BAD_DRAW, NaN summaries, zero frames and zero event counts; no other simulation changes.  Drawn form (C == P ==
 * M == NULL; one without the others is ELFIHIP_ERR_ARG): slot k of phase f of iteration t of simulation g = first + i makes ONE
 * Philox4x32-10 call under key seed with the counter words (((2 t + f) << 10) | k, g, stream low, stream high):
 *     C[k] = (w0 num_cells) >> 32;  P[k] = ((w1 << 21) | (w2 >> 11)) 2^-53;  M[k] = w3 >> 30
 * The direction is keyed by the slot, not by the order of the events, so no draw depends on what happened before it, and a
 * simulation's result is a function of (pm, pp, init, seed, stream, first + i) and the shape alone: not of n, of the launch, or of
 * the wavefront that ran it.  (The reference's RandomState.choice rejects to be exactly uniform; the multiply-high candidate is
 * biased by at most num_cells / 2^32 < 2.4e-7.  The reference draws a direction per event in event order; its stream is not
 * reproduced.)  elfihip_assay_draws writes the C, P, M of the drawn form for num_cells (n, n_iter, 2) int32 slots per row -- zero
 * past them, num_cells clamped to [0, cells] (the host form refuses values outside) -- into memory: the drawn form IS the given
 * form on them, with num_cells the cell counts the simulation went through (0 where the grid was full).
 * Limits: 1 <= nrows ncols <= ELFIHIP_ASSAY_MAX_CELLS, 1 <= n_iter <= ELFIHIP_ASSAY_MAX_ITER, 1 <= obs_every <= n_iter (so n_obs
 * >= 1), 1 <= n <= ELFIHIP_ASSAY_MAX_BATCH, first >= 0 and first + n <= 2^32, init bytes 0 or 1; anything else is
 * ELFIHIP_ERR_ARG, before the device is touched.
 * Host forms: contiguous host arrays, synchronise.  _dev forms: device pointers, S with the caller's leading dimension lds >=
 * n_obs + 1 in doubles, no synchronisation; init is a host array in both and is done with when the call returns. */
#define ELFIHIP_ASSAY_MAX_CELLS 1024
#define ELFIHIP_ASSAY_MAX_ITER (1 << 21)
#define ELFIHIP_ASSAY_MAX_BATCH 2147483647LL
#define ELFIHIP_ASSAY_OK 0
#define ELFIHIP_ASSAY_BAD_DRAW 1
int elfihip_assay_summaries(elfihip_ctx* ctx, const int32_t* C, const double* P, const uint8_t* M, uint64_t seed, uint64_t stream,
                            int64_t first, int64_t n, int nrows, int ncols, int n_iter, int obs_every, const uint8_t* init,
                            const double* pm, const double* pp, double* S, int32_t* status, int64_t* events, uint32_t* frames);
int elfihip_assay_summaries_dev(elfihip_ctx* ctx, const int32_t* dC, const double* dP, const uint8_t* dM, uint64_t seed,
                                uint64_t stream, int64_t first, int64_t n, int nrows, int ncols, int n_iter, int obs_every,
                                const uint8_t* init, const double* dpm, const double* dpp, double* dS, int64_t lds,
                                int32_t* dstatus, int64_t* devents, uint32_t* dframes);
int elfihip_assay_draws(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_iter, int cells,
                        const int32_t* num_cells, int32_t* C, double* P, uint8_t* M);
int elfihip_assay_draws_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int n_iter, int cells,
                            const int32_t* dnum_cells, int32_t* dC, double* dP, uint8_t* dM);

/* The birth-death-mutation example (elfi/examples/bdm.py, the process of Tanaka et al. 2006 as the reference's cpp/bdm.cpp
 * evaluates it; the NumPy statement is tests/bdm_ref.py): a jump chain of a few dozen to about a thousand events per
 * simulation, two uniforms per event, one wavefront per simulation (csrc/bdm.hip).  No executable, no files.
 * Per simulation: alpha, delta, tau (n each: birth, death and mutation rate) and the host scalars N and mode.
 *   State.  clusters[0 .. N) unsigned counts, clusters[0] = 1; pop = 1, cluster_end = 1; cap = N + (mode == 1).
 *   Rates.  FMA contraction off: c0 = 0.0 + alpha, c1 = c0 + delta, c2 = c1 + tau, tot = c2.
 *   Loop.  While 0 < pop < cap, event k = 1, 2, .. takes two uniforms ue_k, uc_k in [0, 1):
 *     event = the first i with c_i > ue_k tot; cluster = the first i < cluster_end with
 *     (double)(clusters[0] + .. + clusters[i]) > uc_k (double)pop (the cumulative sum is an integer).
 *     event 0: clusters[cluster] += 1, pop += 1.  event 1: clusters[cluster] -= 1, pop -= 1.
 *     event 2, only if clusters[cluster] > 1: clusters[cluster] -= 1, the first j in [0, N) with clusters[j] == 0 becomes 1 and
 *     cluster_end = max(cluster_end, j + 1).  Event 2 on a singleton changes nothing, but counts as an event and uses both draws.
 *   Undo.  mode 1 (Stadler's stopping rule, the one the ELFI model uses) stops when the population WOULD exceed N: the birth
 *     that reached cap is taken back.  mode 0 stops on reaching N.
 *   A search that finds no index -- impossible for valid rates and uniforms below 1, u tot < tot and u pop < pop in fp64 -- takes
 *   its last candidate (event 2, cluster cluster_end - 1); nothing is ever indexed outside [0, N).
 * Randomness.  Given form: U (n, 2 max_events) doubles, column 2 (k - 1) is ue_k and the next uc_k.  Every uniform is checked
 * before anything is indexed by it: one that is NaN or outside [0, 1) ends ITS simulation with status INVALID (events = the
 * events completed before it); no other simulation changes.  Drawn form (U == NULL): event k of simulation i reads Philox4x32-10
 * counter ((first + i) << 32) | k of (seed, stream), in philox.hpp's layout (counter words k, first + i, stream low, stream
 * high; key seed):  ue_k = ((w0 << 21) | (w1 >> 11)) 2^-53,  uc_k = ((w2 << 21) | (w3 >> 11)) 2^-53.
 * elfihip_bdm_draws writes these into memory, U (n, 2 n_events): the drawn form IS the given form on them.  A simulation's
 * result depends only on its own parameters, (seed, stream, first + i), N and mode: not on n, the grid, max_events short of
 * reaching it, or the wavefront that ran it.
 * status (n) int32, events (n) int64 (the events made):
 *   ELFIHIP_BDM_REACHED_N 0      the population reached N: normal outputs
 *   ELFIHIP_BDM_EXTINCT 1        pop reached 0: clusters all 0, T1 = 0 / 0 = NaN and T2 = 1, as NumPy gives
 *   ELFIHIP_BDM_OUT_OF_EVENTS 2  max_events used up: clusters as they stand (no undo), both summaries and the distance NaN
 *                                (the reference has no bound and with alpha = delta = 0 never returns)
 *   ELFIHIP_BDM_INVALID 3        a rate NaN, negative or infinite, tot zero or infinite, or a bad given uniform: clusters 0,
 *                                summaries and distance NaN; 0 events for bad rates
 * Outputs, each may be NULL.  Cl (n, N) int32.  T (n, 2): T1 = count(clusters > 0) / sum(clusters), one fp64 division of two
 * exact integers; T2 = 1 - sum((clusters / t2_n)^2): divide, square, then NumPy's pairwise sum over the N terms -- bit-identical
 * to the reference's T2(clusters, n=t2_n).  D (n): |T1 - obs[0]|, the example's minkowski p = 1 on one summary, bit-identical to
 * elfihip_dist_rows on that column; obs is a HOST pointer to one double in both forms.
 * Limits: 1 <= N <= ELFIHIP_BDM_MAX_N, mode 0 or 1, 1 <= max_events <= ELFIHIP_BDM_MAX_EVENTS, n >= 1, first >= 0 and
 * first + n <= 2^32; anything else is ELFIHIP_ERR_ARG, and so is a distance without obs.  (The reference's
 * cpp/example_input.txt runs N = 10000: a third level of the search tree would carry it.)
 * Host forms: contiguous host arrays, synchronise.  _dev forms: device pointers, U, Cl and T with the caller's leading dimension
 * (ldu >= 2 max_events in doubles, ldc >= N in int32, ldt >= 2 in doubles), no synchronisation. */
#define ELFIHIP_BDM_MAX_N 4096
#define ELFIHIP_BDM_MAX_EVENTS (1 << 30)
#define ELFIHIP_BDM_REACHED_N 0
#define ELFIHIP_BDM_EXTINCT 1
#define ELFIHIP_BDM_OUT_OF_EVENTS 2
#define ELFIHIP_BDM_INVALID 3
int elfihip_bdm_clusters(elfihip_ctx* ctx, const double* U, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int N,
                         int mode, int64_t max_events, const double* alpha, const double* delta, const double* tau, double t2_n,
                         const double* obs, int32_t* Cl, int32_t* status, int64_t* events, double* T, double* D);
int elfihip_bdm_clusters_dev(elfihip_ctx* ctx, const double* dU, int64_t ldu, uint64_t seed, uint64_t stream, int64_t first,
                             int64_t n, int N, int mode, int64_t max_events, const double* dalpha, const double* ddelta,
                             const double* dtau, double t2_n, const double* obs, int32_t* dCl, int64_t ldc, int32_t* dstatus,
                             int64_t* devents, double* dT, int64_t ldt, double* dD);
int elfihip_bdm_draws(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int64_t n_events, double* U);
int elfihip_bdm_draws_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t first, int64_t n, int64_t n_events,
                          double* dU, int64_t ldu);

/* Symmetric (beta = 0) alpha-stable variates, S1 parameterisation: the Chambers-Mallows-Stuck transform as SciPy 1.15's
 * levy_stable.rvs evaluates it (_rvs_Z1), in SciPy's order of operations, FMA contraction off (csrc/stable.hpp; the NumPy
 * statement is tests/toad_ref.py: stable_step).  From an angle TH in (-pi/2, pi/2) and a standard exponential W:
 *   alpha NaN or outside (0, 2], scale NaN or negative: NaN for that element, the batch goes on.
 *   alpha == 1: ((2 / pi) ((pi / 2) tan TH)) scale -- SciPy's alpha1func at beta = 0, 2 / pi and pi / 2 its doubles.
 *   otherwise: aTH = alpha TH, Z = (W / (cos TH / tan aTH + sin TH)) ((cos aTH + sin aTH tan TH) / W) ^ (1 / alpha); Z scale.
 * angle == expo == NULL (one without the other is ELFIHIP_ERR_ARG): element e draws its own from Philox counter e of stream
 * (seed, stream) -- TH = u1 pi + (-pi / 2) with u1 = ((r0 << 21) | (r1 >> 11)) 2^-53 in [0, 1), W = -log(u2) with u2 =
 * (((r2 << 21) | (r3 >> 11)) + 1) 2^-53 in (0, 1] -- so element e does not depend on n or on where it is drawn.  With angle
 * and expo (n each) the transform is applied to them and nothing is drawn.  The device differs from NumPy on the same TH
 * and W only through tan, sin, cos and pow.  beta != 0 and the S0 parameterisation are not provided.
 * Host form: host pointers, synchronises; _dev form: device pointers, no synchronisation, writes out[0 .. n - 1] only. */
int elfihip_stable(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, const double* alpha, const double* scale,
                   const double* angle, const double* expo, double* out);
int elfihip_stable_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, const double* dalpha, const double* dscale,
                       const double* dangle, const double* dexpo, double* dout);

/* Marchand's toad movement model (elfi/examples/toad.py) with An, Nott and Drovandi's summaries, one workgroup per
 * simulation (csrc/toad.hip; the NumPy statement is tests/toad_ref.py).  Per simulation alpha, gamma, p0 (n each).  X[0] = 0;
 * cell (day i = 1 .. n_days - 1, toad j), number c = (i - 1) n_toads + j, has four draws U, TH, W, R:
 *   the toad returns iff U < p0, and then X[i][j] = X[R][j], 0 <= R < i;
 *   otherwise X[i][j] = X[i - 1][j] + dx with dx = the stable transform above of (alpha, gamma, TH, W).
 * Given draws: U, TH, W doubles and R int32, each (n, cells) with cells = (n_days - 1) n_toads -- what the reference draws
 * per day as uniform((n_toads, batch)), levy_stable's uniform pi + (-pi / 2) and standard_exponential, choice(i, size),
 * transposed; all four or none.  A given R outside [0, i) makes that toad's positions NaN from day i on.
 * U == NULL: drawn here, a fixed function of (seed, stream, g = first_index + row, i, j), whatever the batch or the launch:
 * with the 64-bit Philox counter e = (g << 32) | (i << 16) | j,
 *   stream `stream`:      TH and W of element e exactly as elfihip_stable draws them;
 *   stream `stream + 1`:  U = ((r0 << 21) | (r1 >> 11)) 2^-53 in [0, 1), R = floor(r2 i / 2^32) (multiply-high of ONE word: day r
 *                         has probability floor or ceil of 2^32 / i over 2^32, within i 2^-32 < 2^-26 relative of 1 / i for i <
 *                         64, below 2^-19 at the largest i; NumPy's choice rejects instead -- its bits are not reproduced).
 * first_index + n <= 2^32.
 * Summaries, for every lag in lags (host array, n_lags of them, each in [1, n_days - 1]) over the n_toads (n_days - lag)
 * displacements |X[i + lag] - X[i]|: the number below thd; np.nanmedian of the others; log(max(diff(np.nanquantile(others,
 * p)), exp(-20))) for the nq probabilities p (host array, increasing in [0, 1]) -- nq + 1 columns per lag, lag by lag, then
 * np.nan_to_num(., nan=inf): NaN (no toad left: every column but the count) becomes +inf and an infinity the largest finite
 * double of its sign.  NaN displacements are neither counted nor sorted, as nanquantile drops them.  On given dx the
 * positions are NumPy's bit for bit; on the positions the counts and medians are, the log differences differ by the device's
 * log (a difference at or below exp(-20) gives -20 exactly).
 * An invalid parameter row -- alpha outside (0, 2], gamma < 0, p0 outside [0, 1], or NaN -- gives NaN summaries, positions and
 * steps for that row alone.  Limits: n >= 1, n_days >= 2, n_toads >= 1, n_days n_toads <= ELFIHIP_TOAD_MAX_CELLS, 1 .. MAX_LAGS
 * lags, 1 .. MAX_QUANTILES probabilities, thd not NaN; anything else is ELFIHIP_ERR_ARG.
 * Outputs: S (n, (nq + 1) n_lags); optional, each may be NULL: X (n, n_days n_toads) the positions, row-major (day, toad) --
 * the reference's X is (n_days, n_toads, batch); Dx (n, cells) the steps of every cell, used or not; Uo, THo, Wo, Ro (n, cells)
 * the draws used, all four or none.  Host form: contiguous host arrays, synchronises.  _dev form: device pointers, the
 * given draws at pitch ldd, S at lds, X at ldx, Dx at lddx, the draw outputs at ldo (in elements), no synchronisation;
 * lags and p are host arrays in both. */
#define ELFIHIP_TOAD_MAX_CELLS 8192
#define ELFIHIP_TOAD_MAX_LAGS 8
#define ELFIHIP_TOAD_MAX_QUANTILES 64
int elfihip_toad_summaries(elfihip_ctx* ctx, const double* U, const double* TH, const double* W, const int32_t* R, uint64_t seed,
                           uint64_t stream, int64_t first_index, int64_t n, int n_toads, int n_days, int n_lags, const int* lags,
                           int nq, const double* p, double thd, const double* alpha, const double* gamma, const double* p0,
                           double* S, double* X, double* Dx, double* Uo, double* THo, double* Wo, int32_t* Ro);
int elfihip_toad_summaries_dev(elfihip_ctx* ctx, const double* dU, const double* dTH, const double* dW, const int32_t* dR,
                               int64_t ldd, uint64_t seed, uint64_t stream, int64_t first_index, int64_t n, int n_toads,
                               int n_days, int n_lags, const int* lags, int nq, const double* p, double thd,
                               const double* dalpha, const double* dgamma, const double* dp0, double* dS, int64_t lds,
                               double* dX, int64_t ldx, double* dDx, int64_t lddx, double* dUo, double* dTHo, double* dWo,
                               int32_t* dRo, int64_t ldo);

/* General alpha-stable variates: SciPy 1.15's levy_stable.rvs(alpha, beta, loc, scale) per element, in SciPy's order of
 * operations, FMA contraction off (csrc/stable.hpp: stable_general; the NumPy statement is tests/sv_ref.py:
 * stable_general_step).  From an angle TH and a standard exponential W, with aTH = alpha TH:
 *   alpha NaN or outside (0, 2], beta NaN or outside [-1, 1], scale NaN or negative: NaN for that element, the batch goes on
 *   (SciPy raises for the whole call -- the one difference).
 *   Z, SciPy's _rvs_Z1:
 *     alpha == 1: (2 / pi) ((pi / 2 + beta TH) tan TH - beta log(((pi / 2) W cos TH) / (pi / 2 + beta TH)));
 *     beta == 0:  the symmetric expression of elfihip_stable above, one and the same function;
 *     otherwise:  val0 = beta tan(pi alpha / 2), th0 = atan(val0) / alpha, val3 = W / (cos TH / tan(alpha (th0 + TH)) + sin TH),
 *                 Z = val3 (((cos aTH + sin aTH tan TH) - val0 (sin aTH - cos aTH tan TH)) / W) ^ (1 / alpha).
 *   X1 = Z scale + loc; at alpha == 1, X1 = X1 + (((2 beta) scale) log(scale)) / pi (levy_stable.rvs's shift in S1); with s0 = 1
 *   (the S0 parameterisation) then X1 - ((((beta 2) scale) log(scale)) / pi) at alpha == 1 and X1 - (scale beta) tan((pi alpha)
 *   / 2) elsewhere; s0 = 0 is S1.  scale == 0 at alpha == 1 is 0 log 0 = NaN, as in SciPy.
 * angle == expo == NULL (one without the other is ELFIHIP_ERR_ARG): element e draws TH and W from Philox counter e of stream
 * (seed, stream) exactly as elfihip_stable does, so at beta = 0, loc = 0, s0 = 0 element e is elfihip_stable's element e.
 * With angle and expo (n each) the transform is applied to them and nothing is drawn.  The device differs from NumPy on the
 * same TH and W only through tan, sin, cos, atan, log and pow.
 * Host form: host pointers, synchronises; _dev form: device pointers, no synchronisation, writes out[0 .. n - 1] only. */
int elfihip_stable_general(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, int s0, const double* alpha,
                           const double* beta, const double* loc, const double* scale, const double* angle, const double* expo,
                           double* out);
int elfihip_stable_general_dev(elfihip_ctx* ctx, uint64_t seed, uint64_t stream, int64_t n, int s0, const double* dalpha,
                               const double* dbeta, const double* dloc, const double* dscale, const double* dangle,
                               const double* dexpo, double* dout);

/* The alpha-stable stochastic-volatility model (elfi/examples/stochastic_volatility_model.py) with its quantile-based
 * kurtosis and skewness, one workgroup per simulation (csrc/sv.hip; the NumPy statement is tests/sv_ref.py).  Per simulation
 * alpha, beta, kappa, eta, mu, phi, sigma (n each) and optionally x0 (n, or NULL).  Cell t = 0 .. n_obs - 1 has three draws:
 * a standard normal Z, an angle TH and a standard exponential W.
 *   x[0] = Z[0] (sigma / sqrt(1 - min(phi phi, 0.99999))) + mu, or with x0: x[0] = Z[0] sigma + (mu + phi (x0 - mu));
 *   x[t] = Z[t] sigma + (mu + phi (x[t - 1] - mu))          the reference's log_vol: ss.norm.rvs is standard_normal scale + loc;
 *   v[t] = the general stable transform above of (alpha, beta, loc = eta, scale = kappa, s0 = 1, TH[t], W[t]);
 *   y[t] = exp(0.5 x[t]) v[t].
 * Given draws: Z, TH, W doubles, each (n, n_obs) -- the reference draws n_obs times standard_normal(batch), then uniform((n_obs,
 * batch)) pi + (-pi / 2) and standard_exponential((n_obs, batch)), transposed here; all three or none.
 * Z == NULL: drawn here, a fixed function of (seed, stream, g = first_index + row, t), whatever the batch or the launch: with
 * the 64-bit Philox counter e = (g << 32) | t,
 *   stream `stream`:      TH and W of element e exactly as elfihip_stable and elfihip_stable_general draw them;
 *   stream `stream + 1`:  Z = the first normal of counter e: sqrt(-2 log u1) cospi(2 u2), u1 = (((r0 << 21) | (r1 >> 11)) + 1)
 *                         2^-53 in (0, 1], u2 = ((r2 << 21) | (r3 >> 11)) 2^-53 in [0, 1).
 * first_index + n <= 2^32.
 * Summaries: with q = (q_kurt[0 .. 3], q_skew[0 .. 2]) (host array of 7 probabilities in [0, 1]; the example's are 0.05, 0.25,
 * 0.75, 0.95 and 0.05, 0.5, 0.95) and Q = np.quantile(y, q) (method 'linear'): S[0] = (Q3 - Q0) / (Q2 - Q1), S[1] = ((Q6 - Q5) -
 * (Q5 - Q4)) / (Q6 - Q4).  A NaN in y makes both NaN, as np.quantile does; n_obs = 1 gives 0 / 0.  On given Z the chain x is
 * NumPy's bit for bit, on y the summaries are; v and y differ by the device's tan, sin, cos, atan, log, pow and exp.
 * An invalid parameter row -- alpha outside (0, 2], beta outside [-1, 1], kappa < 0, sigma < 0, or any parameter NaN (x0
 * included when given) -- is NaN throughout (S, y, x, v) for that row alone.  Limits: n >= 1, 1 <= n_obs <= ELFIHIP_SV_MAX_OBS;
 * anything else is ELFIHIP_ERR_ARG.
 * Outputs: S (n, 2); optional, each may be NULL: Y, X, V (n, n_obs) the returns, log-volatilities and shocks; Zo, THo, Wo (n,
 * n_obs) the draws used, all three or none.  Host form: contiguous host arrays, synchronises.  _dev form: device pointers,
 * the given draws at pitch ldd, S at lds, Y at ldy, X at ldx, V at ldv, the draw outputs at ldo (in elements), no
 * synchronisation; q is a host array in both. */
#define ELFIHIP_SV_MAX_OBS 4096
int elfihip_sv_summaries(elfihip_ctx* ctx, const double* Z, const double* TH, const double* W, uint64_t seed, uint64_t stream,
                         int64_t first_index, int64_t n, int n_obs, const double* q, const double* alpha, const double* beta,
                         const double* kappa, const double* eta, const double* mu, const double* phi, const double* sigma,
                         const double* x0, double* S, double* Y, double* X, double* V, double* Zo, double* THo, double* Wo);
int elfihip_sv_summaries_dev(elfihip_ctx* ctx, const double* dZ, const double* dTH, const double* dW, int64_t ldd, uint64_t seed,
                             uint64_t stream, int64_t first_index, int64_t n, int n_obs, const double* q, const double* dalpha,
                             const double* dbeta, const double* dkappa, const double* deta, const double* dmu, const double* dphi,
                             const double* dsigma, const double* dx0, double* dS, int64_t lds, double* dY, int64_t ldy, double* dX,
                             int64_t ldx, double* dV, int64_t ldv, double* dZo, double* dTHo, double* dWo, int64_t ldo);

/* The stochastic Lorenz-96 forecast model (elfi/examples/lorenz.py), fused the same way: draws, the Runge-Kutta recurrence,
 * the six summaries and the distance in one pass; series and summaries bit-identical to the reference's NumPy on the same
 * draws.  K = n_obs variables in 4 .. ELFIHIP_LORENZ_MAX_VARS, T = n_timestep >= 2 rows, T K <= ELFIHIP_LORENZ_MAX_TERMS
 * (NumPy's reduction buffer: beyond it its summation order changes); anything else is ELFIHIP_ERR_ARG.
 * E (n, T - 1, K) standard normals -- the reference's normal(0, 1, (batch, K)) of steps 1 .. T - 1, stacked along axis 1;
 * E == NULL: element e of that row-major array is normal number e of (seed, stream), as elfihip_randn_dev writes them.
 * Row 0 of a series is y0 -- one row of K values shared by all simulations or (n, K).  For i = 1 .. T - 1, with c =
 * sqrt(1 - phi^2) and h = total_duration / T as the host computes them:
 *     eta  = phi eta + E_i c                                                    (eta starts as 0)
 *     dy_k = ((((-y[k-2] y[k-1] + y[k-1] y[k+1]) - y[k]) + f) - (theta1 + y[k] theta2)) + eta[k]       (indices cyclic)
 *     k1 = h dy(y), k2 = h dy(y + k1 / 2), k3 = h dy(y + k2 / 2), k4 = h dy(y + k3), y = y + (((k1 + 2 k2) + 2 k3) + k4) / 6
 * S (n, 6): Mean, Var, Autocov, Cov, CrosscovPrev, CrosscovNext (lorenz.py: mean, var, autocov, cov, xcov(prev), xcov(next)).
 * Y (n, T K): the series, (T, K) row-major per simulation.  D (n): euclidean distance of the row of S to obs (6 values),
 * bit-identical to elfihip_dist_rows on S.  Host form: y0_per_simulation 0 = y0 is (K), else (n, K).  _dev form: ldE, lds,
 * ldy are the pitches between simulations, ldy0 == 0 says one shared row, else the pitch of the (n, K) rows. */
#define ELFIHIP_LORENZ_MAX_VARS 64
#define ELFIHIP_LORENZ_MAX_TERMS 8192
int elfihip_lorenz_summaries(elfihip_ctx* ctx, const double* E, uint64_t seed, uint64_t stream, int64_t n, int n_obs,
                             int n_timestep, const double* t1, const double* t2, double f, double c, double phi, double h,
                             const double* y0, int y0_per_simulation, const double* obs, double* S, double* Y, double* D);
int elfihip_lorenz_summaries_dev(elfihip_ctx* ctx, const double* dE, int64_t ldE, uint64_t seed, uint64_t stream, int64_t n,
                                 int n_obs, int n_timestep, const double* dt1, const double* dt2, double f, double c, double phi,
                                 double h, const double* dy0, int64_t ldy0, const double* obs, double* dS, int64_t lds,
                                 double* dY, int64_t ldy, double* dD);

/* The g-and-k quantile-distribution models (elfi/examples/gnk.py, bignk.py), fused the same way: draws, the quantile
 * function, a sort of every (simulation, dimension) column, the octiles, the robust statistics and the distance in one
 * pass.  dim = 1 (GNK) or 2 (BiGNK), n_obs >= 2, n_obs dim <= ELFIHIP_SERIES_MAX_OBS; anything else is ELFIHIP_ERR_ARG.
 * P (n, 4) = A, B, g, k at dim = 1, (n, 9) = A1, A2, B1, B2, g1, g2, k1, k2, rho at dim = 2 (the reference's argument
 * order); c a host scalar.  Z (n, n_obs dim): the normals, (n_obs, dim) row-major per simulation and at dim = 2 ALREADY
 * correlated (what multivariate_normal.rvs returns); Z == NULL: element e of the row-major (n, n_obs, dim) array is normal
 * number e of (seed, stream), as elfihip_randn_dev writes them, and at dim = 2 the pair (e0, e1) of an observation becomes
 * z0 = e0, z1 = (rho e0) + (sqrt(1 - rho rho) e1) -- the distribution of the reference's draws, not their bits.
 * Per element, with the parameters of its dimension and the device's exp and pow:
 *     y = A + ((B (1 + c ((1 - exp(-(g z))) / (1 + exp(-(g z)))))) pow(1 + z z, k)) z
 * -- the reference's order of operations; exp(-(g z)) = inf gives NaN as there.  The series is within a few units
 * eps (|A| + |y - A|) of NumPy's (the two exp / pow differ in the last place and the bracket amplifies that);
 * everything after it is exact arithmetic on the series and bit-identical to NumPy:
 * Y (n, n_obs dim): the series, (n_obs, dim) row-major per simulation -- the reference's ss_order, whose np.sort runs
 * along the last axis.  Zo, same shape: the normals used.  Ys, same shape: every column sorted, np.sort(y, axis=1), NaNs
 * last.  O (n, 7 dim) = [E1_d0, E1_d1, E2_d0, ...]: ss_octile = np.percentile(y, linspace(12.5, 87.5, 7), axis=1) from the
 * positions the host computed by NumPy's virtual-index rule -- sorted neighbours a = s[lo[k]], b = s[hi[k]], weight t[k]:
 * a + (b - a) t[k] if t[k] < 0.5, else b - (b - a) (1 - t[k]); a column that holds a NaN gives NaN throughout.
 * R (n, 4 dim) = [A_d0, A_d1, B_d0, ...]: ss_robust, ss_A = E4, ss_B = E6 - E2 (an exactly zero ss_B becomes 0 + DBL_EPSILON),
 * ss_g = ((E6 + E2) - 2 E4) / ss_B, ss_k = (((E7 - E5) + E3) - E1) / ss_B.
 * D (n): euclidean distance of ONE of these rows, named by `which`, to obs (n_obs dim, 7 dim or 4 dim values); bit-identical
 * to elfihip_dist_rows 'euclidean' on that row (whose order of summation changes at 300 values, here as there), and equal to
 * the reference's euclidean_multiss up to the order of its sum.  The row need not be among the outputs.  The columns are
 * sorted only when Ys, O, R or a distance on one of them is asked for.  Every output may be NULL.
 * lo, hi, t (7 each, needed for O, R and their distances) and obs are HOST arrays in both forms; an obs of more than 64
 * values is copied to the device on the context's stream.  _dev form: device pointers, every matrix with the caller's
 * leading dimension (in doubles), no synchronisation.  The host form takes contiguous arrays and synchronises. */
#define ELFIHIP_GNK_ORDER 0
#define ELFIHIP_GNK_SORTED 1
#define ELFIHIP_GNK_OCTILE 2
#define ELFIHIP_GNK_ROBUST 3
int elfihip_gnk_summaries(elfihip_ctx* ctx, const double* Z, uint64_t seed, uint64_t stream, int64_t n, int n_obs, int dim,
                          const double* P, double c, const int* lo, const int* hi, const double* t, const double* obs,
                          int which, double* Y, double* Zo, double* Ys, double* O, double* R, double* D);
int elfihip_gnk_summaries_dev(elfihip_ctx* ctx, const double* dZ, int64_t ldz, uint64_t seed, uint64_t stream, int64_t n,
                              int n_obs, int dim, const double* dP, int64_t ldp, double c, const int* lo, const int* hi,
                              const double* t, const double* obs, int which, double* dY, int64_t ldy, double* dZo,
                              int64_t ldzo, double* dYs, int64_t ldys, double* dO, int64_t ldo, double* dR, int64_t ldr,
                              double* dD);

/* ------------------------------------------------------------------- GP surrogate
 * Replaces the GPy model behind elfi.methods.bo.gpy_regression.GPyRegression
 * (elfi/methods/bo/gpy_regression.py:15-364): kernel RBF(variance, lengthscale) + Bias
 * (:260-280), Gaussian noise, exact inference.  One elfihip_gp holds the evidence
 * (X (n,d), y (n)) and, after elfihip_gp_factorize, L = chol(K + (noise + 1e-8) I),
 * L^-T and alpha = K^-1 y in device memory.  Host pointers in, host pointers out.
 */
/* capacity: the largest n this GP will hold (rounded up to a multiple of 128), 1 <= capacity <= 131072.
 * d: the input dimension, 1 <= d <= 256 (anything else is ELFIHIP_ERR_ARG); the device rows are padded to
 * dp = d rounded up to a multiple of 4.  Every entry point below works for every accepted d; which form a call takes
 * depends on dp:
 *   dp <= 24: the query points of a call of at most 16 points, and the evidence row of a one-point
 *             elfihip_gp_append / elfihip_gp_extend, travel in the kernel arguments (no copy); calls with at least
 *             min_points points (elfihip_gp_set_dense_threshold) take the dense form of the triangular products.
 *   dp  > 24: query points and appended rows are uploaded (a prediction or LCB call of at most 128 points still reads its
 *             points from pinned memory and gets its results without a copy); there is no dense form: every call streams the factor
 *             in groups of at most 128 points.
 * The Gram matrix of elfihip_gp_factorize stages X in chunks of 64 columns, so its LDS need does not grow with d. */
int elfihip_gp_create(elfihip_ctx* ctx, int d, int64_t capacity, elfihip_gp** gp);
int elfihip_gp_free(elfihip_gp* gp);
/* kern.rbf.variance, kern.rbf.lengthscale, kern.bias.variance, Gaussian_noise.variance
 * (gpy_regression.py:151-155). */
int elfihip_gp_set_hyper(elfihip_gp* gp, double rbf_variance, double lengthscale, double bias_variance,
                         double noise_variance);
/* The stationary part of the covariance function (the `kernel=` of GPyRegression, gpy_regression.py:260-280), with
 * a = |x - x'| / lengthscale and s_f = rbf_variance of elfihip_gp_set_hyper:
 *   0 rbf       s_f exp(-a^2 / 2)                                         (the default)
 *   1 matern32  s_f (1 + sqrt(3) a) exp(-sqrt(3) a)                       ([GPy-upstream] Matern32)
 *   2 matern52  s_f (1 + sqrt(5) a + 5 a^2 / 3) exp(-sqrt(5) a)           ([GPy-upstream] Matern52)
 * The bias and noise terms are unchanged.  Every entry point below follows the kind: fit, extend, prediction with gradients,
 * the acquisition surfaces, the hyper-parameter gradients (isotropic and per dimension) and the search for the mean's
 * minimiser.  Like elfihip_gp_set_hyper the call invalidates the factorisation (and K^-1): set the kind before the data,
 * or factorise again.  Any other value of `kind` is ELFIHIP_ERR_ARG and changes nothing. */
int elfihip_gp_set_kernel(elfihip_gp* gp, int kind);
int elfihip_gp_get_kernel(const elfihip_gp* gp, int* kind);
/* Replace / extend the evidence (GPyRegression.update, gpy_regression.py:286-315: np.r_[X_old, x]). */
int elfihip_gp_set_data(elfihip_gp* gp, const double* X, const double* y, int64_t n);
int elfihip_gp_append(elfihip_gp* gp, const double* X_new, const double* y_new, int64_t k);
/* Gram matrix + Cholesky + L^-T + alpha (what GPy's ExactGaussianInference does when
 * gpy_regression.py:283-284 / :311-312 construct GPRegression).  log_marginal may be NULL.
 * A failed plain Cholesky is retried the way GPy's `jitchol` does it ([GPy-upstream] GPy/util/linalg.py, reached
 * through ExactGaussianInference / pdinv from GPyRegression.update and .optimize, elfi/methods/bo/gpy_regression.py:286-323):
 * jitter = mean(diag Ky) * 1e-6 on the diagonal, ten times more per failed try, at most `maxtries` (5) tries; L, alpha,
 * log Z and L^-T then belong to the jittered matrix, as GPy's posterior object does.  ELFIHIP_ERR_NOT_PD only when the
 * last try fails too ("not positive definite, even with jitter": LinAlgError in the reference, which
 * GPyRegression.optimize catches and warns about, gpy_regression.py:320-323). */
int elfihip_gp_factorize(elfihip_gp* gp, double* log_marginal);
/* The ladder above: maxtries >= 0 sets the retries allowed (GPy: 5; 0 = fail at the first non-positive pivot),
 * maxtries < 0 leaves it.  jitter receives what the CURRENT factor carries on its diagonal besides noise + 1e-8 (0 when
 * the plain Cholesky went through), tries the retries the latest elfihip_gp_factorize made.  Pointers may be NULL.
 * elfihip_gp_extend refuses to border a factor that carries jitter (it refactors instead, as GPy would). */
int elfihip_gp_jitchol(elfihip_gp* gp, int maxtries, double* jitter, int* tries);
/* How elfihip_gp_factorize schedules its sweep over the 128-wide block columns (no reference counterpart: GPy hands
 * the factorisation to LAPACK).  schedule 0 = chosen by size (default), 1 = two-stream look-ahead with panel groups,
 * 2 = fused steps on the caller's stream (panel solve, diagonal tile, then ONE launch with the next diagonal block
 * beside the trailing update: three launches per block column); any other schedule is ELFIHIP_ERR_ARG.
 * panel_group 0 = by size, else 1 / 2 / 4 panels per pass over the trailing matrix (schedule 1).  Results agree to
 * rounding between schedules; each is deterministic. */
int elfihip_gp_set_schedule(elfihip_gp* gp, int schedule, int panel_group);
/* Which form the two triangular products of a prediction call take (no reference counterpart: the reference predicts
 * one point per call, gpy_regression.py:98-147,179-223; bo/utils.py:97-103 runs its starts one after the other).  Calls
 * with fewer than min_points query points stream the factor once per <= 128 points through (row block, k chunk)
 * workgroups -- HBM-bound, right for the 10 starts of the default LCBSC; calls with at least min_points points (default
 * 112: the 256 parallel starts of BASELINE configs[4], many-chain sampling) run both products as dense 64 x 64 MFMA
 * tiles with full-k accumulation -- matrix-pipe-bound (csrc/gp_dense.hip).  min_points <= 0 restores the default;
 * a huge value keeps every call on the streaming form.  tile_rows: rows of the factor per output tile of the dense form,
 * 0 = by size (the tallest of 64 / 32 / 16 that still gives about one workgroup per CU), else 64, 32 or 16.  Results agree
 * to rounding; each form is deterministic. */
int elfihip_gp_set_dense_threshold(elfihip_gp* gp, int64_t min_points, int tile_rows);
/* How a prediction call with few points (every step of the multi-start search, bo/utils.py:97-103) is launched:
 * form 0 (default) = four launches -- kernel rows | first triangular product | second | assembly -- the reduction of the
 * first product's chunk partials and the gradient sums of the second run as epilogues of the LAST workgroup to arrive at
 * each 32-row block (write-through partials, one relaxed device-scope arrival per workgroup, one acquire by the last
 * arriver); form 1 = the six launches of round 2 (product, reduction, product, gradient sums as kernels of their own).
 * Mean / variance are bit-identical between the forms, gradients agree to rounding (32- against 64-row chunks).
 * Acquisition lock-steps (elfihip_gp_lcb with a gradient, elfihip_gp_lcb_minimize) additionally have a THREE-launch form:
 * u = K^-1 kb from ONE product with the symmetric K^-1 instead of the two dependent triangular products (GPy's own
 * closed form with woodbury_inv, gpy_regression.py:127-140).  Under form 0 it takes over once a factorisation has served
 * 64 lock-steps -- or at once when the caller has formed K^-1 for this factorisation (elfihip_gp_form_kinv) -- (forming
 * K^-1 costs what 40-80 lock-steps save; afterwards elfihip_gp_extend borders the matrix, rank one, with every new
 * point) and while (max L_ii / min L_ii)^2 <= 1e5 (the variance k(x,x) - kb . u then agrees with
 * the triangular form to 1e-10 k(x,x)); form 2 = never (fused triangular products only); form 3 = from the first
 * lock-step on.  elfihip_gp_predict / _predict_grad always use the triangular products. */
int elfihip_gp_set_lockstep_form(elfihip_gp* gp, int form);
/* State of the above for the current factorisation: whether acquisition lock-steps multiply with K^-1 now, how many
 * lock-steps the factorisation has served, and the ESTIMATE of cond(K) that keeps hopeless matrices from being formed:
 * min(n (max L_ii / min L_ii)^2, n (var + bias + s) / s) with s = noise + 1e-8 + jitter (only the second is a true upper
 * bound; the first can lie below cond(K)).  What makes the K^-1 form fail safe is not this number: the first lock-step with
 * a newly formed K^-1 is also run through the triangular products and the two variances must agree to 1e-9 k(x,x), or the
 * factorisation keeps the triangular form.  Any pointer may be NULL. */
int elfihip_gp_lockstep_info(const elfihip_gp* gp, int* kinv_in_use, int64_t* steps, double* cond_estimate);
/* Device time per phase, for roofline accounting (bench.py; no reference counterpart).  While enabled, HIP events on the
 * GP's stream bracket the phases of elfihip_gp_factorize (Gram matrix | sweep | alpha + log-determinant), of single-group
 * prediction calls -- elfihip_gp_predict / _predict_grad / _lcb and every step of elfihip_gp_lcb_minimize -- (kernel row |
 * first triangular product + its reduction | second triangular product | gradient sums + final assembly) and of
 * elfihip_gp_nlml_grad (K^-1 tiles with the fused gradient contractions).  enable > 0 starts a fresh measurement,
 * 0 stops it, < 0 only reads; phase_ms / phase_calls (ELFIHIP_PHASE_COUNT entries each, may be NULL) receive the sums of
 * milliseconds and the number of timed calls per phase collected so far. */
enum {
  ELFIHIP_PHASE_GRAM = 0,
  ELFIHIP_PHASE_SWEEP = 1,
  ELFIHIP_PHASE_ALPHA = 2,
  ELFIHIP_PHASE_KSTAR = 3,
  ELFIHIP_PHASE_TRI_FIRST = 4,
  ELFIHIP_PHASE_TRI_SECOND = 5,
  ELFIHIP_PHASE_GRAD_FINISH = 6,
  ELFIHIP_PHASE_KINV_GRAD = 7,
  ELFIHIP_PHASE_COUNT = 8
};
int elfihip_gp_profile(elfihip_gp* gp, int enable, double* phase_ms, int64_t* phase_calls);
/* What GPy evaluates once per objective call of GPyRegression.optimize() (gpy_regression.py:317-323
 * -> [GPy-upstream] ExactGaussianInference + kern.update_gradients_full): the log marginal
 * likelihood and its gradient w.r.t. (rbf.variance, rbf.lengthscale, bias.variance,
 * Gaussian_noise.variance), grad[4], from dL/dK = 0.5 (alpha alpha^T - K^-1).  Priors and the
 * positivity transform are host-side scalars (elfi_amd/hyperopt.py).  Needs a factorised GP. */
int elfihip_gp_nlml_grad(elfihip_gp* gp, double* log_marginal, double* grad);
/* The same with the lengthscale's derivative split by input dimension, for an RBF kernel with one lengthscale per
 * dimension (GPy: RBF(input_dim, ARD=True)).  grad[4] is what elfihip_gp_nlml_grad returns;
 *     grad_dim[c] = sum_ij dL/dK_ij K_rbf,ij (X_ic - X_jc)^2 / lengthscale^3,   c < d,
 * is d logZ / d (the lengthscale of dimension c alone) at the point where all of them equal the GP's lengthscale, so
 * sum_c grad_dim[c] == grad[1] up to summation order.  The object itself stays isotropic: a caller with lengthscales l_c
 * keeps the evidence as x / l with lengthscale 1 (elfi_amd/gp.py: ScaledGPHandle) and d logZ / d l_c is grad_dim[c] / l_c.
 * The K^-1 tiles are those of elfihip_gp_nlml_grad; every tile's epilogue adds d contractions, reduced in a fixed order
 * (two calls return the same bits).  Needs a factorised GP. */
int elfihip_gp_nlml_grad_ard(elfihip_gp* gp, double* log_marginal, double* grad, double* grad_dim);
/* Materialise K^-1 (GPy's posterior.woodbury_inv, read by gpy_regression.py:158) for
 * elfihip_gp_get(gp, 5, ...).  Not needed by predict / gradients / nlml_grad. */
int elfihip_gp_form_kinv(elfihip_gp* gp);
/* GPyRegression.update with unchanged hyper-parameters (what elfi.BOLFI does for every batch between
 * two hyper-parameter optimisations, bolfi.py:219 -> gpy_regression.py:304-312): append k evidence
 * points and bring L, L^-T, alpha and the log marginal up to date by bordering -- one new row /
 * column per point, two passes over L^-T (O(n^2)) instead of the O(n^3) rebuild the reference
 * performs.  Same result as elfihip_gp_append + elfihip_gp_factorize to rounding.  Falls back to
 * exactly that when the GP is not factorised yet or the padded size (multiple of 128) grows. */
int elfihip_gp_extend(elfihip_gp* gp, const double* X_new, const double* y_new, int64_t k, double* log_marginal);
int elfihip_gp_size(const elfihip_gp* gp, int64_t* n, int64_t* capacity, int* d);
/* Copy state to the host: 0 = L (n*n lower), 1 = L^-T (n*n upper), 2 = alpha (n),
 * 3 = X (n*d), 4 = y (n), 5 = K^-1 (n*n, after elfihip_gp_form_kinv). */
int elfihip_gp_get(elfihip_gp* gp, int which, double* out);

/* GPyRegression.predict(x, noiseless) (gpy_regression.py:98-147; closed form :127-140):
 * mu_s = k_s^T alpha,  var_s = clip(s_f + s_b - k_s^T K^-1 k_s, 1e-15) (+ noise unless noiseless).
 * Xs is (S, d) row-major; mu, var get S doubles each. */
int elfihip_gp_predict(elfihip_gp* gp, const double* Xs, int64_t S, int noiseless, double* mu, double* var);
/* GPyRegression.predictive_gradients(x) (gpy_regression.py:179-223; closed form :206-218):
 * dmu (S,d), dvar (S,d).  mu/var (noiseless) are returned too when non-NULL. */
int elfihip_gp_predict_grad(elfihip_gp* gp, const double* Xs, int64_t S, double* mu, double* var,
                            double* dmu, double* dvar);
/* LCBSC.evaluate / evaluate_gradient (elfi/methods/bo/acquisition.py:262-301) for S points at
 * once: val_s = mu - sqrt(beta var),  grad_s = dmu - 0.5 dvar sqrt(beta / var)  (noiseless). */
int elfihip_gp_lcb(elfihip_gp* gp, const double* Xs, int64_t S, double beta, double* val, double* grad);

/* The inner optimisation of AcquisitionBase.acquire (elfi/methods/bo/acquisition.py:146-163 ->
 * minimize(), elfi/methods/bo/utils.py:40-111) for the LCBSC rule: minimise
 * a(x) = mu(x) - sqrt(beta var(x)) inside the box [lower, upper] from S start points (S, d).
 * The reference runs scipy L-BFGS-B from each start in turn, one GP prediction per evaluation;
 * here all starts advance in lock-step with ONE batched device evaluation per step; each start
 * is an L-BFGS-B state machine with scipy's defaults (csrc/lbfgsb.hpp, csrc/gp_acq.hip).
 * x_out (S,d) and f_out (S) receive every start's end point / value (the caller takes the
 * arg-min, utils.py:105-109); iters_out (S) and n_eval_out (total point evaluations) may be NULL. */
int elfihip_gp_lcb_minimize(elfihip_gp* gp, const double* starts, int64_t S, const double* lower,
                            const double* upper, double beta, int maxiter, double* x_out, double* f_out,
                            int* iters_out, int64_t* n_eval_out);
/* Options of that search (no environment switches): host_threads of the quasi-Newton algebra for searches of >= 64 starts
 * (0: min(16, hardware threads, CPUs the cgroup grants)); trace: 1 = one line per search on stderr (rounds, evaluations,
 * device / host milliseconds), 2 = + active points and device time of every round, 0 = nothing. */
int elfihip_gp_set_acq_options(elfihip_gp* gp, int host_threads, int trace);

/* GPyRegression.predict_mean alone (gpy_regression.py:98-147, the mean of :127-140): mu_s = sum_i (k(x_s, X_i) + s_b) alpha_i
 * for S host points Xs (S, d) row-major, mu (S).  No triangular product and none of the prediction scratch is touched: O(n d)
 * per point.  The terms are those of elfihip_gp_predict -- r2 = (|x|^2 + |X_i|^2) - 2 x.X_i clipped at 0,
 * k = s_f exp(r2 (-1 / 2 l^2)), |x|^2 summed on the host in ascending order of the dimension -- in a FIXED order of
 * summation that depends on n alone: one workgroup of 256 threads per point; thread t adds the terms i = t, t + 256,
 * t + 512, ... in ascending order; the 64 lanes of each wave are added by the xor butterfly (distances 32, 16, 8, 4, 2, 1);
 * the four waves as ((w0 + w1) + w2) + w3.  So one call with S points gives the bits of S calls with one point, and the
 * result differs from elfihip_gp_predict's mean (256-row blocks, then the blocks in order) by the order of n additions:
 * at most 2 n 2^-53 sum_i |alpha_i| (s_f + s_b).  Every accepted d (1 ... 256); S from 0 to 2^31 - 1 (one workgroup per
 * point in one launch; ELFIHIP_ERR_ARG beyond). */
int elfihip_gp_predict_mean(elfihip_gp* gp, const double* Xs, int64_t S, double* mu);

/* The global minimiser of the GP mean inside the box [lower, upper] by differential evolution on the device: what
 * stochastic_optimization (elfi/methods/bo/utils.py:9-37; SciPy's differential_evolution with a latin-hypercube start and
 * polish) computes for BayesianOptimization.extract_result (elfi/methods/inference/bolfi.py:180-199), one GP prediction per
 * trial vector.  Here a generation is ONE launch (workgroup i makes member i's trial, evaluates the mean at it as
 * elfihip_gp_predict_mean does, and selects), the populations alternate between two device buffers, and the host reads the
 * converged flag once per chunk of generations (elfihip_gp_set_minimize_chunk); launches after convergence pass the
 * population through.
 *
 * The algorithm is SciPy's defaults (strategy best1bin, dither (0.5, 1), recombination 0.7, init latinhypercube) in their
 * DEFERRED form (updating='deferred'); tests/de_ref.py states it in NumPy:
 *   population   NP = max(5, popsize d) members in unit coordinates; unit p maps to x = (lo + hi) / 2 + (p - 1/2) |hi - lo|.
 *                Start: member i, dimension j = (perm_j(i) + u_ij) / NP, perm_j the stable argsort of NP uniforms.
 *   generation g = 1, 2, ...: one dither F = 1/2 + u / 2.  For member i: r0 = floor(u (NP - 1)), plus one if >= i;
 *                r1 = floor(u (NP - 2)), plus one if >= min(i, r0), then plus one if >= max(i, r0) -- so r0 != r1, both != i;
 *                fill point floor(u d); trial_j = b_j + F (p_r0,j - p_r1,j) where j is the fill point or u_j < 0.7, else
 *                p_i,j; b the member of lowest energy (lowest index on ties); a coordinate outside [0, 1] is redrawn
 *                uniformly (SciPy's _ensure_constraint).  All NP trials are evaluated on the generation's OLD population;
 *                a trial replaces its member when its energy is <= the member's.
 *   stop         after generation g >= 1 when std(E) <= tol |mean(E)| (population standard deviation), or after maxiter
 *                generations.
 *   polish       elfihip_gp_lcb_minimize from the best member with beta = 0 (the mean and its analytic gradient, L-BFGS-B);
 *                accepted only if the mean-only evaluation gives it a lower energy than the best member.
 *   random       draw (generation g, member i, slot s) = the 53-bit uniform ((r0 << 21) | (r1 >> 11)) 2^-53 of the first
 *   numbers      two words of Philox4x32-10 at counter (i (2 d + 4) + s, g, stream) under key seed (64-bit values: low
 *                word first).  Slots: 0, 1 the indices r0, r1; 2 the fill point; 3 + j the crossover of dimension j;
 *                3 + d + j its redraw; 3 + 2 d the dither (member 0's slot is the generation's).  Generation 0 is the
 *                start: slot 3 + j the uniform perm_j orders by, slot 3 + d + j the u_ij.  No draw depends on how many
 *                redraws happened.
 * A non-finite energy ends the call with ELFIHIP_ERR_STATE.  Limits (ELFIHIP_ERR_ARG before any launch): popsize >= 1,
 * popsize d <= 3840, maxiter >= 0, tol >= 0, lower < upper, all finite.
 * x_out (d) and f_out: the minimiser and the mean there (mean-only evaluation).  info_out (4, or NULL): generations made,
 * point evaluations (NP (generations + 1) + those of the polish), converged (0 / 1), polish accepted (0 / 1).  pop_out
 * (NP, d) and energies_out (NP), each or NULL: the final unit population and its energies -- with maxiter = 0 the start
 * population.
 * Decided difference from the reference: SciPy updates immediately, draws from MT19937, and the number of its draws
 * depends on the data; a run here is another, equally valid search for the same quantity. */
int elfihip_gp_minimize_mean(elfihip_gp* gp, const double* lower, const double* upper, uint64_t seed, uint64_t stream,
                             int popsize, int maxiter, double tol, int polish, double* x_out, double* f_out,
                             int64_t* info_out, double* pop_out, double* energies_out);
/* Generations enqueued between two reads of the converged flag (0: the default, 8; at most 1024).  The result does not
 * depend on it. */
int elfihip_gp_set_minimize_chunk(elfihip_gp* gp, int generations);

/* ExpIntVar (elfi/methods/bo/acquisition.py:629-821) needs the GP's posterior covariance between its M
 * integration points and each candidate: cov(p_i, q) = k(p_i, q) - k(p_i, X) K^-1 k(X, q), which the
 * reference forms per evaluate() call with cho_factor + cho_solve of the n x n matrix (:800-808).
 * set_integration_points stores V_P = L^-1 k(X, P) for P (M, d) once (valid until the evidence or the
 * hyper-parameters change); cross_cov then returns cov (M, S) row-major and, optionally, the noiseless
 * predictive variance var_q (S) of the S candidates Q (S, d): one streaming pass over V_P per 128 candidates. */
int elfihip_gp_set_integration_points(elfihip_gp* gp, const double* P, int64_t M);
int elfihip_gp_cross_cov(elfihip_gp* gp, const double* Q, int64_t S, double* cov, double* var_q);
/* The PRIOR covariance between two point sets under the GP's current hyper-parameters, out (na, nb) row-major:
 * k(a, b) = rbf.variance exp(-|a - b|^2 / 2 lengthscale^2) + bias.variance -- GPy's `kern.K(X, X2)`, which the reference's
 * ExpIntVar reaches for through `model._gp.kern.K` (elfi/methods/bo/acquisition.py:754,770).  B == NULL: k(A, A) with an
 * exact diagonal.  Host pointers; no factorisation needed. */
int elfihip_gp_kernel_matrix(elfihip_gp* gp, const double* A, int64_t na, const double* B, int64_t nb, double* out);
/* MaxVar / RandMaxVar surface (elfi/methods/bo/acquisition.py:392-463): the variance of the unnormalised approximate
 * posterior prior(x)^2 [Phi_skew(eps) - Phi(eps)^2] at S points and its gradient, from ONE batched prediction with the
 * skew-normal / Owen's-T epilogue on the device (the reference: three single-point GP predictions and SciPy's skewnorm
 * per value/gradient pair).  prior_pdf (S) and prior_grad_logpdf (S, d) are the prior's density and the gradient of its
 * logarithm at the points (host callables of the caller's prior object); val (S), grad (S, d). */
int elfihip_gp_maxvar(elfihip_gp* gp, const double* Xs, int64_t S, double eps, const double* prior_pdf,
                      const double* prior_grad_logpdf, double* val, double* grad);
/* ExpIntVar loss (acquisition.py:795-821) of S candidates against the integration points fixed by
 * elfihip_gp_set_integration_points: 2 sum_i w_i T(z_i, a_is) with the posterior covariances taken from the device
 * factorisation (the reference: cho_factor + cho_solve of the n x n matrix per call).  w_int = omega_i prior(p_i)^2,
 * mean_int / var_int = GP mean and noiseless variance at the integration points (M each); loss (S). */
int elfihip_gp_expintvar(elfihip_gp* gp, const double* Q, int64_t S, double eps, const double* w_int,
                         const double* mean_int, const double* var_int, double* loss);

/* ---- the same multi-start search for objectives the HOST assembles -----------------------
 * scipy.optimize.minimize(method='L-BFGS-B') as the reference calls it from minimize()
 * (elfi/methods/bo/utils.py:97-103: jac given, bounds, maxiter, SciPy's default tolerances), turned
 * inside out so that S searches share batched evaluations: the acquisition rules other than LCBSC
 * (MaxVar.acquire, acquisition.py:349-384) combine device predictions with host-side formulas, so their
 * objective cannot live inside the library.  Usage: create with the S start points; then repeat
 *   n = pending(idx, x)        the searches that wait for an evaluation and where (n == 0: all done)
 *   feed(n, f, g)              objective values (n) and gradients (n, d) at those points, same order
 * and read every search's end point.  Pure host code (no device, no context). */
typedef struct elfihip_lbfgsb elfihip_lbfgsb;
int elfihip_lbfgsb_create(int d, int64_t S, const double* lower, const double* upper, const double* starts,
                          int maxiter, elfihip_lbfgsb** out);
/* idx (S) / x (S, d) receive the waiting searches' indices and points; returns their number, < 0 on error. */
int64_t elfihip_lbfgsb_pending(elfihip_lbfgsb* h, int64_t* idx, double* x);
int elfihip_lbfgsb_feed(elfihip_lbfgsb* h, int64_t n, const double* f, const double* g);
/* x (S, d), f (S), iters (S), status (S: 1 projected gradient, 2 relative reduction, 3 maxiter, 4 abnormal, 5 maxfun = 15000 evaluations);
 * any of f / iters / status may be NULL. */
int elfihip_lbfgsb_result(const elfihip_lbfgsb* h, double* x, double* f, int* iters, int* status);
int elfihip_lbfgsb_free(elfihip_lbfgsb* h);

/* ------------------------------------------------------------------- ROMC: Robust Optimisation Monte Carlo (csrc/romc.hip)
 * elfi.ROMC (elfi/methods/inference/romc.py; RomcPosterior, elfi/methods/posteriors.py:393-800) for the MA2 example: D = 2
 * parameters, 3 <= n_obs <= 126.  ROMC freezes the simulator's noise into n1 deterministic objectives and evaluates them
 * hundreds of thousands of times; here problem i's noise is one row of a matrix the handle keeps on the device, and every
 * call below is one launch with one wavefront per problem or region.
 *
 * The objective.  f_i(theta) = D D, D the distance of elfihip_ma2_distance_dev for the row w_i and theta = (t1, t2):
 *   x_k = (w[k+2] + t1 w[k+1]) + t2 w[k], S1 / S2 the lag-1 / lag-2 means in NumPy's pairwise order, FMA contraction off,
 *   D = sqrt((S1 - obs1)^2 + (S2 - obs2)^2)
 * -- bit for bit the square of that call's distance.  The rule is D D, not pow(D, 2): the reference's float(d) ** 2 goes
 * through libm's pow, which differs from d d in about one value of a thousand.
 *
 * The handle owns the (n1, n_obs + 2) noise matrix: either the caller's W, or row i = normals 0 .. n_obs + 1 of stream
 * (seeds[i], streams[i]) of elfihip_randn_dev, i.e. what elfihip_ma2_draw_distance_dev(seeds[i], streams[i], n = 1)
 * simulates from.  Exactly one of W and the (seeds, streams) pair is given.  The host forms return when the work is done
 * and answer a problem index outside [0, n1) with ELFIHIP_ERR_ARG; the _dev forms enqueue on the context's stream, return
 * without synchronising and answer such an index with NaN (counts: the region adds nothing). */
typedef struct elfihip_romc elfihip_romc;
enum { ELFIHIP_ROMC_MA2 = 0 };
#define ELFIHIP_ROMC_DIM 2
#define ELFIHIP_ROMC_MAX_OBS 126
#define ELFIHIP_ROMC_MAX_PROBLEMS (1 << 20)
#define ELFIHIP_ROMC_MAX_POINTS (1 << 24)
enum {
  ELFIHIP_ROMC_SOLVED = 0,     /* the simplex met xatol and fatol */
  ELFIHIP_ROMC_MAXFEV = 1,     /* SciPy's warnflag 1: the evaluation limit */
  ELFIHIP_ROMC_MAXITER = 2,    /* SciPy's warnflag 2: the iteration limit */
  ELFIHIP_ROMC_NONFINITE = 3   /* an objective value was NaN or infinite: the problem ended there, its outputs are NaN */
};
int elfihip_romc_create(elfihip_ctx* ctx, int model, int64_t n1, int n_obs, double obs1, double obs2, const double* W,
                        const uint64_t* seeds, const uint64_t* streams, elfihip_romc** out);
int elfihip_romc_create_dev(elfihip_ctx* ctx, int model, int64_t n1, int n_obs, double obs1, double obs2, const double* dW,
                            int64_t ldw, const uint64_t* dseeds, const uint64_t* dstreams, elfihip_romc** out);
int elfihip_romc_free(elfihip_romc* h);
/* f[p] = f_{prob[p]}(theta[p]) for P pairs; theta (P, 2) (device form: pitch ldt), prob (P).  One wavefront walks the pairs
 * of one problem. */
int elfihip_romc_objective(elfihip_romc* h, int64_t P, const double* theta, const int64_t* prob, double* f);
int elfihip_romc_objective_dev(elfihip_romc* h, int64_t P, const double* dtheta, int64_t ldt, const int64_t* dprob, double* df);
/* Every problem's minimum from its start x0 (n1, 2), one wavefront per problem: SciPy's _minimize_neldermead as
 * scipy.optimize.minimize(fun, x0, method='Nelder-Mead') runs it -- the initial simplex x0 and per coordinate x0_k 1.05 (0.00025
 * where x0_k is zero); reflection 2 c - w, expansion 3 c - 2 w, contraction 1.5 c - 0.5 w, inside contraction 0.5 c + 0.5 w,
 * shrink b + 0.5 (v - b) with c the centroid of all vertices but the worst w and b the best; xatol = fatol = 1e-4; an
 * evaluation beyond maxfev is refused and ends the iteration without counting it; the sort after every iteration keeps
 * ties in order.  SciPy's defaults are maxiter = maxfev = 200 D; a limit SciPy would leave infinite is given as INT32_MAX
 * (the smaller of the two is at most 2^20).  status as the enum above; a value that is not finite ends the problem.
 * At a solved point the Hessian by central second differences with the steps h_k = 2^-13 max(1, |x_k|):
 *   H_kk = ((f(x + h_k e_k) - f0) + (f(x - h_k e_k) - f0)) / (h_k h_k),   f0 = f_min,
 *   H_01 = H_10 = ((f(++) - f(+-)) - (f(-+) - f(--))) / ((4 h_0) h_1);
 * NaN for a problem that was not solved.  x_min (n1, 2), f_min (n1), hess (n1, 2, 2), nfev / nit (n1) SciPy's counts (the
 * eight evaluations of the Hessian are not in nfev). */
int elfihip_romc_solve(elfihip_romc* h, const double* x0, int maxiter, int maxfev, double* x_min, double* f_min, double* hess,
                       int32_t* nfev, int32_t* nit, int32_t* status);
int elfihip_romc_solve_dev(elfihip_romc* h, const double* dx0, int64_t ldx0, int maxiter, int maxfev, double* dx_min, int64_t ldx,
                           double* df_min, double* dhess, int32_t* dnfev, int32_t* dnit, int32_t* dstatus);
/* The bounding boxes of R accepted problems: prob (R), centre (R, 2), hess (R, 2, 2).
 * Rotation: a cyclic Jacobi sweep of the symmetric part a = H_00, d = H_11, b = (H_01 + H_10) 0.5 -- for b != 0:
 *   tau = (d - a) / (2 b), t = 1 / (tau + sqrt(1 + tau tau)) for tau >= 0, else -1 / (-tau + sqrt(1 + tau tau)),
 *   c = 1 / sqrt(1 + t t), s = t c, lambda = (a - t b, d + t b), rotation = [[c, s], [-s, c]] (columns: the eigenvectors)
 * -- and the identity when an entry of H or an eigenvalue is not finite or min |lambda| <= max |lambda| D eps (NumPy's
 * matrix_rank rule, which the reference's _find_rotation_vector applies).
 * Limits: the reference's line_search (romc.py:1971-2015) operation for operation along + and - column d from the centre,
 * one wavefront per (region, direction, side): limits (R, 2, 2) = [direction][-left offset, right offset], nfev (R, 2, 2)
 * the evaluations of each search (at most K (rep_lim + 2)).  1 <= K <= 64, 0 <= rep_lim <= 2^20, eta > 0. */
int elfihip_romc_regions(elfihip_romc* h, int64_t R, const int64_t* prob, const double* centre, const double* hess, double eps_region,
                         int K, double eta, int rep_lim, double* rotation, double* limits, int32_t* nfev);
int elfihip_romc_regions_dev(elfihip_romc* h, int64_t R, const int64_t* dprob, const double* dcentre, const double* dhess,
                             double eps_region, int K, double eta, int rep_lim, double* drotation, double* dlimits, int32_t* dnfev);
/* n2 points per region, uniform in its box, and the region's objective there: with u_jk the 53-bit uniform of the first two
 * words of Philox counter 2 j + k of stream (seed, stream + r), r the region's position in the call,
 *   t_k = u_jk (limits[r][k][1] - limits[r][k][0]) + limits[r][k][0],   theta[r][j][i] = (rot[i][0] t_0 + rot[i][1] t_1) + centre[i]
 * theta (R, n2, 2) (device form: pitch ldth per point), f (R, n2). */
int elfihip_romc_sample(elfihip_romc* h, int64_t R, const int64_t* prob, const double* centre, const double* rotation,
                        const double* limits, int64_t n2, uint64_t seed, uint64_t stream, double* theta, double* f);
int elfihip_romc_sample_dev(elfihip_romc* h, int64_t R, const int64_t* dprob, const double* dcentre, const double* drotation,
                            const double* dlimits, int64_t n2, uint64_t seed, uint64_t stream, double* dtheta, int64_t ldth, double* df);
/* count[b] = sum over the R regions of 1[f_{prob[r]}(theta_b) <= eps] (RomcPosterior._sum_over_indicators); with contain = 1
 * the point must also lie in the box (_sum_over_regions_indicators, NDimBoundingBox.contains):
 *   y_k = (ri[k][0] p_0 + ri[k][1] p_1) + (ri[k][0] (-c_0) + ri[k][1] (-c_1)),   limits[r][k][0] <= y_k <= limits[r][k][1]
 * with ri = rotation_inv (R, 2, 2); centre, rotation_inv and limits may be NULL with contain = 0.  theta (BS, 2) (device
 * form: pitch ldt), count (BS) int32, combined with integer atomics: the result does not depend on scheduling. */
int elfihip_romc_count(elfihip_romc* h, int64_t BS, const double* theta, int64_t R, const int64_t* prob, double eps, int contain,
                       const double* centre, const double* rotation_inv, const double* limits, int32_t* count);
int elfihip_romc_count_dev(elfihip_romc* h, int64_t BS, const double* dtheta, int64_t ldt, int64_t R, const int64_t* dprob, double eps,
                           int contain, const double* dcentre, const double* drotation_inv, const double* dlimits, int32_t* dcount);

/* ------------------------------------------------------------------- R-BSL: the slice samplers for gamma
 * Replaces slice_gamma_mean / slice_gamma_variance (elfi/methods/bsl/slice_gamma_mean.py, slice_gamma_variance.py), which
 * elfi.BSL calls between two likelihood evaluations of a misspecification-robust chain.  G independent problems in one
 * launch, one wavefront each; problem g is one chain's state: y (m), mean (m), cov (m, m; only the lower triangle is read,
 * rows at pitch ldc), gamma_in (m), loglik_in.  1 <= m <= 64, 0 <= max_iter <= 2^20, tau > 0, w > 0, ldc >= m, G >= 0;
 * anything else is ELFIHIP_ERR_ARG before any launch.  y, mean, gamma_in and gamma_out are (G, m) without pitch.
 *
 * Statement, with std = sqrt(diag(cov)), loglik = loglik_in, ll_curr = loglik_in; for ii = 0 .. m - 1 in order:
 *   e = -log(1 - d) of one draw d;  g = gamma[ii];  target = (loglik + prior(gamma)) - e
 *   mean (0):      lower = g - w, upper = g + w;  i = 0, while i <= max_iter: loglik = L(lower), stop when
 *                  loglik + prior(gamma | ii: lower) < target, else lower = lower - w, ++i;  the same with upper, + w
 *   variance (1):  lower = 0, upper = g + w; only the upper bound steps out
 *   shrink:        i = 0, while i < max_iter: prop = lower + (upper - lower) d of one draw d, loglik = L(prop); when
 *                  loglik + prior(gamma | ii: prop) > target: gamma[ii] = prop, ll_curr = loglik, stop; else prop < g moves
 *                  lower, anything else upper, ++i
 * `loglik` is the value of the LAST likelihood evaluated so far (after a shrink loop that used up max_iter: the last
 * rejected trial's), as in the reference.  L(x) = -1/2 ((m log 2 pi + log det C) + r' C^-1 r) with gamma[ii] = x and
 *   mean:      r = y - (mean + std o gamma), C = cov;     prior = m log((1 / tau) / 2) - (1 / tau) sum |gamma_i|
 *   variance:  r = y - mean, C = cov + diag((std o gamma)^2);   prior = sum (-(gamma_i / tau) - log tau), -inf below zero
 * evaluated from one Cholesky factorisation per call (mean) or per coordinate (variance, of C without coordinate ii's own
 * term) and a rank-one change per trial.  FMA contraction off, every sum in a fixed order, no atomics: a problem's result
 * does not depend on G.
 *
 * Draws: doubles in [0, 1), one per exponential and one per uniform, in the order above -- RandomState.exponential(1) and
 * RandomState.uniform(lower, upper) of the double random_sample() would return.  U (G, n_u): problem g takes U[g][0],
 * U[g][1], ...; U == NULL (n_u is not looked at): draw k is the 53-bit uniform of the first two words of Philox counter k of
 * stream (seed, stream + g).
 *
 * gamma_out (G, m), loglik_out (G) = ll_curr, used (G) the draws consumed, evals (G) the likelihood evaluations, status (G):
 * with OUT_OF_DRAWS (the buffer ended: used = n_u) and NONFINITE (a Cholesky pivot that is not positive, or a target that is
 * not finite -- SciPy raises, or goes on with -inf, there) the problem ends, gamma_out and loglik_out are NaN; the other
 * problems of the call are not affected, and the call gives ELFIHIP_OK.  The host form returns when the work is done; the
 * _dev form enqueues on the context's stream and returns without synchronising. */
enum { ELFIHIP_SLICE_MEAN = 0, ELFIHIP_SLICE_VARIANCE = 1 };
enum { ELFIHIP_SLICE_OK = 0, ELFIHIP_SLICE_OUT_OF_DRAWS = 1, ELFIHIP_SLICE_NONFINITE = 2 };
int elfihip_slice_gamma(elfihip_ctx* ctx, int adjustment, int64_t G, int m, const double* y, const double* mean, const double* cov,
                        int64_t ldc, const double* gamma_in, const double* loglik_in, double tau, double w, int64_t max_iter,
                        const double* U, int64_t n_u, uint64_t seed, uint64_t stream, double* gamma_out, double* loglik_out,
                        int64_t* used, int64_t* evals, int32_t* status);
int elfihip_slice_gamma_dev(elfihip_ctx* ctx, int adjustment, int64_t G, int m, const double* dy, const double* dmean,
                            const double* dcov, int64_t ldc, const double* dgamma_in, const double* dloglik_in, double tau,
                            double w, int64_t max_iter, const double* dU, int64_t n_u, uint64_t seed, uint64_t stream,
                            double* dgamma_out, double* dloglik_out, int64_t* dused, int64_t* devals, int32_t* dstatus);

/* ------------------------------------------------------------------- multi-GPU exchange (one process per GPU)
 * Replaces the pickled returns of ELFI's batch farm (elfi/client.py:268-274; the per-batch farm-out of
 * elfi/methods/parameter_inference.py:283-292): the ranks' small per-round results travel device to device over RCCL
 * (xGMI), and a factorised GP can be handed from one rank to the others.  RCCL (librccl.so) is loaded at run time by the
 * first of these calls; everything runs on the context's stream and does not synchronise.  Bootstrap as with NCCL: rank 0
 * calls elfihip_comm_unique_id (128 bytes), hands them to the other ranks by any out-of-band means (the launcher's
 * rendezvous, a file, MPI), every rank calls elfihip_comm_init_rank with its context (= its GPU). */
typedef struct elfihip_comm elfihip_comm;
int elfihip_comm_unique_id(elfihip_ctx* ctx, void* id128);
int elfihip_comm_init_rank(elfihip_ctx* ctx, const void* id128, int rank, int world_size, elfihip_comm** out);
int elfihip_comm_free(elfihip_comm* comm);
/* drecv (world_size * count) in rank order, on every rank / on `root` only (NULL elsewhere). */
int elfihip_comm_allgather_f64(elfihip_comm* comm, const double* dsend, int64_t count, double* drecv);
int elfihip_comm_gather_f64(elfihip_comm* comm, const double* dsend, int64_t count, double* drecv, int root);
int elfihip_comm_bcast_f64(elfihip_comm* comm, double* dbuf, int64_t count, int root);
/* The root's factorised GP (evidence, hyper-parameters, L, L^-T, K^-1 y, log-marginal terms) to every rank's GP object of
 * the same input dimension and capacity -- instead of the same rebuild on every GPU (the kernels are deterministic, so
 * replicas are bit-identical either way); synchronises the stream (a header travels first). */
int elfihip_comm_bcast_factor(elfihip_comm* comm, elfihip_gp* gp, int root);

#ifdef __cplusplus
}
#endif
#endif /* ELFIHIP_H */
