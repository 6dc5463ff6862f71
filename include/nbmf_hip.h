/*
 * nbmf_hip.h — C ABI of libnbmf_hip.so: the MI355X (gfx950) implementation of the NBMF-MM
 * multiplicative-update inner loop.
 *
 * The reference (siddC/nbmf_mm) has no FFI of its own: its seam is the Python call
 *   nbmf_mm_solver(...)            src/nbmf_mm/_solver.py:61-216   (outer loop)
 *   nbmf_mm_update_beta_dir(...)   src/nbmf_mm/_solver.py:5-59     (one MM iteration)
 *   NBMFMM.transform(...)          src/nbmf_mm/_base.py:162-199    (simplex-factor-only loop)
 * Each entry point below names the reference lines it replaces.  INTEGRATION.md shows the ctypes
 * stub a maintainer of the reference would add to call this library from _solver.py.
 *
 * Conventions
 *   - every function returns 0 (NBMF_OK) or a negative NBMF_ERR_* code; nbmf_last_error() gives the
 *     message of the last failure on the calling thread;
 *   - host buffers are caller-owned, C-contiguous (row-major), float64 unless stated, and are copied
 *     during the call; device memory is owned by the context;
 *   - INTERNAL LAYOUT (that of _solver.py after its orientation transpose, :113-136): the data matrix
 *     Y is m x n, the simplex factor W is k x m (columns sum to 1), the Beta factor H is k x n;
 *   - a context is not thread-safe; distinct contexts are independent; one context = one GPU.
 *     Row-sharded multi-GPU runs use one process (and one context) per GPU, joined by
 *     nbmf_comm_init (RCCL all-reduce of the k x n H-step products each iteration).
 */
#ifndef NBMF_HIP_H
#define NBMF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBMF_OK 0
#define NBMF_ERR_ARG (-1)       /* bad argument (shape, NULL, unsupported k) */
#define NBMF_ERR_HIP (-2)       /* a HIP runtime call failed, or no gfx950 device */
#define NBMF_ERR_RANGE (-3)     /* data outside [0,1]: the caller raises ValueError("X must be binary"), _base.py:90-91 */
#define NBMF_ERR_STATE (-4)     /* call order violated (e.g. run before upload) */
#define NBMF_ERR_COMM (-5)      /* RCCL failure */

#define NBMF_MASK_NONE 0
#define NBMF_MASK_F64 1         /* float64 weights; Y*mask semantics of _solver.py:30-32 */
#define NBMF_MASK_U8 2          /* bool / uint8, nonzero = observed */
#define NBMF_MASK_BITS 3        /* bit-packed (the layout under NBMF_DATA_BITS), a set bit = observed */

#define NBMF_PROJ_NORMALIZE 0   /* the reference path: /n then column renormalise, _solver.py:54,57 */
#define NBMF_PROJ_DUCHI 1       /* README.md:27-35 extension: per-row observed count, Euclidean projection */

#define NBMF_FLAG_BINARY_PATH 1 /* out_flags bit: data was {0,1} (and mask {0,1}) -> 1 byte/entry storage */

#define NBMF_MAX_K 512        /* up to 128 components run in one fused sweep; more run as slices of 128 sharing a
                                 stored Theta (8 bytes per entry of extra device memory) */

typedef struct nbmf_ctx nbmf_ctx;

/* library / device ------------------------------------------------------------------------ */
int nbmf_abi_version(void);
/* First 12 hex digits of the SHA-256 over the sources this binary was compiled from (csrc/nbmf_hip.hip, the .inc files beside it sorted
 * by name, include/nbmf_hip.h), stamped by csrc/Makefile; "unstamped" for a build that did not go through it.  bench.py
 * prints it on its line and tools/refresh_profiles.sh refuses a profile whose library is not the tree's. */
const char* nbmf_source_hash(void);
const char* nbmf_last_error(void);
int nbmf_device_count(int* count);
/* The PCI bus id of HIP device `device` ("0000:75:00.0"): which PHYSICAL card an index means in this process.  A launcher may
 * narrow every rank's view to its own card, which is then device 0 everywhere; ranks compare these strings, not indices, to
 * tell whether they share a card (bench.py: RCCL refuses two ranks on one device).  No reference counterpart. */
int nbmf_device_bus_id(int device, char* buf, int len);

/* Create a context for an m x n internal problem with k components on HIP device `device`.
 * Replaces the implicit NumPy allocations of _solver.py:109-136. */
int nbmf_create(int64_t m, int64_t n, int k, int device, nbmf_ctx** out);
int nbmf_destroy(nbmf_ctx* ctx);

/* Hyper-parameters of nbmf_mm_solver (_solver.py:66-67,74) plus the projection extension.  Any positive
 * normal eps is accepted.  The fastest form of the binary path's sweeps needs 1e-12 <= eps < 2^-22 (the reference's
 * default, 1e-8, is in there) and factors inside the range a fit keeps; outside it the sweeps take the reference's
 * own selects, one reciprocal per entry and, below 1e-70, a log-likelihood that cannot underflow (one frexp per
 * entry instead of one per trip): same results, 10-20 % slower. */
int nbmf_set_hyper(nbmf_ctx* ctx, double alpha, double beta, double eps, int projection);

/* Upload the data matrix and optional mask (replaces the per-iteration Y*mask, Y.T*mask.T,
 * (1-Y).T*mask.T products of _solver.py:22-32 by a one-time pack into MFMA tile order).
 *   transposed = 0: x is the m x n internal matrix, leading dimension ldx (elements);
 *   transposed = 1: x is n x m (the user's V under orientation="dir-beta", _solver.py:113-120)
 *                   and Y = x^T; the mask has the same shape/orientation as x.
 * mask may be NULL (mask_kind NBMF_MASK_NONE).  out_flags (may be NULL) receives NBMF_FLAG_*.
 * Returns NBMF_ERR_RANGE if any entry of x is outside [0,1] or not finite. */
int nbmf_upload(nbmf_ctx* ctx, const double* x, int64_t ldx, int transposed,
                const void* mask, int mask_kind, int64_t ldmask, int* out_flags);

/* The same upload from a host array of the given element type: NBMF_DATA_F64 (nbmf_upload), NBMF_DATA_F32, or NBMF_DATA_U8 -- uint8 /
 * bool data, one byte per entry, values 0 and 1 (anything else is out of range: NBMF_ERR_RANGE, the "X must be
 * binary" of _base.py:90-91).  The reference converts every input to float64 first (check_array(dtype=float64),
 * _base.py:83; `Y * mask` at _solver.py:30 would do it anyway); a caller that holds its binary matrix as bool or
 * uint8 hands it over as it is -- BASELINE configs[4]'s 360k x 17k is 6.1 GB that way instead of 49 GB -- and the
 * pack kernel reads the bytes (nbmf_upload_v(ctx, ptr, dtype{f64,u8}, ld); 7 "Memory at config 5").
 * ldx in ELEMENTS.  The fit is bit for bit that of the float64 upload of the same values (tested). */
#define NBMF_DATA_F64 0
#define NBMF_DATA_U8 1
#define NBMF_DATA_F32 2   /* float32 data: converted on the device (exactly, as the reference's dtype=float64 conversion does): 4 bytes per entry over PCIe */
/* BIT-PACKED operands (NBMF_DATA_BITS for x, NBMF_MASK_BITS for a mask; the two are independent, and either goes with any
 * kind of the other).  A packed matrix of logical shape rows x n is rows x ceil(n / 8) bytes; every row is packed on its
 * own as np.packbits(A != 0, axis=1) does: entry j of a row is bit 7 - j % 8 of its byte j / 8.  The 8 * ceil(n / 8) - n
 * pad bits of a row's last byte mean nothing and may hold anything.  The leading dimension of a packed array is in BYTES
 * and at least ceil(n / 8); no byte of a row beyond ceil(n / 8) - 1 is read.  One bit per entry crosses to the device, a
 * kernel there expands it into the staging the uint8 rows are copied into, and everything behind that staging runs as
 * it does for NBMF_DATA_U8 / NBMF_MASK_U8: every result is bit for bit that of the uint8 operand of the same values
 * (tested).  Packed data are binary by construction: no NBMF_ERR_RANGE.  `transposed` and nbmf_set_storage as for uint8.
 * NBMF_ERR_ARG for ldx (ldmask) < ceil(n / 8), n the row length of the array as passed.
 * The rows go up in chunks of at most 256 MiB of staged rows (NBMF_UPLOAD_CHUNK_ROWS in the environment, a test hook,
 * sets the chunk height instead: rounded up to a multiple of 128; every x_kind). */
#define NBMF_DATA_BITS 3
int nbmf_upload_v(nbmf_ctx* ctx, const void* x, int x_kind, int64_t ldx, int transposed,
                  const void* mask, int mask_kind, int64_t ldmask, int* out_flags);

/* Sparse upload of BINARY data: the user's matrix given as a CSR pattern (canonical: sorted or not, but no
 * duplicate entries; every stored entry means 1), optionally with a second CSR pattern of the OBSERVED entries
 * (mask_indptr NULL = everything observed).  Replaces `Y = Y.toarray()` of _solver.py:28-29 / _base.py:86-87
 * plus the pack: the dense matrix is never formed, on the host or on the device (1 byte per entry and image, as
 * for dense binary data).  indptr has rows+1 entries of the user's matrix (m, or n when transposed != 0). */
int nbmf_upload_csr(nbmf_ctx* ctx, const int64_t* indptr, const int32_t* indices, int64_t nnz, int transposed,
                    const int64_t* mask_indptr, const int32_t* mask_indices, int64_t mask_nnz, int* out_flags);

/* Measurement helper with no reference counterpart: fill the context with synthetic BINARY data generated on
 * the device instead of nbmf_upload -- entry (i, j) of the internal m x n matrix is 1 with probability
 * `density` and observed with probability `observed`, from a counter-based hash of (seed, i*n + j)
 * (splitmix64; nbmf_mm_amd/_hip.py:synthetic_reference regenerates it in NumPy).  For shapes whose float64
 * host array would be impractical (BASELINE configs[4]: 360k x 17k = 49 GB). */
int nbmf_generate(nbmf_ctx* ctx, uint64_t seed, double density, double observed);

/* Generate this context's SLICE of a larger synthetic matrix: entry (i, j) of the context is entry (row0 + i,
 * col0 + j) of a global matrix with n_global columns, i.e. the hash counter is (row0 + i) * n_global + (col0 + j).
 * With row0 = col0 = 0 and n_global = n this is nbmf_generate.  For multi-GPU runs at sizes no host array can
 * hold (BASELINE configs[3], 262144 x 8192 over 8 ranks): every rank generates the rows it owns of the SAME matrix
 * a single context would generate whole, so sharded and unsharded runs can be compared entry for entry. */
int nbmf_generate_slice(nbmf_ctx* ctx, uint64_t seed, double density, double observed, int64_t row0, int64_t col0,
                        int64_t n_global);

/* Storage path of the NEXT nbmf_upload.  NBMF_STORAGE_AUTO (default): the cheapest path the data allows -- byte
 * codes for binary data with a binary (or no) mask, doubles otherwise.  NBMF_STORAGE_F64: never the
 * byte codes, i.e. the arithmetic of the reference for real-valued V in [0, 1] (_base.py:90 accepts it; its tests
 * feed np.random.rand) even when the values happen to be binary.  NBMF_STORAGE_F64_WEIGHTS: doubles plus a tile of
 * float64 weights per data tile (the Y * mask of _solver.py:30-32 with a real-valued mask; all-ones without a mask).
 * Measurement and test hook with no reference counterpart: results agree with the automatic path to rounding. */
#define NBMF_STORAGE_AUTO 0
#define NBMF_STORAGE_F64 1
#define NBMF_STORAGE_F64_WEIGHTS 2
int nbmf_set_storage(nbmf_ctx* ctx, int storage);

/* Number of observed entries held by this context: Y.size or count_nonzero(mask), _solver.py:151,155. */
int nbmf_get_n_obs(nbmf_ctx* ctx, double* n_obs);

/* Factors in internal layout: W is k x m, H is k x n, C-contiguous (_solver.py:132-136; the caller
 * has already drawn / transposed / column-normalised them). */
int nbmf_set_factors(nbmf_ctx* ctx, const double* W_kxm, const double* H_kxn);
int nbmf_get_factors(nbmf_ctx* ctx, double* W_kxm, double* H_kxn);

/* The hot loop, _solver.py:143-175: up to max_iter MM iterations (H-step, W-step, loss) with the
 * relative-change stop rule (:169-174, checked on device).  losses must hold max_iter doubles;
 * *n_iter receives iteration+1 (:215).  Factors stay on the device (nbmf_get_factors). */
int nbmf_run(nbmf_ctx* ctx, int max_iter, double tol, double* losses, int* n_iter);

/* n_problems INDEPENDENT fits of the data this context holds, each with its own Beta prior (alpha[p], beta[p]) and its
 * own initial factors (W0: n_problems x k x m, H0: n_problems x k x n, internal layout as nbmf_set_factors), the
 * other hyper-parameters (eps, projection) as set: the loops of the reference's experiment driver -- the 36-point
 * (alpha, beta) grids and the K sweeps of examples/reproduce_magron2022.py:75-340 over train_nbmf_mm (:49-73) -- and
 * the n_init restarts of README.md:144.  Outputs per problem: losses (row p of an n_problems x max_iter array, the
 * first n_iter[p] entries), n_iter[p], final factors (W_out, H_out, shaped like the inputs).
 * Small problems (the reference's datasets: 50 x 85 ... 1226 x 285) run as many at a time as the chip holds, in ONE
 * persistent launch per group -- each fit keeps its CUs, its own barrier words and stops on its own; larger ones run
 * one after the other.  Either way problem p's results are bit for bit those of nbmf_set_hyper(alpha[p], beta[p]) +
 * nbmf_set_factors + nbmf_run + nbmf_get_factors.  The context's own factors are left as they were when the
 * single-launch path served the batch, and hold the last problem's otherwise. */
int nbmf_run_batch(nbmf_ctx* ctx, int n_problems, const double* alpha, const double* beta, const double* W0, const double* H0,
                   int max_iter, double tol, double* losses, int* n_iter, double* W_out, double* H_out);
/* Diagnostics: persistent launches nbmf_run_batch made on this context and the problems they served. */
int nbmf_batch_stats(nbmf_ctx* ctx, int* launches, int* problems);
/* Diagnostics: how the two sweeps of an iteration are cut (valid after an upload / generate): chunks of the H-pass and of
 * the W-pass and the row blocks (16 rows of the swept image) per chunk; a sweep launches (column strips / 4) x chunks
 * workgroups.  Any pointer may be NULL. */
int nbmf_sweep_info(nbmf_ctx* ctx, int* h_chunks, int* h_blocks_per_chunk, int* w_chunks, int* w_blocks_per_chunk);
/* Diagnostics, process-wide: sweeps launched in the two-state W variant (binary data observed everywhere, no pad rows in the
 * swept dimension: the bracket of _solver.py:53 with two states per entry instead of three) and in the ragged-K variant
 * (fewer components than the layout holds), and runs that RESUMED after a sweep could not assemble the previous iteration's
 * loss (_solver.py:148-162) within its bound -- a GPU shared with a tenant that saturates it -- and went on with the loss
 * in a launch of its own.  Tests use it to make sure the variant they mean to test is the one that ran.
 * Any pointer may be NULL. */
int nbmf_variant_stats(long long* full_w_launches, long long* ragged_k_launches, long long* loss_assembly_recoveries);

/* Progress reports while nbmf_run works (the `verbose` prints of _solver.py:165-166 need the losses as they
 * arrive, not after the run): with a callback set, nbmf_run synchronises after every `every` iterations and
 * hands over the losses that have become final since the last report -- iterations [first, first+count),
 * `losses` pointing at the first of them.  The loss of iteration t is settled by the sweep of iteration t+1
 * (SURVEY N3), so reports trail the device by one iteration; the values are those nbmf_run returns.
 * fn == NULL (the default) switches reporting off: no intermediate synchronisation. */
typedef void (*nbmf_progress_fn)(void* user, int first, int count, const double* losses);
int nbmf_set_progress(nbmf_ctx* ctx, nbmf_progress_fn fn, void* user, int every);

/* Diagnostics: how many nbmf_run calls of this context were served by the single-launch path for small problems
 * (one persistent kernel runs the whole loop of _solver.py:143-175), and how many of those gave
 * up at a grid barrier and were redone by the five-kernel path.  Environment: NBMF_PERSISTENT=0 switches the
 * single-launch path off. */
int nbmf_small_stats(nbmf_ctx* ctx, int* runs, int* aborted);

/* Diagnostics, process-wide: fits (nbmf_run calls and problems of nbmf_run_batch) the single-launch engine has served to
 * the end, persistent launches that gave up (their fits were redone by the launches), and nbmf_run calls the
 * launch-per-kernel engine has served.  The GPU tests that run every case once per engine read them to make sure the
 * engine they name is the one that ran (a persistent kernel that silently gave up would otherwise pass as the other).
 * Any pointer may be NULL. */
int nbmf_engine_stats(long long* persistent_served, long long* persistent_aborted, long long* launches_served);

/* n_steps repetitions of the simplex-factor update with the Beta factor frozen: the loop body of
 * NBMFMM.transform, _base.py:178-193 (always "normalize", eps as set by nbmf_set_hyper). */
int nbmf_w_only_steps(nbmf_ctx* ctx, int n_steps);

/* Loss of the current factors, _solver.py:148-162. */
int nbmf_loss(nbmf_ctx* ctx, double* loss);

/* Sum over entries of Ym*log(Theta+eps) + (1-Ym)*log(1-Theta+eps) for the current factors (summed over
 * ranks when a communicator is attached): the numerator of NBMFMM.score, _base.py:239-247 (divide by
 * nbmf_get_n_obs), and the data term of the loss, _solver.py:150-154.  clip_theta != 0 clips Theta to [0, 1]
 * first, as NBMFMM.inverse_transform does (_base.py:210) before score evaluates it. */
int nbmf_loglik(nbmf_ctx* ctx, int clip_theta, double* loglik);

/* Strictly masked variant: sum over OBSERVED entries only of mask*(Y log(Theta+eps) + (1-Y) log(1-Theta+eps)),
 * the held-out log-likelihood of examples/reproduce_magron2022.py:40-47 (compute_perplexity: divide by
 * nbmf_get_n_obs, negate, exponentiate).  A Theta-only sweep (no back-products). */
int nbmf_loglik_strict(nbmf_ctx* ctx, double* loglik);

/* Theta at `count` index pairs of the internal m x n matrix, for the factors the context holds
 * (after nbmf_set_factors or a run): out[t] = Theta[rows[t], cols[t]], clipped to [0, 1] first if
 * clip_theta != 0 (NBMFMM.inverse_transform, _base.py:201-210).  Needs factors, not data; NBMF_ERR_STATE while a
 * communicator is attached (detach first).  Every pair is checked on the device before it is used: one outside
 * [0, m) x [0, n) gives NBMF_ERR_ARG with the lowest offending position in the message (what `out` holds is unspecified
 * then), and the context stays usable.  Runs in chunks of NBMF_PREDICT_PAIRS pairs (environment; default 1 << 22); the value
 * at a pair depends on the pair and the factors only.  Synchronises the context's stream before it returns. */
int nbmf_predict_at(nbmf_ctx* ctx, const int64_t* rows, const int64_t* cols, int64_t count,
                    int clip_theta, double* out);

/* Theta for rows [row0, row0 + nrows) and all n columns.
 * NBMF_PREDICT_F64: float64, `out` row-major with leading dimension ldout (elements, >= n).
 * NBMF_PREDICT_U8:  one byte per entry, 1 where theta > threshold (strictly; theta after the clip
 *                   if clip_theta), else 0; ldout in bytes.  Columns n .. ldout-1 of `out` are not written.
 * Runs in panels of NBMF_PREDICT_PANEL_ROWS rows (environment; default: the multiple of 16 that keeps a panel at or under
 * 256 MiB); an entry's value does not depend on the panels.  Same state rules and synchronisation as above. */
#define NBMF_PREDICT_F64 0
#define NBMF_PREDICT_U8 1
int nbmf_predict_rows(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int clip_theta, int out_kind,
                      double threshold, void* out, int64_t ldout);

/* A yes / no decision per entry of Theta for rows [row0, row0 + nrows) and all n columns, returned as bits: entry j of row
 * i is bit 7 - j % 8 of out[(i - row0) * ldout + j / 8] (np.packbits(..., axis=1); the layout of NBMF_DATA_BITS, so the result
 * is an operand of every call that takes bits).  theta[i, j] is bit for bit the entry nbmf_predict_rows(..., clip_theta,
 * NBMF_PREDICT_F64, ...) returns, and the decision is
 * NBMF_BITS_THRESHOLD: theta > threshold, strictly: the bits of nbmf_predict_rows' NBMF_PREDICT_U8 bytes; `seed` is ignored.
 * NBMF_BITS_SAMPLE:    u < theta: one draw of X ~ Bernoulli(Theta), with the counter-based uniform of nbmf_generate at
 *                      row0 = col0 = 0: u = (splitmix64(seed * 0x100000001B3 + i * n + j) >> 11) * 2^-53, in [0, 1), the
 *                      arithmetic modulo 2^64.  theta = 0 never draws a one and theta >= 1 always does; `threshold` is
 *                      ignored.  The host can regenerate any u (nbmf_mm_amd._hip.hash_uniform does).
 * A NaN theta decides 0 in both modes.  Exactly ceil(n / 8) bytes of each output row are written, whatever ldout (bytes,
 * >= ceil(n / 8)) is, and the pad bits of a row's last byte are written as zeros.  A row's bits depend on the factors, the
 * mode's argument and its own row and column numbers only: not on row0, on the panels (NBMF_PREDICT_PANEL_ROWS, as above;
 * a panel row stages nA / 8 bytes) or on other rows; the same call twice gives the same bytes.  NBMF_ERR_ARG for an unknown
 * mode, a NaN threshold in threshold mode, ldout < ceil(n / 8), rows outside [0, m), or a NULL out with nrows > 0;
 * nrows == 0 touches nothing.  Same state rules and synchronisation as nbmf_predict_rows. */
#define NBMF_BITS_THRESHOLD 0
#define NBMF_BITS_SAMPLE 1
int nbmf_theta_bits(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int clip_theta, int mode,
                    double threshold, uint64_t seed, uint8_t* out, int64_t ldout);

/* The `top` columns with the largest Theta in each of the rows [row0, row0 + nrows), ranked on the device: for every
 * row i and slot s < top, out_cols[(i - row0) * ldout + s] is the s-th column in the order "Theta descending (compared
 * numerically), ties by ascending column" over the ELIGIBLE columns of the row, and out_scores (may be NULL) its Theta.
 * A column j in [0, n) is eligible unless exclude[(i - row0) * ldx + j] != 0 (exclude may be NULL: nothing is skipped;
 * otherwise nrows x n bytes, ldx >= n, nothing beyond column n - 1 is read) or Theta[i, j] is NaN.  Theta[i, j] is bit
 * for bit the entry nbmf_predict_rows(..., clip_theta, NBMF_PREDICT_F64, ...) returns.  A row with fewer than `top`
 * eligible columns (top > n is allowed) ends in column -1 / score NaN.  Nothing outside slots [0, top) of an output row
 * is written (ldout >= top, in elements).  The result of a row depends on that row, the factors and its exclude bytes
 * only: not on row0, on the panels (NBMF_PREDICT_PANEL_ROWS, as above) or on other rows; the same call twice gives
 * the same bits.  NBMF_ERR_ARG for top outside [1, NBMF_TOP_N_MAX], rows outside [0, m), ldout < top, ldx < n with an
 * exclude, or a NULL out_cols with nrows > 0; nrows == 0 touches nothing.  Same state rules and synchronisation as above. */
#define NBMF_TOP_N_MAX 256
int nbmf_top_n(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int top, int clip_theta,
               const uint8_t* exclude, int64_t ldx, int64_t* out_cols, double* out_scores, int64_t ldout);
/* The same with the exclude matrix in the given form: NBMF_DATA_U8 (nbmf_top_n) or NBMF_DATA_BITS (bit-packed as under
 * nbmf_upload_v, ldx in bytes and >= ceil(n / 8), a set bit = skipped; unpacked on the device into the panel the bytes are
 * copied into: the same result bit for bit).  NBMF_ERR_ARG for any other exclude_kind. */
int nbmf_top_n_v(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int top, int clip_theta,
                 const void* exclude, int exclude_kind, int64_t ldx, int64_t* out_cols, double* out_scores, int64_t ldout);

/* The Bernoulli log-likelihood of Theta against data, per row and per column, for the rows [row0, row0 + nrows).
 * theta[i, j] is bit for bit the entry nbmf_predict_rows(..., clip_theta, NBMF_PREDICT_F64, ...) returns.  An entry is
 * OBSERVED if mask is NULL or mask[(i - row0) * ldmask + j] != 0; its term is
 *   x_kind NBMF_DATA_U8  (one byte per entry, nonzero means x = 1):  t = log(x ? theta + eps : (1 - theta) + eps)
 *   x_kind NBMF_DATA_F64 (x in [0, 1]):                              t = x log(theta + eps) + (1 - x) log((1 - theta) + eps)
 * with the logarithm's argument formed in exactly that order and the products and the sum of the second form rounded one
 * by one (what NumPy computes from nbmf_predict_rows' theta), and the device library's log.  Unobserved entries contribute
 * nothing.  row_ll[i - row0] is the sum of t over row i's observed entries and row_obs[i - row0] their count; col_ll[j] and
 * col_obs[j] the same for column j over the call's rows.  This is the strict, observed-only sum of nbmf_loglik_strict and
 * of examples/reproduce_magron2022.py's compute_perplexity, broken down; without a mask it is also the summand of
 * NBMFMM.score (nbmf_loglik with clip_theta).  x and mask are nrows x n, row-major with leading dimensions ldx (elements)
 * and ldmask (bytes), both >= n; nothing beyond column n - 1 is read.  Any of the four outputs may be NULL (not all):
 * row outputs hold nrows entries, column outputs n.
 * A row's result depends on that row, the factors, its data and its mask bytes only -- not on row0, on the panels or on
 * other rows; a column's result depends on (row0, nrows), the factors and the data only, not on the panels; the same call
 * twice gives the same bits (fixed summation orders, integer counts, no floating-point atomics).  Runs in panels like
 * nbmf_predict_rows (NBMF_PREDICT_PANEL_ROWS, rounded up to a multiple of 16 here; panels after the first start on a
 * multiple of 16 of the absolute row index).  NBMF_ERR_ARG for rows outside [0, m), an unknown x_kind, ldx < n, ldmask < n
 * with a mask, a NaN or negative eps, all four outputs NULL, or a NULL x with nrows > 0; nrows == 0 reads nothing, leaves
 * the row outputs alone and zero-fills the column outputs.  Same state rules and synchronisation as nbmf_predict_rows. */
int nbmf_score_rows(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int clip_theta, double eps,
                    const void* x, int x_kind /* NBMF_DATA_U8 | NBMF_DATA_F64 */, int64_t ldx,
                    const uint8_t* mask /* NULL: all observed; nonzero = observed */, int64_t ldmask,
                    double* row_ll, int64_t* row_obs,   /* nrows each, either may be NULL */
                    double* col_ll, int64_t* col_obs);  /* n each, either may be NULL */
/* The same with a kind for the mask as well, and bit-packed operands: x_kind may also be NBMF_DATA_BITS (the term of
 * NBMF_DATA_U8), mask_kind is NBMF_MASK_NONE (mask is ignored), NBMF_MASK_U8 or NBMF_MASK_BITS.  Packed operands are laid
 * out as under nbmf_upload_v, their leading dimension in bytes and >= ceil(n / 8); they are unpacked on the device into
 * the panels the bytes are copied into, so every sum and count is bit for bit that of the uint8 operands of the same
 * values.  NBMF_ERR_ARG also for an unknown mask_kind and for a NULL mask with mask_kind set. */
int nbmf_score_rows_v(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int clip_theta, double eps,
                      const void* x, int x_kind /* NBMF_DATA_U8 | NBMF_DATA_F64 | NBMF_DATA_BITS */, int64_t ldx,
                      const void* mask, int mask_kind /* NBMF_MASK_NONE | NBMF_MASK_U8 | NBMF_MASK_BITS */, int64_t ldmask,
                      double* row_ll, int64_t* row_obs, double* col_ll, int64_t* col_obs);

/* The observed zeros and the observed ones of the rows [row0, row0 + nrows) of the data, counted by the Theta they got: the
 * two integer histograms that ROC AUC and a calibration curve are functions of.  theta[i, j] is bit for bit the entry
 * nbmf_predict_rows(..., clip_theta = 1, NBMF_PREDICT_F64, ...) returns: the clip to [0, 1] is always on.  An entry is
 * OBSERVED if mask is NULL or mask[(i - row0) * ldmask + j] != 0; its class is c = (x[(i - row0) * ldx + j] != 0), and with
 *   p = theta * bins   (one rounded double multiplication),   b = (long long)p,   b = bins - 1 where b >= bins
 * it adds 1 to hist[c * bins + b]: bin b holds the thetas in [b / bins, (b + 1) / bins) -- a theta exactly on an edge
 * belongs to the upper bin -- and the last bin holds theta = 1 as well.  A NaN theta is in neither histogram: it adds 1 to
 * nan_count[c] (nan_count may be NULL).  Unobserved entries count nowhere, so hist sums to the observed entries less the NaN
 * ones.  x and mask are nrows x n bytes, row-major with leading dimensions ldx and ldmask, both >= n; nothing beyond column
 * n - 1 is read.  The counts are exact integers: they do not depend on row0's alignment, on the panels (NBMF_PREDICT_PANEL_ROWS,
 * as nbmf_predict_rows) or on the order the device adds them in, and the same call twice gives the same arrays (integer
 * adds only, no floating-point atomics); the counts of two disjoint row ranges add up to those of their union.
 * NBMF_ERR_ARG for rows outside [0, m), bins outside [1, NBMF_HIST_MAX_BINS], ldx < n, ldmask < n with a mask, a NULL hist,
 * or a NULL x with nrows > 0 -- no output is touched then; nrows == 0 reads nothing and zero-fills the outputs.  Same state
 * rules and synchronisation as nbmf_predict_rows. */
#define NBMF_HIST_MAX_BINS 1024
int nbmf_theta_hist(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int bins,
                    const uint8_t* x, int64_t ldx,
                    const uint8_t* mask /* NULL: all observed; nonzero = observed */, int64_t ldmask,
                    int64_t* hist /* [2][bins]: class 0 first */, int64_t* nan_count /* [2], may be NULL */);
/* The same with kinds: x_kind NBMF_DATA_U8 or NBMF_DATA_BITS, mask_kind NBMF_MASK_NONE, NBMF_MASK_U8 or NBMF_MASK_BITS, packed
 * operands as for nbmf_score_rows_v (leading dimension in bytes, >= ceil(n / 8)): the same counts. */
int nbmf_theta_hist_v(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int bins,
                      const void* x, int x_kind, int64_t ldx, const void* mask, int mask_kind, int64_t ldmask,
                      int64_t* hist, int64_t* nan_count);

/* Expected counts: the observed entries of the rows [row0, row0 + nrows) of the data, summed by (row, column group) and by
 * column into the five integers that the expected count of ones under the model, its variance, the z-score of the observed
 * count, the Brier score and Tjur's coefficient of discrimination are functions of.  theta[i, j] is bit for bit the entry
 * nbmf_predict_rows(..., clip_theta = 1, NBMF_PREDICT_F64, ...) returns: the clip is always on, as in nbmf_theta_hist.  With
 * Q = 2^NBMF_MOMENT_FRAC_BITS,
 *   q1 = (int64) rint(theta * Q)             (the product is exact; rint rounds half to even)
 *   q2 = (int64) rint((theta * theta) * Q)   (one rounded product, scaled exactly)
 * -- NumPy: np.rint(theta * 2.0**32).astype(np.int64), np.rint((theta * theta) * 2.0**32).astype(np.int64).  An entry is
 * OBSERVED as in nbmf_theta_hist (mask_kind NBMF_MASK_NONE, or its mask byte or bit nonzero).  An observed entry whose theta
 * is not NaN adds to its slot
 *   field 0  N_OBS    1                  field 2  S1       q1
 *   field 1  N_ONES   x != 0             field 3  S2       q2                field 4  S1_ONES   x != 0 ? q1 : 0
 * one whose theta is NaN adds 1 to nan_count[x != 0] (may be NULL) and nothing else.  The slots:
 *   row_tab[((i - row0) * groups + g) * 5 + field]   g = col_group[j], where that is not -1 ("in no group"; col_group NULL:
 *                                                    every column is in group 0); may be NULL
 *   col_tab[j * 5 + field]                           over the call's rows, whatever column j's group; may be NULL (not both)
 * So S1 / Q is the expected number of ones among a slot's observed entries, (S1 - S2) / Q its variance, N_ONES what was seen.
 * x, mask, their kinds and leading dimensions are those of nbmf_theta_hist_v (x_kind NBMF_DATA_U8 or NBMF_DATA_BITS, mask_kind
 * NBMF_MASK_NONE, NBMF_MASK_U8 or NBMF_MASK_BITS; nothing beyond column n - 1 is read; bits and bytes give identical arrays).
 * Every sum is an exact integer: it does not depend on row0's alignment, on the panels (NBMF_PREDICT_PANEL_ROWS, as
 * nbmf_predict_rows), on NBMF_MOMENT_COPIES (the copies of the column table the device spreads its adds over; default 32) or
 * on the order the device adds in -- integer adds only, no floating-point atomics --; the same call twice gives the same
 * arrays, and col_tab and nan_count of disjoint row ranges add up to those of their union.  A slot sums at most
 * max(n, nrows) entries of at most Q each: nrows is at most 2^30 here and n is below 2^24 (what the product kernels launch),
 * so no sum reaches 2^63.
 * NBMF_ERR_ARG, with no output touched, for rows outside [0, m), nrows above 2^30, groups outside
 * [1, NBMF_MOMENT_MAX_GROUPS], a label outside [-1, groups) (checked on the host before anything is launched), an unknown
 * x_kind or mask_kind, a NULL mask with mask_kind set, a bad leading dimension, both tables NULL, or a NULL x with nrows > 0.
 * nrows == 0 reads nothing and zero-fills col_tab and nan_count.  Same state rules and synchronisation as nbmf_predict_rows. */
#define NBMF_MOMENT_MAX_GROUPS 16
#define NBMF_MOMENT_FRAC_BITS 32
#define NBMF_MOMENT_FIELDS 5   /* N_OBS, N_ONES, S1, S2, S1_ONES */
int nbmf_moment_rows_v(nbmf_ctx* ctx, int64_t row0, int64_t nrows,
                       const void* x, int x_kind, int64_t ldx,          /* NBMF_DATA_U8 | NBMF_DATA_BITS */
                       const void* mask, int mask_kind, int64_t ldmask, /* NONE | U8 | BITS */
                       const int32_t* col_group /* n labels in [-1, groups); NULL: every column in group 0 */, int groups,
                       int64_t* row_tab /* [nrows][groups][5], may be NULL */,
                       int64_t* col_tab /* [n][5], may be NULL (not both) */,
                       int64_t* nan_count /* [2], may be NULL */);

/* The best entries of Theta over the whole row range [row0, row0 + nrows), as ONE list of (row, column) pairs ranked on the
 * device: the global question nbmf_top_n (per row, at most NBMF_TOP_N_MAX slots) cannot answer.  theta[i, j] is bit for bit
 * the entry nbmf_predict_rows(..., clip_theta, NBMF_PREDICT_F64, ...) returns.  Two kinds of request:
 *   NBMF_PAIRS_THETA       score s = theta, best is LARGEST.  x is the exclude matrix (may be NULL: nothing is skipped): an
 *                          entry is eligible unless its exclude byte or bit is nonzero.  Takes no mask.
 *   NBMF_PAIRS_LIKELIHOOD  score s = theta where x != 0, else 1.0 - theta (one rounded subtraction): the probability the
 *                          model gave to what was observed.  Best is SMALLEST.  x is the data; an entry is eligible where
 *                          it is observed: mask nonzero, or mask_kind NBMF_MASK_NONE.
 * In both kinds an entry whose score is NaN is never eligible, and columns >= n and rows outside the request do not exist.
 * The result is the first `top` eligible entries in the order "score, best first, compared numerically (-0.0 equals +0.0),
 * then ascending row, then ascending column": out_rows[s] (absolute row numbers), out_cols[s] and out_scores[s] (may be
 * NULL; a score keeps its own bits, so a returned -0.0 is -0.0) for s < *out_count = min(top, eligible entries).  Slots at
 * or beyond *out_count are not written; each array holds `top` entries.
 * x_kind is NBMF_DATA_U8 (one byte per entry) or NBMF_DATA_BITS, mask_kind NBMF_MASK_NONE, NBMF_MASK_U8 or NBMF_MASK_BITS;
 * operands are nrows x n with the leading-dimension rules of nbmf_theta_hist_v (bytes: >= n; packed: in bytes, >=
 * ceil(n / 8)), nothing beyond column n - 1 is read, and packed operands are unpacked on the device into the staging the
 * bytes are copied into: bits and bytes give identical results.  The operands go to the device once and stay there for
 * the whole call (nrows x round_up(n, 4) bytes each, plus packed rows as they came, plus 24 bytes per candidate slot:
 * top + max(65536, top / 8) of them, at least one row's worth; NBMF_PAIRS_SLACK in the environment sets the slack in
 * entries, 0 forcing the selection through every digit and the tie pass -- the result is the same): a request that does not fit fails with NBMF_ERR_HIP and a message that says so --
 * ask for fewer rows per call and merge.  No Theta panel is stored.
 * The result depends on the factors, the operands and (row0, nrows, top) only -- not on how the work is blocked, on
 * NBMF_HIST_COPIES (the copies of the digit counters, as nbmf_theta_hist), on NBMF_PAIRS_SLACK or on the order workgroups arrive in (integer
 * adds only, no floating-point atomics; the candidates are sorted by (score, row, column) before they are returned) -- and
 * the same call twice gives the same arrays.  So the call on a row range equals the merge of the calls on two ranges that
 * partition it.
 * NBMF_ERR_ARG, with nothing written, for top outside [1, NBMF_TOP_PAIRS_MAX], rows outside [0, m), an unknown kind, x_kind
 * or mask_kind, a bad leading dimension, a mask given to NBMF_PAIRS_THETA, a NULL mask with mask_kind set, a NULL out_rows,
 * out_cols or out_count, or a NULL x in the likelihood kind with nrows > 0.  nrows == 0 sets *out_count = 0 and reads
 * nothing.  Same state rules and synchronisation as nbmf_predict_rows. */
#define NBMF_TOP_PAIRS_MAX (1 << 22)
#define NBMF_PAIRS_THETA 0
#define NBMF_PAIRS_LIKELIHOOD 1
int nbmf_top_pairs(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int64_t top, int clip_theta, int kind,
                   const void* x, int x_kind, int64_t ldx,            /* THETA: the exclude matrix (may be NULL); LIKELIHOOD: the data */
                   const void* mask, int mask_kind, int64_t ldmask,   /* LIKELIHOOD only; NBMF_MASK_NONE: all observed */
                   int64_t* out_rows, int64_t* out_cols, double* out_scores, int64_t* out_count);

/* Where given entries of Theta stand in the order nbmf_top_n ranks their row by: the position of held-out (row, column)
 * entries among all n columns, at any depth, with a few integers per entry leaving the device instead of the row.  The
 * TARGETS of row row0 + r are the columns indices[indptr[r] .. indptr[r + 1]) -- a CSR slice; indptr[0] may be greater than
 * 0, so nrows + 1 entries of a larger CSR's indptr can be passed with its whole indices.  Targets of a row may come in any
 * order and may repeat; each is answered on its own.  With theta[j] bit for bit the entry nbmf_predict_rows(..., clip_theta,
 * NBMF_PREDICT_F64, ...) returns, a column j' is ELIGIBLE if theta[j'] is not NaN and it is not excluded (exclude as in
 * nbmf_top_n: nrows x n bytes, leading dimension ldx >= n, nonzero = skipped, nothing beyond column n - 1 read), and
 *   out_eligible[r] = the eligible columns of the row
 * and for a target j at position p of indices that is eligible, over the eligible columns j' and comparing numerically
 * (-0.0 equals +0.0),
 *   out_above[p] = #{j' : theta[j'] > theta[j]},     out_tied[p] = #{j' != j : theta[j'] == theta[j]},
 *   out_rank[p]  = out_above[p] + #{j' < j : theta[j'] == theta[j]},     out_scores[p] = theta[j]:
 * out_rank is 0-based and is the slot nbmf_top_n puts column j in (the same order, tie rule and eligibility), for any
 * depth, not only below NBMF_TOP_N_MAX.  A target that is itself excluded or NaN gets rank = above = tied = -1 and its
 * theta as the score (NaN stays NaN; an excluded target still reports its theta).  The four per-target outputs are indexed
 * like indices; positions outside [indptr[0], indptr[nrows]) are neither read nor written.  Any output may be NULL, not
 * all five.  A row's results depend on that row, the factors, its exclude bytes and its targets only -- not on row0, on the
 * panels (NBMF_PREDICT_PANEL_ROWS, as nbmf_predict_rows) or on other rows -- and the same call twice gives the same bits:
 * the counts are integers (integer adds only, no floating-point atomics).  The cost of a row is ceil(targets / 8) passes
 * over its n columns.  NBMF_ERR_ARG for rows outside [0, m), a NULL indptr, indptr[0] < 0 or a decreasing indptr, a NULL
 * indices with targets present, a target column outside [0, n) (the message names the lowest offending position; indptr
 * and the columns are checked on the host), ldx < n with an exclude, or all outputs NULL -- before anything is launched,
 * and no output is touched then; nrows == 0 touches nothing.  Same state rules and synchronisation as nbmf_top_n. */
int nbmf_rank_rows(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int clip_theta,
                   const int64_t* indptr /* nrows + 1 */, const int32_t* indices,
                   const uint8_t* exclude /* may be NULL */, int64_t ldx,
                   int64_t* out_rank, int64_t* out_above, int64_t* out_tied, double* out_scores,
                   int64_t* out_eligible /* nrows */);
/* The same with the exclude matrix in the given form, as nbmf_top_n_v: NBMF_DATA_U8 or NBMF_DATA_BITS. */
int nbmf_rank_rows_v(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int clip_theta,
                     const int64_t* indptr, const int32_t* indices,
                     const void* exclude, int exclude_kind, int64_t ldx,
                     int64_t* out_rank, int64_t* out_above, int64_t* out_tied, double* out_scores,
                     int64_t* out_eligible);

/* Similarity within one side of the matrix: the factors read as an embedding.  The ITEMS of axis 0 are the m samples, whose
 * vectors are the columns of W (k x m); the items of axis 1 are the n features, whose vectors are the columns of H (k x n).
 * L is m or n accordingly, F the axis's factor and C the other one.  The score s(a, b) of items a and b, in float64:
 *   NBMF_SIM_DOT      s = sum_k F[k, a] F[k, b]
 *   NBMF_SIM_COSINE   s = u_a . u_b with u_a = F[:, a] / ||F[:, a]||_2; a zero vector has u = 0: its score with everything
 *                     is 0, not NaN
 *   NBMF_SIM_PROFILE  the cosine between the PREDICTED PROFILES of a and b -- the unclipped row of Theta of a sample, the
 *                     column of Theta of a feature -- reduced to factor space: with G = C C^T (k x k),
 *                     s = f_a^T G f_b / sqrt((f_a^T G f_a)(f_b^T G f_b)); an item with f^T G f = 0 scores 0 with everything.
 *                     Two correlated components are not treated as unrelated by this one.
 * `query` holds nq item indices in [0, L), in any order, repeats allowed; NULL means the items 0 .. nq - 1 (nq <= L then).
 * nbmf_similarity writes s(query[t], b) for every item b to out[t * ldout + b] (ldout >= L; nothing beyond column L - 1 of a
 * row is written).  An entry depends on its two items, the factors, axis and metric only -- not on the panels
 * (NBMF_PREDICT_PANEL_ROWS, as nbmf_predict_rows; a panel row stages L doubles) or on the other queries -- and the same call
 * twice gives the same bits (ordered sums, no floating-point atomics).  DOT and COSINE are bitwise symmetric:
 * s(a, b) == s(b, a).  NBMF_ERR_ARG for an unknown axis or metric, nq < 0, nq > L with a NULL query, a query index outside
 * [0, L) (the message names the lowest offending position; checked on the host before anything is launched), ldout < L,
 * or a NULL out with nq > 0; nq == 0 touches nothing.  Same state rules and synchronisation as nbmf_predict_rows. */
#define NBMF_SIM_DOT 0
#define NBMF_SIM_COSINE 1
#define NBMF_SIM_PROFILE 2
int nbmf_similarity(nbmf_ctx* ctx, int axis, int metric, const int64_t* query, int64_t nq, double* out, int64_t ldout);
/* The `top` items most similar to each query item, ranked on the device: nbmf_top_n's contract with "column" read as item
 * and no clip.  For every query position t and slot s < top, out_idx[t * ldout + s] is the s-th item in the order "score
 * descending (compared numerically), ties by ascending index" over the ELIGIBLE items of row t, and out_scores (may be
 * NULL) its score, bit for bit the entry nbmf_similarity returns for the same (query, item).  An item is eligible unless
 * its score is NaN or, with skip_self != 0, it IS query[t] -- by index: a different item with an identical vector stays
 * eligible and ties by ascending index.  A row with fewer than `top` eligible items (top > L is allowed) ends in index
 * -1 / score NaN; nothing outside slots [0, top) of an output row is written (ldout >= top, in elements).  A row's result
 * depends on its query index, the factors, axis and metric only.  NBMF_ERR_ARG as nbmf_similarity, and for top outside
 * [1, NBMF_TOP_N_MAX], ldout < top, or a NULL out_idx with nq > 0. */
int nbmf_neighbors(nbmf_ctx* ctx, int axis, int metric, const int64_t* query, int64_t nq, int top, int skip_self,
                   int64_t* out_idx, double* out_scores, int64_t ldout);

/* Held-out entries kept on the device, and their Bernoulli log-likelihood summed there: the held-out curve of a fit
 * without the factors leaving the device, and early stopping on it.  `count` index pairs of the internal m x n matrix with
 * one byte of truth each (nonzero means x = 1), in any order, repeats allowed; 9 bytes per pair stay resident (rows and
 * columns as int32).  The pairs are checked on the host before anything is kept: one outside [0, m) x [0, n) gives
 * NBMF_ERR_ARG with the lowest offending position in the message, and the context keeps the eval set it had.  count == 0
 * switches evaluation off and frees the arrays.  every >= 1 and patience >= 0 (else NBMF_ERR_ARG) say how nbmf_run uses
 * the set, see below; they do not enter the sum.  NBMF_ERR_STATE while a communicator is attached, and nbmf_comm_init* on
 * a context that holds an eval set returns NBMF_ERR_STATE as well.
 *
 * nbmf_eval_loglik: the sum over the pairs of t = log(x ? theta + eps : (1 - theta) + eps), the argument formed in that
 * order, eps that of nbmf_set_hyper, the device library's log (nbmf_score_rows' term), where theta is bit for bit what
 * nbmf_predict_at(..., clip_theta = 0) returns for the pair.  Summation order: the 32 pairs [32 b, 32 b + 32) make
 * partial b (a fixed tree), and the partials are folded in a fixed order by one workgroup: the value depends on the
 * factors, the pairs in the order given and eps only -- not on every / patience, on when it is computed or on which call
 * computed it -- and the same evaluation twice gives the same bits.  No floating-point atomics.  Needs factors and an eval
 * set, not data (NBMF_ERR_STATE otherwise; state rules of nbmf_predict_at); synchronises before it returns.
 *
 * nbmf_run on a context with an eval set is served by the launch-per-kernel engine (not the single-launch engine, not
 * NBMF_USE_GRAPH) in batches that end on the multiples of `every`; behind each batch the set is evaluated and the host
 * looks at the value at once (a progress callback's reports are delivered at those looks).  An evaluation is labelled
 * with s, the number of MM iterations its factors have had -- the unit of n_iter: s = every, 2 every, ..., and the last
 * label always equals n_iter: where max_iter is no multiple of `every` one more evaluation is made at the end, and where
 * the tol rule ends the run between two multiples the evaluation behind that batch has seen exactly the final factors
 * and is recorded under n_iter.  An evaluation IMPROVES if its sum is strictly greater than the best so far (the first
 * always does); the factor images are then copied device-to-device into a snapshot, with the stream drained and nothing
 * enqueued behind the evaluation.  With patience = p > 0 the run ends at the p-th consecutive evaluation on a multiple
 * of `every` that does not improve: n_iter is that evaluation's s, losses[0 .. s) are final (the last one from the
 * usual Theta-only sweep), the context's factors are those after s iterations.  patience = 0 records the curve and
 * never stops; the losses, the factors and the curve are then bit for bit those of the run without an eval set.
 * nbmf_run_batch on a context with an eval set returns NBMF_ERR_STATE.
 *
 * nbmf_get_eval: what the last nbmf_run recorded -- *n_evals evaluations (all of them, whatever cap is), the first
 * min(cap, *n_evals) labels and sums in iters / logliks, the label of the best one (0 if none) and whether the patience
 * rule ended the run.  Any pointer may be NULL.  nbmf_get_best_factors: the snapshot of the last run as
 * nbmf_get_factors lays factors out (either pointer may be NULL); NBMF_ERR_STATE if the last run made no evaluation. */
int nbmf_set_eval(nbmf_ctx* ctx, const int64_t* rows, const int64_t* cols, const uint8_t* x, int64_t count,
                  int every, int patience);
int nbmf_eval_loglik(nbmf_ctx* ctx, double* loglik);
int nbmf_get_eval(nbmf_ctx* ctx, int cap, int* n_evals, int* iters, double* logliks, int* best_iter, int* stopped_early);
int nbmf_get_best_factors(nbmf_ctx* ctx, double* W_kxm, double* H_kxn);

/* The held-out split drawn on the device: the eval set is taken out of the data the context holds, no mask and no index
 * list crossing from the host, and can be put back so that the next fold of a cross-validation needs no upload.  No
 * reference counterpart (examples/reproduce_magron2022.py:26-38 loads ready-made train / val / test masks from a file).
 * THE RULE.  The entry at row u, column v of the USER's matrix (U x V; the internal matrix, or its transpose when
 * transposed != 0, as under nbmf_upload) has the counter idx = u * V + v and the uniform
 *   unif = (splitmix64((seed * 0x100000001B3 + idx) ^ 0xA0761D6478BD642F) >> 11) * 2^-53,   arithmetic modulo 2^64:
 * the uniform of nbmf_generate / nbmf_theta_bits with a salt of its own, so a split with the seed a sample was drawn with is
 * another draw.  The entry is HELD OUT iff it is observed and lo <= unif < hi (compared as the 53-bit integers: exact).
 * The same (seed, shape of the user's matrix) gives the same split under both orientations, and the intervals
 * [f / k, (f + 1) / k), f = 0 .. k - 1, partition the observed entries.
 * nbmf_hold_out: every held-out entry becomes "valid, unobserved" in both images, and the list of them -- (row, col) in
 * INTERNAL coordinates, truth 1 for an observed one and 0 for an observed zero, in row-major order of the internal matrix
 * with columns ascending (what np.nonzero gives) -- becomes the context's eval set exactly as nbmf_set_eval would have
 * installed it with those pairs, every and patience: nbmf_eval_loglik, the evaluations of nbmf_run, nbmf_get_eval and
 * nbmf_get_best_factors work unchanged, and the sums are bit for bit those of the host route.  A plain eval set that was
 * there is replaced.  The order of the list is fixed (row counts, a 64-bit exclusive prefix sum on the device, positions
 * from ballots and population counts; integers only); *count (may be NULL) receives its length.  The lane masks, the
 * observed counts (nbmf_get_n_obs drops by *count) and the per-row counts are made again as after an upload, so every
 * later call sees the data as if it had been uploaded with the held-out entries masked.  Needs data on the byte-code
 * path (NBMF_FLAG_BINARY_PATH; uploaded or generated), no factors: NBMF_ERR_STATE "hold-out needs binary data with a
 * binary or no mask" otherwise, NBMF_ERR_STATE while a communicator is attached and while a hold-out is in place ("undo
 * it first").  NBMF_ERR_ARG unless 0 <= lo < hi <= 1, every >= 1, patience >= 0; for a split that "holds out no entry" or
 * "leaves no observed entry" -- the context is then exactly as it was, images, counts and any previous eval set: the
 * entries are counted before anything changes --; and beyond the limits of nbmf_set_eval.
 * nbmf_hold_out_undo: every listed entry is observed again with its value, the derived state is made again (data that was
 * observed everywhere runs the two-state W sweep again), and the eval set is released.  NBMF_ERR_STATE without a hold-out.
 * While a hold-out is in place nbmf_set_eval returns NBMF_ERR_STATE, with count == 0 too: the list is the only record of
 * what was cleared.  A new nbmf_upload* / nbmf_generate* makes the context forget that its set came from a hold-out; the
 * list stays, as a plain eval set does across an upload.
 * nbmf_get_eval_pairs: the eval set the context holds, however it got there: *count (0 without one) and the first
 * min(cap, *count) triples as int64 / int64 / uint8 in internal coordinates.  Any output pointer may be NULL. */
int nbmf_hold_out(nbmf_ctx* ctx, uint64_t seed, int transposed, double lo, double hi, int every, int patience, int64_t* count);
int nbmf_hold_out_undo(nbmf_ctx* ctx);
int nbmf_get_eval_pairs(nbmf_ctx* ctx, int64_t cap, int64_t* count, int64_t* rows, int64_t* cols, uint8_t* x);

/* Multi-GPU, one process (and one context) per GPU.  The internal matrix Y is split over the ranks along
 *   shard_axis 0: its ROWS    -> W[:, rows] is local, H is replicated; each iteration all-reduces the k x n
 *                 H-step products [P1 | P2 | loglik] (2*K*N+1 doubles) before the H-update;
 *   shard_axis 1: its COLUMNS -> H[:, cols] is local, W is replicated; each iteration all-reduces the k x m
 *                 W-step bracket (K*M doubles) before the W-update, and [loglik, prior A, prior B] (3 doubles)
 *                 before the stop test.
 * (beta-dir with V split by rows, or dir-beta with V split by columns, is axis 0; the other two
 * combinations are axis 1.)  Rank 0 calls nbmf_comm_unique_id and distributes the 128 bytes; every rank,
 * after nbmf_upload of its shard, calls nbmf_comm_init.  The global observed count (and, for axis 1, the
 * global column count and per-row observed counts) are reduced there.  No reference counterpart (the
 * reference is single-process). */
int nbmf_comm_unique_id(void* id128);
int nbmf_comm_init(nbmf_ctx* ctx, const void* id128, int nranks, int rank, int shard_axis);

/* Same sharded run with the all-reduce done by the caller on a host buffer (sum over ranks, in place,
 * return 0 on success).  Used by the tests (two ranks sharing one GPU, gloo) and as a fallback
 * transport; the device work and the control flow are identical to the RCCL path. */
typedef int (*nbmf_host_allreduce_fn)(void* user, double* buf, int64_t count);
int nbmf_comm_init_host(nbmf_ctx* ctx, nbmf_host_allreduce_fn fn, void* user, int nranks, int rank, int shard_axis);

/* Peer transport: the same exchanges done by the library's own kernels straight over xGMI (each rank maps
 * every other rank's exchange arena through HIP IPC).  Axis 0 fuses the H-update into a reduce-scatter: each
 * rank sums its 1/R column slice of [P1 | P2] in rank order, updates that slice of H and stores it into every
 * rank's arena, so K*N instead of 2*K*N doubles travel back and the update is not repeated R times; axis 1
 * all-reduces the W-step bracket in place (two-shot).  Sums are in rank order -> bitwise reproducible and
 * identical on all ranks.  Every wait is bounded (NBMF_PEER_TIMEOUT_MS, default 30000): a stalled job ends
 * with NBMF_ERR_COMM, never with a hung GPU.
 *   1. every rank: nbmf_peer_export(ctx, shard_axis, handle)   -> NBMF_PEER_HANDLE_BYTES opaque bytes
 *   2. all-gather the handle blocks in rank order (any host channel)
 *   3. every rank: nbmf_comm_init_peer(ctx, all_handles, nranks, rank, shard_axis)
 *      (maps the arenas, runs a known-answer exchange, reduces the global counts; on failure the context is
 *       left unattached so the caller can fall back to nbmf_comm_init)
 * One process per rank, or several ranks (contexts, one host thread each) in one process: a handle block also
 * names the exporting process and the arena's address there, and a rank of the same process uses the memory
 * directly (HIP IPC does not map a handle inside the process that exported it; across devices of one process peer
 * access is enabled instead).  At most 16 ranks.  No reference counterpart. */
#define NBMF_PEER_HANDLE_BYTES 192
int nbmf_peer_export(nbmf_ctx* ctx, int shard_axis, void* handle);
int nbmf_comm_init_peer(nbmf_ctx* ctx, const void* handles, int nranks, int rank, int shard_axis);

/* Row split (shard_axis 0) only: cut the per-iteration exchange into `panels` column panels (1 or 2).  With 2, the
 * second panel's exchange travels on a side stream while the first panel's H-update is applied and the W-pass
 * starts on the chunks that read only those columns.  0 = the default (1 panel, or 2 if the
 * environment says NBMF_OVERLAP=1).  Takes effect at the next nbmf_comm_init*; every rank must choose the same. */
int nbmf_set_exchange_panels(nbmf_ctx* ctx, int panels);

/* Bound on every wait of the peer transport attached NEXT (milliseconds; 0 = the default: NBMF_PEER_TIMEOUT_MS from
 * the environment, else 30000).  A caller that is only probing a transport (bench.py times each candidate over a few
 * iterations before the run) sets a short bound for the probe and the default for the run, so that a transport which
 * cannot work on this machine costs seconds, not a timeout per exchange. */
int nbmf_set_peer_timeout_ms(nbmf_ctx* ctx, double ms);

/* Cancel from another thread (the ONLY call that may be made on a context while its owner thread is inside one): sticky;
 * the owner's nbmf_run returns NBMF_ERR_STATE at its next iteration boundary, and what it has already enqueued is cut
 * short on the device by the run's own stop flag (the word the kernels honour after convergence, _solver.py:169-175).
 * The reference's loop is interrupted by KeyboardInterrupt between NumPy calls; this is what a host thread that joins
 * rank threads (NBMF(n_gpus=N)) uses for the same purpose.  The context can only be destroyed afterwards. */
int nbmf_cancel(nbmf_ctx* ctx);

/* Drop the attached communicator (RCCL, host or peer): the context is a single-GPU context over its own
 * shard again and another nbmf_comm_init* may follow.  Collective in effect: every rank must do the same. */
int nbmf_comm_detach(nbmf_ctx* ctx);

/* What the attached transport itself reports (no reference counterpart: diagnostics of the sharded loop that replaces
 * _solver.py:143-175 on several GPUs).  kind: 0 none, 1 RCCL, 2 peer, 3 host.  nranks_seen: RCCL -- ncclCommCount of the
 * communicator (-1 if this librccl has no such symbol); peer -- arenas mapped, this rank's included; host -- the nranks
 * it was given.  remote: RCCL -- ncclCommCuDevice (the device RCCL bound the communicator to, -1 if unknown); peer / host
 * -- how many of the other ranks' buffers are reached from outside this context.  Any pointer may be NULL. */
int nbmf_comm_info(nbmf_ctx* ctx, int* kind, int* nranks_seen, int* remote);

/* Measurement: HIP-event timing of the two fused pass kernels on the context's stream.  enable: 0 = off, 1 = every
 * sweep, n > 1 = the sweeps of every n-th iteration of a run (a timed dispatch costs ~2.5 us: at sub-millisecond
 * iterations a sample of the launches keeps the measurement from slowing what it measures). */
int nbmf_timing_enable(nbmf_ctx* ctx, int enable);
/* ms summed over launches since enable, and launch counts; any pointer may be NULL. */
int nbmf_timing_get(nbmf_ctx* ctx, double* hpass_ms, int* hpass_launches, double* wpass_ms, int* wpass_launches);
int nbmf_synchronize(nbmf_ctx* ctx);
/* hipDeviceSynchronize() on `device`: everything queued on that GPU by this process has finished (bench.py
 * brackets its timed region with it). */
int nbmf_device_synchronize(int device);

/* Self-test hook used by the GPU tests: applies one of the pass kernel's scalar device routines to n
 * caller-supplied values (op 0: Newton reciprocal used on the binary path; op 1: the natural logarithm
 * of the general path; op 2: the general path's quotient, evaluated as (1 - 0.75 x) / x; ops 3, 4: the two quotients
 * of an entry from one shared reciprocal, (1 - 0.75 x) / x and 0.75 x / ((1 - (x - 1e-8)) + 1e-8); op 5: 1/x by the
 * binary path's shared reciprocal of four, groups of four consecutive values; op 6: op 1 with the product sweeps' table; op 7: the table-free logarithm of the sweeps' running products) so the host can compare with IEEE 1/x,
 * log(x) and the IEEE quotients (accuracy contracts: tests/test_gpu_parity.py). */
#define NBMF_SELFTEST_RCP 0
#define NBMF_SELFTEST_LOG 1
#define NBMF_SELFTEST_DIV 2
#define NBMF_SELFTEST_DIV_PAIR_A 3
#define NBMF_SELFTEST_DIV_PAIR_B 4
#define NBMF_SELFTEST_RCP_OF_FOUR 5
int nbmf_selftest_unary(int device, int op, int n, const double* x, double* y);
/* Test hook: the kernel that unpacks bit-packed operands, on the caller's arrays.  bits is rows x ceil(n / 8) bytes with
 * leading dimension ldbits (layout: nbmf_upload_v), out is rows x ldout bytes: out goes up whole, the kernel writes the byte
 * 0 or 1 to out[r * ldout + j] for r < rows, j < n, and out comes back whole -- columns n .. ldout - 1 as they were.
 * NBMF_ERR_ARG, before any device call, for a NULL bits or out, a negative size, ldbits < ceil(n / 8) or ldout < n. */
int nbmf_selftest_unpack_bits(int device, const uint8_t* bits, int64_t ldbits, int64_t rows, int64_t n,
                              uint8_t* out, int64_t ldout);

#define NBMF_SELFTEST_LOG_1024 6  /* ... with the 1024-entry table of the product sweeps (series to r^4/4) */
#define NBMF_SELFTEST_LOG_PRODUCT 7  /* log of a sweep's running product: no table, no memory access */

/* Measurement helper with no reference counterpart: the f64 matrix rate of `device` as THIS machine delivers it -- a
 * loop of nothing but v_mfma_f64_16x16x4_f64 (four independent accumulators in VGPRs, two waves on every SIMD), one
 * launch of about target_ms milliseconds after a warm-up.  bench.py prints it beside the datasheet figure
 * (roofline.peak_measured; SURVEY 8d asks for the measured peak of the box that ran the bench).  tflops: 2048 flop per
 * MFMA and wave / time; cycles_per_mfma: SIMD cycles per MFMA at the nominal 2.4 GHz (64 = the datasheet's 78.6 TFLOP/s
 * on 1024 SIMDs); launch_ms: the timed launch.  Any pointer may be NULL. */
int nbmf_selftest_mfma_peak(int device, double target_ms, double* tflops, double* cycles_per_mfma, double* launch_ms);

#ifdef __cplusplus
}
#endif
#endif /* NBMF_HIP_H */
