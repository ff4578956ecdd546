/*
 * nnlm_mi355x.h -- C ABI of libnnlm_mi355x.so: the MI355X (gfx950) implementation of the hot
 * path of the R package linxihui/NNLM (alternating nnmf() loop + single-solve nnlm()).
 *
 * This header is the drop-in boundary.  The reference's FFI for this path is the pair of
 * registered .Call routines `_NNLM_c_nnmf` (17 SEXP args) and `_NNLM_c_nnlm` (9 SEXP args)
 * (reference src/RcppExports.cpp:10-27, :29-54, :56-65; called from R/RcppExports.R:4-10).
 * `nnlm_c_nnmf()` / `nnlm_c_nnlm()` below take exactly those arguments as plain pointers and
 * sizes and return exactly the members of the reference's named result lists
 * (src/nnmf.cpp:211-219, src/nnlm.cpp:49-52).  pkg/src/r_glue.c shows the Rinternals-only
 * .Call stub a maintainer adds on the R side; nnlm_amd/_lib.py is the ctypes binding used here.
 *
 * Conventions (all taken from the reference):
 *   - every matrix is column-major (R / Armadillo), fp64 at the boundary;
 *   - logical masks are `int` arrays (R LGLSXP), non-zero = masked (entry is never updated) -- NA_LOGICAL (INT_MIN) included:
 *     the reference converts the matrix to arma::umat and tests `mask(k) > 0` (src/RcppExports.cpp:38-39, src/base_algorithms.cpp:21);
 *   - missing entries of A / y are any non-finite value (NA, NaN, +-Inf), src/nnmf.cpp:65-68;
 *   - method: 1 scd+mse, 2 lee+mse, 3 scd+mkl, 4 lee+mkl (R/misc.R:28-35);
 *   - alpha/beta: [L2, angle, L1] (src/nnmf.cpp:19-20).
 * Inputs are never written.  No exceptions cross this ABI: every function returns NNLM_OK or an
 * error code and leaves a message retrievable with nnlm_last_error().
 */
#ifndef NNLM_MI355X_H
#define NNLM_MI355X_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNLM_ABI_VERSION 1

/* return codes */
#define NNLM_OK 0
#define NNLM_ERR_ARG 1       /* invalid argument (the reference would throw from Armadillo / R stop()) */
#define NNLM_ERR_HIP 2       /* HIP runtime failure (no device, out of memory, launch failure) */
#define NNLM_ERR_INTERRUPT 3 /* the check_interrupt callback asked to stop (Rcpp::checkUserInterrupt) */
#define NNLM_ERR_COMM 4      /* RCCL failure */
#define NNLM_ERR_UNSUPPORTED 5

/* arithmetic modes: what A is stored as in HBM and which MFMA the cross-products run on.
 * Gram matrices, mu = G*x - c, the coordinate sweeps and all reductions are fp64 in both modes. */
#define NNLM_PREC_F32 0 /* A fp32 in HBM (4 bytes per element); the A-streaming cross products take their operands as split-fp16 pairs
                         * (hi + lo * 2^-11: 22 significant bits) on v_mfma_f32_16x16x32_f16, fp32 partial sums flushed into fp64
                         * every 256 elements; KL solvers keep their state in fp32 */
#define NNLM_PREC_F64 1 /* A and GEMM operands fp64, v_mfma_f64_16x16x4_f64 (strict-parity mode; the default of the one-shot entries) */

/*
 * Host callbacks = the R API points the reference touches from its main thread.
 * Any member (or the whole struct pointer) may be NULL.
 */
typedef struct nnlm_callbacks {
    void *ctx;
    int (*check_interrupt)(void *ctx);                        /* src/nnmf.cpp:111; non-zero aborts the run */
    void (*progress)(void *ctx, unsigned done, unsigned total); /* RcppProgress increment, src/nnmf.cpp:60,112 (verbose==1) */
    void (*print)(void *ctx, const char *text);               /* Rprintf, src/nnmf.cpp:100-104,155-156,188-189,194-198 (verbose==2) */
    void (*warning)(void *ctx, const char *text);             /* Rcpp::warning, src/nnmf.cpp:208-209 */
    double (*unif_rand)(void *ctx);                           /* R's RNG behind arma::randu, src/nnmf.cpp:84,94; src/nnlm.cpp:39 */
} nnlm_callbacks;

/* ------------------------------------------------------------------------------------------
 * One-shot entries (what `.Call("_NNLM_c_nnmf", ...)` / `.Call("_NNLM_c_nnlm", ...)` bind to)
 * ---------------------------------------------------------------------------------------- */

/* Length the four trace vectors must have: ceil(max_iter/trace)+1 (src/nnmf.cpp:53-54). */
unsigned nnlm_trace_capacity(unsigned max_iter, unsigned trace);

/*
 * Replaces c_nnmf (reference src/nnmf.cpp:4-220; signature src/RcppExports.cpp:29-51).
 *   A        n x m, const, may contain non-finite = missing
 *   k        rank K (already includes known-profile columns, R/misc.R:84)
 *   W_init   n x k initial W, or NULL for the default 0.01*U(0,1) init (src/nnmf.cpp:82-88)
 *   H_init   k x m initial H, or NULL (src/nnmf.cpp:92-98)
 *   Wm, Hm   n x k / k x m logical masks, or NULL when empty (src/nnmf.cpp:75-80)
 *   n_threads accepted for signature compatibility; the GPU path ignores it
 * Outputs (caller-allocated): W_out n x k, H_out k x m, four traces of nnlm_trace_capacity()
 * doubles each with *n_trace entries used (src/nnmf.cpp:200-206), *n_iteration (src/nnmf.cpp:218),
 * *warned = 1 iff the reference would have raised "Target tolerance not reached. Try a larger
 * max.iter." (src/nnmf.cpp:208-209; the text is also passed to cb->warning).
 */
int nnlm_c_nnmf(const double *A, int n, int m, unsigned k,
                const double *W_init, const double *H_init, const int *Wm, const int *Hm,
                const double alpha[3], const double beta[3],
                unsigned max_iter, double rel_tol, int n_threads, int verbose, int show_warning,
                unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace,
                double *W_out, double *H_out,
                double *mse_error, double *mkl_error, double *target_error, double *average_epoch,
                int *n_trace, unsigned *n_iteration, int *warned,
                const nnlm_callbacks *cb);
/* nnlm_c_nnmf on a sparse A (canonical CSC, see nnlm_set_matrix_csc); the arguments after k are those of nnlm_c_nnmf.  Methods 1 and 2. */
int nnlm_c_nnmf_csc(int n, int m, const long long *colptr, const int *rowidx, const double *x, unsigned k,
                    const double *W_init, const double *H_init, const int *Wm, const int *Hm,
                    const double alpha[3], const double beta[3],
                    unsigned max_iter, double rel_tol, int n_threads, int verbose, int show_warning,
                    unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace,
                    double *W_out, double *H_out,
                    double *mse_error, double *mkl_error, double *target_error, double *average_epoch,
                    int *n_trace, unsigned *n_iteration, int *warned,
                    const nnlm_callbacks *cb);
/* nnlm_c_nnmf_csc through nnlm_set_matrix_csc_kl: the same arguments, all four methods (KL loss: k <= 64, stored values >= 0). */
int nnlm_c_nnmf_csc_kl(int n, int m, const long long *colptr, const int *rowidx, const double *x, unsigned k,
                       const double *W_init, const double *H_init, const int *Wm, const int *Hm,
                       const double alpha[3], const double beta[3],
                       unsigned max_iter, double rel_tol, int n_threads, int verbose, int show_warning,
                       unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace,
                       double *W_out, double *H_out,
                       double *mse_error, double *mkl_error, double *target_error, double *average_epoch,
                       int *n_trace, unsigned *n_iteration, int *warned,
                       const nnlm_callbacks *cb);
/* nnlm_c_nnmf_csc with the absent entries of A missing (see nnlm_set_matrix_csc_missing); same arguments.  Methods 1 and 2, k <= 64. */
int nnlm_c_nnmf_csc_missing(int n, int m, const long long *colptr, const int *rowidx, const double *x, unsigned k,
                            const double *W_init, const double *H_init, const int *Wm, const int *Hm,
                            const double alpha[3], const double beta[3],
                            unsigned max_iter, double rel_tol, int n_threads, int verbose, int show_warning,
                            unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace,
                            double *W_out, double *H_out,
                            double *mse_error, double *mkl_error, double *target_error, double *average_epoch,
                            int *n_trace, unsigned *n_iteration, int *warned,
                            const nnlm_callbacks *cb);

/* nnlm_c_nnmf_csc_missing with one weight per stored entry (see nnlm_set_matrix_csc_weighted): weight[nnz] in the order of x, and
 * absent_missing = 1 (absent entries missing: weighted NMF) or 0 (absent entries are zeros of weight 1: implicit feedback); the other
 * arguments are those of nnlm_c_nnmf_csc_missing.  Methods 1 and 2, k <= 64. */
int nnlm_c_nnmf_csc_weighted(int n, int m, const long long *colptr, const int *rowidx, const double *x, const double *weight,
                             int absent_missing, unsigned k,
                             const double *W_init, const double *H_init, const int *Wm, const int *Hm,
                             const double alpha[3], const double beta[3],
                             unsigned max_iter, double rel_tol, int n_threads, int verbose, int show_warning,
                             unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace,
                             double *W_out, double *H_out,
                             double *mse_error, double *mkl_error, double *target_error, double *average_epoch,
                             int *n_trace, unsigned *n_iteration, int *warned,
                             const nnlm_callbacks *cb);

/*
 * Replaces c_nnlm (reference src/nnlm.cpp:4-53; signature src/RcppExports.cpp:10-27).
 *   x n x p, y n x q (may contain missing), mask p x q or NULL, beta0 p x q or NULL (-> U(0,1) init).
 * Outputs: coefficient p x q, *n_iteration = summed per-column sweeps (src/nnlm.cpp:44-51).
 */
int nnlm_c_nnlm(const double *x, const double *y, int n, int p, int q,
                const double alpha[3], const int *mask, const double *beta0,
                unsigned max_iter, double rel_tol, int n_threads, int method,
                double *coefficient, int *n_iteration, const nnlm_callbacks *cb);
/* nnlm_c_nnlm with a sparse y (n x q, canonical CSC, see nnlm_set_matrix_csc); x stays dense; the arguments after q are those of
 * nnlm_c_nnlm.  Methods 1 and 2. */
int nnlm_c_nnlm_csc(const double *x, int n, int p, int q, const long long *ycolptr, const int *yrowidx, const double *yx,
                    const double alpha[3], const int *mask, const double *beta0,
                    unsigned max_iter, double rel_tol, int n_threads, int method,
                    double *coefficient, int *n_iteration, const nnlm_callbacks *cb);
/* nnlm_c_nnlm_csc through nnlm_set_matrix_csc_kl: the same arguments, all four methods (KL loss: p <= 64, stored values >= 0). */
int nnlm_c_nnlm_csc_kl(const double *x, int n, int p, int q, const long long *ycolptr, const int *yrowidx, const double *yx,
                       const double alpha[3], const int *mask, const double *beta0,
                       unsigned max_iter, double rel_tol, int n_threads, int method,
                       double *coefficient, int *n_iteration, const nnlm_callbacks *cb);
/* nnlm_c_nnlm_csc with the absent entries of y missing (the recommender's fold-in of new columns); same arguments.  Methods 1 and 2,
 * p <= 64. */
int nnlm_c_nnlm_csc_missing(const double *x, int n, int p, int q, const long long *ycolptr, const int *yrowidx, const double *yx,
                            const double alpha[3], const int *mask, const double *beta0,
                            unsigned max_iter, double rel_tol, int n_threads, int method,
                            double *coefficient, int *n_iteration, const nnlm_callbacks *cb);
/* nnlm_c_nnlm_csc_missing with one weight per stored entry of y (weight[nnz], absent_missing as in nnlm_c_nnmf_csc_weighted): the
 * weighted fold-in of new columns.  Methods 1 and 2, p <= 64. */
int nnlm_c_nnlm_csc_weighted(const double *x, int n, int p, int q, const long long *ycolptr, const int *yrowidx, const double *yx,
                             const double *weight, int absent_missing,
                             const double alpha[3], const int *mask, const double *beta0,
                             unsigned max_iter, double rel_tol, int n_threads, int method,
                             double *coefficient, int *n_iteration, const nnlm_callbacks *cb);

/* ------------------------------------------------------------------------------------------
 * Resident API: the same path with A kept in HBM across calls.  The one-shot entries are thin
 * wrappers over it; bench.py and the parity tests of single half-steps use it directly.
 * ---------------------------------------------------------------------------------------- */
typedef struct nnlm_handle nnlm_handle;

/* device = HIP device ordinal; precision = NNLM_PREC_*.  Fails loudly when no gfx950 device exists. */
int nnlm_create(nnlm_handle **out, int device, int precision);
void nnlm_destroy(nnlm_handle *h);
/* Process-wide caches: the streams / events / small buffers of the last destroyed handle wait for the next nnlm_create on the same
 * device, and nnlm_set_matrix keeps its two pinned bounce buffers (up to 2 x 64 MB of pinned host memory).  Both are released at exit;
 * an embedder that unloads the library earlier (the R package's .onUnload, pkg/src/r_glue.c) or wants the memory back calls this.
 * Handles in use are not affected. */
int nnlm_release_caches(void);
const char *nnlm_last_error(const nnlm_handle *h); /* h may be NULL: error of the last failed nnlm_create / one-shot call */
int nnlm_abi_version(void);

/* Upload A (n x m, fp64, column-major; never written).  One pass on the device converts to the resident layout,
 * finds the non-finite entries -- NA, NaN, +Inf and -Inf alike are "missing" (src/nnmf.cpp:65-69) -- and sums the constant
 * KL part (src/nnmf.cpp:70,73).  The matrix is streamed through pinned staging buffers filled by a few host threads.
 * NNLM_PREC_F32 only: NNLM_ERR_UNSUPPORTED when A holds a finite entry beyond FLT_MAX or its largest entry is below 2^-100
 * (the 4-byte resident copy cannot represent it; NNLM_PREC_F64 takes such a matrix, as the reference does). */
int nnlm_set_matrix(nnlm_handle *h, const double *A, int n, int m);
/* Sparse A, n x m in canonical CSC: colptr[m+1] (colptr[0] = 0, non-decreasing, colptr[m] = nnz; 64-bit, so nnz may exceed 2^31),
 * rowidx[nnz] strictly increasing within a column, 0 <= rowidx < n, x[nnz] finite (rowidx / x may be NULL when nnz = 0).  Absent
 * entries are ZEROS, not missing.  Replaces whatever matrix the handle held (nnlm_set_matrix does the same in reverse).  The handle keeps
 * the CSC and the CSR of the same matrix in HBM (values in the mode's type, int32 indices, int64 pointers) and nothing n x m sized.
 * NNLM_ERR_ARG for a non-canonical structure or a non-finite value; NNLM_PREC_F32 applies nnlm_set_matrix's range rule
 * (NNLM_ERR_UNSUPPORTED).  nnz = 0, empty rows and empty columns are legal.  On such a handle nnlm_half_step, nnlm_iterate, nnlm_run and
 * nnlm_errors work for methods 1 and 2 (square loss), at any rank, with masks; methods 3 and 4 (KL loss), nnlm_comm_init and
 * nnlm_debug_partial return NNLM_ERR_UNSUPPORTED.  nnlm_errors' KL sum leaves out the zeros' -eps log(wh + eps), at most 3.7e-15 each. */
int nnlm_set_matrix_csc(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x);
/* nnlm_set_matrix_csc for count data that is to be fitted with KL loss: the same arguments, contract and validation, and one more rule --
 * every stored value is >= 0 (NNLM_ERR_ARG names the first negative one).  The handle is the sparse handle nnlm_set_matrix_csc leaves
 * (absent entries are zeros; methods 1 and 2, the traces, nnlm_top_n's exclusion and nnlm_get_info behave bit for bit as there) and
 * ALSO runs methods 3 and 4 in nnlm_half_step, nnlm_iterate and nnlm_run: scd_kl_update / lee_kl_update over the stored entries of each
 * line (a zero entry of A adds an exact 0 to every sum of those loops but the column sums of the fixed factor), O(nnz k) per half-step,
 * nothing n x m sized -- at most one state value per stored entry besides the matrix.  Masks, known profiles, all three penalties, any
 * inner_max_iter, both arithmetic modes (state fp32 / fp64).  Rank <= 64 for methods 3 and 4 (NNLM_ERR_UNSUPPORTED beyond);
 * nnlm_comm_init and the batch entries return NNLM_ERR_UNSUPPORTED.  Two runs give bit-identical results.  nnlm_get_info: "sparse_kl". */
int nnlm_set_matrix_csc_kl(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x);
/* nnlm_set_matrix_csc for restarts and rank sweeps: the same arguments, contract, validation and resident layout (absent entries are
 * zeros).  The handle is the sparse handle nnlm_set_matrix_csc leaves -- nnlm_set_factors, nnlm_half_step, nnlm_iterate, nnlm_run,
 * nnlm_errors, nnlm_top_n and nnlm_predict_entries behave bit for bit as there -- and ALSO accepts nnlm_set_factors_batch,
 * nnlm_run_batch and nnlm_get_factors_batch: per half-step ONE SpMM over the non-zeros at the stacked rank, per trace iteration ONE
 * walk over the non-zeros for the error sums of all members.  The batch's own limits hold (methods 1 and 2, rank sum <= 64, no
 * communicator).  A handle loaded by any other sparse entry refuses the batch entries as before.  nnlm_get_info: "sparse_batch". */
int nnlm_set_matrix_csc_batch(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x);
/* nnlm_set_matrix_csc_kl for restarts and rank sweeps of count data: the same arguments, contract and validation (a negative stored
 * value is refused) and the same resident layout.  The handle is the sparse KL handle nnlm_set_matrix_csc_kl leaves -- solo calls behave
 * bit for bit as there -- and ALSO accepts nnlm_set_factors_batch, nnlm_run_batch and nnlm_get_factors_batch with ALL FOUR methods.
 * Methods 1 and 2 run as on a handle of nnlm_set_matrix_csc_batch, bit for bit.  Methods 3 and 4 (KL loss): per half-step one row copy
 * and one column-sum launch for the stacked fixed factor, then ONE solver launch over the lines of at most "sparse_kl_short_max" stored
 * entries for all active members (a wavefront per line interleaves "sparse_kl_batch_group" members); a longer line is solved once per
 * member.  Member b of the batch equals the solo fit of rank k[b] on an nnlm_set_matrix_csc_kl handle from the same start after the
 * same number of iterations BIT FOR BIT (the traces differ by the error block's summation order).  The batch's other limits hold (rank
 * sum <= 64, no masks, no communicator).  nnlm_get_info: "sparse_kl_batch". */
int nnlm_set_matrix_csc_kl_batch(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x);
/* The same CSC contract and validation as nnlm_set_matrix_csc, but absent entries are MISSING (a score matrix: movies x customers): every
 * stored entry is an observation, an explicitly stored zero included, and the factorisation fits the stored entries only -- the
 * reference's update_with_missing() (src/update_with_missing.cpp:58-139) on the matrix with NA at the absent entries, without anything
 * n x m sized: per-column Grams over the stored rows of each column are formed in column chunks of at most min(1 GiB,
 * nnlm_debug_alloc_limit) bytes.  nnlm_matrix_info: n_non_missing = nnz, any_missing = (nnz < n m), kl_const over the stored entries;
 * nnlm_errors' sums run over the stored entries.  Works on such a handle: nnlm_half_step, nnlm_iterate, nnlm_run, nnlm_errors, methods 1
 * and 2, both modes, ranks 1..64, masks and known profiles.  NNLM_ERR_UNSUPPORTED: methods 3 and 4, rank > 64 (nnlm_set_factors),
 * nnlm_comm_init, nnlm_debug_partial and the batch entries (their door: nnlm_set_matrix_csc_missing_batch). */
int nnlm_set_matrix_csc_missing(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x);
/* Per-entry weights on a sparse A: the CSC contract and validation of nnlm_set_matrix_csc / nnlm_set_matrix_csc_missing plus
 * weight[nnz], one weight c_e per stored entry in the order of x -- not NULL, every weight finite and >= 0 (NNLM_ERR_ARG names the first
 * offender; a weight of 0 is legal); NNLM_PREC_F32 applies the range rules to c a as to a.  absent_missing = 1: an absent entry is
 * missing (weighted NMF on the stored entries); absent_missing = 0: an absent entry is a zero of weight 1 (implicit feedback, Hu, Koren
 * & Volinsky 2008: c = 1 + alpha r on the stored entries).  The loss is 1/2 sum over the observed entries of c (a - (WH))^2 + the
 * reference's penalties; a half-step is the reference's update_with_missing() / update() on the column problem whose rows are scaled by
 * sqrt(c): per column G_j = c0 G_full + sum over its stored entries of (c_e - c0) y y^T and b_j = sum of c_e a_e y (c0 = the weight of
 * an absent entry), then the per-column solvers of the NA path; nothing n x m sized.  The handle is the one the unweighted door leaves
 * for the same absent semantics -- nnlm_matrix_info's N (nnz, a weight-0 entry counted, or n m), check_k, nnlm_top_n's exclusion and
 * nnlm_predict_entries -- plus the weights and the products c a in both orientations; kl_const is the weighted constant.  Traces:
 * mse = sum c (a - wh)^2 / N, mkl = kl_const + sum c (-(a + eps) log(wh + eps) + wh) / N over the observed entries.  With every weight
 * 1 and absent_missing = 1 all results equal nnlm_set_matrix_csc_missing's bit for bit.  Methods 1 and 2, both modes, ranks 1..64,
 * masks, known profiles, all three penalties.  NNLM_ERR_UNSUPPORTED: methods 3 and 4, rank > 64, the batch entries, nnlm_comm_init,
 * nnlm_debug_partial, nnlm_svd and the NNDSVD starts.  nnlm_get_info: "sparse_weighted". */
int nnlm_set_matrix_csc_weighted(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x,
                                 const double *weight, int absent_missing);
/* nnlm_set_matrix_csc_missing for restarts, rank sweeps and rank selection: the same contract and validation, with an optional HOLD-OUT
 * pattern ho_colptr[m + 1] / ho_rowidx[] -- a canonical CSC pattern that must be a subset of the stored pattern; ho_colptr == NULL: no
 * hold-out set.  Held-out entries leave the stored set on the host before the CSC and the CSR are built; their values stay on the device
 * (mode's type) for nnlm_holdout_errors.  The handle is then the sparse-missing handle of the TRAINING entries: nnlm_matrix_info, the
 * segment layout and every solo call are those of nnlm_set_matrix_csc_missing on the training CSC, bit for bit.  It ALSO accepts
 * nnlm_set_factors_batch, nnlm_run_batch and nnlm_get_factors_batch: per half-step ONE SpMM at the stacked rank and, per column chunk,
 * ONE launch for the per-column Grams of all members (each bit-equal to the solo Gram at the member's rank); per trace iteration ONE
 * walk over the stored entries for the error sums of all members.  The batch's own limits hold (methods 1 and 2, rank sum <= 64, no
 * masks, no communicator).  nnlm_get_info: "matrix_absent_missing" = 1, "sparse_batch" = 1, "matrix_holdout" = the held-out count
 * (0 is legal; -1 without a pattern), "sp_gram_batch_pairs".  NNLM_ERR_ARG, naming the first offender: a held-out position that is
 * not stored, a non-canonical pattern, every stored entry held out. */
int nnlm_set_matrix_csc_missing_batch(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x,
                                      const long long *ho_colptr, const int *ho_rowidx);
/* Dense finite A (fp64, column-major) with a HOLD-OUT set: colptr[m + 1] / rowidx[] is a canonical CSC pattern (the validation of
 * nnlm_set_matrix_csc; an empty pattern is legal) of the entries kept out of the fit.  The handle is then in the state nnlm_set_matrix
 * leaves for A with NA at the pattern -- missing bits, 0 in every resident copy, n_non_missing / any_missing / kl_const over the
 * training entries -- and keeps the held-out entries on the device as a CSC of their own (values in the mode's type, int32 indices,
 * int64 pointers: O(held-out entries)).  The pattern is applied chunk by chunk in the upload's host staging buffer: A is not
 * written and no second n x m array is made.  NNLM_ERR_ARG: a non-finite entry of A (named in the message), a non-canonical pattern,
 * a pattern that holds out every entry.  nnlm_half_step, nnlm_iterate, nnlm_run and nnlm_errors behave as on the NA matrix (all four
 * methods); nnlm_set_factors_batch / nnlm_run_batch accept such a handle (below); nnlm_comm_init returns NNLM_ERR_UNSUPPORTED.
 * nnlm_get_info "matrix_holdout": the held-out count, -1 on any other handle. */
int nnlm_set_matrix_holdout(nnlm_handle *h, const double *A, int n, int m, const long long *colptr, const int *rowidx);
/* Errors of the current factors on the held-out entries: mse[b] = mean (a - wh)^2, mkl[b] = mean (a + eps) log((a + eps) / (wh + eps))
 * - a + wh, for the B members of a batch (arrays of length B) or the solo factors (length 1).  fp64 sums in a fixed order, no
 * atomics; synchronises.  An empty hold-out set gives NaN for both; NNLM_ERR_ARG on a handle without a hold-out set.  Hold-out sets
 * come from nnlm_set_matrix_holdout (dense A) and nnlm_set_matrix_csc_missing_batch (sparse A, absent entries missing). */
int nnlm_holdout_errors(nnlm_handle *h, double *mse, double *mkl);
/* ------------------------------------------------------------------------------------------
 * Scores of the current factors without forming W H.  Both entries run on a handle that holds a matrix (any kind: it gives n and m)
 * and solo factors; both read the fp64 masters of the factors, so a score is the same in both arithmetic modes, at any rank (beyond 64
 * included); both synchronise.  Their workspaces live for the call and are processed in rounds: nothing n x m or n_lines x n sized is
 * allocated.  NNLM_ERR_UNSUPPORTED: a handle with batched factors or a communicator.  NNLM_ERR_ARG: no matrix or no factors set.
 * ---------------------------------------------------------------------------------------- */
/* out[e] = sum_q W[rows[e], q] * H[q, cols[e]], fp64, q ascending.  rows / cols: host int32, 0-based, count >= 0 (count = 0 succeeds and
 * writes nothing).  NNLM_ERR_ARG names an index out of range. */
int nnlm_predict_entries(nnlm_handle *h, long long count, const int *rows, const int *cols, double *out);
/* by = 0: for every listed column j, the n_top rows i with the largest (W H)[i, j]; by = 1: for every listed row i, the n_top columns.
 * lines: host int32[n_lines] (NULL = all lines of that side, n_lines ignored).  exclude = 1: entries STORED in the resident sparse
 * matrix (either absent semantics) are not candidates.  idx_out: int32[n_lines][n_top], score_out: double[n_lines][n_top].
 * Results come in descending score order and EQUAL SCORES IN ASCENDING INDEX ORDER: (score descending, index ascending) is a total order,
 * so the result is a function of the scores alone, and the bits of a score are a function of (i, j, W, H) alone -- neither depends on
 * the lines asked for, the device's size or how the candidates were sliced.  A line with fewer than n_top candidates is padded with index
 * -1 and score NaN; a NaN score is never selected.  1 <= n_top <= 128.
 * NNLM_ERR_UNSUPPORTED: n_top > 128; exclude = 1 on a handle whose matrix is not sparse.  NNLM_ERR_ARG: a line out of range, n_top < 1,
 * by / exclude outside {0, 1}.  nnlm_profile_get names: "topn", "topn_merge" ("predict_entries" for the entry above);
 * nnlm_get_info "topn_slices": candidate slices of the last launch. */
int nnlm_top_n(nnlm_handle *h, int by, int n_top, const int *lines, long long n_lines, int exclude, int *idx_out, double *score_out);
/* Ranking metrics of those lists against held-out entries, on the device: the lists of a round of lines are evaluated where
 * nnlm_top_n's kernels leave them and are never copied to the host.  by, lines, n_lines and exclude mean what they mean for nnlm_top_n
 * and carry its checks.  cutoffs: host int32[n_cut], 1 <= n_cut <= 8, strictly ascending values in 1 .. 128; n_top = the last one.
 * held_ptr / held_idx: the held-out pattern on the host IN THE ORIENTATION OF by -- by = 0: a CSC, m + 1 int64 pointers and int32 row
 * indices; by = 1: a CSR, n + 1 pointers and column indices -- indices strictly ascending inside a line and in range; a pattern without
 * entries is legal (held_idx may then be NULL); entries of lines that are not listed are ignored.  The whole pattern is checked on the
 * host before anything is uploaded (NNLM_ERR_ARG names the first offending line or entry); the entries of the listed lines are then
 * uploaded once.  With exclude = 1 a held-out entry that the resident matrix STORES could never be listed: the call is refused with
 * NNLM_ERR_ARG naming the first such entry in (position in lines, index) order, and nothing is evaluated.
 * Per listed line l with held-out set T, t = |T|, and list L[0 .. n_top) exactly as nnlm_top_n returns it (padding -1 never hits), for
 * a cutoff c:  hits_c = #{p < c : L[p] in T};  first = the smallest p with L[p] in T, or -1;  dcg_c = sum over hits p < c of d[p],
 * d[p] = 1 / log2(p + 2) (a table computed once on the host in fp64);  apn_c = sum over hits p < c of hits_(p+1) / (p + 1); both sums in
 * ascending p.  From them: precision = hits_c / c, recall = hits_c / t, hit rate = [hits_c > 0], NDCG = dcg_c / sum_{p < min(c, t)} d[p],
 * AP = apn_c / min(c, t), RR = 1 / (first + 1) if 0 <= first < c, else 0.
 * A line is EVALUATED iff it is listed and t > 0; *n_eval_out = their number.  agg_out: double[n_cut][6], the means over the evaluated
 * lines of precision, recall, hit rate, NDCG, AP and RR (all NaN when no line is evaluated).  The sums are fp64 in a fixed order (a
 * fixed-shape reduction per round of 16384 lines, then the rounds in order; no atomics on data): two calls give identical bits, and
 * a line's values do not depend on which other lines were asked for.  line_out: NULL, or double[n_lines][2 + 3 n_cut]: t, first, then
 * hits_c, dcg_c, apn_c per cutoff (the integers exactly); a listed line with t = 0 gets t = 0, first = -1 and zeros.
 * NNLM_ERR_UNSUPPORTED: a cutoff above 128, and whatever nnlm_top_n refuses so.  NNLM_ERR_ARG: n_cut outside 1 .. 8, a cutoff below 1 or
 * not ascending, and whatever nnlm_top_n refuses so.  nnlm_profile_get name: "topn_eval" (next to "topn", "topn_merge");
 * nnlm_get_info "topn_eval_lines": the evaluated lines of the last call.  Synchronises. */
int nnlm_top_n_eval(nnlm_handle *h, int by, const int *cutoffs, int n_cut, const int *lines, long long n_lines, int exclude,
                    const long long *held_ptr, const int *held_idx, double *agg_out, long long *n_eval_out, double *line_out);

/* Number of finite entries of A (N_non_missing, src/nnmf.cpp:51,69) and the any_missing flag.  Sparse A: n m and 0, and kl_const counts
 * the zeros ((n m - nnz) eps log eps); absent entries missing (nnlm_set_matrix_csc_missing): nnz and (nnz < n m). */
int nnlm_matrix_info(nnlm_handle *h, double *n_non_missing, int *any_missing, double *kl_const);

/* Set rank, factors (W n x k, H k x m; NULL = zeros) and masks (NULL = none). */
int nnlm_set_factors(nnlm_handle *h, unsigned k, const double *W, const double *H, const int *Wm, const int *Hm);
int nnlm_get_factors(nnlm_handle *h, double *W, double *H);

/* ------------------------------------------------------------------------------------------
 * Matrices and factors that already live in device memory (a tensor pipeline's output, an earlier fit): no trip through the host.
 * A descriptor is plain data: element (i, j) of the matrix is at ptr[i * row_stride + j * col_stride], strides in ELEMENTS, both
 * positive, and the layout may not overlap itself: col_stride >= rows * row_stride (column-major family) or row_stride >= cols *
 * col_stride (row-major family).  ptr is device or managed memory of the handle's device.  Every rule is checked before a kernel reads
 * the pointer; a violation is NNLM_ERR_ARG naming the argument (a host pointer, another device's memory, a dtype out of range, a zero
 * or negative stride, an overlapping layout, an extent past the end of its allocation, and -- best effort -- a buffer of the handle itself).
 * `stream` is the caller's hipStream_t on which the data was produced or will be consumed (NULL: the default stream).  Ordering goes
 * through events: an input entry makes the handle's stream wait for what the caller's stream holds at the call; the output entry also
 * makes the caller's stream wait for the export.  The two set entries return after their kernels have run (as the host entries return
 * after their copies); the get entry does not wait on the host at all.
 * ---------------------------------------------------------------------------------------- */
typedef struct { const void *ptr; int dtype; long long row_stride, col_stride; } nnlm_dev_matrix; /* strides in elements */
enum { NNLM_DT_F64 = 0, NNLM_DT_F32 = 1, NNLM_DT_F16 = 2, NNLM_DT_BF16 = 3 };
/* nnlm_set_matrix on the fp64 widening of A's values (any of the four types, exact): non-finite entries are missing, NNLM_PREC_F32
 * applies the same range rule (NNLM_ERR_UNSUPPORTED), and the handle afterwards is the plain dense handle nnlm_set_matrix leaves -- A,
 * the missing bits and n_non_missing are that upload's bit for bit; kl_const too when row_stride = 1 (the same partial sums in the same
 * order), otherwise it differs by summation order only.  row_stride = 1 (R / Fortran order) and col_stride = 1 (C order) are read and
 * written in contiguous runs (one pass over A); other strides are gathered element by element: correct, not fast. */
int nnlm_set_matrix_device(nnlm_handle *h, const nnlm_dev_matrix *A, int n, int m, void *stream);
/* nnlm_set_factors with W (n x k) and H (k x m) in device memory, any of the four types; a NULL descriptor = zeros; the masks stay
 * host arrays with the same meaning. */
int nnlm_set_factors_device(nnlm_handle *h, unsigned k, const nnlm_dev_matrix *W, const nnlm_dev_matrix *H, const int *Wm, const int *Hm,
                            void *stream);
/* The current factors into the caller's buffers: dtype NNLM_DT_F64 or NNLM_DT_F32 (rounded to nearest); only the n x k / k x m entries
 * are written, the gaps of a strided buffer stay as they are; a NULL descriptor = not wanted. */
int nnlm_get_factors_device(nnlm_handle *h, const nnlm_dev_matrix *W, const nnlm_dev_matrix *H, void *stream);

/* A SPARSE matrix that already lives in device memory, compressed by columns (CSC) or by rows (CSR): ptr has m + 1 (CSC) or n + 1 (CSR)
 * entries, idx and val have nnz entries each, all three contiguous device (or managed) arrays of the handle's device.  ptr_dtype and
 * idx_dtype are NNLM_IT_I32 or NNLM_IT_I64, independently; val_dtype is one of the four NNLM_DT_*.  `stream` as for nnlm_set_matrix_device.
 * The call returns after its last read of the caller's arrays; the handle owns copies.
 *
 * The handle afterwards is the one the matching host entry leaves for the fp64 widening of the same values -- the six resident arrays
 * (both sides, indices ascending in every line), nnz, n_non_missing, any_missing, the byte count, the sizing of the partial sums, the
 * long-column tables (missing door) and long-line lists (KL doors), the flags -- with kl_const differing by summation order only.
 * `door` chooses that entry: 0 nnlm_set_matrix_csc, NNLM_SP_BATCH nnlm_set_matrix_csc_batch, NNLM_SP_KL nnlm_set_matrix_csc_kl,
 * NNLM_SP_KL | NNLM_SP_BATCH nnlm_set_matrix_csc_kl_batch, NNLM_SP_ABSENT_MISSING nnlm_set_matrix_csc_missing, NNLM_SP_ABSENT_MISSING |
 * NNLM_SP_BATCH nnlm_set_matrix_csc_missing_batch without a hold-out set; NNLM_SP_ABSENT_MISSING | NNLM_SP_KL is NNLM_ERR_ARG.
 *
 * Everything is done by kernels (k_sparse_ingest.h): the given side is checked and copied with type conversion,
 * the other side is built by a stable radix sort.  Nothing of size nnz crosses to the host; the two int64 pointer arrays come back,
 * (n + m + 2) * 8 bytes.  Refusals follow the host entries' contract, same codes, first offender named (for CSR the words "row" and
 * "column" trade places): ptr[0] != 0, a decreasing pointer, ptr[last] != nnz, nnz > n m, an index out of range, indices of a line not
 * strictly increasing, a non-finite value, a negative value on a KL door, the two range rules of NNLM_PREC_F32 (NNLM_ERR_UNSUPPORTED), a
 * sharded handle (NNLM_ERR_UNSUPPORTED), a pointer that is not device memory of the handle's device, a bad dtype, layout or door code.
 * No value read from the caller's arrays is used as an address before it has been checked: a malformed input ends in a refusal, and a
 * refused call leaves the handle's previous matrix and factors as they were.  Temporaries (at most 24 bytes per stored entry beside the
 * new resident arrays, see DESIGN) are freed before the call returns; a failed allocation is NNLM_ERR_HIP with the handle unchanged.
 * nnlm_get_info "matrix_min_col_observed" / "matrix_min_row_observed" answer for a handle loaded here: the fewest stored entries of a
 * column / of a row on the missing doors, n / m on the others. */
enum { NNLM_IT_I32 = 0, NNLM_IT_I64 = 1 };
enum { NNLM_SP_CSC = 0, NNLM_SP_CSR = 1 };
enum { NNLM_SP_ABSENT_MISSING = 1, NNLM_SP_KL = 2, NNLM_SP_BATCH = 4 }; /* `door` bits */
typedef struct { const void *ptr, *idx, *val; int ptr_dtype, idx_dtype, val_dtype, layout; long long nnz; } nnlm_dev_sparse;
int nnlm_set_matrix_sparse_device(nnlm_handle *h, const nnlm_dev_sparse *A, int n, int m, int door, void *stream);
/* TEST HOOK: the resident arrays of one side of the handle's sparse matrix (side 0: by columns, ptr_out [m + 1], idx_out = rows; side 1:
 * by rows, ptr_out [n + 1], idx_out = columns; idx_out and val_out [nnz]), values widened to fp64.  A NULL output = not wanted.
 * NNLM_ERR_ARG when the handle holds no sparse matrix. */
int nnlm_debug_sparse_resident(nnlm_handle *h, int side, long long *ptr_out, int *idx_out, double *val_out);
/* nnlm_set_matrix_csc_weighted for a sparse A AND its weights in device memory.  A is what
 * nnlm_set_matrix_sparse_device takes.  Wt carries the weights: Wt->val holds Wt->nnz weights of any of the four NNLM_DT_* types, chosen
 * independently of A's (not NULL when nnz > 0), and
 *   - Wt->ptr == NULL and Wt->idx == NULL: the weights are in the order of A->val, Wt->nnz must equal A->nnz (the other fields are unused);
 *   - both given: Wt is a sparse matrix of A's layout and shape, with integer types of its own, whose stored pattern must equal A's.  A
 *     kernel compares the pattern (pointers, then indices) before any weight is read; a difference is NNLM_ERR_ARG naming the first
 *     line that differs;
 *   - one NULL and the other not, or Wt->layout != A->layout in the second form: NNLM_ERR_ARG.
 * absent_missing as in nnlm_set_matrix_csc_weighted (the weighted handle has no batch and no KL door).  `stream`: the one stream on which
 * both descriptors' arrays were produced.
 *
 * The handle afterwards is the one nnlm_set_matrix_csc_weighted leaves for the fp64 widening of the same values and weights: the six
 * structural arrays, the weights and the products c a of both sides (c a is ONE fp64 multiply of the widenings, then rounded to the mode's
 * type), nnz, n_non_missing, any_missing, the byte count, the long-column tables of both orientations, "sparse_weighted"; kl_const is the
 * weighted constant up to summation order; the observed minima answer as after nnlm_set_matrix_sparse_device.
 *
 * Refusals, in this order, each leaving the handle's previous matrix and factors untouched: (1) arguments, descriptors and the
 * device-memory rules of all arrays of both descriptors; (2) A's pointers; (3) A's entries -- all as nnlm_set_matrix_sparse_device, so
 * an offence of A anywhere wins over a weight offence at an earlier entry; (4) the pattern of the weights; (5) the first weight that is
 * not a finite number >= 0, worded as the host entry words it (entry number in the given layout's order; -0.0 is legal); (6)
 * NNLM_PREC_F32's range rules in the host entry's order and words: entries with |a|, c or |c a| beyond the fp32 range, max |A| too small,
 * max |weight * A| too small (NNLM_ERR_UNSUPPORTED).  Temporaries: at most 37.1 bytes per stored entry beside the ten new resident arrays
 * (DESIGN section 4.24). */
int nnlm_set_matrix_sparse_device_weighted(nnlm_handle *h, const nnlm_dev_sparse *A, const nnlm_dev_sparse *Wt, int n, int m, int absent_missing,
                                           void *stream);
/* TEST HOOK, the sibling of nnlm_debug_sparse_resident: the resident weights (wt_out [nnz]) and products c a (wa_out [nnz]) of one side,
 * widened to fp64.  A NULL output = not wanted.  NNLM_ERR_ARG on a handle without per-entry weights. */
int nnlm_debug_sparse_resident_weighted(nnlm_handle *h, int side, double *wt_out, double *wa_out);

/*
 * One half-step = update()/update_with_missing() (reference src/update_with_missing.cpp:3-55, :58-139).
 * which = 0 updates W (solves A^T ~ H^T W^T with `reg` = alpha), 1 updates H (`reg` = beta).
 * Asynchronous on the handle's stream; the integer sweep count is accumulated on the device.
 */
int nnlm_half_step(nnlm_handle *h, int which, const double reg[3], unsigned inner_max_iter,
                   double inner_rel_tol, int method);
/* n_iter outer iterations (W half-step then H half-step, src/nnmf.cpp:114-133), asynchronous. */
int nnlm_iterate(nnlm_handle *h, unsigned n_iter, const double alpha[3], const double beta[3],
                 unsigned inner_max_iter, double inner_rel_tol, int method);
/* The alternating loop of c_nnmf (reference src/nnmf.cpp:100-209) on the resident matrix and factors: same arguments,
 * traces, stopping rule, warning and callbacks as nnlm_c_nnmf, without the upload.  nnlm_c_nnmf is
 * create + set_matrix + set_factors + nnlm_run + get_factors; bench.py times this call. */
int nnlm_run(nnlm_handle *h, const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol, int verbose,
             int show_warning, unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace,
             double *mse_error, double *mkl_error, double *target_error, double *average_epoch, int *n_trace,
             unsigned *n_iteration, int *warned, const nnlm_callbacks *cb);
/* Summed per-column sweeps since the last reset (total_raw_iter, src/nnmf.cpp:106,158); synchronises. */
int nnlm_take_sweeps(nnlm_handle *h, long long *sweeps, int reset);
/* Error block (src/nnmf.cpp:121-126,135-140): mse = mean((A-WH)^2), mkl_var = mean(-(A+eps)log(WH+eps)+WH)
 * over finite entries, plus the penalty sums add_penalty() needs (src/nnmf.cpp:224-240):
 * pen[0..2] = sum(W^2), sum over i of (sum_q W[i,q])^2, sum(W); pen[3..5] the same for H.  Synchronises. */
int nnlm_errors(nnlm_handle *h, double *mse, double *mkl_var, double pen[6]);
int nnlm_sync(nnlm_handle *h);

/* ------------------------------------------------------------------------------------------
 * Batched factorisation: B independent nnmf() runs of ONE dense matrix (random restarts, rank sweeps) that share every pass over A.
 * Member b has rank k[b] and its own factors; all members share the matrix and the arguments of nnlm_run.  1 <= B <= 64, sum of
 * k[b] <= 64, methods 1 and 2 (square loss), dense A without missing entries, one GPU, no masks: anything else is refused with
 * NNLM_ERR_UNSUPPORTED (KL loss, missing entries, a sparse A, a communicator, a rank sum beyond 64) or NNLM_ERR_ARG (B or a rank out
 * of range).  Each member's factors, traces, n_iteration and warning are those nnlm_run gives for that member alone (same mode).
 * Missing entries are accepted in ONE form: a hold-out handle (nnlm_set_matrix_holdout).  Every member then solves each column with the
 * Gram over that column's observed rows, as a solo missing-value run does, behind the same single cross product; the traces' sums
 * run over the training entries.  A matrix that arrived with NA / NaN / Inf through nnlm_set_matrix stays refused.
 * A sparse A is accepted through three doors: nnlm_set_matrix_csc_batch (absent entries zeros), nnlm_set_matrix_csc_missing_batch
 * (absent entries missing, with or without a hold-out set) and nnlm_set_matrix_csc_kl_batch (absent entries zeros, stored values >= 0:
 * the one handle on which the batch also runs methods 3 and 4, KL loss).
 * ---------------------------------------------------------------------------------------- */
/* k[B] ranks; W = the members' n x k[b] blocks one after another (column-major each), H = their k[b] x m blocks one after another;
 * NULL = zeros.  Replaces the handle's factors (nnlm_set_factors ends a batch). */
int nnlm_set_factors_batch(nnlm_handle *h, unsigned B, const unsigned *k, const double *W, const double *H);
/* The members' factors, laid out as nnlm_set_factors_batch takes them. */
int nnlm_get_factors_batch(nnlm_handle *h, double *W, double *H);
/* nnlm_run for every member: the four traces are [B][nnlm_trace_capacity(max_iter, trace)] (member b's trace starts at
 * b * capacity), n_trace, n_iteration and warned are [B].  A member whose stopping rule fires (its own target error) is frozen:
 * its later sweeps are skipped.  The loop ends when every member has stopped or max_iter is reached.  Per half-step ONE
 * cross product of A with the stacked factors; per trace iteration ONE pass over A for the error sums of all members. */
int nnlm_run_batch(nnlm_handle *h, const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol, int verbose,
                   int show_warning, unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace,
                   double *mse_error, double *mkl_error, double *target_error, double *average_epoch, int *n_trace,
                   unsigned *n_iteration, int *warned, const nnlm_callbacks *cb);
/* create + set_matrix + set_factors_batch + run_batch + get_factors_batch (precision as nnlm_c_nnmf).  W_init / H_init NULL: each
 * member gets the default init of nnlm_c_nnmf, drawn member by member (W before H). */
int nnlm_c_nnmf_batch(const double *A, int n, int m, unsigned B, const unsigned *k, const double *W_init, const double *H_init,
                      const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol, int n_threads, int verbose,
                      int show_warning, unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace, double *W_out,
                      double *H_out, double *mse_error, double *mkl_error, double *target_error, double *average_epoch, int *n_trace,
                      unsigned *n_iteration, int *warned, const nnlm_callbacks *cb);

/* nnlm_c_nnmf_batch on a sparse A (canonical CSC, absent entries zeros; loaded by nnlm_set_matrix_csc_batch); the arguments after x
 * are those of nnlm_c_nnmf_batch after m, the default inits are drawn in the same order. */
int nnlm_c_nnmf_csc_batch(int n, int m, const long long *colptr, const int *rowidx, const double *x, unsigned B, const unsigned *k,
                          const double *W_init, const double *H_init, const double alpha[3], const double beta[3], unsigned max_iter,
                          double rel_tol, int n_threads, int verbose, int show_warning, unsigned inner_max_iter, double inner_rel_tol,
                          int method, unsigned trace, double *W_out, double *H_out, double *mse_error, double *mkl_error,
                          double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration, int *warned,
                          const nnlm_callbacks *cb);

/* nnlm_c_nnmf_csc_batch through nnlm_set_matrix_csc_kl_batch: the same arguments, all four methods (KL loss: stored values >= 0). */
int nnlm_c_nnmf_csc_kl_batch(int n, int m, const long long *colptr, const int *rowidx, const double *x, unsigned B, const unsigned *k,
                             const double *W_init, const double *H_init, const double alpha[3], const double beta[3], unsigned max_iter,
                             double rel_tol, int n_threads, int verbose, int show_warning, unsigned inner_max_iter, double inner_rel_tol,
                             int method, unsigned trace, double *W_out, double *H_out, double *mse_error, double *mkl_error,
                             double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration, int *warned,
                             const nnlm_callbacks *cb);

/* nnlm_c_nnmf_csc_batch on a sparse A whose absent entries are MISSING (nnlm_set_matrix_csc_missing_batch), with an optional hold-out
 * pattern ho_colptr / ho_rowidx after x (ho_colptr NULL: none) and holdout_mse[B], holdout_mkl[B] at the end: nnlm_holdout_errors of the
 * final factors, NaN without a set or with an empty one.  The default inits are drawn in the same order. */
int nnlm_c_nnmf_csc_missing_batch(int n, int m, const long long *colptr, const int *rowidx, const double *x, const long long *ho_colptr,
                                  const int *ho_rowidx, unsigned B, const unsigned *k, const double *W_init, const double *H_init,
                                  const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol, int n_threads, int verbose,
                                  int show_warning, unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace, double *W_out,
                                  double *H_out, double *mse_error, double *mkl_error, double *target_error, double *average_epoch,
                                  int *n_trace, unsigned *n_iteration, int *warned, double *holdout_mse, double *holdout_mkl,
                                  const nnlm_callbacks *cb);

/* nnlm_c_nnmf_batch on A with the pattern (colptr, rowidx) held out (nnlm_set_matrix_holdout), + holdout_mse[B], holdout_mkl[B]:
 * nnlm_holdout_errors of the final factors. */
int nnlm_c_nnmf_holdout_batch(const double *A, int n, int m, const long long *colptr, const int *rowidx, unsigned B, const unsigned *k,
                              const double *W_init, const double *H_init, const double alpha[3], const double beta[3], unsigned max_iter,
                              double rel_tol, int n_threads, int verbose, int show_warning, unsigned inner_max_iter, double inner_rel_tol,
                              int method, unsigned trace, double *W_out, double *H_out, double *mse_error, double *mkl_error,
                              double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration, int *warned,
                              double *holdout_mse, double *holdout_mkl, const nnlm_callbacks *cb);

/* ------------------------------------------------------------------------------------------
 * Truncated SVD of the resident matrix and the NNDSVD start (Boutsidis & Gallopoulos 2008) made from it: a deterministic, data-driven
 * start for W and H, and a decomposition that is a product of its own (scree, rank-k baseline).  DESIGN section 4.22.
 * Randomised subspace iteration with a sketch of width l and `power_iters` power iterations, 2 power_iters + 2 passes over A through the
 * cross products of the half-steps (split-fp16 in NNLM_PREC_F32, strict fp64 in NNLM_PREC_F64, the SpMM on a sparse handle, one launch
 * per 64 rows beyond l = 64): Y = omega A^T, Q = orth(Y); power_iters times Z = orth(Q A), Q = orth(Z A^T); B = Q A, B B^T = V L V^T,
 * sigma = sqrt(L) descending, U = V^T Q, Vt = Sigma^-1 V^T B.  orth is Gram-based and runs twice: G = X X^T = E L E^T (cyclic Jacobi in
 * fp64 on the host, fixed sweep order), X <- diag(L_i^-1/2 where L_i > 1e-12 L_max, else 0) E^T X: a direction that is dropped (every A of
 * rank below l drops some) becomes a zero row and stays one; in the last step such a direction has sigma = 0 and a zero row of Vt.
 * The library draws nothing: omega (l x m, laid out as nnlm_set_factors takes H: column-major, l rows) comes from the caller.  The sign
 * of a triplet is unspecified but joint for u_j and v_j.  No atomics on data: two calls with one omega give identical bits.
 * ---------------------------------------------------------------------------------------- */
/* Needs a matrix on the handle.  Leaves the decomposition resident (U [LP][npad], Vt [LP][mpad] in fp64 on the device, sigma on the host)
 * until the next matrix, and leaves the handle WITHOUT factors, as after nnlm_set_matrix (the factor buffers were its workspace).
 * Supported: a dense finite A however it arrived, and a sparse A whose absent entries are zeros (all four doors and the device ingest
 * that leaves those handles), both arithmetic modes.  NNLM_ERR_UNSUPPORTED, named in the message: a matrix with missing entries (NaN
 * upload, a non-empty hold-out set, the absent = missing doors), a handle with a communicator.  NNLM_ERR_ARG: l outside 1 .. min(n, m), a
 * NULL or non-finite omega.  No width is refused: the rotation kernel narrows its column tile as l grows (32 columns up to l = 512, 16 up
 * to 848, 8 up to 1280) and works out of place beyond; the host's Jacobi, O(l^3) per sweep, is what bounds l in practice.
 * nnlm_get_info: "svd_width" (l, -1 none), "svd_kept" (directions the last orth kept), "svd_rotate_form" (column tile of the last
 * rotation: 32, 16 or 8; 0 out of place; -1 none yet), "svd_ms_cross" / "svd_ms_gram" / "svd_ms_rotate" / "svd_ms_eig" / "svd_ms_wait" /
 * "svd_ms_setup" / "svd_ms_total" (host milliseconds of the last call by phase: cross products, Grams, rotations, host
 * eigendecompositions, waits and transfers, setting and freeing the rank-l factor buffers, the whole call; with nnlm_profile_enable
 * every phase waits for its kernels, so the first three hold their device time). */
int nnlm_svd(nnlm_handle *h, unsigned l, unsigned power_iters, const double *omega);
/* Test hook: the form of the rotations of nnlm_svd calls from now on (process-global, as the other nnlm_debug_* settings): 32, 16 or 8 =
 * that column tile wherever it fits the width, 0 = out of place, -1 = the width decides.  The forms give identical bits. */
int nnlm_debug_set_svd_rotate(int form);
/* The first k <= l triplets: sigma [k], U n x k, Vt k x m (column-major); any output may be NULL. */
int nnlm_get_svd(nnlm_handle *h, unsigned k, double *sigma, double *U, double *Vt);
/* NNDSVD from the first k <= l triplets; leaves exactly the state nnlm_set_factors(h, k, W, H, NULL, NULL) leaves for these W, H.
 * Component 0: sqrt(sigma_0) |u_0|, sqrt(sigma_0) |v_0|.  Component j >= 1: with the positive and negative parts of u_j, v_j and
 * p = |u+| |v+|, g = |u-| |v-|, the positive pair if p >= g, else the negative pair; W[:, j] = sqrt(sigma_j t) part_u / |part_u|, H[j, :]
 * likewise, t the chosen product; sigma_j t = 0 gives a zero column and row.  variant 0 (nndsvd) leaves the zeros: fine for the SCD
 * methods, but Lee's multiplicative updates (methods 2 and 4) keep a zero forever and KL loss divides by W H.  variant 1 (nndsvda)
 * replaces every exact zero of W and H by mean(A) over all n m entries (absent entries of a sparse A count as zeros), summed in fp64 in
 * a fixed order from the resident values -- in NNLM_PREC_F32 those are the fp32 roundings of A.  NNLM_ERR_ARG: no decomposition on the
 * handle, k = 0 or k > l, variant outside {0, 1}. */
int nnlm_set_factors_nndsvd(nnlm_handle *h, unsigned k, int variant);
/* nnlm_set_factors_batch with member b started from the NNDSVD of the first k[b] triplets: bit for bit the first k[b] components of
 * nnlm_set_factors_nndsvd at the largest rank (component j depends on triplet j alone), so one decomposition serves a rank sweep.
 * Needs max k[b] <= l (NNLM_ERR_ARG); every rule of nnlm_set_factors_batch holds (rank sum <= 64, the handle's own batch refusals). */
int nnlm_set_factors_nndsvd_batch(nnlm_handle *h, unsigned B, const unsigned *k, int variant);

/* Per-kernel device timing (HIP events on the handle's stream) for bench.py's roofline block.
 * names: "xprod_h" (A-streaming W^T A), "xprod_w" (A H^T), "xprod_w_err" (the same with the fused error sums), "gram", "sweep_h",
 * "sweep_w", "errors" (a separate pass over A), "err_reduce" (reduction of the fused error sums), "allgather", "allreduce", "unpack";
 * sparse A: "spmm_h" (W^T A), "spmm_w" (A H^T), "sp_errors" (error block), "sp_gram" (per-column Grams when absent entries are missing), "spkl_copy" (KL loss: row copy and column sums of the
 * fixed factor), "spkl_solve_h" / "spkl_solve_w" (KL loss: the per-line solvers, starting states included);
 * batched factorisation: "batch_errors" (the one pass over A of a
 * trace iteration), "batch_pen" (the members' penalty sums). */
int nnlm_profile_enable(nnlm_handle *h, int on);
int nnlm_profile_get(nnlm_handle *h, const char *name, double *total_ms, long long *launches);
int nnlm_profile_reset(nnlm_handle *h);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU (one process per GPU, RCCL over xGMI).  A is replicated.  The column of the factor being
 * solved is the unit: per half-step a rank forms the cross product of ITS 1/N of the columns over the
 * whole contraction (1/N of A from HBM), the Gram of the fixed factor (dense: one shared k x k Gram,
 * replicated; missing values: one per column), solves its columns into a packed slab, and ONE
 * ncclAllGather returns the updated factor to every rank (NNLM_FORM_COLS, the default).  Dense square loss also
 * has the form north_star words (NNLM_FORM_REDUCE, chosen with nnlm_comm_set_form): each rank contracts
 * its slab of rows (H half-step) / columns (W half-step), ONE ncclAllReduce sums the partial
 * [Gram | cross-product] buffer, then the column-sharded sweep and the all-gather -- same HBM bytes and
 * kernel time per rank (profiles/r02_shard_times.json), one more collective of (KP^2 + KP cols) doubles.
 * Error block: each rank reduces its share of A, two doubles are all-reduced.
 * ---------------------------------------------------------------------------------------- */
#define NNLM_COMM_ID_BYTES 128
#define NNLM_FORM_COLS 0   /* column-sharded half-steps, one all-gather each (every method) */
#define NNLM_FORM_REDUCE 1 /* dense square loss, rank <= 64: contraction-sharded [G | C] + all-reduce, then sweep + all-gather */
int nnlm_comm_unique_id(char id[NNLM_COMM_ID_BYTES]); /* rank 0 creates, the host layer broadcasts */
int nnlm_comm_init(nnlm_handle *h, const char id[NNLM_COMM_ID_BYTES], int rank, int nranks);
/* id == NULL makes a "virtual rank": the handle only computes rank's slab of an nranks-way split and leaves the
 * partial sums un-reduced (used with nnlm_debug_partial to test the shard arithmetic on one device). */
/* Form of the dense square-loss half-step across ranks (NNLM_FORM_*); nnlm_comm_init resets it to NNLM_FORM_COLS.  The other
 * half-steps (missing values, KL, rank > 64) are column-sharded whatever is set here. */
int nnlm_comm_set_form(nnlm_handle *h, int form);
int nnlm_comm_info(nnlm_handle *h, int *rank, int *nranks);
/* Contraction range [begin, end) owned by `rank` of `nranks`: rows i of A for the H half-step (which = 1), columns j
 * for the W half-step (which = 0).  Pure function of the sizes (no device needed). */
int nnlm_shard_range(int n, int m, int precision, int which, int rank, int nranks, int *begin, int *end);
/* Columns [col0, col1) of the factor being solved (m columns of H for which = 1, n rows of A = columns of W^T for which = 0) that
 * `rank` solves, and the width cpr of the packed slab [k][cpr] every rank contributes to the all-gather.  Pure function. */
int nnlm_shard_cols(int ncols, int rank, int nranks, int *cpr, int *col0, int *col1);
/* Test hook: partial [Gram k x k | cross product k x cols] of this (virtual) rank's slab, column-major, before the
 * all-reduce and before the regularisation edits of src/update_with_missing.cpp:20-24. */
int nnlm_debug_partial(nnlm_handle *h, int which, double *G_out, double *C_out);

/* Test hooks for virtual ranks (several handles in one process, nnlm_comm_init(h, NULL, r, P)): nnlm_debug_phase runs ONE
 * phase of a sharded half-step -- 1: cross product + Gram of the rank's contraction slab folded into [G | C];
 * 2: sweep of the rank's columns into its packed slab; 3: unpack of the gathered slabs -- and nnlm_debug_exchange does,
 * through the host, what ncclAllReduce (stage 1) / ncclAllGather (stage 2) do between them on a real node. */
int nnlm_debug_phase(nnlm_handle *h, int which, int phase, const double reg[3], unsigned inner_max_iter,
                     double inner_rel_tol, int method);
int nnlm_debug_exchange(nnlm_handle **handles, int nranks, int which, int stage);
/* The nnlm_debug_* entries are TEST HOOKS, not part of the production surface: process-global (atomic) settings read once per
 * nnlm_create / allocation, never to be changed while another thread creates handles.
 * Test hook: handles created from now on plan their launches as if the device had `cus` compute units (0 = the device's own
 * count) -- small problems then take the launch forms large ones take on the real device (persistent SCD sweep). */
int nnlm_debug_set_cus(int cus);
/* Test hook: handles created from now on launch xprod16_tn_kernel (the split-fp16 cross product) with `waves` = 8 or 10 wavefronts per
 * block -- 128- or 160-column tiles -- wherever that form exists (10: ranks up to 52); 0 = the launch plan decides. */
int nnlm_debug_set_xprod_waves(int waves);
/* Test hook: cache policy of the stream of A in the A-streaming cross products (xprod16_tn_kernel, xprod16_err_kernel, xprod_tn_kernel)
 * of handles created from now on.  The requests for A of the contraction stages >= nt_from_stage (the global stage index: 64 fp32-mode /
 * 32 strict-mode contraction elements each) are non-temporal: 0 = all of A, INT_MAX = none, -1 = the library's choice.  Values below -1
 * are refused.  A cache policy changes no value: results are bit-identical for every setting. */
int nnlm_debug_set_a_stream(int nt_from_stage);
/* The launch plan of one xprod16_tn_kernel launch: ldc output columns (a multiple of 128), `stages` contraction stages of 64 elements,
 * rank k <= 64, `cus` compute units, force_waves as nnlm_debug_set_xprod_waves.  Pure function, works without a GPU.
 * out[0..6] = wavefronts per block, split-K slabs S, stages per slab, tiles, blocks (tiles x S), 4-row pieces of the factor image a
 * stage loads (all 4 ceil(k / 16); 13 at k = 49 .. 52), LDS bytes of a block; out[7] = 0. */
int nnlm_xprod_plan(int ldc, int stages, int k, int cus, int force_waves, int out[8]);
/* Which KL solver (methods 3 and 4) a dense half-step with a contraction of length p takes at rank k in arithmetic mode `precision`, with
 * mask_words 64-bit mask words per column of the solved factor (0: no mask), when its matrix-sized workspaces fit (the fallbacks on a
 * failed allocation -- own starting states, streaming -- are run-time answers and not part of the plan).  Pure function, works without a
 * GPU.  out[0] = kernel: 0 kl_tile_kernel with two row buffers, 1 kl_tile_kernel with one row buffer, 2 kl_reg64_kernel, 3
 * kl_stream_kernel; out[1] = exact pieces per thread (16-byte pieces of the contraction: 4 floats / 2 doubles x 512 threads); out[2] = the
 * instantiated piece count that runs (kl_reg64_kernel rounds up to 1, 2, 3, 5, 7, 10, 12, 14, 16, 18, 20); out[3] = columns per block;
 * out[4] = dynamic LDS bytes of a block; out[5] = wavefronts of a block (of 8) that own a last instantiated piece holding data;
 * out[6] = out[7] = 0.  Streaming: out[1..3] = out[5] = 0. */
int nnlm_kl_plan(int p, int k, int precision, int mask_words, int out[8]);
/* Test hook: the matrix-sized workspaces of the KL solvers (starting states of all columns, transposed copy of A, streaming scratch)
 * "do not fit" when they exceed `bytes` (0 = no limit): the half-step then takes its smaller-footprint path -- the streaming kernel
 * over column chunks -- exactly as it does when hipMalloc itself says no. */
int nnlm_debug_alloc_limit(size_t bytes);
/* Test hook: while `on` is not 0, a per-column Gram buffer (missing values: the dense path's buffer of one KP x KP block per column, the
 * chunk buffer of the sparse doors whose absent entries are missing or weighted) is filled with 0xFF bytes -- every double a NaN -- when
 * it is allocated, on the handle's stream, ahead of its first use.  The Gram kernels write the upper triangle up to k of a block and
 * nothing else; results must not depend on what the rest holds.  Off (the default) it costs one branch per allocation. */
int nnlm_debug_poison_workspaces(int on);
/* Facts about the handle's last launches, for bench.py's kernel attribution: key = "cus" (compute units the launch policy
 * counts), "xprod_waves_w" / "xprod_waves_h" and "xprod_splits_w" / "xprod_splits_h" (wavefronts per block and split-K slabs of the last
 * xprod16_tn_kernel launch of the W / H half-step, 0 none yet), "xprod_splits_err" (slabs of the last xprod16_err_kernel launch, 0 none yet),
 * "a_stream_nt_from" (the nt_from_stage -- see nnlm_debug_set_a_stream -- the last A-streaming cross-product launch was given, -1 none yet), "sweep_form_w" / "sweep_form_h" (SCD sweep of the last W / H half-step: 0 plain sweep_scd_q_kernel, 1 persistent
 * sweep_scd_qw_kernel -- both strict fp64 --, 2 sweep_scd_f_kernel, 3 sweep_row_kernel (fp32-operand mode: 3 while the launch is one
 * round of four-column wavefronts, at most 32 columns per CU), -1 none yet), "sweep_groups_w" /
 * "sweep_groups_h" (column groups -- form 2: wavefronts -- per workgroup of that launch), "lee_lanes_w" / "lee_lanes_h" and
 * "lee_regs_w" / "lee_regs_h" (Lee's multiplicative updates at ranks up to 64: lanes per column L -- 4, 2 or 1, chosen from the END column
 * of the launch -- and coordinate registers per lane R of the sweep_ls_kernel<R, L, 2> launch of the last W / H half-step, -1 none
 * yet), "na_solver_w" / "na_solver_h" (square loss with missing values -- every column solves with a Gram of its own --: family of the last
 * per-column solver launch of the W / H half-step: 0 colsolve_row_kernel, 1 colsolve_strict_kernel, 2 colsolve_ls_kernel, 3
 * sweep_generic_kernel with per-column Grams (rank > 64), -1 none yet), "na_solver_kr_w" / "na_solver_kr_h" (the KR of that instantiation;
 * colsolve_ls_kernel: 16 NKQ; sweep_generic_kernel: k), "na_gram_w" / "na_gram_h" (family of the last per-column Gram launch of the W / H
 * half-step: 0 na_gram_f16_kernel, 1 na_gram_lds_kernel, 2 na_gram_lds_kernel in its tail form, 3 sp_gram_kernel, 4
 * na_gram_generic_kernel, -1 none yet), "na_gram_nt_w" / "na_gram_nt_h" (the NT / NKQ of that instantiation),
 * "kl_form_w" / "kl_form_h" (KL solver of the last W / H half-step: 0 kl_tile_kernel on the starting states of the wh_store GEMM, 1 kl_tile_kernel forming its own starting states
 * -- no room for the matrix-sized buffer --, 2 kl_reg64_kernel (strict), 3 kl_stream_kernel over column chunks, -1 none yet),
 * "kl_pieces_w" / "kl_pieces_h" and "kl_cols_w" / "kl_cols_h" (instantiated pieces per thread and columns per block of the kl_tile_kernel
 * or kl_reg64_kernel launch of the last W / H half-step -- out[2] and out[3] of nnlm_kl_plan --, 0 when it streamed, -1 none yet),
 * "matrix_nnz" (non-zeros of a sparse matrix, -1 for a dense one), "matrix_bytes" (device bytes the resident matrix occupies),
 * "matrix_min_col_observed" / "matrix_min_row_observed" (dense matrix: the fewest observed -- finite -- entries of any column / any row,
 * n / m without missing entries; counted on the device at the first query; -1 on a sparse handle loaded from host arrays; on one loaded
 * by nnlm_set_matrix_sparse_device the fewest stored entries of a column / row when absent entries are missing, else n / m),
 * "sp_ingest_check_share" / "sp_ingest_sort_tile" (stored entries per workgroup of the entry check and of a radix pass of
 * nnlm_set_matrix_sparse_device: constants of the build), "debug_sparse_values_address" (TEST HOOK: the device address of the resident
 * by-column values of a sparse handle -- exact in a double --, -1 without one: a buffer of the handle for the aliasing rule's tests),
 * "matrix_absent_missing" (1 after nnlm_set_matrix_csc_missing, else 0), "sp_gram_chunks" / "sp_gram_bytes" (column chunks of the last
 * half-step on such a handle, device bytes of the per-column Gram buffer), "sp_workers" (workers -- groups of 16, 32 or 64 lanes, each
 * owning a range of non-zeros -- of one spmm_kernel launch on the resident sparse matrix at the current rank, 0 without one),
 * "sp_gram_workers" (sp_gram_kernel workers of the last half-step whose absent entries are missing, summed over its column chunks),
 * "sp_gram_batch_pairs" (upper 16 x 16 tile pairs of the stacked Gram that the sp_gram_batch_kernel launches of the last batch half-step
 * on a handle loaded by nnlm_set_matrix_csc_missing_batch formed: those meeting an ACTIVE member's diagonal block; 0 none yet),
 * "sparse_batch" (1 after nnlm_set_matrix_csc_batch, nnlm_set_matrix_csc_missing_batch or nnlm_set_matrix_csc_kl_batch, else 0), "sp_batch_waves" (wavefronts of one sp_batch_errors_kernel launch on the
 * resident sparse matrix -- a function of its non-zeros and the CU count only --, 0 without one), "sparse_kl" (1 after nnlm_set_matrix_csc_kl, else 0), "sparse_kl_form_w" / "sparse_kl_form_h" (KL solver forms of the last W / H half-step on
 * such a handle: bit 0 = sp_kl_solve_kernel ran, a wavefront per line of at most "sparse_kl_short_max" stored entries; bit 1 =
 * sp_kl_solve_long_kernel ran, a workgroup per longer line; -1 none yet), "sparse_kl_batch" (1 after nnlm_set_matrix_csc_kl_batch, else
 * 0), "sparse_kl_batch_form_w" / "sparse_kl_batch_form_h" (forms of the last batched KL W / H half-step: bit 0 = sp_kl_batch_kernel ran,
 * one launch over the short lines for all active members; bit 1 = sp_kl_solve_long_kernel ran once per active member; -1 none yet),
 * "sparse_kl_batch_group" (member chains a wavefront of sp_kl_batch_kernel interleaves: 1, 2 or 4; the library's default, or the value of
 * the environment variable NNLM_SPKL_BATCH_GROUP when the handle was created -- results do not depend on it, only the time). */
int nnlm_get_info(nnlm_handle *h, const char *key, double *value);

#ifdef __cplusplus
}
#endif
#endif /* NNLM_MI355X_H */
