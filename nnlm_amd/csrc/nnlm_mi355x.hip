// nnlm_mi355x.hip -- host side of libnnlm_mi355x.so: device-resident state (nnlm_handle), kernel
// launches for one half-step, the alternating driver restating c_nnmf / c_nnlm, and the C ABI of
// include/nnlm_mi355x.h.  gfx950 only; no CPU fallback: every entry fails with NNLM_ERR_HIP when no
// device is present.
//
// Reference map (relative to /root/reference):
//   nnlm_c_nnmf      <- c_nnmf            src/nnmf.cpp:4-220
//   nnlm_c_nnlm      <- c_nnlm            src/nnlm.cpp:4-53
//   half_step()      <- update()          src/update_with_missing.cpp:3-55
//                       update_with_missing()  src/update_with_missing.cpp:58-139
//   penalties()      <- add_penalty()     src/nnmf.cpp:224-240
#include "../../include/nnlm_mi355x.h"
#include "common.h"
#include "k_batch.h"
#include "k_errors.h"
#include "k_generic.h"
#include "k_gram.h"
#include "k_ingest.h"
#include "k_kl.h"
#include "k_missing.h"
#include "k_prep.h"
#include "k_sweep.h"
#include "k_sweep_q.h"
#include "k_xprod.h"
#include "k_xprod16.h"
#include "tu_sweepq.h"
#include "tu_svd.h"
#include "tu_topn.h"

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

static thread_local std::string g_last_error;

enum ProfId { P_XPROD_H = 0, P_XPROD_W, P_GRAM, P_SWEEP_H, P_SWEEP_W, P_ERRORS, P_XPROD_W_ERR, P_ALLGATHER, P_ALLREDUCE, P_UNPACK, P_ERR_REDUCE,
              P_SPMM_H, P_SPMM_W, P_SP_ERRORS, P_BATCH_ERRORS, P_BATCH_PEN, P_SP_GRAM, P_INGEST, P_TOPN, P_TOPN_MERGE, P_PREDICT_ENTRIES, P_TOPN_EVAL,
              P_SPKL_COPY, P_SPKL_H, P_SPKL_W, P_SP_BATCH_ERRORS, P_SPKL_BATCH_H, P_SPKL_BATCH_W,
              P_SP_INGEST, P_SP_INGEST_PTR, P_SP_INGEST_CHECK, P_SP_INGEST_BUILD, P_COUNT };
// ("xprod_w_err": W half-step cross products that also evaluate the error sums -- the fused launches have a scope of their own;
//  "allgather" / "allreduce": the RCCL collective of a sharded half-step between two events on the stream it is enqueued on;
//  "unpack": shard_unpack_kernel + the sum of the ranks' Gram partial sums behind it)
//  "errors": a separate pass over A (errors_f32_kernel / errors64_kernel + its reduction); "err_reduce": the reduction of the partial sums the
//  fused cross product left behind -- 5 us, no HBM work: it must not be priced as a pass over A
//  "spmm_h" / "spmm_w": the cross products of a sparse A (row copy of the fixed factor + spmm_kernel + its fix-up); "sp_errors": the error
//  block of a sparse A (sums over the non-zeros, the two Grams and the factors' sums)
//  "batch_errors": the error block of a batched factorisation (errors_batch_kernel + its reduction: one pass over A for all members);
//  "batch_pen": its per-member penalty sums; "sp_gram": the per-column Grams of a sparse A whose absent entries are missing (sp_gram_kernel
//  + its fix-up, both half-steps); "ingest": the ingest kernels of nnlm_set_matrix_device (k_ingest.h), without the common tail
//  "topn" / "topn_merge" / "predict_entries": topn_kernel, topn_merge_kernel and predict_entries_kernel alone (k_topn.h; the row copies
//  and the transfers around them are not in it); "topn_eval": the kernels of nnlm_top_n_eval behind them (topn_eval_kernel + its reduction
//  per round, topn_eval_overlap_kernel once)
//  "spkl_copy": the row copy and the column sums of the fixed factor of a KL half-step on a sparse A; "spkl_solve_h" / "spkl_solve_w": its
//  solver launches (k_sparse_kl.h: starting states in the prologue, short and long form)
//  "sp_batch_errors": the error block of a batched factorisation on a sparse A (k_sparse_batch.h: the row copies, the stacked Grams and
//  coordinate sums, ONE sp_batch_errors_kernel launch over the non-zeros for all members, its reduction and the closing kernel)
//  "spkl_batch_h" / "spkl_batch_w": the solver launches of a batched KL half-step on a sparse A (k_sparse_kl_batch.h: ONE launch over the
//  short lines for all active members, then the long form once per active member); its row copy and column sums are in "spkl_copy"
//  "sp_ingest": nnlm_set_matrix_sparse_device from its first kernel to its last copy (k_sparse_ingest.h; the host's waits for the verdicts
//  between the stages are inside it); "sp_ingest_ptr" / "sp_ingest_check" / "sp_ingest_build": the kernels of its stages alone -- the
//  pointer check, the entry check with the conversions, the index histogram + its scan + the radix passes
static const char *kProfNames[P_COUNT] = {"xprod_h", "xprod_w", "gram", "sweep_h", "sweep_w", "errors", "xprod_w_err", "allgather", "allreduce", "unpack", "err_reduce",
                                          "spmm_h", "spmm_w", "sp_errors", "batch_errors", "batch_pen", "sp_gram", "ingest", "topn", "topn_merge", "predict_entries", "topn_eval",
                                          "spkl_copy", "spkl_solve_h", "spkl_solve_w", "sp_batch_errors", "spkl_batch_h", "spkl_batch_w",
                                          "sp_ingest", "sp_ingest_ptr", "sp_ingest_check", "sp_ingest_build"};

// A chunk of the columns of a sparse-missing half-step whose Grams are held at once (nnlm_handle::spg_plan): columns [c0, c1), long
// columns longc[l0 .. l1)
struct SpgChunk {
    int c0, c1, l0, l1;
};

struct ProfRec {
    int id;
    hipEvent_t e0, e1;
};

struct nnlm_handle {
    int device = 0;
    int cus = 256;              // compute units of the device (sweep launch policy: one wavefront of the SCD sweep per SIMD, 4 SIMDs per CU)
    int sweep_wgs = 0;          // workgroups of the last sweep_scd_q(w)_kernel launch = Gram partial-sum slabs it left behind
    int cur_which = 1;          // the half-step in progress (0: W, 1: H)
    int kl_pieces[2] = {-1, -1}, kl_cols[2] = {-1, -1}; // per half-step: instantiated pieces per thread and columns per block of its last kl_tile_kernel / kl_reg64_kernel launch (0 streaming)
    int kl_form[2] = {-1, -1}; // per half-step: its last KL solver launch (0 tile kernel on the GEMM's states, 1 tile kernel on its own states, 2 strict register kernel, 3 streaming)
    int sweep_form[2] = {-1, -1}, sweep_groups[2] = {0, 0}; // per half-step (0: W, 1: H): form of its last SCD sweep launch (0 plain, 1 persistent) and
                                                             // column groups per workgroup (nnlm_get_info)
    int lee_lanes[2] = {-1, -1}, lee_regs[2] = {-1, -1};    // per half-step: L and R of its last sweep_ls_kernel<R, L, 2> launch (nnlm_get_info)
    // per half-step, the last launches with per-column Grams (missing values; nnlm_get_info "na_solver_*", "na_gram_*"): the solver's family
    // (0 colsolve_row_kernel, 1 colsolve_strict_kernel, 2 colsolve_ls_kernel, 3 sweep_generic_kernel) and KR, the Gram kernel's family
    // (0 na_gram_f16_kernel, 1 na_gram_lds_kernel, 2 its tail form, 3 sp_gram_kernel, 4 na_gram_generic_kernel) and NT / NKQ
    int na_solver[2] = {-1, -1}, na_solver_kr[2] = {-1, -1}, na_gram[2] = {-1, -1}, na_gram_nt[2] = {-1, -1};
    int prec = NNLM_PREC_F32;
    hipStream_t stream = nullptr;   // main: cross products, solvers
    hipStream_t stream_e = nullptr; // error block, concurrent with the (speculative) next W half-step
    hipEvent_t ev_hdone = nullptr, ev_err = nullptr, ev_xdone = nullptr;
    std::string err;

    // problem
    int n = 0, m = 0, npad = 0, mpad = 0;
    void *A = nullptr;          // T [mpad][npad]
    uint32_t *miss = nullptr;   // [mpad][npad/32]
    uint32_t *missT = nullptr;  // [npad][mpad/32], only when any_missing
    bool any_missing = false;
    bool dense_cols = true;     // multi-GPU form of the dense square-loss half-step (half_step): column-sharded (true) or all-reduce
    int upk_max_for = -1;       // multi-GPU: the half-step (0: W, 1: H) whose unpack left max|factor| in maxbits[6 + which], or -1
    int gshard_for = -1;        // multi-GPU: the factor (0: W, 1: H) whose Gram the last unpack summed into Graw from the ranks' partial sums, or -1
    int y16_for = -1;           // multi-GPU: the factor whose split-fp16 copy (and exponent, scal_exp[1]) the last unpack left in Y16, or -1
    size_t pack_tail = 0;       // doubles behind the k x cpr slab in the packed payload of the current half-step (KP * KP Gram partial sums, or 0)
    unsigned *fixed_maxw = nullptr; // word holding max|fixed factor| of the half-step in progress (split-fp16 copies)
    double n_non_missing = 0.0, kl_const = 0.0;
    int min_obs[2] = {-2, -2};  // fewest observed entries of a column / of a row (nnlm_get_info; observed_min_kernel on first query), -2 = not yet

    // factors
    int k = 0, NKQ = 0, KP = 0, KP8 = 0;
    double *W64 = nullptr, *H64 = nullptr;        // [KP][npad], [KP][mpad]  (W64 = W64b[wcur])
    void *Wop = nullptr;                          // T [KP][npad] (aliases W64 in f64 mode)  (Wop = Wopb[wcur])
    double *W64b[2] = {nullptr, nullptr};         // W is double buffered: every W half-step writes the other buffer, so a
    void *Wopb[2] = {nullptr, nullptr};           // speculative half-step can be dropped and the error block can read W_i
    int wcur = 0;
    float *Hkq = nullptr;                         // fp32 [KP][mpad] copy of H, refreshed by nnlm_errors (f32 mode)
    unsigned long long *Wmask = nullptr, *Hmask = nullptr; // [npad][MW], [mpad][MW]: bit q of a column's words = entry (q, col) is masked
    bool has_wmask = false, has_hmask = false;
    int MW = 1;                                   // 64-bit mask words per column = ceil(k / 64)
    void *AT = nullptr;                           // T [npad][mpad]: contraction-contiguous copy of A for the W half-step of the paths that
                                                  // stream it with the TN kernels (rank > 64) or per column (KL, F32 mode); made on first use
    double *klsw = nullptr, *klsw_cols = nullptr; // KL: row sums of the fixed factor [KP] / per column over its non-missing entries [cols][KP]
    void *klst = nullptr;                         // kl_stream_kernel: [cols][2][ld] state vectors + data columns
    size_t klst_bytes = 0;
    bool what_tight = false;                      // the matrix-sized What / What64 could not be had for this matrix (not retried every half-step)
    bool klst_tight = false;                      // the full-size streaming scratch could not be had: the chunked one is kept
    bool at_tight = false;                        // the transposed copy AT could not be had (soft request of the KL solvers)

    // workspaces
    double *Cx = nullptr;
    size_t Cx_elems = 0;
    double *gslabs = nullptr, *Graw = nullptr; // Graw = head of red
    double *red = nullptr;               // [KP*KP | KP*max(npad,mpad)]: the buffer one all-reduce sums
    // NA path: per orientation (0: rows of A for the W half-step, 1: columns for the H half-step) the CSR lists of the rows a
    // column's Gram sums over (k_missing.h); built on first use, they live as long as the matrix
    uint32_t *na_ptr[2] = {nullptr, nullptr}, *na_meta[2] = {nullptr, nullptr};
    int *na_idx[2] = {nullptr, nullptr};
    double *Yrow = nullptr;              // [max(npad,mpad)][KP] row-major copy of the fixed factor (NA path)
    double *Gcols = nullptr;             // [max(n,m)][KP][KP] per-column Grams (NA path): upper triangle only at rank <= 64 (na_gram_f16 /
                                         // na_gram_lds write it, the colsolve kernels read G[min][max]); the full matrix for the generic
                                         // rank > 64 kernels (na_gram_generic_kernel, sweep_generic_kernel)
    double *partials = nullptr;
    size_t partials_elems = 0;
    double *scal = nullptr;              // 16 doubles of reduction results
    // sparse A (nnlm_set_matrix_csc, k_sparse.h): CSC and the CSR of the same matrix, values in the mode's type; nothing n x m sized exists
    // on such a handle (A, miss, A16, AT, What stay NULL) and x16 is off
    bool sparse = false;
    long long nnz = 0;
    long long *sp_cptr = nullptr, *sp_rptr = nullptr; // [m + 1], [n + 1]
    int *sp_ridx = nullptr, *sp_cidx = nullptr;       // row of each CSC entry, column of each CSR entry (ascending within a column / row)
    void *sp_cval = nullptr, *sp_rval = nullptr;      // values, fp32 (F32 mode) or fp64
    size_t sp_bytes = 0;                              // device bytes of the six arrays
    void *sp_Y = nullptr;                             // [max(npad, mpad)][KP] row copy of the fixed factor (mode's type)
    double *sp_carry = nullptr;                       // [spmm workers][64] heads of the columns that straddle a worker boundary
    double *sp_Wrow = nullptr;                        // error block: [npad][KP] fp64 rows of W
    double *sp_eslabs = nullptr;                      // error block: Gram partial sums
    double *sp_eG = nullptr;                          // error block: W^T W, H H^T [KP][KP] each, W's and H's sums over i / j [KP] each, S1..S3
    double *sp_epart = nullptr;                       // error block: per-workgroup partial sums
    // sparse A whose absent entries are MISSING (nnlm_set_matrix_csc_missing, k_sparse_na.h).  Per orientation (0: W half-step over the
    // CSR, 1: H half-step over the CSC), made with the matrix: the host copy of the pointers, the Gram slots of the long columns in front
    // of each column (segoff) and the list of the long columns.  Per orientation and budget: the column chunks whose Grams are held at
    // once; the buffer they share (freed with the factors)
    bool sp_missing = false;
    // per-entry weights on the stored entries (nnlm_set_matrix_csc_weighted): the handle of the unweighted door for the same absent
    // semantics, plus the weights and the premultiplied values c_e a_e in both orientations (mode's type) and the per-orientation
    // tables of the per-column path, which every square-loss half-step of such a handle takes (half_step_sparse_missing)
    bool sp_weighted = false;
    void *sp_cwt = nullptr, *sp_rwt = nullptr; // weights, CSC / CSR order
    void *sp_cwa = nullptr, *sp_rwa = nullptr; // c_e a_e, CSC / CSR order
    // sparse A loaded for KL loss (nnlm_set_matrix_csc_kl, k_sparse_kl.h): a sparse handle whose methods 3 and 4 run.  Per orientation (0: rows
    // of A for the W half-step, 1: columns for the H half-step) the lines of more than SPKL_SHORT_MAX stored entries, on the device
    bool sp_kl = false;
    // sparse A loaded for the batched factorisation (nnlm_set_matrix_csc_batch): the ordinary sparse handle (absent entries zeros) that
    // nnlm_set_factors_batch / nnlm_run_batch also accept (batch_refusal)
    bool sp_batch = false;
    int *spkl_longc[2] = {nullptr, nullptr};
    int spkl_nlong[2] = {0, 0}, spkl_nshort[2] = {0, 0};
    void *spkl_state = nullptr;     // [nnz] states of the long lines' entries (mode's type), on first use
    int spkl_form[2] = {-1, -1};    // per half-step: forms of its last KL launch (bit 0 short, bit 1 long; nnlm_get_info)
    int spklb_form[2] = {-1, -1};   // the same of its last BATCHED KL launch (bit 0: sp_kl_batch_kernel, bit 1: per-member long launches)
    int spklb_group = nnlm_spkl_batch_group(); // member chains a wavefront of sp_kl_batch_kernel interleaves
    std::vector<long long> spg_hptr[2];
    long long *spg_segoff[2] = {nullptr, nullptr};
    int *spg_longc[2] = {nullptr, nullptr};
    std::vector<SpgChunk> spg_plan[2];
    size_t spg_plan_cap[2] = {0, 0}, spg_plan_slots[2] = {0, 0}; // Gram slots per chunk: allowed, and taken by the largest chunk (columns + segments)
    double *spg_buf = nullptr;
    size_t spg_buf_bytes = 0;
    int spg_chunks = 0; // chunks of the last such half-step (nnlm_get_info "sp_gram_chunks")
    int spg_workers = 0; // sp_gram_kernel workers of that half-step, summed over its chunks (nnlm_get_info "sp_gram_workers")
    unsigned long long *sweeps = nullptr; // [2] device counters; sw_active = the one the current trace window sums into
    int sw_active = 0;
    double *host_res = nullptr;           // pinned: 8 reduction results + sweep counter of the asynchronous error block

    // multi-GPU
    int rank = 0, nranks = 1;
    void *comm = nullptr;
    bool sharded = false;       // nranks > 1, or a real 1-rank communicator (exercises the sharded code path on one GPU)
    double *pack_send = nullptr; // [KP][cpr]: this rank's updated columns, contiguous for ncclAllGather
    double *pack_all = nullptr;  // [nranks][KP][cpr]
    size_t pack_elems = 0;
    double *sweepq_img = nullptr;             // operand image of sweep_scd_q_kernel (k_sweep_q.h), rewritten every half-step
    // split-fp16 cross products (k_xprod16.h; F32 mode, single GPU): A16 [mpad][npad], A16T [npad][mpad], Y16 [KP][max(npad,mpad)]
    bool x16 = false;
    uint32_t *A16 = nullptr, *A16T = nullptr, *Y16 = nullptr;
    unsigned *maxbits = nullptr; // device [16]: bit patterns of max|factor|: [0] absmax_f64_kernel, [1],[2] alternately gram_partial_kernel, [3] block counter, [6],[7] shard_unpack_kernel (W, H),
                                 // [11] a batch member's own rows of the fixed factor (hold-out handle), [4],[5] alternately the fast sweep kernel's own max of what it solved (k_sweep_q.h), [8] the same for a rank's
                                 // column shard (travels behind its packed slab: gram_fold_tail_kernel clears it)
    // What the fast sweep leaves behind for the next half-step (dense one-GPU split-fp16 path): max|x| in maxbits[4 + sg_par] and
    // sg_nslabs Gram partial sums (one per workgroup) in sg_slabs.  sg_which: the factor they describe (1 = H, 0 = W, -1 = none).
    int sg_which = -1, sg_par = 0, sg_nslabs = 0;
    int sg_other = -1;           // the factor whose max the OTHER word (maxbits[4 + (sg_par ^ 1)]) still holds, or -1
    int sg_prev = -1;            // sg_which as the current half-step found it (becomes sg_other after its sweep)
    bool sg_request = false;     // set by half_step for the sweep it is about to launch
    double *sg_slabs = nullptr;
    int mb_par = 0;
    bool pack_ready = false;     // sweepq_img already produced for this half-step (the one-stream dense flow packs it ahead of the cross product)
    int *scal_exp = nullptr;     // device: {eA, eY, eW of the fused error block}
    float *What = nullptr;       // [mpad][npad] fp32 W^T H: starting state vectors of a KL half-step (wh_store_kernel), on first use
    double *What64 = nullptr;    // the same in fp64 for the strict mode (wh_store64_kernel)
    uint32_t *W16c = nullptr, *H16c = nullptr; // kq-contiguous split copies [npad][2][64], [mpad][2][64] (fused error block)
    bool fuse_err = false;       // request: the next W half-step's cross product also evaluates the error sums of (W, H) now current
    int cus_device = 0;          // the device's CU count (cus may be the test hook's)
    int xprod_waves = 0;         // test hook (nnlm_debug_set_xprod_waves): block width of xprod16_tn_kernel, 0 = the plan decides
    int a_stream = -1;           // test hook (nnlm_debug_set_a_stream): first stage whose A requests are non-temporal, -1 = the library's choice (a_stream_nt)
    int a_stream_last = -1;      // what the last A-streaming cross-product launch was given (-1 = none yet)
    int xp_err_splits = 0;       // slabs of the last xprod16_err_kernel launch
    int xp_waves[2] = {0, 0}, xp_splits[2] = {0, 0}; // [which]: wavefronts per block and slabs of the last xprod16_tn_kernel launch
    int fused_nb = 0;            // answer: number of (sum of squares, KL) pairs it left in `partials` (0 = not fused)
    // multi-GPU: the error block of a trace iteration is enqueued from INSIDE the speculative W half-step, right behind its cross product:
    // its all-reduces (two sums, one sweep counter) must be issued ahead of that half-step's all-gather -- RCCL runs a communicator's
    // collectives in issue order, and behind the all-gather the host would learn the stopping decision only when the whole half-step is done
    bool err_hook = false, err_need_pen = true, err_launched = false;
    unsigned *err_zero_word = nullptr; // the fused kernel clears this word (max|x| of the sweep that follows it; see factor16_fold_err_kernel)
    unsigned long long *sweeps_tmp = nullptr; // device scratch for the all-reduced sweep counter

    // batched factorisation (nnlm_set_factors_batch): bB members stacked in the factor buffers, member b owns rows boff[b] .. boff[b+1]-1;
    // the factor buffers then carry row_pad zero rows behind their KP (the per-member Gram kernels read 16 ceil(k_b / 16) rows from off_b)
    int bB = 0, row_pad = 0;
    std::vector<int> bk, boff;
    int *boff_dev = nullptr;                // [bB + 1]
    double *bG = nullptr;                   // [bB][64 * 64] per-member Grams
    unsigned long long *bsweeps = nullptr;  // [bB] per-member sweep counters
    double *bpart = nullptr;                // partial sums of the batched error block / penalties
    size_t bpart_elems = 0;
    double *bres = nullptr;                 // [8 bB]: {sum sq, sum KL} per member, then 3 W and 3 H penalty sums per member
    double *bsp_Hrow = nullptr;             // sparse A: [m][KP] fp64 rows of H (the rows of W: sp_Wrow), error block
    double *bsp_part = nullptr;             // sparse A: [3 bB][workgroups] partial sums of sp_batch_errors_kernel, then [3 bB] their sums
    int bspg_pairs = 0;                     // sparse A, absent = missing: tile pairs the last half-step's sp_gram_batch_kernel launches formed
                                            // (nnlm_get_info "sp_gram_batch_pairs")

    // hold-out set (nnlm_set_matrix_holdout): the resident matrix is A with NA at the pattern (the dense NA layout
    // above); the held-out entries themselves stay here as a CSC -- values in the mode's type, the column of every entry beside its row
    bool holdout = false;
    long long ho_nnz = 0;
    long long *ho_cptr = nullptr; // [m + 1]
    int *ho_ridx = nullptr, *ho_cidx = nullptr;
    void *ho_val = nullptr;

    int topn_slices = 0; // candidate slices of the last topn_kernel launch (nnlm_get_info "topn_slices")
    long long topn_eval_lines = 0; // evaluated lines of the last nnlm_top_n_eval (nnlm_get_info "topn_eval_lines")

    // truncated SVD of the resident matrix (nnlm_svd): the leading svd_l triplets, one row per triplet as the factor
    // masters keep their components; they live as long as the matrix.  svd_l = 0: none
    int svd_l = 0, svd_LP = 0, svd_kept = 0; // sketch width, its padding to 16, directions the last orth kept
    double *svdU = nullptr, *svdVt = nullptr; // [svd_LP][npad], [svd_LP][mpad]
    std::vector<double> svd_sigma;            // [svd_l], descending
    double svd_mean = 0.0;                    // mean(A) over all n m entries, from the resident values (the nndsvda fill)
    bool svd_mean_known = false;
    double svd_ms[7] = {0};                   // host milliseconds of the last nnlm_svd: cross products, Grams, rotations, host eigendecompositions,
                                              // waits and transfers, the whole call, setting and freeing the rank-l factor buffers (the device's
                                              // share is in the first three only with profiling on)
    int svd_form = -1;                        // form of the last rotation (nnlm_svd_rotate_form), -1 none yet

    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    double prof_ms[P_COUNT] = {0};
    long long prof_n[P_COUNT] = {0};
};

// Dynamic LDS beyond 64 KB must be granted per kernel.  The launch helpers are void: a refusal is remembered here and reported by the
// next LAUNCHCHK (every half-step / error block ends with one), together with whatever the launch itself then raised.  The latch is
// per thread, not per handle: fail() and every public entry that launches clear it, so a refusal never outlives the call it
// happened in and is never reported against another handle's launch.
static thread_local hipError_t g_attr_err = hipSuccess;
static thread_local const char *g_attr_what = "";

static int fail(nnlm_handle *h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (h) h->err = buf;
    g_attr_err = hipSuccess; // (a refused attribute latched on the way here belongs to this failure, not to a later launch)
    return code;
}

// What a handle with per-entry weights (nnlm_set_matrix_csc_weighted) does not do: square loss, methods 1 and 2, rank <= 64, one fit
static int weighted_refusal(nnlm_handle *h, const char *who, const char *what)
{
    return fail(h, NNLM_ERR_UNSUPPORTED, "%s: %s is not supported on a matrix with per-entry weights (nnlm_set_matrix_csc_weighted: square loss, "
                                         "methods 1 and 2, rank <= %d, single fits on one GPU)", who, what, NNLM_KQ_MAX);
}

template <typename... P>
static bool any_null(const P *...p) { return (... || !p); }

#define HIPCHK(h, call)                                                                                              \
    do {                                                                                                             \
        hipError_t e__ = (call);                                                                                     \
        if (e__ != hipSuccess) return fail(h, NNLM_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

static inline void set_dyn_lds(const void *fn, int lds, const char *what)
{
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess && g_attr_err == hipSuccess) {
        g_attr_err = e;
        g_attr_what = what;
    }
}
#define LAUNCHCHK(h)                                                                                                              \
    do {                                                                                                                          \
        if (g_attr_err != hipSuccess) {                                                                                           \
            const hipError_t ea__ = g_attr_err;                                                                                   \
            g_attr_err = hipSuccess;                                                                                              \
            (void)hipGetLastError();                                                                                              \
            return fail(h, NNLM_ERR_HIP, "hipFuncSetAttribute(%s, MaxDynamicSharedMemorySize) failed: %s", g_attr_what, hipGetErrorString(ea__)); \
        }                                                                                                                         \
        HIPCHK(h, hipGetLastError());                                                                                             \
    } while (0)

// split-fp16 cross products (k_xprod16.h): THE cross products of the F32 mode
static bool x16_enabled(int precision) { return precision == NNLM_PREC_F32; }

static size_t esize(const nnlm_handle *h) { return h->prec == NNLM_PREC_F64 ? 8 : 4; }

// ---------------------------------------------------------------------------------------------
// profiling helpers
// ---------------------------------------------------------------------------------------------
struct ProfScope {
    nnlm_handle *h;
    ProfRec r;
    bool on;
    hipStream_t st;
    ProfScope(nnlm_handle *h_, int id, hipStream_t st_ = nullptr) : h(h_), on(h_->prof), st(st_ ? st_ : h_->stream)
    {
        if (on) {
            r.id = id;
            hipEventCreate(&r.e0);
            hipEventCreate(&r.e1);
            hipEventRecord(r.e0, st);
        }
    }
    ~ProfScope()
    {
        if (on) {
            hipEventRecord(r.e1, st);
            h->recs.push_back(r);
        }
    }
};

static void sync_all(nnlm_handle *h)
{
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->stream_e) hipStreamSynchronize(h->stream_e);
}

static void prof_collect(nnlm_handle *h)
{
    if (h->recs.empty()) return;
    sync_all(h);
    for (auto &r : h->recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
            h->prof_ms[r.id] += ms;
            h->prof_n[r.id] += 1;
        }
        hipEventDestroy(r.e0);
        hipEventDestroy(r.e1);
    }
    h->recs.clear();
}

// RCCL entry points, resolved lazily with dlopen (single-GPU runs never touch librccl)
struct Rccl {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
static Rccl g_rccl;

static int rccl_load()
{
    if (g_rccl.lib) return NNLM_OK;
    void *lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) return fail(nullptr, NNLM_ERR_COMM, "cannot load librccl: %s", dlerror());
    g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(lib, "ncclCommInitRank");
    g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(lib, "ncclAllReduce");
    g_rccl.AllGather = (decltype(g_rccl.AllGather))dlsym(lib, "ncclAllGather");
    g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(lib, "ncclCommDestroy");
    g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(lib, "ncclGetErrorString");
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.AllGather || !g_rccl.CommDestroy)
        return fail(nullptr, NNLM_ERR_COMM, "librccl lacks a required symbol");
    g_rccl.lib = lib;
    return NNLM_OK;
}

// ---------------------------------------------------------------------------------------------
// create / destroy
// ---------------------------------------------------------------------------------------------
extern "C" int nnlm_abi_version(void) { return NNLM_ABI_VERSION; }

extern "C" const char *nnlm_last_error(const nnlm_handle *h) { return h ? h->err.c_str() : g_last_error.c_str(); }

extern "C" unsigned nnlm_trace_capacity(unsigned max_iter, unsigned trace)
{
    if (trace < 1) trace = 1;
    return (unsigned)std::ceil((double)max_iter / (double)trace) + 1; // src/nnmf.cpp:53-54
}

static std::atomic<int> g_debug_cus{0}; // nnlm_debug_set_cus (test hook, read once per nnlm_create): compute units the launch policies of new handles count (0 = the device's)
static std::atomic<int> g_debug_a_stream{-1}; // nnlm_debug_set_a_stream (test hook, read once per nnlm_create): first contraction stage whose requests for A are non-temporal, -1 = the library's choice (a_stream_nt)
static std::atomic<int> g_debug_xprod_waves{0}; // nnlm_debug_set_xprod_waves (test hook, read once per nnlm_create): 8 | 10 wavefronts per block of xprod16_tn_kernel, 0 = the plan decides
// Pinned bounce buffers of nnlm_set_matrix, kept between calls.  Pinning costs ~0.3 ms per MB: two fresh 64 MB buffers were ~40 ms of EVERY
// upload (half of config 2's 78 ms, most of the 53 ms an 80 MB matrix took -- scripts/gpu_call_breakdown.py).  One pair per process, taken
// by the call that finds it free (a concurrent upload on another thread allocates its own and frees it), released at exit.
static std::mutex g_bounce_mu;
static double *g_bounce[2] = {nullptr, nullptr};
static size_t g_bounce_bytes = 0;
static bool g_bounce_busy = false, g_bounce_atexit = false;
static void bounce_release_at_exit()
{
    // (the HIP runtime may already be gone when exit handlers run: errors are ignored)
    for (int b = 0; b < 2; b++)
        if (g_bounce[b]) (void)hipHostFree(g_bounce[b]);
    g_bounce[0] = g_bounce[1] = nullptr;
    g_bounce_bytes = 0;
}
// both buffers of at least `bytes`, or false (none to be had / the pair is in use): *cached tells the caller whether to give them back
static bool bounce_acquire(size_t bytes, double *out[2], bool *cached)
{
    {
        std::lock_guard<std::mutex> lk(g_bounce_mu);
        if (!g_bounce_busy) {
            if (g_bounce_bytes < bytes) {
                for (int b = 0; b < 2; b++)
                    if (g_bounce[b]) (void)hipHostFree(g_bounce[b]);
                g_bounce[0] = g_bounce[1] = nullptr;
                g_bounce_bytes = 0;
                if (hipHostMalloc(&g_bounce[0], bytes) != hipSuccess || hipHostMalloc(&g_bounce[1], bytes) != hipSuccess) {
                    (void)hipGetLastError();
                    for (int b = 0; b < 2; b++)
                        if (g_bounce[b]) (void)hipHostFree(g_bounce[b]);
                    g_bounce[0] = g_bounce[1] = nullptr;
                    return false;
                }
                g_bounce_bytes = bytes;
                if (!g_bounce_atexit) {
                    g_bounce_atexit = true;
                    atexit(bounce_release_at_exit);
                }
            }
            g_bounce_busy = true;
            out[0] = g_bounce[0], out[1] = g_bounce[1];
            *cached = true;
            return true;
        }
    }
    *cached = false; // another upload holds the pair: buffers of this call's own
    out[0] = out[1] = nullptr;
    if (hipHostMalloc(&out[0], bytes) != hipSuccess || hipHostMalloc(&out[1], bytes) != hipSuccess) {
        (void)hipGetLastError();
        for (int b = 0; b < 2; b++)
            if (out[b]) (void)hipHostFree(out[b]);
        out[0] = out[1] = nullptr;
        return false;
    }
    return true;
}
static void bounce_give_back(double *buf[2], bool cached)
{
    if (cached) {
        std::lock_guard<std::mutex> lk(g_bounce_mu);
        g_bounce_busy = false;
    } else
        for (int b = 0; b < 2; b++)
            if (buf[b]) (void)hipHostFree(buf[b]);
    buf[0] = buf[1] = nullptr;
}

static std::atomic<size_t> g_debug_alloc_limit{0}; // nnlm_debug_alloc_limit (test hook): matrix-sized KL workspaces beyond this many bytes "do not fit" (0 = no limit)

// Matrix-sized workspaces of the KL solvers (starting states of all columns, transposed copy of A, streaming scratch): the callers have
// a smaller-footprint path when one of them cannot be had, so a failure here is an answer, not an error.
static hipError_t big_malloc(void **p, size_t bytes)
{
    *p = nullptr;
    const size_t lim = g_debug_alloc_limit.load(std::memory_order_relaxed);
    if (lim && bytes > lim) return hipErrorOutOfMemory;
    const hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
    }
    return e;
}

extern "C" int nnlm_debug_alloc_limit(size_t bytes)
{
    g_debug_alloc_limit = bytes;
    return NNLM_OK;
}

static std::atomic<int> g_debug_poison{0}; // nnlm_debug_poison_workspaces (test hook): new per-column Gram buffers are filled with 0xFF bytes (every double a NaN)

extern "C" int nnlm_debug_poison_workspaces(int on)
{
    g_debug_poison = on ? 1 : 0;
    return NNLM_OK;
}

// A per-column Gram buffer that was just allocated: the Gram kernels write the upper triangle up to k of every KP x KP block and nothing
// else, so the rest holds whatever the allocation held.  The test hook makes that NaN, on the handle's stream, ahead of the first use.
static hipError_t poison_new_gram(void *p, size_t bytes, hipStream_t st)
{
    if (!g_debug_poison.load(std::memory_order_relaxed)) return hipSuccess;
    return hipMemsetAsync(p, 0xFF, bytes, st);
}

extern "C" int nnlm_debug_set_xprod_waves(int waves)
{
    if (waves != 0 && waves != 8 && waves != 10) return fail(nullptr, NNLM_ERR_ARG, "nnlm_debug_set_xprod_waves: %d (0, 8 or 10)", waves);
    g_debug_xprod_waves = waves;
    return NNLM_OK;
}

extern "C" int nnlm_debug_set_a_stream(int nt_from_stage)
{
    if (nt_from_stage < -1) return fail(nullptr, NNLM_ERR_ARG, "nnlm_debug_set_a_stream: %d (-1, or a stage >= 0)", nt_from_stage);
    g_debug_a_stream = nt_from_stage;
    return NNLM_OK;
}

extern "C" int nnlm_debug_set_cus(int cus)
{
    if (cus < 0) return fail(nullptr, NNLM_ERR_ARG, "nnlm_debug_set_cus: %d", cus);
    g_debug_cus = cus;
    return NNLM_OK;
}

// The streams, events and small buffers of a destroyed handle wait here for the next nnlm_create on the same device (one set per process):
// creating and destroying them is 5 + 5 ms of every one-shot call -- half of a 200 x 100 nnmf() of 100 iterations (scripts/gpu_call_breakdown.py).
// The handle itself is always a fresh object: no state of a previous call survives, only resources do.
struct HandleRes {
    bool valid = false;
    int device = -1, cus = 0;
    hipStream_t stream = nullptr, stream_e = nullptr;
    hipEvent_t ev_hdone = nullptr, ev_err = nullptr, ev_xdone = nullptr;
    double *scal = nullptr, *host_res = nullptr, *sweepq_img = nullptr;
    unsigned long long *sweeps = nullptr, *sweeps_tmp = nullptr;
    unsigned *maxbits = nullptr;
    int *scal_exp = nullptr;
};
static std::mutex g_res_mu;
static HandleRes g_res;
static bool g_res_atexit = false;
static void handle_res_destroy(HandleRes &r)
{
    (void)hipFree(r.scal), (void)hipFree(r.sweeps), (void)hipHostFree(r.host_res), (void)hipFree(r.sweeps_tmp), (void)hipFree(r.sweepq_img);
    (void)hipFree(r.maxbits), (void)hipFree(r.scal_exp);
    if (r.ev_hdone) (void)hipEventDestroy(r.ev_hdone);
    if (r.ev_err) (void)hipEventDestroy(r.ev_err);
    if (r.ev_xdone) (void)hipEventDestroy(r.ev_xdone);
    if (r.stream_e) (void)hipStreamDestroy(r.stream_e);
    if (r.stream) (void)hipStreamDestroy(r.stream);
    r = HandleRes{};
}
static void handle_res_release_at_exit()
{
    if (g_res.valid) handle_res_destroy(g_res); // (errors ignored: the runtime may be shutting down)
}

extern "C" int nnlm_create(nnlm_handle **out, int device, int precision)
{
    if (!out) return fail(nullptr, NNLM_ERR_ARG, "nnlm_create: out is NULL");
    *out = nullptr;
    if (precision != NNLM_PREC_F32 && precision != NNLM_PREC_F64) return fail(nullptr, NNLM_ERR_ARG, "nnlm_create: unknown precision %d", precision);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, NNLM_ERR_HIP, "nnlm_create: no HIP device available (%s); libnnlm_mi355x has no CPU path", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= ndev) return fail(nullptr, NNLM_ERR_ARG, "nnlm_create: device %d out of range (0..%d)", device, ndev - 1);
    HIPCHK(nullptr, hipSetDevice(device));
    HandleRes res;
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (g_res.valid && g_res.device == device) {
            res = g_res;
            g_res = HandleRes{};
        }
    }
    if (res.valid) { // the resources of a handle this process destroyed earlier (same device: the architecture check has been made)
        nnlm_handle *h = new nnlm_handle();
        h->device = device;
        h->prec = precision;
        h->cus = h->cus_device = res.cus;
        if (const int dc = g_debug_cus.load(std::memory_order_relaxed); dc > 0) h->cus = dc;
        h->xprod_waves = g_debug_xprod_waves.load(std::memory_order_relaxed);
        h->a_stream = g_debug_a_stream.load(std::memory_order_relaxed);
        h->stream = res.stream, h->stream_e = res.stream_e;
        h->ev_hdone = res.ev_hdone, h->ev_err = res.ev_err, h->ev_xdone = res.ev_xdone;
        h->scal = res.scal, h->sweeps = res.sweeps, h->host_res = res.host_res, h->sweeps_tmp = res.sweeps_tmp, h->sweepq_img = res.sweepq_img;
        h->maxbits = res.maxbits, h->scal_exp = res.scal_exp;
        // (inherited streams may be dead -- hipDeviceReset by the host application, a fork, a sticky error raised after the destroy: a
        //  cached set that does not answer is dropped and the call goes on to create a fresh one)
        const bool alive = hipMemsetAsync(h->sweeps, 0, 2 * sizeof(unsigned long long), h->stream) == hipSuccess &&
                           hipMemsetAsync(h->scal_exp, 0, 4 * sizeof(int), h->stream) == hipSuccess &&
                           hipMemsetAsync(h->maxbits, 0, 16 * sizeof(unsigned), h->stream) == hipSuccess &&
                           hipStreamSynchronize(h->stream) == hipSuccess && hipStreamSynchronize(h->stream_e) == hipSuccess;
        if (alive) {
            h->x16 = x16_enabled(precision);
            *out = h;
            return NNLM_OK;
        }
        (void)hipGetLastError();
        delete h; // (a plain object at this point: the resources are still `res`'s)
        handle_res_destroy(res);
    }
    hipDeviceProp_t prop;
    HIPCHK(nullptr, hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, NNLM_ERR_HIP, "nnlm_create: device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
    nnlm_handle *h = new nnlm_handle();
    h->device = device;
    h->prec = precision;
    h->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->cus_device = h->cus;
    if (const int dc = g_debug_cus.load(std::memory_order_relaxed); dc > 0) h->cus = dc; // test hook (nnlm_debug_set_cus): the sweep's launch policy at small sizes
    h->xprod_waves = g_debug_xprod_waves.load(std::memory_order_relaxed);
    h->a_stream = g_debug_a_stream.load(std::memory_order_relaxed);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->stream_e, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_hdone, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_err, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_xdone, hipEventDisableTiming) != hipSuccess) {
        delete h;
        return fail(nullptr, NNLM_ERR_HIP, "nnlm_create: stream/event creation failed");
    }
    if (hipMalloc(&h->scal, 16 * sizeof(double)) != hipSuccess || hipMalloc(&h->sweeps, 2 * sizeof(unsigned long long)) != hipSuccess ||
        hipHostMalloc(&h->host_res, 16 * sizeof(double)) != hipSuccess ||
        hipMalloc(&h->sweeps_tmp, sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&h->sweepq_img, sweepq_img_doubles(16, true) * sizeof(double)) != hipSuccess ||
        hipMalloc(&h->maxbits, 16 * sizeof(unsigned)) != hipSuccess || hipMalloc(&h->scal_exp, 4 * sizeof(int)) != hipSuccess) {
        delete h;
        return fail(nullptr, NNLM_ERR_HIP, "nnlm_create: hipMalloc failed");
    }
    if (hipMemsetAsync(h->sweeps, 0, 2 * sizeof(unsigned long long), h->stream) != hipSuccess ||
        hipMemsetAsync(h->scal_exp, 0, 4 * sizeof(int), h->stream) != hipSuccess ||
        hipMemsetAsync(h->maxbits, 0, 16 * sizeof(unsigned), h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) {
        const hipError_t em = hipGetLastError();
        HandleRes dead; // (not through nnlm_destroy: it would offer these resources to the next create)
        dead.stream = h->stream, dead.stream_e = h->stream_e, dead.ev_hdone = h->ev_hdone, dead.ev_err = h->ev_err, dead.ev_xdone = h->ev_xdone;
        dead.scal = h->scal, dead.sweeps = h->sweeps, dead.host_res = h->host_res, dead.sweeps_tmp = h->sweeps_tmp, dead.sweepq_img = h->sweepq_img;
        dead.maxbits = h->maxbits, dead.scal_exp = h->scal_exp;
        delete h;
        handle_res_destroy(dead);
        return fail(nullptr, NNLM_ERR_HIP, "nnlm_create: clearing the handle's counters failed: %s", hipGetErrorString(em));
    }
    h->x16 = x16_enabled(precision);
    *out = h;
    return NNLM_OK;
}

// The process-wide caches (the streams / events / scratch of the last destroyed handle, the pinned bounce buffers of nnlm_set_matrix: up to
// 2 x 64 MB of pinned host memory) are released at exit; an embedder that unloads the library earlier (an R package's .onUnload hook)
// or wants the pinned memory back calls this.  Handles in use are not affected.
extern "C" int nnlm_release_caches(void)
{
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (g_res.valid) handle_res_destroy(g_res);
    }
    {
        std::lock_guard<std::mutex> lk(g_bounce_mu);
        if (!g_bounce_busy) bounce_release_at_exit();
    }
    return NNLM_OK;
}

// Everything a half-step may find left behind by the previous one describes the factors as the library last wrote them: any other
// writer of the factors (nnlm_set_factors) or of the exchange (nnlm_comm_init) calls this.
static void invalidate_factor_caches(nnlm_handle *h)
{
    h->upk_max_for = -1;
    h->gshard_for = -1;
    h->y16_for = -1;
    h->sg_which = h->sg_other = -1;
    h->pack_ready = false;
}

static void free_batch(nnlm_handle *h)
{
    hipFree(h->boff_dev);
    hipFree(h->bG);
    hipFree(h->bsweeps);
    hipFree(h->bpart);
    hipFree(h->bres);
    hipFree(h->bsp_Hrow);
    hipFree(h->bsp_part);
    h->boff_dev = nullptr;
    h->bG = h->bpart = h->bres = h->bsp_Hrow = h->bsp_part = nullptr;
    h->bsweeps = nullptr;
    h->bpart_elems = 0;
    h->bspg_pairs = 0;
    h->bB = 0;
    h->bk.clear();
    h->boff.clear();
}

static void free_factors(nnlm_handle *h)
{
    free_batch(h);
    for (int i = 0; i < 2; i++) {
        if (h->Wopb[i] && h->Wopb[i] != (void *)h->W64b[i]) hipFree(h->Wopb[i]);
        hipFree(h->W64b[i]);
        h->W64b[i] = nullptr;
        h->Wopb[i] = nullptr;
    }
    h->wcur = 0;
    hipFree(h->H64);
    hipFree(h->Hkq);
    h->Hkq = nullptr;
    hipFree(h->Wmask);
    hipFree(h->Hmask);
    hipFree(h->Cx);
    hipFree(h->What);
    hipFree(h->What64);
    h->What = nullptr;
    h->What64 = nullptr;
    hipFree(h->klsw);
    hipFree(h->klsw_cols);
    hipFree(h->klst);
    h->klsw = h->klsw_cols = nullptr;
    h->klst = nullptr;
    h->klst_bytes = 0;
    h->what_tight = h->klst_tight = false; // (another rank, other workspace sizes: asked again)
    hipFree(h->Y16);
    hipFree(h->W16c);
    hipFree(h->H16c);
    h->Y16 = h->W16c = h->H16c = nullptr;
    hipFree(h->gslabs);
    hipFree(h->sg_slabs);
    h->sg_slabs = nullptr;
    h->sg_which = h->sg_other = -1;
    hipFree(h->red);
    hipFree(h->pack_send);
    hipFree(h->pack_all);
    h->pack_send = h->pack_all = nullptr;
    h->pack_elems = 0;
    hipFree(h->Yrow);
    hipFree(h->Gcols);
    h->red = h->Yrow = h->Gcols = nullptr;
    hipFree(h->sp_Y);
    hipFree(h->sp_carry);
    hipFree(h->sp_Wrow);
    hipFree(h->sp_eslabs);
    hipFree(h->sp_eG);
    hipFree(h->sp_epart);
    h->sp_Y = nullptr;
    h->sp_carry = h->sp_Wrow = h->sp_eslabs = h->sp_eG = h->sp_epart = nullptr;
    hipFree(h->spg_buf);
    h->spg_buf = nullptr;
    h->spg_buf_bytes = 0;
    for (int o = 0; o < 2; o++) h->spg_plan[o].clear(), h->spg_plan_cap[o] = 0; // (the plan depends on KP)
    h->W64 = h->H64 = nullptr;
    h->Wop = nullptr;
    h->Wmask = h->Hmask = nullptr;
    h->Cx = h->gslabs = h->Graw = nullptr;
    h->k = 0;
}

static void free_svd(nnlm_handle *h)
{
    hipFree(h->svdU);
    hipFree(h->svdVt);
    h->svdU = h->svdVt = nullptr;
    h->svd_l = h->svd_LP = h->svd_kept = 0;
    h->svd_sigma.clear();
    h->svd_mean_known = false;
}

static void free_matrix(nnlm_handle *h)
{
    free_svd(h); // (a decomposition describes the matrix it was made from)
    for (int o = 0; o < 2; o++) {
        hipFree(h->na_ptr[o]);
        hipFree(h->na_meta[o]);
        hipFree(h->na_idx[o]);
        h->na_ptr[o] = h->na_meta[o] = nullptr;
        h->na_idx[o] = nullptr;
    }
    hipFree(h->A);
    hipFree(h->AT);
    h->AT = nullptr;
    h->what_tight = h->klst_tight = h->at_tight = false; // (what did not fit beside the last matrix may fit beside the next)
    hipFree(h->A16);
    hipFree(h->A16T);
    h->A16 = h->A16T = nullptr;
    hipFree(h->miss);
    hipFree(h->missT);
    hipFree(h->partials);
    h->A = nullptr;
    h->miss = nullptr;
    h->missT = nullptr;
    h->partials = nullptr;
    hipFree(h->sp_cptr);
    hipFree(h->sp_rptr);
    hipFree(h->sp_ridx);
    hipFree(h->sp_cidx);
    hipFree(h->sp_cval);
    hipFree(h->sp_rval);
    h->sp_cptr = h->sp_rptr = nullptr;
    h->sp_ridx = h->sp_cidx = nullptr;
    h->sp_cval = h->sp_rval = nullptr;
    h->sp_bytes = 0;
    h->sparse = false;
    for (int o = 0; o < 2; o++) {
        hipFree(h->spg_segoff[o]);
        hipFree(h->spg_longc[o]);
        h->spg_segoff[o] = nullptr;
        h->spg_longc[o] = nullptr;
        h->spg_hptr[o].clear();
        h->spg_plan[o].clear();
        h->spg_plan_cap[o] = 0;
    }
    h->sp_missing = false;
    hipFree(h->sp_cwt);
    hipFree(h->sp_rwt);
    hipFree(h->sp_cwa);
    hipFree(h->sp_rwa);
    h->sp_cwt = h->sp_rwt = h->sp_cwa = h->sp_rwa = nullptr;
    h->sp_weighted = false;
    for (int o = 0; o < 2; o++) {
        hipFree(h->spkl_longc[o]);
        h->spkl_longc[o] = nullptr;
        h->spkl_nlong[o] = h->spkl_nshort[o] = 0;
        h->spkl_form[o] = h->spklb_form[o] = -1;
    }
    hipFree(h->spkl_state);
    h->spkl_state = nullptr;
    h->sp_kl = false;
    h->sp_batch = false;
    h->nnz = 0;
    hipFree(h->ho_cptr);
    hipFree(h->ho_ridx);
    hipFree(h->ho_cidx);
    hipFree(h->ho_val);
    h->ho_cptr = nullptr;
    h->ho_ridx = h->ho_cidx = nullptr;
    h->ho_val = nullptr;
    h->ho_nnz = 0;
    h->holdout = false;
    h->x16 = x16_enabled(h->prec); // (a sparse matrix turned it off)
    h->min_obs[0] = h->min_obs[1] = -2;
    h->n = h->m = 0;
}

// a matrix is set: the dense resident layout or the sparse one
static bool has_matrix(const nnlm_handle *h) { return h && (h->A || h->sparse); }

// device bytes of the resident matrix: dense A, its missing-entry bitmaps and split-fp16 / transposed copies; or the CSC + CSR arrays
static double matrix_bytes(const nnlm_handle *h)
{
    if (h->sparse) return (double)h->sp_bytes;
    if (!h->A) return 0.0;
    const double cnt = (double)h->npad * h->mpad;
    double b = cnt * esize(h) + 4096 + (double)h->mpad * (h->npad / 32) * 4 + 64;
    if (h->missT) b += (double)h->npad * (h->mpad / 32) * 4 + 64;
    if (h->A16) b += cnt * 4 + 4096;
    if (h->A16T) b += cnt * 4 + 4096;
    if (h->AT) b += cnt * esize(h) + 4096;
    return b;
}

extern "C" void nnlm_destroy(nnlm_handle *h)
{
    if (!h) return;
    hipSetDevice(h->device);
    sync_all(h);
    prof_collect(h);
    if (h->comm && g_rccl.CommDestroy) { // (before the streams its collectives were enqueued on go away)
        g_rccl.CommDestroy((ncclComm_t)h->comm);
        h->comm = nullptr;
    }
    free_factors(h);
    free_matrix(h);
    HandleRes res;
    res.valid = true, res.device = h->device, res.cus = h->cus_device;
    res.stream = h->stream, res.stream_e = h->stream_e;
    res.ev_hdone = h->ev_hdone, res.ev_err = h->ev_err, res.ev_xdone = h->ev_xdone;
    res.scal = h->scal, res.sweeps = h->sweeps, res.host_res = h->host_res, res.sweeps_tmp = h->sweeps_tmp, res.sweepq_img = h->sweepq_img;
    res.maxbits = h->maxbits, res.scal_exp = h->scal_exp;
    delete h;
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (!g_res.valid && hipGetLastError() == hipSuccess) { // (the streams are idle: sync_all above; a sticky error keeps nothing)
            g_res = res;
            res.valid = false;
            if (!g_res_atexit) {
                g_res_atexit = true;
                atexit(handle_res_release_at_exit);
            }
        }
    }
    if (res.valid) handle_res_destroy(res);
}

// ---------------------------------------------------------------------------------------------
// matrix upload
// ---------------------------------------------------------------------------------------------
// The upload in three parts, shared by the host route (set_matrix_impl) and the device route (nnlm_set_matrix_device):
// matrix_alloc -- the resident buffers, zeroed; a fill -- the host chunk loop below or the device ingest (k_ingest.h), each leaving A,
// miss and the three sums of the prep pass; matrix_finish -- everything that follows from them.
static int matrix_alloc(nnlm_handle *h, int n, int m)
{
    HIPCHK(h, hipSetDevice(h->device));
    free_factors(h);
    free_matrix(h);
    h->n = n;
    h->m = m;
    h->npad = round_up_i(n, NNLM_PAD_N);
    h->mpad = round_up_i(m, NNLM_PAD_M);
    const size_t es = esize(h);
    const size_t a_bytes = (size_t)h->npad * h->mpad * es;
    const size_t miss_words = (size_t)h->mpad * (h->npad / 32);
    HIPCHK(h, hipMalloc(&h->A, a_bytes + 4096));
    HIPCHK(h, hipMalloc(&h->miss, miss_words * 4 + 64));
    HIPCHK(h, hipMemsetAsync(h->A, 0, a_bytes + 4096, h->stream));
    HIPCHK(h, hipMemsetAsync(h->miss, 0, miss_words * 4 + 64, h->stream));
    // partial-sum workspace shared by the prep / error / penalty reductions
    const size_t err_blocks = (size_t)(h->npad / ERR_TILE) * (h->mpad / ERR_TILE);
    const int gx = h->npad / PREP_BLOCK;
    const size_t prep_blocks = (size_t)gx * PREP_GRID_Y;
    h->partials_elems = 3 * (err_blocks > 2 * prep_blocks ? err_blocks : 2 * prep_blocks) + 64; // (two slots of prep partial sums)
    HIPCHK(h, hipMalloc(&h->partials, h->partials_elems * sizeof(double)));
    return NNLM_OK;
}

static int matrix_finish(nnlm_handle *h, double cnt, double klc, double over);

// nnlm_set_matrix and nnlm_set_matrix_holdout: one upload.  ho_colptr / ho_rowidx (validated by the caller, NULL for a plain upload):
// the held-out pattern.  Every chunk of columns then passes through a host staging buffer in which A is checked to be finite and the
// pattern's entries are replaced by NaN before the DMA -- prep_convert_kernel sees exactly what it sees for a matrix that arrived with
// NaN there, so the resident state is that upload's bit for bit, and no second n x m array exists anywhere.  ho_val[e]: the values taken out.
static int set_matrix_impl(nnlm_handle *h, const double *A, int n, int m, const long long *ho_colptr, const int *ho_rowidx, double *ho_val)
{
    const bool ho = ho_colptr != nullptr;
    if (const int rc_alloc = matrix_alloc(h, n, m)) return rc_alloc;
    const int gx = h->npad / PREP_BLOCK;
    const size_t prep_blocks = (size_t)gx * PREP_GRID_Y;

    // Upload: the caller's matrix is pageable host memory (R's heap, a numpy array).  hipMemcpy from pageable memory stages through
    // ONE runtime thread (4.3 GB/s measured: 0.37 s of a 0.7 s nnmf() call of 500 iterations at config 2).  Here: chunks of whole
    // columns are copied by a few host threads into one of two PINNED bounce buffers, from there by DMA into one of two device
    // staging buffers, converted by prep_convert_kernel -- the host copy of chunk i + 1 runs beside the DMA and the prep pass of chunk i.
    const size_t stage_bytes_max = (size_t)64 << 20;
    int cols_per_chunk = (int)(stage_bytes_max / ((size_t)n * 8));
    if (cols_per_chunk < 1) cols_per_chunk = 1;
    if (cols_per_chunk > m) cols_per_chunk = m;
    const size_t chunk_bytes = (size_t)cols_per_chunk * n * 8;
    double *stage[2] = {nullptr, nullptr}, *bounce[2] = {nullptr, nullptr};
    double *hp[2] = {nullptr, nullptr}; // pinned: the prep pass's partial sums of each slot
    hipEvent_t ev_done[2] = {nullptr, nullptr};
    int rc = NNLM_OK;
    // (matrices of a few MB go through the runtime's pageable path: its own staging buffers are pinned already)
    bool bounce_cached = false;
    bool pinned = (size_t)n * m * 8 >= ((size_t)4 << 20) && bounce_acquire(chunk_bytes, bounce, &bounce_cached);
    std::vector<double> hostbuf[2]; // hold-out upload without the pinned buffers: the chunk's host copy (the caller's A is not written)
    if (ho && !pinned) {
        try {
            hostbuf[0].resize(chunk_bytes / 8);
            hostbuf[1].resize(chunk_bytes / 8);
        } catch (...) {
            rc = fail(h, NNLM_ERR_HIP, "nnlm_set_matrix_holdout: host staging buffer (%zu bytes)", chunk_bytes);
        }
    }
    for (int b = 0; b < 2 && rc == NNLM_OK; b++) {
        if (hipMalloc(&stage[b], chunk_bytes) != hipSuccess) rc = fail(h, NNLM_ERR_HIP, "nnlm_set_matrix: staging buffer (%zu bytes)", chunk_bytes);
        else if (hipHostMalloc(&hp[b], 3 * prep_blocks * sizeof(double)) != hipSuccess || hipEventCreateWithFlags(&ev_done[b], hipEventDisableTiming) != hipSuccess)
            rc = fail(h, NNLM_ERR_HIP, "nnlm_set_matrix: pinned result buffer / event");
    }
    unsigned nthreads = std::thread::hardware_concurrency();
    nthreads = nthreads >= 16 ? 8u : (nthreads >= 4 ? nthreads / 2 : 1u);
    auto host_copy = [&](double *dst, const double *src, size_t bytes) { // a few threads: one saturates ~10 GB/s of memcpy, the DMA takes 4-5x that
        if (nthreads <= 1 || bytes < ((size_t)8 << 20)) {
            memcpy(dst, src, bytes);
            return;
        }
        // (no exception may cross the C ABI: a std::thread that cannot be created -- thread limit of a container -- or a vector that
        //  cannot grow leaves its piece, and every piece after it, to a plain memcpy on this thread, and the mode is kept off from then on)
        std::vector<std::thread> th;
        const size_t per = ((bytes / nthreads) + 4095) & ~(size_t)4095;
        size_t started = 0; // bytes handed to worker threads
        try {
            th.reserve(nthreads);
            for (unsigned t = 0; t < nthreads; t++) {
                const size_t o = (size_t)t * per;
                if (o >= bytes) break;
                const size_t len = (bytes - o < per) ? bytes - o : per;
                th.emplace_back([=]() { memcpy((char *)dst + o, (const char *)src + o, len); });
                started = o + len;
            }
        } catch (...) {
            nthreads = 1;
        }
        if (started < bytes) memcpy((char *)dst + started, (const char *)src + started, bytes - started);
        for (auto &x : th) x.join();
    };
    double cnt = 0.0, klc = 0.0, over = 0.0;
    auto collect = [&](int b) -> int { // wait for slot b's prep pass and add its partial sums (fixed order: chunk by chunk)
        const hipError_t e = hipEventSynchronize(ev_done[b]);
        if (e != hipSuccess) return fail(h, NNLM_ERR_HIP, "prep pass failed: %s", hipGetErrorString(e));
        for (size_t q = 0; q < prep_blocks; q++) {
            cnt += hp[b][3 * q];
            klc += hp[b][3 * q + 1];
            over += hp[b][3 * q + 2];
        }
        return NNLM_OK;
    };
    int pending[2] = {0, 0}, slot = 0;
    for (int j0 = 0; j0 < m && rc == NNLM_OK; j0 += cols_per_chunk, slot ^= 1) {
        const int cols = (m - j0 < cols_per_chunk) ? m - j0 : cols_per_chunk;
        const size_t bytes = (size_t)cols * n * 8;
        if (pending[slot]) { // the slot's previous chunk: its DMA has read the bounce buffer, its prep pass the staging buffer
            rc = collect(slot);
            pending[slot] = 0;
            if (rc != NNLM_OK) break;
        }
        const double *src = A + (size_t)j0 * n;
        if (pinned) {
            host_copy(bounce[slot], src, bytes);
            src = bounce[slot];
        } else if (ho) {
            memcpy(hostbuf[slot].data(), src, bytes);
            src = hostbuf[slot].data();
        }
        if (ho) { // finite A, then NaN at the pattern (the slot's previous DMA has been waited for above)
            double *buf = const_cast<double *>(src);
            for (int c = 0; c < cols && rc == NNLM_OK; c++) {
                double *col = buf + (size_t)c * n;
                unsigned long long bad = 0;
                for (int i = 0; i < n; i++) {
                    unsigned long long u;
                    memcpy(&u, col + i, 8);
                    bad |= (unsigned long long)(((u >> 52) & 0x7FFull) == 0x7FFull);
                }
                if (bad) {
                    int i = 0;
                    while (std::isfinite(col[i])) i++;
                    rc = fail(h, NNLM_ERR_ARG, "nnlm_set_matrix_holdout: A[%d, %d] is not finite; a hold-out handle needs a finite A (missing "
                                               "entries enter through the pattern only)", i, j0 + c);
                    break;
                }
                for (long long q = ho_colptr[j0 + c]; q < ho_colptr[j0 + c + 1]; q++) {
                    ho_val[q] = col[ho_rowidx[q]];
                    col[ho_rowidx[q]] = std::nan("");
                }
            }
            if (rc != NNLM_OK) break;
        }
        hipError_t e = hipMemcpyAsync(stage[slot], src, bytes, hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) { rc = fail(h, NNLM_ERR_HIP, "upload of A failed: %s", hipGetErrorString(e)); break; }
        dim3 grid(gx, PREP_GRID_Y);
        double *part = h->partials + (size_t)slot * 3 * prep_blocks;
        if (h->prec == NNLM_PREC_F64)
            prep_convert_kernel<double><<<grid, PREP_BLOCK, 0, h->stream>>>(stage[slot], (size_t)n, (size_t)1, n, cols, j0, (double *)h->A, h->npad, h->miss, part);
        else
            prep_convert_kernel<float><<<grid, PREP_BLOCK, 0, h->stream>>>(stage[slot], (size_t)n, (size_t)1, n, cols, j0, (float *)h->A, h->npad, h->miss, part);
        e = hipMemcpyAsync(hp[slot], part, 3 * prep_blocks * sizeof(double), hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess) e = hipEventRecord(ev_done[slot], h->stream);
        if (e != hipSuccess) { rc = fail(h, NNLM_ERR_HIP, "prep pass failed: %s", hipGetErrorString(e)); break; }
        pending[slot] = 1;
    }
    // (in chunk order: the slot used last holds the newest chunk)
    for (int q = 0; q < 2; q++) {
        const int b = slot ^ q; // slot was flipped past the last chunk: slot = the older one
        if (pending[b] && rc == NNLM_OK) rc = collect(b);
    }
    hipStreamSynchronize(h->stream);
    if (pinned) bounce_give_back(bounce, bounce_cached);
    for (int b = 0; b < 2; b++) {
        hipFree(stage[b]);
        if (hp[b]) hipHostFree(hp[b]);
        if (ev_done[b]) hipEventDestroy(ev_done[b]);
    }
    if (rc != NNLM_OK) {
        if (ho) free_matrix(h);
        return rc;
    }
    return matrix_finish(h, cnt, klc, over);
}

// The common tail of an upload: cnt / klc / over = the prep pass's sums over the whole matrix (finite entries, the constant KL part, finite
// entries beyond the range of the fp32 resident copy).
static int matrix_finish(nnlm_handle *h, double cnt, double klc, double over)
{
    const int n = h->n, m = h->m;
    if (over > 0.0) {
        free_matrix(h);
        return fail(h, NNLM_ERR_UNSUPPORTED, "%.0f finite entries of A exceed the fp32 range (|a| > 3.4e38): the fp32-operand mode cannot hold them; "
                                             "use the strict fp64 mode (NNLM_PREC_F64, the default of nnlm_c_nnmf / nnlm_c_nnlm)", over);
    }
    h->n_non_missing = cnt;
    h->any_missing = cnt != (double)n * (double)m;
    h->kl_const = klc / cnt; // mean((A+eps) log(A+eps) - A) over finite entries, src/nnmf.cpp:70,73
    if (h->x16) { // split-fp16 copies of A and of its transpose, pre-scaled by 2^eA (k_xprod16.h)
        const size_t cnt_a = (size_t)h->npad * h->mpad;
        HIPCHK(h, hipMemsetAsync(h->maxbits, 0, sizeof(unsigned), h->stream));
        absmax_f32_kernel<<<1024, 256, 0, h->stream>>>((const float *)h->A, cnt_a, h->maxbits);
        unsigned mb = 0;
        HIPCHK(h, hipMemcpyAsync(&mb, h->maxbits, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        float mx;
        memcpy(&mx, &mb, 4);
        if (mx > 0.0f && mx < 7.8886090522101181e-31f) { // 2^-100: entries 2^-26 below the largest one are fp32 denormals
            free_matrix(h);
            return fail(h, NNLM_ERR_UNSUPPORTED, "max |A| = %.3g is too close to the bottom of the fp32 range for the fp32-operand mode (entries would "
                                                 "be denormal or flushed to zero); rescale A or use the strict fp64 mode", (double)mx);
        }
        const int eA = split16_exponent(mx);
        HIPCHK(h, hipMemcpyAsync(h->scal_exp, &eA, sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMalloc(&h->A16, cnt_a * 4 + 4096));
        HIPCHK(h, hipMalloc(&h->A16T, cnt_a * 4 + 4096));
        const float scale = ldexpf(1.0f, eA);
        a16_convert_kernel<<<(unsigned)((cnt_a + 255) / 256), 256, 0, h->stream>>>((const float *)h->A, cnt_a, scale, h->A16);
        dim3 gt(h->npad / 64, h->mpad / 64);
        a16_transpose_kernel<<<gt, 256, 0, h->stream>>>((const float *)h->A, h->npad, h->npad, h->mpad, scale, h->A16T);
        HIPCHK(h, hipStreamSynchronize(h->stream));
        LAUNCHCHK(h);
    }
    if (h->any_missing) { // row-wise view of the missing mask for the W half-step
        const size_t wordsT = (size_t)h->npad * (h->mpad / 32);
        HIPCHK(h, hipMalloc(&h->missT, wordsT * 4 + 64));
        dim3 grid((h->mpad / 32 + 255) / 256, h->npad);
        miss_transpose_kernel<<<grid, 256, 0, h->stream>>>(h->miss, h->npad, h->mpad, h->missT);
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return NNLM_OK;
}

extern "C" int nnlm_set_matrix(nnlm_handle *h, const double *A, int n, int m)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "nnlm_set_matrix: handle is NULL");
    if (!A || n <= 0 || m <= 0) return fail(h, NNLM_ERR_ARG, "nnlm_set_matrix: A must be a non-empty n x m matrix (n=%d, m=%d)", n, m);
    return set_matrix_impl(h, A, n, m, nullptr, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------
// matrices and factors in device memory
// ---------------------------------------------------------------------------------------------
static size_t dt_size(int dt) { return dt == NNLM_DT_F64 ? 8 : (dt == NNLM_DT_F32 ? 4 : 2); }

// The handle's matrix and factor allocations, which a caller's buffer may not be (base = start of the allocation the caller's pointer
// lies in).  Best effort: the matrix, its copies and bit matrices, the factor masters, operand copies and masks -- not every workspace --,
// and only where hipMemGetAddressRange can name the allocation.
static bool owns_allocation(const nnlm_handle *h, const void *base)
{
    const void *mine[] = {h->A, h->AT, h->miss, h->missT, h->A16, h->A16T, h->partials, h->W64b[0], h->W64b[1], h->Wopb[0], h->Wopb[1], h->H64,
                          h->Hkq, h->Wmask, h->Hmask, h->Y16, h->W16c, h->H16c, h->Cx, h->red, h->gslabs, h->sg_slabs, h->What, h->What64,
                          h->sp_cptr, h->sp_rptr, h->sp_ridx, h->sp_cidx, h->sp_cval, h->sp_rval, h->sp_Y, h->bG, h->ho_val,
                          h->sp_cwt, h->sp_rwt, h->sp_cwa, h->sp_rwa};
    for (const void *p : mine)
        if (p && p == base) return true;
    return false;
}

// Everything that can be known about a descriptor before a kernel touches its pointer: rows x cols elements, `name` = the argument.
static int dev_matrix_check(nnlm_handle *h, const char *who, const char *name, const nnlm_dev_matrix *d, int rows, int cols, bool output)
{
    if (!d->ptr) return fail(h, NNLM_ERR_ARG, "%s: %s.ptr is NULL", who, name);
    if (d->dtype < NNLM_DT_F64 || d->dtype > NNLM_DT_BF16) return fail(h, NNLM_ERR_ARG, "%s: %s.dtype = %d is not one of NNLM_DT_F64 .. NNLM_DT_BF16", who, name, d->dtype);
    if (output && d->dtype > NNLM_DT_F32)
        return fail(h, NNLM_ERR_ARG, "%s: %s.dtype = %d: the output types are NNLM_DT_F64 and NNLM_DT_F32 (F16 / BF16 are input types only)", who, name, d->dtype);
    if (d->row_stride < 1 || d->col_stride < 1)
        return fail(h, NNLM_ERR_ARG, "%s: the strides of %s must be positive (row_stride = %lld, col_stride = %lld): broadcast and reversed views are "
                                     "not accepted", who, name, d->row_stride, d->col_stride);
    const bool col_major = d->col_stride / rows >= d->row_stride && d->col_stride >= (long long)rows * d->row_stride;
    const bool row_major = d->row_stride / cols >= d->col_stride && d->row_stride >= (long long)cols * d->col_stride;
    if (!col_major && !row_major)
        return fail(h, NNLM_ERR_ARG, "%s: the layout of %s overlaps itself (%d x %d, row_stride = %lld, col_stride = %lld): one stride must span "
                                     "the whole extent of the other dimension", who, name, rows, cols, d->row_stride, d->col_stride);
    const size_t es = dt_size(d->dtype);
    if ((uintptr_t)d->ptr % es) return fail(h, NNLM_ERR_ARG, "%s: %s.ptr is not aligned to its %zu-byte elements", who, name, es);
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    const hipError_t e = hipPointerGetAttributes(&at, d->ptr);
    (void)hipGetLastError(); // (the query leaves a sticky error behind for a pointer the runtime does not know)
    if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged))
        return fail(h, NNLM_ERR_ARG, "%s: %s.ptr is not device (or managed) memory -- a host pointer?", who, name);
    if (at.type == hipMemoryTypeDevice && at.device != h->device)
        return fail(h, NNLM_ERR_ARG, "%s: %s lives on device %d, the handle on device %d", who, name, at.device, h->device);
    void *base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(d->ptr)) == hipSuccess) {
        const size_t span = ((size_t)(rows - 1) * (size_t)d->row_stride + (size_t)(cols - 1) * (size_t)d->col_stride + 1) * es;
        if ((const char *)d->ptr + span > (const char *)base + size)
            return fail(h, NNLM_ERR_ARG, "%s: %s (%d x %d with its strides) reaches %zu bytes past the end of its allocation", who, name, rows, cols,
                        (size_t)(((const char *)d->ptr + span) - ((const char *)base + size)));
        if (owns_allocation(h, base)) return fail(h, NNLM_ERR_ARG, "%s: %s aliases a buffer of the handle itself", who, name);
    } else
        (void)hipGetLastError();
    return NNLM_OK;
}

// `waiter` continues behind everything enqueued on `producer` so far: an event, no host wait
static int stream_after(nnlm_handle *h, hipStream_t waiter, hipStream_t producer)
{
    hipEvent_t ev = nullptr;
    HIPCHK(h, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, producer);
    if (e == hipSuccess) e = hipStreamWaitEvent(waiter, ev, 0);
    hipEventDestroy(ev); // (released by the runtime once the recorded work has passed it)
    if (e != hipSuccess) return fail(h, NNLM_ERR_HIP, "stream ordering (event record / wait) failed: %s", hipGetErrorString(e));
    return NNLM_OK;
}

// The device fill of an upload: A in the caller's type S and strides -> h->A (T), h->miss and the prep pass's three sums.
//   row_stride == 1: ingest_cols_kernel over the host route's column chunks and (gx, 64) grid; the per-block partial sums of all chunks come
//                    back in one copy and are added chunk by chunk, block by block -- the host route's order, hence its kl_const bit for bit;
//   col_stride == 1: ingest_rows_kernel (the transposition through LDS);
//   otherwise:       ingest_gather_kernel over the same chunks.
template <typename S, typename T>
static int ingest_fill(nnlm_handle *h, const nnlm_dev_matrix *d, double sums[3])
{
    const int n = h->n, m = h->m;
    const S *src = (const S *)d->ptr;
    T *dst = (T *)h->A;
    const bool rows_route = d->col_stride == 1 && d->row_stride != 1;
    const int tiles_j = (m + INGEST_TILE - 1) / INGEST_TILE;
    const dim3 grid_r(h->npad / INGEST_TILE, tiles_j < INGEST_GRID_Y ? tiles_j : INGEST_GRID_Y);
    int cols_per_chunk = (int)(((size_t)64 << 20) / ((size_t)n * 8)); // (the host route's chunks: set_matrix_impl)
    if (cols_per_chunk < 1) cols_per_chunk = 1;
    if (cols_per_chunk > m) cols_per_chunk = m;
    const int gx = h->npad / PREP_BLOCK;
    const size_t prep_blocks = (size_t)gx * PREP_GRID_Y;
    const size_t chunks = ((size_t)m + cols_per_chunk - 1) / cols_per_chunk;
    const size_t blocks = rows_route ? (size_t)grid_r.x * grid_r.y : chunks * prep_blocks;
    double *part = nullptr;
    HIPCHK(h, hipMalloc(&part, 3 * blocks * sizeof(double)));
    if (rows_route) {
        ProfScope ps(h, P_INGEST);
        const int vec = ((uintptr_t)src % 16 == 0 && ((size_t)d->row_stride * sizeof(S)) % 16 == 0) ? 1 : 0;
        ingest_rows_kernel<S, T><<<grid_r, 256, 0, h->stream>>>(src, (size_t)d->row_stride, vec, n, m, dst, h->npad, h->miss, part);
    } else {
        ProfScope ps(h, P_INGEST);
        const dim3 grid(gx, PREP_GRID_Y);
        size_t c = 0;
        for (int j0 = 0; j0 < m; j0 += cols_per_chunk, c++) {
            const int cols = (m - j0 < cols_per_chunk) ? m - j0 : cols_per_chunk;
            const S *s0 = src + (size_t)j0 * (size_t)d->col_stride;
            double *pc = part + 3 * c * prep_blocks;
            if (d->row_stride == 1) // ingest_cols_kernel<S, T>
                prep_convert_kernel<T, S, false><<<grid, PREP_BLOCK, 0, h->stream>>>(s0, (size_t)d->col_stride, (size_t)1, n, cols, j0, dst, h->npad, h->miss, pc);
            else // ingest_gather_kernel<S, T>
                prep_convert_kernel<T, S, true><<<grid, PREP_BLOCK, 0, h->stream>>>(s0, (size_t)d->col_stride, (size_t)d->row_stride, n, cols, j0, dst, h->npad, h->miss, pc);
        }
    }
    std::vector<double> hp;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        try {
            hp.resize(3 * blocks);
        } catch (...) {
            hipStreamSynchronize(h->stream);
            hipFree(part);
            return fail(h, NNLM_ERR_HIP, "nnlm_set_matrix_device: host buffer for %zu partial sums", 3 * blocks);
        }
        e = hipMemcpyAsync(hp.data(), part, 3 * blocks * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    hipFree(part);
    if (e != hipSuccess || e2 != hipSuccess) return fail(h, NNLM_ERR_HIP, "ingest pass failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    double cnt = 0.0, klc = 0.0, over = 0.0;
    for (size_t q = 0; q < blocks; q++) {
        cnt += hp[3 * q];
        klc += hp[3 * q + 1];
        over += hp[3 * q + 2];
    }
    sums[0] = cnt, sums[1] = klc, sums[2] = over;
    return NNLM_OK;
}

// f(S{}) for the source type of a descriptor
template <typename F>
static int with_dtype(int dtype, F &&f)
{
    switch (dtype) {
    case NNLM_DT_F64: return f(double{});
    case NNLM_DT_F32: return f(float{});
    case NNLM_DT_F16: return f(nnlm_f16{});
    default: return f(nnlm_bf16{});
    }
}

extern "C" int nnlm_set_matrix_device(nnlm_handle *h, const nnlm_dev_matrix *A, int n, int m, void *stream)
{
    const char *who = "nnlm_set_matrix_device";
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "%s: handle is NULL", who);
    if (!A || n <= 0 || m <= 0) return fail(h, NNLM_ERR_ARG, "%s: A must be a non-empty n x m matrix (n=%d, m=%d)", who, n, m);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = dev_matrix_check(h, who, "A", A, n, m, false);
    if (rc != NNLM_OK) return rc;
    if ((rc = matrix_alloc(h, n, m)) != NNLM_OK) return rc;
    if ((rc = stream_after(h, h->stream, (hipStream_t)stream)) != NNLM_OK) { // the caller's stream produced A
        free_matrix(h);
        return rc;
    }
    double sums[3] = {0.0, 0.0, 0.0};
    rc = with_dtype(A->dtype, [&](auto s) {
        typedef decltype(s) S;
        return h->prec == NNLM_PREC_F64 ? ingest_fill<S, double>(h, A, sums) : ingest_fill<S, float>(h, A, sums);
    });
    if (rc != NNLM_OK) {
        free_matrix(h);
        return rc;
    }
    return matrix_finish(h, sums[0], sums[1], sums[2]);
}

// Dense finite A with a hold-out pattern (include/nnlm_mi355x.h)
extern "C" int nnlm_set_matrix_holdout(nnlm_handle *h, const double *A, int n, int m, const long long *colptr, const int *rowidx)
{
    const char *who = "nnlm_set_matrix_holdout";
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "%s: handle is NULL", who);
    if (!A || n <= 0 || m <= 0 || !colptr) return fail(h, NNLM_ERR_ARG, "%s: A must be a non-empty n x m matrix with a pattern colptr[m + 1] (n=%d, m=%d)", who, n, m);
    if (h->sharded) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: a hold-out handle is single-GPU only (this handle has a communicator)", who);
    // the pattern: canonical CSC, as nnlm_set_matrix_csc checks it
    if (colptr[0] != 0) return fail(h, NNLM_ERR_ARG, "%s: colptr[0] = %lld, must be 0", who, colptr[0]);
    for (int j = 0; j < m; j++)
        if (colptr[j + 1] < colptr[j]) return fail(h, NNLM_ERR_ARG, "%s: colptr decreases at column %d", who, j);
    const long long nnz = colptr[m];
    if (nnz > 0 && !rowidx) return fail(h, NNLM_ERR_ARG, "%s: rowidx is NULL with %lld held-out entries", who, nnz);
    if (nnz > (long long)n * (long long)m) return fail(h, NNLM_ERR_ARG, "%s: %lld held-out entries exceed n * m", who, nnz);
    for (int j = 0; j < m; j++)
        for (long long e = colptr[j]; e < colptr[j + 1]; e++) {
            const int i = rowidx[e];
            if (i < 0 || i >= n) return fail(h, NNLM_ERR_ARG, "%s: row index %d out of range at entry %lld (column %d)", who, i, e, j);
            if (e > colptr[j] && i <= rowidx[e - 1])
                return fail(h, NNLM_ERR_ARG, "%s: row indices of column %d are not strictly increasing (entry %lld)", who, j, e);
        }
    if (nnz == (long long)n * (long long)m) return fail(h, NNLM_ERR_ARG, "%s: every entry is held out; nothing is left to fit", who);
    std::vector<double> hv((size_t)nnz);
    std::vector<int> cidx((size_t)nnz);
    for (int j = 0; j < m; j++)
        for (long long e = colptr[j]; e < colptr[j + 1]; e++) cidx[e] = j;
    int rc = set_matrix_impl(h, A, n, m, colptr, rowidx, hv.data());
    if (rc != NNLM_OK) return rc;
    h->holdout = true;
    h->ho_nnz = nnz;
    const size_t es = esize(h);
    auto up = [&]() -> int {
        HIPCHK(h, hipMalloc(&h->ho_cptr, (size_t)(m + 1) * 8));
        HIPCHK(h, hipMalloc(&h->ho_ridx, (size_t)nnz * 4 + 64));
        HIPCHK(h, hipMalloc(&h->ho_cidx, (size_t)nnz * 4 + 64));
        HIPCHK(h, hipMalloc(&h->ho_val, (size_t)nnz * es + 64));
        HIPCHK(h, hipMemcpy(h->ho_cptr, colptr, (size_t)(m + 1) * 8, hipMemcpyHostToDevice));
        if (nnz > 0) {
            HIPCHK(h, hipMemcpy(h->ho_ridx, rowidx, (size_t)nnz * 4, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(h->ho_cidx, cidx.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
            if (h->prec == NNLM_PREC_F64) HIPCHK(h, hipMemcpy(h->ho_val, hv.data(), (size_t)nnz * 8, hipMemcpyHostToDevice));
            else {
                std::vector<float> hf(hv.begin(), hv.end());
                HIPCHK(h, hipMemcpy(h->ho_val, hf.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
            }
        }
        return NNLM_OK;
    };
    rc = up();
    if (rc != NNLM_OK) free_matrix(h);
    return rc;
}

// Sparse A (include/nnlm_mi355x.h): canonical CSC, absent entries are zeros.  Validated on the host, the CSR of the same matrix is built
// there too (counting sort by row: the columns of a row come out ascending), both are uploaded once in the mode's value type.
template <typename T>
static int sp_upload(nnlm_handle *h, const long long *colptr, const int *rowidx, const double *x, const std::vector<long long> &rptr,
                     const std::vector<int> &cidx, const std::vector<double> &rval)
{
    const int n = h->n, m = h->m;
    const long long nnz = h->nnz;
    const size_t vb = (size_t)nnz * sizeof(T) + 64, ib = (size_t)nnz * 4 + 64;
    HIPCHK(h, hipMalloc(&h->sp_cptr, (size_t)(m + 1) * 8));
    HIPCHK(h, hipMalloc(&h->sp_rptr, (size_t)(n + 1) * 8));
    HIPCHK(h, hipMalloc(&h->sp_ridx, ib));
    HIPCHK(h, hipMalloc(&h->sp_cidx, ib));
    HIPCHK(h, hipMalloc(&h->sp_cval, vb));
    HIPCHK(h, hipMalloc(&h->sp_rval, vb));
    h->sp_bytes = (size_t)(m + 1) * 8 + (size_t)(n + 1) * 8 + 2 * ib + 2 * vb;
    HIPCHK(h, hipMemcpy(h->sp_cptr, colptr, (size_t)(m + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->sp_rptr, rptr.data(), (size_t)(n + 1) * 8, hipMemcpyHostToDevice));
    if (nnz > 0) {
        HIPCHK(h, hipMemcpy(h->sp_ridx, rowidx, (size_t)nnz * 4, hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->sp_cidx, cidx.data(), (size_t)nnz * 4, hipMemcpyHostToDevice));
        std::vector<T> v((size_t)nnz);
        for (long long e = 0; e < nnz; e++) v[e] = (T)x[e];
        HIPCHK(h, hipMemcpy(h->sp_cval, v.data(), (size_t)nnz * sizeof(T), hipMemcpyHostToDevice));
        for (long long e = 0; e < nnz; e++) v[e] = (T)rval[e];
        HIPCHK(h, hipMemcpy(h->sp_rval, v.data(), (size_t)nnz * sizeof(T), hipMemcpyHostToDevice));
    }
    return NNLM_OK;
}

// Sparse A whose absent entries are missing (k_sparse_na.h): per orientation the host copy of the pointers, the segment slots of the
// long columns (more than SPG_SEG stored entries) in front of each column and the list of the long columns, on the device
static int spg_layout(nnlm_handle *h, int o, const long long *ptr, int ncols)
{
    h->spg_hptr[o].assign(ptr, ptr + ncols + 1);
    std::vector<long long> so((size_t)ncols + 1, 0);
    std::vector<int> lc;
    for (int c = 0; c < ncols; c++) {
        const long long len = ptr[c + 1] - ptr[c];
        const long long ns = len > SPG_SEG ? (len + SPG_SEG - 1) / SPG_SEG : 0;
        so[(size_t)c + 1] = so[c] + ns;
        if (ns) lc.push_back(c);
    }
    HIPCHK(h, hipMalloc(&h->spg_segoff[o], so.size() * 8));
    HIPCHK(h, hipMemcpy(h->spg_segoff[o], so.data(), so.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMalloc(&h->spg_longc[o], (lc.size() + 1) * 4));
    if (!lc.empty()) HIPCHK(h, hipMemcpy(h->spg_longc[o], lc.data(), lc.size() * 4, hipMemcpyHostToDevice));
    h->sp_bytes += so.size() * 8 + (lc.size() + 1) * 4;
    return NNLM_OK;
}

// Sparse A for KL loss (k_sparse_kl.h): the lines of orientation o that the long form takes
static int spkl_layout(nnlm_handle *h, int o, const long long *ptr, int ncols)
{
    std::vector<int> lc;
    const long long lim = nnlm_spkl_short_max();
    for (int c = 0; c < ncols; c++)
        if (ptr[c + 1] - ptr[c] > lim) lc.push_back(c);
    h->spkl_nlong[o] = (int)lc.size();
    h->spkl_nshort[o] = ncols - (int)lc.size();
    HIPCHK(h, hipMalloc(&h->spkl_longc[o], (lc.size() + 1) * 4));
    if (!lc.empty()) HIPCHK(h, hipMemcpy(h->spkl_longc[o], lc.data(), lc.size() * 4, hipMemcpyHostToDevice));
    h->sp_bytes += (lc.size() + 1) * 4;
    return NNLM_OK;
}

// The common tail of the sparse set-matrix entries, behind the six resident arrays: the partial sums' buffer, what absent entries are,
// the per-orientation tables of the door (host pointer arrays colptr [m + 1], rowptr [n + 1]) and the KL constant from klc = the sum of
// (v + eps) log(v + eps) - v over the stored entries.  Frees the matrix on failure.
static int sp_finish(nnlm_handle *h, const char *who, const long long *colptr, const long long *rowptr, double klc, bool absent_missing, bool kl)
{
    const int n = h->n, m = h->m;
    const long long nnz = h->nnz;
    // partial sums of the error block (three per workgroup of sp_errors_kernel) and of the penalty sums (three per 256 columns)
    const int nw = nnlm_sp_workers(nnz, 64, h->cus_device); // (the most workgroups any rank asks for: one worker per wavefront)
    const size_t eb = (size_t)(nw + 3) / 4, pb = (size_t)((n > m ? n : m) + 255) / 256;
    h->partials_elems = 3 * (eb > pb ? eb : pb) + 64;
    if (hipMalloc(&h->partials, h->partials_elems * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        free_matrix(h);
        return fail(h, NNLM_ERR_HIP, "%s: hipMalloc of %zu partial sums failed", who, h->partials_elems);
    }
    if (absent_missing) {
        h->sp_missing = true;
        h->n_non_missing = (double)nnz; // N_non_missing, src/nnmf.cpp:69
        h->any_missing = (double)nnz != (double)n * (double)m;
        h->kl_const = klc / h->n_non_missing; // src/nnmf.cpp:70: over the stored entries only
        int rl = spg_layout(h, 1, colptr, m);
        if (rl == NNLM_OK) rl = spg_layout(h, 0, rowptr, n);
        if (rl != NNLM_OK) {
            free_matrix(h);
            return rl;
        }
        return NNLM_OK;
    }
    if (kl) {
        h->sp_kl = true;
        int rl = spkl_layout(h, 1, colptr, m);
        if (rl == NNLM_OK) rl = spkl_layout(h, 0, rowptr, n);
        if (rl != NNLM_OK) {
            free_matrix(h);
            return rl;
        }
    }
    h->n_non_missing = (double)n * (double)m;
    h->any_missing = false;
    // the zeros add (n m - nnz) eps log eps
    h->kl_const = (klc + ((double)n * (double)m - (double)nnz) * (NNLM_TINY * std::log(NNLM_TINY))) / h->n_non_missing;
    return NNLM_OK;
}

// sp_finish for a handle with per-entry weights, behind the four weight arrays as well: klc is the weighted sum (-> kl_const_w), and the
// per-column path runs for the zero semantics too, so its tables are built for either
static int sp_finish_weighted(nnlm_handle *h, const char *who, const long long *colptr, const long long *rowptr, double klc, bool absent_missing)
{
    int rw = sp_finish(h, who, colptr, rowptr, klc, absent_missing, false);
    if (rw != NNLM_OK) return rw;
    if (!absent_missing) {
        rw = spg_layout(h, 1, colptr, h->m);
        if (rw == NNLM_OK) rw = spg_layout(h, 0, rowptr, h->n);
        if (rw != NNLM_OK) {
            free_matrix(h);
            return rw;
        }
    }
    h->sp_weighted = true;
    return NNLM_OK;
}

// The CSC contract of the sparse set-matrix entries, checked in the order they have always reported it (first offender named)
static int csc_check(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x, bool absent_missing, const char *who,
                     bool kl)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "%s: handle is NULL", who);
    if (n <= 0 || m <= 0 || !colptr) return fail(h, NNLM_ERR_ARG, "%s: A must be a non-empty n x m matrix with colptr[m + 1] (n=%d, m=%d)", who, n, m);
    if (h->sharded) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: a sparse matrix is single-GPU only (this handle has a communicator)", who);
    if (colptr[0] != 0) return fail(h, NNLM_ERR_ARG, "%s: colptr[0] = %lld, must be 0", who, colptr[0]);
    for (int j = 0; j < m; j++)
        if (colptr[j + 1] < colptr[j]) return fail(h, NNLM_ERR_ARG, "%s: colptr decreases at column %d", who, j);
    const long long nnz = colptr[m];
    if (nnz > 0 && (!rowidx || !x)) return fail(h, NNLM_ERR_ARG, "%s: rowidx / x is NULL with nnz = %lld", who, nnz);
    if (nnz > (long long)n * (long long)m) return fail(h, NNLM_ERR_ARG, "%s: nnz = %lld exceeds n * m", who, nnz);
    for (int j = 0; j < m; j++)
        for (long long e = colptr[j]; e < colptr[j + 1]; e++) {
            const int i = rowidx[e];
            if (i < 0 || i >= n) return fail(h, NNLM_ERR_ARG, "%s: row index %d out of range at entry %lld (column %d)", who, i, e, j);
            if (e > colptr[j] && i <= rowidx[e - 1])
                return fail(h, NNLM_ERR_ARG, "%s: row indices of column %d are not strictly increasing (entry %lld)", who, j, e);
            const double v = x[e];
            if (!std::isfinite(v))
                return fail(h, NNLM_ERR_ARG, absent_missing ? "%s: entry %lld (row %d, column %d) is not finite; a stored entry is an observation "
                                                              "(leave a missing entry out of the structure)"
                                                            : "%s: entry %lld (row %d, column %d) is not finite; a sparse matrix has no missing entries "
                                                              "(use nnlm_set_matrix for NA data)", who, e, i, j);
            if (kl && v < 0.0)
                return fail(h, NNLM_ERR_ARG, "%s: entry %lld (row %d, column %d) is negative (%g); KL loss needs non-negative data", who, e, i, j, v);
        }
    return NNLM_OK;
}

// One value array of a sparse handle in the mode's type, from its fp64 host copy (nnz + slack elements, as sp_upload sizes them)
template <typename T> static int sp_upload_values(nnlm_handle *h, void **dst, const double *src, long long nnz)
{
    const size_t vb = (size_t)nnz * sizeof(T) + 64;
    HIPCHK(h, hipMalloc(dst, vb));
    h->sp_bytes += vb;
    if (nnz > 0) {
        std::vector<T> v((size_t)nnz);
        for (long long e = 0; e < nnz; e++) v[e] = (T)src[e];
        HIPCHK(h, hipMemcpy(*dst, v.data(), (size_t)nnz * sizeof(T), hipMemcpyHostToDevice));
    }
    return NNLM_OK;
}

// nnlm_set_matrix_csc and nnlm_set_matrix_csc_missing: one contract, one body; `absent_missing` chooses what an absent entry is.
// weight != NULL (nnlm_set_matrix_csc_weighted): one weight c_e >= 0 per stored entry, in the order of x.  The handle is the one the
// unweighted door leaves for the same absent semantics (N, check_k, structure), plus the weights and the products c_e a_e (formed in
// fp64 here) in both orientations, the per-orientation tables of the per-column path for either semantics, and the weighted KL constant.
static int set_matrix_csc_impl(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x, bool absent_missing,
                               const char *who, bool kl = false, const double *weight = nullptr)
{
    const int rcc = csc_check(h, n, m, colptr, rowidx, x, absent_missing, who, kl);
    if (rcc != NNLM_OK) return rcc;
    const long long nnz = colptr[m];
    if (weight)
        for (int j = 0; j < m; j++)
            for (long long e = colptr[j]; e < colptr[j + 1]; e++)
                if (!std::isfinite(weight[e]) || weight[e] < 0.0)
                    return fail(h, NNLM_ERR_ARG, "%s: weight %g of entry %lld (row %d, column %d) is not a finite number >= 0", who, weight[e], e,
                                rowidx[e], j);
    std::vector<long long> rptr((size_t)n + 1, 0);
    double over = 0.0, mx = 0.0, wmx = 0.0, klc = 0.0;
    for (int j = 0; j < m; j++)
        for (long long e = colptr[j]; e < colptr[j + 1]; e++) {
            const int i = rowidx[e];
            const double v = x[e];
            rptr[(size_t)i + 1]++;
            if (std::fabs(v) > 3.4028234663852886e38) over += 1.0;
            const double fv = std::fabs((double)(float)v);
            if (fv > mx) mx = fv;
            if (!weight) {
                klc += (v + NNLM_TINY) * std::log(v + NNLM_TINY) - v; // src/nnmf.cpp:70,73 over the non-zeros
                continue;
            }
            // (the fp32 range rules hold for c a as for a -- the cross product reads it -- and for c itself; a weight of 1 changes nothing)
            const double c = weight[e], ca = c * v;
            if (std::fabs(v) <= 3.4028234663852886e38 && (std::fabs(ca) > 3.4028234663852886e38 || c > 3.4028234663852886e38)) over += 1.0;
            const double fca = std::fabs((double)(float)ca);
            if (fca > wmx) wmx = fca;
            klc += c * ((v + NNLM_TINY) * std::log(v + NNLM_TINY) - v);
        }
    if (h->prec == NNLM_PREC_F32 && over > 0.0)
        return fail(h, NNLM_ERR_UNSUPPORTED, "%.0f entries of A%s exceed the fp32 range (|a| > 3.4e38): the fp32-operand mode cannot hold them; "
                                             "use the strict fp64 mode (NNLM_PREC_F64, the default of the one-shot entries)", over,
                    weight ? " (or their weights, or weight * A)" : "");
    if (h->prec == NNLM_PREC_F32 && mx > 0.0 && mx < 7.8886090522101181e-31)
        return fail(h, NNLM_ERR_UNSUPPORTED, "max |A| = %.3g is too close to the bottom of the fp32 range for the fp32-operand mode; rescale A or use "
                                             "the strict fp64 mode", mx);
    if (weight && h->prec == NNLM_PREC_F32 && wmx > 0.0 && wmx < 7.8886090522101181e-31)
        return fail(h, NNLM_ERR_UNSUPPORTED, "max |weight * A| = %.3g is too close to the bottom of the fp32 range for the fp32-operand mode; rescale "
                                             "or use the strict fp64 mode", wmx);
    for (int i = 0; i < n; i++) rptr[(size_t)i + 1] += rptr[i];
    std::vector<int> cidx((size_t)nnz);
    std::vector<double> rval((size_t)nnz), cwa, rwt, rwa; // (weighted: c a in CSC order; c and c a permuted to the CSR exactly as rval)
    if (weight) cwa.resize((size_t)nnz), rwt.resize((size_t)nnz), rwa.resize((size_t)nnz);
    {
        std::vector<long long> next(rptr.begin(), rptr.end() - 1);
        for (int j = 0; j < m; j++)
            for (long long e = colptr[j]; e < colptr[j + 1]; e++) {
                const long long d = next[rowidx[e]]++;
                cidx[d] = j;
                rval[d] = x[e];
                if (weight) rwt[d] = weight[e], cwa[e] = rwa[d] = weight[e] * x[e];
            }
    }
    HIPCHK(h, hipSetDevice(h->device));
    sync_all(h);
    free_factors(h);
    free_matrix(h);
    h->n = n;
    h->m = m;
    h->npad = round_up_i(n, NNLM_PAD_N); // (the factors keep their padded layouts)
    h->mpad = round_up_i(m, NNLM_PAD_M);
    h->sparse = true;
    h->x16 = false;
    h->nnz = nnz;
    const int rc = h->prec == NNLM_PREC_F64 ? sp_upload<double>(h, colptr, rowidx, x, rptr, cidx, rval) : sp_upload<float>(h, colptr, rowidx, x, rptr, cidx, rval);
    if (rc != NNLM_OK) {
        free_matrix(h);
        return rc;
    }
    if (!weight) return sp_finish(h, who, colptr, rptr.data(), klc, absent_missing, kl);
    auto up = [&](void **dst, const double *src) {
        return h->prec == NNLM_PREC_F64 ? sp_upload_values<double>(h, dst, src, nnz) : sp_upload_values<float>(h, dst, src, nnz);
    };
    int rw = up(&h->sp_cwt, weight);
    if (rw == NNLM_OK) rw = up(&h->sp_rwt, rwt.data());
    if (rw == NNLM_OK) rw = up(&h->sp_cwa, cwa.data());
    if (rw == NNLM_OK) rw = up(&h->sp_rwa, rwa.data());
    if (rw != NNLM_OK) {
        free_matrix(h);
        return rw;
    }
    return sp_finish_weighted(h, who, colptr, rptr.data(), klc, absent_missing);
}

extern "C" int nnlm_set_matrix_csc(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x)
{
    return set_matrix_csc_impl(h, n, m, colptr, rowidx, x, false, "nnlm_set_matrix_csc");
}

extern "C" int nnlm_set_matrix_csc_missing(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x)
{
    return set_matrix_csc_impl(h, n, m, colptr, rowidx, x, true, "nnlm_set_matrix_csc_missing");
}

extern "C" int nnlm_set_matrix_csc_weighted(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x,
                                            const double *weight, int absent_missing)
{
    const char *who = "nnlm_set_matrix_csc_weighted";
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "%s: handle is NULL", who);
    if (!weight) return fail(h, NNLM_ERR_ARG, "%s: weight is NULL (one weight per stored entry, in the order of x)", who);
    return set_matrix_csc_impl(h, n, m, colptr, rowidx, x, absent_missing != 0, who, false, weight);
}

extern "C" int nnlm_set_matrix_csc_kl(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x)
{
    return set_matrix_csc_impl(h, n, m, colptr, rowidx, x, false, "nnlm_set_matrix_csc_kl", true);
}

// The sparse KL handle of nnlm_set_matrix_csc_kl (same arguments, checks, resident layout and long-line lists) that the batch entries also
// accept, with all four methods: the flag is all that differs
extern "C" int nnlm_set_matrix_csc_kl_batch(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x)
{
    const int rc = set_matrix_csc_impl(h, n, m, colptr, rowidx, x, false, "nnlm_set_matrix_csc_kl_batch", true);
    if (rc == NNLM_OK) h->sp_batch = true;
    return rc;
}

// The sparse handle of nnlm_set_matrix_csc (same arguments, checks and resident layout; absent entries are zeros) that the batch entries
// also accept: the flag is all that differs
extern "C" int nnlm_set_matrix_csc_batch(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x)
{
    const int rc = set_matrix_csc_impl(h, n, m, colptr, rowidx, x, false, "nnlm_set_matrix_csc_batch");
    if (rc == NNLM_OK) h->sp_batch = true;
    return rc;
}

// The sparse-missing handle of nnlm_set_matrix_csc_missing that the batch entries also accept, with an optional
// hold-out pattern (canonical CSC, a subset of the stored pattern; ho_colptr == NULL: none).  Held-out entries leave the stored set on the
// host, before the CSC and the CSR are built: the resident matrix IS the plain upload of the training entries.  Their values stay in
// ho_cptr / ho_ridx / ho_cidx / ho_val (the mode's type), as nnlm_set_matrix_holdout keeps them, for nnlm_holdout_errors.
extern "C" int nnlm_set_matrix_csc_missing_batch(nnlm_handle *h, int n, int m, const long long *colptr, const int *rowidx, const double *x,
                                                 const long long *ho_colptr, const int *ho_rowidx)
{
    const char *who = "nnlm_set_matrix_csc_missing_batch";
    if (!ho_colptr) {
        const int rc = set_matrix_csc_impl(h, n, m, colptr, rowidx, x, true, who);
        if (rc == NNLM_OK) h->sp_batch = true;
        return rc;
    }
    int rc = csc_check(h, n, m, colptr, rowidx, x, true, who, false);
    if (rc != NNLM_OK) return rc;
    const long long nnz = colptr[m];
    if (ho_colptr[0] != 0) return fail(h, NNLM_ERR_ARG, "%s: ho_colptr[0] = %lld, must be 0", who, ho_colptr[0]);
    for (int j = 0; j < m; j++)
        if (ho_colptr[j + 1] < ho_colptr[j]) return fail(h, NNLM_ERR_ARG, "%s: ho_colptr decreases at column %d", who, j);
    const long long hn = ho_colptr[m];
    if (hn > 0 && !ho_rowidx) return fail(h, NNLM_ERR_ARG, "%s: ho_rowidx is NULL with %lld held-out entries", who, hn);
    // one merge per column: every held-out row must be a stored row of that column; what is not held out is the training set
    std::vector<long long> tptr((size_t)m + 1, 0);
    std::vector<int> tidx, hcol((size_t)hn);
    std::vector<double> tval, hval((size_t)hn);
    tidx.reserve((size_t)(nnz > hn ? nnz - hn : 0));
    tval.reserve(tidx.capacity());
    for (int j = 0; j < m; j++) {
        long long e = colptr[j];
        const long long e1 = colptr[j + 1];
        for (long long g = ho_colptr[j]; g < ho_colptr[j + 1]; g++) {
            const int i = ho_rowidx[g];
            if (i < 0 || i >= n) return fail(h, NNLM_ERR_ARG, "%s: held-out row index %d out of range at entry %lld (column %d)", who, i, g, j);
            if (g > ho_colptr[j] && i <= ho_rowidx[g - 1])
                return fail(h, NNLM_ERR_ARG, "%s: held-out row indices of column %d are not strictly increasing (entry %lld)", who, j, g);
            for (; e < e1 && rowidx[e] < i; e++) tidx.push_back(rowidx[e]), tval.push_back(x[e]);
            if (e >= e1 || rowidx[e] != i)
                return fail(h, NNLM_ERR_ARG, "%s: held-out entry %lld (row %d, column %d) is not a stored entry", who, g, i, j);
            hcol[(size_t)g] = j;
            hval[(size_t)g] = x[e++];
        }
        for (; e < e1; e++) tidx.push_back(rowidx[e]), tval.push_back(x[e]);
        tptr[(size_t)j + 1] = (long long)tidx.size();
    }
    if (nnz > 0 && hn == nnz) return fail(h, NNLM_ERR_ARG, "%s: every stored entry is held out; nothing is left to fit", who);
    rc = set_matrix_csc_impl(h, n, m, tptr.data(), tidx.data(), tval.data(), true, who);
    if (rc != NNLM_OK) return rc;
    h->sp_batch = true;
    h->holdout = true;
    h->ho_nnz = hn;
    const size_t es = esize(h);
    auto up = [&]() -> int {
        HIPCHK(h, hipMalloc(&h->ho_cptr, (size_t)(m + 1) * 8));
        HIPCHK(h, hipMalloc(&h->ho_ridx, (size_t)hn * 4 + 64));
        HIPCHK(h, hipMalloc(&h->ho_cidx, (size_t)hn * 4 + 64));
        HIPCHK(h, hipMalloc(&h->ho_val, (size_t)hn * es + 64));
        HIPCHK(h, hipMemcpy(h->ho_cptr, ho_colptr, (size_t)(m + 1) * 8, hipMemcpyHostToDevice));
        if (hn > 0) {
            HIPCHK(h, hipMemcpy(h->ho_ridx, ho_rowidx, (size_t)hn * 4, hipMemcpyHostToDevice));
            HIPCHK(h, hipMemcpy(h->ho_cidx, hcol.data(), (size_t)hn * 4, hipMemcpyHostToDevice));
            if (h->prec == NNLM_PREC_F64) HIPCHK(h, hipMemcpy(h->ho_val, hval.data(), (size_t)hn * 8, hipMemcpyHostToDevice));
            else {
                std::vector<float> hf(hval.begin(), hval.end());
                HIPCHK(h, hipMemcpy(h->ho_val, hf.data(), (size_t)hn * 4, hipMemcpyHostToDevice));
            }
        }
        return NNLM_OK;
    };
    rc = up();
    if (rc != NNLM_OK) free_matrix(h);
    return rc;
}

// Sparse A that already lives in device memory (include/nnlm_mi355x.h, DESIGN section 4.21, k_sparse_ingest.h): the work of
// set_matrix_csc_impl as kernels.  Everything is built in allocations of its own; the handle is touched only after the last stage has
// succeeded, so a refusal leaves its previous matrix and factors alone.
namespace {
struct SpiBufs { // device allocations of one ingest: released at the end of the call unless the handle has taken them
    std::vector<void *> v;
    ~SpiBufs()
    {
        for (void *p : v) hipFree(p);
    }
    template <typename P> bool get(P **p, size_t bytes)
    {
        void *q = nullptr;
        if (hipMalloc(&q, bytes ? bytes : 8) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        v.push_back(q);
        *p = (P *)q;
        return true;
    }
    void release(void *p) { v.erase(std::find(v.begin(), v.end(), p)); } // (the handle owns it now)
};
} // namespace

// One of the three arrays of a nnlm_dev_sparse, len contiguous elements of es bytes: dev_matrix_check's rules for a pointer (alignment,
// device or managed memory of the handle's device, the extent inside its allocation, not a buffer of the handle), before a kernel reads it
static int dev_array_check(nnlm_handle *h, const char *who, const char *name, const void *ptr, size_t es, long long len)
{
    if ((uintptr_t)ptr % es) return fail(h, NNLM_ERR_ARG, "%s: %s is not aligned to its %zu-byte elements", who, name, es);
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof at);
    const hipError_t e = hipPointerGetAttributes(&at, ptr);
    (void)hipGetLastError(); // (the query leaves a sticky error behind for a pointer the runtime does not know)
    if (e != hipSuccess || (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged))
        return fail(h, NNLM_ERR_ARG, "%s: %s is not device (or managed) memory -- a host pointer?", who, name);
    if (at.type == hipMemoryTypeDevice && at.device != h->device)
        return fail(h, NNLM_ERR_ARG, "%s: %s lives on device %d, the handle on device %d", who, name, at.device, h->device);
    void *base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(ptr)) == hipSuccess) {
        const size_t span = (size_t)len * es;
        if ((const char *)ptr + span > (const char *)base + size)
            return fail(h, NNLM_ERR_ARG, "%s: %s (%lld elements) reaches %zu bytes past the end of its allocation", who, name, len,
                        (size_t)(((const char *)ptr + span) - ((const char *)base + size)));
        if (owns_allocation(h, base)) return fail(h, NNLM_ERR_ARG, "%s: %s aliases a buffer of the handle itself", who, name);
    } else
        (void)hipGetLastError();
    return NNLM_OK;
}

// The body of nnlm_set_matrix_sparse_device (weighted = false: Wt is not looked at, `door` holds the door bits) and of
// nnlm_set_matrix_sparse_device_weighted (weighted = true: `door` holds NNLM_SP_ABSENT_MISSING or 0).  The weights add the descriptor
// checks, two stages between the entry check and the range rules -- their pattern (when they bring one), then the weights themselves --
// two payloads of the sort and four resident arrays; everything else is one code path.
static int sparse_device_impl(nnlm_handle *h, const char *who, const nnlm_dev_sparse *A, bool weighted, const nnlm_dev_sparse *Wt, int n, int m,
                              int door, void *stream)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "%s: handle is NULL", who);
    if (!A) return fail(h, NNLM_ERR_ARG, "%s: A is NULL", who);
    if (A->layout != NNLM_SP_CSC && A->layout != NNLM_SP_CSR)
        return fail(h, NNLM_ERR_ARG, "%s: A.layout = %d is neither NNLM_SP_CSC nor NNLM_SP_CSR", who, A->layout);
    const bool csc = A->layout == NNLM_SP_CSC;
    const char *pname = csc ? "colptr" : "rowptr", *lname = csc ? "column" : "row", *iname = csc ? "row" : "column";
    if (n <= 0 || m <= 0 || !A->ptr)
        return fail(h, NNLM_ERR_ARG, "%s: A must be a non-empty n x m matrix with %s[%s + 1] (n=%d, m=%d)", who, pname, csc ? "m" : "n", n, m);
    if ((A->ptr_dtype != NNLM_IT_I32 && A->ptr_dtype != NNLM_IT_I64) || (A->idx_dtype != NNLM_IT_I32 && A->idx_dtype != NNLM_IT_I64))
        return fail(h, NNLM_ERR_ARG, "%s: A.ptr_dtype = %d, A.idx_dtype = %d: each must be NNLM_IT_I32 or NNLM_IT_I64", who, A->ptr_dtype, A->idx_dtype);
    if (A->val_dtype < NNLM_DT_F64 || A->val_dtype > NNLM_DT_BF16)
        return fail(h, NNLM_ERR_ARG, "%s: A.val_dtype = %d is not one of NNLM_DT_F64 .. NNLM_DT_BF16", who, A->val_dtype);
    const int all_doors = NNLM_SP_ABSENT_MISSING | NNLM_SP_KL | NNLM_SP_BATCH;
    if (door < 0 || (door & ~all_doors))
        return fail(h, NNLM_ERR_ARG, "%s: door = %d has bits other than NNLM_SP_ABSENT_MISSING, NNLM_SP_KL and NNLM_SP_BATCH", who, door);
    const bool absent_missing = door & NNLM_SP_ABSENT_MISSING, kl = door & NNLM_SP_KL, batch = door & NNLM_SP_BATCH;
    if (absent_missing && kl)
        return fail(h, NNLM_ERR_ARG, "%s: door = NNLM_SP_ABSENT_MISSING | NNLM_SP_KL: KL loss on a sparse matrix takes absent entries as zeros", who);
    if (h->sharded) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: a sparse matrix is single-GPU only (this handle has a communicator)", who);
    const long long nnz = A->nnz;
    if (nnz < 0) return fail(h, NNLM_ERR_ARG, "%s: nnz = %lld is negative", who, nnz);
    if (nnz > 0 && (!A->idx || !A->val)) return fail(h, NNLM_ERR_ARG, "%s: idx / val is NULL with nnz = %lld", who, nnz);
    const int lines = csc ? m : n, other = csc ? n : m; // lines of the given side, of the side to build
    const bool p64 = A->ptr_dtype == NNLM_IT_I64, i64 = A->idx_dtype == NNLM_IT_I64, f64 = h->prec == NNLM_PREC_F64;
    // the weights: aligned with A.val (no ptr, no idx), or a sparse matrix of A's layout whose pattern stage 2a compares with A's
    const bool wpat = weighted && Wt && Wt->ptr && Wt->idx;
    bool wp64 = false, wi64 = false;
    if (weighted) {
        if (!Wt) return fail(h, NNLM_ERR_ARG, "%s: Wt is NULL (one weight per stored entry)", who);
        if ((Wt->ptr == nullptr) != (Wt->idx == nullptr))
            return fail(h, NNLM_ERR_ARG, "%s: Wt.ptr and Wt.idx must both be NULL (weights in the order of A.val) or both be given (weights as a "
                                         "sparse matrix of A's pattern)", who);
        if (Wt->val_dtype < NNLM_DT_F64 || Wt->val_dtype > NNLM_DT_BF16)
            return fail(h, NNLM_ERR_ARG, "%s: Wt.val_dtype = %d is not one of NNLM_DT_F64 .. NNLM_DT_BF16", who, Wt->val_dtype);
        if (Wt->nnz < 0) return fail(h, NNLM_ERR_ARG, "%s: Wt.nnz = %lld is negative", who, Wt->nnz);
        if (wpat) {
            if (Wt->layout != A->layout)
                return fail(h, NNLM_ERR_ARG, "%s: Wt.layout = %d differs from A.layout = %d", who, Wt->layout, A->layout);
            if ((Wt->ptr_dtype != NNLM_IT_I32 && Wt->ptr_dtype != NNLM_IT_I64) || (Wt->idx_dtype != NNLM_IT_I32 && Wt->idx_dtype != NNLM_IT_I64))
                return fail(h, NNLM_ERR_ARG, "%s: Wt.ptr_dtype = %d, Wt.idx_dtype = %d: each must be NNLM_IT_I32 or NNLM_IT_I64", who, Wt->ptr_dtype,
                            Wt->idx_dtype);
            wp64 = Wt->ptr_dtype == NNLM_IT_I64, wi64 = Wt->idx_dtype == NNLM_IT_I64;
        } else if (Wt->nnz != nnz) // (weights with a pattern of their own: the pattern stage names the first line that differs)
            return fail(h, NNLM_ERR_ARG, "%s: Wt.nnz = %lld, but A.nnz = %lld (one weight per stored entry, in the order of A.val)", who, Wt->nnz, nnz);
        if (Wt->nnz > 0 && !Wt->val) return fail(h, NNLM_ERR_ARG, "%s: Wt.val is NULL with Wt.nnz = %lld", who, Wt->nnz);
    }
    HIPCHK(h, hipSetDevice(h->device));
    int rc = dev_array_check(h, who, "A.ptr", A->ptr, p64 ? 8 : 4, (long long)lines + 1);
    if (rc == NNLM_OK && nnz > 0) rc = dev_array_check(h, who, "A.idx", A->idx, i64 ? 8 : 4, nnz);
    if (rc == NNLM_OK && nnz > 0) rc = dev_array_check(h, who, "A.val", A->val, dt_size(A->val_dtype), nnz);
    if (rc == NNLM_OK && wpat) rc = dev_array_check(h, who, "Wt.ptr", Wt->ptr, wp64 ? 8 : 4, (long long)lines + 1);
    if (rc == NNLM_OK && wpat && Wt->nnz > 0) rc = dev_array_check(h, who, "Wt.idx", Wt->idx, wi64 ? 8 : 4, Wt->nnz);
    if (rc == NNLM_OK && weighted && Wt->nnz > 0) rc = dev_array_check(h, who, "Wt.val", Wt->val, dt_size(Wt->val_dtype), Wt->nnz);
    if (rc != NNLM_OK) return rc;
    g_attr_err = hipSuccess;
    hipStream_t st = h->stream;
    if ((rc = stream_after(h, st, (hipStream_t)stream)) != NNLM_OK) return rc; // the caller's stream produced the arrays
    auto hipfail = [&](const char *what, hipError_t e) {
        hipStreamSynchronize(st); // (nothing of this call is left in flight over buffers about to be freed)
        (void)hipGetLastError();
        return fail(h, NNLM_ERR_HIP, "%s: %s failed: %s", who, what, hipGetErrorString(e));
    };
    auto nomem = [&](const char *what) {
        hipStreamSynchronize(st);
        return fail(h, NNLM_ERR_HIP, "%s: hipMalloc of %s failed (nnz = %lld)", who, what, nnz);
    };

    SpiBufs bufs;
    const size_t es = f64 ? 8 : 4, vb = (size_t)nnz * es + 64, ib = (size_t)nnz * 4 + 64; // (sp_upload's sizes)
    long long *gptr = nullptr, *optr = nullptr; // the given side's resident arrays, the built side's
    int *gidx = nullptr, *oidx = nullptr;
    void *gval = nullptr, *oval = nullptr;
    if (!bufs.get(&gptr, (size_t)(lines + 1) * 8) || !bufs.get(&optr, (size_t)(other + 1) * 8) || !bufs.get(&gidx, ib) || !bufs.get(&oidx, ib) ||
        !bufs.get(&gval, vb) || !bufs.get(&oval, vb))
        return nomem("the resident arrays");
    void *gwt = nullptr, *owt = nullptr, *gwa = nullptr, *owa = nullptr; // the weights and the products c a, given side / built side
    if (weighted && (!bufs.get(&gwt, vb) || !bufs.get(&owt, vb) || !bufs.get(&gwa, vb) || !bufs.get(&owa, vb))) return nomem("the resident weights");
    std::vector<long long> hg, ho; // host copies of the two pointer arrays
    std::vector<long long> hcode;
    std::vector<double> hstat;
    const int nb_ptr = (lines + 256) / 256;
    const long long share = nnlm_spi_check_share(), tile = nnlm_spi_sort_tile(), stile = nnlm_spi_scan_tile();
    const int nb_chk = (int)((nnz + share - 1) / share), nb_sort = (int)((nnz + tile - 1) / tile);
    const int nb_pidx = wpat ? (int)((nnz + 255) / 256) : 0; // (the index comparison of the weights' pattern: one thread per entry)
    try {
        hg.resize((size_t)lines + 1);
        ho.resize((size_t)other + 1);
        hcode.resize((size_t)std::max(std::max(nb_ptr, nb_chk), nb_pidx));
        hstat.resize(3 * (size_t)nb_chk);
    } catch (...) {
        return fail(h, NNLM_ERR_HIP, "%s: host buffers for %d + %d pointers", who, n + 1, m + 1);
    }
    ProfScope ps_all(h, P_SP_INGEST);

    // stage 1: the pointers
    long long *dcode = nullptr;
    double *dstat = nullptr;
    if (!bufs.get(&dcode, hcode.size() * 8) || !bufs.get(&dstat, hstat.size() * 8)) return nomem("the per-block verdicts");
    {
        ProfScope ps(h, P_SP_INGEST_PTR);
        nnlm_tu_spi_ptr(A->ptr, p64, lines, nnz, gptr, dcode, st);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(hcode.data(), dcode, (size_t)nb_ptr * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(hg.data(), gptr, (size_t)(lines + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hipfail("the pointer check", e);
    {
        long long first = LLONG_MAX;
        for (int b = 0; b < nb_ptr; b++) first = hcode[b] < first ? hcode[b] : first;
        if (first == 0) return fail(h, NNLM_ERR_ARG, "%s: %s[0] = %lld, must be 0", who, pname, hg[0]);
        if (first <= lines) return fail(h, NNLM_ERR_ARG, "%s: %s decreases at %s %d", who, pname, lname, (int)(first - 1));
        if (first == (long long)lines + 1)
            return fail(h, NNLM_ERR_ARG, "%s: %s[%d] = %lld, but A.nnz = %lld", who, pname, lines, hg[(size_t)lines], nnz);
    }
    if (nnz > (long long)n * (long long)m) return fail(h, NNLM_ERR_ARG, "%s: nnz = %lld exceeds n * m", who, nnz);

    // stage 2: the entries, on pointers that hold; the given side's indices and values land in their resident types
    const int bits = other <= 1 ? 0 : 32 - __builtin_clz((unsigned)(other - 1)), passes = (bits + 7) / 8;
    int *ltmp = nullptr, *keyb = nullptr, *keyc = nullptr; // line numbers' other buffer; the keys after an odd / an even pass
    void *vtmp = nullptr, *wtmp = nullptr, *atmp = nullptr;
    long long *ghist = nullptr, *bsum = nullptr;
    const long long scan_len = 256LL * nb_sort > (long long)other + 1 ? 256LL * nb_sort : (long long)other + 1;
    if (nnz > 0) {
        if (passes >= 1 && (!bufs.get(&ltmp, ib) || !bufs.get(&vtmp, vb) || !bufs.get(&ghist, 256 * (size_t)nb_sort * 8))) return nomem("the sort buffers");
        if (passes >= 1 && weighted && (!bufs.get(&wtmp, vb) || !bufs.get(&atmp, vb))) return nomem("the sort buffers");
        if (passes >= 2 && !bufs.get(&keyb, ib)) return nomem("the sort buffers");
        if (passes >= 3 && !bufs.get(&keyc, ib)) return nomem("the sort buffers");
    }
    if (!bufs.get(&bsum, (size_t)((scan_len + stile - 1) / stile) * 8)) return nomem("the scan buffer");
    // the entries' line numbers and values start where an even number of passes ends in the resident arrays
    int *lcur = (passes & 1) ? ltmp : oidx, *lnext = (passes & 1) ? oidx : ltmp;
    void *vcur = (passes & 1) ? vtmp : oval, *vnext = (passes & 1) ? oval : vtmp;
    void *wcur = (passes & 1) ? wtmp : owt, *wnext = (passes & 1) ? owt : wtmp;
    void *acur = (passes & 1) ? atmp : owa, *anext = (passes & 1) ? owa : atmp;
    double over = 0.0, mx = 0.0, wmx = 0.0, klc = 0.0;
    if (nnz > 0) {
        {
            ProfScope ps(h, P_SP_INGEST_CHECK);
            nnlm_tu_spi_check(gptr, lines, A->idx, i64, A->val, A->val_dtype, f64, nnz, other, kl, gidx, gval, vcur, lcur, dcode, dstat, st);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(hcode.data(), dcode, (size_t)nb_chk * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hstat.data(), dstat, 3 * (size_t)nb_chk * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hipfail("the entry check", e);
        long long first = LLONG_MAX;
        for (int b = 0; b < nb_chk; b++) first = hcode[b] < first ? hcode[b] : first;
        if (first != LLONG_MAX) {
            const long long eo = first >> 3;
            const int kind = (int)(first & 7);
            long long *di = dcode; // (the verdicts are read: their buffers carry the offender's index and value)
            long long oi = 0;
            double ov = 0.0;
            nnlm_tu_spi_fetch(A->idx, i64, A->val, A->val_dtype, eo, di, dstat, st);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(&oi, di, 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(&ov, dstat, 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hipfail("reading the offending entry", e);
            const int j = (int)(std::upper_bound(hg.begin(), hg.end(), eo) - hg.begin()) - 1;
            if (kind == 0) return fail(h, NNLM_ERR_ARG, "%s: %s index %lld out of range at entry %lld (%s %d)", who, iname, oi, eo, lname, j);
            if (kind == 1) return fail(h, NNLM_ERR_ARG, "%s: %s indices of %s %d are not strictly increasing (entry %lld)", who, iname, lname, j, eo);
            if (kind == 2)
                return fail(h, NNLM_ERR_ARG, absent_missing ? "%s: entry %lld (%s %lld, %s %d) is not finite; a stored entry is an observation "
                                                              "(leave a missing entry out of the structure)"
                                                            : "%s: entry %lld (%s %lld, %s %d) is not finite; a sparse matrix has no missing entries "
                                                              "(use nnlm_set_matrix for NA data)", who, eo, iname, oi, lname, j);
            return fail(h, NNLM_ERR_ARG, "%s: entry %lld (%s %lld, %s %d) is negative (%g); KL loss needs non-negative data", who, eo, iname, oi, lname, j, ov);
        }
        for (int b = 0; b < nb_chk; b++) { // block order, as ingest_fill sums
            over += hstat[3 * (size_t)b];
            if (hstat[3 * (size_t)b + 1] > mx) mx = hstat[3 * (size_t)b + 1];
            klc += hstat[3 * (size_t)b + 2];
        }
    }
    // stage 2a: the pattern the weights bring, against the accepted one: pointers first, indices only behind equal pointers
    if (wpat) {
        long long first = LLONG_MAX;
        {
            ProfScope ps(h, P_SP_INGEST_CHECK);
            nnlm_tu_spi_pattern_ptr(Wt->ptr, wp64, gptr, lines, dcode, st);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(hcode.data(), dcode, (size_t)nb_ptr * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hipfail("the pattern check of the weights", e);
        for (int b = 0; b < nb_ptr; b++) first = hcode[b] < first ? hcode[b] : first;
        if (first == LLONG_MAX && Wt->nnz != nnz)
            return fail(h, NNLM_ERR_ARG, "%s: Wt.nnz = %lld, but the pointers of the weights end at %lld", who, Wt->nnz, nnz);
        if (first == LLONG_MAX && nnz > 0) {
            {
                ProfScope ps(h, P_SP_INGEST_CHECK);
                nnlm_tu_spi_pattern_idx(Wt->idx, wi64, gidx, nnz, dcode, st);
            }
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(hcode.data(), dcode, (size_t)nb_pidx * 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hipfail("the pattern check of the weights", e);
            long long eo = LLONG_MAX;
            for (int b = 0; b < nb_pidx; b++) eo = hcode[b] < eo ? hcode[b] : eo;
            if (eo != LLONG_MAX) first = (long long)(std::upper_bound(hg.begin(), hg.end(), eo) - hg.begin()) - 1;
        }
        if (first != LLONG_MAX)
            return fail(h, NNLM_ERR_ARG, "%s: the stored pattern of weights differs from the matrix's (first in %s %d)", who, lname, (int)first);
    }
    // stage 2b: the weights themselves, c a and what the range rules and the KL constant need of them
    if (weighted && nnz > 0) {
        {
            ProfScope ps(h, P_SP_INGEST_CHECK);
            nnlm_tu_spi_wcheck(A->val, A->val_dtype, Wt->val, Wt->val_dtype, f64, nnz, gwt, wcur, gwa, acur, dcode, dstat, st);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(hcode.data(), dcode, (size_t)nb_chk * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(hstat.data(), dstat, 3 * (size_t)nb_chk * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return hipfail("the weight check", e);
        long long eo = LLONG_MAX;
        for (int b = 0; b < nb_chk; b++) eo = hcode[b] < eo ? hcode[b] : eo;
        if (eo != LLONG_MAX) {
            long long oi = 0;
            double ow = 0.0;
            nnlm_tu_spi_fetch(A->idx, i64, Wt->val, Wt->val_dtype, eo, dcode, dstat, st);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(&oi, dcode, 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipMemcpyAsync(&ow, dstat, 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hipfail("reading the offending weight", e);
            const int j = (int)(std::upper_bound(hg.begin(), hg.end(), eo) - hg.begin()) - 1;
            return fail(h, NNLM_ERR_ARG, "%s: weight %g of entry %lld (row %d, column %d) is not a finite number >= 0", who, ow, eo,
                        csc ? (int)oi : j, csc ? j : (int)oi);
        }
        klc = 0.0; // (the weighted sum takes the place of the plain one)
        for (int b = 0; b < nb_chk; b++) {
            over += hstat[3 * (size_t)b];
            if (hstat[3 * (size_t)b + 1] > wmx) wmx = hstat[3 * (size_t)b + 1];
            klc += hstat[3 * (size_t)b + 2];
        }
    }
    if (!f64 && over > 0.0)
        return fail(h, NNLM_ERR_UNSUPPORTED, "%.0f entries of A%s exceed the fp32 range (|a| > 3.4e38): the fp32-operand mode cannot hold them; "
                                             "use the strict fp64 mode (NNLM_PREC_F64, the default of the one-shot entries)", over,
                    weighted ? " (or their weights, or weight * A)" : "");
    if (!f64 && mx > 0.0 && mx < 7.8886090522101181e-31)
        return fail(h, NNLM_ERR_UNSUPPORTED, "max |A| = %.3g is too close to the bottom of the fp32 range for the fp32-operand mode; rescale A or use "
                                             "the strict fp64 mode", mx);
    if (!f64 && wmx > 0.0 && wmx < 7.8886090522101181e-31)
        return fail(h, NNLM_ERR_UNSUPPORTED, "max |weight * A| = %.3g is too close to the bottom of the fp32 range for the fp32-operand mode; rescale "
                                             "or use the strict fp64 mode", wmx);

    // stage 3: the other side, on indices that hold
    {
        ProfScope ps(h, P_SP_INGEST_BUILD);
        e = hipMemsetAsync(optr, 0, (size_t)(other + 1) * 8, st);
        if (e == hipSuccess && nnz > 0) {
            nnlm_tu_spi_count(gidx, nnz, optr, st);
            nnlm_tu_spi_scan(optr, (long long)other + 1, bsum, st);
            const int *kin = gidx;
            for (int p = 0; p < passes; p++) {
                int *kout = p == passes - 1 ? nullptr : ((p & 1) ? keyc : keyb);
                if (weighted) nnlm_tu_spi_sort_pass(kin, lcur, vcur, kout, lnext, vnext, f64, nnz, 8 * p, ghist, bsum, st, wcur, acur, wnext, anext);
                else nnlm_tu_spi_sort_pass(kin, lcur, vcur, kout, lnext, vnext, f64, nnz, 8 * p, ghist, bsum, st);
                kin = kout;
                std::swap(lcur, lnext);
                std::swap(vcur, vnext);
                std::swap(wcur, wnext);
                std::swap(acur, anext);
            }
        }
    }
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ho.data(), optr, (size_t)(other + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st); // the last read of the caller's arrays was in stage 2
    if (e != hipSuccess) return hipfail("building the other side", e);

    // the handle takes the six arrays: from here on this is set_matrix_csc_impl behind its uploads
    sync_all(h);
    free_factors(h);
    free_matrix(h);
    h->n = n;
    h->m = m;
    h->npad = round_up_i(n, NNLM_PAD_N);
    h->mpad = round_up_i(m, NNLM_PAD_M);
    h->sparse = true;
    h->x16 = false;
    h->nnz = nnz;
    h->sp_cptr = csc ? gptr : optr, h->sp_rptr = csc ? optr : gptr;
    h->sp_ridx = csc ? gidx : oidx, h->sp_cidx = csc ? oidx : gidx;
    h->sp_cval = csc ? gval : oval, h->sp_rval = csc ? oval : gval;
    for (void *p : {(void *)gptr, (void *)optr, (void *)gidx, (void *)oidx, gval, oval}) bufs.release(p);
    h->sp_bytes = (size_t)(m + 1) * 8 + (size_t)(n + 1) * 8 + 2 * ib + 2 * vb;
    if (weighted) {
        h->sp_cwt = csc ? gwt : owt, h->sp_rwt = csc ? owt : gwt;
        h->sp_cwa = csc ? gwa : owa, h->sp_rwa = csc ? owa : gwa;
        for (void *p : {gwt, owt, gwa, owa}) bufs.release(p);
        h->sp_bytes += 4 * vb;
    }
    const std::vector<long long> &hc = csc ? hg : ho, &hr = csc ? ho : hg;
    rc = weighted ? sp_finish_weighted(h, who, hc.data(), hr.data(), klc, absent_missing) : sp_finish(h, who, hc.data(), hr.data(), klc, absent_missing, kl);
    if (rc != NNLM_OK) return rc;
    h->sp_batch = batch;
    if (absent_missing) { // the fewest stored entries of a column / of a row
        long long mc = LLONG_MAX, mr = LLONG_MAX;
        for (int j = 0; j < m; j++) mc = std::min(mc, hc[(size_t)j + 1] - hc[j]);
        for (int i = 0; i < n; i++) mr = std::min(mr, hr[(size_t)i + 1] - hr[i]);
        h->min_obs[0] = (int)mc, h->min_obs[1] = (int)mr;
    } else
        h->min_obs[0] = n, h->min_obs[1] = m;
    return NNLM_OK;
}

extern "C" int nnlm_set_matrix_sparse_device(nnlm_handle *h, const nnlm_dev_sparse *A, int n, int m, int door, void *stream)
{
    return sparse_device_impl(h, "nnlm_set_matrix_sparse_device", A, false, nullptr, n, m, door, stream);
}

extern "C" int nnlm_set_matrix_sparse_device_weighted(nnlm_handle *h, const nnlm_dev_sparse *A, const nnlm_dev_sparse *Wt, int n, int m,
                                                      int absent_missing, void *stream)
{
    return sparse_device_impl(h, "nnlm_set_matrix_sparse_device_weighted", A, true, Wt, n, m, absent_missing ? NNLM_SP_ABSENT_MISSING : 0, stream);
}

// One value array of a sparse handle (the mode's type, nnz elements), widened to fp64 on the host
static int sp_download_values(nnlm_handle *h, double *out, const void *src)
{
    const size_t nnz = (size_t)h->nnz;
    if (h->prec == NNLM_PREC_F64) HIPCHK(h, hipMemcpy(out, src, nnz * 8, hipMemcpyDeviceToHost));
    else {
        std::vector<float> f(nnz);
        HIPCHK(h, hipMemcpy(f.data(), src, nnz * 4, hipMemcpyDeviceToHost));
        for (size_t e = 0; e < nnz; e++) out[e] = (double)f[e];
    }
    return NNLM_OK;
}

extern "C" int nnlm_debug_sparse_resident(nnlm_handle *h, int side, long long *ptr_out, int *idx_out, double *val_out)
{
    const char *who = "nnlm_debug_sparse_resident";
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "%s: handle is NULL", who);
    if (!h->sparse) return fail(h, NNLM_ERR_ARG, "%s: the handle holds no sparse matrix", who);
    if (side != 0 && side != 1) return fail(h, NNLM_ERR_ARG, "%s: side = %d is neither 0 (by columns) nor 1 (by rows)", who, side);
    HIPCHK(h, hipSetDevice(h->device));
    sync_all(h);
    const int lines = side == 0 ? h->m : h->n;
    const size_t nnz = (size_t)h->nnz;
    if (ptr_out) HIPCHK(h, hipMemcpy(ptr_out, side == 0 ? h->sp_cptr : h->sp_rptr, (size_t)(lines + 1) * 8, hipMemcpyDeviceToHost));
    if (idx_out && nnz) HIPCHK(h, hipMemcpy(idx_out, side == 0 ? h->sp_ridx : h->sp_cidx, nnz * 4, hipMemcpyDeviceToHost));
    if (val_out && nnz) return sp_download_values(h, val_out, side == 0 ? h->sp_cval : h->sp_rval);
    return NNLM_OK;
}

extern "C" int nnlm_debug_sparse_resident_weighted(nnlm_handle *h, int side, double *wt_out, double *wa_out)
{
    const char *who = "nnlm_debug_sparse_resident_weighted";
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "%s: handle is NULL", who);
    if (!h->sparse || !h->sp_weighted) return fail(h, NNLM_ERR_ARG, "%s: the handle holds no sparse matrix with per-entry weights", who);
    if (side != 0 && side != 1) return fail(h, NNLM_ERR_ARG, "%s: side = %d is neither 0 (by columns) nor 1 (by rows)", who, side);
    HIPCHK(h, hipSetDevice(h->device));
    sync_all(h);
    int rc = NNLM_OK;
    if (wt_out && h->nnz) rc = sp_download_values(h, wt_out, side == 0 ? h->sp_cwt : h->sp_rwt);
    if (rc == NNLM_OK && wa_out && h->nnz) rc = sp_download_values(h, wa_out, side == 0 ? h->sp_cwa : h->sp_rwa);
    return rc;
}

extern "C" int nnlm_matrix_info(nnlm_handle *h, double *n_non_missing, int *any_missing, double *kl_const)
{
    if (!has_matrix(h)) return fail(h, NNLM_ERR_ARG, "nnlm_matrix_info: no matrix set");
    if (n_non_missing) *n_non_missing = h->n_non_missing;
    if (any_missing) *any_missing = h->any_missing ? 1 : 0;
    if (kl_const) *kl_const = h->kl_const;
    return NNLM_OK;
}

// ---------------------------------------------------------------------------------------------
// factors
// ---------------------------------------------------------------------------------------------
// Launch plan of an A-streaming cross product over `cols` output columns (a multiple of 128) and `stages` contraction stages.
// The kernels run one block per CU (their LDS ring fills the CU), so a launch executes in ceil(blocks / cus) rounds of ceil(stages / S)
// stages each; every block also pays ~3 stage times of pipeline fill/drain, and every slab costs fp64 writes here and fp64 reads in the
// solver that sums the slabs (S = 16 instead of 3 at config 2 made the sweep's start-up 0.06 ms longer -- measured).
// The split-fp16 kernel (k_xprod16.h) has two block widths, 8 or 10 wavefronts = 128 or 160 columns: where 128-column tiles times an
// integer slab count leave CUs idle (config 2, H half-step: 79 x 3 = 237 blocks of 256; W half-step: 158 x 3 = 474, two rounds), 160-column
// tiles can fill them (64 x 4 = 256 and 127 x 2 = 254).  A 160-column stage moves more bytes through the CU than a 128-column one, so a
// stage is priced by its bytes, relative to the 128-column stage: A bytes + XPLAN_Y_WEIGHT x factor bytes (L2 hits).  Pick the cheapest
// (wavefronts, S <= 16); ties go to 8 wavefronts and to the smaller S.  With 8 wavefronts the relative price is 1 and the choice of S is
// the one this function made before it knew of a second width.
// Measured (scripts/exp/xprod_exp.hip -DXPROD_BLOCKS, profiles/xprod_blocks_ab.harness.md): 16 against 13 factor pieces per stage change the
// time of config 2's launches by 0.6 - 0.8 %, which makes a factor byte worth 0.06 - 0.09 of a byte of A; with 0.08 the model puts the
// 160-column form at 0.94 (H) and 0.90 (W) of the 128-column one, measured 0.98 and 0.91.
#define XPLAN_Y_WEIGHT 0.08  // a factor byte (L2 hit) against a byte of A (HBM)
#define XPLAN_SLAB_COST 0.75 // a slab, in 128-column stage times (as before: the sweep's longer start-up, see above)
// Factor pieces (4 rows each) a stage of xprod16_tn_kernel loads at rank k: all 4 NKQ, except at k = 49 .. 52, where the 13 that can be
// non-zero are what lets the 160-column ring fit (one trimmed instantiation, used by both widths; trimming alone gains < 1 %)
static int xprod16_pieces(int k) { return (k > 48 && k <= 52) ? 13 : 4 * (k < 1 ? 1 : k > NNLM_KQ_MAX ? 4 : (k + 15) / 16); }
struct XPlan {
    int nwv, S, sps, tiles_x, yp, lds;
};
// force_waves: 0 = both widths where allowed
static XPlan xprod_plan(int cols, int stages, int k, int cus, int force_waves, bool allow10)
{
    if (cus < 1) cus = 1;
    if (stages < 1) stages = 1;
    const int smax = 16;
    const int nkq = k < 1 ? 1 : k > NNLM_KQ_MAX ? 4 : (k + 15) / 16; // (rank > 64: launches of 64 rows each, all pieces)
    const int yp = xprod16_pieces(k);
    const bool can10 = allow10 && k >= 1 && k <= NNLM_KQ_MAX && xprod16_lds_bytes(10, nkq, yp) <= 160 * 1024;
    const double stage8 = 8 * 4096 + XPLAN_Y_WEIGHT * yp * 1024, stage10 = 10 * 4096 + XPLAN_Y_WEIGHT * yp * 1024;
    int best_s = 1, best_w = 8;
    double best_cost = 1e300;
    for (int w = 8; w <= 10; w += 2) {
        if (w == 10 && (!can10 || force_waves == 8)) continue;
        if (w == 8 && force_waves == 10 && can10) continue;
        const int tiles = (cols + 16 * w - 1) / (16 * w);
        const double rel = w == 8 ? 1.0 : stage10 / stage8;
        for (int s = 1; s <= smax; s++) {
            if (s > 1 && stages / s < 8) break;
            const long blocks = (long)tiles * s;
            const long rounds = (blocks + cus - 1) / cus;
            const int per_block = (stages + s - 1) / s;
            const double cost = (double)rounds * (per_block + 3) * rel + XPLAN_SLAB_COST * s;
            if (cost < best_cost - 1e-9) {
                best_cost = cost;
                best_s = s;
                best_w = w;
            }
        }
    }
    XPlan r;
    int per = (stages + best_s - 1) / best_s;
    if (per < 1) per = 1;
    r.S = (stages + per - 1) / per;
    if (r.S < 1) r.S = 1;
    r.sps = per;
    r.nwv = best_w;
    r.tiles_x = (cols + 16 * best_w - 1) / (16 * best_w);
    r.yp = yp;
    r.lds = xprod16_lds_bytes(best_w, nkq, yp);
    return r;
}

struct HalfPlan {
    int stage_begin, stage_end, S, sps, tiles_x;
    int nwv = XPROD_WAVES; // wavefronts per block: 16 nwv columns per tile (10: xprod16_tn_kernel only)
    int cols = 0;          // columns the launch covers, from col_off on (a multiple of 128)
    int col_off = 0; // first column of the factor being solved that this launch covers (column shards of the multi-GPU NA path)
};

// What the orientation of half-step `which` decides.  which = 1: the H half-step, contraction over the rows i of A (A as stored), W
// fixed; which = 0: the W half-step, contraction over the columns j -- the same "TN" kernels on the transposed copy of A (A16T in the
// split-fp16 mode, AT otherwise), made once per matrix; the reference transposes A in EVERY iteration, src/nnmf.cpp:131.  H fixed.
// The view holds no pointer that changes inside a half-step: AT is made on first use (a_contig) and the W buffers flip in swap_w.
struct Side {
    int which;
    const double *Y;          // master of the fixed factor [KP][ldy]
    int ldy, p;               // contraction length: padded (= ld of the fixed factor) and true
    int ncols, ldc;           // columns solved: true and padded (= ld of the solved factor and of the Cx slabs)
    size_t slab_stride;       // KP * ldc
    const double *X;          // master of the factor solved
    double *Xout;             // where the half-step writes it: H in place, W into the alternate buffer W64b[wcur ^ 1]
    void *op;                 // GEMM-operand copy written next to it (SweepArgs::op): W only
    int op_mode, op_ld;
    const unsigned long long *mask;
    const uint32_t *bits;     // missing-value bits of each solved column over the contraction (miss / missT), NULL without missing values
    int words;                // 32-bit words of `bits` per column
    const uint32_t *A16;      // split-fp16 copy of A, contraction contiguous (A16 / A16T)
    const long long *sp_ptr;  // sparse A: CSC (H half-step) or CSR (W half-step)
    const int *sp_idx;
    const void *sp_val;
    const void *sp_wt, *sp_wa; // weighted handle: the weights and the products c a in the orientation's order (else NULL)
    int prof_xprod, prof_sweep, prof_spmm;
};

static Side side_of(const nnlm_handle *h, int which)
{
    Side s;
    s.which = which;
    if (which == 1) {
        s.Y = h->W64; s.ldy = h->npad; s.p = h->n;
        s.ncols = h->m; s.ldc = h->mpad;
        s.X = s.Xout = h->H64;
        s.op = nullptr; s.op_mode = 0; s.op_ld = 0; // (H has no GEMM-operand copy: every consumer reads the master or makes its own split / fp32 copy)
        s.mask = h->has_hmask ? h->Hmask : nullptr;
        s.bits = h->miss;
        s.A16 = h->A16;
        s.sp_ptr = h->sp_cptr; s.sp_idx = h->sp_ridx; s.sp_val = h->sp_cval;
        s.sp_wt = h->sp_cwt; s.sp_wa = h->sp_cwa;
        s.prof_xprod = P_XPROD_H; s.prof_sweep = P_SWEEP_H; s.prof_spmm = P_SPMM_H;
    } else {
        s.Y = h->H64; s.ldy = h->mpad; s.p = h->m;
        s.ncols = h->n; s.ldc = h->npad;
        s.X = h->W64; s.Xout = h->W64b[h->wcur ^ 1];
        s.op = h->Wopb[h->wcur ^ 1]; s.op_mode = (h->prec == NNLM_PREC_F64) ? 0 : 1; s.op_ld = h->npad;
        s.mask = h->has_wmask ? h->Wmask : nullptr;
        s.bits = h->missT;
        s.A16 = h->A16T;
        s.sp_ptr = h->sp_rptr; s.sp_idx = h->sp_cidx; s.sp_val = h->sp_rval;
        s.sp_wt = h->sp_rwt; s.sp_wa = h->sp_rwa;
        s.prof_xprod = h->fuse_err ? P_XPROD_W_ERR : P_XPROD_W; s.prof_sweep = P_SWEEP_W; s.prof_spmm = P_SPMM_W;
    }
    if (!h->any_missing) s.bits = nullptr;
    s.words = s.ldy / 32;
    s.slab_stride = (size_t)h->KP * s.ldc;
    return s;
}

// A with the contraction contiguous, [ncols][ldy] in the mode's element type (the W half-step's copy AT: ensure_AT first)
static const void *a_contig(const nnlm_handle *h, const Side &s) { return s.which == 1 ? h->A : h->AT; }

// The sweep counter a half-step adds to: the active one, or the alternate one of a speculative half-step (accepted by sw_active ^= 1)
static unsigned long long *sweep_counter(nnlm_handle *h, bool speculative) { return h->sweeps + (speculative ? h->sw_active ^ 1 : h->sw_active); }

// The sweep of side s at rank h->k over all its columns, from the Gram h->Graw and one slab of h->Cx; callers change what differs
static SweepArgs sweep_args(const nnlm_handle *h, const Side &s, const double reg[3], unsigned inner_max_iter, double inner_rel_tol,
                            unsigned long long *sweeps)
{
    SweepArgs a;
    a.X = s.X;
    a.Xout = s.Xout;
    a.ldx = a.ldo = a.ldc = s.ldc;
    a.ocol0 = a.col0 = 0;
    a.Graw = h->Graw;
    a.KPg = h->KP;
    a.Cx = h->Cx;
    a.slab_stride = s.slab_stride;
    a.nslabs = 1;
    a.ncols = s.ncols;
    a.k = h->k;
    a.r0 = reg[0], a.r1 = reg[1], a.r2 = reg[2];
    a.mask = s.mask;
    a.max_iter = inner_max_iter;
    a.rel_tol = inner_rel_tol;
    a.op = s.op;
    a.op_mode = s.op_mode;
    a.op_ld = s.op_ld;
    a.op_f64 = (h->prec == NNLM_PREC_F64) ? 1 : 0;
    a.sweeps = sweeps;
    return a;
}

// contraction elements one stage of a cross product covers (the granularity of the multi-GPU split): 256 bytes of A in the mode's type
// (the split-fp16 kernels' stages of 64 elements are the same in the fp32-operand mode, the only mode that has them)
static int stage_elems(const nnlm_handle *h) { return XPROD_ROWB / (int)esize(h); }

// The kernel a dense half-step of side `which` launches decides which widths the plan may use: only xprod16_tn_kernel has the 160-column
// form -- the fused cross product / error kernel of a trace iteration and the strict kernels keep 128 columns.
// fused: the launch is the fused kernel's (callers pass h->fuse_err of the W half-step being planned)
static bool xprod_wide_ok(const nnlm_handle *h, int which, bool fused) { return h->x16 && !h->sparse && h->k >= 1 && h->k <= NNLM_KQ_MAX && !(which == 0 && fused); }

// plan of `cols` columns from p.col_off on over the stages [p.stage_begin, p.stage_end)
static void plan_cols(const nnlm_handle *h, int which, int cols, HalfPlan &p, bool fused)
{
    int len = p.stage_end - p.stage_begin;
    if (len < 1) len = 1;
    // xprod16_tn_kernel is planned for the handle's CU count (the test hook's, if set); the fused and the strict kernels for the device's
    // own, as before: the strict mode's results do not depend on nnlm_debug_set_cus (the sweep forms it selects are bit-identical)
    const bool tn16 = h->x16 && !h->sparse && !(which == 0 && fused);
    const int cus = (tn16 || h->cus_device < 1) ? h->cus : h->cus_device;
    const XPlan x = xprod_plan(cols, len, h->k, cus, h->xprod_waves, xprod_wide_ok(h, which, fused));
    p.S = x.S, p.sps = x.sps, p.tiles_x = x.tiles_x, p.nwv = x.nwv, p.cols = cols;
}

static HalfPlan plan_half(const nnlm_handle *h, int which, int rank, int nranks, bool fused)
{
    const Side s = side_of(h, which);
    HalfPlan p;
    const int stages_total = s.ldy / stage_elems(h);
    // this rank's slab of the contraction
    const int per_rank = (stages_total + nranks - 1) / nranks;
    p.stage_begin = rank * per_rank;
    p.stage_end = p.stage_begin + per_rank;
    if (p.stage_end > stages_total) p.stage_end = stages_total;
    if (p.stage_begin > stages_total) p.stage_begin = stages_total;
    plan_cols(h, which, s.ldc, p, fused);
    return p;
}

static void pack_mask_cols(const int *mask, int k, int ncols, bool transposed_input, int ld_in, std::vector<unsigned long long> &out, int npadded,
                           int mw)
{
    // transposed_input: mask is ncols x k column-major (Wm, n x k); else k x ncols column-major (Hm); mw words per column
    out.assign((size_t)npadded * mw, 0ull);
    for (int c = 0; c < ncols; c++)
        for (int q = 0; q < k; q++) {
            const int v = transposed_input ? mask[(size_t)q * ld_in + c] : mask[(size_t)c * ld_in + q];
            if (v != 0) out[(size_t)c * mw + (q >> 6)] |= (1ull << (q & 63));
        }
}

// Setting factors in three parts, shared by the host route (set_factors_impl) and the device route (nnlm_set_factors_device):
// factors_alloc -- cache invalidation, buffers and workspaces of rank k; a fill of W64 / H64 / Wop; factors_masks.
// row_pad: zero rows behind the KP rows of the masters W64b / H64 (a batched factorisation reads up to 63 rows past a member's last)
static int factors_alloc(nnlm_handle *h, int k, int row_pad)
{
    HIPCHK(h, hipSetDevice(h->device));
    sync_all(h);
    invalidate_factor_caches(h);
    free_batch(h);
    HIPCHK(h, hipMemset(h->maxbits + 8, 0, sizeof(unsigned)));
    if (k != h->k || row_pad != h->row_pad) {
        free_factors(h);
        h->k = k;
        h->row_pad = row_pad;
        h->NKQ = (k + 15) / 16; // > 4 beyond rank 64: the generic kernels of k_generic.h take over
        h->KP = 16 * h->NKQ;
        h->KP8 = round_up_i(k, 8);
        h->MW = (k + 63) / 64;
        const size_t es = esize(h);
        for (int i = 0; i < 2; i++) {
            HIPCHK(h, hipMalloc(&h->W64b[i], (size_t)(h->KP + row_pad) * h->npad * 8));
            HIPCHK(h, hipMemset(h->W64b[i], 0, (size_t)(h->KP + row_pad) * h->npad * 8));
            if (h->prec == NNLM_PREC_F64) h->Wopb[i] = h->W64b[i];
            else {
                HIPCHK(h, hipMalloc(&h->Wopb[i], (size_t)h->KP * h->npad * es));
                HIPCHK(h, hipMemset(h->Wopb[i], 0, (size_t)h->KP * h->npad * es));
            }
        }
        HIPCHK(h, hipMalloc(&h->H64, (size_t)(h->KP + row_pad) * h->mpad * 8));
        if (row_pad) HIPCHK(h, hipMemset(h->H64 + (size_t)h->KP * h->mpad, 0, (size_t)row_pad * h->mpad * 8));
        if (h->prec == NNLM_PREC_F32) HIPCHK(h, hipMalloc(&h->Hkq, (size_t)h->KP * h->mpad * sizeof(float)));
        HIPCHK(h, hipMalloc(&h->Wmask, (size_t)h->npad * h->MW * 8));
        HIPCHK(h, hipMalloc(&h->Hmask, (size_t)h->mpad * h->MW * 8));
        // split-K slabs: sized for the worst case over ranks (nranks = 1 gives the largest S)
        // (the W half-step has two plans: with and without the fused error kernel, which keeps 128-column blocks)
        const HalfPlan ph = plan_half(h, 1, 0, 1, false), pw = plan_half(h, 0, 0, 1, false), pw2 = plan_half(h, 0, 0, 1, true);
        size_t eh = (size_t)ph.S * h->KP * h->mpad, ew = (size_t)(pw.S > pw2.S ? pw.S : pw2.S) * h->KP * h->npad;
        if (h->x16) {
            HIPCHK(h, hipMalloc(&h->Y16, (size_t)h->KP * (h->npad > h->mpad ? h->npad : h->mpad) * 4 + 4096));
            HIPCHK(h, hipMalloc(&h->W16c, (size_t)h->npad * 64 * 4 + 4096));
            HIPCHK(h, hipMalloc(&h->H16c, (size_t)h->mpad * 64 * 4 + 4096));
        }
        h->Cx_elems = eh > ew ? eh : ew;
        const size_t big = (size_t)(h->npad > h->mpad ? h->npad : h->mpad);
        if (h->sparse) h->Cx_elems = (size_t)h->KP * big; // (one slab: the SpMM has no split-K)
        HIPCHK(h, hipMalloc(&h->Cx, h->Cx_elems * 8));
        HIPCHK(h, hipMemset(h->Cx, 0, h->Cx_elems * 8)); // rows >= k of a slab are never written: keep them finite
        const int gb = (h->npad > h->mpad ? h->npad : h->mpad) / GRAM_COLS_PER_BLOCK + 1;
        HIPCHK(h, hipMalloc(&h->gslabs, (size_t)gb * h->KP * h->KP * 8));
        // (a sparse handle uses the head only: Graw; the [G | C] buffer of the multi-GPU all-reduce is dense-only)
        HIPCHK(h, hipMalloc(&h->red, ((size_t)h->KP * h->KP + (h->sparse ? 0 : (size_t)h->KP * big)) * 8));
        h->Graw = h->red;
        if (h->sparse) { // row copy of the fixed factor, SpMM carries, error block workspaces (k_sparse.h)
            const int KP = h->KP;
            HIPCHK(h, hipMalloc(&h->sp_Y, big * KP * es + 4096));
            HIPCHK(h, hipMalloc(&h->sp_carry, (size_t)nnlm_sp_workers(h->nnz, KP, h->cus_device) * 64 * 8));
            HIPCHK(h, hipMalloc(&h->sp_Wrow, (size_t)h->npad * KP * 8));
            HIPCHK(h, hipMalloc(&h->sp_eslabs, (size_t)gb * KP * KP * 8));
            HIPCHK(h, hipMalloc(&h->sp_eG, ((size_t)2 * KP * KP + 2 * KP + 8) * 8));
            const size_t eb = (size_t)(nnlm_sp_workers(h->nnz, KP, h->cus_device) / (64 / nnlm_sp_lanes(KP)) + 3) / 4;
            const size_t rb = (big + 2047) / 2048;
            HIPCHK(h, hipMalloc(&h->sp_epart, (5 * eb > KP * rb ? 5 * eb : KP * rb) * 8 + 64)); // (five per workgroup: the weighted error block)
        }
    }
    h->wcur = 0;
    h->W64 = h->W64b[0];
    h->Wop = h->Wopb[0];
    h->sg_which = h->sg_other = -1;
    h->sw_active = 0;
    HIPCHK(h, hipMemset(h->sweeps, 0, 2 * sizeof(unsigned long long)));
    return NNLM_OK;
}

static int factors_masks(nnlm_handle *h, int k, const int *Wm, const int *Hm)
{
    const int n = h->n, m = h->m, npad = h->npad, mpad = h->mpad;
    std::vector<unsigned long long> mk;
    h->has_wmask = Wm != nullptr;
    h->has_hmask = Hm != nullptr;
    if (Wm) {
        pack_mask_cols(Wm, k, n, true, n, mk, npad, h->MW);
        HIPCHK(h, hipMemcpy(h->Wmask, mk.data(), (size_t)npad * h->MW * 8, hipMemcpyHostToDevice));
    }
    if (Hm) {
        pack_mask_cols(Hm, k, m, false, k, mk, mpad, h->MW);
        HIPCHK(h, hipMemcpy(h->Hmask, mk.data(), (size_t)mpad * h->MW * 8, hipMemcpyHostToDevice));
    }
    return NNLM_OK;
}

static int set_factors_impl(nnlm_handle *h, int k, const double *W, const double *H, const int *Wm, const int *Hm, int row_pad)
{
    if (const int rc = factors_alloc(h, k, row_pad)) return rc;
    const int KP = h->KP, n = h->n, m = h->m, npad = h->npad, mpad = h->mpad;
    // host-side repack into the padded resident layouts (k*(n+m) elements: negligible)
    std::vector<double> w64((size_t)KP * npad, 0.0), h64((size_t)KP * mpad, 0.0);
    if (W)
        for (int q = 0; q < k; q++)
            for (int i = 0; i < n; i++) w64[(size_t)q * npad + i] = W[(size_t)q * n + i]; // W is n x k column-major
    if (H)
        for (int j = 0; j < m; j++)
            for (int q = 0; q < k; q++) h64[(size_t)q * mpad + j] = H[(size_t)j * k + q]; // H is k x m column-major
    HIPCHK(h, hipMemcpy(h->W64, w64.data(), w64.size() * 8, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(h->H64, h64.data(), h64.size() * 8, hipMemcpyHostToDevice));
    if (h->prec != NNLM_PREC_F64) {
        std::vector<float> wop((size_t)KP * npad);
        for (size_t e = 0; e < wop.size(); e++) wop[e] = (float)w64[e];
        HIPCHK(h, hipMemcpy(h->Wop, wop.data(), wop.size() * 4, hipMemcpyHostToDevice));
    }
    return factors_masks(h, k, Wm, Hm);
}

extern "C" int nnlm_set_factors(nnlm_handle *h, unsigned k_, const double *W, const double *H, const int *Wm, const int *Hm)
{
    if (!has_matrix(h)) return fail(h, NNLM_ERR_ARG, "nnlm_set_factors: set the matrix first");
    const int k = (int)k_;
    if (k < 1) return fail(h, NNLM_ERR_ARG, "nnlm_set_factors: rank k must be >= 1");
    if (h->sparse && h->sp_weighted && k > NNLM_KQ_MAX) return weighted_refusal(h, "nnlm_set_factors", "a rank above 64");
    if (h->sparse && h->sp_missing && k > NNLM_KQ_MAX)
        return fail(h, NNLM_ERR_UNSUPPORTED, "nnlm_set_factors: rank %d on a sparse matrix whose absent entries are missing: the rank is at most %d", k,
                    NNLM_KQ_MAX);
    return set_factors_impl(h, k, W, H, Wm, Hm, 0);
}

extern "C" int nnlm_get_factors(nnlm_handle *h, double *W, double *H)
{
    if (!h || !h->W64) return fail(h, NNLM_ERR_ARG, "nnlm_get_factors: no factors set");
    HIPCHK(h, hipSetDevice(h->device));
    sync_all(h);
    const int k = h->k, n = h->n, m = h->m, npad = h->npad, mpad = h->mpad;
    if (W) {
        std::vector<double> w64((size_t)h->KP * npad);
        HIPCHK(h, hipMemcpy(w64.data(), h->W64, w64.size() * 8, hipMemcpyDeviceToHost));
        for (int q = 0; q < k; q++) memcpy(W + (size_t)q * n, &w64[(size_t)q * npad], (size_t)n * 8);
    }
    if (H) {
        std::vector<double> h64((size_t)h->KP * mpad);
        HIPCHK(h, hipMemcpy(h64.data(), h->H64, h64.size() * 8, hipMemcpyDeviceToHost));
        for (int j = 0; j < m; j++)
            for (int q = 0; q < k; q++) H[(size_t)j * k + q] = h64[(size_t)q * mpad + j];
    }
    return NNLM_OK;
}

// Factors from device memory: W n x k, H k x m in the caller's type and strides (NULL = zeros); masks are host arrays.
extern "C" int nnlm_set_factors_device(nnlm_handle *h, unsigned k_, const nnlm_dev_matrix *W, const nnlm_dev_matrix *H, const int *Wm, const int *Hm,
                                       void *stream)
{
    const char *who = "nnlm_set_factors_device";
    if (!has_matrix(h)) return fail(h, NNLM_ERR_ARG, "%s: set the matrix first", who);
    const int k = (int)k_;
    if (k < 1) return fail(h, NNLM_ERR_ARG, "%s: rank k must be >= 1", who);
    if (h->sparse && h->sp_weighted && k > NNLM_KQ_MAX) return weighted_refusal(h, who, "a rank above 64");
    if (h->sparse && h->sp_missing && k > NNLM_KQ_MAX)
        return fail(h, NNLM_ERR_UNSUPPORTED, "%s: rank %d on a sparse matrix whose absent entries are missing: the rank is at most %d", who, k, NNLM_KQ_MAX);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = NNLM_OK;
    if (W && (rc = dev_matrix_check(h, who, "W", W, h->n, k, false)) != NNLM_OK) return rc;
    if (H && (rc = dev_matrix_check(h, who, "H", H, k, h->m, false)) != NNLM_OK) return rc;
    if ((rc = factors_alloc(h, k, 0)) != NNLM_OK) return rc;
    if ((rc = stream_after(h, h->stream, (hipStream_t)stream)) != NNLM_OK) return rc; // the caller's stream produced W and H
    float *wop = h->prec == NNLM_PREC_F64 ? nullptr : (float *)h->Wop;
    dim3 gw(h->npad / 256, h->KP), gh((h->mpad + 255) / 256, h->KP);
    // W n x k: (c = i, q) at ptr[i row_stride + q col_stride]; H k x m: (c = j, q) at ptr[q row_stride + j col_stride]
    with_dtype(W ? W->dtype : NNLM_DT_F64, [&](auto s) {
        typedef decltype(s) S;
        factor_ingest_kernel<S><<<gw, 256, 0, h->stream>>>(W ? (const S *)W->ptr : nullptr, W ? W->row_stride : 0, W ? W->col_stride : 0, h->n, k, h->W64, wop, h->npad);
        return 0;
    });
    with_dtype(H ? H->dtype : NNLM_DT_F64, [&](auto s) {
        typedef decltype(s) S;
        factor_ingest_kernel<S><<<gh, 256, 0, h->stream>>>(H ? (const S *)H->ptr : nullptr, H ? H->col_stride : 0, H ? H->row_stride : 0, h->m, k, h->H64, nullptr, h->mpad);
        return 0;
    });
    LAUNCHCHK(h);
    HIPCHK(h, hipStreamSynchronize(h->stream)); // (where nnlm_set_factors' copies wait: the caller's buffers are free again on return)
    return factors_masks(h, k, Wm, Hm);
}

// The current factors into the caller's device buffers (F64 or F32, any non-overlapping strides; NULL = not wanted).  No host wait: the
// export runs on the handle's stream behind the caller's earlier work, and the caller's stream continues behind the export.
extern "C" int nnlm_get_factors_device(nnlm_handle *h, const nnlm_dev_matrix *W, const nnlm_dev_matrix *H, void *stream)
{
    const char *who = "nnlm_get_factors_device";
    if (!h || !h->W64) return fail(h, NNLM_ERR_ARG, "%s: no factors set", who);
    HIPCHK(h, hipSetDevice(h->device));
    int rc = NNLM_OK;
    if (W && (rc = dev_matrix_check(h, who, "W", W, h->n, h->k, true)) != NNLM_OK) return rc;
    if (H && (rc = dev_matrix_check(h, who, "H", H, h->k, h->m, true)) != NNLM_OK) return rc;
    if ((rc = stream_after(h, h->stream, h->stream_e)) != NNLM_OK) return rc;
    if ((rc = stream_after(h, h->stream, (hipStream_t)stream)) != NNLM_OK) return rc; // the caller's earlier use of the buffers
    if (W) {
        dim3 g((h->n + 255) / 256, h->k);
        if (W->dtype == NNLM_DT_F64) factor_export_kernel<double><<<g, 256, 0, h->stream>>>(h->W64, h->npad, h->n, (double *)W->ptr, W->row_stride, W->col_stride);
        else factor_export_kernel<float><<<g, 256, 0, h->stream>>>(h->W64, h->npad, h->n, (float *)W->ptr, W->row_stride, W->col_stride);
    }
    if (H) {
        dim3 g((h->m + 255) / 256, h->k);
        if (H->dtype == NNLM_DT_F64) factor_export_kernel<double><<<g, 256, 0, h->stream>>>(h->H64, h->mpad, h->m, (double *)H->ptr, H->col_stride, H->row_stride);
        else factor_export_kernel<float><<<g, 256, 0, h->stream>>>(h->H64, h->mpad, h->m, (float *)H->ptr, H->col_stride, H->row_stride);
    }
    LAUNCHCHK(h);
    return stream_after(h, (hipStream_t)stream, h->stream);
}

// nnlm_get_info "matrix_min_col_observed" / "matrix_min_row_observed": on first query, cached with the matrix
static int observed_min(nnlm_handle *h, int which, double *value)
{
    if (h->sparse && h->min_obs[0] >= 0) { // (nnlm_set_matrix_sparse_device counted them from its host copies of the pointers)
        *value = h->min_obs[which];
        return NNLM_OK;
    }
    if (h->sparse || !h->A) {
        *value = -1.0;
        return NNLM_OK;
    }
    if (h->min_obs[0] == -2) {
        if (!h->any_missing) h->min_obs[0] = h->n, h->min_obs[1] = h->m;
        else {
            HIPCHK(h, hipSetDevice(h->device));
            int *out = nullptr, init[2] = {INT_MAX, INT_MAX}, res[2] = {0, 0};
            HIPCHK(h, hipMalloc(&out, sizeof init));
            hipError_t e = hipMemcpyAsync(out, init, sizeof init, hipMemcpyHostToDevice, h->stream);
            observed_min_kernel<<<(h->m + 3) / 4, 256, 0, h->stream>>>(h->miss, h->m, h->npad / 32, h->n, out);
            observed_min_kernel<<<(h->n + 3) / 4, 256, 0, h->stream>>>(h->missT, h->n, h->mpad / 32, h->m, out + 1);
            if (e == hipSuccess) e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(res, out, sizeof res, hipMemcpyDeviceToHost, h->stream);
            const hipError_t e2 = hipStreamSynchronize(h->stream);
            hipFree(out);
            if (e != hipSuccess || e2 != hipSuccess) return fail(h, NNLM_ERR_HIP, "observed_min_kernel failed: %s", hipGetErrorString(e != hipSuccess ? e : e2));
            h->min_obs[0] = res[0], h->min_obs[1] = res[1];
        }
    }
    *value = h->min_obs[which];
    return NNLM_OK;
}

// ---------------------------------------------------------------------------------------------
// half-step
// ---------------------------------------------------------------------------------------------
// Calls f(std::integral_constant<int, N>{}) for the number N of 16-row blocks of a factor a kernel instantiation covers: nkq = 1, 2, 3
// as they are; anything >= 4 -> 4 (rank <= 64, or one 64-row slice of the rank > 64 loops)
template <typename F>
static void with_nkq(int nkq, F &&f)
{
    switch (nkq) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
    }
}

// Cache policy of the stream of A in the three A-streaming cross products (xprod16_tn_kernel, xprod16_err_kernel, xprod_tn_kernel): the
// requests of the contraction stages >= this one are non-temporal (glds16_s_nt, k_xprod.h) -- 0: all of A, INT_MAX: none, R in between:
// the first 64 R contraction elements of every column keep the default policy.  Measured at config 2 (DESIGN.md section 4.1,
// profiles/a_stream_policy_ab.md).  A kernel class keeps the policy only where its own launches were measurably shorter with it; the
// others are launched with INT_MAX: the fused kernel (bound by its error wavefronts, not by the stream) and the strict kernel (bound by
// the fp64 matrix pipe) gained nothing.  A pass whose bytes, together with the other half-step's pass over the other copy, fit the 256 MB
// Infinity Cache finds them there in the next iteration and keeps the default policy too (4000 x 2000: 2 % slower non-temporally; 8000 x
// 4000, 2 x 131 MB, no longer).  nnlm_debug_set_a_stream overrides all of it per handle.
static constexpr int A_STREAM_NT_FROM = 16;
static constexpr size_t A_STREAM_MIN_PASS_BYTES = (size_t)128 << 20;
enum AStreamClass { A_STREAM_PLAIN = 0, A_STREAM_FUSED = 1, A_STREAM_STRICT = 2 }; // xprod16_tn_kernel, xprod16_err_kernel, xprod_tn_kernel
static constexpr bool A_STREAM_CLASS_NT[3] = {true, false, false};
static int a_stream_nt(nnlm_handle *h, AStreamClass c, const HalfPlan &p)
{
    // (a stage is 256 bytes of every column in all three kernels)
    const size_t pass_bytes = (size_t)p.tiles_x * 16 * p.nwv * (size_t)(p.stage_end - p.stage_begin) * XPROD_ROWB;
    const int own = (A_STREAM_CLASS_NT[c] && pass_bytes > A_STREAM_MIN_PASS_BYTES) ? A_STREAM_NT_FROM : INT_MAX;
    return h->a_stream_last = (h->a_stream >= 0 ? h->a_stream : own);
}

// xprod_tn_kernel (k_xprod.h) over rows [0, 16 NKQ (+ KT tail rows)) of the fixed factor Y into the slabs at C (the rank > 64 loops:
// one launch per 64 rows of Y and C)
template <typename T, int NKQ, int KT = 0>
static void launch_xprod_tn(nnlm_handle *h, const T *Amat, int lda, const T *Y, int ldy, double *C, int ldc, size_t slab_stride, const HalfPlan &p)
{
    dim3 grid(p.tiles_x, p.S);
    const int lds = xprod_tn_lds_bytes(16 * (NKQ + (KT > 0 ? 1 : 0)));
    set_dyn_lds((const void *)xprod_tn_kernel<T, NKQ, KT>, lds, "xprod_tn_kernel");
    xprod_tn_kernel<T, NKQ, KT><<<grid, XPROD_THREADS, lds, h->stream>>>(Amat + (size_t)p.col_off * lda, lda, Y, ldy, C + p.col_off, ldc, slab_stride,
                                                                          p.stage_begin, p.stage_end, p.sps, a_stream_nt(h, A_STREAM_STRICT, p));
}

// Strict mode, rank <= 64 (the masters are the operands: Wop aliases W64).  MFMA tiles / VALU tail rows for rank k: k = 16*NKQ + rem;
// a remainder of 1..4 rows (with at least one full tile) is not padded to a whole 16-wide MFMA tile but handled as 2 or 4 tail rows (k_xprod.h).
static void launch_xprod_nkq(nnlm_handle *h, const Side &s, const HalfPlan &p)
{
    const double *Amat = (const double *)a_contig(h, s);
    auto go = [&](auto nkq, auto kt) { launch_xprod_tn<double, nkq, kt>(h, Amat, s.ldy, s.Y, s.ldy, h->Cx, s.ldc, s.slab_stride, p); };
    const int full = h->k / 16, rem = h->k % 16;
    if (full >= 1 && rem >= 1 && rem <= 4)
        with_nkq(full, [&](auto N) {
            constexpr int F = N < 4 ? N : 3; // (full <= 3: k <= 64)
            if (rem <= 2) go(std::integral_constant<int, F>{}, std::integral_constant<int, 2>{});
            else go(std::integral_constant<int, F>{}, std::integral_constant<int, 4>{});
        });
    else
        with_nkq(h->NKQ, [&](auto N) { go(N, std::integral_constant<int, 0>{}); });
}

// Split-fp16 cross product (k_xprod16.h): split copy of the fixed factor scaled by its own power of two, then the
// A-streaming kernel on A16 (H half-step) or A16T (W half-step: the transposed copy makes it the same "TN" kernel).
// q0: first of the 16 NKQ rows of the split copy and of the slabs this launch covers (rank > 64: one launch per 64 rows)
template <int NKQ, int NWV, int YP>
static void launch_xprod16_nwy(nnlm_handle *h, const Side &s, const HalfPlan &p, int q0)
{
    dim3 grid(p.tiles_x, p.S);
    const int lds = xprod16_lds_bytes(NWV, NKQ, YP);
    set_dyn_lds((const void *)xprod16_tn_kernel<NKQ, NWV, YP>, lds, "xprod16_tn_kernel");
    xprod16_tn_kernel<NKQ, NWV, YP><<<grid, 64 * NWV, lds, h->stream>>>(s.A16 + (size_t)p.col_off * s.ldy, s.ldy, h->Y16 + (size_t)q0 * s.ldy, s.ldy,
                                                                        h->Cx + (size_t)q0 * s.ldc + p.col_off, s.ldc, p.cols, s.slab_stride,
                                                                        p.stage_begin, p.stage_end, p.sps, h->scal_exp, a_stream_nt(h, A_STREAM_PLAIN, p));
}
// The instantiations: all 4 NKQ factor pieces in both widths for NKQ <= 3; NKQ = 4 with all 16 pieces (8 wavefronts only: the 160-column
// ring does not fit) and with the 13 pieces of k = 49 .. 52 in both widths (rows >= k of the split copy are zero: factor16_kernel).
template <int NKQ>
static void launch_xprod16_m(nnlm_handle *h, const Side &s, const HalfPlan &p, int q0 = 0)
{
    const bool trim = NKQ == 4 && xprod16_pieces(h->k - q0) == 13;
    if constexpr (NKQ == 4) {
        if (p.nwv == 10 && !trim) { // (xprod_plan admits 10 wavefronts only where the ring fits: not reached)
            g_attr_err = hipErrorInvalidValue, g_attr_what = "xprod16_tn_kernel: 160-column blocks at a rank whose ring does not fit";
            return;
        }
        if (trim && p.nwv == 10) launch_xprod16_nwy<4, 10, 13>(h, s, p, q0);
        else if (trim) launch_xprod16_nwy<4, 8, 13>(h, s, p, q0);
        else launch_xprod16_nwy<4, 8, 16>(h, s, p, q0);
    } else {
        if (p.nwv == 10) launch_xprod16_nwy<NKQ, 10, 4 * NKQ>(h, s, p, q0);
        else launch_xprod16_nwy<NKQ, 8, 4 * NKQ>(h, s, p, q0);
    }
    h->xp_waves[s.which] = p.nwv, h->xp_splits[s.which] = p.S;
}
// split copy of the fixed factor, scaled by its own power of two (two small kernels, outside the cross product's timing
// scope).  Measured: making these faster (2-D absmax grid, no memset) or moving sweep_consts_kernel to the Gram stream
// made the step SLOWER by 1 % -- the Gram kernels then overlap more of the (now HBM-bound) cross product.
// mb: device word that already holds max|factor| (from gram_partial_kernel), or NULL: compute it here
// w_max_in_zero_word: zero_word (about to be cleared for this half-step's sweep) still holds max|W| of the current W, left by
// the sweep that solved it -- the fused error block's split copy of W then needs no absmax pass (24 us) of its own.
static void prepare_factor16(nnlm_handle *h, const Side &s, unsigned *mb = nullptr, unsigned *zero_word = nullptr, bool w_max_in_zero_word = false)
{
    const double *Ym = s.Y;
    const int ldm = s.ldy, plen_true = s.p;
    h->y16_for = -1; // (Y16 is rewritten)
    if (!mb) {
        mb = h->maxbits;
        hipMemsetAsync(mb, 0, sizeof(unsigned), h->stream);
        absmax_f64_kernel<<<(plen_true + 255) / 256, 256, 0, h->stream>>>(Ym, ldm, plen_true, h->k, mb);
    }
    const size_t cnt = (size_t)h->KP * ldm;
    const bool fuse = s.which == 0 && h->fuse_err; // the fused error block also needs H and W with kq contiguous (same exponent for H)
    if (fuse && w_max_in_zero_word && zero_word) // (before factor16_kernel clears that word)
        factor16c_kernel<<<h->npad / 64, 256, 0, h->stream>>>(h->W64, h->npad, h->n, h->k, zero_word, h->scal_exp + 2, h->W16c);
    factor16_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>(Ym, ldm, plen_true, h->k, h->KP, ldm, mb, h->scal_exp + 1, h->Y16, zero_word);
    if (fuse) {
        factor16c_kernel<<<h->mpad / 64, 256, 0, h->stream>>>(h->H64, h->mpad, h->m, h->k, mb, nullptr, h->H16c);
        if (!(w_max_in_zero_word && zero_word)) {
            // (a word of its own: maxbits[0] may be the fixed factor's maximum that the NA flow's row copy reads later, fixed_maxw)
            unsigned *wmb = h->maxbits + 10;
            hipMemsetAsync(wmb, 0, sizeof(unsigned), h->stream);
            absmax_f64_kernel<<<(h->n + 255) / 256, 256, 0, h->stream>>>(h->W64, h->npad, h->n, h->k, wmb);
            factor16c_kernel<<<h->npad / 64, 256, 0, h->stream>>>(h->W64, h->npad, h->n, h->k, wmb, h->scal_exp + 2, h->W16c);
        }
    }
}
template <int NKQ>
static void launch_xprod16_err_m(nnlm_handle *h, const HalfPlan &p)
{
    dim3 grid(p.tiles_x, p.S);
    const int lds = xprod16_err_lds_bytes(NKQ);
    if (h->any_missing) {
        set_dyn_lds((const void *)xprod16_err_kernel<NKQ, true>, lds, "xprod16_err_kernel");
        xprod16_err_kernel<NKQ, true><<<grid, XPROD_THREADS, lds, h->stream>>>(h->A16T, h->mpad, h->Y16, h->mpad, h->H16c, h->W16c, h->Cx, h->npad,
                                                                               (size_t)16 * NKQ * h->npad, p.stage_begin, p.stage_end, p.sps, h->scal_exp,
                                                                               h->scal_exp + 2, h->n, h->m, h->partials, h->err_zero_word, h->missT,
                                                                               h->mpad / 32, p.col_off, a_stream_nt(h, A_STREAM_FUSED, p));
    } else {
        set_dyn_lds((const void *)xprod16_err_kernel<NKQ, false>, lds, "xprod16_err_kernel");
        xprod16_err_kernel<NKQ, false><<<grid, XPROD_THREADS, lds, h->stream>>>(h->A16T, h->mpad, h->Y16, h->mpad, h->H16c, h->W16c, h->Cx, h->npad,
                                                                                (size_t)16 * NKQ * h->npad, p.stage_begin, p.stage_end, p.sps, h->scal_exp,
                                                                                h->scal_exp + 2, h->n, h->m, h->partials, h->err_zero_word, nullptr, 0,
                                                                                p.col_off, a_stream_nt(h, A_STREAM_FUSED, p));
    }
    h->err_zero_word = nullptr;
    h->fused_nb = p.tiles_x * p.S;
    h->xp_err_splits = p.S;
}
static void launch_xprod16(nnlm_handle *h, const Side &s, const HalfPlan &p)
{
    if (s.which == 0 && h->fuse_err) with_nkq(h->NKQ, [&](auto N) { launch_xprod16_err_m<N>(h, p); });
    else with_nkq(h->NKQ, [&](auto N) { launch_xprod16_m<N>(h, s, p); });
}

// ---- rank > 64 (k_generic.h): the same A-streaming kernels, launched once per 64 rows of the fixed factor --------------
static bool generic_rank(const nnlm_handle *h) { return h->k > NNLM_KQ_MAX; }

// contraction-contiguous copy of A ([npad][mpad], element type of the mode), made once per matrix
// soft: a copy that does not fit is reported as NNLM_ERR_UNSUPPORTED without an error message (the KL solvers then take their streaming path)
static int ensure_AT(nnlm_handle *h, bool soft = false)
{
    if (h->AT) return NNLM_OK;
    const size_t bytes = (size_t)h->npad * h->mpad * esize(h) + 4096;
    if (soft) {
        if (big_malloc(&h->AT, bytes) != hipSuccess) return NNLM_ERR_UNSUPPORTED;
    } else
        HIPCHK(h, hipMalloc(&h->AT, bytes));
    dim3 grid(h->npad / 64, h->mpad / 64);
    if (h->prec == NNLM_PREC_F64) transpose_kernel<double><<<grid, 256, 0, h->stream>>>((const double *)h->A, h->npad, (double *)h->AT, h->mpad);
    else transpose_kernel<float><<<grid, 256, 0, h->stream>>>((const float *)h->A, h->npad, (float *)h->AT, h->mpad);
    LAUNCHCHK(h);
    return NNLM_OK;
}

template <typename T>
static int launch_xprod_generic_t(nnlm_handle *h, const Side &s, const HalfPlan &p)
{
    const T *Y = (const T *)h->Wop;
    if (s.which == 0) {
        int rc = ensure_AT(h);
        if (rc != NNLM_OK) return rc;
        if (h->prec == NNLM_PREC_F64) Y = (const T *)h->H64;
        else { // fp32 [KP][mpad] copy of H
            const size_t cnt = (size_t)h->KP * h->mpad;
            factor_to_f32_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>(h->H64, cnt, h->Hkq);
            Y = (const T *)h->Hkq;
        }
    }
    const T *Amat = (const T *)a_contig(h, s);
    for (int q0 = 0; q0 < h->KP; q0 += 64)
        with_nkq((h->KP - q0) / 16, [&](auto N) {
            launch_xprod_tn<T, N>(h, Amat, s.ldy, Y + (size_t)q0 * s.ldy, s.ldy, h->Cx + (size_t)q0 * s.ldc, s.ldc, s.slab_stride, p);
        });
    return NNLM_OK;
}

static int launch_xprod_generic(nnlm_handle *h, const Side &s, const HalfPlan &p)
{
    if (h->x16) { // split-fp16 copies A16 / A16T exist: the split copy of the factor (prepare_factor16) covers all KP rows
        for (int q0 = 0; q0 < h->KP; q0 += 64) with_nkq((h->KP - q0) / 16, [&](auto N) { launch_xprod16_m<N>(h, s, p, q0); });
        return NNLM_OK;
    }
    if (h->prec == NNLM_PREC_F64) return launch_xprod_generic_t<double>(h, s, p);
    return launch_xprod_generic_t<float>(h, s, p);
}

// Gram partial sums of columns [c_begin, c_end) of Y into `slabs`, one per block of GRAM_COLS_PER_BLOCK columns: returns their number.
// mb (optional, rank <= 64): zeroed word that receives the bit pattern of max|Y| over the range (the split-fp16 copy's scale: no absmax pass)
static int launch_gram_partial(const nnlm_handle *h, const double *Y, int ld, int c_begin, int c_end, double *slabs, unsigned *mb, hipStream_t st)
{
    int nb = (c_end - c_begin + GRAM_COLS_PER_BLOCK - 1) / GRAM_COLS_PER_BLOCK;
    if (nb < 1) nb = 1;
    if (generic_rank(h)) {
        dim3 grid(nb, h->NKQ * (h->NKQ + 1) / 2);
        gram_partial_generic_kernel<<<grid, 256, 0, st>>>(Y, ld, c_begin, c_end, h->NKQ, slabs);
    } else
        with_nkq(h->NKQ, [&](auto N) { gram_partial_kernel<N><<<nb, 256, 0, st>>>(Y, ld, c_begin, c_end, slabs, mb); });
    return nb;
}

// Gram of the fixed factor over its columns [c_begin, c_end) into Graw
static void launch_gram(nnlm_handle *h, const Side &s, int c_begin, int c_end, unsigned *mb = nullptr)
{
    const int KP = h->KP;
    const int nb = launch_gram_partial(h, s.Y, s.ldy, c_begin, c_end, h->gslabs, mb, h->stream);
    if (generic_rank(h)) gram_reduce_kernel<<<(KP * KP + 255) / 256, 256, 0, h->stream>>>(h->gslabs, nb, KP, h->Graw);
    else // (16 wavefronts per 64 entries, every 16th slab each: 5 us where the one-thread-per-entry sum over ~80 slabs took 20-25)
        gram_fold_kernel<<<KP * KP / 64, 1024, 0, h->stream>>>(h->gslabs, nb, KP, h->Graw, SweepImg{});
}

template <int R, int L>
static void launch_sweep_m(int method, const SweepArgs &a, hipStream_t s)
{
    const int cpw = 64 / L; // columns per wavefront
    const int nb = (a.ncols + cpw - 1) / cpw;
    (void)method; // Lee's multiplicative updates only: SCD-LS is sweep_scd_q_kernel at every rank <= 64 (launch_sweep)
    sweep_ls_kernel<R, L, 2><<<nb, 64, 0, s>>>(a);
}

// registers per lane R = STEP * idx, idx = 1..8
template <int STEP, int L>
static void launch_sweep_l(int idx, int method, const SweepArgs &a, hipStream_t s)
{
    switch (idx) {
    case 1: launch_sweep_m<1 * STEP, L>(method, a, s); break;
    case 2: launch_sweep_m<2 * STEP, L>(method, a, s); break;
    case 3: launch_sweep_m<3 * STEP, L>(method, a, s); break;
    case 4: launch_sweep_m<4 * STEP, L>(method, a, s); break;
    case 5: launch_sweep_m<5 * STEP, L>(method, a, s); break;
    case 6: launch_sweep_m<6 * STEP, L>(method, a, s); break;
    case 7: launch_sweep_m<7 * STEP, L>(method, a, s); break;
    default: launch_sweep_m<8 * STEP, L>(method, a, s); break;
    }
}

// Lanes per column.  The sweep is bound by the per-wavefront issue rate (fp64 VALU: one instruction per 8 cycles per
// wave, measured), so fewer FMAs per lane (larger L) wins as long as the SIMDs are not oversubscribed: L = 4 up to
// 4 wavefronts per SIMD (measured at config 2: L=4 0.56 ms, L=2 0.85 ms, L=1 1.5 ms per half-step).
static int sweep_lanes_per_column(int ncols)
{
    const long slots = 1024L * 4; // SIMDs x wavefronts per SIMD
    if (((long)ncols * 4 + 63) / 64 <= slots) return 4;
    if (((long)ncols * 2 + 63) / 64 <= slots) return 2;
    return 1;
}

// SCD-LS for ranks up to 64, both modes: sweep_scd_q_kernel (k_sweep_q.h: one wavefront per 16 columns, the whole recurrence on the
// 4x4x4 fp64 matrix instruction).  fp32-operand mode: rows of G divided by their diagonal, one instruction per chain pass; strict
// fp64 mode: the reference's arithmetic (correctly rounded mu / G[q][q]).
static bool sweep_fast(const nnlm_handle *h) { return h->prec == NNLM_PREC_F32 && h->k <= NNLM_KQ_MAX; }

// (the instantiations of sweep_scd_q_kernel / sweep_scd_qw_kernel / sweep_scd_f_kernel -- 64 heavy ones each -- live in translation units of
//  their own, tu_sweepq.hip / tu_sweepqw.hip / tu_sweepf.hip, compiled next to this one: tu_sweepq.h)
// fp32-operand mode: the fp32-chain kernel (k_sweep_f.h).  One wavefront per 16 columns; four per workgroup (one per SIMD) while the
// launch has at most one wavefront per SIMD of the device, eight (two per SIMD, 128 columns per workgroup) beyond -- the instruction
// streams of two wavefronts interleave where a lone one leaves every second issue slot empty.  Reads a.Graw; no operand image.
// Gram partial-sum slabs a sweep launch may leave behind: one per workgroup -- 64 columns (k_sweep_q.h), 64 / 128 (k_sweep_f.h), or 16 / 32 in
// the row form, which is taken for at most one workgroup per CU
static size_t sg_slab_count(const nnlm_handle *h)
{
    const int big = h->n > h->m ? h->n : h->m;
    const int wide = (big + SWEEPQ_COLS - 1) / SWEEPQ_COLS, row = (big + 15) / 16 < h->cus ? (big + 15) / 16 : h->cus;
    return (size_t)(wide > row ? wide : row) + 1;
}
static void launch_sweep_f(nnlm_handle *h, const SweepArgs &a)
{
    const int ncols = a.ncols - a.col0, NB = (a.k + 3) / 4;
    h->sweep_wgs = 0;
    h->pack_ready = false;
    if (ncols <= 0) return;
    // Row form (k_sweep_r.h: four columns per wavefront, no matrix instruction in the chain) while the launch is ONE round of its
    // wavefronts: workgroups of four wavefronts (one per SIMD) up to one workgroup per CU, of eight (two per SIMD) up to 32 columns per CU.
    // Mid-size problems and the column shards of a multi-GPU run; beyond (the benchmark's 10000 / 20000 columns on one GPU) the
    // matrix-pipe kernel below, whose 157 workgroups are one round where the row form's would be two or three.
    if (a.k <= SWEEPR_KMAX && ncols <= 32 * h->cus) {
        const int NWr = (ncols <= 16 * h->cus) ? 4 : 8;
        const int nbr = (ncols + 4 * NWr - 1) / (4 * NWr);
        h->sweep_wgs = nbr;
        h->sweep_form[h->cur_which] = 3;
        h->sweep_groups[h->cur_which] = NWr;
        nnlm_tu_sweep_r(a, nbr, NWr, h->stream);
        return;
    }
    const int ngroups = (ncols + 15) / 16, simds = 4 * h->cus;
    const int NW = ngroups > simds ? 8 : 4;
    const int nb = (ncols + 16 * NW - 1) / (16 * NW);
    h->sweep_wgs = nb;
    h->sweep_form[h->cur_which] = 2;
    h->sweep_groups[h->cur_which] = NW;
    const hipError_t ea = nnlm_tu_sweep_f(a, nb, NB, NW, h->stream);
    if (ea != hipSuccess && g_attr_err == hipSuccess) {
        g_attr_err = ea;
        g_attr_what = "sweep_scd_f_kernel";
    }
}

static void launch_sweep_q(nnlm_handle *h, const SweepArgs &a)
{
    if (h->prec == NNLM_PREC_F32) return launch_sweep_f(h, a);
    int nb = (a.ncols - a.col0 + SWEEPQ_COLS - 1) / SWEEPQ_COLS;
    const int NB = (a.k + 3) / 4;
    h->sweep_wgs = 0;
    if (nb <= 0) return;
    if (!h->pack_ready)
        sweepq_pack_kernel<<<8, 256, 0, h->stream>>>(a.Graw, a.KPg, a.k, a.r0, a.r1, NB, h->sweepq_img, 1);
    h->pack_ready = false;
    // Launch policy.  A SIMD runs one wavefront (16 columns) of this sweep at full speed and a second one adds its whole time: the plain
    // form costs ceil(groups / SIMDs) rounds of S sweeps.  The persistent form gives every CU G column groups, shared by its four
    // wavefronts by the wrap-around rule -- ceil(G S / 4) sweeps per round of (one workgroup per CU) -- and is taken, with the G that
    // costs least, whenever that is less: the benchmark's W half-step (1250 groups on 1024 SIMDs) G = 5, 1.25 S instead of 2 S;
    // 2500 groups G = 5 in two rounds of workgroups, 2.5 S instead of 3 S (G = 10 in one round costs the same: a tie keeps the smaller
    // G, so 8 and 10 are never taken).  (Costs in quarters of S.)
    const int ngroups = (a.ncols - a.col0 + 15) / 16, simds = 4 * h->cus;
    int G = 0;
    if (ngroups > simds && a.max_iter >= 4) {
        long best = ((long)ngroups + simds - 1) / simds * 4; // the plain form
        for (int g = 5; g <= SWEEPQ_WRAP_MAXG; g++) {
            if (sweepqw_lds_bytes(h->KP, NB, true, g) > (size_t)160 * 1024) break;
            const long wgs = ((long)ngroups + g - 1) / g, rounds = (wgs + h->cus - 1) / h->cus;
            if (rounds * g < best) best = rounds * g, G = g;
        }
    }
    if (G) nb = (ngroups + G - 1) / G;
    h->sweep_wgs = nb;
    h->sweep_form[h->cur_which] = G ? 1 : 0;
    h->sweep_groups[h->cur_which] = G ? G : 4;
    const hipError_t ea = G ? nnlm_tu_sweep_qw(a, h->sweepq_img, nb, NB, true, G, h->stream) : nnlm_tu_sweep_q(a, h->sweepq_img, nb, NB, true, h->stream);
    if (ea != hipSuccess && g_attr_err == hipSuccess) {
        g_attr_err = ea;
        g_attr_what = G ? "sweep_scd_qw_kernel" : "sweep_scd_q_kernel";
    }
}

// rank > 64: one wavefront per column, coordinates in LDS (k_generic.h); g_stride != 0: per-column Grams (missing values)
static int launch_sweep_generic(nnlm_handle *h, int method, const SweepArgs &a, size_t g_stride)
{
    const int ncols = a.ncols - a.col0;
    if (ncols <= 0) return NNLM_OK;
    const bool g_in_lds = g_stride == 0 && sweep_generic_lds_bytes(a.k, a.KPg, true) <= (size_t)160 * 1024;
    const size_t lds = sweep_generic_lds_bytes(a.k, a.KPg, g_in_lds);
    if (lds > (size_t)160 * 1024) return fail(h, NNLM_ERR_UNSUPPORTED, "rank %d needs %zu bytes of LDS per workgroup (limit 160 KiB)", a.k, lds);
    const int nb = (ncols + 3) / 4;
    if (method == 1) {
        set_dyn_lds((const void *)sweep_generic_kernel<1>, (int)lds, "sweep_generic_kernel");
        sweep_generic_kernel<1><<<nb, 256, lds, h->stream>>>(a, g_stride, h->MW, g_in_lds ? 1 : 0);
    } else {
        set_dyn_lds((const void *)sweep_generic_kernel<2>, (int)lds, "sweep_generic_kernel");
        sweep_generic_kernel<2><<<nb, 256, lds, h->stream>>>(a, g_stride, h->MW, g_in_lds ? 1 : 0);
    }
    return NNLM_OK;
}

static int launch_sweep(nnlm_handle *h, int method, const SweepArgs &a)
{
    if (generic_rank(h)) return launch_sweep_generic(h, method, a, 0);
    if (method == 1) {
        launch_sweep_q(h, a);
        return NNLM_OK;
    }
    // Lee's multiplicative updates: sweep_ls_kernel, L lanes per column
    const int L = sweep_lanes_per_column(a.ncols);
    const int rneed = (h->k + L - 1) / L;
    const int step = 8 / L, idx = (rneed + step - 1) / step; // R = step * idx
    h->lee_lanes[h->cur_which] = L;
    h->lee_regs[h->cur_which] = step * idx;
    if (L == 4) launch_sweep_l<2, 4>(idx, method, a, h->stream);      // R = 2..16, k <= 64
    else if (L == 2) launch_sweep_l<4, 2>(idx, method, a, h->stream); // R = 4..32
    else launch_sweep_l<8, 1>(idx, method, a, h->stream);             // R = 8..64
    return NNLM_OK;
}

// strict fp64 mode: kl_reg64_kernel (k_kl.h).  EPT2 = double2 chunks of the contraction per thread (rounded up to an
// instantiated value), C = columns per workgroup (C * EPT2 <= 20 chunks = 160 state registers)
template <int EPT2, int C>
static void launch_kl64_m(int method, const Kl64Args &ka, hipStream_t s, int ran[2])
{
    ran[0] = EPT2, ran[1] = C; // (the instantiation itself, not the ladder's word for it)
    const int nb = (ka.ncols - ka.colbase + C - 1) / C;
    if (nb <= 0) return;
    const size_t lds = kl64_lds_bytes(EPT2, C, ka.k);
    if (method == 3) {
        set_dyn_lds((const void *)kl_reg64_kernel<EPT2, C, 3>, (int)lds, "kl_reg64_kernel");
        kl_reg64_kernel<EPT2, C, 3><<<nb, KL64_THREADS, lds, s>>>(ka);
    } else {
        set_dyn_lds((const void *)kl_reg64_kernel<EPT2, C, 4>, (int)lds, "kl_reg64_kernel");
        kl_reg64_kernel<EPT2, C, 4><<<nb, KL64_THREADS, lds, s>>>(ka);
    }
}
static int kl64_ept2(int p) { return ((p + 1) / 2 + KL64_THREADS - 1) / KL64_THREADS; } // > 20: too long for the register-resident kernel
static bool kl64_fits(int p, int k) { return kl64_ept2(p) <= 20 && kl64_lds_bytes(kl64_ept2(p) <= 5 ? 5 : (kl64_ept2(p) <= 10 ? 10 : 20), 4, k) <= (size_t)160 * 1024; }
// the rounding ladder: the instantiated piece count that takes e exact pieces (e <= 20), and its columns per block
static int kl64_inst(int e)
{
    static const int rungs[] = {1, 2, 3, 5, 7, 10, 12, 14, 16, 18, 20};
    for (int r : rungs)
        if (e <= r) return r;
    return 20;
}
static int kl64_cols(int inst) { return inst <= 5 ? 4 : (inst <= 10 ? 2 : 1); }
static void launch_kl64(int method, const Kl64Args &ka, hipStream_t s, int ran[2])
{
    switch (kl64_inst(kl64_ept2(ka.p))) {
    case 1: launch_kl64_m<1, 4>(method, ka, s, ran); break;
    case 2: launch_kl64_m<2, 4>(method, ka, s, ran); break;
    case 3: launch_kl64_m<3, 4>(method, ka, s, ran); break;
    case 5: launch_kl64_m<5, 4>(method, ka, s, ran); break;
    case 7: launch_kl64_m<7, 2>(method, ka, s, ran); break;
    case 10: launch_kl64_m<10, 2>(method, ka, s, ran); break;
    case 12: launch_kl64_m<12, 1>(method, ka, s, ran); break;
    case 14: launch_kl64_m<14, 1>(method, ka, s, ran); break;
    case 16: launch_kl64_m<16, 1>(method, ka, s, ran); break;
    case 18: launch_kl64_m<18, 1>(method, ka, s, ran); break;
    default: launch_kl64_m<20, 1>(method, ka, s, ran); break;
    }
}

// F32 mode: kl_tile_kernel (k_kl.h).  EPT4 = float4 chunks of the contraction per thread, C = columns per workgroup
// (C * EPT4 * 8 state registers per thread).
template <int EPT4, int C, bool ONEBUF = false>
static void launch_kl_tile_m(int method, const KlTileArgs &ta, int nb, size_t lds, hipStream_t s, int ran[2])
{
    ran[0] = EPT4, ran[1] = C; // (the instantiation itself)
    if (method == 3) {
        set_dyn_lds((const void *)kl_tile_kernel<EPT4, C, 3, ONEBUF>, (int)lds, "kl_tile_kernel");
        kl_tile_kernel<EPT4, C, 3, ONEBUF><<<nb, KLT_THREADS, lds, s>>>(ta);
    } else {
        set_dyn_lds((const void *)kl_tile_kernel<EPT4, C, 4, ONEBUF>, (int)lds, "kl_tile_kernel");
        kl_tile_kernel<EPT4, C, 4, ONEBUF><<<nb, KLT_THREADS, lds, s>>>(ta);
    }
}
// up to 10 pieces per thread: two row buffers, 2 .. 8 columns per block; 11 .. 20 (contractions up to ~40400): one row buffer, one column
static int kl_tile_cols(int ept4) { return ept4 <= 2 ? 8 : (ept4 <= 5 ? 4 : (ept4 <= 10 ? 2 : 1)); }
static int kl_tile_nbuf(int ept4) { return ept4 <= 10 ? 2 : 1; }
static int kl_tile_ept4(int p)
{
    const int e = (kl_tile_p4(p) + KLT_THREADS - 1) / KLT_THREADS; // float4 pieces per thread: the instantiation is exact
    return e <= 20 ? e : 0;                                        // 0: contraction too long for the register-resident kernel
}
static bool kl_tile_fits(int p, int k, int mw_masked)
{
    const int e = kl_tile_ept4(p);
    return e > 0 && kl_tile_lds_bytes(p, k, kl_tile_cols(e), mw_masked, kl_tile_nbuf(e)) <= (size_t)160 * 1024 &&
           2 * round_up_i(k, 2) * ERRF_TILE * 4 <= 160 * 1024;
}
static void launch_kl_tile(int method, const KlTileArgs &ta, hipStream_t s, int ran[2])
{
    const int e = kl_tile_ept4(ta.p), C = kl_tile_cols(e);
    const int nb = (ta.ncols - ta.colbase + C - 1) / C;
    if (nb <= 0) return;
    const size_t lds = kl_tile_lds_bytes(ta.p, ta.k, C, ta.mask ? ta.mw : 0, kl_tile_nbuf(e));
    switch (e) {
    case 11: launch_kl_tile_m<11, 1, true>(method, ta, nb, lds, s, ran); break;
    case 12: launch_kl_tile_m<12, 1, true>(method, ta, nb, lds, s, ran); break;
    case 13: launch_kl_tile_m<13, 1, true>(method, ta, nb, lds, s, ran); break;
    case 14: launch_kl_tile_m<14, 1, true>(method, ta, nb, lds, s, ran); break;
    case 15: launch_kl_tile_m<15, 1, true>(method, ta, nb, lds, s, ran); break;
    case 16: launch_kl_tile_m<16, 1, true>(method, ta, nb, lds, s, ran); break;
    case 17: launch_kl_tile_m<17, 1, true>(method, ta, nb, lds, s, ran); break;
    case 18: launch_kl_tile_m<18, 1, true>(method, ta, nb, lds, s, ran); break;
    case 19: launch_kl_tile_m<19, 1, true>(method, ta, nb, lds, s, ran); break;
    case 20: launch_kl_tile_m<20, 1, true>(method, ta, nb, lds, s, ran); break;
    case 1: launch_kl_tile_m<1, 8>(method, ta, nb, lds, s, ran); break;
    case 2: launch_kl_tile_m<2, 8>(method, ta, nb, lds, s, ran); break;
    case 3: launch_kl_tile_m<3, 4>(method, ta, nb, lds, s, ran); break;
    case 4: launch_kl_tile_m<4, 4>(method, ta, nb, lds, s, ran); break;
    case 5: launch_kl_tile_m<5, 4>(method, ta, nb, lds, s, ran); break;
    case 6: launch_kl_tile_m<6, 2>(method, ta, nb, lds, s, ran); break;
    case 7: launch_kl_tile_m<7, 2>(method, ta, nb, lds, s, ran); break;
    case 8: launch_kl_tile_m<8, 2>(method, ta, nb, lds, s, ran); break;
    case 9: launch_kl_tile_m<9, 2>(method, ta, nb, lds, s, ran); break;
    default: launch_kl_tile_m<10, 2>(method, ta, nb, lds, s, ran); break;
    }
}

template <typename T>
static int launch_kl_stream(nnlm_handle *h, int method, const KlArgs &a, int mw, void *st, size_t ldst, hipStream_t s)
{
    const size_t lds = (size_t)(a.k + 24) * 8;
    if (a.ncols <= a.col0) return NNLM_OK;
    if (lds > (size_t)160 * 1024)
        return fail(h, NNLM_ERR_UNSUPPORTED, "KL solver: rank %d needs %zu bytes of LDS per workgroup (limit 160 KiB)", a.k, lds);
    if (method == 3) {
        HIPCHK(h, hipFuncSetAttribute((const void *)kl_stream_kernel<T, 3>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        kl_stream_kernel<T, 3><<<a.ncols - a.col0, 256, lds, s>>>(a, mw, (T *)st, ldst);
    } else {
        HIPCHK(h, hipFuncSetAttribute((const void *)kl_stream_kernel<T, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        kl_stream_kernel<T, 4><<<a.ncols - a.col0, 256, lds, s>>>(a, mw, (T *)st, ldst);
    }
    return NNLM_OK;
}

template <int NKQ>
static void launch_colsolve_m(const SweepArgs &a, size_t g_stride, hipStream_t s) // Lee's multiplicative updates, per-column Grams
{
    const int nb = (a.ncols - a.col0 + 3) / 4;
    if (nb <= 0) return;
    colsolve_ls_kernel<NKQ, 2><<<nb, 256, 0, s>>>(a, g_stride);
}

// F32 mode, SCD: colsolve_row_kernel (k_colsolve_row.h, tu_colsolve.hip): four columns per wavefront, the step's delta by DPP row broadcast
// Not for per-entry weights with absent entries zeros: there every Gram carries the shared Gram of ALL rows while b_j sums over the few
// stored ones, so from a distant start the scaled gradient is hundreds of times the solution (6.7 against 0.02 with one stored entry
// among 4000 zeros) and a gradient carried in fp32 leaves 1.3e-4 on it, beyond the mode's 1e-4 -- that path solves in fp64
// (colsolve_strict_kernel) in both modes.
static bool colsolve_fast_ok(const nnlm_handle *h, int method)
{
    if (h->sparse && h->sp_weighted && !h->sp_missing) return false;
    return method == 1 && h->prec == NNLM_PREC_F32 && h->k <= NNLM_KQ_MAX;
}

template <int NKQ>
static int launch_colsolve_strict_m(const SweepArgs &a, size_t g_stride, hipStream_t s) // returns the KR of its instantiation
{
    const int nb = (a.ncols - a.col0 + 3) / 4;
    constexpr int KS = NKQ > 1 ? 16 * (NKQ - 1) + 4 : 16;
    if (NKQ > 1 && a.k <= KS) {
        if (nb <= 0) return KS;
        if (a.mask) colsolve_strict_kernel<NKQ, true, KS><<<nb, 256, 0, s>>>(a, g_stride);
        else colsolve_strict_kernel<NKQ, false, KS><<<nb, 256, 0, s>>>(a, g_stride);
        return KS;
    }
    if (nb <= 0) return 16 * NKQ;
    if (a.mask) colsolve_strict_kernel<NKQ, true><<<nb, 256, 0, s>>>(a, g_stride);
    else colsolve_strict_kernel<NKQ, false><<<nb, 256, 0, s>>>(a, g_stride);
    return 16 * NKQ;
}
static void launch_colsolve(nnlm_handle *h, int method, const SweepArgs &a, size_t g_stride)
{
    if (colsolve_fast_ok(h, method)) {
        h->na_solver[h->cur_which] = 0;
        h->na_solver_kr[h->cur_which] = a.k <= 48 ? 16 * ((a.k + 15) / 16) : (a.k <= 50 ? 50 : 64); // (the classes of nnlm_tu_colsolve_row)
        nnlm_tu_colsolve_row(a, g_stride, h->stream);
        return;
    }
    // SCD in the reference's arithmetic (strict mode): the unrolled lane-local form; Lee's updates: colsolve_lee_kernel
    h->na_solver[h->cur_which] = method == 1 ? 1 : 2;
    with_nkq(h->NKQ, [&](auto N) {
        if (method == 1) h->na_solver_kr[h->cur_which] = launch_colsolve_strict_m<N>(a, g_stride, h->stream);
        else {
            launch_colsolve_m<N>(a, g_stride, h->stream);
            h->na_solver_kr[h->cur_which] = 16 * N;
        }
    });
}

// CSR row lists of orientation `which` (see nnlm_handle::na_ptr): count, prefix sum on the host (once), fill
static int ensure_na_lists(nnlm_handle *h, const Side &s)
{
    const int which = s.which, words = s.words, p = s.p, ncols = s.ncols;
    const uint32_t *bits = s.bits;
    if (h->na_ptr[which]) return NNLM_OK;
    uint32_t *cnt = nullptr;
    HIPCHK(h, hipMalloc(&cnt, (size_t)ncols * 4));
    na_count_kernel<<<(ncols + 3) / 4, 256, 0, h->stream>>>(bits, words, p, ncols, cnt);
    std::vector<uint32_t> hc(ncols), hptr(ncols + 1), hmeta(ncols);
    HIPCHK(h, hipMemcpyAsync(hc.data(), cnt, (size_t)ncols * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    hipFree(cnt);
    size_t total = 0;
    for (int c = 0; c < ncols; c++) {
        const uint32_t miss = hc[c];
        const bool complement = (size_t)miss * 2 <= (size_t)p; // sum over the missing rows and subtract from the full Gram
        const uint32_t len = complement ? miss : (uint32_t)p - miss;
        hptr[c] = (uint32_t)total;
        hmeta[c] = len | (complement ? 0x80000000u : 0u);
        total += len;
    }
    hptr[ncols] = (uint32_t)total;
    if (total >= 0x7FFFFFFFull) return fail(h, NNLM_ERR_UNSUPPORTED, "missing-value row lists exceed 2^31 entries");
    HIPCHK(h, hipMalloc(&h->na_ptr[which], (size_t)(ncols + 1) * 4));
    HIPCHK(h, hipMalloc(&h->na_meta[which], (size_t)ncols * 4));
    HIPCHK(h, hipMalloc(&h->na_idx[which], (total + 128) * 4)); // (slack: the Gram kernels request whole groups / steps of indices ahead of the end)
    HIPCHK(h, hipMemcpyAsync(h->na_ptr[which], hptr.data(), (size_t)(ncols + 1) * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->na_meta[which], hmeta.data(), (size_t)ncols * 4, hipMemcpyHostToDevice, h->stream));
    na_fill_kernel<<<ncols, 256, 0, h->stream>>>(bits, words, p, h->na_ptr[which], h->na_meta[which], h->na_idx[which]);
    HIPCHK(h, hipStreamSynchronize(h->stream)); // hptr / hmeta go out of scope
    return NNLM_OK;
}

// Row-major copy of the fixed factor the NA / KL-with-NA paths gather from: [p][KP] doubles or floats, or -- split-fp16 Grams --
// [p + 64][64 hi | 64 lo halves] (256 bytes per row whatever KP is; the rows behind p are zero)
static size_t yrow_bytes(const nnlm_handle *h)
{
    const size_t big = (size_t)(h->npad > h->mpad ? h->npad : h->mpad);
    const size_t a = big * h->KP * 8, b = (big + 64) * 256;
    return a > b ? a : b;
}

// workspaces made on first use (freed with the factors)
static int ensure_yrow(nnlm_handle *h)
{
    if (!h->Yrow) HIPCHK(h, hipMalloc(&h->Yrow, yrow_bytes(h)));
    return NNLM_OK;
}
static int ensure_gcols(nnlm_handle *h)
{
    if (!h->Gcols) {
        const size_t bytes = (size_t)(h->n > h->m ? h->n : h->m) * h->KP * h->KP * 8;
        HIPCHK(h, hipMalloc(&h->Gcols, bytes));
        HIPCHK(h, poison_new_gram(h->Gcols, bytes, h->stream));
    }
    return NNLM_OK;
}
static int ensure_sg_slabs(nnlm_handle *h)
{
    if (!h->sg_slabs) HIPCHK(h, hipMalloc(&h->sg_slabs, sg_slab_count(h) * h->KP * h->KP * 8));
    return NNLM_OK;
}
static int ensure_klsw(nnlm_handle *h)
{
    if (!h->klsw) HIPCHK(h, hipMalloc(&h->klsw, (size_t)h->KP * 8));
    return NNLM_OK;
}
static int ensure_klsw_cols(nnlm_handle *h)
{
    if (!h->klsw_cols) HIPCHK(h, hipMalloc(&h->klsw_cols, (size_t)(h->n > h->m ? h->n : h->m) * h->KP * 8));
    return NNLM_OK;
}

// Per-column Grams of columns [c0, c1) into Gcols (row lists exist for all the side's columns).  A member of a batched factorisation
// (member = true) passes ITS rows of the fixed factor (Y, rank h->k = k_b: rows behind k_b are its neighbour's and enter the row copy
// as zeros), its own full Gram (Gfull, row stride h->KP) and the word that holds max|Y| over its own rows (maxw, F32 mode)
static int launch_na_gram(nnlm_handle *h, const Side &s, int c0, int c1, const double *Y = nullptr, const double *Gfull = nullptr,
                          const unsigned *maxw = nullptr)
{
    const int nc = c1 - c0, p = s.p;
    const bool member = Y != nullptr;
    if (!member) Y = s.Y, Gfull = h->Graw, maxw = h->fixed_maxw ? h->fixed_maxw : h->maxbits;
    if (nc <= 0) return NNLM_OK;
    int rc = ensure_na_lists(h, s);
    if (rc != NNLM_OK) return rc;
    const uint32_t *ptr = h->na_ptr[s.which], *meta = h->na_meta[s.which];
    const int *idx = h->na_idx[s.which];
    // The kernels gather ROWS of the fixed factor [KP][ldy]: row-major copy Yrow.
    // F32 mode: the Grams on the fp16 matrix cores from the split copy of the rows (na_gram_f16_kernel).
    // max|fixed factor| is in *fixed_maxw (prepare_factor16 ran for this half-step's cross product).
    if (h->x16 && !generic_rank(h)) {
        // [p + 64 rows][64 hi | 64 lo halves]; rows p .. are zero (the kernel's "no row" index)
        factor16c_kernel<<<p / 64 + 1, 256, 0, h->stream>>>(Y, s.ldy, p, h->k, maxw, h->scal_exp + 3, (uint32_t *)h->Yrow);
        const int nb = (nc + 3) / 4;
        h->na_gram[s.which] = 0, h->na_gram_nt[s.which] = h->NKQ;
        with_nkq(h->NKQ, [&](auto N) {
            na_gram_f16_kernel<N><<<nb, 256, 0, h->stream>>>(ptr, meta, idx, (const uint32_t *)h->Yrow, p, h->scal_exp + 3, Gfull, h->Gcols, c1, c0, h->k);
        });
        return NNLM_OK;
    }
    if (member) factor_rows_kernel<double><<<(p + 255) / 256, 256, 0, h->stream>>>(Y, s.ldy, p, h->KP, h->Yrow, h->k);
    else factor_rows_kernel<double><<<(p + 255) / 256, 256, 0, h->stream>>>(Y, s.ldy, p, h->KP, h->Yrow);
    if (generic_rank(h)) { // rank > 64: k_generic.h
        const int lds = 16 * h->KP * 8;
        na_gram_generic_kernel<<<nc, 256, lds, h->stream>>>(ptr, meta, idx, h->Yrow, h->KP, Gfull, h->Gcols, c0);
        h->na_gram[s.which] = 4, h->na_gram_nt[s.which] = h->NKQ;
        return NNLM_OK;
    }
    // strict mode: fp64 rows gathered by LDS-DMA, v_mfma_f64_16x16x4_f64 (k_missing.h, na_gram_lds_kernel); tail form for k = 16 j + 1, + 2
    const int nb = (nc + 3) / 4;
    const int ntail = h->k - 16 * (h->NKQ - 1);
    const bool tl = h->NKQ >= 2 && (ntail == 1 || ntail == 2);
    with_nkq(h->NKQ, [&](auto N) {
        auto go = [&](auto nt, auto tail) {
            h->na_gram[s.which] = tail ? 2 : 1, h->na_gram_nt[s.which] = nt; // (the instantiation itself)
            na_gram_lds_kernel<double, nt, tail><<<nb, 256, 0, h->stream>>>(ptr, meta, idx, (const double *)h->Yrow, Gfull, h->Gcols, c1, c0, h->k);
        };
        if constexpr (N == 1) go(N, std::false_type{});
        else if (tl) go(std::integral_constant<int, N - 1>{}, std::true_type{});
        else go(N, std::false_type{});
    });
    return NNLM_OK;
}

// KL methods: no Gram, no cross product -- one block per column streams the column of A and the fixed factor.
// After a W half-step has been enqueued into the alternate buffers: make them current.
static void swap_w(nnlm_handle *h)
{
    h->wcur ^= 1;
    h->W64 = h->W64b[h->wcur];
    h->Wop = h->Wopb[h->wcur];
}

// Phases of a sharded half-step (test hooks drive virtual ranks phase by phase; production runs PH_ALL):
//   PH_A   cross product + Gram over this rank's contraction slab, folded into the [G | C] buffer (before the all-reduce)
//   PH_B   sweep of this rank's columns into the packed slab (after the all-reduce, before the all-gather)
//   PH_C   unpack of the all-gathered slabs into the resident layouts
enum { PH_ALL = 0, PH_A = 1, PH_B = 2, PH_C = 3 };
static int half_step_solve(nnlm_handle *h, const Side &s, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method,
                           int nslabs, bool speculative, int phase, bool colshard = false);

static int pack_prepare(nnlm_handle *h, int ncols, struct ShardCols *out, size_t tail);
static int pack_gather_unpack(nnlm_handle *h, const Side &s, int phase);

// Columns of the factor being solved that this rank sweeps (multi-GPU): equal slabs of cpr columns (multiple of 256).
struct ShardCols {
    int cpr, col0, col1;
};
static ShardCols shard_cols(const nnlm_handle *h, int ncols)
{
    ShardCols c;
    c.cpr = round_up_i((ncols + h->nranks - 1) / h->nranks, 256); // (a whole number of cross-product tiles in both orientations)
    c.col0 = h->rank * c.cpr < ncols ? h->rank * c.cpr : ncols;
    c.col1 = c.col0 + c.cpr < ncols ? c.col0 + c.cpr : ncols;
    return c;
}

// Row sums of the fixed factor (klsw) and, with missing values, per column over its non-missing entries for this launch's columns
// (klsw_cols; src/update_with_missing.cpp:122,130): *sumw_cols = klsw_cols, or NULL
static int kl_row_sums(nnlm_handle *h, const Side &s, const KlArgs &a, const double **sumw_cols)
{
    int rc = ensure_klsw(h);
    if (rc != NNLM_OK) return rc;
    kl_sumw_kernel<<<h->k, 256, 0, h->stream>>>(a.Y, a.ldy, a.p, h->klsw);
    *sumw_cols = nullptr;
    if (!h->any_missing) return NNLM_OK;
    if ((rc = ensure_yrow(h)) != NNLM_OK || (rc = ensure_klsw_cols(h)) != NNLM_OK || (rc = ensure_na_lists(h, s)) != NNLM_OK) return rc;
    factor_rows_kernel<<<(a.p + 255) / 256, 256, 0, h->stream>>>(a.Y, a.ldy, a.p, h->KP, h->Yrow);
    if (a.ncols > a.col0) // (this rank's columns only)
        kl_sumw_cols_kernel<<<(a.ncols - a.col0 + 3) / 4, 256, 0, h->stream>>>(h->na_ptr[s.which] + a.col0, h->na_meta[s.which] + a.col0, h->na_idx[s.which],
                                                                              h->Yrow, h->KP, h->k, h->klsw, h->klsw_cols + (size_t)a.col0 * h->KP, h->KP,
                                                                              a.ncols - a.col0);
    *sumw_cols = h->klsw_cols;
    return NNLM_OK;
}

// Column tiles of width `tile` that hold this launch's columns [a.col0, a.ncols): their number and the first one's first column
// (multi-GPU: only the tiles of this rank's shard -- its first column is a multiple of 256)
struct KlTiles {
    int ny;
    size_t cofs;
};
static KlTiles kl_tiles(const KlArgs &a, int tile)
{
    const int ct0 = a.col0 / tile, ct1 = (a.ncols + tile - 1) / tile;
    return {ct1 > ct0 ? ct1 - ct0 : 0, (size_t)ct0 * tile};
}

// the fields KlTileArgs and Kl64Args share with KlArgs, and the row sums
template <typename K>
static void kl_common_args(K &o, const nnlm_handle *h, const KlArgs &a, const double *sumw_cols)
{
    o.p = a.p;
    o.ncols = a.ncols;
    o.k = a.k;
    o.X = a.X;
    o.Xout = a.Xout;
    o.ldx = a.ldx;
    o.colbase = a.col0;
    o.ldo = a.ldo;
    o.ocol0 = a.ocol0;
    o.sumw = h->klsw;
    o.sumw_cols = sumw_cols;
    o.ldsw = h->KP;
    o.r0 = a.r0;
    o.r1 = a.r1;
    o.r2 = a.r2;
    o.mask = a.mask;
    o.max_iter = a.max_iter;
    o.rel_tol = a.rel_tol;
    o.op = a.op;
    o.op_mode = a.op_mode;
    o.op_ld = a.op_ld;
    o.sweeps = a.sweeps;
}

// Across GPUs the KL methods shard by columns of the factor being solved (the solvers need a column's whole contraction and
// exchange nothing while they run): a rank solves its columns into the packed slab, ONE all-gather returns the factor.
static int half_step_kl(nnlm_handle *h, const Side &s, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method,
                        bool speculative, int phase)
{
    h->pack_tail = 0; // (the KL slabs travel alone)
    if (h->sharded && phase == PH_A) return NNLM_OK; // (test hooks: nothing to all-reduce)
    if (h->sharded && phase == PH_C) {
        int rc = pack_gather_unpack(h, s, phase);
        if (rc == NNLM_OK && s.which == 0 && !speculative) swap_w(h);
        return rc;
    }
    KlArgs a;
    a.k = h->k;
    a.r0 = reg[0];
    a.r1 = reg[1];
    a.r2 = reg[2];
    a.max_iter = inner_max_iter;
    a.rel_tol = inner_rel_tol;
    a.sweeps = sweep_counter(h, speculative);
    a.A = h->A;
    a.op_f64 = (h->prec == NNLM_PREC_F64) ? 1 : 0;
    a.X = s.X; a.Xout = s.Xout; a.ldx = s.ldc; a.Y = s.Y; a.ldy = s.ldy;
    a.a_col_stride = s.which == 1 ? (size_t)h->npad : 1; a.a_i_stride = s.which == 1 ? 1 : (size_t)h->npad; // (A is [mpad][npad])
    a.bits = s.bits; a.words = s.words;
    a.p = s.p; a.ncols = s.ncols;
    a.mask = s.mask;
    a.op = s.op; a.op_mode = s.op_mode; a.op_ld = s.op_ld;
    a.ldo = a.ldx;
    if (h->sharded) { // this rank's columns only, into the packed slab; the unpack writes masters and operands
        ShardCols sc;
        int rcp = pack_prepare(h, s.ncols, &sc, 0);
        if (rcp != NNLM_OK) return rcp;
        a.col0 = sc.col0;
        a.ncols = sc.col1;
        a.Xout = h->pack_send;
        a.ldo = sc.cpr;
        a.ocol0 = sc.col0;
        a.op = nullptr;
        a.op_mode = 0;
    }
    {
    ProfScope ps(h, s.prof_sweep);
    // The register-resident kernels start from the states y = Yt^T x of ALL columns (one GEMM into a matrix-sized buffer) and read
    // contraction-contiguous data (a transposed copy of A for the W half-step): one to two more copies of the matrix in HBM.  Where they
    // cannot be had, the streaming kernel takes the half-step in column chunks, with whatever scratch it can get (strided reads of A for
    // the W half-step: slow, and the reference's arithmetic either way) -- an allocation that fails here is not an error.
    bool tile_path = h->prec == NNLM_PREC_F32 && kl_tile_fits(a.p, h->k, a.mask ? h->MW : 0);
    bool reg64_path = h->prec == NNLM_PREC_F64 && !generic_rank(h) && kl64_fits(a.p, h->k);
    // No room for the matrix-sized What: with two row buffers (contractions up to 20480) kl_tile_kernel forms its starting states itself
    // from the rows of the fixed factor -- 8-12 % slower than the GEMM + read-back at config 3 (4.67 -> 5.03 ms per step,
    // profiles/r06_kl_own_init_ab.log), far ahead of the streaming kernel.  `what_tight` keeps a failed allocation from being retried in
    // every half-step; nnlm_set_matrix clears it.
    bool kl_own_init = false;
    if (tile_path && !h->What) {
        if (h->what_tight || big_malloc((void **)&h->What, (size_t)h->npad * h->mpad * sizeof(float) + 4096) != hipSuccess) {
            h->what_tight = true;
            if (kl_tile_nbuf(kl_tile_ept4(a.p)) == 2) kl_own_init = true;
            else tile_path = false;
        }
    }
    if (reg64_path && !h->What64 &&
        (h->what_tight || big_malloc((void **)&h->What64, (size_t)h->npad * h->mpad * sizeof(double) + 4096) != hipSuccess)) {
        h->what_tight = true;
        reg64_path = false;
    }
    if ((tile_path || reg64_path) && s.which == 0) {
        const int rc = h->at_tight ? NNLM_ERR_UNSUPPORTED : ensure_AT(h, true);
        if (rc == NNLM_ERR_UNSUPPORTED) {
            // the W half-step goes to the streaming kernel: the matrix-sized starting-state buffer is exactly the memory its scratch
            // needs (the H half-step then forms its states itself / streams too), and the failing allocation is not retried every half-step
            h->at_tight = true;
            tile_path = reg64_path = kl_own_init = false;
            hipFree(h->What), hipFree(h->What64);
            h->What = nullptr, h->What64 = nullptr;
            h->what_tight = true;
        } else if (rc != NNLM_OK) return rc;
    }
    if (tile_path) {
        // ---- fp32-operand mode: register-resident state, rows of the fixed factor staged through LDS (kl_tile_kernel) ----
        KlTileArgs ta;
        const size_t cnt = (size_t)h->KP * h->mpad; // fp32 [KP][mpad] copy of H (fixed factor of the W half-step, operand of the GEMM below)
        factor_to_f32_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>(h->H64, cnt, h->Hkq);
        // starting state vectors y = Yt^T x of ALL columns as one GEMM, in the layout the solver reads: [column][contraction] (W half-step,
        // roles swapped: What^T [row of A][column of A], next to the transposed fp32 copy of A)
        const int k2 = round_up_i(h->k, 2);
        const int lds = 2 * k2 * ERRF_TILE * (int)sizeof(float);
        set_dyn_lds((const void *)wh_store_kernel, lds, "wh_store_kernel");
        const KlTiles ct = kl_tiles(a, ERRF_TILE);
        const float *Yf = s.which == 1 ? (const float *)h->Wop : h->Hkq, *Xf = s.which == 1 ? h->Hkq : (const float *)h->Wop; // fixed, solved factor
        const int nx = s.ldy / ERRF_TILE;
        if (ct.ny > 0 && !kl_own_init)
            wh_store_kernel<<<8u * ((nx + 7) / 8) * ct.ny, 256, lds, h->stream>>>(Yf, s.ldy, Xf + ct.cofs, s.ldc, k2, h->What + ct.cofs * s.ldy, s.ldy, nx);
        ta.Adata = (const float *)a_contig(h, s);
        ta.Yf = Yf;
        ta.lda = (size_t)s.ldy;
        ta.Yinit = kl_own_init ? nullptr : h->What;
        ta.ldyf = s.ldy;
        const double *sumw_cols;
        int rc = kl_row_sums(h, s, a, &sumw_cols);
        if (rc != NNLM_OK) return rc;
        kl_common_args(ta, h, a, sumw_cols);
        ta.mw = h->MW;
        int ran[2] = {0, 0};
        launch_kl_tile(method, ta, h->stream, ran);
        h->kl_form[s.which] = kl_own_init ? 1 : 0;
        h->kl_pieces[s.which] = ran[0], h->kl_cols[s.which] = ran[1];
    } else if (reg64_path) {
        // ---- strict fp64 mode: register-resident fp64 state, the row of the fixed factor parked in LDS between the passes ----
        // (starting states: What64[j][i], the layout of A; W half-step, roles swapped: What64^T [row of A][column of A], next to AT)
        Kl64Args ka;
        const int k4 = round_up_i(h->k, 4);
        const KlTiles ct = kl_tiles(a, 64);
        dim3 grid(s.ldy / 64, ct.ny > 0 ? ct.ny : 1);
        if (ct.ny > 0)
            wh_store64_kernel<<<grid, 256, 0, h->stream>>>(s.Y, s.ldy, s.X + ct.cofs, s.ldc, k4, h->What64 + ct.cofs * s.ldy, (size_t)s.ldy, s.p,
                                                           s.ncols - (int)ct.cofs);
        ka.Adata = (const double *)a_contig(h, s);
        ka.lda = (size_t)s.ldy;
        ka.Yinit = h->What64;
        ka.Y = a.Y;
        ka.ldy = a.ldy;
        const double *sumw_cols;
        int rc = kl_row_sums(h, s, a, &sumw_cols);
        if (rc != NNLM_OK) return rc;
        kl_common_args(ka, h, a, sumw_cols);
        int ran[2] = {0, 0};
        launch_kl64(method, ka, h->stream, ran);
        h->kl_form[s.which] = 2;
        h->kl_pieces[s.which] = ran[0], h->kl_cols[s.which] = ran[1];
    } else {
        // ---- no size limits: state vectors and data columns streamed from a scratch buffer (kl_stream_kernel), `chunk` columns at a
        // time: the whole range when the scratch for it can be had (two vectors per column), otherwise as many as fit
        const size_t per_col = (size_t)2 * s.ldy * esize(h);
        const int range = a.ncols > a.col0 ? a.ncols - a.col0 : 0;
        int chunk = range;
        if (range > 0 && h->klst_bytes < (size_t)range * per_col) {
            // A smaller scratch is kept only once an allocation of the full size has actually failed for this matrix (`klst_tight`):
            // otherwise the two half-steps of an iteration, whose sizes differ slightly (n x mpad against m x npad), would have the
            // larger one split into a full launch + a tail launch of a few columns in every iteration.
            if (h->klst_tight && h->klst_bytes >= (size_t)64 * per_col && h->klst_bytes / per_col >= (size_t)range / 8)
                chunk = (int)(h->klst_bytes / per_col);
            else {
                hipFree(h->klst);
                h->klst = nullptr;
                h->klst_bytes = 0;
                for (;; chunk = (chunk + 1) / 2) {
                    if (big_malloc(&h->klst, (size_t)chunk * per_col) == hipSuccess) break;
                    h->klst_tight = true;
                    if (chunk <= 64) return fail(h, NNLM_ERR_HIP, "KL solver: no scratch for even %d columns (%zu bytes)", chunk, (size_t)chunk * per_col);
                }
                h->klst_bytes = (size_t)chunk * per_col;
            }
        }
        h->kl_form[s.which] = 3;
        h->kl_pieces[s.which] = h->kl_cols[s.which] = 0;
        const int col_end = a.ncols;
        for (int c0 = a.col0; c0 < col_end; c0 += chunk) {
            KlArgs ac = a;
            ac.col0 = c0;
            ac.ncols = (c0 + chunk < col_end) ? c0 + chunk : col_end;
            // (the kernel addresses the scratch by absolute column: the chunk's slots start at its first column)
            char *st = (char *)h->klst - (size_t)c0 * per_col;
            const int rcs = (h->prec == NNLM_PREC_F64) ? launch_kl_stream<double>(h, method, ac, h->MW, st, (size_t)s.ldy, h->stream)
                                                       : launch_kl_stream<float>(h, method, ac, h->MW, st, (size_t)s.ldy, h->stream);
            if (rcs != NNLM_OK) return rcs;
        }
    }
    }
    LAUNCHCHK(h);
    if (h->sharded) {
        if (phase == PH_B) return NNLM_OK; // test hooks: the caller gathers the slabs
        int rc = pack_gather_unpack(h, s, phase);
        if (rc != NNLM_OK) return rc;
    }
    if (s.which == 0 && !speculative) swap_w(h);
    return NNLM_OK;
}

static int errors_launch(nnlm_handle *h, hipStream_t st, bool with_sweeps, int fused_nb, bool need_pen);

// W^T A over the CSC (H half-step) / A H^T over the CSR (W half-step) into ONE slab of Cx: a row copy of the fixed factor, spmm_kernel
// (k_sparse.h; rank > 64: one SpMM launch per 64 coordinates)
static void sp_cross(nnlm_handle *h, const Side &s)
{
    const int p = s.p;
    {
        ProfScope ps(h, s.prof_spmm);
        const bool f64 = h->prec == NNLM_PREC_F64;
        if (f64) factor_rows_kernel<double><<<(p + 255) / 256, 256, 0, h->stream>>>(s.Y, s.ldy, p, h->KP, (double *)h->sp_Y);
        else factor_rows_kernel<float><<<(p + 255) / 256, 256, 0, h->stream>>>(s.Y, s.ldy, p, h->KP, (float *)h->sp_Y);
        SpmmArgs a;
        a.ptr = s.sp_ptr;
        a.idx = s.sp_idx;
        a.val = h->sp_weighted ? s.sp_wa : s.sp_val; // (per-entry weights: b_j sums c_e a_e y_row(e) -- the same kernel on c a)
        a.Y = h->sp_Y;
        a.nnz = h->nnz;
        a.ncols = s.ncols;
        a.KP = h->KP;
        a.nworkers = nnlm_sp_workers(h->nnz, h->KP, h->cus_device);
        a.chunk = (h->nnz + a.nworkers - 1) / a.nworkers;
        if (a.chunk < 1) a.chunk = 1;
        a.C = h->Cx;
        a.ldc = s.ldc;
        a.carry = h->sp_carry;
        for (int q0 = 0; q0 < h->KP; q0 += 64) {
            a.q0 = q0;
            nnlm_tu_spmm(a, f64, h->stream);
        }
    }
}

// Column chunks of orientation o whose Grams (slot = KP^2 doubles each, + the segment slots of their long columns) fit in
// min(1 GiB, nnlm_debug_alloc_limit) bytes, at least one column per chunk; planned once per budget, the buffer grows to the largest chunk
static int spg_prepare(nnlm_handle *h, int o, size_t slot)
{
    size_t budget = (size_t)1 << 30;
    const size_t lim = g_debug_alloc_limit.load(std::memory_order_relaxed);
    if (lim && lim < budget) budget = lim;
    size_t cap = budget / (slot * 8);
    if (cap < 1) cap = 1;
    if (h->spg_plan_cap[o] != cap) {
        const std::vector<long long> &hp = h->spg_hptr[o];
        const int ncols = (int)hp.size() - 1;
        std::vector<SpgChunk> &pl = h->spg_plan[o];
        pl.clear();
        size_t mx = 0, cols = 0, segs = 0;
        SpgChunk ch{0, 0, 0, 0};
        int l = 0;
        auto close = [&](int c) {
            ch.c1 = c;
            ch.l1 = l;
            pl.push_back(ch);
            mx = cols + segs > mx ? cols + segs : mx;
            ch = SpgChunk{c, c, l, l};
            cols = segs = 0;
        };
        for (int c = 0; c < ncols; c++) {
            const long long len = hp[(size_t)c + 1] - hp[c];
            const size_t ns = len > SPG_SEG ? (size_t)((len + SPG_SEG - 1) / SPG_SEG) : 0;
            if (cols > 0 && cols + segs + 1 + ns > cap) close(c);
            cols++;
            segs += ns;
            if (ns) l++;
        }
        close(ncols);
        h->spg_plan_slots[o] = mx;
        h->spg_plan_cap[o] = cap;
    }
    const size_t need = h->spg_plan_slots[o] * slot * 8;
    if (need > h->spg_buf_bytes) {
        sync_all(h); // (the previous buffer may still be read)
        hipFree(h->spg_buf);
        h->spg_buf = nullptr;
        h->spg_buf_bytes = 0;
        HIPCHK(h, hipMalloc(&h->spg_buf, need));
        h->spg_buf_bytes = need;
        HIPCHK(h, poison_new_gram(h->spg_buf, need, h->stream));
    }
    return NNLM_OK;
}

// Square-loss half-step on a sparse A whose absent entries are missing (k_sparse_na.h; update_with_missing, src/update_with_missing.cpp:58-139):
// the cross product of the zero semantics (it sums over the stored entries either way), then chunk by chunk the per-column Grams over the
// stored rows (sp_gram_kernel + its fix-up) and the dense NA path's per-column solvers on them (launch_colsolve, unchanged).  Nothing
// max(n, m) x KP^2 sized is held: a chunk's Grams live in spg_buf, and the solvers find column col at (col - gcol0) * KP^2 (gcol0 = c0).
// Per-entry weights (nnlm_set_matrix_csc_weighted): the reference's half-step on the column problem whose rows are scaled by sqrt(c) --
// G_j = c0 G_full + sum over the stored entries of (c_e - c0) y y^T, b_j = sum of c_e a_e y, c0 = 0 (absent = missing) or 1 (absent =
// zero: the shared Gram of the fixed factor is formed first, raw, and the Gram kernels add it once per column).
static int half_step_sparse_missing(nnlm_handle *h, const Side &s, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method,
                                    bool speculative)
{
    const bool shared_gram = h->sp_weighted && !h->sp_missing;
    if (shared_gram) {
        ProfScope ps(h, P_GRAM, h->stream);
        launch_gram(h, s, 0, s.p);
    }
    sp_cross(h, s);
    if (speculative) HIPCHK(h, hipEventRecord(h->ev_xdone, h->stream));
    h->cur_which = s.which;
    const int o = s.which, KP = h->KP;
    const size_t slot = (size_t)KP * KP;
    int rc = spg_prepare(h, o, slot);
    if (rc != NNLM_OK) return rc;
    int workers = 0;
    SweepArgs a = sweep_args(h, s, reg, inner_max_iter, inner_rel_tol, sweep_counter(h, speculative));
    SpGramArgs g;
    g.ptr = s.sp_ptr;
    g.idx = s.sp_idx;
    g.Y = h->sp_Y;
    g.segoff = h->spg_segoff[o];
    g.G = h->spg_buf; // [chunk columns][slot], then the chunk's segment slots
    if (h->sp_weighted) {
        g.wt = s.sp_wt;
        g.cw0 = shared_gram ? 1.0 : 0.0;
        g.Gfull = shared_gram ? h->Graw : nullptr;
    }
    const std::vector<long long> &hp = h->spg_hptr[o];
    for (const SpgChunk &ch : h->spg_plan[o]) {
        {
            ProfScope ps(h, P_SP_GRAM);
            g.c0 = ch.c0;
            g.c1 = ch.c1;
            g.seg = h->spg_buf + (size_t)(ch.c1 - ch.c0) * slot;
            const long long nnz = hp[ch.c1] - hp[ch.c0];
            g.nworkers = nnlm_spg_workers(nnz, h->cus_device);
            workers += g.nworkers;
            g.chunk = (nnz + g.nworkers - 1) / g.nworkers;
            if (g.chunk < 1) g.chunk = 1;
            nnlm_tu_sp_gram(g, h->NKQ, h->prec == NNLM_PREC_F64, h->stream);
            h->na_gram[o] = 3, h->na_gram_nt[o] = h->NKQ;
            nnlm_tu_sp_gram_fixup(g, h->spg_longc[o] + ch.l0, ch.l1 - ch.l0, KP, h->stream);
        }
        ProfScope ps(h, s.prof_sweep);
        a.col0 = ch.c0;
        a.ncols = ch.c1;
        a.Graw = h->spg_buf; // (the chunk's Grams: column col at spg_buf + (col - gcol0) * slot)
        a.gcol0 = ch.c0;
        launch_colsolve(h, method, a, slot);
    }
    h->spg_chunks = (int)h->spg_plan[o].size();
    h->spg_workers = workers;
    LAUNCHCHK(h);
    if (s.which == 0 && !speculative) swap_w(h);
    return NNLM_OK;
}

static int spkl_rank_refusal(nnlm_handle *h, const char *who)
{
    return fail(h, NNLM_ERR_UNSUPPORTED, "%s: rank %d with KL loss on a sparse matrix: the sparse KL solvers take ranks up to %d (use a dense matrix)", who,
                h->k, NNLM_KQ_MAX);
}

// KL half-step on a sparse A loaded by nnlm_set_matrix_csc_kl (k_sparse_kl.h; update(), src/update_with_missing.cpp:27,47-49, on the
// stored entries): the row copy and the column sums of the fixed factor, then the per-line solvers -- the short form over all lines (it
// leaves out the long ones), the long form over the list made when the matrix was set.  Nothing n x m sized; one T per stored entry
// (spkl_state) when the orientation has a long line.
static int half_step_sparse_kl(nnlm_handle *h, const Side &s, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method,
                               bool speculative)
{
    if (h->k > NNLM_KQ_MAX) return spkl_rank_refusal(h, "half_step");
    const int o = s.which;
    const bool f64 = h->prec == NNLM_PREC_F64;
    int rc = ensure_klsw(h);
    if (rc != NNLM_OK) return rc;
    if (h->spkl_nlong[o] > 0 && !h->spkl_state) HIPCHK(h, hipMalloc(&h->spkl_state, (size_t)h->nnz * (f64 ? 8 : 4) + 64));
    {
        ProfScope ps(h, P_SPKL_COPY);
        if (f64) factor_rows_kernel<double><<<(s.p + 255) / 256, 256, 0, h->stream>>>(s.Y, s.ldy, s.p, h->KP, (double *)h->sp_Y);
        else factor_rows_kernel<float><<<(s.p + 255) / 256, 256, 0, h->stream>>>(s.Y, s.ldy, s.p, h->KP, (float *)h->sp_Y);
        kl_sumw_kernel<<<h->k, 256, 0, h->stream>>>(s.Y, s.ldy, s.p, h->klsw);
    }
    SpKlArgs a;
    a.ptr = s.sp_ptr; a.idx = s.sp_idx; a.val = s.sp_val;
    a.Y = h->sp_Y;
    a.KP = h->KP; a.ncols = s.ncols; a.k = h->k;
    a.X = s.X; a.Xout = s.Xout; a.ldx = s.ldc;
    a.sumw = h->klsw;
    a.r0 = reg[0]; a.r1 = reg[1]; a.r2 = reg[2];
    a.mask = s.mask; a.mw = h->MW;
    a.max_iter = inner_max_iter; a.rel_tol = inner_rel_tol;
    a.op = s.op; a.op_mode = s.op_mode; a.op_ld = s.op_ld;
    a.sweeps = sweep_counter(h, speculative);
    a.state = h->spkl_state;
    a.longc = h->spkl_longc[o];
    a.nlong = h->spkl_nlong[o];
    {
        ProfScope ps(h, o == 1 ? P_SPKL_H : P_SPKL_W);
        nnlm_tu_sp_kl(a, method, f64, h->spkl_nshort[o], h->stream);
    }
    h->spkl_form[o] = (h->spkl_nshort[o] > 0 ? 1 : 0) | (h->spkl_nlong[o] > 0 ? 2 : 0);
    LAUNCHCHK(h);
    if (s.which == 0 && !speculative) swap_w(h);
    return NNLM_OK;
}

// Square-loss half-step on a sparse A (k_sparse.h): the Gram of the fixed factor (launch_gram), the SpMM (sp_cross) into ONE slab of Cx,
// then the solvers of the dense path unchanged (half_step_solve; rank > 64: the generic Gram and sweep).  Absent entries missing (and some
// absent): half_step_sparse_missing.
static int half_step_sparse(nnlm_handle *h, const Side &s, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method, bool speculative)
{
    if (method >= 3 && h->sp_kl) return half_step_sparse_kl(h, s, reg, inner_max_iter, inner_rel_tol, method, speculative);
    if (method >= 3 && h->sp_weighted) return weighted_refusal(h, "half_step", "methods 3 and 4 (KL loss)");
    if (method >= 3)
        return fail(h, NNLM_ERR_UNSUPPORTED, "method %d (KL loss) is not available for a sparse matrix: use loss = 'mse' (methods 1, 2) or a dense matrix", method);
    // (every entry stored: the reference's update(), src/update_with_missing.cpp:3-55 -- the shared Gram of the zero semantics)
    // (per-entry weights: every column has a Gram of its own whatever an absent entry is, and whether or not anything is absent)
    if (h->sp_weighted) {
        if (h->k > NNLM_KQ_MAX) return weighted_refusal(h, "half_step", "a rank above 64");
        return half_step_sparse_missing(h, s, reg, inner_max_iter, inner_rel_tol, method, speculative);
    }
    if (h->sp_missing && h->any_missing) return half_step_sparse_missing(h, s, reg, inner_max_iter, inner_rel_tol, method, speculative);
    {
        ProfScope ps(h, P_GRAM, h->stream);
        launch_gram(h, s, 0, s.p);
    }
    sp_cross(h, s);
    if (speculative) HIPCHK(h, hipEventRecord(h->ev_xdone, h->stream));
    return half_step_solve(h, s, reg, inner_max_iter, inner_rel_tol, method, 1, speculative, PH_ALL, false);
}

// speculative (W half-step only): the result goes to the alternate W buffers and the alternate sweep counter and is
// NOT made current; the caller accepts it later with swap_w() / sw_active ^= 1, or simply drops it.
static int half_step(nnlm_handle *h, int which, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method,
                     bool partial_only = false, bool speculative = false, int phase = PH_ALL)
{
    if (!has_matrix(h) || !h->W64) return fail(h, NNLM_ERR_ARG, "half_step: matrix and factors must be set first");
    if (method < 1 || method > 4) return fail(h, NNLM_ERR_ARG, "method must be 1..4 (got %d)", method);
    HIPCHK(h, hipSetDevice(h->device));
    g_attr_err = hipSuccess; // (a refusal latched by an earlier call on this thread that returned before its LAUNCHCHK is not this call's)
    const int sg_which = h->sg_which; // what the previous sweep left behind (any half-step rewrites a factor: reset first)
    const int sg_other = h->sg_other;
    h->sg_prev = sg_which;
    h->sg_which = h->sg_other = -1;
    h->sg_request = false;
    const Side s = side_of(h, which);
    const int solved_by = which ^ 1; // the half-step that solved this half-step's fixed factor
    if (h->sparse) return half_step_sparse(h, s, reg, inner_max_iter, inner_rel_tol, method, speculative);
    if (generic_rank(h) && h->sharded && method < 3 && !h->any_missing && !h->dense_cols)
        return fail(h, NNLM_ERR_UNSUPPORTED, "rank > %d across GPUs: only the column-sharded form (nnlm_comm_set_form(h, NNLM_FORM_COLS))", NNLM_KQ_MAX);
    if (partial_only) phase = PH_A;
    if (method >= 3) return half_step_kl(h, s, reg, inner_max_iter, inner_rel_tol, method, speculative, phase);
    // Missing values across GPUs: every column has a Gram of its own, so the column is the unit: a rank forms the
    // cross product of ITS columns over the whole contraction, their Grams, solves them, and ONE all-gather returns the factor --
    // no all-reduce.  Test hooks: phase 1 is empty, phase 2 computes and packs, phase 3 unpacks.
    // Dense square loss across GPUs, two forms.  "reduce" (north_star's wording): contraction-sharded [G | C], one
    // all-reduce, column-sharded sweep, one all-gather.  "cols": the column-sharded form of the NA / KL paths -- a rank forms the cross
    // product of ITS columns over the whole contraction (it holds all of A and, after the previous all-gather, all of the fixed
    // factor), the full Gram of the fixed factor (2 k^2 p flops, replicated), sweeps its columns, ONE all-gather.  Same HBM bytes per
    // rank (1/N of A either way), no all-reduce of the (KP^2 + KP cols) doubles: nnlm_comm_set_form, NNLM_FORM_COLS (default) | NNLM_FORM_REDUCE.
    // (read when the communicator is set up: nnlm_comm_init)
    const bool colshard = h->sharded && (h->any_missing || h->dense_cols);
    if (colshard && phase == PH_A) return NNLM_OK;
    if (phase == PH_C || (phase == PH_B && !colshard)) {
        const HalfPlan pp = plan_half(h, which, h->rank, h->nranks, h->fuse_err);
        return half_step_solve(h, s, reg, inner_max_iter, inner_rel_tol, method, pp.S, speculative, phase, colshard);
    }
    if (h->any_missing) { // NA path workspaces, on first use
        int rc = ensure_yrow(h);
        if (rc == NNLM_OK) rc = ensure_gcols(h);
        if (rc != NNLM_OK) return rc;
    }
    HalfPlan p = plan_half(h, which, colshard ? 0 : h->rank, colshard ? 1 : h->nranks, h->fuse_err);
    if (colshard) { // own columns only, whole contraction
        const ShardCols sc = shard_cols(h, s.ncols);
        const int tile = XPROD_TN_BJ;
        p.col_off = sc.col0;
        p.tiles_x = 0, p.cols = 0;
        if (sc.col1 > sc.col0) plan_cols(h, which, (sc.col1 - sc.col0 + tile - 1) / tile * tile, p, h->fuse_err);
        const size_t need = (size_t)p.S * s.slab_stride;
        if (need > h->Cx_elems) { // (fewer tiles -> deeper split-K than the single-GPU plan the slabs were sized for)
            sync_all(h);
            hipFree(h->Cx);
            h->Cx = nullptr;
            h->Cx_elems = 0;
            HIPCHK(h, hipMalloc(&h->Cx, need * 8));
            HIPCHK(h, hipMemset(h->Cx, 0, need * 8));
            h->Cx_elems = need;
        }
    }
    // Dense SCD half-step of the split-fp16 mode on ONE stream.  The small kernels between a sweep and the next cross product
    // cost as much as they overlap (kernel timeline: 47 us from sweep end to cross product start, 24 us from its end to the
    // next sweep, a third of it cross-stream event latency), so they are fused instead: gram_partial also yields max|factor|
    // (no absmax pass, no memset), gram_reduce also writes the chain-wave constants of the strict sweep, and nothing waits on
    // another stream.
    h->pack_ready = false;
    if (h->x16 && !h->sharded && !h->any_missing && method == 1 && !generic_rank(h)) {
        // The one-wavefront sweep kernel (k_sweep_q.h) leaves max|x| and the Gram partial sums of the factor it solved -- the fixed
        // factor of the NEXT half-step -- behind, computed from its LDS image (+1 us per sweep): the kernels in front of the cross
        // product are then factor16_fold (split copy + sum of the workgroups' slabs) and the sweep's operand image, neither of
        // which needs a fence -- gram_partial (12 us) and the "last block" step of gram_reduce_consts (most of its 15 us:
        // __threadfence() is a cross-XCD cache write-back here) are gone.
        const bool fastsw = sweep_fast(h);
        if (fastsw) {
            int rc = ensure_sg_slabs(h);
            if (rc != NNLM_OK) return rc;
        }
        unsigned *smax_w = fastsw ? h->maxbits + 4 + (h->sg_par ^ 1) : nullptr; // this half-step's sweep writes its max here
        h->sg_request = fastsw;
        {
            ProfScope ps(h, P_GRAM, h->stream);
            if (fastsw && sg_which == solved_by) {
                SweepImg im;
                im.img = nullptr; // (fp32-operand mode: sweep_scd_f_kernel builds its operands from Graw itself -- no image)
                im.NB = (h->k + 3) / 4, im.NP = sweepq_np(im.NB, false), im.k = h->k, im.r0 = reg[0], im.r1 = reg[1];
                if (h->fuse_err && which == 0 && sg_other == 0) {
                    // trace iteration, max|W| still in the word W's sweep left it in: the split copies of H (rows and kq-contiguous) and of
                    // W (kq-contiguous) and the fold in one launch; the fused kernel clears that word for this half-step's sweep
                    const size_t cnt = (size_t)h->KP * h->mpad;
                    const unsigned nblk = (unsigned)(h->KP * h->KP / 64 + (cnt + 1023) / 1024 + h->mpad / 64 + h->npad / 64);
                    factor16_fold_err_kernel<<<nblk, 1024, 0, h->stream>>>(h->H64, h->mpad, h->m, h->W64, h->npad, h->n, h->k, h->KP, h->maxbits + 4 + h->sg_par,
                                                                           smax_w, h->scal_exp + 1, h->scal_exp + 2, h->Y16, h->H16c, h->W16c, h->sg_slabs,
                                                                           h->sg_nslabs, h->Graw, im);
                    h->y16_for = -1;
                    h->err_zero_word = smax_w;
                } else if (h->fuse_err) { // (the general routine)
                    prepare_factor16(h, s, h->maxbits + 4 + h->sg_par, smax_w, which == 0 && sg_other == 0);
                    gram_fold_kernel<<<h->KP * h->KP / 64, 1024, 0, h->stream>>>(h->sg_slabs, h->sg_nslabs, h->KP, h->Graw, im);
                } else {
                    const size_t cnt = (size_t)h->KP * s.ldy;
                    factor16_fold_kernel<<<(unsigned)(h->KP * h->KP / 64 + (cnt + 1023) / 1024), 1024, 0, h->stream>>>(
                        s.Y, s.ldy, s.p, h->k, h->KP, s.ldy, h->maxbits + 4 + h->sg_par, h->scal_exp + 1, h->Y16, smax_w, h->sg_slabs, h->sg_nslabs, h->Graw, im);
                }
                h->pack_ready = true;
            } else {
                unsigned *mb = h->maxbits + 1 + h->mb_par, *mb_next = h->maxbits + 1 + (h->mb_par ^ 1);
                h->mb_par ^= 1;
                const int nb = launch_gram_partial(h, s.Y, s.ldy, 0, s.p, h->gslabs, mb, h->stream);
                prepare_factor16(h, s, mb, smax_w);
                gram_reduce_kernel<<<(h->KP * h->KP + 255) / 256, 256, 0, h->stream>>>(h->gslabs, nb, h->KP, h->Graw);
                HIPCHK(h, hipMemsetAsync(mb_next, 0, sizeof(unsigned), h->stream)); // the max word the NEXT half-step's gram_partial accumulates into
            }
        }
        {
            ProfScope ps(h, s.prof_xprod);
            launch_xprod16(h, s, p);
        }
        if (speculative) HIPCHK(h, hipEventRecord(h->ev_xdone, h->stream));
        return half_step_solve(h, s, reg, inner_max_iter, inner_rel_tol, method, p.S, speculative, phase);
    }
    // 1. Gram of the fixed factor over this rank's contraction slab -- on the main stream, AHEAD of the cross product.  (Rounds 1-2
    // ran it on a second stream next to the A-streaming kernel: the cross product owns every CU's LDS, the Gram kernel got slots
    // only as its workgroups retired and stretched from 0.03 to 0.5-1.0 ms while slowing the cross product down with it --
    // profiles/r03_f64_cfg2_a_kernel_stats.csv: xprod_tn 0.44 .. 1.6 ms, gram_partial 0.03 .. 0.99 ms.)
    // (multi-GPU, dense SCD, column form: the unpack of the previous half-step already summed the ranks' Gram partial sums of this
    //  half-step's fixed factor into Graw -- shard_gram_sum_kernel -- instead of every rank recomputing the whole Gram)
    const bool gram_cached = colshard && method == 1 && !h->any_missing && !generic_rank(h) && h->gshard_for == solved_by;
    // (one GPU, strict mode, dense SCD: the sweep that solved the fixed factor left the Gram partial sums of its workgroups behind, as
    //  in the split-fp16 flow above -- one fold instead of gram_partial + gram_reduce over the whole factor)
    const bool sg_strict = !h->sharded && !h->x16 && h->prec == NNLM_PREC_F64 && method == 1 && !h->any_missing && !generic_rank(h);
    if (sg_strict) {
        int rc = ensure_sg_slabs(h);
        if (rc != NNLM_OK) return rc;
        h->sg_request = true; // this half-step's sweep leaves its slabs for the next one
    }
    unsigned *gmb = nullptr;
    if (sg_strict && sg_which == solved_by) {
        ProfScope ps(h, P_GRAM, h->stream);
        SweepImg im; // (the fold also writes the sweep's operand image: no sweepq_pack_kernel launch)
        im.img = h->sweepq_img, im.NB = (h->k + 3) / 4, im.NP = sweepq_np(im.NB, true), im.k = h->k, im.r0 = reg[0], im.r1 = reg[1];
        gram_fold_kernel<<<h->KP * h->KP / 64, 1024, 0, h->stream>>>(h->sg_slabs, h->sg_nslabs, h->KP, h->Graw, im);
        h->pack_ready = true;
        h->gshard_for = -1;
    } else if (!gram_cached) {
        h->gshard_for = -1;
        ProfScope ps(h, P_GRAM, h->stream);
        const int CE = stage_elems(h);
        int c0 = p.stage_begin * CE, c1 = p.stage_end * CE;
        const int lim = s.p;
        if (c1 > lim) c1 = lim;
        if (c0 > c1) c0 = c1;
        // (one GPU, split-fp16 mode: the Gram pass also leaves max|fixed factor| for the split copies -- no absmax pass; the two
        // words alternate as in the dense path above, each zeroed one half-step before its use)
        if (h->x16 && !h->sharded && !generic_rank(h) && c0 == 0 && c1 == lim) {
            gmb = h->maxbits + 1 + h->mb_par;
            h->mb_par ^= 1;
        }
        launch_gram(h, s, c0, c1, gmb);
        if (gmb) HIPCHK(h, hipMemsetAsync(h->maxbits + 1 + h->mb_par, 0, sizeof(unsigned), h->stream));
    }
    // 2. cross product slabs
    if (h->x16) {
        // (multi-GPU: the unpack of the previous half-step left max|fixed factor| behind -- no absmax pass)
        unsigned *mb = (h->sharded && h->upk_max_for == solved_by) ? h->maxbits + 6 + solved_by : gmb;
        // (dense SCD, column form: that unpack also wrote the split copy and its exponent -- the ranks' maxima travelled with the slabs)
        if (!(h->sharded && mb && h->y16_for == solved_by && !h->fuse_err)) prepare_factor16(h, s, mb);
        h->fixed_maxw = mb ? mb : h->maxbits;
    }
    if (p.tiles_x > 0) {
        ProfScope ps(h, s.prof_xprod);
        if (generic_rank(h)) {
            int rcx = launch_xprod_generic(h, s, p);
            if (rcx != NNLM_OK) return rcx;
        } else if (h->x16) launch_xprod16(h, s, p);
        else {
            if (which == 0) {
                int rca = ensure_AT(h);
                if (rca != NNLM_OK) return rca;
            }
            launch_xprod_nkq(h, s, p);
        }
    }
    if (speculative) HIPCHK(h, hipEventRecord(h->ev_xdone, h->stream)); // the error block starts once A is no longer streamed
    if (speculative && h->err_hook) { // (multi-GPU trace iteration: see err_hook)
        h->err_hook = false;
        int fnb = h->fused_nb;
        if (h->fuse_err && fnb == 0) { // a rank without columns launched no fused cross product: it contributes zeros to the two sums
            HIPCHK(h, hipMemsetAsync(h->partials, 0, 2 * sizeof(double), h->stream));
            HIPCHK(h, hipEventRecord(h->ev_xdone, h->stream));
            fnb = 1;
        }
        const int rce = errors_launch(h, h->stream_e, true, fnb, h->err_need_pen);
        if (rce != NNLM_OK) return rce;
        h->fused_nb = 0;
        h->err_launched = true;
    }
    // (multi-GPU) fold the split-K slabs into the contiguous [G | C] buffer; ONE all-reduce sums it over ranks
    if (h->sharded && !colshard) {
        const size_t cnt = s.slab_stride;
        slab_reduce_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>(h->Cx, p.S, cnt, h->red + (size_t)h->KP * h->KP);
        if (phase == PH_A) return NNLM_OK; // test hooks: the caller performs the exchange
        if (h->comm) {
            ProfScope ps(h, P_ALLREDUCE);
            ncclResult_t r = g_rccl.AllReduce(h->red, h->red, (size_t)h->KP * h->KP + cnt, ncclDouble, ncclSum, (ncclComm_t)h->comm, h->stream);
            if (r != ncclSuccess) return fail(h, NNLM_ERR_COMM, "ncclAllReduce failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
        }
    }
    return half_step_solve(h, s, reg, inner_max_iter, inner_rel_tol, method, p.S, speculative, phase, colshard);
}

static int shard_unpack(nnlm_handle *h, const Side &s)
{
    ProfScope ps(h, P_UNPACK);
    const int which = s.which;
    const ShardCols sc = shard_cols(h, s.ncols);
    const int f64 = (h->prec == NNLM_PREC_F64) ? 1 : 0;
    unsigned *maxw = h->x16 ? h->maxbits + 6 + which : nullptr; // max|factor| for the next half-step's split copy (no absmax pass there)
    // dense SCD in the column form (pack_tail = KP * KP Gram partial sums + the rank's max|x|): max|factor| is known before an entry is
    // read, so the unpack writes the split-fp16 copy of the factor -- the fixed factor of the NEXT half-step -- and its exponent too
    const bool tail_max = h->pack_tail != 0 && h->x16;
    const size_t tail_max_off = tail_max ? (size_t)h->k * sc.cpr + (size_t)h->KP * h->KP : (size_t)-1;
    uint32_t *y16 = (tail_max && !generic_rank(h)) ? h->Y16 : nullptr;
    const int rows = y16 ? h->KP : h->k; // (the k meaningful rows of every rank's [KP][cpr] slab travel, not the padding; the split copy is zero padded)
    const size_t tot = (size_t)h->nranks * rows * sc.cpr;
    if (maxw && !tail_max) HIPCHK(h, hipMemsetAsync(maxw, 0, sizeof(unsigned), h->stream));
    h->upk_max_for = maxw ? which : -1;
    const size_t rank_stride = (size_t)h->k * sc.cpr + h->pack_tail;
    shard_unpack_kernel<<<(unsigned)((tot + 255) / 256), 256, 0, h->stream>>>(h->pack_all, h->nranks, rows, sc.cpr, h->k, s.ncols, s.Xout, s.ldc, s.op,
                                                                               s.op_mode, s.op_ld, f64, maxw, rank_stride, tail_max_off, y16, s.ldc,
                                                                               h->scal_exp + 1);
    h->y16_for = y16 ? which : -1;
    if (h->gshard_for == which) h->gshard_for = -1; // (that factor has just been rewritten)
    if (h->pack_tail) { // the Gram of the factor just gathered = the sum of the ranks' partial sums, in rank order
        const int cnt = h->KP * h->KP;
        shard_gram_sum_kernel<<<(cnt + 255) / 256, 256, 0, h->stream>>>(h->pack_all, h->nranks, rank_stride, (size_t)h->k * sc.cpr, cnt, h->Graw);
        h->gshard_for = which;
    }
    LAUNCHCHK(h);
    return NNLM_OK;
}

// packed slab [KP][cpr] this rank solves its columns into (zeroed) and the gathered [nranks][KP][cpr]
// tail: doubles that travel behind the slab's k meaningful rows (at offset k * cpr: the slab's padding rows are not gathered)
static int pack_prepare(nnlm_handle *h, int ncols, struct ShardCols *out, size_t tail)
{
    const ShardCols sc = shard_cols(h, ncols);
    const size_t need = (size_t)h->KP * sc.cpr + tail;
    if (h->pack_elems < need * h->nranks) {
        hipFree(h->pack_send);
        hipFree(h->pack_all);
        h->pack_send = h->pack_all = nullptr;
        h->pack_elems = 0;
        HIPCHK(h, hipMalloc(&h->pack_send, need * 8));
        HIPCHK(h, hipMalloc(&h->pack_all, need * h->nranks * 8));
        h->pack_elems = need * h->nranks;
        HIPCHK(h, hipMemsetAsync(h->pack_send, 0, need * 8, h->stream));
    } else if (sc.col1 <= sc.col0) // a rank without columns sends zeros (nothing below writes its slab or its tail)
        HIPCHK(h, hipMemsetAsync(h->pack_send, 0, need * 8, h->stream));
    // (otherwise no memset per half-step: the solvers write every live entry -- rows < k of the rank's columns --, the tail is written
    //  whole, and the unpack reads nothing else)
    *out = sc;
    return NNLM_OK;
}
// ONE ncclAllGather of the packed slabs, then every rank writes masters and GEMM operands of all columns
static int pack_gather_unpack(nnlm_handle *h, const Side &s, int phase)
{
    const ShardCols sc = shard_cols(h, s.ncols);
    if (h->comm) {
        ProfScope ps(h, P_ALLGATHER);
        ncclResult_t r = g_rccl.AllGather(h->pack_send, h->pack_all, (size_t)h->k * sc.cpr + h->pack_tail, ncclDouble, (ncclComm_t)h->comm,
                                          h->stream); // rows 0 .. k-1 (+ the Gram partial sums behind them)
        if (r != ncclSuccess) return fail(h, NNLM_ERR_COMM, "ncclAllGather failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    } else if (phase == PH_ALL)
        return fail(h, NNLM_ERR_COMM, "virtual rank %d of %d has no communicator: drive it with nnlm_debug_phase()", h->rank, h->nranks);
    return shard_unpack(h, s);
}

// 3. per-column solve (+ multi-GPU: all-gather of the solved column slabs and unpack into the resident layouts)
// colshard: the cross product was formed over the whole contraction for this rank's columns only (missing values: per-column
// Grams make the column the natural unit) -- its split-K slabs are read directly, nothing was all-reduced.
static int half_step_solve(nnlm_handle *h, const Side &s, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method,
                           int nslabs, bool speculative, int phase, bool colshard)
{
    h->cur_which = s.which;
    // dense SCD in the column form: the Gram partial sums of this rank's columns travel with its slab (shard_gram_sum_kernel)
    // (+ one double: the rank's max|x|, so that the unpack can write the split-fp16 copy of the factor as well)
    h->pack_tail = (h->sharded && colshard && method == 1 && !h->any_missing && !generic_rank(h)) ? (size_t)h->KP * h->KP + 1 : 0;
    if (phase != PH_C) {
        ProfScope ps(h, s.prof_sweep);
        SweepArgs a = sweep_args(h, s, reg, inner_max_iter, inner_rel_tol, sweep_counter(h, speculative));
        if (h->sharded && !colshard) a.Cx = h->red + (size_t)h->KP * h->KP; // (the all-reduced [G | C] buffer: one slab)
        else a.nslabs = nslabs;
        const bool sg = h->sg_request; // (only on the dense one-GPU split-fp16 path, where k_sweep_q.h runs)
        h->sg_request = false;
        if (sg) {
            a.maxbits = h->x16 ? h->maxbits + 4 + (h->sg_par ^ 1) : nullptr; // (max|x| is the split copy's scale: fp32-operand mode only)
            a.gram_slabs = h->sg_slabs;
        }
        if (h->sharded) { // sweep only this rank's columns into the packed slab; the unpack writes masters and operands
            ShardCols sc;
            int rcp = pack_prepare(h, s.ncols, &sc, h->pack_tail);
            if (rcp != NNLM_OK) return rcp;
            a.col0 = sc.col0;
            a.ncols = sc.col1;
            a.Xout = h->pack_send;
            a.ldo = sc.cpr;
            a.ocol0 = sc.col0;
            a.op = nullptr;
            a.op_mode = 0;
            if (h->pack_tail) {
                int rc = ensure_sg_slabs(h);
                if (rc != NNLM_OK) return rc;
                a.gram_slabs = h->sg_slabs; // (one slab per workgroup of sweep_scd_q_kernel; folded behind the packed slab below)
                a.maxbits = h->x16 ? h->maxbits + 8 : nullptr; // (the sweep's atomicMax; handed to the tail and cleared by gram_fold_tail_kernel)
            }
        }
        if (h->any_missing) {
            // per-column Gram over the finite rows of each column (src/update_with_missing.cpp:90), then the solver
            int rcg = launch_na_gram(h, s, a.col0, a.ncols);
            if (rcg != NNLM_OK) return rcg;
            a.Graw = h->Gcols;
            if (generic_rank(h)) {
                int rcs = launch_sweep_generic(h, method, a, (size_t)h->KP * h->KP);
                if (rcs != NNLM_OK) return rcs;
                h->na_solver[s.which] = 3, h->na_solver_kr[s.which] = h->k;
            } else
                launch_colsolve(h, method, a, (size_t)h->KP * h->KP);
        } else if (a.ncols > a.col0) {
            int rcs = launch_sweep(h, method, a);
            if (rcs != NNLM_OK) return rcs;
            if (h->sharded && h->pack_tail) {
                const int nsl = h->sweep_wgs; // (one slab per workgroup of the sweep launch)
                gram_fold_tail_kernel<<<h->KP * h->KP / 64, 1024, 0, h->stream>>>(h->sg_slabs, nsl, h->KP, h->pack_send + (size_t)h->k * a.ldo, h->maxbits + 8);
            }
            if (sg) { // the next half-step finds max and Gram partial sums of this factor
                h->sg_nslabs = h->sweep_wgs; // (one slab per workgroup of the sweep launch)
                h->sg_par ^= 1;
                h->sg_which = s.which;
                h->sg_other = h->sg_prev; // the word this sweep did not touch
            }
        }
        LAUNCHCHK(h);
        if (h->sharded && phase == PH_B) return NNLM_OK; // test hooks: the caller gathers the slabs
    }
    if (h->sharded) {
        int rc = pack_gather_unpack(h, s, phase);
        if (rc != NNLM_OK) return rc;
    }
    if (s.which == 0 && !speculative) swap_w(h);
    return NNLM_OK;
}

extern "C" int nnlm_half_step(nnlm_handle *h, int which, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method)
{
    if (which != 0 && which != 1) return fail(h, NNLM_ERR_ARG, "nnlm_half_step: which must be 0 (W) or 1 (H)");
    if (!reg) return fail(h, NNLM_ERR_ARG, "nnlm_half_step: reg is NULL");
    return half_step(h, which, reg, inner_max_iter, inner_rel_tol, method);
}

// Test hook: run the cross-product + Gram stage of a half-step for this (virtual) rank and return the partial
// [G (k x k) | C (k x cols)] sums, column-major, before any all-reduce and before the regularisation edits.
extern "C" int nnlm_debug_partial(nnlm_handle *h, int which, double *G_out, double *C_out)
{
    if (!h || !h->W64) return fail(h, NNLM_ERR_ARG, "nnlm_debug_partial: matrix and factors must be set first");
    if (h->sparse && h->sp_weighted) return weighted_refusal(h, "nnlm_debug_partial", "the partial-sum hook");
    if (h->sparse) return fail(h, NNLM_ERR_UNSUPPORTED, "nnlm_debug_partial: the handle holds a sparse matrix (the hook reads the dense split-K slabs)");
    if (which != 0 && which != 1) return fail(h, NNLM_ERR_ARG, "nnlm_debug_partial: which must be 0 or 1");
    const double z[3] = {0, 0, 0};
    // sharded handles return right after the slab fold; a 1-rank handle runs a zero-sweep solve (a no-op on the
    // factors) and its slabs are folded here
    int rc = half_step(h, which, z, 0, 0.0, 1, true);
    if (rc != NNLM_OK) return rc;
    const Side s = side_of(h, which);
    const int ld = s.ldc;
    if (!h->sharded) {
        const HalfPlan q = plan_half(h, which, 0, 1, h->fuse_err);
        const size_t cnt = s.slab_stride;
        slab_reduce_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>(h->Cx, q.S, cnt, h->red + (size_t)h->KP * h->KP);
    }
    sync_all(h);
    const int KP = h->KP, k = h->k;
    const int cols = s.ncols;
    std::vector<double> buf((size_t)KP * KP + (size_t)KP * ld);
    HIPCHK(h, hipMemcpy(buf.data(), h->red, buf.size() * 8, hipMemcpyDeviceToHost));
    if (G_out)
        for (int r = 0; r < k; r++)
            for (int q2 = 0; q2 < k; q2++) G_out[(size_t)r * k + q2] = buf[(size_t)q2 * KP + r];
    if (C_out)
        for (int c = 0; c < cols; c++)
            for (int q2 = 0; q2 < k; q2++) C_out[(size_t)c * k + q2] = buf[(size_t)KP * KP + (size_t)q2 * ld + c];
    return NNLM_OK;
}

// Test hooks for virtual ranks (several handles in one process, no communicator): run ONE phase of a sharded half-step
// (1 = PH_A, 2 = PH_B, 3 = PH_C) and let nnlm_debug_exchange() stand in for the collective between phases.
extern "C" int nnlm_debug_phase(nnlm_handle *h, int which, int phase, const double reg[3], unsigned inner_max_iter, double inner_rel_tol,
                                int method)
{
    if (!h || !reg || (which != 0 && which != 1) || phase < PH_A || phase > PH_C) return fail(h, NNLM_ERR_ARG, "nnlm_debug_phase: bad arguments");
    if (!h->sharded) return fail(h, NNLM_ERR_ARG, "nnlm_debug_phase: handle is not sharded (call nnlm_comm_init first)");
    // (nothing is reset here: nnlm_set_factors -- the only other writer of the factors -- invalidates what the last unpack left behind,
    //  so virtual ranks take the production path: cached Gram, max|factor| and split copy from the previous half-step's unpack)
    return half_step(h, which, reg, inner_max_iter, inner_rel_tol, method, false, false, phase);
}

// stage 1: what ncclAllReduce does to the [G | C] buffers (host sum in rank order); stage 2: what ncclAllGather does to the
// packed column slabs.  hs[r] must be the handle of virtual rank r; all handles describe the same problem.
extern "C" int nnlm_debug_exchange(nnlm_handle **hs, int P, int which, int stage)
{
    if (!hs || P < 1 || (which != 0 && which != 1) || (stage != 1 && stage != 2)) return fail(nullptr, NNLM_ERR_ARG, "nnlm_debug_exchange: bad arguments");
    nnlm_handle *h0 = hs[0];
    for (int r = 0; r < P; r++) {
        if (!hs[r] || hs[r]->nranks != P || hs[r]->rank != r) return fail(h0, NNLM_ERR_ARG, "nnlm_debug_exchange: hs[%d] is not virtual rank %d of %d", r, r, P);
        HIPCHK(hs[r], hipSetDevice(hs[r]->device));
        sync_all(hs[r]);
    }
    const Side s0 = side_of(h0, which);
    if (stage == 1) {
        const size_t cnt = (size_t)h0->KP * h0->KP + s0.slab_stride;
        std::vector<double> sum(cnt, 0.0), tmp(cnt);
        for (int r = 0; r < P; r++) {
            HIPCHK(hs[r], hipMemcpy(tmp.data(), hs[r]->red, cnt * 8, hipMemcpyDeviceToHost));
            for (size_t e = 0; e < cnt; e++) sum[e] += tmp[e];
        }
        for (int r = 0; r < P; r++) HIPCHK(hs[r], hipMemcpy(hs[r]->red, sum.data(), cnt * 8, hipMemcpyHostToDevice));
    } else {
        const ShardCols sc = shard_cols(h0, s0.ncols);
        const size_t per = (size_t)h0->k * sc.cpr + h0->pack_tail; // (as the ncclAllGather call: the first k rows of the slab + its tail)
        std::vector<double> all(per * P);
        for (int r = 0; r < P; r++) HIPCHK(hs[r], hipMemcpy(all.data() + per * r, hs[r]->pack_send, per * 8, hipMemcpyDeviceToHost));
        for (int r = 0; r < P; r++) HIPCHK(hs[r], hipMemcpy(hs[r]->pack_all, all.data(), per * P * 8, hipMemcpyHostToDevice));
    }
    return NNLM_OK;
}

extern "C" int nnlm_iterate(nnlm_handle *h, unsigned n_iter, const double alpha[3], const double beta[3], unsigned inner_max_iter,
                            double inner_rel_tol, int method)
{
    for (unsigned i = 0; i < n_iter; i++) {
        int rc = half_step(h, 0, alpha, inner_max_iter, inner_rel_tol, method); // update W, src/nnmf.cpp:131
        if (rc != NNLM_OK) return rc;
        rc = half_step(h, 1, beta, inner_max_iter, inner_rel_tol, method); // update H, src/nnmf.cpp:133
        if (rc != NNLM_OK) return rc;
    }
    return NNLM_OK;
}

extern "C" int nnlm_take_sweeps(nnlm_handle *h, long long *sweeps, int reset)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "nnlm_take_sweeps: handle is NULL");
    HIPCHK(h, hipSetDevice(h->device));
    unsigned long long v = 0;
    const unsigned long long *src = h->sweeps + h->sw_active;
    if (h->sharded && h->comm) {
        HIPCHK(h, hipMemcpyAsync(h->sweeps_tmp, src, sizeof v, hipMemcpyDeviceToDevice, h->stream));
        ncclResult_t r = g_rccl.AllReduce(h->sweeps_tmp, h->sweeps_tmp, 1, ncclUint64, ncclSum, (ncclComm_t)h->comm, h->stream);
        if (r != ncclSuccess) return fail(h, NNLM_ERR_COMM, "ncclAllReduce (sweep counter) failed");
        src = h->sweeps_tmp;
    }
    HIPCHK(h, hipMemcpyAsync(&v, src, sizeof v, hipMemcpyDeviceToHost, h->stream));
    if (reset) HIPCHK(h, hipMemsetAsync(h->sweeps + h->sw_active, 0, sizeof v, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (sweeps) *sweeps = (long long)v;
    return NNLM_OK;
}

extern "C" int nnlm_sync(nnlm_handle *h)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "nnlm_sync: handle is NULL");
    HIPCHK(h, hipSetDevice(h->device));
    sync_all(h);
    LAUNCHCHK(h);
    return NNLM_OK;
}

// ---------------------------------------------------------------------------------------------
// error block
// ---------------------------------------------------------------------------------------------
// Enqueue the error block on stream `st` for the CURRENT factors (pointers captured now); the 8 sums and, when
// `with_sweeps`, the active sweep counter land in the pinned host_res[0..8]; ev_err fires when they are there.
// fused_nb > 0: the two sums were left as fused_nb partial pairs in h->partials by the cross product of the speculative
// W half-step (xprod16_err_kernel); only their reduction, the penalties and the counters remain.
// need_pen: the six penalty sums of add_penalty() -- nnlm_run skips them when alpha = beta = 0 (penalties() then uses none of them)
static int errors_launch(nnlm_handle *h, hipStream_t st, bool with_sweeps, int fused_nb, bool need_pen)
{
    const int k4 = round_up_i(h->k, 4);
    if (fused_nb > 0) {
        HIPCHK(h, hipStreamWaitEvent(st, h->ev_xdone, 0)); // (ahead of the scope: the wait for the fused cross product is not this phase's time)
        ProfScope ps(h, P_ERR_REDUCE, st);
        reduce_partials_kernel<<<1, REDUCE_THREADS, 0, st>>>(h->partials, (size_t)fused_nb, 2, h->scal);
        if (h->sharded && h->comm) { // every rank's fused cross product covered ITS part of A: sum the two sums
            ncclResult_t r = g_rccl.AllReduce(h->scal, h->scal, 2, ncclDouble, ncclSum, (ncclComm_t)h->comm, st);
            if (r != ncclSuccess) return fail(h, NNLM_ERR_COMM, "ncclAllReduce (fused error sums) failed");
        }
    } else if (h->sparse) {
        // Sparse A: sums over the non-zeros (sp_errors_kernel), then the zeros' share from the Grams -- sum over all entries of (WH)^2 =
        // <W^T W, H H^T> -- and the sum of all entries of WH from the factors' sums (sp_err_final_kernel).  All reductions fp64, fixed order.
        ProfScope ps(h, P_SP_ERRORS, st);
        const int KP = h->KP, n = h->n, m = h->m;
        double *G = h->sp_eG, *sums = G + (size_t)2 * KP * KP, *S = sums + 2 * KP;
        // (absent entries missing, src/nnmf.cpp:124-125: the sums over the stored entries are the sums -- S1 and S3 + sum of wh)
        factor_rows_kernel<double><<<(n + 255) / 256, 256, 0, st>>>(h->W64, h->npad, n, KP, h->sp_Wrow);
        for (int f = 0; f < 2 && !h->sp_missing; f++) {
            const double *X = f == 0 ? h->W64 : h->H64;
            const int ld = f == 0 ? h->npad : h->mpad, cols = f == 0 ? n : m;
            const int nb = launch_gram_partial(h, X, ld, 0, cols, h->sp_eslabs, nullptr, st);
            gram_reduce_kernel<<<(KP * KP + 255) / 256, 256, 0, st>>>(h->sp_eslabs, nb, KP, G + (size_t)f * KP * KP);
            const int rb = (cols + 2047) / 2048;
            nnlm_tu_sp_rowsums(X, ld, cols, KP, h->sp_epart, rb, st);
            reduce_partials_kernel<<<1, REDUCE_THREADS, 0, st>>>(h->sp_epart, (size_t)rb, KP, sums + (size_t)f * KP);
        }
        const int nw = nnlm_sp_workers(h->nnz, KP, h->cus_device);
        long long chunk = (h->nnz + nw - 1) / nw;
        if (chunk < 1) chunk = 1;
        const int eb = (nw / (64 / nnlm_sp_lanes(KP)) + 3) / 4;
        if (h->sp_weighted) { // five weighted sums over the stored entries; the zeros of the zero semantics have weight 1 (k_sparse.h)
            nnlm_tu_sp_errors_weighted(h->sp_cptr, h->sp_ridx, h->sp_cval, h->sp_cwt, h->prec == NNLM_PREC_F64, m, h->nnz, chunk, nw, h->sp_Wrow, KP,
                                       h->k, h->H64, h->mpad, h->sp_epart, eb, st);
            reduce_partials_kernel<<<1, REDUCE_THREADS, 0, st>>>(h->sp_epart, (size_t)eb, 5, S);
            nnlm_tu_sp_err_final_weighted(S, G, G + (size_t)KP * KP, sums, sums + KP, h->k, KP, h->sp_missing, h->scal, st);
        } else {
            nnlm_tu_sp_errors(h->sp_cptr, h->sp_ridx, h->sp_cval, h->prec == NNLM_PREC_F64, m, h->nnz, chunk, nw, h->sp_Wrow, KP, h->k, h->H64,
                              h->mpad, h->sp_epart, eb, h->sp_missing, st);
            reduce_partials_kernel<<<1, REDUCE_THREADS, 0, st>>>(h->sp_epart, (size_t)eb, 3, S);
            if (h->sp_missing) nnlm_tu_sp_err_final_missing(S, h->scal, st);
            else nnlm_tu_sp_err_final(S, G, G + (size_t)KP * KP, sums, sums + KP, h->k, KP, h->scal, st);
        }
    } else {
        ProfScope ps(h, P_ERRORS, st);
        const uint32_t *miss = h->any_missing ? h->miss : nullptr;
        size_t nb;
        // multi-GPU: each rank reduces its share of the j-tiles; the two sums are all-reduced below
        const bool err_generic = generic_rank(h) && h->prec == NNLM_PREC_F32; // rank > 64: the LDS-free kernel with fp32 A
        const int tile = (h->prec == NNLM_PREC_F64 || err_generic) ? ERR_TILE : ERRF_TILE;
        const int tj = h->mpad / tile, per = (tj + h->nranks - 1) / h->nranks;
        const int jt0 = h->sharded ? (h->rank * per < tj ? h->rank * per : tj) : 0;
        const int jcnt = h->sharded ? ((jt0 + per < tj ? jt0 + per : tj) - jt0) : tj;
        if (jcnt <= 0) {
            nb = 0;
        } else if (h->prec == NNLM_PREC_F64 && !generic_rank(h)) {
            // one 64-row i-tile x a chunk of j-tiles per block; ~8 rounds of the 2 x 256 resident blocks
            const int nit = h->npad / ERR_TILE;
            int nchunks = (8 * 512 + nit / 2) / nit;
            if (nchunks < 1) nchunks = 1;
            if (nchunks > jcnt) nchunks = jcnt;
            const int chunk = (jcnt + nchunks - 1) / nchunks;
            nchunks = (jcnt + chunk - 1) / chunk;
            nb = (size_t)nit * nchunks;
            const int lds = errors64_lds_bytes(k4);
            if (miss) {
                set_dyn_lds((const void *)errors64_kernel<true>, lds, "errors64_kernel");
                errors64_kernel<true><<<(unsigned)nb, ERR64_THREADS, lds, st>>>((const double *)h->A, h->npad, miss, h->W64, h->npad, h->H64, h->mpad, h->n,
                                                                                h->m, k4, h->partials, jt0, jcnt, chunk, nit);
            } else {
                set_dyn_lds((const void *)errors64_kernel<false>, lds, "errors64_kernel");
                errors64_kernel<false><<<(unsigned)nb, ERR64_THREADS, lds, st>>>((const double *)h->A, h->npad, nullptr, h->W64, h->npad, h->H64, h->mpad,
                                                                                 h->n, h->m, k4, h->partials, jt0, jcnt, chunk, nit);
            }
        } else if (h->prec == NNLM_PREC_F64) {
            dim3 grid(h->npad / ERR_TILE, jcnt);
            nb = (size_t)grid.x * grid.y;
            errors_kernel<double><<<grid, 256, 0, st>>>((const double *)h->A, h->npad, miss, h->W64, h->npad, h->H64, h->mpad, h->n, h->m, k4, h->partials, jt0);
        } else if (err_generic) {
            dim3 grid(h->npad / ERR_TILE, jcnt);
            nb = (size_t)grid.x * grid.y;
            errors_kernel<float><<<grid, 256, 0, st>>>((const float *)h->A, h->npad, miss, h->W64, h->npad, h->H64, h->mpad, h->n, h->m, k4, h->partials, jt0);
        } else {
            const int nx = h->npad / ERRF_TILE;
            const unsigned grid = 8u * ((nx + 7) / 8) * jcnt; // (XCD-aware numbering: k_errors.h)
            nb = (size_t)nx * jcnt;
            const int k2 = round_up_i(h->k, 2);
            const int lds = 2 * k2 * ERRF_TILE * (int)sizeof(float);
            const size_t cnt = (size_t)h->KP * h->mpad;
            factor_to_f32_kernel<<<(unsigned)((cnt + 255) / 256), 256, 0, st>>>(h->H64, cnt, h->Hkq);
            if (h->any_missing) {
                set_dyn_lds((const void *)errors_f32_kernel<true>, lds, "errors_f32_kernel");
                errors_f32_kernel<true><<<grid, 256, lds, st>>>((const float *)h->A, h->npad, h->missT, h->mpad / 32, (const float *)h->Wop, h->npad, h->Hkq,
                                                                h->mpad, h->n, h->m, k2, h->partials, jt0, nx);
            } else {
                set_dyn_lds((const void *)errors_f32_kernel<false>, lds, "errors_f32_kernel");
                errors_f32_kernel<false><<<grid, 256, lds, st>>>((const float *)h->A, h->npad, nullptr, 0, (const float *)h->Wop, h->npad, h->Hkq, h->mpad,
                                                                 h->n, h->m, k2, h->partials, jt0, nx);
            }
        }
        reduce_partials_kernel<<<1, REDUCE_THREADS, 0, st>>>(h->partials, nb, 2, h->scal);
        if (h->sharded && h->comm) {
            ncclResult_t r = g_rccl.AllReduce(h->scal, h->scal, 2, ncclDouble, ncclSum, (ncclComm_t)h->comm, st);
            if (r != ncclSuccess) return fail(h, NNLM_ERR_COMM, "ncclAllReduce (error sums) failed");
        }
    }
    if (need_pen) {
        const int nbw = (h->n + 255) / 256, nbh = (h->m + 255) / 256;
        penalty_kernel<<<nbw, 256, 0, st>>>(h->W64, h->npad, h->n, h->k, h->partials);
        reduce_partials_kernel<<<1, REDUCE_THREADS, 0, st>>>(h->partials, (size_t)nbw, 3, h->scal + 2);
        penalty_kernel<<<nbh, 256, 0, st>>>(h->H64, h->mpad, h->m, h->k, h->partials);
        reduce_partials_kernel<<<1, REDUCE_THREADS, 0, st>>>(h->partials, (size_t)nbh, 3, h->scal + 5);
    } else // (not recomputed: the collector must never see sums of an earlier call -- penalties() and need_pen could drift apart)
        HIPCHK(h, hipMemsetAsync(h->scal + 2, 0, 6 * sizeof(double), st));
    HIPCHK(h, hipMemcpyAsync(h->host_res, h->scal, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (with_sweeps) {
        const unsigned long long *src = h->sweeps + h->sw_active;
        if (h->sharded && h->comm) { // every rank swept its own columns: sum the integer counters
            HIPCHK(h, hipMemcpyAsync(h->sweeps_tmp, src, sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
            ncclResult_t r = g_rccl.AllReduce(h->sweeps_tmp, h->sweeps_tmp, 1, ncclUint64, ncclSum, (ncclComm_t)h->comm, st);
            if (r != ncclSuccess) return fail(h, NNLM_ERR_COMM, "ncclAllReduce (sweep counter) failed");
            src = h->sweeps_tmp;
        }
        HIPCHK(h, hipMemcpyAsync(h->host_res + 8, src, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipMemsetAsync(h->sweeps + h->sw_active, 0, sizeof(unsigned long long), st));
    }
    HIPCHK(h, hipEventRecord(h->ev_err, st));
    LAUNCHCHK(h);
    return NNLM_OK;
}

static int errors_collect(nnlm_handle *h, double *mse, double *mkl_var, double pen[6], long long *raw_sweeps)
{
    HIPCHK(h, hipEventSynchronize(h->ev_err));
    if (mse) *mse = h->host_res[0] / h->n_non_missing;
    if (mkl_var) *mkl_var = h->host_res[1] / h->n_non_missing;
    if (pen)
        for (int i = 0; i < 6; i++) pen[i] = h->host_res[2 + i];
    if (raw_sweeps) {
        unsigned long long v;
        memcpy(&v, h->host_res + 8, sizeof v);
        *raw_sweeps = (long long)v;
    }
    return NNLM_OK;
}

extern "C" int nnlm_errors(nnlm_handle *h, double *mse, double *mkl_var, double pen[6])
{
    if (!has_matrix(h) || !h->W64) return fail(h, NNLM_ERR_ARG, "nnlm_errors: matrix and factors must be set first");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = errors_launch(h, h->stream, false, 0, true);
    if (rc != NNLM_OK) return rc;
    return errors_collect(h, mse, mkl_var, pen, nullptr);
}

// ---------------------------------------------------------------------------------------------
// profiling
// ---------------------------------------------------------------------------------------------
extern "C" int nnlm_profile_enable(nnlm_handle *h, int on)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "handle is NULL");
    prof_collect(h);
    h->prof = on != 0;
    return NNLM_OK;
}
extern "C" int nnlm_profile_reset(nnlm_handle *h)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "handle is NULL");
    prof_collect(h);
    for (int i = 0; i < P_COUNT; i++) {
        h->prof_ms[i] = 0;
        h->prof_n[i] = 0;
    }
    return NNLM_OK;
}
extern "C" int nnlm_profile_get(nnlm_handle *h, const char *name, double *total_ms, long long *launches)
{
    if (!h || !name) return fail(h, NNLM_ERR_ARG, "nnlm_profile_get: bad arguments");
    prof_collect(h);
    for (int i = 0; i < P_COUNT; i++)
        if (strcmp(name, kProfNames[i]) == 0) {
            if (total_ms) *total_ms = h->prof_ms[i];
            if (launches) *launches = h->prof_n[i];
            return NNLM_OK;
        }
    return fail(h, NNLM_ERR_ARG, "nnlm_profile_get: unknown kernel class '%s'", name);
}

// ---------------------------------------------------------------------------------------------
// multi-GPU: RCCL, loaded lazily (single-GPU runs never touch librccl)
// ---------------------------------------------------------------------------------------------
extern "C" int nnlm_comm_unique_id(char id[NNLM_COMM_ID_BYTES])
{
    static_assert(NNLM_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
    if (!id) return fail(nullptr, NNLM_ERR_ARG, "nnlm_comm_unique_id: id is NULL");
    int rc = rccl_load();
    if (rc != NNLM_OK) return rc;
    ncclUniqueId u;
    ncclResult_t r = g_rccl.GetUniqueId(&u);
    if (r != ncclSuccess) return fail(nullptr, NNLM_ERR_COMM, "ncclGetUniqueId failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    memcpy(id, u.internal, NNLM_COMM_ID_BYTES);
    return NNLM_OK;
}

// id == NULL: "virtual rank" -- the handle computes rank's slab of an nranks-way split and leaves the partial
// [G | C] buffer un-reduced (single-device tests of the shard arithmetic, see nnlm_debug_partial).
extern "C" int nnlm_comm_init(nnlm_handle *h, const char id[NNLM_COMM_ID_BYTES], int rank, int nranks)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "nnlm_comm_init: handle is NULL");
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(h, NNLM_ERR_ARG, "nnlm_comm_init: bad rank %d of %d", rank, nranks);
    if (h->sparse && h->sp_weighted) return weighted_refusal(h, "nnlm_comm_init", "a communicator (multi-GPU)");
    if (h->sparse && h->sp_kl)
        return fail(h, NNLM_ERR_UNSUPPORTED, "nnlm_comm_init: the handle holds a sparse matrix loaded for KL loss (nnlm_set_matrix_csc_kl); the sparse KL "
                                             "path is single-GPU only");
    if (h->sparse) return fail(h, NNLM_ERR_UNSUPPORTED, "nnlm_comm_init: the handle holds a sparse matrix; the sparse path is single-GPU only");
    if (h->holdout) return fail(h, NNLM_ERR_UNSUPPORTED, "nnlm_comm_init: the handle holds a matrix with a hold-out set; that path is single-GPU only");
    HIPCHK(h, hipSetDevice(h->device));
    if (h->comm) {
        g_rccl.CommDestroy((ncclComm_t)h->comm);
        h->comm = nullptr;
    }
    h->rank = rank;
    h->nranks = nranks;
    invalidate_factor_caches(h); // (what an unpack left behind belongs to the previous communicator's exchange)
    h->pack_tail = 0;
    h->sharded = nranks > 1 || (id != nullptr); // a real 1-rank communicator runs the sharded path on one GPU (tests)
    h->dense_cols = true;                        // NNLM_FORM_COLS; nnlm_comm_set_form chooses the all-reduce form
    if (!id) return NNLM_OK;
    int rc = rccl_load();
    if (rc != NNLM_OK) return rc;
    ncclUniqueId u;
    memcpy(u.internal, id, NNLM_COMM_ID_BYTES);
    ncclComm_t comm = nullptr;
    ncclResult_t r = g_rccl.CommInitRank(&comm, nranks, u, rank);
    if (r != ncclSuccess) return fail(h, NNLM_ERR_COMM, "ncclCommInitRank(rank %d of %d) failed: %s", rank, nranks, g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
    h->comm = comm;
    return NNLM_OK;
}

extern "C" int nnlm_comm_set_form(nnlm_handle *h, int form)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "nnlm_comm_set_form: handle is NULL");
    if (form != NNLM_FORM_COLS && form != NNLM_FORM_REDUCE) return fail(h, NNLM_ERR_ARG, "nnlm_comm_set_form: unknown form %d", form);
    if (h->dense_cols != (form == NNLM_FORM_COLS)) {
        HIPCHK(h, hipSetDevice(h->device));
        sync_all(h);
        invalidate_factor_caches(h); // (Gram, max and split copy an unpack left behind belong to the other form's exchange)
        h->pack_tail = 0;
        h->dense_cols = form == NNLM_FORM_COLS;
    }
    return NNLM_OK;
}

extern "C" int nnlm_get_info(nnlm_handle *h, const char *key, double *value)
{
    if (!h || !key || !value) return fail(h, NNLM_ERR_ARG, "nnlm_get_info: NULL argument");
    if (strcmp(key, "cus") == 0) *value = h->cus;
    else if (strcmp(key, "xprod_waves_w") == 0) *value = h->xp_waves[0]; // (xprod16_tn_kernel, last launch of each side; 0 = none yet)
    else if (strcmp(key, "xprod_waves_h") == 0) *value = h->xp_waves[1];
    else if (strcmp(key, "xprod_splits_w") == 0) *value = h->xp_splits[0];
    else if (strcmp(key, "xprod_splits_h") == 0) *value = h->xp_splits[1];
    else if (strcmp(key, "xprod_splits_err") == 0) *value = h->xp_err_splits; // (xprod16_err_kernel: the W half-step of a trace iteration)
    else if (strcmp(key, "a_stream_nt_from") == 0) *value = h->a_stream_last; // (last A-streaming cross product, any of the three kernels; -1 = none yet)
    else if (strcmp(key, "sweep_form_w") == 0) *value = h->sweep_form[0]; // (0 / 1 strict kernels, 2 k_sweep_f.h, 3 k_sweep_r.h)
    else if (strcmp(key, "sweep_form_h") == 0) *value = h->sweep_form[1];
    else if (strcmp(key, "sweep_groups_w") == 0) *value = h->sweep_groups[0];
    else if (strcmp(key, "sweep_groups_h") == 0) *value = h->sweep_groups[1];
    else if (strcmp(key, "lee_lanes_w") == 0) *value = h->lee_lanes[0]; // (sweep_ls_kernel<R, L, 2> of the last Lee half-step)
    else if (strcmp(key, "lee_lanes_h") == 0) *value = h->lee_lanes[1];
    else if (strcmp(key, "lee_regs_w") == 0) *value = h->lee_regs[0];
    else if (strcmp(key, "lee_regs_h") == 0) *value = h->lee_regs[1];
    else if (strcmp(key, "na_solver_w") == 0) *value = h->na_solver[0]; // (last launches with per-column Grams: see nnlm_handle::na_solver)
    else if (strcmp(key, "na_solver_h") == 0) *value = h->na_solver[1];
    else if (strcmp(key, "na_solver_kr_w") == 0) *value = h->na_solver_kr[0];
    else if (strcmp(key, "na_solver_kr_h") == 0) *value = h->na_solver_kr[1];
    else if (strcmp(key, "na_gram_w") == 0) *value = h->na_gram[0];
    else if (strcmp(key, "na_gram_h") == 0) *value = h->na_gram[1];
    else if (strcmp(key, "na_gram_nt_w") == 0) *value = h->na_gram_nt[0];
    else if (strcmp(key, "na_gram_nt_h") == 0) *value = h->na_gram_nt[1];
    else if (strcmp(key, "kl_form_w") == 0) *value = h->kl_form[0];
    else if (strcmp(key, "kl_form_h") == 0) *value = h->kl_form[1];
    else if (strcmp(key, "kl_pieces_w") == 0) *value = h->kl_pieces[0]; // (instantiated pieces per thread / columns per block of the last
    else if (strcmp(key, "kl_pieces_h") == 0) *value = h->kl_pieces[1]; //  kl_tile_kernel or kl_reg64_kernel launch; 0 streaming, -1 none yet)
    else if (strcmp(key, "kl_cols_w") == 0) *value = h->kl_cols[0];
    else if (strcmp(key, "kl_cols_h") == 0) *value = h->kl_cols[1];
    else if (strcmp(key, "matrix_nnz") == 0) *value = h->sparse ? (double)h->nnz : -1.0;
    else if (strcmp(key, "matrix_holdout") == 0) *value = h->holdout ? (double)h->ho_nnz : -1.0;
    else if (strcmp(key, "matrix_bytes") == 0) *value = matrix_bytes(h);
    else if (strcmp(key, "matrix_min_col_observed") == 0) return observed_min(h, 0, value);
    else if (strcmp(key, "matrix_min_row_observed") == 0) return observed_min(h, 1, value);
    else if (strcmp(key, "matrix_absent_missing") == 0) *value = (h->sparse && h->sp_missing) ? 1.0 : 0.0;
    else if (strcmp(key, "sparse_weighted") == 0) *value = (h->sparse && h->sp_weighted) ? 1.0 : 0.0;
    else if (strcmp(key, "sparse_kl") == 0) *value = (h->sparse && h->sp_kl) ? 1.0 : 0.0;
    else if (strcmp(key, "sparse_batch") == 0) *value = (h->sparse && h->sp_batch) ? 1.0 : 0.0;
    else if (strcmp(key, "sp_batch_waves") == 0) *value = h->sparse ? nnlm_spb_waves(h->nnz, h->cus) : 0;
    else if (strcmp(key, "sparse_kl_form_w") == 0) *value = h->spkl_form[0];
    else if (strcmp(key, "sparse_kl_form_h") == 0) *value = h->spkl_form[1];
    else if (strcmp(key, "sparse_kl_short_max") == 0) *value = nnlm_spkl_short_max();
    else if (strcmp(key, "sp_ingest_check_share") == 0) *value = nnlm_spi_check_share();
    else if (strcmp(key, "sp_ingest_sort_tile") == 0) *value = nnlm_spi_sort_tile();
    else if (strcmp(key, "debug_sparse_values_address") == 0) *value = (h->sparse && h->sp_cval) ? (double)(uintptr_t)h->sp_cval : -1.0;
    else if (strcmp(key, "sparse_kl_batch") == 0) *value = (h->sparse && h->sp_kl && h->sp_batch) ? 1.0 : 0.0;
    else if (strcmp(key, "sparse_kl_batch_form_w") == 0) *value = h->spklb_form[0];
    else if (strcmp(key, "sparse_kl_batch_form_h") == 0) *value = h->spklb_form[1];
    else if (strcmp(key, "sparse_kl_batch_group") == 0) *value = h->spklb_group;
    else if (strcmp(key, "sp_gram_chunks") == 0) *value = h->spg_chunks;
    else if (strcmp(key, "sp_gram_bytes") == 0) *value = (double)h->spg_buf_bytes;
    else if (strcmp(key, "sp_workers") == 0) *value = (h->sparse && h->KP > 0) ? nnlm_sp_workers(h->nnz, h->KP, h->cus_device) : 0;
    else if (strcmp(key, "sp_gram_workers") == 0) *value = h->spg_workers;
    else if (strcmp(key, "sp_gram_batch_pairs") == 0) *value = h->bspg_pairs;
    else if (strcmp(key, "topn_slices") == 0) *value = h->topn_slices;
    else if (strcmp(key, "topn_eval_lines") == 0) *value = (double)h->topn_eval_lines;
    else if (strcmp(key, "svd_width") == 0) *value = h->svd_l > 0 ? h->svd_l : -1;
    else if (strcmp(key, "svd_kept") == 0) *value = h->svd_l > 0 ? h->svd_kept : -1;
    else if (strcmp(key, "svd_ms_cross") == 0) *value = h->svd_ms[0];
    else if (strcmp(key, "svd_ms_gram") == 0) *value = h->svd_ms[1];
    else if (strcmp(key, "svd_ms_rotate") == 0) *value = h->svd_ms[2];
    else if (strcmp(key, "svd_ms_eig") == 0) *value = h->svd_ms[3];
    else if (strcmp(key, "svd_ms_wait") == 0) *value = h->svd_ms[4];
    else if (strcmp(key, "svd_ms_total") == 0) *value = h->svd_ms[5];
    else if (strcmp(key, "svd_ms_setup") == 0) *value = h->svd_ms[6];
    else if (strcmp(key, "svd_rotate_form") == 0) *value = h->svd_form;
    else return fail(h, NNLM_ERR_ARG, "nnlm_get_info: unknown key '%s'", key);
    return NNLM_OK;
}

extern "C" int nnlm_comm_info(nnlm_handle *h, int *rank, int *nranks)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "handle is NULL");
    if (rank) *rank = h->rank;
    if (nranks) *nranks = h->nranks;
    return NNLM_OK;
}

// Contraction range [begin, end) (in rows i of A for which = 1, columns j for which = 0) that rank `rank` of
// `nranks` owns.  Pure function of the sizes: the partition is stage-granular (a stage = 256 bytes of an A column for
// the TN kernel, 32 columns for the NT kernel), clipped to the true extent.
extern "C" int nnlm_shard_range(int n, int m, int precision, int which, int rank, int nranks, int *begin, int *end)
{
    if (n < 1 || m < 1 || nranks < 1 || rank < 0 || rank >= nranks || (which != 0 && which != 1) || !begin || !end)
        return fail(nullptr, NNLM_ERR_ARG, "nnlm_shard_range: bad arguments");
    nnlm_handle t;
    t.prec = precision;
    t.x16 = x16_enabled(precision);
    t.n = n;
    t.m = m;
    t.npad = round_up_i(n, NNLM_PAD_N);
    t.mpad = round_up_i(m, NNLM_PAD_M);
    const HalfPlan p = plan_half(&t, which, rank, nranks, false);
    const int CE = stage_elems(&t);
    const int lim = side_of(&t, which).p;
    int c0 = p.stage_begin * CE, c1 = p.stage_end * CE;
    if (c1 > lim) c1 = lim;
    if (c0 > c1) c0 = c1;
    *begin = c0;
    *end = c1;
    return NNLM_OK;
}

// The plan of one xprod16_tn_kernel launch over ldc output columns (a multiple of 128) and `stages` contraction stages at rank k on
// `cus` compute units, with `force_waves` as nnlm_debug_set_xprod_waves sets it.  Pure function; out[8] = wavefronts per block, slabs S,
// stages per slab, tiles, blocks, factor pieces per stage, LDS bytes of a block, 0.
extern "C" int nnlm_xprod_plan(int ldc, int stages, int k, int cus, int force_waves, int *out)
{
    if (ldc < 128 || ldc % 128 || stages < 1 || k < 1 || k > NNLM_KQ_MAX || cus < 1 || (force_waves != 0 && force_waves != 8 && force_waves != 10) || !out)
        return fail(nullptr, NNLM_ERR_ARG, "nnlm_xprod_plan: bad arguments");
    const XPlan x = xprod_plan(ldc, stages, k, cus, force_waves, true);
    out[0] = x.nwv, out[1] = x.S, out[2] = x.sps, out[3] = x.tiles_x, out[4] = x.tiles_x * x.S, out[5] = x.yp, out[6] = x.lds, out[7] = 0;
    return NNLM_OK;
}

// Which KL solver a half-step with a contraction of length p takes at rank k (mask_words: 64-bit mask words per column of the solved
// factor, 0 without a mask) when its matrix-sized workspaces fit -- the decisions of half_step_kl(), launch_kl_tile() and launch_kl64()
// from their own helpers.  Pure function; out[8] = kernel (0 kl_tile_kernel with two row buffers, 1 with one, 2 kl_reg64_kernel,
// 3 kl_stream_kernel), exact pieces per thread, instantiated pieces (reg64 rounds up), columns per block, dynamic LDS bytes, wavefronts of
// a block that own a last (instantiated) piece, 0, 0.
extern "C" int nnlm_kl_plan(int p, int k, int precision, int mask_words, int *out)
{
    if (p < 1 || k < 1 || (precision != NNLM_PREC_F32 && precision != NNLM_PREC_F64) || mask_words < 0 || !out)
        return fail(nullptr, NNLM_ERR_ARG, "nnlm_kl_plan: bad arguments");
    for (int i = 0; i < 8; i++) out[i] = 0;
    if (precision == NNLM_PREC_F32 && kl_tile_fits(p, k, mask_words)) {
        const int e = kl_tile_ept4(p), C = kl_tile_cols(e), nbuf = kl_tile_nbuf(e), P4 = kl_tile_p4(p);
        out[0] = nbuf == 2 ? 0 : 1, out[1] = out[2] = e, out[3] = C;
        out[4] = (int)kl_tile_lds_bytes(p, k, C, mask_words, nbuf);
        for (int w = 0; w < KLT_THREADS / 64; w++) out[5] += (e - 1) * KLT_THREADS + 64 * w < P4; // `last` of kl_tile_kernel
    } else if (precision == NNLM_PREC_F64 && k <= NNLM_KQ_MAX && kl64_fits(p, k)) {
        const int e = kl64_ept2(p), inst = kl64_inst(e), C = kl64_cols(inst), P2 = (p + 1) / 2;
        out[0] = 2, out[1] = e, out[2] = inst, out[3] = C;
        out[4] = (int)kl64_lds_bytes(inst, C, k);
        for (int w = 0; w < KL64_THREADS / 64; w++) out[5] += (inst - 1) * KL64_THREADS + 64 * w < P2; // chunks that hold data
    } else {
        out[0] = 3;
        out[4] = (k + 24) * 8; // (launch_kl_stream)
    }
    return NNLM_OK;
}

// Columns [col0, col1) of the factor being solved that `rank` of `nranks` sweeps, and the slab width cpr of the all-gather
// (every rank sends [k][cpr]).  Pure function of the sizes.
extern "C" int nnlm_shard_cols(int ncols, int rank, int nranks, int *cpr, int *col0, int *col1)
{
    if (ncols < 1 || nranks < 1 || rank < 0 || rank >= nranks || !cpr || !col0 || !col1) return fail(nullptr, NNLM_ERR_ARG, "nnlm_shard_cols: bad arguments");
    nnlm_handle t;
    t.rank = rank;
    t.nranks = nranks;
    const ShardCols sc = shard_cols(&t, ncols);
    *cpr = sc.cpr;
    *col0 = sc.col0;
    *col1 = sc.col1;
    return NNLM_OK;
}

// ---------------------------------------------------------------------------------------------
// one-shot drivers
// ---------------------------------------------------------------------------------------------
// Arithmetic mode of the one-shot entries (= what the R layer reaches through r_glue.c): the reference is fp64 throughout
// and its own testthat vectors are held at 1.5e-8, so the drop-in default is the strict fp64 mode; the fp32-operand mode
// (A in 4 bytes per element, split-fp16 cross products; what bench.py times on a resident handle) is an explicit opt-in:
// NNLM_PRECISION=f32.
static int env_precision()
{
    const char *e = getenv("NNLM_PRECISION");
    if (e && (strcmp(e, "f32") == 0 || strcmp(e, "fp32") == 0 || strcmp(e, "0") == 0)) return NNLM_PREC_F32;
    return NNLM_PREC_F64;
}
static int env_device()
{
    const char *e = getenv("NNLM_DEVICE");
    return e ? atoi(e) : 0;
}

struct Lcg {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    double next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) * (1.0 / 9007199254740992.0);
    }
};

static void cb_print(const nnlm_callbacks *cb, const char *fmt, ...)
{
    if (!cb || !cb->print) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    cb->print(cb->ctx, buf);
}

// add_penalty, src/nnmf.cpp:224-240 (same order of the six terms)
static double penalties(double terr, const double pen[6], double N, const double alpha[3], const double beta[3])
{
    if (alpha[0] != alpha[1]) terr += 0.5 * (alpha[0] - alpha[1]) * pen[0] / N;
    if (beta[0] != beta[1]) terr += 0.5 * (beta[0] - beta[1]) * pen[3] / N;
    if (alpha[1] != 0) terr += 0.5 * alpha[1] * pen[1] / N;
    if (beta[1] != 0) terr += 0.5 * beta[1] * pen[4] / N;
    if (alpha[2] != 0) terr += alpha[2] * pen[2] / N;
    if (beta[2] != 0) terr += beta[2] * pen[5] / N;
    return terr;
}

// What the alternating loops of nnlm_run (one model) and nnlm_run_batch (one per member) share of the reference's outer loop,
// src/nnmf.cpp:100-209: their arguments, the checks, the trace setup and the poll at the top of every iteration.
struct OuterLoop {
    nnlm_handle *h;
    const double *alpha, *beta;
    unsigned max_iter;
    double rel_tol;
    int verbose, show_warning, method;
    unsigned trace;
    double *mse_error, *mkl_error, *target_error, *average_epoch; // [models][cap]
    int *n_trace;
    unsigned *n_iteration;
    int *warned;
    const nnlm_callbacks *cb;
    unsigned cap = 0; // trace entries of one model
    bool need_pen = false;

    int check(const char *who) const
    {
        if (any_null(alpha, beta, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned))
            return fail(h, NNLM_ERR_ARG, "%s: NULL argument", who);
        if (method < 1 || method > 4) return fail(h, NNLM_ERR_ARG, "method must be 1..4 (got %d)", method);
        return NNLM_OK;
    }
    void start(unsigned models)
    {
        if (trace < 1) trace = 1; // src/nnmf.cpp:53
        cap = nnlm_trace_capacity(max_iter, trace);
        for (size_t e = 0; e < (size_t)models * cap; e++) mkl_error[e] = h->kl_const; // src/nnmf.cpp:70,73
        // the six penalty sums are read by penalties() only through these conditions (src/nnmf.cpp:224-240)
        need_pen = alpha[0] != alpha[1] || beta[0] != beta[1] || alpha[1] != 0 || beta[1] != 0 || alpha[2] != 0 || beta[2] != 0;
    }
    int poll(unsigned i) const
    {
        if (cb && cb->check_interrupt && cb->check_interrupt(cb->ctx)) { // src/nnmf.cpp:111
            sync_all(h);
            return fail(h, NNLM_ERR_INTERRUPT, "interrupted");
        }
        if (verbose == 1 && cb && cb->progress) cb->progress(cb->ctx, i + 1, max_iter); // src/nnmf.cpp:112
        return NNLM_OK;
    }
    bool closing_entry(unsigned i) const { return (unsigned)(i - 1) % trace != 0; } // src/nnmf.cpp:164 (unsigned arithmetic)
};

// The stopping rule of one model and its trace: entries base .. base + cap - 1 of the four arrays (src/nnmf.cpp:135-160, 208)
struct StopRule {
    int member;      // the batch member its verbose rows name; -1 in a solo run
    size_t base;
    double rel_err;  // rel_tol + 1 before the first entry
    double terr_last = 1e99;
    unsigned n = 0;  // entries booked
    bool running(const OuterLoop &L) const { return std::fabs(rel_err) > L.rel_tol; } // src/nnmf.cpp:109
    // mse, kl: the sums already divided by the non-missing entries of A; raw: the sweeps since the previous entry
    void book(const OuterLoop &L, unsigned it, double mse, double kl, const double pen[6], long long raw)
    {
        const size_t e = base + n++;
        L.mse_error[e] = mse;
        L.mkl_error[e] += kl;
        L.average_epoch[e] = (double)raw / (double)(L.h->n + L.h->m); // src/nnmf.cpp:145
        const double t = penalties((L.method < 3) ? 0.5 * mse : L.mkl_error[e], pen, L.h->n_non_missing, L.alpha, L.beta);
        L.target_error[e] = t;
        rel_err = 2 * (terr_last - t) / (terr_last + t + NNLM_TINY); // src/nnmf.cpp:153
        terr_last = t;
        if (L.verbose == 2) {
            char row[512];
            snprintf(row, sizeof row, "%10d | %10.4f | %10.4f | %10.4f | %10.g\n", it + 1, mse, L.mkl_error[e], t, rel_err);
            if (member < 0) cb_print(L.cb, "%s", row);
            else cb_print(L.cb, "%6d %s", member, row);
        }
    }
    void finish(const OuterLoop &L, unsigned n_iteration)
    {
        const size_t b = member < 0 ? 0 : member;
        L.n_trace[b] = (int)n;
        L.n_iteration[b] = n_iteration;
        L.warned[b] = (L.show_warning && rel_err > L.rel_tol) ? 1 : 0; // src/nnmf.cpp:208
        if (L.warned[b] && L.cb && L.cb->warning) L.cb->warning(L.cb->ctx, "Target tolerance not reached. Try a larger max.iter.");
    }
};

// The alternating loop of c_nnmf (reference src/nnmf.cpp:100-209) on a resident handle: matrix and factors are already in
// HBM.  Semantics are the reference's, iteration by iteration.  What is MI355X-specific is the schedule at a trace
// iteration: the error block runs on its own stream (HBM/MFMA bound) while the NEXT iteration's W half-step is enqueued
// speculatively on the main stream (its sweep is VALU/matrix-core bound and touches no HBM to speak of) into the second
// W buffer; when the host has the error block's result it either accepts the speculative half-step (swap buffers) or,
// if the stopping rule fired, drops it -- W_i is still intact in the first buffer.
extern "C" int nnlm_run(nnlm_handle *h, const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol, int verbose,
                        int show_warning, unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace,
                        double *mse_error, double *mkl_error, double *target_error, double *average_epoch, int *n_trace,
                        unsigned *n_iteration, int *warned, const nnlm_callbacks *cb)
{
    if (!has_matrix(h) || !h->W64) return fail(h, NNLM_ERR_ARG, "nnlm_run: matrix and factors must be set first");
    OuterLoop L{h, alpha, beta, max_iter, rel_tol, verbose, show_warning, method, trace, mse_error, mkl_error, target_error, average_epoch,
                n_trace, n_iteration, warned, cb};
    int rc = L.check("nnlm_run");
    if (rc != NNLM_OK) return rc;
    if (h->sparse && method >= 3 && h->sp_weighted) return weighted_refusal(h, "nnlm_run", "methods 3 and 4 (KL loss)");
    if (h->sparse && method >= 3 && !h->sp_kl)
        return fail(h, NNLM_ERR_UNSUPPORTED, "method %d (KL loss) is not available for a sparse matrix: use loss = 'mse' (methods 1, 2) or a dense matrix", method);
    if (h->sparse && method >= 3 && h->k > NNLM_KQ_MAX) return spkl_rank_refusal(h, "nnlm_run");
    HIPCHK(h, hipSetDevice(h->device));
#define CHK(x)                  \
    do {                        \
        rc = (x);               \
        if (rc != NNLM_OK) {    \
            g_last_error = h->err; \
            return rc;          \
        }                       \
    } while (0)

    L.start(1);
    if (verbose == 2) { // src/nnmf.cpp:100-104
        cb_print(cb, "\n%10s | %10s | %10s | %10s | %10s\n", "Iteration", "MSE", "MKL", "Target", "Rel. Err.");
        cb_print(cb, "--------------------------------------------------------------\n");
    }
    StopRule rule{-1, 0, rel_tol + 1};
    unsigned i = 0;

    // spec.pending: the W half-step of iteration i is already enqueued (speculatively).  Whatever way this function is left
    // with one pending (stopping rule, interrupt, a failed call), the guard drops it: W_i is untouched, the alternate sweep
    // counter is cleared and the "what the last sweep left behind" state forgets the dropped sweep.
    struct SpecDrop {
        nnlm_handle *h;
        bool pending = false;
        void drop()
        {
            if (!pending) return;
            h->sg_which = h->sg_other = -1;
            h->gshard_for = h->upk_max_for = h->y16_for = -1; // (multi-GPU: what the dropped half-step's unpack left behind describes a W that is not current)
            h->fuse_err = false;
            h->fused_nb = 0;
            hipMemsetAsync(sweep_counter(h, true), 0, sizeof(unsigned long long), h->stream);
            pending = false;
        }
        ~SpecDrop() { drop(); }
    } spec{h};
    for (; i < max_iter && rule.running(L); i++) { // src/nnmf.cpp:109
        CHK(L.poll(i));
        if (spec.pending) { // accept: its buffers and its sweep counter become the current ones
            swap_w(h);
            h->sw_active ^= 1;
            spec.pending = false;
        } else
            CHK(half_step(h, 0, alpha, inner_max_iter, inner_rel_tol, method)); // update W, src/nnmf.cpp:131
        CHK(half_step(h, 1, beta, inner_max_iter, inner_rel_tol, method));      // update H, src/nnmf.cpp:133
        if (i % L.trace == 0) {                                                 // src/nnmf.cpp:135-160
            HIPCHK(h, hipEventRecord(h->ev_hdone, h->stream));
            HIPCHK(h, hipStreamWaitEvent(h->stream_e, h->ev_hdone, 0));
            // (multi-GPU: the dense square-loss flows of the fp32-operand mode at rank <= 64 -- every rank's speculative cross product
            //  covers its own part of A, so the fused sums are a partition of the error sums; the accept / drop decision is a function
            //  of the all-reduced sums and therefore the same on every rank)
            const bool spec_sharded = h->sharded && h->x16 && !generic_rank(h) && !h->any_missing;
            h->err_launched = false;
            if (i + 1 < max_iter && (!h->sharded || spec_sharded) && method < 3) {
                // speculative W half-step of iteration i+1 (not made current: h->W64 still is W_i below).  The error block
                // (one more pass over A) starts together with it: since the cross product became HBM bound (k_xprod16.h) the
                // two streams of A share the bandwidth, but the error block is then finished before the latency-bound sweep
                // needs the CUs -- measured +2 % over holding it back until the cross product is done
                // Split-fp16 mode without missing values: that half-step's cross product streams A with H_i as its fixed
                // factor while W_i is still current, so it evaluates the error sums of (W_i, H_i) on the way
                // (xprod16_err_kernel) and no separate pass over A is needed.
                h->fuse_err = h->x16 && !generic_rank(h);
                h->fused_nb = 0;
                h->err_hook = h->sharded;
                h->err_need_pen = L.need_pen;
                rc = half_step(h, 0, alpha, inner_max_iter, inner_rel_tol, method, false, true);
                h->fuse_err = false;
                h->err_hook = false;
                if (rc != NNLM_OK) {
                    g_last_error = h->err;
                    return rc;
                }
                spec.pending = true;
                // Strict mode: errors64_kernel and the fp64 cross product both live on the fp64 matrix / vector pipe and serialise when they
                // share the chip (0.98 ms for the pair against 0.40 + 0.60).  The error block therefore starts when the speculative cross
                // product has finished streaming A -- beside the SWEEP, which is bound by dependent latency and leaves the pipe half idle.
                // (round 5, bench.py --precision f64: 1.506 against 1.516-1.526 ms per step; the cross product 0.40 instead of 0.69 ms, the error
                //  block 0.42 instead of 0.34)
                // (tried for the NA flow of the F32 mode too, scripts/gpu_r5_n.sh: the cross product 0.29 -> 0.16 ms, the Gram + solver kernels
                //  1.05 -> 1.21 beside errors_f32_kernel -- 2.277 against 2.268 ms per iteration: the work is conserved, not hidden)
                if (h->prec == NNLM_PREC_F64 && !h->fused_nb) HIPCHK(h, hipStreamWaitEvent(h->stream_e, h->ev_xdone, 0));
            } else
                h->fused_nb = 0;
            if (!h->err_launched) CHK(errors_launch(h, h->stream_e, true, h->fused_nb, L.need_pen)); // reads W_i, H_i and the active sweep counter (then zeroes it)
            h->err_launched = false;
            h->fused_nb = 0;
            // H (and the fp32 copy the error kernel reads) must not be rewritten before the error block is done
            HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_err, 0));
            double mse, kl, pen[6];
            long long raw = 0;
            CHK(errors_collect(h, &mse, &kl, pen, &raw));
            rule.book(L, i, mse, kl, pen, raw);
        }
    }
    spec.drop(); // the stopping rule fired: the speculative half-step (if any) is discarded, W_i is untouched
    if (L.closing_entry(i)) {
        double mse, kl, pen[6];
        long long raw = 0;
        CHK(errors_launch(h, h->stream, true, 0, L.need_pen)); // (error sums and the sweep counter in one round trip)
        CHK(errors_collect(h, &mse, &kl, pen, &raw));
        rule.book(L, i, mse, kl, pen, raw);
    }

    if (verbose == 2) { // src/nnmf.cpp:194-198
        cb_print(cb, "--------------------------------------------------------------\n");
        cb_print(cb, "%10s | %10s | %10s | %10s | %10s\n\n", "Iteration", "MSE", "MKL", "Target", "Rel. Err.");
    }
    sync_all(h);
    LAUNCHCHK(h);
    rule.finish(L, i);
    return NNLM_OK;
}

// ---------------------------------------------------------------------------------------------
// batched factorisation: B independent square-loss models of one dense matrix (or, DESIGN section 4.18, of a sparse
// one loaded by nnlm_set_matrix_csc_batch: the cross product is then sp_cross, the error block k_sparse_batch.h), ranks k_b with sum <= 64, stacked
// in the factor buffers.  Per half-step ONE cross product of A with the stacked fixed factor (rows off_b .. off_b + k_b - 1 of its
// slabs are member b's), then per active member the Gram of ITS rows of the fixed factor and the existing sweep on its row block of
// Cx / X (pointer offsets; every sweep kernel reads and writes rows q < a.k only).  Per trace iteration one errors_batch_kernel pass.
// ---------------------------------------------------------------------------------------------
static_assert(SPB_BATCH_MAX == BATCH_MAX, "sp_batch_errors_kernel keeps one LDS slot per member");
static int batch_refusal(nnlm_handle *h, const char *who)
{
    if (h->sparse && h->sp_weighted) return weighted_refusal(h, who, "the batched factorisation");
    if (h->sparse && h->sp_kl && !h->sp_batch)
        return fail(h, NNLM_ERR_UNSUPPORTED, "%s: a sparse matrix loaded for KL loss (nnlm_set_matrix_csc_kl) is not supported by the batched factorisation "
                                             "(dense A, square loss only)", who);
    // (the doors: a sparse matrix loaded by nnlm_set_matrix_csc_batch -- absent entries zeros, square loss --, by
    //  nnlm_set_matrix_csc_kl_batch -- the same with KL loss too -- or by nnlm_set_matrix_csc_missing_batch -- absent entries missing -- passes)
    if (h->sparse && !h->sp_batch)
        return fail(h, NNLM_ERR_UNSUPPORTED, "%s: a sparse matrix is not supported by the batched factorisation (dense A only)", who);
    if (h->any_missing && !h->holdout && !h->sparse) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: A has missing (NA, NaN or +-Inf) entries; the batched factorisation needs a finite A", who);
    if (h->sharded) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: the batched factorisation runs on one GPU (no communicator)", who);
    return NNLM_OK;
}

// The members' ranks: 1 <= B <= BATCH_MAX of them (need: what the message asks for), each >= 1 (NNLM_ERR_ARG); then the caller's own
// refusals (refuse()); then a sum of at most 64 (NNLM_ERR_UNSUPPORTED)
template <typename Refuse>
static int batch_ranks(nnlm_handle *h, const char *who, const char *need, unsigned B, const unsigned *k, Refuse refuse)
{
    if (B < 1 || B > BATCH_MAX || !k) return fail(h, NNLM_ERR_ARG, "%s: need 1 <= B <= %d %s (B = %u)", who, BATCH_MAX, need, B);
    long K = 0;
    for (unsigned b = 0; b < B; b++) {
        if (k[b] < 1) return fail(h, NNLM_ERR_ARG, "%s: rank of member %u must be >= 1", who, b);
        K += k[b];
    }
    const int rc = refuse();
    if (rc != NNLM_OK) return rc;
    if (K > NNLM_KQ_MAX) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: the ranks sum to %ld; a batch holds at most %d", who, K, NNLM_KQ_MAX);
    return NNLM_OK;
}

static int batch_setup(nnlm_handle *h, unsigned B, const unsigned *k, const std::vector<int> &off);

extern "C" int nnlm_set_factors_batch(nnlm_handle *h, unsigned B, const unsigned *k, const double *W, const double *H)
{
    if (!has_matrix(h)) return fail(h, NNLM_ERR_ARG, "nnlm_set_factors_batch: set the matrix first");
    int rc = batch_ranks(h, "nnlm_set_factors_batch", "members and their ranks", B, k, [&] { return batch_refusal(h, "nnlm_set_factors_batch"); });
    if (rc != NNLM_OK) return rc;
    const int m = h->m;
    std::vector<int> off(B + 1, 0);
    for (unsigned b = 0; b < B; b++) off[b + 1] = off[b] + (int)k[b];
    const int K = off[B];
    // H arrives as the members' k_b x m blocks one after another: the stacked K x m matrix, column-major
    std::vector<double> Hs;
    if (H) {
        Hs.assign((size_t)K * m, 0.0);
        size_t src = 0;
        for (unsigned b = 0; b < B; b++) {
            for (int j = 0; j < m; j++)
                for (unsigned q = 0; q < k[b]; q++) Hs[(size_t)j * K + off[b] + q] = H[src + (size_t)j * k[b] + q];
            src += (size_t)k[b] * m;
        }
    }
    // (W: the members' n x k_b blocks one after another ARE the stacked n x K matrix)
    rc = set_factors_impl(h, K, W, H ? Hs.data() : nullptr, nullptr, nullptr, 64);
    if (rc != NNLM_OK) return rc;
    return batch_setup(h, B, k, off);
}

// The batch's own state behind stacked factors of rank off[B] (set with 64 padding rows): the members' offsets and workspaces
static int batch_setup(nnlm_handle *h, unsigned B, const unsigned *k, const std::vector<int> &off)
{
    h->bB = (int)B;
    h->bk.assign(k, k + B);
    h->boff = off;
    const int nit = h->npad / 64, mt = (h->m + 63) / 64;
    const int nch = mt < 1 ? 1 : (mt < (1024 + nit - 1) / nit ? mt : (1024 + nit - 1) / nit);
    const size_t eparts = (size_t)2 * B * nit * nch, pparts = (size_t)3 * B * (((h->n > h->m ? h->n : h->m) + 255) / 256);
    h->bpart_elems = eparts > pparts ? eparts : pparts;
    HIPCHK(h, hipMalloc(&h->boff_dev, (B + 1) * sizeof(int)));
    HIPCHK(h, hipMemcpy(h->boff_dev, off.data(), (B + 1) * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(h, hipMalloc(&h->bG, (size_t)B * 64 * 64 * 8));
    HIPCHK(h, hipMalloc(&h->bsweeps, B * sizeof(unsigned long long)));
    HIPCHK(h, hipMemset(h->bsweeps, 0, B * sizeof(unsigned long long)));
    HIPCHK(h, hipMalloc(&h->bpart, h->bpart_elems * 8));
    HIPCHK(h, hipMalloc(&h->bres, (size_t)8 * B * 8));
    if (h->sparse) { // error block (k_sparse_batch.h): the row copy of H beside sp_Wrow, the partial sums of the kernel and their sums
        const size_t nblk = (size_t)(nnlm_spb_waves(h->nnz, h->cus) + 3) / 4;
        HIPCHK(h, hipMalloc(&h->bsp_Hrow, (size_t)h->mpad * h->KP * 8));
        HIPCHK(h, hipMalloc(&h->bsp_part, ((size_t)3 * B * nblk + 3 * B) * 8));
    }
    return NNLM_OK;
}

extern "C" int nnlm_get_factors_batch(nnlm_handle *h, double *W, double *H)
{
    if (!h || !h->bB) return fail(h, NNLM_ERR_ARG, "nnlm_get_factors_batch: no batch set");
    const int K = h->k, m = h->m;
    std::vector<double> Hs;
    if (H) Hs.resize((size_t)K * m);
    int rc = nnlm_get_factors(h, W, H ? Hs.data() : nullptr);
    if (rc != NNLM_OK || !H) return rc;
    size_t dst = 0;
    for (int b = 0; b < h->bB; b++) {
        const int kb = h->bk[b], o = h->boff[b];
        for (int j = 0; j < m; j++)
            for (int q = 0; q < kb; q++) H[dst + (size_t)j * kb + q] = Hs[(size_t)j * K + o + q];
        dst += (size_t)kb * m;
    }
    return NNLM_OK;
}

#include "host_svd.h"

// The tile pairs of sp_gram_batch_kernel (k_sparse_na_batch.h) for the active members of a stack: bit pi (upper pairs ta <= tb, ta-major,
// NT = KP / 16 tiles a side) is set when the 16 x 16 pair meets some active member's diagonal block [off_b, off_b + k_b)^2; *tiles: the
// coordinate tiles the set pairs touch
static unsigned spg_batch_pairs(int NT, const std::vector<int> &off, const std::vector<char> &act, unsigned *tiles)
{
    unsigned pairs = 0, tl = 0;
    int pi = 0;
    for (int ta = 0; ta < NT; ta++)
        for (int tb = ta; tb < NT; tb++, pi++)
            for (size_t b = 0; b + 1 < off.size(); b++) {
                if (!act[b]) continue;
                const int lo = off[b], hi = off[b + 1]; // both tiles must hold a coordinate of the member
                if (lo < 16 * ta + 16 && hi > 16 * ta && lo < 16 * tb + 16 && hi > 16 * tb) pairs |= 1u << pi, tl |= (1u << ta) | (1u << tb);
            }
    *tiles = tl;
    return pairs;
}

// Steps 2 and 3 of a batch half-step on a sparse A whose absent entries are missing, behind sp_cross at the stacked KP:
// chunk by chunk ONE sp_gram_batch_kernel launch (+ its fix-up) for the per-column Grams of all active members -- column c's slot holds
// the members' own padded Grams one after another (goff_b = sum of KP_b'^2 in front of member b) -- then per active member the per-column
// solver on its row block, exactly as half_step_sparse_missing launches it at rank k_b (Graw = the member's Gram inside the slot,
// g_stride = the slot).  The Gram workers follow h->cus (the test hook's count): the Grams do not depend on it.
static int batch_solve_sparse_missing(nnlm_handle *h, const Side &s, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method,
                                      const std::vector<char> &act)
{
    const int B = h->bB, o = s.which, KPs = h->KP, NT = h->NKQ;
    const size_t es = esize(h);
    std::vector<int> goff(B + 1, 0);
    for (int b = 0; b < B; b++) {
        const int kp = 16 * ((h->bk[b] + 15) / 16);
        goff[b + 1] = goff[b] + kp * kp;
    }
    const size_t slot = (size_t)goff[B];
    int rc = spg_prepare(h, o, slot);
    if (rc != NNLM_OK) return rc;
    SpGramBatchArgs g;
    g.g.ptr = s.sp_ptr;
    g.g.idx = s.sp_idx;
    g.g.Y = h->sp_Y;
    g.g.segoff = h->spg_segoff[o];
    g.g.G = h->spg_buf; // [chunk columns][slot], then the chunk's segment slots
    g.slot = slot;
    g.pairs = spg_batch_pairs(NT, h->boff, act, &g.tiles);
    for (int i = 0; i < 128; i++) g.tab[i] = i < 64 ? -1 : 0;
    for (int b = 0; b < B; b++) {
        if (!act[b]) continue;
        const int kp = 16 * ((h->bk[b] + 15) / 16), ob = h->boff[b];
        for (int i = ob; i < h->boff[b + 1]; i++) g.tab[i] = b, g.tab[64 + i] = goff[b] + (i - ob) * kp - ob;
    }
    h->bspg_pairs = __builtin_popcount(g.pairs);
    const std::vector<long long> &hp = h->spg_hptr[o];
    const int K = h->k, NKQ = h->NKQ, KP8 = h->KP8, MW = h->MW;
    int workers = 0;
    for (const SpgChunk &ch : h->spg_plan[o]) {
        {
            ProfScope ps(h, P_SP_GRAM);
            g.g.c0 = ch.c0;
            g.g.c1 = ch.c1;
            g.g.seg = h->spg_buf + (size_t)(ch.c1 - ch.c0) * slot;
            const long long nnz = hp[ch.c1] - hp[ch.c0];
            g.g.nworkers = nnlm_spg_workers(nnz, h->cus);
            workers += g.g.nworkers;
            g.g.chunk = (nnz + g.g.nworkers - 1) / g.g.nworkers;
            if (g.g.chunk < 1) g.g.chunk = 1;
            nnlm_tu_sp_gram_batch(g, NT, h->prec == NNLM_PREC_F64, h->stream);
            nnlm_tu_sp_gram_batch_fixup(g, h->spg_longc[o] + ch.l0, ch.l1 - ch.l0, KPs, h->stream);
        }
        ProfScope ps(h, s.prof_sweep);
        for (int b = 0; b < B; b++) {
            if (!act[b]) continue;
            const int kb = h->bk[b], ob = h->boff[b];
            h->k = kb, h->NKQ = (kb + 15) / 16, h->KP = 16 * h->NKQ, h->KP8 = round_up_i(kb, 8), h->MW = 1;
            SweepArgs a = sweep_args(h, s, reg, inner_max_iter, inner_rel_tol, h->bsweeps + b);
            a.Cx = h->Cx + (size_t)ob * s.ldc;
            a.X = s.X + (size_t)ob * s.ldc;
            a.Xout = s.Xout + (size_t)ob * s.ldc;
            if (s.op) a.op = (char *)s.op + (size_t)ob * s.op_ld * es;
            else a.op_mode = 0;
            a.col0 = ch.c0;
            a.ncols = ch.c1;
            a.Graw = h->spg_buf + goff[b]; // (column col's Gram of this member: + (col - gcol0) * slot)
            a.gcol0 = ch.c0;
            launch_colsolve(h, method, a, slot);
        }
        h->k = K, h->NKQ = NKQ, h->KP = KPs, h->KP8 = KP8, h->MW = MW;
    }
    h->spg_chunks = (int)h->spg_plan[o].size();
    h->spg_workers = workers;
    return NNLM_OK;
}

// KL half-step of every active member on a sparse A loaded by nnlm_set_matrix_csc_kl_batch (no SpMM, no Gram, no Cx):
// ONE row copy of the stacked fixed factor and ONE launch for the column sums of its K coordinates, then ONE sp_kl_batch_kernel launch
// over the short lines for all active members (k_sparse_kl_batch.h; larger ranks first, so that the members a wavefront interleaves have
// ranks close to each other -- a member's result does not depend on the order).  Lines beyond the short form stay per member:
// sp_kl_solve_long_kernel as half_step_sparse_kl launches it, on the member's offsets, one member after another on the stream, so the
// one state per stored entry (spkl_state) serves them all.
static int batch_half_step_sparse_kl(nnlm_handle *h, const Side &s, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method,
                                     const std::vector<char> &act)
{
    const int o = s.which, B = h->bB;
    const bool f64 = h->prec == NNLM_PREC_F64;
    const size_t es = esize(h);
    int rc = ensure_klsw(h);
    if (rc != NNLM_OK) return rc;
    if (h->spkl_nlong[o] > 0 && !h->spkl_state) HIPCHK(h, hipMalloc(&h->spkl_state, (size_t)h->nnz * es + 64));
    {
        ProfScope ps(h, P_SPKL_COPY);
        if (f64) factor_rows_kernel<double><<<(s.p + 255) / 256, 256, 0, h->stream>>>(s.Y, s.ldy, s.p, h->KP, (double *)h->sp_Y);
        else factor_rows_kernel<float><<<(s.p + 255) / 256, 256, 0, h->stream>>>(s.Y, s.ldy, s.p, h->KP, (float *)h->sp_Y);
        kl_sumw_kernel<<<h->k, 256, 0, h->stream>>>(s.Y, s.ldy, s.p, h->klsw);
    }
    SpKlBatchArgs ba;
    SpKlArgs &a = ba.a;
    a.ptr = s.sp_ptr; a.idx = s.sp_idx; a.val = s.sp_val;
    a.Y = h->sp_Y;
    a.KP = h->KP; a.ncols = s.ncols; a.k = h->k;
    a.X = s.X; a.Xout = s.Xout; a.ldx = s.ldc;
    a.sumw = h->klsw;
    a.r0 = reg[0]; a.r1 = reg[1]; a.r2 = reg[2];
    a.mask = nullptr; a.mw = 1; // (a batch has no masks)
    a.max_iter = inner_max_iter; a.rel_tol = inner_rel_tol;
    a.op = s.op; a.op_mode = s.op ? s.op_mode : 0; a.op_ld = s.op_ld;
    a.sweeps = nullptr;
    a.state = h->spkl_state;
    a.longc = h->spkl_longc[o];
    a.nlong = h->spkl_nlong[o];
    ba.sweeps = h->bsweeps;
    ba.nmem = 0;
    for (int b = 0; b < 64; b++) ba.mem[b] = ba.off[b] = ba.kb[b] = 0;
    for (int b = 0; b < B; b++) {
        ba.off[b] = (unsigned char)h->boff[b];
        ba.kb[b] = (unsigned char)h->bk[b];
        if (act[b]) ba.mem[ba.nmem++] = (unsigned char)b;
    }
    std::stable_sort(ba.mem, ba.mem + ba.nmem, [&](unsigned char x, unsigned char y) { return h->bk[x] > h->bk[y]; });
    int form = 0;
    {
        ProfScope ps(h, o == 1 ? P_SPKL_BATCH_H : P_SPKL_BATCH_W);
        if (h->spkl_nshort[o] > 0 && ba.nmem > 0) {
            nnlm_tu_sp_kl_batch(ba, method, f64, h->spklb_group, h->stream);
            form |= 1;
        }
        for (int b = 0; b < B && a.nlong > 0; b++) {
            if (!act[b]) continue;
            const int ob = h->boff[b];
            SpKlArgs m = a;
            m.Y = (const char *)a.Y + (size_t)ob * es; // (the member's coordinates of a row of the stacked copy; the row stride stays a.KP)
            m.k = h->bk[b];
            m.X = a.X + (size_t)ob * a.ldx;
            m.Xout = a.Xout + (size_t)ob * a.ldx;
            m.sumw = a.sumw + ob;
            if (a.op) m.op = (char *)a.op + (size_t)ob * a.op_ld * es;
            m.sweeps = h->bsweeps + b;
            nnlm_tu_sp_kl_long(m, method, f64, h->stream);
            form |= 2;
        }
    }
    h->spklb_form[o] = form;
    LAUNCHCHK(h);
    return NNLM_OK;
}

// One half-step of every active member (act[b] != 0).  W is solved in place (no speculation, so no second buffer): a frozen member's
// rows are never written.
static int batch_half_step(nnlm_handle *h, int which, const double reg[3], unsigned inner_max_iter, double inner_rel_tol, int method,
                           const std::vector<char> &act)
{
    g_attr_err = hipSuccess;
    Side s = side_of(h, which);
    if (which == 0) {
        s.Xout = const_cast<double *>(s.X);
        s.op = h->Wop;
    }
    h->sg_which = h->sg_other = -1;
    h->sg_request = false;
    h->fuse_err = false;
    h->cur_which = which;
    if (method >= 3) return batch_half_step_sparse_kl(h, s, reg, inner_max_iter, inner_rel_tol, method, act); // (nnlm_run_batch: that handle only)
    HalfPlan p = plan_half(h, which, 0, 1, h->fuse_err);
    if (h->sparse) p.S = 1; // (one slab: the SpMM has no split-K)
    // Hold-out handle with a non-empty set: A has missing entries, every column solves with a Gram of its own.  The
    // cross product below needs nothing new (A holds 0 at a missing entry); the NA workspaces: the row copy for the stacked KP (at least
    // any member's), ONE buffer of per-column Grams sized for the largest member -- the members run one after another on this stream
    const bool na = h->any_missing && !h->sparse;
    if (na) {
        int rcw = ensure_yrow(h);
        if (rcw != NNLM_OK) return rcw;
        if (!h->Gcols) {
            int kpm = 16;
            for (int b = 0; b < h->bB; b++) kpm = kpm > 16 * ((h->bk[b] + 15) / 16) ? kpm : 16 * ((h->bk[b] + 15) / 16);
            const size_t bytes = (size_t)(h->n > h->m ? h->n : h->m) * kpm * kpm * 8;
            HIPCHK(h, hipMalloc(&h->Gcols, bytes));
            HIPCHK(h, poison_new_gram(h->Gcols, bytes, h->stream));
        }
    }
    // 1. one cross product for all members: split-fp16 copy of the whole stacked factor (ONE scale, max over all members), then the
    //    A-streaming kernel exactly as a rank-K solo half-step launches it
    // Sparse A (nnlm_set_matrix_csc_batch): the SpMM at the stacked KP -- one walk over the CSC / CSR, every row of the fixed factor
    // gathered once at the stacked width; lane = coordinate, so a member's rows of the slab do not depend on its neighbours
    if (h->sparse) sp_cross(h, s);
    else if (h->x16) prepare_factor16(h, s);
    else if (which == 0) {
        int rca = ensure_AT(h);
        if (rca != NNLM_OK) return rca;
    }
    if (!h->sparse) {
        // (strict mode: always the whole-tile instantiation, never the VALU tail rows of launch_xprod_nkq -- every row of the slabs is then
        //  formed by the same MFMA sequence wherever its member sits, and a member's result does not depend on its neighbours)
        ProfScope ps(h, s.prof_xprod);
        if (h->x16) with_nkq(h->NKQ, [&](auto N) { launch_xprod16_m<N>(h, s, p); });
        else
            with_nkq(h->NKQ, [&](auto N) {
                launch_xprod_tn<double, N, 0>(h, (const double *)a_contig(h, s), s.ldy, s.Y, s.ldy, h->Cx, s.ldc, s.slab_stride, p);
            });
    }
    // Sparse A whose absent entries are missing (nnlm_set_matrix_csc_missing_batch) with something absent: every column solves with a Gram
    // over its stored rows.  (Every entry stored: the shared-Gram steps below, as the reference calls update().)
    if (h->sparse && h->sp_missing && h->any_missing) {
        const int rcm = batch_solve_sparse_missing(h, s, reg, inner_max_iter, inner_rel_tol, method, act);
        h->pack_ready = false;
        if (rcm != NNLM_OK) return rcm;
        LAUNCHCHK(h);
        return NNLM_OK;
    }
    // 2. + 3. per member: Gram of its own rows of the fixed factor, then its sweep -- launched as a solo rank-k_b half-step launches them
    const int K = h->k, NKQ = h->NKQ, KP = h->KP, KP8 = h->KP8, MW = h->MW;
    const size_t es = esize(h);
    int rc = NNLM_OK;
    for (int b = 0; b < h->bB && rc == NNLM_OK; b++) {
        if (!act[b]) continue;
        const int kb = h->bk[b], o = h->boff[b];
        h->k = kb, h->NKQ = (kb + 15) / 16, h->KP = 16 * h->NKQ, h->KP8 = round_up_i(kb, 8), h->MW = 1;
        double *G = h->bG + (size_t)b * 64 * 64;
        {
            ProfScope ps(h, P_GRAM);
            const int nb = launch_gram_partial(h, s.Y + (size_t)o * s.ldy, s.ldy, 0, s.p, h->gslabs, nullptr, h->stream);
            gram_fold_kernel<<<h->KP * h->KP / 64, 1024, 0, h->stream>>>(h->gslabs, nb, h->KP, G, SweepImg{});
        }
        // (the member's rows of the stacked slabs and factor; a batch has no masks)
        SweepArgs a = sweep_args(h, s, reg, inner_max_iter, inner_rel_tol, h->bsweeps + b);
        a.Graw = G;
        a.Cx = h->Cx + (size_t)o * s.ldc;
        a.nslabs = p.S;
        a.X = s.X + (size_t)o * s.ldc;
        a.Xout = s.Xout + (size_t)o * s.ldc;
        if (s.op) a.op = (char *)s.op + (size_t)o * s.op_ld * es;
        else a.op_mode = 0;
        h->pack_ready = false; // (strict mode: the sweep packs its operand image from this member's Gram)
        ProfScope ps(h, s.prof_sweep);
        if (na) {
            // as a solo rank-k_b missing-value half-step launches them (half_step_solve): the member's per-column Grams over the observed
            // rows from ITS rows of the fixed factor and ITS full Gram (complement form), then the column solver on its row block.
            // F32 mode: the split-fp16 row copy takes its scale from max|Y| over the member's own k_b rows (the stacked factor's scale
            // would cost a small member the bits its neighbours' magnitude takes, and make it depend on them)
            const double *Yb = s.Y + (size_t)o * s.ldy;
            unsigned *mw = h->maxbits + 11;
            if (h->x16) {
                if (hipMemsetAsync(mw, 0, sizeof(unsigned), h->stream) != hipSuccess) {
                    rc = fail(h, NNLM_ERR_HIP, "batch half-step: hipMemsetAsync failed");
                    break;
                }
                absmax_f64_kernel<<<(s.p + 255) / 256, 256, 0, h->stream>>>(Yb, s.ldy, s.p, kb, mw);
            }
            rc = launch_na_gram(h, s, 0, s.ncols, Yb, G, mw);
            if (rc != NNLM_OK) break;
            a.Graw = h->Gcols;
            a.nslabs = p.S;
            launch_colsolve(h, method, a, (size_t)h->KP * h->KP);
            continue;
        }
        rc = launch_sweep(h, method, a);
    }
    h->k = K, h->NKQ = NKQ, h->KP = KP, h->KP8 = KP8, h->MW = MW;
    h->pack_ready = false;
    if (rc != NNLM_OK) return rc;
    LAUNCHCHK(h);
    return NNLM_OK;
}

// Error block of every member with amask bit b set: res[2b], res[2b+1] = sum of squares / KL sum, res[2B + 3b ..] and res[5B + 3b ..]
// the W and H penalty sums (zeros when !need_pen), sw[b] = member b's sweep counter (then cleared).  Synchronises.
static int batch_errors(nnlm_handle *h, unsigned long long amask, bool need_pen, std::vector<double> &res, std::vector<long long> &sw)
{
    const int B = h->bB;
    hipStream_t st = h->stream;
    if (h->sparse) {
        // Sparse A (k_sparse_batch.h): fp64 row copies of the stacked W and H; ONE launch over the non-zeros for the three sums of every
        // member; the zeros' share from the Grams of the stacked factors (gram_partial_kernel at the stacked KP: an entry of the Gram is
        // a sum over the columns of the products of ITS two rows in a fixed order, so a member's diagonal block depends on neither its
        // position nor its neighbours) and one launch per factor for the sums of all coordinates; one kernel closes all members
        ProfScope ps(h, P_SP_BATCH_ERRORS, st);
        const int KP = h->KP, n = h->n, m = h->m;
        double *G = h->sp_eG, *sums = G + (size_t)2 * KP * KP;
        factor_rows_kernel<double><<<(n + 255) / 256, 256, 0, st>>>(h->W64, h->npad, n, KP, h->sp_Wrow);
        factor_rows_kernel<double><<<(m + 255) / 256, 256, 0, st>>>(h->H64, h->mpad, m, KP, h->bsp_Hrow);
        // (absent entries missing: the sums run over the stored entries only, nothing is owed for the others -- no Grams, no coordinate sums)
        for (int f = 0; f < 2 && !h->sp_missing; f++) {
            const double *X = f == 0 ? h->W64 : h->H64;
            const int ld = f == 0 ? h->npad : h->mpad, cols = f == 0 ? n : m;
            const int nb = launch_gram_partial(h, X, ld, 0, cols, h->sp_eslabs, nullptr, st);
            gram_reduce_kernel<<<(KP * KP + 255) / 256, 256, 0, st>>>(h->sp_eslabs, nb, KP, G + (size_t)f * KP * KP);
            const int rb = (cols + 2047) / 2048;
            nnlm_tu_sp_rowsums(X, ld, cols, KP, h->sp_epart, rb, st);
            reduce_partials_kernel<<<1, REDUCE_THREADS, 0, st>>>(h->sp_epart, (size_t)rb, KP, sums + (size_t)f * KP);
        }
        // (the split over the non-zeros: nnz and the CU count -- the test hook's, nnlm_debug_set_cus -- decide it, not B or KP)
        const int nwaves = nnlm_spb_waves(h->nnz, h->cus), nblk = (nwaves + 3) / 4;
        double *S = h->bsp_part + (size_t)3 * B * nblk;
        if (h->sp_missing)
            nnlm_tu_sp_batch_errors_missing(h->sp_cptr, h->sp_ridx, h->sp_cval, h->prec == NNLM_PREC_F64, m, h->nnz, nnlm_spb_chunk(h->nnz, nwaves),
                                            nwaves, h->sp_Wrow, h->bsp_Hrow, KP, h->boff_dev, B, amask, h->bsp_part, st);
        else
            nnlm_tu_sp_batch_errors(h->sp_cptr, h->sp_ridx, h->sp_cval, h->prec == NNLM_PREC_F64, m, h->nnz, nnlm_spb_chunk(h->nnz, nwaves), nwaves,
                                    h->sp_Wrow, h->bsp_Hrow, KP, h->boff_dev, B, amask, h->bsp_part, st);
        batch_reduce_kernel<<<3 * B, 256, 0, st>>>(h->bsp_part, nblk, S);
        if (h->sp_missing) nnlm_tu_sp_batch_final_missing(S, B, amask, h->bres, st);
        else nnlm_tu_sp_batch_final(S, G, G + (size_t)KP * KP, sums, sums + KP, h->boff_dev, B, KP, amask, h->bres, st);
    } else {
        ProfScope ps(h, P_BATCH_ERRORS, st);
        const int nit = h->npad / 64, mt = (h->m + 63) / 64;
        const int nch = mt < 1 ? 1 : (mt < (1024 + nit - 1) / nit ? mt : (1024 + nit - 1) / nit);
        const int nblk = nit * nch;
        dim3 grid(nit, nch);
        if (h->any_missing) { // (a hold-out handle: the entries with a set miss bit stay out of both sums)
            if (h->prec == NNLM_PREC_F64)
                errors_batch_kernel<double, true><<<grid, 256, 0, st>>>((const double *)h->A, h->npad, h->W64, h->npad, h->H64, h->mpad, h->n, h->m,
                                                                       h->boff_dev, B, amask, h->bpart, nblk, h->miss, h->npad / 32);
            else
                errors_batch_kernel<float, true><<<grid, 256, 0, st>>>((const float *)h->A, h->npad, h->W64, h->npad, h->H64, h->mpad, h->n, h->m,
                                                                      h->boff_dev, B, amask, h->bpart, nblk, h->miss, h->npad / 32);
        } else if (h->prec == NNLM_PREC_F64)
            errors_batch_kernel<double><<<grid, 256, 0, st>>>((const double *)h->A, h->npad, h->W64, h->npad, h->H64, h->mpad, h->n, h->m, h->boff_dev,
                                                             B, amask, h->bpart, nblk);
        else
            errors_batch_kernel<float><<<grid, 256, 0, st>>>((const float *)h->A, h->npad, h->W64, h->npad, h->H64, h->mpad, h->n, h->m, h->boff_dev,
                                                            B, amask, h->bpart, nblk);
        batch_reduce_kernel<<<2 * B, 256, 0, st>>>(h->bpart, nblk, h->bres);
    }
    if (need_pen) {
        ProfScope ps(h, P_BATCH_PEN, st);
        for (int f = 0; f < 2; f++) {
            const int cols = f == 0 ? h->n : h->m, nbx = (cols + 255) / 256;
            batch_penalty_kernel<<<dim3(nbx, B), 256, 0, st>>>(f == 0 ? h->W64 : h->H64, f == 0 ? h->npad : h->mpad, cols, h->boff_dev, h->bpart);
            batch_reduce_kernel<<<3 * B, 256, 0, st>>>(h->bpart, nbx, h->bres + (size_t)(2 + 3 * f) * B);
        }
    } else
        HIPCHK(h, hipMemsetAsync(h->bres + 2 * B, 0, (size_t)6 * B * 8, st));
    res.resize((size_t)8 * B);
    std::vector<unsigned long long> v(B);
    HIPCHK(h, hipMemcpyAsync(res.data(), h->bres, (size_t)8 * B * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(v.data(), h->bsweeps, B * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemsetAsync(h->bsweeps, 0, B * sizeof(unsigned long long), st));
    HIPCHK(h, hipStreamSynchronize(st));
    LAUNCHCHK(h);
    sw.assign(B, 0);
    for (int b = 0; b < B; b++) sw[b] = (long long)v[b];
    return NNLM_OK;
}

// The alternating loop of c_nnmf (src/nnmf.cpp:100-209) for every member at once.  Member b stops when ITS stopping rule fires (its own
// target error, src/nnmf.cpp:153); from then on its sweeps are skipped and its trace, n_iteration and warning stay what a solo run's are.
// Outputs: [B][capacity] traces (capacity = nnlm_trace_capacity(max_iter, trace)), [B] n_trace / n_iteration / warned.
extern "C" int nnlm_run_batch(nnlm_handle *h, const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol, int verbose,
                              int show_warning, unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace,
                              double *mse_error, double *mkl_error, double *target_error, double *average_epoch, int *n_trace,
                              unsigned *n_iteration, int *warned, const nnlm_callbacks *cb)
{
    if (!h || !h->bB) return fail(h, NNLM_ERR_ARG, "nnlm_run_batch: set the matrix and a batch of factors (nnlm_set_factors_batch) first");
    OuterLoop L{h, alpha, beta, max_iter, rel_tol, verbose, show_warning, method, trace, mse_error, mkl_error, target_error, average_epoch,
                n_trace, n_iteration, warned, cb};
    int rc = L.check("nnlm_run_batch");
    if (rc != NNLM_OK) return rc;
    // (KL loss: the handle of nnlm_set_matrix_csc_kl_batch alone)
    if (method >= 3 && !(h->sparse && h->sp_kl && h->sp_batch))
        return fail(h, NNLM_ERR_UNSUPPORTED, "nnlm_run_batch: method %d (KL loss) is not supported by the batched factorisation: square loss (methods 1, 2) only", method);
    rc = batch_refusal(h, "nnlm_run_batch");
    if (rc != NNLM_OK) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    sync_all(h);
    const int B = h->bB;
    L.start(B);
    std::vector<StopRule> rule;
    for (int b = 0; b < B; b++) rule.push_back(StopRule{b, (size_t)b * L.cap, rel_tol + 1});
    std::vector<unsigned> nit(B, 0);
    std::vector<char> act(B, 1);
    std::vector<double> res;
    std::vector<long long> sw;
    auto book = [&](int b, unsigned it) {
        double pen[6];
        for (int c = 0; c < 3; c++) pen[c] = res[2 * B + 3 * b + c], pen[3 + c] = res[5 * B + 3 * b + c];
        rule[b].book(L, it, res[2 * b] / h->n_non_missing, res[2 * b + 1] / h->n_non_missing, pen, sw[b]);
    };
    auto mask_of = [&](const std::vector<char> &f) {
        unsigned long long mk = 0;
        for (int b = 0; b < B; b++)
            if (f[b]) mk |= 1ull << b;
        return mk;
    };
    if (verbose == 2) {
        cb_print(cb, "\n%6s %10s | %10s | %10s | %10s | %10s\n", "Member", "Iteration", "MSE", "MKL", "Target", "Rel. Err.");
        cb_print(cb, "---------------------------------------------------------------------\n");
    }
    unsigned i = 0;
    for (; i < max_iter && mask_of(act); i++) {
        CHK(L.poll(i));
        CHK(batch_half_step(h, 0, alpha, inner_max_iter, inner_rel_tol, method, act)); // update W, src/nnmf.cpp:131
        CHK(batch_half_step(h, 1, beta, inner_max_iter, inner_rel_tol, method, act));  // update H, src/nnmf.cpp:133
        if (i % L.trace == 0) {
            CHK(batch_errors(h, mask_of(act), L.need_pen, res, sw));
            for (int b = 0; b < B; b++) {
                if (!act[b]) continue;
                book(b, i);
                if (!rule[b].running(L)) { // src/nnmf.cpp:109: this member's loop ends after iteration i
                    act[b] = 0;
                    nit[b] = i + 1;
                }
            }
        }
    }
    // members still running reached max_iter: the last trace entry of src/nnmf.cpp:164 (unsigned arithmetic)
    std::vector<char> last(B, 0);
    for (int b = 0; b < B; b++)
        if (act[b]) {
            nit[b] = i;
            last[b] = L.closing_entry(i);
        }
    if (mask_of(last)) {
        CHK(batch_errors(h, mask_of(last), L.need_pen, res, sw));
        for (int b = 0; b < B; b++)
            if (last[b]) book(b, i);
    }
    sync_all(h);
    LAUNCHCHK(h);
    for (int b = 0; b < B; b++) rule[b].finish(L, nit[b]);
    return NNLM_OK;
}

// Held-out errors of the current factors (include/nnlm_mi355x.h): mse[b], mkl[b] for the bB members of a batch, or [0] for solo factors.
// Row copies of W and H, holdout_errors_kernel over the held-out CSC, batch_reduce_kernel; workspaces live for the call.  Synchronises.
extern "C" int nnlm_holdout_errors(nnlm_handle *h, double *mse, double *mkl)
{
    if (!h || !h->holdout) return fail(h, NNLM_ERR_ARG, "nnlm_holdout_errors: the handle has no hold-out set (nnlm_set_matrix_holdout)");
    if (!h->W64 || !mse || !mkl) return fail(h, NNLM_ERR_ARG, "nnlm_holdout_errors: set the factors first; mse and mkl must not be NULL");
    HIPCHK(h, hipSetDevice(h->device));
    g_attr_err = hipSuccess;
    const int B = h->bB ? h->bB : 1, K = h->k, n = h->n, m = h->m;
    if (h->ho_nnz == 0) {
        for (int b = 0; b < B; b++) mse[b] = mkl[b] = std::nan("");
        sync_all(h);
        return NNLM_OK;
    }
    std::vector<int> off(B + 1, 0);
    if (h->bB) off = h->boff;
    else off[1] = K;
    const long long nnz = h->ho_nnz;
    long long nbx = (nnz + 1023) / 1024; // at least four entries per lane
    if (nbx > 2048) nbx = 2048;
    const long long chunk = (nnz + nbx - 1) / nbx;
    double *rows = nullptr, *part = nullptr;
    int *offd = nullptr;
    const size_t nrow = (size_t)(n + m) * K, npart = (size_t)2 * B * nbx;
    hipError_t e = hipMalloc(&rows, nrow * 8);
    if (e == hipSuccess) e = hipMalloc(&part, (npart + 2 * B) * 8);
    if (e == hipSuccess) e = hipMalloc(&offd, (B + 1) * sizeof(int));
    std::vector<double> out((size_t)2 * B);
    hipStream_t st = h->stream;
    if (e == hipSuccess) e = hipMemcpyAsync(offd, off.data(), (B + 1) * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        double *Wrow = rows, *Hrow = rows + (size_t)n * K;
        factor_rows_kernel<double><<<(n + 255) / 256, 256, 0, st>>>(h->W64, h->npad, n, K, Wrow);
        factor_rows_kernel<double><<<(m + 255) / 256, 256, 0, st>>>(h->H64, h->mpad, m, K, Hrow);
        dim3 grid((unsigned)nbx, B);
        if (h->prec == NNLM_PREC_F64)
            holdout_errors_kernel<double><<<grid, 256, 0, st>>>(h->ho_ridx, h->ho_cidx, (const double *)h->ho_val, nnz, chunk, Wrow, Hrow, K, offd, part);
        else
            holdout_errors_kernel<float><<<grid, 256, 0, st>>>(h->ho_ridx, h->ho_cidx, (const float *)h->ho_val, nnz, chunk, Wrow, Hrow, K, offd, part);
        batch_reduce_kernel<<<2 * B, 256, 0, st>>>(part, (int)nbx, part + npart);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out.data(), part + npart, (size_t)2 * B * 8, hipMemcpyDeviceToHost, st);
    }
    const hipError_t es = hipStreamSynchronize(st); // (before the workspaces go)
    if (e == hipSuccess) e = es;
    hipFree(rows);
    hipFree(part);
    hipFree(offd);
    if (e != hipSuccess) return fail(h, NNLM_ERR_HIP, "nnlm_holdout_errors failed: %s", hipGetErrorString(e));
    sync_all(h);
    for (int b = 0; b < B; b++) mse[b] = out[2 * b] / (double)nnz, mkl[b] = out[2 * b + 1] / (double)nnz;
    return NNLM_OK;
}

// ---------------------------------------------------------------------------------------------
// scores of the current factors without W H (k_topn.h)
// ---------------------------------------------------------------------------------------------
// Device buffers that live for one call
struct CallBufs {
    std::vector<void *> p;
    template <typename T> hipError_t get(T **out, size_t count)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, (count ? count : 1) * sizeof(T));
        if (e == hipSuccess) p.push_back(q);
        *out = (T *)q;
        return e;
    }
    ~CallBufs()
    {
        for (void *q : p) hipFree(q);
    }
};

// what both entries ask of the handle; fills K4 and the row copies Wrow [n][K4], Hrow [m][K4] (enqueued on the handle's stream)
static int score_prepare(nnlm_handle *h, const char *who, CallBufs &bufs, int &K4, double *&Wrow, double *&Hrow)
{
    if (!h) return fail(nullptr, NNLM_ERR_ARG, "%s: handle is NULL", who);
    if (h->bB) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: the handle holds the factors of a batch; scores are read from solo factors (nnlm_set_factors)", who);
    if (h->sharded || h->comm) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: the handle has a communicator; scores are read on one GPU", who);
    if (!has_matrix(h)) return fail(h, NNLM_ERR_ARG, "%s: no matrix set", who);
    if (!h->W64 || !h->H64) return fail(h, NNLM_ERR_ARG, "%s: no factors set", who);
    HIPCHK(h, hipSetDevice(h->device));
    g_attr_err = hipSuccess;
    K4 = 4 * ((h->k + 3) / 4);
    HIPCHK(h, bufs.get(&Wrow, (size_t)h->n * K4));
    HIPCHK(h, bufs.get(&Hrow, (size_t)h->m * K4));
    factor_rows_kernel<double><<<(h->n + 255) / 256, 256, 0, h->stream>>>(h->W64, h->npad, h->n, K4, Wrow, h->k);
    factor_rows_kernel<double><<<(h->m + 255) / 256, 256, 0, h->stream>>>(h->H64, h->mpad, h->m, K4, Hrow, h->k);
    HIPCHK(h, hipGetLastError());
    return NNLM_OK;
}

// a failure between the first launch and the end of the call: the stream is drained before the call's buffers go
static int score_fail(nnlm_handle *h, const char *who, hipError_t e)
{
    (void)hipStreamSynchronize(h->stream);
    return fail(h, NNLM_ERR_HIP, "%s failed: %s", who, hipGetErrorString(e));
}

extern "C" int nnlm_predict_entries(nnlm_handle *h, long long count, const int *rows, const int *cols, double *out)
{
    const char *who = "nnlm_predict_entries";
    if (h && count < 0) return fail(h, NNLM_ERR_ARG, "%s: count = %lld", who, count);
    if (h && count > 0 && (!rows || !cols || !out)) return fail(h, NNLM_ERR_ARG, "%s: rows, cols and out must not be NULL", who);
    if (h && has_matrix(h))
        for (long long e = 0; e < count; e++) {
            if (rows[e] < 0 || rows[e] >= h->n) return fail(h, NNLM_ERR_ARG, "%s: rows[%lld] = %d is out of range (n = %d)", who, e, rows[e], h->n);
            if (cols[e] < 0 || cols[e] >= h->m) return fail(h, NNLM_ERR_ARG, "%s: cols[%lld] = %d is out of range (m = %d)", who, e, cols[e], h->m);
        }
    CallBufs bufs;
    int K4 = 0;
    double *Wrow = nullptr, *Hrow = nullptr;
    if (const int rc = score_prepare(h, who, bufs, K4, Wrow, Hrow); rc != NNLM_OK) {
        if (h && h->stream) (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    hipStream_t st = h->stream;
    const long long CH = 1LL << 22; // entries per round: 64 MB of indices and results
    int *rd = nullptr, *cd = nullptr;
    double *od = nullptr;
    const size_t chn = (size_t)(count < CH ? count : CH);
    hipError_t e = bufs.get(&rd, chn);
    if (e == hipSuccess) e = bufs.get(&cd, chn);
    if (e == hipSuccess) e = bufs.get(&od, chn);
    for (long long e0 = 0; e0 < count && e == hipSuccess; e0 += CH) {
        const long long ne = count - e0 < CH ? count - e0 : CH;
        e = hipMemcpyAsync(rd, rows + e0, (size_t)ne * sizeof(int), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(cd, cols + e0, (size_t)ne * sizeof(int), hipMemcpyHostToDevice, st);
        if (e != hipSuccess) break;
        {
            ProfScope ps(h, P_PREDICT_ENTRIES);
            nnlm_tu_predict_entries(rd, cd, ne, Wrow, Hrow, K4, h->k, od, st);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(out + e0, od, (size_t)ne * 8, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st); // (the round's buffers are reused)
    }
    if (e != hipSuccess) return score_fail(h, who, e);
    sync_all(h);
    return NNLM_OK;
}

// candidate slices of a launch over `ngroups` groups of 16 lines: enough wavefronts to fill the device (8 per CU), slices of at least 1024
// candidates, at most one per lane of topn_merge_kernel; the slice length is a multiple of the 16-candidate tile
static void topn_slicing(int ngroups, int ncand, int cus, int &nslices, int &slice_len)
{
    const long long target = 8LL * (cus > 0 ? cus : 256);
    long long ns = (target + ngroups - 1) / ngroups;
    const long long most = ((long long)ncand + 1023) / 1024;
    if (ns > most) ns = most;
    if (ns > TOPN_MAX_SLICES) ns = TOPN_MAX_SLICES;
    if (ns < 1) ns = 1;
    slice_len = (int)((((long long)ncand + ns - 1) / ns + 15) / 16 * 16);
    nslices = (ncand + slice_len - 1) / slice_len;
}

// by, exclude, n_top, lines and the out arrays of nnlm_top_n and nnlm_top_n_eval (`outs`: what must not be NULL there)
static int topn_check_args(nnlm_handle *h, const char *who, int by, int n_top, const int *lines, long long n_lines, int exclude, bool have_outs,
                           const char *outs)
{
    if (by != 0 && by != 1) return fail(h, NNLM_ERR_ARG, "%s: by = %d (0: per column, 1: per row)", who, by);
    if (exclude != 0 && exclude != 1) return fail(h, NNLM_ERR_ARG, "%s: exclude = %d (0 or 1)", who, exclude);
    if (n_top < 1) return fail(h, NNLM_ERR_ARG, "%s: n_top = %d (1 .. %d)", who, n_top, TOPN_MAX);
    if (n_top > TOPN_MAX) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: n_top = %d, at most %d are selected", who, n_top, TOPN_MAX);
    if (lines && n_lines < 0) return fail(h, NNLM_ERR_ARG, "%s: n_lines = %lld", who, n_lines);
    if (!have_outs) return fail(h, NNLM_ERR_ARG, "%s: %s must not be NULL", who, outs);
    if (exclude && has_matrix(h) && !h->sparse)
        return fail(h, NNLM_ERR_UNSUPPORTED, "%s: exclude = 1 needs a sparse matrix on the handle (its stored entries are what is excluded)", who);
    if (lines && has_matrix(h)) {
        const int side = by == 0 ? h->m : h->n;
        for (long long l = 0; l < n_lines; l++)
            if (lines[l] < 0 || lines[l] >= side)
                return fail(h, NNLM_ERR_ARG, "%s: lines[%lld] = %d is out of range (%s = %d)", who, l, lines[l], by == 0 ? "m" : "n", side);
    }
    return NNLM_OK;
}

// The rounds of 16384 lines behind nnlm_top_n and nnlm_top_n_eval, after score_prepare: per round the lines go up, the candidates are
// sliced, topn_kernel and topn_merge_kernel leave the round's lists in id / sd [nl][n_top] (device), round(l0, nl, id, sd) enqueues what
// the entry does with them (a hipError_t), and the stream is drained before the next round reuses the buffers.
template <typename Round>
static int topn_rounds(nnlm_handle *h, const char *who, CallBufs &bufs, int K4, const double *Wrow, const double *Hrow, int by, int n_top,
                       const int *lines, long long n_lines, int exclude, Round round)
{
    hipStream_t st = h->stream;
    const long long L = lines ? n_lines : (by == 0 ? h->m : h->n);
    const int LCH = 16384; // lines per round (a multiple of the 64 lines of a full workgroup)
    TopnArgs a{};
    a.Crow = by == 0 ? Wrow : Hrow;
    a.Lrow = by == 0 ? Hrow : Wrow;
    a.ncand = by == 0 ? h->n : h->m;
    a.K4 = K4;
    a.ntop = n_top;
    a.cap = nnlm_topn_cap(n_top);
    if (exclude) {
        a.xptr = by == 0 ? h->sp_cptr : h->sp_rptr;
        a.xidx = by == 0 ? h->sp_ridx : h->sp_cidx;
    }
    const int nw = nnlm_topn_waves(n_top);
    size_t most_lists = 0; // partial lists of the largest round
    for (long long l0 = 0; l0 < L; l0 += LCH) {
        const int nl = (int)(L - l0 < LCH ? L - l0 : LCH);
        int ns, sl;
        topn_slicing((nl + 15) / 16, a.ncand, h->cus, ns, sl);
        if ((size_t)nl * ns > most_lists) most_lists = (size_t)nl * ns;
    }
    const size_t chl = (size_t)(L < LCH ? L : LCH);
    int *ld = nullptr, *id = nullptr;
    double *sd = nullptr;
    hipError_t e = bufs.get(&a.part_s, most_lists * n_top);
    if (e == hipSuccess) e = bufs.get(&a.part_i, most_lists * n_top);
    if (e == hipSuccess) e = bufs.get(&id, chl * n_top);
    if (e == hipSuccess) e = bufs.get(&sd, chl * n_top);
    if (e == hipSuccess && lines) e = bufs.get(&ld, chl);
    for (long long l0 = 0; l0 < L && e == hipSuccess; l0 += LCH) {
        const int nl = (int)(L - l0 < LCH ? L - l0 : LCH);
        a.line0 = (int)l0;
        a.nlines = nl;
        a.lines = nullptr;
        if (lines) {
            e = hipMemcpyAsync(ld, lines + l0, (size_t)nl * sizeof(int), hipMemcpyHostToDevice, st);
            if (e != hipSuccess) break;
            a.lines = ld;
        }
        topn_slicing((nl + 15) / 16, a.ncand, h->cus, a.nslices, a.slice_len);
        h->topn_slices = a.nslices;
        {
            ProfScope ps(h, P_TOPN);
            nnlm_tu_topn(a, nw, st);
        }
        {
            ProfScope ps(h, P_TOPN_MERGE);
            nnlm_tu_topn_merge(a, id, sd, st);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = round(l0, nl, (const int *)id, (const double *)sd);
        if (e == hipSuccess) e = hipStreamSynchronize(st); // (the round's buffers are reused)
    }
    if (e != hipSuccess) return score_fail(h, who, e);
    return NNLM_OK;
}

extern "C" int nnlm_top_n(nnlm_handle *h, int by, int n_top, const int *lines, long long n_lines, int exclude, int *idx_out, double *score_out)
{
    const char *who = "nnlm_top_n";
    if (h)
        if (const int rc = topn_check_args(h, who, by, n_top, lines, n_lines, exclude, idx_out && score_out, "idx_out and score_out"); rc != NNLM_OK)
            return rc;
    CallBufs bufs;
    int K4 = 0;
    double *Wrow = nullptr, *Hrow = nullptr;
    if (const int rc = score_prepare(h, who, bufs, K4, Wrow, Hrow); rc != NNLM_OK) {
        if (h && h->stream) (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    hipStream_t st = h->stream;
    const int rc = topn_rounds(h, who, bufs, K4, Wrow, Hrow, by, n_top, lines, n_lines, exclude, [&](long long l0, int nl, const int *id, const double *sd) {
        hipError_t e = hipMemcpyAsync(idx_out + (size_t)l0 * n_top, id, (size_t)nl * n_top * sizeof(int), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(score_out + (size_t)l0 * n_top, sd, (size_t)nl * n_top * 8, hipMemcpyDeviceToHost, st);
        return e;
    });
    if (rc != NNLM_OK) return rc;
    sync_all(h);
    return NNLM_OK;
}

// Ranking metrics of the top-n lists against held-out entries (k_topn.h): the lists never leave the device
extern "C" int nnlm_top_n_eval(nnlm_handle *h, int by, const int *cutoffs, int n_cut, const int *lines, long long n_lines, int exclude,
                               const long long *held_ptr, const int *held_idx, double *agg_out, long long *n_eval_out, double *line_out)
{
    const char *who = "nnlm_top_n_eval";
    int n_top = 1;
    if (h) {
        if (n_cut < 1 || n_cut > TOPN_EVAL_MAX_CUT) return fail(h, NNLM_ERR_ARG, "%s: n_cut = %d (1 .. %d cutoffs)", who, n_cut, TOPN_EVAL_MAX_CUT);
        if (!cutoffs) return fail(h, NNLM_ERR_ARG, "%s: cutoffs must not be NULL", who);
        for (int c = 0; c < n_cut; c++) {
            if (cutoffs[c] < 1) return fail(h, NNLM_ERR_ARG, "%s: cutoffs[%d] = %d (1 .. %d)", who, c, cutoffs[c], TOPN_MAX);
            if (cutoffs[c] > TOPN_MAX) return fail(h, NNLM_ERR_UNSUPPORTED, "%s: cutoffs[%d] = %d, at most %d are selected", who, c, cutoffs[c], TOPN_MAX);
            if (c > 0 && cutoffs[c] <= cutoffs[c - 1])
                return fail(h, NNLM_ERR_ARG, "%s: cutoffs[%d] = %d does not ascend (cutoffs[%d] = %d)", who, c, cutoffs[c], c - 1, cutoffs[c - 1]);
        }
        n_top = cutoffs[n_cut - 1];
        if (const int rc = topn_check_args(h, who, by, n_top, lines, n_lines, exclude, agg_out && n_eval_out, "agg_out and n_eval_out"); rc != NNLM_OK)
            return rc;
        if (!held_ptr) return fail(h, NNLM_ERR_ARG, "%s: held_ptr must not be NULL", who);
        if (has_matrix(h)) { // the pattern, in the orientation of `by`: canonical, as nnlm_set_matrix_csc checks a CSC
            const int side = by == 0 ? h->m : h->n, ncand = by == 0 ? h->n : h->m;
            const char *ln = by == 0 ? "column" : "row", *cn = by == 0 ? "row" : "column";
            if (held_ptr[0] != 0) return fail(h, NNLM_ERR_ARG, "%s: held_ptr[0] = %lld, must be 0", who, held_ptr[0]);
            for (int j = 0; j < side; j++)
                if (held_ptr[j + 1] < held_ptr[j]) return fail(h, NNLM_ERR_ARG, "%s: held_ptr decreases at %s %d", who, ln, j);
            if (held_ptr[side] > 0 && !held_idx) return fail(h, NNLM_ERR_ARG, "%s: held_idx is NULL with %lld held-out entries", who, held_ptr[side]);
            for (int j = 0; j < side; j++)
                for (long long e = held_ptr[j]; e < held_ptr[j + 1]; e++) {
                    const int i = held_idx[e];
                    if (i < 0 || i >= ncand)
                        return fail(h, NNLM_ERR_ARG, "%s: held-out %s index %d out of range at entry %lld (%s %d)", who, cn, i, e, ln, j);
                    if (e > held_ptr[j] && i <= held_idx[e - 1])
                        return fail(h, NNLM_ERR_ARG, "%s: held-out %s indices of %s %d are not strictly increasing (entry %lld)", who, cn, ln, j, e);
                }
        }
    }
    CallBufs bufs;
    int K4 = 0;
    double *Wrow = nullptr, *Hrow = nullptr;
    if (const int rc = score_prepare(h, who, bufs, K4, Wrow, Hrow); rc != NNLM_OK) {
        if (h && h->stream) (void)hipStreamSynchronize(h->stream);
        return rc;
    }
    hipStream_t st = h->stream;
    const long long L = lines ? n_lines : (by == 0 ? h->m : h->n);
    // the held-out entries of the listed lines by list position (all lines: the caller's arrays as they are)
    std::vector<long long> hp;
    std::vector<int> hi;
    const long long *hp_host = held_ptr;
    const int *hi_host = held_idx;
    if (lines) {
        hp.resize((size_t)L + 1);
        hp[0] = 0;
        for (long long l = 0; l < L; l++) hp[l + 1] = hp[l] + (held_ptr[lines[l] + 1] - held_ptr[lines[l]]);
        hi.resize((size_t)hp[L]);
        for (long long l = 0; l < L; l++)
            if (hp[l + 1] > hp[l]) memcpy(hi.data() + hp[l], held_idx + held_ptr[lines[l]], (size_t)(hp[l + 1] - hp[l]) * sizeof(int));
        hp_host = hp.data();
        hi_host = hi.data();
    }
    const long long hn = hp_host[L];
    long long n_eval = 0;
    for (long long l = 0; l < L; l++) n_eval += hp_host[l + 1] > hp_host[l] ? 1 : 0;
    double disc[TOPN_MAX], idcg[TOPN_MAX + 1];
    idcg[0] = 0.0;
    for (int p = 0; p < TOPN_MAX; p++) disc[p] = 1.0 / std::log2((double)p + 2.0), idcg[p + 1] = idcg[p] + disc[p];
    const int LCH = 16384, nv = 6 * n_cut + 1, rw = 2 + 3 * n_cut;
    const size_t chl = (size_t)(L < LCH ? L : LCH);
    TopnEvalArgs ea{};
    ea.ntop = n_top;
    ea.ncut = n_cut;
    for (int c = 0; c < n_cut; c++) ea.cut[c] = cutoffs[c];
    ea.pstride = LCH;
    long long *hpd = nullptr;
    int *hid = nullptr, *lall = nullptr;
    double *tab = nullptr, *acc = nullptr;
    unsigned long long *key = nullptr;
    hipError_t e = bufs.get(&hpd, (size_t)L + 1);
    if (e == hipSuccess) e = bufs.get(&hid, (size_t)hn);
    if (e == hipSuccess) e = bufs.get(&tab, (size_t)2 * TOPN_MAX + 1);
    if (e == hipSuccess) e = bufs.get(&acc, (size_t)nv);
    if (e == hipSuccess) e = bufs.get(&ea.part, (size_t)nv * LCH);
    if (e == hipSuccess && line_out) e = bufs.get(&ea.rec, chl * rw);
    if (e == hipSuccess) e = hipMemcpyAsync(hpd, hp_host, ((size_t)L + 1) * sizeof(long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && hn > 0) e = hipMemcpyAsync(hid, hi_host, (size_t)hn * sizeof(int), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tab, disc, sizeof(disc), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(tab + TOPN_MAX, idcg, sizeof(idcg), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(acc, 0, (size_t)nv * 8, st);
    ea.hidx = hid;
    ea.disc = tab;
    ea.idcg = tab + TOPN_MAX;
    if (e == hipSuccess && exclude && hn > 0) { // a held-out entry the matrix stores is never a candidate: refuse the first one
        unsigned long long none = ~0ull, got = ~0ull;
        e = bufs.get(&key, 1);
        if (e == hipSuccess && lines) e = bufs.get(&lall, (size_t)L);
        if (e == hipSuccess && lines) e = hipMemcpyAsync(lall, lines, (size_t)L * sizeof(int), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(key, &none, sizeof(none), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            ProfScope ps(h, P_TOPN_EVAL);
            nnlm_tu_topn_eval_overlap(lall, L, hpd, hid, by == 0 ? h->sp_cptr : h->sp_rptr, by == 0 ? h->sp_ridx : h->sp_cidx, key, st);
        }
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&got, key, sizeof(got), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e == hipSuccess && got != none) {
            const long long l = (long long)(got >> 32);
            const int c = (int)(got & 0xffffffffull), line = lines ? lines[l] : (int)l;
            return fail(h, NNLM_ERR_ARG, "%s: the held-out entry (row %d, column %d) of lines[%lld] is stored in the resident matrix; with exclude = 1 "
                        "it could never be listed", who, by == 0 ? c : line, by == 0 ? line : c, l);
        }
    }
    if (e != hipSuccess) return score_fail(h, who, e);
    const int rc = topn_rounds(h, who, bufs, K4, Wrow, Hrow, by, n_top, lines, n_lines, exclude, [&](long long l0, int nl, const int *id, const double *) {
        ea.idx = id;
        ea.nlines = nl;
        ea.hptr = hpd + l0;
        {
            ProfScope ps(h, P_TOPN_EVAL);
            nnlm_tu_topn_eval(ea, st);
            nnlm_tu_topn_eval_reduce(ea, acc, st);
        }
        hipError_t e2 = hipGetLastError();
        if (e2 == hipSuccess && line_out) e2 = hipMemcpyAsync(line_out + (size_t)l0 * rw, ea.rec, (size_t)nl * rw * 8, hipMemcpyDeviceToHost, st);
        return e2;
    });
    if (rc != NNLM_OK) return rc;
    double sums[6 * TOPN_EVAL_MAX_CUT + 1];
    e = hipMemcpyAsync(sums, acc, (size_t)nv * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return score_fail(h, who, e);
    sync_all(h);
    if ((long long)sums[nv - 1] != n_eval) return fail(h, NNLM_ERR_HIP, "%s: %lld lines were evaluated on the device, %lld have held-out entries", who, (long long)sums[nv - 1], n_eval);
    for (int v = 0; v < nv - 1; v++) agg_out[v] = n_eval > 0 ? sums[v] / (double)n_eval : std::nan("");
    *n_eval_out = n_eval;
    h->topn_eval_lines = n_eval;
    return NNLM_OK;
}

// The handle of a one-shot entry: created on NNLM_DEVICE in the NNLM_PRECISION mode and given the matrix (set_matrix(h)); destroyed
// when the entry returns
struct OneShot {
    nnlm_handle *h = nullptr;
    template <typename SetMatrix>
    int open(SetMatrix set_matrix)
    {
        const int rc = nnlm_create(&h, env_device(), env_precision());
        return rc != NNLM_OK ? rc : set_matrix(h);
    }
    ~OneShot() { nnlm_destroy(h); }
};

// default init of the c_nnmf one-shots, src/nnmf.cpp:82-98: 0.01 U(0,1) from cb->unif_rand or the built-in generator, member by member
// (ranks k[0 .. B-1]), W before H, W.randu(k, n) drawn column-major (row q of W fastest), masked entries (solo runs only) drawn and
// zeroed.  Only a factor the caller left NULL is drawn: *W / *H then point at the draw.
static void default_factors(const nnlm_callbacks *cb, int n, int m, unsigned B, const unsigned *k, const int *Wm, const int *Hm,
                            const double **W, const double **H, std::vector<double> &Wi, std::vector<double> &Hi)
{
    size_t K = 0;
    for (unsigned b = 0; b < B; b++) K += k[b];
    if (!*W) Wi.resize((size_t)n * K);
    if (!*H) Hi.resize(K * m);
    Lcg lcg;
    auto draw = [&]() { return (cb && cb->unif_rand) ? cb->unif_rand(cb->ctx) : lcg.next(); };
    for (size_t b = 0, wo = 0, ho = 0; b < B; wo += (size_t)n * k[b], ho += (size_t)k[b] * m, b++) {
        if (!*W)
            for (int i = 0; i < n; i++)
                for (unsigned q = 0; q < k[b]; q++) {
                    const double v = draw() * 0.01; // (Wm > 0 on the reference's unsigned matrix: any non-zero, NA_LOGICAL included)
                    Wi[wo + (size_t)q * n + i] = (Wm && Wm[(size_t)q * n + i] != 0) ? 0.0 : v;
                }
        if (!*H)
            for (size_t e = 0; e < (size_t)k[b] * m; e++) {
                const double v = draw() * 0.01;
                Hi[ho + e] = (Hm && Hm[e] != 0) ? 0.0 : v;
            }
    }
    if (!*W) *W = Wi.data();
    if (!*H) *H = Hi.data();
}

// create + set_matrix + set_factors_batch + run_batch + get_factors_batch.  W_init / H_init: the members' n x k_b / k_b x m blocks one
// after another, or NULL for the default 0.01 U(0,1) init of each member (drawn member by member, W before H, as c_nnmf draws it).
extern "C" int nnlm_c_nnmf_batch(const double *A, int n, int m, unsigned B, const unsigned *k, const double *W_init, const double *H_init,
                                 const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol, int n_threads, int verbose,
                                 int show_warning, unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace, double *W_out,
                                 double *H_out, double *mse_error, double *mkl_error, double *target_error, double *average_epoch, int *n_trace,
                                 unsigned *n_iteration, int *warned, const nnlm_callbacks *cb)
{
    (void)n_threads;
    if (any_null(A, k, alpha, beta, W_out, H_out, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned))
        return fail(nullptr, NNLM_ERR_ARG, "nnlm_c_nnmf_batch: NULL argument");
    int rc = batch_ranks(nullptr, "nnlm_c_nnmf_batch", "members", B, k, [&] {
        return (method >= 3 && method <= 4) ? fail(nullptr, NNLM_ERR_UNSUPPORTED, "nnlm_c_nnmf_batch: method %d (KL loss) is not supported by the batched factorisation: square loss (methods 1, 2) only", method)
                                            : NNLM_OK;
    });
    if (rc != NNLM_OK) return rc;
    OneShot os;
    rc = os.open([&](nnlm_handle *h) { return nnlm_set_matrix(h, A, n, m); });
    if (rc != NNLM_OK) return rc;
    nnlm_handle *h = os.h;
    std::vector<double> Wi, Hi;
    default_factors(cb, n, m, B, k, nullptr, nullptr, &W_init, &H_init, Wi, Hi);
    CHK(nnlm_set_factors_batch(h, B, k, W_init, H_init));
    CHK(nnlm_run_batch(h, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, mse_error,
                       mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb));
    CHK(nnlm_get_factors_batch(h, W_out, H_out));
    return NNLM_OK;
}

// nnlm_c_nnmf_batch on a sparse A (canonical CSC, absent entries zeros): the matrix goes through nnlm_set_matrix_csc_batch
extern "C" int nnlm_c_nnmf_csc_batch(int n, int m, const long long *colptr, const int *rowidx, const double *x, unsigned B, const unsigned *k,
                                     const double *W_init, const double *H_init, const double alpha[3], const double beta[3], unsigned max_iter,
                                     double rel_tol, int n_threads, int verbose, int show_warning, unsigned inner_max_iter, double inner_rel_tol,
                                     int method, unsigned trace, double *W_out, double *H_out, double *mse_error, double *mkl_error,
                                     double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration, int *warned,
                                     const nnlm_callbacks *cb)
{
    (void)n_threads;
    if (any_null(colptr, k, alpha, beta, W_out, H_out, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned))
        return fail(nullptr, NNLM_ERR_ARG, "nnlm_c_nnmf_csc_batch: NULL argument");
    int rc = batch_ranks(nullptr, "nnlm_c_nnmf_csc_batch", "members", B, k, [&] {
        return (method >= 3 && method <= 4) ? fail(nullptr, NNLM_ERR_UNSUPPORTED, "nnlm_c_nnmf_csc_batch: method %d (KL loss) is not supported by the batched factorisation: square loss (methods 1, 2) only", method)
                                            : NNLM_OK;
    });
    if (rc != NNLM_OK) return rc;
    OneShot os;
    rc = os.open([&](nnlm_handle *h) { return nnlm_set_matrix_csc_batch(h, n, m, colptr, rowidx, x); });
    if (rc != NNLM_OK) return rc;
    nnlm_handle *h = os.h;
    std::vector<double> Wi, Hi;
    default_factors(cb, n, m, B, k, nullptr, nullptr, &W_init, &H_init, Wi, Hi);
    CHK(nnlm_set_factors_batch(h, B, k, W_init, H_init));
    CHK(nnlm_run_batch(h, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, mse_error,
                       mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb));
    CHK(nnlm_get_factors_batch(h, W_out, H_out));
    return NNLM_OK;
}

// nnlm_c_nnmf_csc_batch through nnlm_set_matrix_csc_kl_batch: the same arguments, all four methods (KL loss: stored values >= 0)
extern "C" int nnlm_c_nnmf_csc_kl_batch(int n, int m, const long long *colptr, const int *rowidx, const double *x, unsigned B, const unsigned *k,
                                        const double *W_init, const double *H_init, const double alpha[3], const double beta[3], unsigned max_iter,
                                        double rel_tol, int n_threads, int verbose, int show_warning, unsigned inner_max_iter, double inner_rel_tol,
                                        int method, unsigned trace, double *W_out, double *H_out, double *mse_error, double *mkl_error,
                                        double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration, int *warned,
                                        const nnlm_callbacks *cb)
{
    (void)n_threads;
    if (any_null(colptr, k, alpha, beta, W_out, H_out, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned))
        return fail(nullptr, NNLM_ERR_ARG, "nnlm_c_nnmf_csc_kl_batch: NULL argument");
    int rc = batch_ranks(nullptr, "nnlm_c_nnmf_csc_kl_batch", "members", B, k, [&] { return NNLM_OK; });
    if (rc != NNLM_OK) return rc;
    OneShot os;
    rc = os.open([&](nnlm_handle *h) { return nnlm_set_matrix_csc_kl_batch(h, n, m, colptr, rowidx, x); });
    if (rc != NNLM_OK) return rc;
    nnlm_handle *h = os.h;
    std::vector<double> Wi, Hi;
    default_factors(cb, n, m, B, k, nullptr, nullptr, &W_init, &H_init, Wi, Hi);
    CHK(nnlm_set_factors_batch(h, B, k, W_init, H_init));
    CHK(nnlm_run_batch(h, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, mse_error,
                       mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb));
    CHK(nnlm_get_factors_batch(h, W_out, H_out));
    return NNLM_OK;
}

// nnlm_c_nnmf_csc_batch on a sparse A whose absent entries are missing, with an optional hold-out pattern (ho_colptr NULL: none): the
// matrix goes through nnlm_set_matrix_csc_missing_batch; + the held-out errors of the final factors per member (NaN without a set or
// with an empty one)
extern "C" int nnlm_c_nnmf_csc_missing_batch(int n, int m, const long long *colptr, const int *rowidx, const double *x, const long long *ho_colptr,
                                             const int *ho_rowidx, unsigned B, const unsigned *k, const double *W_init, const double *H_init,
                                             const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol, int n_threads,
                                             int verbose, int show_warning, unsigned inner_max_iter, double inner_rel_tol, int method,
                                             unsigned trace, double *W_out, double *H_out, double *mse_error, double *mkl_error,
                                             double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration, int *warned,
                                             double *holdout_mse, double *holdout_mkl, const nnlm_callbacks *cb)
{
    (void)n_threads;
    if (any_null(colptr, k, alpha, beta, W_out, H_out, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned) ||
        any_null(holdout_mse, holdout_mkl))
        return fail(nullptr, NNLM_ERR_ARG, "nnlm_c_nnmf_csc_missing_batch: NULL argument");
    int rc = batch_ranks(nullptr, "nnlm_c_nnmf_csc_missing_batch", "members", B, k, [&] {
        return (method >= 3 && method <= 4) ? fail(nullptr, NNLM_ERR_UNSUPPORTED, "nnlm_c_nnmf_csc_missing_batch: method %d (KL loss) is not supported by the batched factorisation: square loss (methods 1, 2) only", method)
                                            : NNLM_OK;
    });
    if (rc != NNLM_OK) return rc;
    OneShot os;
    rc = os.open([&](nnlm_handle *h) { return nnlm_set_matrix_csc_missing_batch(h, n, m, colptr, rowidx, x, ho_colptr, ho_rowidx); });
    if (rc != NNLM_OK) return rc;
    nnlm_handle *h = os.h;
    std::vector<double> Wi, Hi;
    default_factors(cb, n, m, B, k, nullptr, nullptr, &W_init, &H_init, Wi, Hi);
    CHK(nnlm_set_factors_batch(h, B, k, W_init, H_init));
    CHK(nnlm_run_batch(h, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, mse_error,
                       mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb));
    CHK(nnlm_get_factors_batch(h, W_out, H_out));
    if (ho_colptr) CHK(nnlm_holdout_errors(h, holdout_mse, holdout_mkl));
    else
        for (unsigned b = 0; b < B; b++) holdout_mse[b] = holdout_mkl[b] = std::nan("");
    return NNLM_OK;
}

// nnlm_c_nnmf_batch on A with the pattern (colptr, rowidx) held out: + the held-out errors of the final factors, per member
extern "C" int nnlm_c_nnmf_holdout_batch(const double *A, int n, int m, const long long *colptr, const int *rowidx, unsigned B, const unsigned *k,
                                         const double *W_init, const double *H_init, const double alpha[3], const double beta[3],
                                         unsigned max_iter, double rel_tol, int n_threads, int verbose, int show_warning,
                                         unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace, double *W_out, double *H_out,
                                         double *mse_error, double *mkl_error, double *target_error, double *average_epoch, int *n_trace,
                                         unsigned *n_iteration, int *warned, double *holdout_mse, double *holdout_mkl, const nnlm_callbacks *cb)
{
    (void)n_threads;
    if (any_null(A, colptr, k, alpha, beta, W_out, H_out, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned) ||
        any_null(holdout_mse, holdout_mkl))
        return fail(nullptr, NNLM_ERR_ARG, "nnlm_c_nnmf_holdout_batch: NULL argument");
    int rc = batch_ranks(nullptr, "nnlm_c_nnmf_holdout_batch", "members", B, k, [&] {
        return (method >= 3 && method <= 4) ? fail(nullptr, NNLM_ERR_UNSUPPORTED, "nnlm_c_nnmf_holdout_batch: method %d (KL loss) is not supported by the batched factorisation: square loss (methods 1, 2) only", method)
                                            : NNLM_OK;
    });
    if (rc != NNLM_OK) return rc;
    OneShot os;
    rc = os.open([&](nnlm_handle *h) { return nnlm_set_matrix_holdout(h, A, n, m, colptr, rowidx); });
    if (rc != NNLM_OK) return rc;
    nnlm_handle *h = os.h;
    std::vector<double> Wi, Hi;
    default_factors(cb, n, m, B, k, nullptr, nullptr, &W_init, &H_init, Wi, Hi);
    CHK(nnlm_set_factors_batch(h, B, k, W_init, H_init));
    CHK(nnlm_run_batch(h, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, mse_error,
                       mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb));
    CHK(nnlm_get_factors_batch(h, W_out, H_out));
    CHK(nnlm_holdout_errors(h, holdout_mse, holdout_mkl));
    return NNLM_OK;
}

// The one-shot entries share these bodies; the dense and the sparse entries differ only in how the matrix is set (set_matrix(h)) and in
// the name their errors carry (who); matrix: the entry's first matrix array, checked for NULL.
template <typename SetMatrix>
static int c_nnmf_body(const char *who, const void *matrix, SetMatrix set_matrix, int n, int m, unsigned k, const double *W_init, const double *H_init,
                       const int *Wm, const int *Hm, const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol, int verbose,
                       int show_warning, unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace, double *W_out, double *H_out,
                       double *mse_error, double *mkl_error, double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration,
                       int *warned, const nnlm_callbacks *cb)
{
    if (any_null(matrix, alpha, beta, W_out, H_out, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned))
        return fail(nullptr, NNLM_ERR_ARG, "%s: NULL argument", who);
    if (k < 1) return fail(nullptr, NNLM_ERR_ARG, "%s: k must be >= 1", who);
    OneShot os;
    int rc = os.open(set_matrix);
    if (rc != NNLM_OK) return rc;
    nnlm_handle *h = os.h;
    std::vector<double> Wi, Hi;
    default_factors(cb, n, m, 1, &k, Wm, Hm, &W_init, &H_init, Wi, Hi);
    CHK(nnlm_set_factors(h, k, W_init, H_init, Wm, Hm));
    CHK(nnlm_run(h, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, mse_error,
                 mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb));
    CHK(nnlm_get_factors(h, W_out, H_out));
    return NNLM_OK;
}

extern "C" int nnlm_c_nnmf(const double *A, int n, int m, unsigned k, const double *W_init, const double *H_init, const int *Wm,
                           const int *Hm, const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol,
                           int n_threads, int verbose, int show_warning, unsigned inner_max_iter, double inner_rel_tol,
                           int method, unsigned trace, double *W_out, double *H_out, double *mse_error, double *mkl_error,
                           double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration, int *warned,
                           const nnlm_callbacks *cb)
{
    (void)n_threads;
    return c_nnmf_body("nnlm_c_nnmf", A, [&](nnlm_handle *h) { return nnlm_set_matrix(h, A, n, m); }, n, m, k, W_init, H_init, Wm, Hm, alpha,
                       beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method, trace, W_out, H_out, mse_error,
                       mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb);
}

extern "C" int nnlm_c_nnmf_csc(int n, int m, const long long *colptr, const int *rowidx, const double *x, unsigned k, const double *W_init,
                               const double *H_init, const int *Wm, const int *Hm, const double alpha[3], const double beta[3], unsigned max_iter,
                               double rel_tol, int n_threads, int verbose, int show_warning, unsigned inner_max_iter, double inner_rel_tol,
                               int method, unsigned trace, double *W_out, double *H_out, double *mse_error, double *mkl_error,
                               double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration, int *warned,
                               const nnlm_callbacks *cb)
{
    (void)n_threads;
    return c_nnmf_body("nnlm_c_nnmf_csc", colptr, [&](nnlm_handle *h) { return nnlm_set_matrix_csc(h, n, m, colptr, rowidx, x); }, n, m, k,
                       W_init, H_init, Wm, Hm, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method,
                       trace, W_out, H_out, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb);
}

extern "C" int nnlm_c_nnmf_csc_kl(int n, int m, const long long *colptr, const int *rowidx, const double *x, unsigned k, const double *W_init,
                                  const double *H_init, const int *Wm, const int *Hm, const double alpha[3], const double beta[3], unsigned max_iter,
                                  double rel_tol, int n_threads, int verbose, int show_warning, unsigned inner_max_iter, double inner_rel_tol,
                                  int method, unsigned trace, double *W_out, double *H_out, double *mse_error, double *mkl_error,
                                  double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration, int *warned,
                                  const nnlm_callbacks *cb)
{
    (void)n_threads;
    return c_nnmf_body("nnlm_c_nnmf_csc_kl", colptr, [&](nnlm_handle *h) { return nnlm_set_matrix_csc_kl(h, n, m, colptr, rowidx, x); }, n, m, k,
                       W_init, H_init, Wm, Hm, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method,
                       trace, W_out, H_out, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb);
}

extern "C" int nnlm_c_nnmf_csc_missing(int n, int m, const long long *colptr, const int *rowidx, const double *x, unsigned k, const double *W_init,
                                       const double *H_init, const int *Wm, const int *Hm, const double alpha[3], const double beta[3],
                                       unsigned max_iter, double rel_tol, int n_threads, int verbose, int show_warning, unsigned inner_max_iter,
                                       double inner_rel_tol, int method, unsigned trace, double *W_out, double *H_out, double *mse_error,
                                       double *mkl_error, double *target_error, double *average_epoch, int *n_trace, unsigned *n_iteration,
                                       int *warned, const nnlm_callbacks *cb)
{
    (void)n_threads;
    return c_nnmf_body("nnlm_c_nnmf_csc_missing", colptr, [&](nnlm_handle *h) { return nnlm_set_matrix_csc_missing(h, n, m, colptr, rowidx, x); },
                       n, m, k, W_init, H_init, Wm, Hm, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol,
                       method, trace, W_out, H_out, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb);
}

extern "C" int nnlm_c_nnmf_csc_weighted(int n, int m, const long long *colptr, const int *rowidx, const double *x, const double *weight,
                                        int absent_missing, unsigned k, const double *W_init, const double *H_init, const int *Wm, const int *Hm,
                                        const double alpha[3], const double beta[3], unsigned max_iter, double rel_tol, int n_threads, int verbose,
                                        int show_warning, unsigned inner_max_iter, double inner_rel_tol, int method, unsigned trace, double *W_out,
                                        double *H_out, double *mse_error, double *mkl_error, double *target_error, double *average_epoch,
                                        int *n_trace, unsigned *n_iteration, int *warned, const nnlm_callbacks *cb)
{
    (void)n_threads;
    return c_nnmf_body("nnlm_c_nnmf_csc_weighted", colptr,
                       [&](nnlm_handle *h) { return nnlm_set_matrix_csc_weighted(h, n, m, colptr, rowidx, x, weight, absent_missing); }, n, m, k,
                       W_init, H_init, Wm, Hm, alpha, beta, max_iter, rel_tol, verbose, show_warning, inner_max_iter, inner_rel_tol, method,
                       trace, W_out, H_out, mse_error, mkl_error, target_error, average_epoch, n_trace, n_iteration, warned, cb);
}

template <typename SetMatrix>
static int c_nnlm_body(const char *who, const void *y, SetMatrix set_matrix, const double *x, int n, int p, int q, const double alpha[3],
                       const int *mask, const double *beta0, unsigned max_iter, double rel_tol, int method, double *coefficient, int *n_iteration,
                       const nnlm_callbacks *cb)
{
    if (any_null(x, y, alpha, coefficient, n_iteration)) return fail(nullptr, NNLM_ERR_ARG, "%s: NULL argument", who);
    if (n < 1 || p < 1 || q < 1) return fail(nullptr, NNLM_ERR_ARG, "%s: empty x or y", who);
    // y plays A (n x q), x plays W (n x p), beta plays H (p x q): one H half-step, src/nnlm.cpp:44-47
    OneShot os;
    int rc = os.open(set_matrix);
    if (rc != NNLM_OK) return rc;
    nnlm_handle *h = os.h;
    std::vector<double> b0;
    if (!beta0) { // beta.randu(), src/nnlm.cpp:38-39
        b0.resize((size_t)p * q);
        Lcg lcg;
        for (auto &v : b0) v = (cb && cb->unif_rand) ? cb->unif_rand(cb->ctx) : lcg.next();
        beta0 = b0.data();
    }
    CHK(nnlm_set_factors(h, (unsigned)p, x, beta0, nullptr, mask));
    CHK(half_step(h, 1, alpha, max_iter, rel_tol, method));
    long long raw = 0;
    CHK(nnlm_take_sweeps(h, &raw, 1));
    *n_iteration = (int)raw;
    CHK(nnlm_get_factors(h, nullptr, coefficient));
    return NNLM_OK;
}

extern "C" int nnlm_c_nnlm(const double *x, const double *y, int n, int p, int q, const double alpha[3], const int *mask,
                           const double *beta0, unsigned max_iter, double rel_tol, int n_threads, int method, double *coefficient,
                           int *n_iteration, const nnlm_callbacks *cb)
{
    (void)n_threads;
    return c_nnlm_body("nnlm_c_nnlm", y, [&](nnlm_handle *h) { return nnlm_set_matrix(h, y, n, q); }, x, n, p, q, alpha, mask, beta0, max_iter,
                       rel_tol, method, coefficient, n_iteration, cb);
}

extern "C" int nnlm_c_nnlm_csc(const double *x, int n, int p, int q, const long long *ycolptr, const int *yrowidx, const double *yx,
                               const double alpha[3], const int *mask, const double *beta0, unsigned max_iter, double rel_tol, int n_threads,
                               int method, double *coefficient, int *n_iteration, const nnlm_callbacks *cb)
{
    (void)n_threads;
    return c_nnlm_body("nnlm_c_nnlm_csc", ycolptr, [&](nnlm_handle *h) { return nnlm_set_matrix_csc(h, n, q, ycolptr, yrowidx, yx); }, x, n, p,
                       q, alpha, mask, beta0, max_iter, rel_tol, method, coefficient, n_iteration, cb);
}

extern "C" int nnlm_c_nnlm_csc_kl(const double *x, int n, int p, int q, const long long *ycolptr, const int *yrowidx, const double *yx,
                                  const double alpha[3], const int *mask, const double *beta0, unsigned max_iter, double rel_tol, int n_threads,
                                  int method, double *coefficient, int *n_iteration, const nnlm_callbacks *cb)
{
    (void)n_threads;
    return c_nnlm_body("nnlm_c_nnlm_csc_kl", ycolptr, [&](nnlm_handle *h) { return nnlm_set_matrix_csc_kl(h, n, q, ycolptr, yrowidx, yx); }, x, n,
                       p, q, alpha, mask, beta0, max_iter, rel_tol, method, coefficient, n_iteration, cb);
}

extern "C" int nnlm_c_nnlm_csc_missing(const double *x, int n, int p, int q, const long long *ycolptr, const int *yrowidx, const double *yx,
                                       const double alpha[3], const int *mask, const double *beta0, unsigned max_iter, double rel_tol, int n_threads,
                                       int method, double *coefficient, int *n_iteration, const nnlm_callbacks *cb)
{
    (void)n_threads;
    return c_nnlm_body("nnlm_c_nnlm_csc_missing", ycolptr, [&](nnlm_handle *h) { return nnlm_set_matrix_csc_missing(h, n, q, ycolptr, yrowidx, yx); },
                       x, n, p, q, alpha, mask, beta0, max_iter, rel_tol, method, coefficient, n_iteration, cb);
}
extern "C" int nnlm_c_nnlm_csc_weighted(const double *x, int n, int p, int q, const long long *ycolptr, const int *yrowidx, const double *yx,
                                        const double *weight, int absent_missing, const double alpha[3], const int *mask, const double *beta0,
                                        unsigned max_iter, double rel_tol, int n_threads, int method, double *coefficient, int *n_iteration,
                                        const nnlm_callbacks *cb)
{
    (void)n_threads;
    return c_nnlm_body("nnlm_c_nnlm_csc_weighted", ycolptr,
                       [&](nnlm_handle *h) { return nnlm_set_matrix_csc_weighted(h, n, q, ycolptr, yrowidx, yx, weight, absent_missing); }, x, n, p,
                       q, alpha, mask, beta0, max_iter, rel_tol, method, coefficient, n_iteration, cb);
}
#undef CHK
