// tu_sweepq.h -- launch entries of the SCD sweep kernels of k_sweep_q.h.  Their instantiations (one per block count NB = 1 .. 16,
// mask, arithmetic mode: 64 + 64) dominate the build, so they are compiled as translation units of their own, in parallel with
// nnlm_mi355x.hip (nnlm_amd/build.py): tu_sweepq.hip (sweep_scd_q_kernel) and tu_sweepqw.hip (sweep_scd_qw_kernel, the persistent form).
// Both return what hipFuncSetAttribute(MaxDynamicSharedMemorySize) said; the launch itself is checked by the caller (LAUNCHCHK).
#pragma once
#include "k_sweep.h"

// nb workgroups of 64 columns (four wavefronts of 16); img = the operand image written by sweepq_pack_kernel
hipError_t nnlm_tu_sweep_q(const SweepArgs &a, const double *img, int nb, int NB, bool strict, hipStream_t st);
// nb workgroups of G column groups of 16 (one workgroup per CU)
hipError_t nnlm_tu_sweep_qw(const SweepArgs &a, const double *img, int nb, int NB, bool strict, int G, hipStream_t st);
// fp32-operand mode (k_sweep_f.h, tu_sweepf.hip): nb workgroups of NW = 4 or 8 wavefronts of 16 columns; reads a.Graw, no operand image
hipError_t nnlm_tu_sweep_f(const SweepArgs &a, int nb, int NB, int NW, hipStream_t st);
// fp32-operand mode, per-column Grams (k_colsolve_row.h, tu_colsolve.hip): columns a.col0 .. a.ncols - 1, four per wavefront
void nnlm_tu_colsolve_row(const SweepArgs &a, size_t g_stride, hipStream_t st);
// fp32-operand mode, row form (k_sweep_r.h, tu_sweepr.hip): nb workgroups of NW = 4 or 8 wavefronts of FOUR columns; a.k <= SWEEPR_KMAX; reads a.Graw
#define SWEEPR_KMAX 50
void nnlm_tu_sweep_r(const SweepArgs &a, int nb, int NW, hipStream_t st);

// Sparse A (k_sparse.h, tu_sparse.hip): the cross product of a half-step as an SpMM over the non-zeros, and the error sums over them
struct SpmmArgs {
    const long long *ptr; // [ncols + 1]
    const int *idx;       // [nnz] contraction index (row of A for CSC, column for CSR)
    const void *val;      // [nnz] T
    const void *Y;        // [rows][KP] T, row-major fixed factor
    long long nnz, chunk; // non-zeros per worker
    int ncols, KP, q0;    // columns of the output; coordinates q0 .. q0 + 63 (rank > 64: one launch per 64 coordinates)
    int nworkers;
    double *C;            // C[q * ldc + c]
    int ldc;
    double *carry;        // [nworkers][64]
};
// launch entries (tu_sparse.hip); f64 selects T = double, else float
void nnlm_tu_spmm(const SpmmArgs &a, bool f64, hipStream_t st);
// miss: absent entries are missing -- the second sum is sum wh instead of sum wh^2 (k_sparse_na.h)
void nnlm_tu_sp_errors(const long long *ptr, const int *idx, const void *val, bool f64, int ncols, long long nnz, long long chunk, int nworkers,
                       const double *Wrow, int KP, int k, const double *H, int ldh, double *partial, int nblocks, bool miss, hipStream_t st);
// workers of one launch: a multiple of the workers per wavefront; nnz / workers non-zeros each, at least ~64, at most 16 wavefronts per CU
int nnlm_sp_workers(long long nnz, int KP, int cus);
int nnlm_sp_lanes(int KP);
// partial[b][q] = sum of X[q][c] (X [KP][ld] fp64) over columns [2048 b, 2048 (b + 1)) of ncols
void nnlm_tu_sp_rowsums(const double *X, int ld, int ncols, int KP, double *partial, int nblocks, hipStream_t st);
// out[0] = sum of squares, out[1] = KL sum over all n x m entries from s = {S1, S2, S3}, the Grams and the factors' sums (k_sparse.h)
void nnlm_tu_sp_err_final(const double *s, const double *GW, const double *GH, const double *wsum, const double *hsum, int k, int KP, double *out,
                          hipStream_t st);
// Batched factorisation on a sparse A (k_sparse_batch.h): the three sums over the non-zeros of every member b < B with bit b of amask
// set, off [B + 1] (device) the members' first coordinates in the row copies Wrow [n][KP], Hrow [m][KP]; nwaves wavefronts of chunk
// non-zeros each (nnlm_spb_waves, nnlm_spb_chunk: functions of nnz and the CU count only); partial [3 B][(nwaves + 3) / 4]
void nnlm_tu_sp_batch_errors(const long long *ptr, const int *idx, const void *val, bool f64, int ncols, long long nnz, long long chunk, int nwaves,
                             const double *Wrow, const double *Hrow, int KP, const int *off, int B, unsigned long long amask, double *partial,
                             hipStream_t st);
#define SPB_BATCH_MAX 64 // members of a batch: BATCH_MAX of k_batch.h (the kernel keeps a slot per member and wavefront in LDS)
int nnlm_spb_waves(long long nnz, int cus);
long long nnlm_spb_chunk(long long nnz, int nwaves);
// out[2 b], out[2 b + 1] = member b's sum of squares and KL sum over all n x m entries from s [3 B], the stacked Grams and coordinate sums
void nnlm_tu_sp_batch_final(const double *s, const double *GW, const double *GH, const double *wsum, const double *hsum, const int *off, int B, int KP,
                            unsigned long long amask, double *out, hipStream_t st);

// Sparse A whose absent entries are missing (k_sparse_na.h, tu_sparse.hip): per-column Grams over the stored rows of columns [c0, c1)
#define SPG_SEG 2048 // stored entries per segment: a longer column is summed in segments of its own, added in order by the fix-up
struct SpGramArgs {
    const long long *ptr;   // [ncols + 1] CSC (H half-step) / CSR (W half-step)
    const int *idx;         // [nnz] row of the fixed factor of each stored entry
    const void *Y;          // [rows][KP] T, row-major fixed factor
    const long long *segoff; // [ncols + 1] segment slots of the long columns in front of column c
    int c0, c1;             // the launch's columns
    long long chunk;        // stored entries per worker
    int nworkers;
    double *G;              // [c1 - c0][KP][KP] per-column Grams (upper triangle)
    double *seg;            // segment sums of the launch's long columns, [segoff[c1] - segoff[c0]][KP][KP]
    // weighted form (nnlm_set_matrix_csc_weighted): G_j = cw0 G_full + sum over the stored entries e of (wt[e] - cw0) y y^T
    const void *wt = nullptr;      // [nnz] T, weight of each stored entry (NULL: the unweighted kernel)
    double cw0 = 0.0;              // weight of an absent entry: 0 (missing) or 1 (a zero)
    const double *Gfull = nullptr; // cw0 = 1: the shared Gram of the fixed factor [KP][KP], added once per column
};
// workers (one wavefront each) of one Gram launch over nnz stored entries: ~256 each, at most 16 wavefronts per CU
int nnlm_spg_workers(long long nnz, int cus);
void nnlm_tu_sp_gram(const SpGramArgs &a, int NKQ, bool f64, hipStream_t st);
// the nlong long columns longc[0 .. nlong) of the launch: their segment sums into G
void nnlm_tu_sp_gram_fixup(const SpGramArgs &a, const int *longc, int nlong, int KP, hipStream_t st);
// out[0] = S1, out[1] = S3 + S2 (sum of squares, KL sum over the stored entries)
void nnlm_tu_sp_err_final_missing(const double *s, double *out, hipStream_t st);
// Per-entry weights (nnlm_set_matrix_csc_weighted): wt [nnz] T beside val; partial holds FIVE sums per workgroup --
// {sum c r^2, sum wh^2, sum c (-(a + eps) log(wh + eps)), sum c wh, sum wh} over the stored entries
void nnlm_tu_sp_errors_weighted(const long long *ptr, const int *idx, const void *val, const void *wt, bool f64, int ncols, long long nnz,
                                long long chunk, int nworkers, const double *Wrow, int KP, int k, const double *H, int ldh, double *partial,
                                int nblocks, hipStream_t st);
// s = those five sums.  miss: out[0] = s0, out[1] = s2 + s3.  Otherwise (absent entries are zeros of weight 1)
// out[0] = s0 + max(0, <W^T W, H H^T> - s1), out[1] = s2 + sum_q (sum_i W_iq)(sum_j H_qj) + (s3 - s4)
void nnlm_tu_sp_err_final_weighted(const double *s, const double *GW, const double *GH, const double *wsum, const double *hsum, int k, int KP,
                                   bool miss, double *out, hipStream_t st);

// Batched factorisation on such a matrix (k_sparse_na_batch.h): the Grams of all members in one launch.  g.Y is the row copy at the
// STACKED KP; column c's Grams take `slot` doubles of g.G (member b's at goff_b, compact at its own KP_b), a segment of a long column
// `slot` doubles of g.seg.  pairs / tiles: the upper tile pairs (ta <= tb, ta-major) that meet an active member's diagonal block, and
// the coordinate tiles those pairs touch.  tab[i] = member of stacked coordinate i or -1 (not active / beyond the stack),
// tab[64 + i] = goff_b + (i - off_b) KP_b - off_b: element (i, j) of the stack goes to word tab[64 + i] + j of the slot.
struct SpGramBatchArgs {
    SpGramArgs g;
    size_t slot;
    unsigned pairs, tiles;
    int tab[128];
};
void nnlm_tu_sp_gram_batch(const SpGramBatchArgs &a, int NT, bool f64, hipStream_t st);
void nnlm_tu_sp_gram_batch_fixup(const SpGramBatchArgs &a, const int *longc, int nlong, int KP, hipStream_t st);
// The error sums of the batch when absent entries are missing: nnlm_tu_sp_batch_errors with S2_b = sum of wh over the stored entries
void nnlm_tu_sp_batch_errors_missing(const long long *ptr, const int *idx, const void *val, bool f64, int ncols, long long nnz, long long chunk,
                                     int nwaves, const double *Wrow, const double *Hrow, int KP, const int *off, int B, unsigned long long amask,
                                     double *partial, hipStream_t st);
// out[2 b] = S1_b, out[2 b + 1] = S3_b + S2_b for every member with its bit of amask set (nnlm_tu_sp_err_final_missing per member)
void nnlm_tu_sp_batch_final_missing(const double *s, int B, unsigned long long amask, double *out, hipStream_t st);

// Sparse A, KL loss (k_sparse_kl.h, tu_sparse.hip): scd_kl_update / lee_kl_update over the stored entries of the lines [0, ncols)
struct SpKlArgs {
    const long long *ptr;  // [ncols + 1] CSC (H half-step) / CSR (W half-step)
    const int *idx;        // [nnz] row of the fixed factor of each stored entry
    const void *val;       // [nnz] T
    const void *Y;         // [rows][KP] T, row-major fixed factor
    int KP, ncols, k;      // k <= 64
    const double *X;       // [KP][ldx] master of the factor solved, read
    double *Xout;          // same layout, written (may alias X)
    int ldx;
    const double *sumw;    // [k] column sums of the fixed factor
    double r0, r1, r2;
    const unsigned long long *mask; // [ncols][mw] or NULL
    int mw;
    unsigned max_iter;
    double rel_tol;
    void *op;              // fp32 operand copy of the factor solved [KP][op_ld] (op_mode 1: the fp32-operand mode's W), or none
    int op_mode, op_ld;
    unsigned long long *sweeps;
    void *state;           // [nnz] T: states of the long lines' entries (long form)
    const int *longc;      // the lines the long form takes
    int nlong;
};
// the longest line the short form (a wavefront per line) takes
int nnlm_spkl_short_max(void);
// method 3 (SCD) or 4 (Lee); short form over all lines (it skips the long ones) when nshort > 0, long form over a.longc when a.nlong > 0
void nnlm_tu_sp_kl(const SpKlArgs &a, int method, bool f64, int nshort, hipStream_t st);

// The same half-step for the active members of a batch (k_sparse_kl_batch.h): a.Y, a.X, a.Xout, a.sumw and a.op are
// the STACKED factor's, a.k the sum of the ranks, a.mask NULL.  Member b holds the coordinates off[b] .. off[b] + kb[b] - 1 and counts
// its sweeps in sweeps[b]; mem[0 .. nmem) lists the members that run (the others' rows are neither read for a sum nor written).
struct SpKlBatchArgs {
    SpKlArgs a;
    unsigned long long *sweeps; // [B]
    int nmem;
    unsigned char mem[64], off[64], kb[64];
};
#define SPKL_BATCH_G 2 // member chains a wavefront interleaves: the lowest time of 1, 2, 4 at 1 % / F32 / 8 x 8, by under 1 %
// the group size a new handle takes: SPKL_BATCH_G, or NNLM_SPKL_BATCH_GROUP = 1, 2 or 4 (the measurement's switch)
int nnlm_spkl_batch_group(void);
// ONE launch over all lines of at most nnlm_spkl_short_max() stored entries, group = 1, 2 or 4; the longer lines stay the caller's
void nnlm_tu_sp_kl_batch(const SpKlBatchArgs &a, int method, bool f64, int group, hipStream_t st);
// the long form alone (sp_kl_solve_long_kernel over a.longc): a batch launches it once per active member, on that member's offsets
void nnlm_tu_sp_kl_long(const SpKlArgs &a, int method, bool f64, hipStream_t st);

// Ingest of a sparse matrix in device memory (k_sparse_ingest.h, tu_sparse.hip).  i64: the caller's integer type
// (int64, else int32); dtype: the caller's NNLM_DT_* value type; f64: the mode's value type.
int nnlm_spi_check_share(void); // entries per block of the entry check
int nnlm_spi_sort_tile(void);   // entries per block of a radix pass
int nnlm_spi_scan_tile(void);   // elements per block of the scans
// out [lines + 1] = the pointers as int64; blockmin [(lines + 256) / 256] offence codes
void nnlm_tu_spi_ptr(const void *ptr, bool i64, int lines, long long nnz, long long *out, long long *blockmin, hipStream_t st);
// nnz > 0.  blockcode [nb], blockstat [nb][3], nb = ceil(nnz / nnlm_spi_check_share())
void nnlm_tu_spi_check(const long long *ptr, int lines, const void *idx, bool i64, const void *val, int dtype, bool f64, long long nnz, long long other,
                       bool kl, int *idx_out, void *val_out, void *val_sort, int *line_out, long long *blockcode, double *blockstat, hipStream_t st);
void nnlm_tu_spi_fetch(const void *idx, bool i64, const void *val, int dtype, long long e, long long *i_out, double *v_out, hipStream_t st);
void nnlm_tu_spi_count(const int *idx, long long nnz, long long *cnt, hipStream_t st);
// x [len] -> its exclusive scan, in place; bsum: scratch of ceil(len / nnlm_spi_scan_tile()) elements
void nnlm_tu_spi_scan(long long *x, long long len, long long *bsum, hipStream_t st);
// One stable radix pass by (key >> shift) & 255 (kout == NULL: keys not written).  ghist: 256 ceil(nnz / nnlm_spi_sort_tile()) elements;
// bsum: scratch of the scan of ghist.  win != NULL: the weights and the products c a (mode's type) go to wout / aout at the same positions
void nnlm_tu_spi_sort_pass(const int *kin, const int *lin, const void *vin, int *kout, int *lout, void *vout, bool f64, long long nnz, int shift,
                           long long *ghist, long long *bsum, hipStream_t st, const void *win = nullptr, const void *ain = nullptr,
                           void *wout = nullptr, void *aout = nullptr);
// Per-entry weights.  The weights' own pattern against the accepted resident one: blockmin [(lines + 256) / 256] =
// the first line whose extent differs; blockmin [ceil(nnz / 256)] = the first entry whose index differs (nnz > 0)
void nnlm_tu_spi_pattern_ptr(const void *ptr, bool i64, const long long *ref, int lines, long long *blockmin, hipStream_t st);
void nnlm_tu_spi_pattern_idx(const void *idx, bool i64, const int *ref, long long nnz, long long *blockmin, hipStream_t st);
// nnz > 0, on values the entry check has accepted.  wdtype: the weights' NNLM_DT_*; blockcode [nb] = first offending weight's entry,
// blockstat [nb][3] = {entries beyond fp32 through c or c a, max |(float)(c a)|, the weighted KL sum}, nb as for nnlm_tu_spi_check
void nnlm_tu_spi_wcheck(const void *val, int dtype, const void *wgt, int wdtype, bool f64, long long nnz, void *wt_out, void *wt_sort, void *wa_out,
                        void *wa_sort, long long *blockcode, double *blockstat, hipStream_t st);
