// tu_topn.h -- launch entries of the scoring kernels of k_topn.h (tu_topn.hip): listed entries of W H and the fused score-and-select
// kernel behind nnlm_predict_entries / nnlm_top_n.  Neither forms W H: nothing n x m sized exists.
#pragma once
#include <hip/hip_runtime.h>

#define TOPN_MAX 128       // largest n_top
#define TOPN_MAX_SLICES 64 // slices of the candidate range per launch: one lane of topn_merge_kernel each
#define TOPN_REG_STEPS 18  // rank steps of four whose line rows a wavefront keeps in registers (K4 <= 72); beyond: re-read per tile

// A "line" is what the caller listed (a column j for by = 0, a row i for by = 1); a "candidate" is an index of the other side.
struct TopnArgs {
    const double *Crow;    // [ncand][K4] factor rows of the candidates (zeros behind k)
    const double *Lrow;    // [lines of that side][K4] factor rows of the lines
    const int *lines;      // [nlines] the launch's lines (device), or nullptr: line0 .. line0 + nlines - 1
    int line0, nlines;
    int ncand, K4, ntop;
    int cap;               // entries of a line's candidate buffer in LDS, >= ntop + 16
    int nslices, slice_len; // slice s owns candidates [s slice_len, (s + 1) slice_len); slice_len is a multiple of 16
    const long long *xptr; // exclusion: the stored candidates of line l are xidx[xptr[l] .. xptr[l + 1]), ascending; nullptr = none
    const int *xidx;
    double *part_s;        // [nlines][nslices][ntop] partial lists, best first; (NaN, -1) behind a short one
    int *part_i;
};

// candidate buffer entries for n_top, and wavefronts (groups of 16 lines) per workgroup so that its buffers fit 64 KB of LDS
int nnlm_topn_cap(int ntop);
int nnlm_topn_waves(int ntop);
// grid (a.nslices, ceil(groups of 16 lines / nw)), nw wavefronts each
void nnlm_tu_topn(const TopnArgs &a, int nw, hipStream_t st);
// idx_out / score_out [nlines][ntop] from the partial lists
void nnlm_tu_topn_merge(const TopnArgs &a, int *idx_out, double *score_out, hipStream_t st);
// out[e] = sum over q < k of Wrow[rows[e]][q] Hrow[cols[e]][q], q ascending; Wrow [n][K4], Hrow [m][K4]
void nnlm_tu_predict_entries(const int *rows, const int *cols, long long count, const double *Wrow, const double *Hrow, int K4, int k, double *out,
                             hipStream_t st);

// ---- ranking metrics of the merged lists against held-out entries (nnlm_top_n_eval) ----
#define TOPN_EVAL_MAX_CUT 8 // cutoffs per call

// One round: the merged index lists of `nlines` lines as topn_merge_kernel left them, and the held-out indices of those lines.
struct TopnEvalArgs {
    const int *idx;        // [nlines][ntop] merged lists, -1 behind a short one
    int nlines, ntop, ncut;
    int cut[TOPN_EVAL_MAX_CUT]; // ascending, cut[ncut - 1] = ntop
    const long long *hptr; // [nlines + 1] the held-out indices of the round's line l are hidx[hptr[l] .. hptr[l + 1]), ascending
    const int *hidx;
    const double *disc;    // [TOPN_MAX] d[p] = 1 / log2(p + 2)
    const double *idcg;    // [TOPN_MAX + 1] idcg[j] = d[0] + .. + d[j - 1], added in that order
    double *rec;           // [nlines][2 + 3 ncut] per-line records (t, first, then hits, dcg, apn per cutoff), or nullptr
    double *part;          // [6 ncut + 1][pstride] column major: value v of line l at part[v pstride + l]; workgroup w owns l = 4 w .. 4 w + 3.
    int pstride;           //   v = 6 c + (precision, recall, hit rate, NDCG, AP, RR) of cutoff c; v = 6 ncut: 1 if the line is evaluated
};
// one wavefront per line, four per workgroup
void nnlm_tu_topn_eval(const TopnEvalArgs &a, hipStream_t st);
// acc[v] += the sum of column v of a.part over the round's lines, in a fixed order (one workgroup per column)
void nnlm_tu_topn_eval_reduce(const TopnEvalArgs &a, double *acc, hipStream_t st);
// *first_key = min over the held-out entries (list position l, index c) that are stored in the line's xidx range of (l << 32 | c); the
// caller sets it to all ones.  lines: device [nlines] or nullptr = 0 .. nlines - 1; hptr / hidx: of all listed lines, by list position
void nnlm_tu_topn_eval_overlap(const int *lines, long long nlines, const long long *hptr, const int *hidx, const long long *xptr, const int *xidx,
                               unsigned long long *first_key, hipStream_t st);
