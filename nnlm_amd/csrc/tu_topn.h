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
