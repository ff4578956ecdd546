// tu_topn.hip -- the instantiations of the scoring kernels (k_topn.h), see tu_topn.h.
#include "k_topn.h"

// Room for the n_top kept entries plus what arrives until the next prune: one more n_top up to 64 (a prune then halves the buffer),
// 64 beyond (a line's buffer stays under 2.3 KB, so that four wavefronts of 16 lines fit the LDS of a CU); never less than 32.
int nnlm_topn_cap(int ntop) { return ntop < 16 ? 32 : (ntop <= 64 ? 2 * ntop : ntop + 64); }

static size_t topn_lds_bytes(int cap, int nw) { return (size_t)nw * 16 * ((size_t)(cap | 1) * 8 + (size_t)cap * 4); }

int nnlm_topn_waves(int ntop)
{
    const int cap = nnlm_topn_cap(ntop);
    int nw = 4;
    while (nw > 1 && topn_lds_bytes(cap, nw) > 65536) nw >>= 1;
    return nw;
}

template <int NS> static void launch_topn(const TopnArgs &a, int nw, hipStream_t st)
{
    const int ngroups = (a.nlines + 15) / 16;
    dim3 grid((unsigned)a.nslices, (unsigned)((ngroups + nw - 1) / nw));
    topn_kernel<NS><<<grid, 64 * nw, topn_lds_bytes(a.cap, nw), st>>>(a);
}

void nnlm_tu_topn(const TopnArgs &a, int nw, hipStream_t st)
{
    switch (a.K4 / 4 <= TOPN_REG_STEPS ? a.K4 / 4 : 0) {
#define TOPN_CASE(NS) case NS: launch_topn<NS>(a, nw, st); break;
        TOPN_CASE(1) TOPN_CASE(2) TOPN_CASE(3) TOPN_CASE(4) TOPN_CASE(5) TOPN_CASE(6) TOPN_CASE(7) TOPN_CASE(8) TOPN_CASE(9)
        TOPN_CASE(10) TOPN_CASE(11) TOPN_CASE(12) TOPN_CASE(13) TOPN_CASE(14) TOPN_CASE(15) TOPN_CASE(16) TOPN_CASE(17) TOPN_CASE(18)
#undef TOPN_CASE
    default: launch_topn<0>(a, nw, st); break;
    }
}

void nnlm_tu_topn_merge(const TopnArgs &a, int *idx_out, double *score_out, hipStream_t st)
{
    topn_merge_kernel<<<(a.nlines + 3) / 4, 256, 0, st>>>(a.part_s, a.part_i, a.nlines, a.nslices, a.ntop, idx_out, score_out);
}

void nnlm_tu_predict_entries(const int *rows, const int *cols, long long count, const double *Wrow, const double *Hrow, int K4, int k, double *out,
                             hipStream_t st)
{
    long long nbx = (count + 1023) / 1024; // at least four entries per lane
    if (nbx > 4096) nbx = 4096;
    const long long chunk = (count + nbx - 1) / nbx;
    predict_entries_kernel<<<(unsigned)nbx, 256, 0, st>>>(rows, cols, count, chunk, Wrow, Hrow, K4, k, out);
}

void nnlm_tu_topn_eval(const TopnEvalArgs &a, hipStream_t st) { topn_eval_kernel<<<(a.nlines + 3) / 4, 256, 0, st>>>(a); }

void nnlm_tu_topn_eval_reduce(const TopnEvalArgs &a, double *acc, hipStream_t st)
{
    topn_eval_reduce_kernel<<<6 * a.ncut + 1, 256, 0, st>>>(a.part, a.pstride, a.nlines, acc);
}

void nnlm_tu_topn_eval_overlap(const int *lines, long long nlines, const long long *hptr, const int *hidx, const long long *xptr, const int *xidx,
                               unsigned long long *first_key, hipStream_t st)
{
    if (nlines > 0) topn_eval_overlap_kernel<<<(unsigned)((nlines + 3) / 4), 256, 0, st>>>(lines, nlines, hptr, hidx, xptr, xidx, first_key);
}
