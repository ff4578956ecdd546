// k_sparse_na.h -- per-column Grams over the STORED rows of a sparse A whose absent entries are missing (nnlm_set_matrix_csc_missing).
//
// Reference: update_with_missing(), src/update_with_missing.cpp:58-139.  Column j of the half-step sums only over the rows it observes:
//   G_j = sum over the stored entries e of column j of y_row(e) y_row(e)^T        (per-column Gram, :90)
//   b_j = sum over the stored entries e of column j of a_e y_row(e)                (cross product, :91: spmm_kernel of k_sparse.h, unchanged)
// H half-step: the CSC of A, y = rows of W;  W half-step: the CSR of A (= CSC of A^T), y = rows of H -- both resident on the handle.
// The output is what launch_na_gram leaves for the dense NA path: fp64 [col][KP][KP], upper triangle, unscaled (both modes), so the
// per-column solvers (launch_colsolve: colsolve_row_kernel, colsolve_strict_kernel, colsolve_ls_kernel) run unchanged.
//
// Work split (skewed columns: many with 1-5 entries, a few with a large share of all of them).  A column is cut into SEGMENTS of at
// most SPG_SEG stored entries, counted from its start: the cut is a property of the column, not of the launch.  A worker (one
// wavefront) owns a contiguous range of non-zeros, as in spmm_kernel, and sums every segment that STARTS in its range (a segment may run
// past the range's end): one wavefront takes many short columns one after another, a long column is spread over many wavefronts.
//   sp_gram_kernel        one segment at a time: groups of four stored rows on v_mfma_f64_16x16x4_f64, one product per upper tile pair
//                         (lane l: row l / 16 of the group, coordinate 16 t + l % 16 -- the layout of na_gram_lds_kernel), four groups'
//                         gathers in flight.  A column of one segment is written straight into the Gram buffer; a longer one writes
//                         each segment's sum into a slot of its own (segoff: slots of the long columns in front of column c).
//   sp_gram_fixup_kernel  the long columns: their segment sums added in segment order.
// No atomics, and every sum is a fixed function of the column: repeated runs, any worker count and any column chunking give the same
// bits.  Rows of the fixed factor come from the half-step's row copy in the mode's type (fp32 in the fp32-operand mode: the product of
// two fp32 numbers is exact in fp64, so both modes form and accumulate every product in fp64 -- at least as accurate as the split-fp16
// form of na_gram_f16_kernel).  Empty columns get G = 0 (nothing observed: the solvers see TINY I + the regularisation, as on the dense
// NA path and in the reference).
//
// Weighted form (WT; nnlm_set_matrix_csc_weighted): stored entry e has weight c_e >= 0, an absent entry weight c0 = 0 (missing) or 1 (a
// zero), and column j needs  G_j = c0 G_full + sum over its stored entries of (c_e - c0) y_row(e) y_row(e)^T.  A lane loads the weight of
// its stored row beside the row's index, forms c_e - c0 in fp64 and scales ONE operand of each product with it; segments, worker ranges
// and summation order are those of the plain form, and a weight of exactly 1 with c0 = 0 changes no bit (y * 1.0 is exact).  c0 = 1: the
// shared Gram (launch_gram's, raw) is added once per column -- at the store of a one-segment column (an empty column gets G_full: under
// the zero semantics it is a real all-zero column), by the fix-up for a long one.
#pragma once
#include "common.h"
#include "tu_sweepq.h"

// (SPG_SEG, SpGramArgs and the launch entries: tu_sweepq.h)

// smallest c in [lo, hi] with ptr[c] >= e  (ptr[hi] >= e)
__device__ static inline int spg_lower_bound(const long long *__restrict__ ptr, int lo, int hi, long long e)
{
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] < e) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <typename T, int NT, bool WT = false>
__global__ __launch_bounds__(256) void sp_gram_kernel(const SpGramArgs a)
{
    constexpr int KP = 16 * NT, NP = NT * (NT + 1) / 2;
    constexpr int GR = 4; // groups of four rows whose gathers are in flight together
    using M = Mfma<double>;
    const int lane = threadIdx.x & 63, l15 = lane & 15, lg = lane >> 4;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.nworkers) return; // whole wavefront
    const T *Y = (const T *)a.Y;
    const T *wt = (const T *)a.wt;
    const long long E0 = a.ptr[a.c0], E1 = a.ptr[a.c1];
    long long e0 = E0 + (long long)w * a.chunk, e1 = e0 + a.chunk;
    if (e0 > E1) e0 = E1;
    if (e1 > E1) e1 = E1;
    // sum over the stored rows [st, en) of column c (its segment s) into the column's Gram or the segment's slot
    auto segment = [&](int c, long long s, long long st, long long en, bool is_long) {
        typename M::acc_t acc[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) acc[i] = typename M::acc_t{0, 0, 0, 0};
        for (long long e = st; e < en; e += 4 * GR) {
            int ri[GR];
            double cw[GR]; // (WT only) c_e - c0 of the lane's stored row
#pragma unroll
            for (int u = 0; u < GR; u++) {
                const long long r = e + 4 * u + lg;
                ri[u] = r < en ? a.idx[r] : -1;
                if (WT) cw[u] = r < en ? (double)wt[r] - a.cw0 : 0.0;
            }
            double y[GR][NT];
#pragma unroll
            for (int u = 0; u < GR; u++)
#pragma unroll
                for (int t = 0; t < NT; t++) y[u][t] = ri[u] >= 0 ? (double)Y[(size_t)ri[u] * KP + 16 * t + l15] : 0.0;
#pragma unroll
            for (int u = 0; u < GR; u++) {
                int pi = 0;
#pragma unroll
                for (int ta = 0; ta < NT; ta++) {
                    const double ya = WT ? y[u][ta] * cw[u] : y[u][ta];
#pragma unroll
                    for (int tb = ta; tb < NT; tb++, pi++) acc[pi] = M::mma(ya, y[u][tb], acc[pi]);
                }
            }
        }
        double *out = is_long ? a.seg + (size_t)(a.segoff[c] - a.segoff[a.c0] + s) * KP * KP : a.G + (size_t)(c - a.c0) * KP * KP;
        const double *gf = (WT && !is_long) ? a.Gfull : nullptr; // (a long column: the fix-up adds it, once)
        int pi = 0;
#pragma unroll
        for (int ta = 0; ta < NT; ta++)
#pragma unroll
            for (int tb = ta; tb < NT; tb++, pi++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = 16 * ta + M::row_of(lane, r), j = 16 * tb + l15;
                    if (i <= j) out[i * KP + j] = gf ? gf[i * KP + j] + acc[pi][r] : acc[pi][r]; // (upper triangle: the solvers read G[min][max])
                }
    };
    int c = spg_lower_bound(a.ptr, a.c0, a.c1, e0);
    if (c > a.c0 && a.ptr[c - 1] < e0) { // e0 lies inside column c - 1, which started in an earlier worker's range: its segments from e0 on
        const int hc = c - 1;
        const long long ps = a.ptr[hc], pe = a.ptr[hc + 1];
        for (long long s = (e0 - ps + SPG_SEG - 1) / SPG_SEG; ps + s * SPG_SEG < pe && ps + s * SPG_SEG < e1; s++) {
            const long long st = ps + s * SPG_SEG;
            segment(hc, s, st, st + SPG_SEG < pe ? st + SPG_SEG : pe, true); // (s >= 1: only a long column gets here)
        }
    }
    // columns starting in [e0, e1); the last worker also owns the empty columns at the end (start = E1)
    const long long climit = (w == a.nworkers - 1) ? E1 + 1 : e1;
    for (; c < a.c1; c++) {
        const long long ps = a.ptr[c];
        if (ps >= climit) break;
        const long long pe = a.ptr[c + 1];
        const bool is_long = pe - ps > SPG_SEG;
        for (long long s = 0; s == 0 || (ps + s * SPG_SEG < pe && ps + s * SPG_SEG < e1); s++) {
            const long long st = ps + s * SPG_SEG;
            segment(c, s, st, st + SPG_SEG < pe ? st + SPG_SEG : pe, is_long);
        }
    }
}

// One workgroup per long column longc[b] (more than SPG_SEG stored entries): its segment sums added in segment order
template <int KP>
__global__ __launch_bounds__(256) void sp_gram_fixup_kernel(const SpGramArgs a, const int *__restrict__ longc)
{
    const int c = longc[blockIdx.x];
    const long long ns = (a.ptr[c + 1] - a.ptr[c] + SPG_SEG - 1) / SPG_SEG;
    const double *src = a.seg + (size_t)(a.segoff[c] - a.segoff[a.c0]) * KP * KP;
    double *out = a.G + (size_t)(c - a.c0) * KP * KP;
    for (int e = threadIdx.x; e < KP * KP; e += 256) {
        if (e / KP > e % KP) continue; // (upper triangle only)
        double v = src[e];
        for (long long t = 1; t < ns; t++) v += src[(size_t)t * KP * KP + e];
        if (a.Gfull) v += a.Gfull[e]; // (weighted form, absent entries zeros: + the shared Gram, once)
        out[e] = v;
    }
}

// Error sums over the stored entries when absent entries are missing (src/nnmf.cpp:124-125, :169-170): s = {S1, S2, S3} of
// sp_errors_kernel<T, LW, true> (S2 = sum of wh over the stored entries) -> out[0] = S1, out[1] = S3 + S2.  The Grams play no part.
__global__ void sp_err_final_missing_kernel(const double *__restrict__ s, double *__restrict__ out)
{
    if (threadIdx.x == 0) {
        out[0] = s[0];
        out[1] = s[2] + s[1];
    }
}
