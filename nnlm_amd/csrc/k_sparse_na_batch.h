// k_sparse_na_batch.h -- per-column Grams of ALL members of a batch over the stored rows of a sparse A whose absent entries are missing
// (nnlm_set_matrix_csc_missing_batch + nnlm_run_batch).
//
// The members are stacked in the fixed factor's row copy Y [rows][KP] (member b owns coordinates off_b .. off_b + k_b - 1, KP = the
// stacked 16 NT).  A sequence of B solo half-steps gathers every stored row B times (sp_gram_kernel, k_sparse_na.h, is bound by its
// gathers); this kernel gathers it ONCE at the stacked width and forms only the members' diagonal blocks of the stacked Gram.
//
//   sp_gram_batch_kernel        sp_gram_kernel's work split, unchanged: a worker (one wavefront) owns a contiguous range of stored
//                               entries and sums every segment (SPG_SEG entries counted from the column's start) that starts in it, in
//                               groups of four stored rows on v_mfma_f64_16x16x4_f64, four groups' gathers in flight; no atomics.  Two
//                               additions, both wavefront-uniform kernel arguments made on the host from the ACTIVE members:
//                                 pairs  bit pi of the upper tile pairs (ta <= tb, ta-major): the pair meets some active member's
//                                        diagonal block [off_b, off_b + k_b)^2.  An unset pair issues no MFMA and is not written.
//                                 tiles  bit t: some set pair touches coordinate tile t.  An unset tile is not gathered.
//                               Epilogue: element (i, j), i <= j, is written only when i and j belong to the same active member b, to
//                               out[goff_b + (i - off_b) KP_b + (j - off_b)]: the member's Gram sits compactly at its own
//                               KP_b = 16 ceil(k_b / 16) inside the column's slot of sum_b KP_b^2 doubles, where the per-column solvers
//                               (launch_colsolve with g_stride = slot) find it.  tab[i] = the member of coordinate i (-1: none active),
//                               tab[64 + i] = goff_b + (i - off_b) KP_b - off_b, copied from the kernel arguments into LDS.
//                               Entries at i' or j' >= k_b of a member's KP_b x KP_b block are NOT written (in the stack those coordinates
//                               are a neighbour's); the solvers never read them (they read G[min][max] below k only).
//   sp_gram_batch_fixup_kernel  the long columns: their segment sums added in segment order, over the words the epilogue writes only.
//
// Contract: an entry of a member's Gram goes through the same sequence of fp64 FMAs as in a solo sp_gram_kernel run at rank k_b -- same
// segments, same groups of four rows (a row beyond the segment's end contributes +0 products in both), the same instruction, whose
// result element (i, j) is a chain over the group's four rows that depends on neither the element's place in the tile nor the other
// elements.  So it is bit-equal to the solo Gram, whatever the member's position, its neighbours, the worker count and the chunking.
#pragma once
#include "k_sparse_na.h"

template <typename T, int NT>
__global__ __launch_bounds__(256) void sp_gram_batch_kernel(const SpGramBatchArgs b)
{
    constexpr int KP = 16 * NT, NP = NT * (NT + 1) / 2;
    constexpr int GR = 4; // groups of four rows whose gathers are in flight together
    using M = Mfma<double>;
    __shared__ int tab[128];
    if (threadIdx.x < 128) tab[threadIdx.x] = b.tab[threadIdx.x];
    __syncthreads();
    const SpGramArgs &a = b.g;
    const int lane = threadIdx.x & 63, l15 = lane & 15, lg = lane >> 4;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.nworkers) return; // whole wavefront
    const T *Y = (const T *)a.Y;
    const long long E0 = a.ptr[a.c0], E1 = a.ptr[a.c1];
    long long e0 = E0 + (long long)w * a.chunk, e1 = e0 + a.chunk;
    if (e0 > E1) e0 = E1;
    if (e1 > E1) e1 = E1;
    auto segment = [&](int c, long long s, long long st, long long en, bool is_long) {
        typename M::acc_t acc[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) acc[i] = typename M::acc_t{0, 0, 0, 0};
        for (long long e = st; e < en; e += 4 * GR) {
            unsigned pairs = b.pairs, tiles = b.tiles;
            asm volatile("" : "+s"(pairs), "+s"(tiles)); // (opaque per step: the bit tests, hoisted, would each hold a 64-bit lane mask in SGPRs)
            int ri[GR];
#pragma unroll
            for (int u = 0; u < GR; u++) {
                const long long r = e + 4 * u + lg;
                ri[u] = r < en ? a.idx[r] : -1;
            }
            double y[GR][NT];
#pragma unroll
            for (int u = 0; u < GR; u++)
#pragma unroll
                for (int t = 0; t < NT; t++) y[u][t] = (((tiles >> t) & 1u) && ri[u] >= 0) ? (double)Y[(size_t)ri[u] * KP + 16 * t + l15] : 0.0;
#pragma unroll
            for (int u = 0; u < GR; u++) {
                int pi = 0;
#pragma unroll
                for (int ta = 0; ta < NT; ta++)
#pragma unroll
                    for (int tb = ta; tb < NT; tb++, pi++)
                        if ((pairs >> pi) & 1u) acc[pi] = M::mma(y[u][ta], y[u][tb], acc[pi]); // (uniform)
            }
        }
        double *out = is_long ? a.seg + (size_t)(a.segoff[c] - a.segoff[a.c0] + s) * b.slot : a.G + (size_t)(c - a.c0) * b.slot;
        unsigned pairs = b.pairs;
        asm volatile("" : "+s"(pairs));
        int pi = 0;
#pragma unroll
        for (int ta = 0; ta < NT; ta++)
#pragma unroll
            for (int tb = ta; tb < NT; tb++, pi++) {
                if (!((pairs >> pi) & 1u)) continue;
                const int j = 16 * tb + l15, mj = tab[j];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = 16 * ta + M::row_of(lane, r), mi = tab[i];
                    if (i <= j && mi >= 0 && mi == mj) out[tab[64 + i] + j] = acc[pi][r];
                }
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

// One workgroup per long column longc[blockIdx.x]: the segment sums of every word the epilogue writes, added in segment order (the
// order of sp_gram_fixup_kernel); KP = the stacked 16 NT
__global__ __launch_bounds__(256) void sp_gram_batch_fixup_kernel(const SpGramBatchArgs b, const int *__restrict__ longc, int KP)
{
    const SpGramArgs &a = b.g;
    const int c = longc[blockIdx.x];
    const long long ns = (a.ptr[c + 1] - a.ptr[c] + SPG_SEG - 1) / SPG_SEG;
    const double *src = a.seg + (size_t)(a.segoff[c] - a.segoff[a.c0]) * b.slot;
    double *out = a.G + (size_t)(c - a.c0) * b.slot;
    for (int e = threadIdx.x; e < KP * KP; e += 256) {
        const int i = e / KP, j = e % KP;
        if (i > j) continue; // (upper triangle only)
        const int mi = b.tab[i];
        if (mi < 0 || mi != b.tab[j]) continue;
        const int wd = b.tab[64 + i] + j;
        double v = src[wd];
        for (long long t = 1; t < ns; t++) v += src[(size_t)t * b.slot + wd];
        out[wd] = v;
    }
}
