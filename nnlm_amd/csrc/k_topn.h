// k_topn.h -- scores of a fitted model without W H: listed entries (predict_entries_kernel) and, per listed line, the n_top best
// candidates (topn_kernel + topn_merge_kernel).  DESIGN.md section 4.16.
//
// Both read fp64 row copies of the factors, [n][K4] and [m][K4] with K4 = 4 ceil(k / 4) and zeros behind k (factor_rows_kernel).
//
// topn_kernel.  A "line" is a listed column (by = 0) or row (by = 1), a "candidate" an index of the other side.  One wavefront owns 16
// lines for its whole life and a contiguous slice of the candidates; a workgroup is 1, 2 or 4 such wavefronts walking the SAME slice, so
// that a candidate tile fetched by one is an L1 hit for the others.  Per tile of 16 candidates:
//   * scores: K4 / 4 v_mfma_f64_16x16x4_f64 from a zero accumulator, M = candidate, N = line, coordinates in steps of four from 0.  An
//     entry of the result depends on its own operand rows only, so the bits of score (i, j) are a function of (i, j, W, H): not of the
//     slice, the tile's neighbours, the launch geometry or the lines asked for.  A lane ends with four candidates (lg + 4 r) of ONE line
//     (l15): the four lanes l15, l15 + 16, l15 + 32, l15 + 48 serve a line together and hold its state redundantly.
//   * exclusion: the line's stored candidates are a sorted list (the CSC column / CSR row of the resident matrix); a cursor walks it in
//     step with the tiles and marks the stored ones of this tile in a 16-bit word.  They are dropped BEFORE selection: a line that
//     stores half the matrix selects exactly as much as an empty one.
//   * selection: a score is compared in its accumulator register against the line's threshold, the score of its n_top-th best key at the
//     last prune (key = score descending, index ascending: a total order).  Candidates arrive in ascending index order and everything in
//     the buffer came from an earlier tile, so an equal score never beats the threshold and `score > threshold` is the whole test.
//     Survivors are appended to the line's buffer in LDS (positions from the four lanes' counts, no atomics).  A buffer that cannot take
//     16 more is pruned: every entry is ranked by counting the entries before it in the total order, the entry of rank n_top - 1
//     becomes the threshold, and the entries not behind it are compacted in place.
//   * end of slice: the buffer is ranked once more and written, best first, as the line's partial list of this slice.
// topn_merge_kernel: one wavefront per line, one lane per slice; n_top times the best head of the partial lists by the same total order.
// No barrier anywhere: a wavefront shares nothing with its neighbours, and LDS operations of one wavefront complete in order.
#pragma once
#include "common.h"
#include "tu_topn.h"

#include <climits>

__device__ static inline bool topn_before(double sa, int ia, double sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// sum of v over the lanes of this line in front of lane group lg, and over all four
__device__ static inline void topn_line_prefix(int v, int l15, int lg, int &before, int &total)
{
    before = total = 0;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int x = __shfl(v, l15 + 16 * g, 64);
        total += x;
        if (g < lg) before += x;
    }
}

// Every lane owns its own entries (as holdout_errors_kernel does): two contiguous row reads, one FMA chain in coordinate order, one store
__global__ __launch_bounds__(256) void predict_entries_kernel(const int *__restrict__ rows, const int *__restrict__ cols, long long count,
                                                              long long chunk, const double *__restrict__ Wrow, const double *__restrict__ Hrow,
                                                              int K4, int k, double *__restrict__ out)
{
    const long long e0 = (long long)blockIdx.x * chunk;
    long long e1 = e0 + chunk;
    if (e1 > count) e1 = count;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
        const double *w = Wrow + (size_t)rows[e] * K4, *x = Hrow + (size_t)cols[e] * K4;
        double wh = 0.0;
        for (int q = 0; q < k; q++) wh = __builtin_fma(w[q], x[q], wh);
        out[e] = wh;
    }
}

// Prune the 16 buffers of a wavefront (wave-uniform call).  A line with more than N entries keeps its best N; thr = score of the N-th
__device__ static inline void topn_prune(double *sc, int *ix, int N, int l15, int lg, int &cnt, bool &full, double &thr)
{
    const bool need = cnt > N;
    int found = 0, ti = 0;
    double ts = 0.0;
    if (need)
        for (int e = lg; e < cnt; e += 4) {
            const double se = sc[e];
            const int ie = ix[e];
            int rank = 0;
            for (int j = 0; j < cnt; j++) rank += topn_before(sc[j], ix[j], se, ie) ? 1 : 0;
            if (rank == N - 1) found = 1, ts = se, ti = ie;
        }
    double ths = 0.0;
    int thi = 0;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int f = __shfl(found, l15 + 16 * g, 64), i_ = __shfl(ti, l15 + 16 * g, 64);
        const double s_ = __shfl(ts, l15 + 16 * g, 64);
        if (f) ths = s_, thi = i_;
    }
    int cmax = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cmax = max(cmax, __shfl_xor(cmax, o, 64));
    // in place: round e0 reads entries e0 .. e0 + 3 (one LDS read of the whole wavefront) and then writes at or before them
    int kept = 0;
    for (int e0 = 0; e0 < cmax; e0 += 4) {
        const int e = e0 + lg;
        const bool v = need && e < cnt;
        const double se = v ? sc[e] : 0.0;
        const int ie = v ? ix[e] : 0;
        const int keep = v && !topn_before(ths, thi, se, ie);
        int before, total;
        topn_line_prefix(keep, l15, lg, before, total);
        if (keep) sc[kept + before] = se, ix[kept + before] = ie;
        kept += total;
    }
    if (need) cnt = kept, full = true, thr = ths;
}

template <int NS> // NS = K4 / 4 when the line rows stay in registers (1 .. TOPN_REG_STEPS), 0 = any rank
__global__ __launch_bounds__(256) void topn_kernel(const TopnArgs a)
{
    extern __shared__ double topn_lds[];
    constexpr int R = NS > 0 ? NS : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const int grp = blockIdx.y * nw + wave;
    if (grp * 16 >= a.nlines) return; // (the whole wavefront; the kernel has no barrier)
    const int ll = grp * 16 + l15;
    const bool lvalid = ll < a.nlines;
    const int line = lvalid ? (a.lines ? a.lines[ll] : a.line0 + ll) : 0;
    const int N = a.ntop, K4 = a.K4, ns = K4 >> 2;
    const int sstride = a.cap | 1; // (odd: the 16 lines of a wavefront start in different banks)
    double *sc = topn_lds + (size_t)(wave * 16 + l15) * sstride;
    int *ix = (int *)(topn_lds + (size_t)nw * 16 * sstride) + (size_t)(wave * 16 + l15) * a.cap;
    const int cs0 = blockIdx.x * a.slice_len;
    const int cs1 = min(cs0 + a.slice_len, a.ncand);

    const double *lp = a.Lrow + (size_t)line * K4 + lg;
    double lr[R];
    if (NS > 0) {
#pragma unroll
        for (int s = 0; s < NS; s++) lr[s] = lp[4 * s];
    }

    // cursor into the line's stored candidates: the first one at or behind the slice's start
    long long xp = 0, xe = 0;
    int nxt = INT_MAX;
    if (a.xptr && lvalid) {
        long long lo = a.xptr[line], hi = xe = a.xptr[line + 1];
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (a.xidx[mid] < cs0) lo = mid + 1;
            else hi = mid;
        }
        xp = lo;
        if (xp < xe) nxt = a.xidx[xp];
    }

    int cnt = 0;
    bool full = false;
    double thr = 0.0;
    double an[R];
    if (NS > 0 && cs0 < cs1) {
        const double *cp = a.Crow + (size_t)min(cs0 + l15, a.ncand - 1) * K4 + lg;
#pragma unroll
        for (int s = 0; s < NS; s++) an[s] = cp[4 * s];
    }
    for (int c0 = cs0; c0 < cs1; c0 += 16) {
        f64x4 acc = f64x4{0, 0, 0, 0};
        if (NS > 0) {
            double ac[R];
#pragma unroll
            for (int s = 0; s < NS; s++) ac[s] = an[s];
            if (c0 + 16 < cs1) { // the next tile's rows are in flight during this tile's matrix instructions
                const double *cp = a.Crow + (size_t)min(c0 + 16 + l15, a.ncand - 1) * K4 + lg;
#pragma unroll
                for (int s = 0; s < NS; s++) an[s] = cp[4 * s];
            }
#pragma unroll
            for (int s = 0; s < NS; s++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[s], lr[s], acc, 0, 0, 0); // M = candidate, N = line
        } else {
            const double *cp = a.Crow + (size_t)min(c0 + l15, a.ncand - 1) * K4 + lg;
            for (int s = 0; s < ns; s++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(cp[4 * s], lp[4 * s], acc, 0, 0, 0);
        }
        // stored candidates of this tile
        unsigned exm = 0;
        while (nxt < c0 + 16) {
            exm |= 1u << (nxt - c0);
            ++xp;
            nxt = xp < xe ? a.xidx[xp] : INT_MAX;
        }
        unsigned okm = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const double s = acc[r];
            const bool ok = lvalid && c0 + lg + 4 * r < cs1 && !((exm >> (lg + 4 * r)) & 1u) && s == s && (!full || s > thr);
            okm |= (ok ? 1u : 0u) << r;
        }
        if (__ballot(okm != 0) == 0) continue;
        if (__ballot(cnt + 16 > a.cap) != 0) {
            topn_prune(sc, ix, N, l15, lg, cnt, full, thr);
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (full && !(acc[r] > thr)) okm &= ~(1u << r);
        }
        int before, total;
        topn_line_prefix(__popc(okm), l15, lg, before, total);
        int at = cnt + before;
#pragma unroll
        for (int r = 0; r < 4; r++)
            if ((okm >> r) & 1u) {
                sc[at] = acc[r];
                ix[at] = c0 + lg + 4 * r;
                ++at;
            }
        cnt += total;
    }
    // the slice's partial list of this line: rank every entry, the best N go out in order
    if (!lvalid) return;
    double *ps = a.part_s + ((size_t)ll * a.nslices + blockIdx.x) * N;
    int *pi = a.part_i + ((size_t)ll * a.nslices + blockIdx.x) * N;
    for (int e = lg; e < cnt; e += 4) {
        const double se = sc[e];
        const int ie = ix[e];
        int rank = 0;
        for (int j = 0; j < cnt; j++) rank += topn_before(sc[j], ix[j], se, ie) ? 1 : 0;
        if (rank < N) ps[rank] = se, pi[rank] = ie;
    }
    for (int t = min(cnt, N) + lg; t < N; t += 4) ps[t] = __builtin_nan(""), pi[t] = -1;
}

// One wavefront per line, lane = slice (nslices <= 64): N rounds of "best head of the partial lists"
__global__ __launch_bounds__(256) void topn_merge_kernel(const double *__restrict__ part_s, const int *__restrict__ part_i, int nlines, int nslices, int N,
                                                         int *__restrict__ idx_out, double *__restrict__ score_out)
{
    const int lane = threadIdx.x & 63, ll = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ll >= nlines) return;
    const bool mine = lane < nslices;
    const double *ps = part_s + ((size_t)ll * nslices + (mine ? lane : 0)) * N;
    const int *pi = part_i + ((size_t)ll * nslices + (mine ? lane : 0)) * N;
    int head = 0;
    for (int t = 0; t < N; t++) {
        double s = 0.0;
        int i = -1; // (-1: this list is exhausted -- its padding has index -1 too)
        if (mine && head < N) i = pi[head], s = ps[head];
        double bs = s;
        int bi = i;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double os = __shfl_xor(bs, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oi >= 0 && (bi < 0 || topn_before(os, oi, bs, bi))) bs = os, bi = oi;
        }
        if (bi >= 0 && bi == i) ++head;
        if (lane == 0) {
            idx_out[(size_t)ll * N + t] = bi;
            score_out[(size_t)ll * N + t] = bi >= 0 ? bs : __builtin_nan("");
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Ranking metrics of the merged lists against held-out entries (nnlm_top_n_eval).  Nothing here computes a
// score: the kernels read the index lists topn_merge_kernel left in device memory.
//
// topn_eval_kernel: one wavefront per line, four lines per workgroup, nothing shared between them and no barrier.  Lane p looks list
// positions p and p + 64 up in the line's sorted held-out indices (a binary search each); two ballots give the 128 hit bits.  Lane c
// then serves cutoff c alone: hits by popcount under the cutoff's mask, dcg and apn by walking its set bits from the lowest -- the
// ascending-p order of the definitions, at most 128 fp64 additions each.  It writes the cutoff's three record values (when asked) and
// its six derived values into the line's slot of the round's partial; a line without held-out entries writes zeros and is not counted.
// topn_eval_reduce_kernel adds a column of the partial over the round's lines in a fixed shape and adds that to the call's sum: round
// after round on one stream, so the order is fixed and two calls give the same bits.
// ---------------------------------------------------------------------------------------------
// is c among idx[lo .. hi) (ascending)?
__device__ static inline bool topn_eval_held(const int *__restrict__ idx, long long lo, long long hi, int c)
{
    const long long end = hi;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (idx[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && idx[lo] == c;
}

// the bits of `b` (list positions base .. base + 63) from the lowest: one more hit each
__device__ static inline void topn_eval_walk(unsigned long long b, int base, const double *__restrict__ disc, int &h, double &dcg, double &apn)
{
    while (b) {
        const int p = base + __builtin_ctzll(b);
        b &= b - 1;
        ++h;
        dcg += disc[p];
        apn += (double)h / (double)(p + 1);
    }
}

__global__ __launch_bounds__(256) void topn_eval_kernel(const TopnEvalArgs a)
{
    const int lane = threadIdx.x & 63, ll = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ll >= a.nlines) return; // (the whole wavefront)
    const long long h0 = a.hptr[ll], h1 = a.hptr[ll + 1];
    const int t = (int)(h1 - h0);
    const int *L = a.idx + (size_t)ll * a.ntop;
    const int c0 = lane < a.ntop ? L[lane] : -1, c1 = lane + 64 < a.ntop ? L[lane + 64] : -1; // (padding is -1 too: it never hits)
    const unsigned long long b0 = __ballot(c0 >= 0 && topn_eval_held(a.hidx, h0, h1, c0));
    const unsigned long long b1 = __ballot(c1 >= 0 && topn_eval_held(a.hidx, h0, h1, c1));
    const int first = b0 ? __builtin_ctzll(b0) : (b1 ? 64 + __builtin_ctzll(b1) : -1);
    const int rw = 2 + 3 * a.ncut;
    if (lane == 0) {
        a.part[(size_t)6 * a.ncut * a.pstride + ll] = t > 0 ? 1.0 : 0.0;
        if (a.rec) a.rec[(size_t)ll * rw] = (double)t, a.rec[(size_t)ll * rw + 1] = (double)first;
    }
    if (lane >= a.ncut) return;
    int C = 0;
#pragma unroll
    for (int q = 0; q < TOPN_EVAL_MAX_CUT; q++)
        if (q == lane) C = a.cut[q]; // (constant indices: the argument block is never indexed by a register)
    const unsigned long long m0 = C >= 64 ? b0 : b0 & ((1ull << C) - 1ull);
    const unsigned long long m1 = C <= 64 ? 0ull : (C >= 128 ? b1 : b1 & ((1ull << (C - 64)) - 1ull));
    const int hits = __popcll(m0) + __popcll(m1);
    int h = 0;
    double dcg = 0.0, apn = 0.0;
    topn_eval_walk(m0, 0, a.disc, h, dcg, apn);
    topn_eval_walk(m1, 64, a.disc, h, dcg, apn);
    if (a.rec) {
        double *r = a.rec + (size_t)ll * rw + 2 + 3 * lane;
        r[0] = (double)hits, r[1] = dcg, r[2] = apn;
    }
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (t > 0) {
        const int best = min(C, t);
        v[0] = (double)hits / (double)C;
        v[1] = (double)hits / (double)t;
        v[2] = hits > 0 ? 1.0 : 0.0;
        v[3] = dcg / a.idcg[best];
        v[4] = apn / (double)best;
        v[5] = (first >= 0 && first < C) ? 1.0 / (double)(first + 1) : 0.0;
    }
#pragma unroll
    for (int s = 0; s < 6; s++) a.part[(size_t)(6 * lane + s) * a.pstride + ll] = v[s];
}

// acc[blockIdx.x] += sum over l < nlines of part[blockIdx.x pstride + l]: thread sums over l = tid (mod 256), the wavefront's lanes, the
// four wavefronts in order -- a shape that depends on nlines alone
__global__ __launch_bounds__(256) void topn_eval_reduce_kernel(const double *__restrict__ part, int pstride, int nlines, double *__restrict__ acc)
{
    __shared__ double red[4];
    const double *p = part + (size_t)blockIdx.x * pstride;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int b = threadIdx.x;
    for (; b + 768 < nlines; b += 1024) s0 += p[b], s1 += p[b + 256], s2 += p[b + 512], s3 += p[b + 768];
    for (; b < nlines; b += 256) s0 += p[b];
    const double s = wave_sum((s0 + s1) + (s2 + s3));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) acc[blockIdx.x] = acc[blockIdx.x] + (((red[0] + red[1]) + red[2]) + red[3]);
}

// exclude = 1: a held-out entry that the resident matrix stores could never be listed.  One wavefront per listed line; a lane takes
// every 64th held-out entry of the line and searches it among the line's stored indices; the entries ascend, so a lane's first find is
// its smallest.  The smallest (list position, index) key of all wins: an integer minimum on one word, whatever the order of arrival.
__global__ __launch_bounds__(256) void topn_eval_overlap_kernel(const int *__restrict__ lines, long long nlines, const long long *__restrict__ hptr,
                                                                const int *__restrict__ hidx, const long long *__restrict__ xptr,
                                                                const int *__restrict__ xidx, unsigned long long *first_key)
{
    const long long ll = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ll >= nlines) return;
    const int line = lines ? lines[ll] : (int)ll;
    const long long x0 = xptr[line], x1 = xptr[line + 1], h1 = hptr[ll + 1];
    if (x0 == x1) return;
    for (long long e = hptr[ll] + (threadIdx.x & 63); e < h1; e += 64) {
        const int c = hidx[e];
        if (topn_eval_held(xidx, x0, x1, c)) {
            atomicMin(first_key, ((unsigned long long)ll << 32) | (unsigned long long)(unsigned)c);
            break;
        }
    }
}
