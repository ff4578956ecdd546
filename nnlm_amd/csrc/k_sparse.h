// k_sparse.h -- the square-loss half-step and the error block on a sparse A (CSC + the CSR of the same matrix, resident).
//
// The solvers never read A: a half-step needs the Gram of the fixed factor (k_gram.h, unchanged) and the cross product with A,
// which on a sparse matrix is an SpMM over the non-zeros:
//   spmm_kernel        C[q][c] = sum over the non-zeros a_ic of column c of a_ic * Yrow[i][q]   (one slab of the layout the sweeps read)
//                      H half-step: CSC of A, Yrow = rows of W;  W half-step: CSR of A (= CSC of A^T), Yrow = rows of H.
//   spmm_fixup_kernel  the columns that straddle a worker boundary: owner's partial sum + the carries of the following workers, in order
//   sp_errors_kernel   sums over the non-zeros of (a - wh)^2, wh^2 and -(a + eps) log(wh + eps), wh = W[i,:] H[:,c] in fp64
//
// Work split.  A "worker" is a group of LW lanes (LW = 16, 32 or 64: KP = 16 puts four workers in a wavefront, KP = 32 two) and owns a
// contiguous range of NON-ZEROS, not of columns: a column holding half of all non-zeros is spread over half of the workers.  Lane l of
// a worker holds coordinate q = q0 + l.  A worker writes every column that STARTS in its range (empty ones included: zeros); the head of
// its range, when it continues a column that started earlier, goes to carry[w] instead; spmm_fixup_kernel adds those carries to the
// owner's partial in worker order.  No atomics: the result is a fixed function of the matrix, the factor and the worker count.
//
// Arithmetic: values and rows of the fixed factor are T (fp32 in the fp32-operand mode, fp64 in the strict one); the product of two
// fp32 numbers is exact in fp64, so both modes form every product in fp64 and accumulate in fp64.
#pragma once
#include "common.h"
#include "tu_sweepq.h"

#define SPMM_BATCH 8 // non-zeros whose index, value and row gather a worker has in flight at once

// (SpmmArgs and the launch entries: tu_sweepq.h)

// smallest c in [0, ncols] with ptr[c] >= e  (ptr[ncols] = nnz >= e)
__device__ static inline int sp_lower_bound(const long long *__restrict__ ptr, int ncols, long long e)
{
    int lo = 0, hi = ncols;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] < e) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__device__ static inline void sp_worker_range(long long nnz, long long chunk, int w, long long *e0, long long *e1)
{
    const long long b = (long long)w * chunk;
    *e0 = b < nnz ? b : nnz;
    *e1 = (b + chunk) < nnz ? b + chunk : nnz;
}

// sum over the non-zeros [s, t) of val[e] * Y[idx[e]][q]: indices and values of the next batch are loaded while the current batch's
// rows are gathered
template <typename T>
__device__ static inline double sp_segment(const int *__restrict__ idx, const T *__restrict__ val, const T *__restrict__ Y, int KP, int q, bool qv,
                                           long long s, long long t)
{
    double acc = 0.0;
    long long e = s;
    if (e + SPMM_BATCH <= t) {
        int ii[SPMM_BATCH];
        T vv[SPMM_BATCH];
#pragma unroll
        for (int u = 0; u < SPMM_BATCH; u++) ii[u] = idx[e + u], vv[u] = val[e + u];
        while (true) {
            T yy[SPMM_BATCH];
#pragma unroll
            for (int u = 0; u < SPMM_BATCH; u++) yy[u] = qv ? Y[(size_t)ii[u] * KP + q] : (T)0;
            const long long nx = e + SPMM_BATCH;
            const bool more = nx + SPMM_BATCH <= t;
            int ni[SPMM_BATCH];
            T nv[SPMM_BATCH];
#pragma unroll
            for (int u = 0; u < SPMM_BATCH; u++) {
                ni[u] = more ? idx[nx + u] : 0;
                nv[u] = more ? val[nx + u] : (T)0;
            }
#pragma unroll
            for (int u = 0; u < SPMM_BATCH; u++) acc = __builtin_fma((double)vv[u], (double)yy[u], acc);
            e = nx;
            if (!more) break;
#pragma unroll
            for (int u = 0; u < SPMM_BATCH; u++) ii[u] = ni[u], vv[u] = nv[u];
        }
    }
    for (; e < t; e++) {
        const int i = idx[e];
        const T v = val[e];
        const T y = qv ? Y[(size_t)i * KP + q] : (T)0;
        acc = __builtin_fma((double)v, (double)y, acc);
    }
    return acc;
}

template <typename T, int LW>
__global__ __launch_bounds__(256) void spmm_kernel(const SpmmArgs a)
{
    constexpr int NG = 64 / LW; // workers per wavefront
    const int lane = threadIdx.x & 63, ql = lane % LW;
    const int w = (blockIdx.x * 4 + (threadIdx.x >> 6)) * NG + lane / LW;
    if (w >= a.nworkers) return; // (uniform over the worker's lanes; nothing below crosses workers)
    const int q = a.q0 + ql;
    const bool qv = q < a.KP;
    const T *val = (const T *)a.val, *Y = (const T *)a.Y;
    long long e0, e1;
    sp_worker_range(a.nnz, a.chunk, w, &e0, &e1);
    int c = sp_lower_bound(a.ptr, a.ncols, e0);
    if (e0 < e1 && (c == a.ncols || a.ptr[c] > e0)) { // head: e0 lies inside column c - 1, which started in an earlier worker's range
        const long long t = a.ptr[c] < e1 ? a.ptr[c] : e1;
        const double acc = sp_segment<T>(a.idx, val, Y, a.KP, q, qv, e0, t);
        if (qv) a.carry[(size_t)w * 64 + ql] = acc;
    }
    // columns starting in [e0, e1); the last worker also owns the empty columns at the end (start = nnz)
    const long long climit = (w == a.nworkers - 1) ? a.nnz + 1 : e1;
    for (; c < a.ncols; c++) {
        const long long s = a.ptr[c];
        if (s >= climit) break;
        const long long nx = a.ptr[c + 1], t = nx < e1 ? nx : e1;
        const double acc = sp_segment<T>(a.idx, val, Y, a.KP, q, qv, s, t);
        if (qv) a.C[(size_t)q * a.ldc + c] = acc;
    }
}

// One wavefront per worker w.  If w is the FIRST worker whose range continues a column that started earlier, it adds the carries of w,
// w + 1, ... (every worker whose range lies in that column) to the owner's partial sum, in worker order.
__global__ __launch_bounds__(256) void spmm_fixup_kernel(const SpmmArgs a)
{
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= a.nworkers) return;
    long long e0, e1;
    sp_worker_range(a.nnz, a.chunk, w, &e0, &e1);
    if (e0 >= e1) return;
    const int c = sp_lower_bound(a.ptr, a.ncols, e0);
    if (c < a.ncols && a.ptr[c] == e0) return; // no head
    const int hc = c - 1;
    long long p0, p1;
    sp_worker_range(a.nnz, a.chunk, w - 1, &p0, &p1);
    if (a.ptr[hc] < p0) return; // the column started before the previous worker's range: that worker continues it too and does the sum
    const int q = a.q0 + lane;
    if (lane >= 64 || q >= a.KP) return;
    const long long cend = a.ptr[hc + 1];
    double acc = a.C[(size_t)q * a.ldc + hc];
    for (int v = w; v < a.nworkers; v++) {
        long long v0, v1;
        sp_worker_range(a.nnz, a.chunk, v, &v0, &v1);
        if (v0 >= v1 || v0 >= cend) break;
        acc += a.carry[(size_t)v * 64 + lane];
    }
    a.C[(size_t)q * a.ldc + hc] = acc;
}

// Error sums over the non-zeros (CSC): worker = LW lanes, lane l takes coordinates l, l + LW, ...; wh is reduced across the worker's
// lanes.  partial[block] = {sum (a - wh)^2, sum wh^2, sum -(a + eps) log(wh + eps)} (fixed order).  Wrow: [rows][KP] fp64 copy of W,
// H: [KP][ldh] master.  The sums over all n x m entries follow from the Grams and the factors' sums (sp_err_final_kernel).
// MISS (absent entries are missing, k_sparse_na.h): the second sum is sum wh -- the stored entries are all there is.
template <typename T, int LW, bool MISS = false>
__global__ __launch_bounds__(256) void sp_errors_kernel(const long long *__restrict__ ptr, const int *__restrict__ idx, const T *__restrict__ val,
                                                        int ncols, long long nnz, long long chunk, int nworkers, const double *__restrict__ Wrow,
                                                        int KP, int k, const double *__restrict__ H, int ldh, double *__restrict__ partial)
{
    constexpr int NG = 64 / LW;
    const int lane = threadIdx.x & 63, ql = lane % LW, wave = threadIdx.x >> 6;
    const int w = (blockIdx.x * 4 + wave) * NG + lane / LW;
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (w < nworkers) {
        long long e0, e1;
        sp_worker_range(nnz, chunk, w, &e0, &e1);
        if (e0 < e1) {
            int c = sp_lower_bound(ptr, ncols, e0 + 1) - 1; // the column holding e0 (last c with ptr[c] <= e0)
            long long cend = ptr[c + 1];
            for (long long e = e0; e < e1; e++) {
                while (e >= cend) cend = ptr[++c + 1];
                const int i = idx[e];
                double d = 0.0;
                for (int q = ql; q < k; q += LW) d = __builtin_fma(Wrow[(size_t)i * KP + q], H[(size_t)q * ldh + c], d);
#pragma unroll
                for (int o = LW / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, LW);
                if (ql == 0) {
                    const double av = (double)val[e];
                    const double r = av - d;
                    s1 = __builtin_fma(r, r, s1);
                    s2 = MISS ? s2 + d : __builtin_fma(d, d, s2);
                    s3 += -(av + NNLM_TINY) * nnlm_log_pos(d + NNLM_TINY);
                }
            }
        }
    }
    __shared__ double red[3][4];
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    s3 = wave_sum(s3);
    if (lane == 0) red[0][wave] = s1, red[1][wave] = s2, red[2][wave] = s3;
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        partial[3 * (size_t)blockIdx.x + c] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
    }
}

// partial[block][q] = sum of X[q][c] over the block's 2048 columns (X [KP][ld] fp64; rows q >= k are zero)
__global__ __launch_bounds__(256) void sp_rowsum_partial_kernel(const double *__restrict__ X, int ld, int ncols, int KP, double *__restrict__ partial)
{
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 2048 + threadIdx.x;
    for (int q = 0; q < KP; q++) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int c = c0 + 256 * u;
            if (c < ncols) s += X[(size_t)q * ld + c];
        }
        s = wave_sum(s);
        if (lane == 0) red[wave] = s;
        __syncthreads();
        if (threadIdx.x == 0) partial[(size_t)blockIdx.x * KP + q] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();
    }
}

// out[0] = S1 + max(0, <W^T W, H H^T> - S2)  (sum of squares over all n x m entries; the zeros contribute wh^2)
// out[1] = S3 + sum_q (sum_i W_iq)(sum_j H_qj)  (KL sum; the zeros' -eps log(wh + eps) <= 3.7e-15 per entry is left out)
// s = {S1, S2, S3}; GW, GH [KP][KP]; wsum, hsum [KP].  One block, fixed order.
// (thread 0 gets *G = <W^T W, H H^T> and *SW = sum_q wsum[q] hsum[q]; 256 threads, all of them call)
__device__ static inline void sp_err_final_sums(const double *__restrict__ GW, const double *__restrict__ GH, const double *__restrict__ wsum,
                                                const double *__restrict__ hsum, int k, int KP, double (*red)[4], double *G, double *SW)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double gg = 0.0, sw = 0.0;
    for (int e = threadIdx.x; e < k * k; e += 256) {
        const int a = e / k, b = e % k;
        gg = __builtin_fma(GW[(size_t)a * KP + b], GH[(size_t)a * KP + b], gg);
    }
    if (threadIdx.x < k) sw = wsum[threadIdx.x] * hsum[threadIdx.x];
    for (int q = threadIdx.x + 256; q < k; q += 256) sw = __builtin_fma(wsum[q], hsum[q], sw);
    gg = wave_sum(gg);
    sw = wave_sum(sw);
    if (lane == 0) red[0][wave] = gg, red[1][wave] = sw;
    __syncthreads();
    if (threadIdx.x == 0) {
        *G = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        *SW = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}
__global__ __launch_bounds__(256) void sp_err_final_kernel(const double *__restrict__ s, const double *__restrict__ GW, const double *__restrict__ GH,
                                                           const double *__restrict__ wsum, const double *__restrict__ hsum, int k, int KP,
                                                           double *__restrict__ out)
{
    __shared__ double red[2][4];
    double G = 0.0, SW = 0.0;
    sp_err_final_sums(GW, GH, wsum, hsum, k, KP, red, &G, &SW);
    if (threadIdx.x == 0) {
        const double zeros = G - s[1];
        out[0] = s[0] + (zeros > 0.0 ? zeros : 0.0);
        out[1] = s[2] + SW;
    }
}

// Per-entry weights (nnlm_set_matrix_csc_weighted): sp_errors_kernel with the weight c of each stored entry beside its value, same worker
// split and reduction order.  partial[block] = {sum c r^2, sum wh^2, sum c (-(a + eps) log(wh + eps)), sum c wh, sum wh}.  A weight of
// exactly 1 changes no bit of the sums it shares with sp_errors_kernel (c r, then fma(c r, r, s): 1 * r is exact).
template <typename T, int LW>
__global__ __launch_bounds__(256) void sp_errors_weighted_kernel(const long long *__restrict__ ptr, const int *__restrict__ idx,
                                                                 const T *__restrict__ val, const T *__restrict__ wt, int ncols, long long nnz,
                                                                 long long chunk, int nworkers, const double *__restrict__ Wrow, int KP, int k,
                                                                 const double *__restrict__ H, int ldh, double *__restrict__ partial)
{
    constexpr int NG = 64 / LW;
    const int lane = threadIdx.x & 63, ql = lane % LW, wave = threadIdx.x >> 6;
    const int w = (blockIdx.x * 4 + wave) * NG + lane / LW;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (w < nworkers) {
        long long e0, e1;
        sp_worker_range(nnz, chunk, w, &e0, &e1);
        if (e0 < e1) {
            int c = sp_lower_bound(ptr, ncols, e0 + 1) - 1; // the column holding e0 (last c with ptr[c] <= e0)
            long long cend = ptr[c + 1];
            for (long long e = e0; e < e1; e++) {
                while (e >= cend) cend = ptr[++c + 1];
                const int i = idx[e];
                double d = 0.0;
                for (int q = ql; q < k; q += LW) d = __builtin_fma(Wrow[(size_t)i * KP + q], H[(size_t)q * ldh + c], d);
#pragma unroll
                for (int o = LW / 2; o > 0; o >>= 1) d += __shfl_xor(d, o, LW);
                if (ql == 0) {
                    const double av = (double)val[e], cv = (double)wt[e];
                    const double r = av - d;
                    s[0] = __builtin_fma(cv * r, r, s[0]);
                    s[1] = __builtin_fma(d, d, s[1]);
                    const double ca = cv * (av + NNLM_TINY); // (the plain kernel's expression from here on: the same contraction)
                    s[2] += -ca * nnlm_log_pos(d + NNLM_TINY);
                    s[3] += cv * d;
                    s[4] += d;
                }
            }
        }
    }
    __shared__ double red[5][4];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        s[c] = wave_sum(s[c]);
        if (lane == 0) red[c][wave] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int c = threadIdx.x;
        partial[5 * (size_t)blockIdx.x + c] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
    }
}

// The error block of a weighted handle: s = the five sums of sp_errors_weighted_kernel.  miss: the stored entries are all there is.
// Otherwise an absent entry is a zero of weight 1: the sums over all n x m entries as in sp_err_final_kernel, the stored entries' own
// terms re-weighted (s3 - s4 = sum (c - 1) wh).
__global__ __launch_bounds__(256) void sp_err_final_weighted_kernel(const double *__restrict__ s, const double *__restrict__ GW,
                                                                    const double *__restrict__ GH, const double *__restrict__ wsum,
                                                                    const double *__restrict__ hsum, int k, int KP, int miss, double *__restrict__ out)
{
    __shared__ double red[2][4];
    double G = 0.0, SW = 0.0;
    if (!miss) sp_err_final_sums(GW, GH, wsum, hsum, k, KP, red, &G, &SW);
    if (threadIdx.x == 0) {
        if (miss) {
            out[0] = s[0];
            out[1] = s[2] + s[3];
        } else {
            const double zeros = G - s[1];
            out[0] = s[0] + (zeros > 0.0 ? zeros : 0.0);
            out[1] = (s[2] + SW) + (s[3] - s[4]);
        }
    }
}
