// k_batch.h -- the error block of a batched factorisation (nnlm_run_batch): B independent models of ranks k_b share one resident A,
// their factors stacked in the resident layouts, member b owning rows off[b] .. off[b+1]-1 of W [KP][npad] and H [KP][mpad].
//
// errors_batch_kernel: ONE pass over A per trace iteration whatever B is.  A block of 4 wavefronts owns one 64-row i-tile (its K x 64
// slice of W staged in LDS once) and walks the j-tiles jt = blockIdx.y, blockIdx.y + gridDim.y, ...; each wavefront keeps its 32 x 32 piece of the A tile in registers (16
// entries per lane, loaded once) and, member after member, forms W_b^T H_b over that member's own row segment with
// v_mfma_f64_16x16x4_f64 (operand rows outside [off_b, off_b + k_b) are zero: no product crosses members), then adds
// (a - wh)^2 and -(a + eps) ln(wh + eps) + wh of its valid entries in fp64 (the logarithm as the solo error kernels of the mode take
// it).  Per-member wavefront sums accumulate in LDS, one slot per wavefront (no atomics); the block's sums go to
// partial[(2 b + t) nblk + blk] and batch_reduce_kernel adds the blocks in order.
// Bound: n m sizeof(T) bytes of A once, but B x (the MFMA steps of the member's segment + ~30 VALU slots) per entry: issue bound
// beyond a few members.
// NA = true (a hold-out handle): entries whose bit is set in miss [mpad][words] (bit i % 32 of word [j][i / 32]) are
// left out of both sums -- 16 word reads per lane and j-tile beside the 16 entries of A (the 16 lanes of a row group read the same
// word), kept as a 16-bit lane mask; the member loop is unchanged.
//
// holdout_errors_kernel: the two sums of every member over the HELD-OUT entries, a CSC of its own (row, column and value per entry).
// Block (x, b): member b over the entries [x chunk, (x + 1) chunk), a lane takes every 256th of them: wh = the dot over the member's k_b
// coordinates of row i of W and row j of H (row copies [n][K], [m][K]: two contiguous reads of k_b doubles), one logarithm, fp64
// throughout.  Lane sums, wave_sum, the four wavefronts in order, then batch_reduce_kernel over the blocks: a fixed order, no atomics.
// Bound: latency of the two gathered rows per entry (2 k_b 8 bytes); nothing n x m sized is touched.
#pragma once
#include "common.h"
#include "k_errors.h"

#define BATCH_MAX 64

template <typename T, bool NA = false>
__global__ __launch_bounds__(256) void errors_batch_kernel(const T *__restrict__ A, int lda, const double *__restrict__ W64, int ldw,
                                                           const double *__restrict__ H64, int ldh, int n, int m, const int *__restrict__ off,
                                                           int B, unsigned long long amask, double *__restrict__ partial, int nblk,
                                                           const uint32_t *__restrict__ miss = nullptr, int words = 0)
{
    using M = Mfma<double>;
    __shared__ double red[BATCH_MAX][4][2];
    __shared__ f64x2 ltab[64];
    __shared__ double wl[BATCH_MAX * 64]; // rows 0 .. K-1 of W over this block's 64 rows i of A: read from HBM once, not per j-tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, lg = lane >> 4;
    const int K = off[B];
    for (int e = threadIdx.x; e < B * 8; e += 256) (&red[0][0][0])[e] = 0.0;
    for (int e = threadIdx.x; e < K * 64; e += 256) wl[e] = W64[(size_t)(e >> 6) * ldw + blockIdx.x * 64 + (e & 63)];
    nnlm_log_tab_fill(ltab, threadIdx.x);
    __syncthreads();
    const int ib = blockIdx.x * 64 + 32 * (wave & 1), il = 32 * (wave & 1);
    const int mt = m > 0 ? (m + 63) / 64 : 0;
    for (int jt = blockIdx.y; jt < mt; jt += gridDim.y) {
        const int jb = jt * 64 + 32 * (wave >> 1);
        double av[2][2][4];
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++)
#pragma unroll
                for (int r = 0; r < 4; r++) av[a][b][r] = (double)A[(size_t)(jb + 16 * b + M::row_of(lane, r)) * lda + ib + 16 * a + l15];
        unsigned obs = 0xFFFFu; // NA: bit 8 a + 4 b + r = the lane's entry (a, b, r) is observed
        if constexpr (NA) {
            obs = 0u;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int i = ib + 16 * a + l15, j = jb + 16 * b + M::row_of(lane, r);
                        const uint32_t w = miss[(size_t)j * words + (i >> 5)];
                        obs |= (((w >> (i & 31)) & 1u) ^ 1u) << (8 * a + 4 * b + r);
                    }
        }
        for (int mb = 0; mb < B; mb++) {
            if (!((amask >> mb) & 1ull)) continue; // (uniform: frozen members are not summed)
            const int q0 = off[mb], q1 = off[mb + 1];
            f64x4 acc[2][2];
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) acc[a][b] = f64x4{0, 0, 0, 0};
            // (steps of four coordinates counted from the member's own first row: how its products are grouped into the 4-deep
            //  matrix instruction does not depend on where the member sits in the stack)
            for (int kq = q0; kq < q1; kq += 4) {
                const int q = kq + lg;
                const bool own = q < q1;
                double wa[2], hb[2];
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    wa[t] = own ? wl[(own ? q : q0) * 64 + il + 16 * t + l15] : 0.0;
                    hb[t] = own ? H64[(size_t)q * ldh + jb + 16 * t + l15] : 0.0;
                }
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int b = 0; b < 2; b++) acc[a][b] = M::mma(hb[b], wa[a], acc[a][b]); // M = column j, N = row i
            }
            double s2 = 0.0, skl = 0.0;
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int b = 0; b < 2; b++) {
                    const int i = ib + 16 * a + l15;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int j = jb + 16 * b + M::row_of(lane, r);
                        const double ah = acc[a][b][r], x = av[a][b][r];
                        bool valid = (i < n) && (j < m);
                        if constexpr (NA) valid = valid && ((obs >> (8 * a + 4 * b + r)) & 1u);
                        const double d = x - ah;
                        // ln(wh + eps): strict mode the table logarithm of errors64_kernel (absolute error ~2e-16); fp32-operand mode the
                        // native fp32 one of its own error kernels (relative 1e-7 per term) -- the per-member logarithm is this kernel's
                        // largest cost, B of them per entry
                        double lgv;
                        if constexpr (sizeof(T) == 4) lgv = (double)(log2_native((float)(ah + NNLM_TINY)) * NNLM_LN2F);
                        else lgv = nnlm_log_tab(ah + NNLM_TINY, ltab);
                        s2 += valid ? d * d : 0.0;
                        skl += valid ? (-(x + NNLM_TINY) * lgv + ah) : 0.0;
                    }
                }
            s2 = wave_sum(s2);
            skl = wave_sum(skl);
            if (lane == 0) {
                red[mb][wave][0] += s2;
                red[mb][wave][1] += skl;
            }
        }
    }
    __syncthreads();
    const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    for (int c = threadIdx.x; c < 2 * B; c += 256) {
        const int mb = c >> 1, t = c & 1;
        partial[(size_t)c * nblk + blk] = ((red[mb][0][t] + red[mb][1][t]) + red[mb][2][t]) + red[mb][3][t];
    }
}

// Penalty sums of every member of one stacked factor X [KP][ld] (src/nnmf.cpp:224-240), block (x, b): member b over columns
// [256 x, 256 x + 256) -> partial[(3 b + c) gridDim.x + x] = {sum x^2, sum_col (sum_q x[q,col])^2, sum x}
__global__ __launch_bounds__(256) void batch_penalty_kernel(const double *__restrict__ X, int ld, int ncols, const int *__restrict__ off,
                                                            double *__restrict__ partial)
{
    const int col = blockIdx.x * 256 + threadIdx.x, mb = blockIdx.y;
    const int q0 = off[mb], q1 = off[mb + 1];
    double sq = 0.0, cs = 0.0;
    if (col < ncols)
        for (int q = q0; q < q1; q++) {
            const double v = X[(size_t)q * ld + col];
            sq += v * v;
            cs += v;
        }
    double v3[3] = {sq, cs * cs, cs};
    __shared__ double red[3][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        v3[c] = wave_sum(v3[c]);
        if (lane == 0) red[c][wave] = v3[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        partial[(size_t)(3 * mb + c) * gridDim.x + blockIdx.x] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
    }
}

// out[c] = sum over b < nblk of partial[c nblk + b], block c, fixed order (lane-strided partial sums, then the wavefronts in order)
__global__ __launch_bounds__(256) void batch_reduce_kernel(const double *__restrict__ partial, int nblk, double *__restrict__ out)
{
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *p = partial + (size_t)blockIdx.x * nblk;
    double s = 0.0;
    for (int b = threadIdx.x; b < nblk; b += 256) s += p[b];
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Held-out sums of member blockIdx.y (see the head of this file).  off[b] .. off[b + 1] - 1: the member's coordinates in the row copies
// Wrow [n][K], Hrow [m][K]; partial[(2 b + t) gridDim.x + blockIdx.x] = the block's {sum (a - wh)^2, sum (a + eps) ln((a + eps) / (wh + eps)) - a + wh}
template <typename T>
__global__ __launch_bounds__(256) void holdout_errors_kernel(const int *__restrict__ ridx, const int *__restrict__ cidx, const T *__restrict__ val,
                                                             long long nnz, long long chunk, const double *__restrict__ Wrow,
                                                             const double *__restrict__ Hrow, int K, const int *__restrict__ off,
                                                             double *__restrict__ partial)
{
    __shared__ double red[2][4];
    const int mb = blockIdx.y, q0 = off[mb], kb = off[mb + 1] - q0;
    const long long e0 = (long long)blockIdx.x * chunk;
    long long e1 = e0 + chunk;
    if (e1 > nnz) e1 = nnz;
    double s2 = 0.0, skl = 0.0;
    for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
        const double *w = Wrow + (size_t)ridx[e] * K + q0, *x = Hrow + (size_t)cidx[e] * K + q0;
        double wh = 0.0;
        for (int q = 0; q < kb; q++) wh = __builtin_fma(w[q], x[q], wh);
        const double a = (double)val[e], d = a - wh;
        s2 += d * d;
        skl += (a + NNLM_TINY) * log((a + NNLM_TINY) / (wh + NNLM_TINY)) - a + wh;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    s2 = wave_sum(s2);
    skl = wave_sum(skl);
    if (lane == 0) red[0][wave] = s2, red[1][wave] = skl;
    __syncthreads();
    if (threadIdx.x < 2) {
        const int t = threadIdx.x;
        partial[(size_t)(2 * mb + t) * gridDim.x + blockIdx.x] = ((red[t][0] + red[t][1]) + red[t][2]) + red[t][3];
    }
}
