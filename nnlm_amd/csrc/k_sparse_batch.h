// k_sparse_batch.h -- the error block of a batched factorisation on a sparse A (nnlm_set_matrix_csc_batch + nnlm_run_batch): B
// square-loss models of ranks k_b, stacked in the factor buffers (member b owns coordinates off[b] .. off[b+1]-1), share ONE walk over
// the CSC per trace iteration.
//
//   sp_batch_errors_kernel  A LANE OWNS NON-ZEROS (sp_errors_kernel of k_sparse.h spends a worker of 16 to 64 lanes and a butterfly on
//                           each).  A wavefront owns a contiguous range of the non-zeros and takes it in tiles of 64 x SPB_TILE: lane l
//                           holds entries t + l, t + 64 + l, ... (coalesced index and value reads), their row, column and value in
//                           registers.  The column of a lane's first entry comes from a binary search (sp_lower_bound), the following
//                           ones from a walk, as in sp_errors_kernel.  Then, member after member (off_b, k_b and the mask bit are
//                           wavefront-uniform: no lane idles), wh = sum_q W[i, off_b + q] H[off_b + q, j] as a sequential fp64 FMA
//                           chain counted from the member's first coordinate, over the fp64 row copies Wrow [n][KP], Hrow [m][KP]
//                           (two contiguous reads of k_b doubles; the SPB_TILE chains of a lane are independent, their gathers
//                           overlap), one nnlm_log_pos per lane, entry and member, and the three sums
//                             S1 += (a - wh)^2,  S2 += wh^2,  S3 += -(a + eps) ln(wh + eps).
//                           Per member the tile's lane sums are folded across the wavefront (wave_sum) and added to the wavefront's
//                           slot in LDS in tile order; the block's four slots are added in order into partial[(3 b + t) nblk + blk] and
//                           batch_reduce_kernel (k_batch.h) adds the blocks in order.  No atomics, no scratch: nothing per member
//                           lives in registers beyond the tile's three sums, whatever B is.  The result is a fixed function of the
//                           matrix, the member's own coordinates and the wavefront count -- not of B, KP or where the member sits.
//   sp_batch_final_kernel   block b closes member b (sp_err_final_kernel's formula on the member's diagonal block of the stacked Grams
//                           and its own coordinate sums); members whose mask bit is clear are skipped.
//
// The wavefront count (nnlm_spb_waves) is a function of nnz and the CU count only.
#pragma once
#include "common.h"
#include "k_sparse.h"

#define SPB_TILE 4 // non-zeros a lane holds in registers across the member loop

// MISS (absent entries are missing, nnlm_set_matrix_csc_missing_batch): S2 += wh instead of wh^2, as sp_errors_kernel<T, LW, true>
template <typename T, bool MISS = false>
__global__ __launch_bounds__(256) void sp_batch_errors_kernel(const long long *__restrict__ ptr, const int *__restrict__ idx, const T *__restrict__ val,
                                                              int ncols, long long nnz, long long chunk, int nwaves,
                                                              const double *__restrict__ Wrow, const double *__restrict__ Hrow, int KP,
                                                              const int *__restrict__ off, int B, unsigned long long amask,
                                                              double *__restrict__ partial, int nblk)
{
    __shared__ double red[SPB_BATCH_MAX][4][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = blockIdx.x * 4 + wave;
    for (int b = lane; b < B; b += 64) red[b][wave][0] = red[b][wave][1] = red[b][wave][2] = 0.0; // (a wavefront's slots are its own)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // (lane 0 adds to slots its neighbours zeroed: order the two across lanes)
    __builtin_amdgcn_wave_barrier();
    long long e0 = 0, e1 = 0;
    if (w < nwaves) sp_worker_range(nnz, chunk, w, &e0, &e1);
    if (e0 < e1) { // (uniform over the wavefront)
        int c = 0;
        long long cend = 0;
        if (e0 + lane < e1) {
            c = sp_lower_bound(ptr, ncols, e0 + lane + 1) - 1; // the column holding the lane's first entry (last c with ptr[c] <= e)
            cend = ptr[c + 1];
        }
        for (long long t = e0; t < e1; t += 64 * SPB_TILE) {
            int ii[SPB_TILE], cc[SPB_TILE];
            double av[SPB_TILE];
            bool ok[SPB_TILE];
#pragma unroll
            for (int u = 0; u < SPB_TILE; u++) {
                const long long e = t + 64 * u + lane;
                ok[u] = e < e1;
                ii[u] = cc[u] = 0;
                av[u] = 0.0;
                if (ok[u]) {
                    while (e >= cend) cend = ptr[++c + 1]; // (e < nnz = ptr[ncols]: ends with c < ncols)
                    ii[u] = idx[e];
                    cc[u] = c;
                    av[u] = (double)val[e];
                }
            }
            for (int mb = 0; mb < B; mb++) {
                if (!((amask >> mb) & 1ull)) continue; // (uniform: frozen members are not summed)
                const int q0 = off[mb], kb = off[mb + 1] - q0;
                const double *wr[SPB_TILE], *hr[SPB_TILE];
                double wh[SPB_TILE];
#pragma unroll
                for (int u = 0; u < SPB_TILE; u++) {
                    wr[u] = Wrow + (size_t)ii[u] * KP + q0;
                    hr[u] = Hrow + (size_t)cc[u] * KP + q0;
                    wh[u] = 0.0;
                }
                for (int q = 0; q < kb; q++) {
#pragma unroll
                    for (int u = 0; u < SPB_TILE; u++) wh[u] = __builtin_fma(wr[u][q], hr[u][q], wh[u]);
                }
                double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
                for (int u = 0; u < SPB_TILE; u++) {
                    const double r = av[u] - wh[u];
                    const double lg = nnlm_log_pos(wh[u] + NNLM_TINY);
                    if (ok[u]) {
                        s1 = __builtin_fma(r, r, s1);
                        if (MISS) s2 += wh[u];
                        else s2 = __builtin_fma(wh[u], wh[u], s2);
                        s3 += -(av[u] + NNLM_TINY) * lg;
                    }
                }
                s1 = wave_sum(s1);
                s2 = wave_sum(s2);
                s3 = wave_sum(s3);
                if (lane == 0) {
                    red[mb][wave][0] += s1;
                    red[mb][wave][1] += s2;
                    red[mb][wave][2] += s3;
                }
            }
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < 3 * B; c += 256) {
        const int mb = c / 3, t = c % 3;
        partial[(size_t)c * nblk + blockIdx.x] = ((red[mb][0][t] + red[mb][1][t]) + red[mb][2][t]) + red[mb][3][t];
    }
}

// Member blockIdx.x, when its bit of amask is set (sp_err_final_kernel per member):
//   out[2 b]     = S1_b + max(0, <W_b^T W_b, H_b H_b^T> - S2_b)
//   out[2 b + 1] = S3_b + sum_q (sum_i W_iq)(sum_j H_qj) over the member's coordinates
// s [3 B] = {S1_b, S2_b, S3_b}; GW, GH [KP][KP] the Grams of the stacked factors (only the member's diagonal block is read); wsum, hsum
// [KP].  The sums run over the member's own coordinates counted from its first: a fixed order that does not depend on where it sits.
// (A member's block may straddle 16-row tiles; gram_reduce_kernel fills a lower tile from the mirrored upper one.  G(a, b) and G(b, a)
//  are sums of the same products x_a x_b over the columns in the same order, so the mirror holds the bits a direct sum would.)
__global__ __launch_bounds__(256) void sp_batch_final_kernel(const double *__restrict__ s, const double *__restrict__ GW, const double *__restrict__ GH,
                                                             const double *__restrict__ wsum, const double *__restrict__ hsum,
                                                             const int *__restrict__ off, int KP, unsigned long long amask,
                                                             double *__restrict__ out)
{
    __shared__ double red[2][4];
    const int mb = blockIdx.x;
    if (!((amask >> mb) & 1ull)) return; // (uniform over the block)
    const int q0 = off[mb], k = off[mb + 1] - q0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double gg = 0.0, sw = 0.0;
    for (int e = threadIdx.x; e < k * k; e += 256) {
        const int a = q0 + e / k, b = q0 + e % k;
        gg = __builtin_fma(GW[(size_t)a * KP + b], GH[(size_t)a * KP + b], gg);
    }
    if (threadIdx.x < k) sw = wsum[q0 + threadIdx.x] * hsum[q0 + threadIdx.x]; // (k <= 64)
    gg = wave_sum(gg);
    sw = wave_sum(sw);
    if (lane == 0) red[0][wave] = gg, red[1][wave] = sw;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double G = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        const double SW = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        const double zeros = G - s[3 * mb + 1];
        out[2 * mb] = s[3 * mb] + (zeros > 0.0 ? zeros : 0.0);
        out[2 * mb + 1] = s[3 * mb + 2] + SW;
    }
}

// Absent entries missing: member blockIdx.x * 64 + lane closes as sp_err_final_missing_kernel does (the Grams play no part)
__global__ void sp_batch_final_missing_kernel(const double *__restrict__ s, int B, unsigned long long amask, double *__restrict__ out)
{
    const int mb = blockIdx.x * 64 + threadIdx.x;
    if (mb >= B || !((amask >> mb) & 1ull)) return;
    out[2 * mb] = s[3 * mb];
    out[2 * mb + 1] = s[3 * mb + 2] + s[3 * mb + 1];
}
