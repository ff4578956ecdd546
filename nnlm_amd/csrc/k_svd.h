// k_svd.h -- the small kernels of nnlm_svd / nnlm_set_factors_nndsvd.  The passes over A of the randomised
// subspace iteration are the existing cross products (k_xprod16.h / k_xprod.h / k_sparse.h) and its l x l Grams the existing
// gram_partial_kernel + fold (k_gram.h); what is new is what touches the l x ld factor masters only:
//   svd_rotate_kernel   X <- T X for a host-built l x l matrix T (the Gram-based orth, U = V^T Q, Vt = S^-1 V^T B)
//   nndsvd_norms_kernel per component the sums of squares of the positive and negative parts of u_j and v_j (+ its fold)
//   nndsvd_build_kernel the non-negative start written into the factor masters and the fp32 operand copy of W
//   svd_sum_kernel      one fixed-order fp64 sum of the resident values of A (mean(A) of the nndsvda fill) (+ its fold)
// Every kernel takes the padded rank LP at run time, keeps no per-thread array (no scratch), uses no atomics: two calls give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include "tu_svd.h" // NndsvdRow

#define SVD_ROT_COLS 32     // widest column tile of svd_rotate_kernel (narrower ones: 16, 8)
#define SVD_ROT_THREADS 256 // CB columns x 256 / CB row groups
#define SVD_CHUNK 1024      // elements of a line per workgroup of nndsvd_norms_kernel
#define SVD_SUM_CHUNK 4096  // values per workgroup of svd_sum_kernel

// X [LP][ld] fp64, T [LP][LP] row-major (rows and columns >= l are zero).  A workgroup reads its CB columns of X (CB = 32, 16 or 8: the
// tile narrows as LP grows, so that the LDS stays bounded) once into LDS, then forms out[i][c] = sum_j T[i][j] X[j][c], j ascending, for
// RB rows of T at a time (T's rows pass through LDS in chunks of RB), and writes every row of its columns once.  Columns >= ncols
// (padding) are written as zeros.  Dynamic LDS: (LP * CB + RB * LP) doubles.  The sum of an entry is the same chain of fma in every
// form (this kernel at any CB and RB, svd_rotate_global_kernel): the forms give identical bits.
__global__ __launch_bounds__(SVD_ROT_THREADS) void svd_rotate_kernel(double *__restrict__ X, int ld, int ncols, int LP, int RB, int CB,
                                                                    const double *__restrict__ T)
{
    extern __shared__ double svd_lds[];
    double *xs = svd_lds;                    // [LP][CB]
    double *ts = svd_lds + (size_t)LP * CB;  // [RB][LP]
    const int cg = threadIdx.x & (CB - 1), rg = threadIdx.x / CB, nrg = SVD_ROT_THREADS / CB;
    const int c = blockIdx.x * CB + cg;
    // (ld is a multiple of CB and the grid is ld / CB: c < ld in every thread)
    for (int j = rg; j < LP; j += nrg) xs[j * CB + cg] = X[(size_t)j * ld + c];
    for (int r0 = 0; r0 < LP; r0 += RB) {
        const int rows = LP - r0 < RB ? LP - r0 : RB;
        __syncthreads(); // (xs is complete; the previous chunk of T is no longer read)
        for (int e = threadIdx.x; e < rows * LP; e += SVD_ROT_THREADS) ts[e] = T[(size_t)r0 * LP + e];
        __syncthreads();
        for (int i = rg; i < rows; i += nrg) {
            const double *t = ts + (size_t)i * LP;
            double s = 0.0;
            for (int j = 0; j < LP; j++) s = fma(t[j], xs[j * CB + cg], s);
            X[(size_t)(r0 + i) * ld + c] = c < ncols ? s : 0.0;
        }
    }
}

// The same product out of place, for an LP whose narrowest tile does not fit the LDS of a CU (LP > 1280): Y = T X, no LDS, every entry
// of X read LP times through the caches; the caller copies Y back.  grid (ld / 256, LP).
__global__ __launch_bounds__(256) void svd_rotate_global_kernel(const double *__restrict__ X, int ld, int ncols, int LP, const double *__restrict__ T,
                                                               double *__restrict__ Y)
{
    const int i = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ld) return;
    const double *t = T + (size_t)i * LP;
    double s = 0.0;
    for (int j = 0; j < LP; j++) s = fma(t[j], X[(size_t)j * ld + c], s);
    Y[(size_t)i * ld + c] = c < ncols ? s : 0.0;
}

// Fixed-order sum of the 256 values of a workgroup: pairwise through LDS, the same tree in every call.  red [256].
__device__ static inline double svd_block_sum(double v, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// grid (nb, k): block (b, j) sums the squares of the positive and of the negative entries of u_j (U [LP][ldu], n entries) and of v_j
// (Vt [LP][ldv], m entries) over the elements [b SVD_CHUNK, (b + 1) SVD_CHUNK) of both lines: part[(j nb + b) 4 + {0: u+, 1: u-, 2: v+, 3: v-}]
__global__ __launch_bounds__(256) void nndsvd_norms_kernel(const double *__restrict__ U, int ldu, int n, const double *__restrict__ Vt, int ldv, int m,
                                                          double *__restrict__ part)
{
    __shared__ double red[256];
    const int j = blockIdx.y, nb = gridDim.x;
    double up = 0.0, un = 0.0, vp = 0.0, vn = 0.0;
    for (int i = 0; i < SVD_CHUNK / 256; i++) {
        const int c = blockIdx.x * SVD_CHUNK + i * 256 + threadIdx.x;
        if (c < n) {
            const double x = U[(size_t)j * ldu + c];
            if (x > 0.0) up = fma(x, x, up);
            else un = fma(x, x, un);
        }
        if (c < m) {
            const double x = Vt[(size_t)j * ldv + c];
            if (x > 0.0) vp = fma(x, x, vp);
            else vn = fma(x, x, vn);
        }
    }
    up = svd_block_sum(up, red);
    un = svd_block_sum(un, red);
    vp = svd_block_sum(vp, red);
    vn = svd_block_sum(vn, red);
    if (threadIdx.x == 0) {
        double *o = part + ((size_t)j * nb + blockIdx.x) * 4;
        o[0] = up, o[1] = un, o[2] = vp, o[3] = vn;
    }
}

// out[e] = sum over b < nb of part[(e / width) * nb * width + b * width + e % width], b ascending: folds the per-block partial sums of
// nndsvd_norms_kernel (width 4, one group per component) and of svd_sum_kernel (width 1, one group)
__global__ __launch_bounds__(256) void svd_fold_kernel(const double *__restrict__ part, int nb, int width, int cnt, double *__restrict__ out)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= cnt) return;
    const double *p = part + (size_t)(e / width) * nb * width + e % width;
    double s = 0.0;
    for (int b = 0; b < nb; b++) s += p[(size_t)b * width];
    out[e] = s;
}

// grid (ceil(max(ldw, ldh) / 256), rows): row r of W64 [..][ldw] and H64 [..][ldh] from triplet rows[r].src of U / Vt, entries >= n / m
// (padding) zero; fill > 0 (nndsvda) replaces every exact zero of the n / m true entries of a row with src >= 0.  Wop (fp32-operand
// mode, else NULL): the fp32 copy of W beside its master, what nnlm_set_factors leaves.
__global__ __launch_bounds__(256) void nndsvd_build_kernel(const double *__restrict__ U, int ldu, const double *__restrict__ Vt, int ldv,
                                                          const NndsvdRow *__restrict__ rows, double fill, double *__restrict__ W64,
                                                          float *__restrict__ Wop, int ldw, int n, double *__restrict__ H64, int ldh, int m)
{
    const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    const NndsvdRow d = rows[r];
    if (c < ldw) {
        double w = 0.0;
        if (d.src >= 0 && c < n) {
            const double x = U[(size_t)d.src * ldu + c];
            const double a = d.side == 0 ? fabs(x) : (d.side > 0 ? fmax(x, 0.0) : fmax(-x, 0.0));
            w = d.su * a;
            if (w == 0.0) w = fill; // (also turns -0.0 into +0.0 when fill = 0)
        }
        W64[(size_t)r * ldw + c] = w;
        if (Wop) Wop[(size_t)r * ldw + c] = (float)w;
    }
    if (c < ldh) {
        double v = 0.0;
        if (d.src >= 0 && c < m) {
            const double x = Vt[(size_t)d.src * ldv + c];
            const double a = d.side == 0 ? fabs(x) : (d.side > 0 ? fmax(x, 0.0) : fmax(-x, 0.0));
            v = d.sv * a;
            if (v == 0.0) v = fill;
        }
        H64[(size_t)r * ldh + c] = v;
    }
}

// part[b] = sum of x[b SVD_SUM_CHUNK .. (b + 1) SVD_SUM_CHUNK) in fp64 (T: the resident type of A's values), fixed order
template <typename T>
__global__ __launch_bounds__(256) void svd_sum_kernel(const T *__restrict__ x, size_t cnt, double *__restrict__ part)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int i = 0; i < SVD_SUM_CHUNK / 256; i++) {
        const size_t e = (size_t)blockIdx.x * SVD_SUM_CHUNK + (size_t)i * 256 + threadIdx.x;
        if (e < cnt) s += (double)x[e];
    }
    s = svd_block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
