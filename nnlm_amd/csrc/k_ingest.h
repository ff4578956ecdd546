// k_ingest.h -- matrices and factors that already live in device memory (nnlm_set_matrix_device, nnlm_set_factors_device,
// nnlm_get_factors_device).  The resident state these kernels leave is the one the host upload leaves for the
// fp64 widening of the same values: A [mpad][npad] in the mode's type with 0 at the non-finite entries, the bit matrix `miss`, and the
// three sums of prep_convert_kernel (k_prep.h).
//   row_stride == 1 (R / Fortran order, tensor.t() of a C-contiguous tensor): ingest_cols_kernel = prep_convert_kernel reading the
//                    caller's type with leading dimension col_stride, over the host route's chunks and grid -> the same partial sums.
//   col_stride == 1 (C order, the default of the tensor libraries): ingest_rows_kernel, a transposition through LDS.
//   anything else:   ingest_gather_kernel = prep_convert_kernel with both strides: correct, uncoalesced, not meant to be fast.
// Traffic: n m (sizeof(S) + sizeof(T)) bytes + 1 bit per element; measured, the fp64 log of the KL constant bounds the two streaming
// routes at 0.2 - 0.55 of the copy rate.
#pragma once
#include "common.h"
#include "k_prep.h"

// (ingest_cols_kernel<S, T> is prep_convert_kernel<T, S, false>, ingest_gather_kernel<S, T> is prep_convert_kernel<T, S, true>: the
//  host code launches them under those names, ingest_fill in nnlm_mi355x.hip)

#define INGEST_TILE 64                 // rows (i) and columns (j) of one tile
#define INGEST_PITCH (INGEST_TILE + 1) // doubles per LDS row: lanes that walk i at a fixed j hit bank pairs 2 apart, no conflict
#define INGEST_GRID_Y 64

// src: element (i, j) at src[i * ld + j].  A workgroup walks the tiles (blockIdx.x, blockIdx.y + t gridDim.y) of 64 x 64 elements:
// rows are read along j in 16-byte pieces where the address allows it (vec: base and ld are multiples of 16 bytes; the piece lies
// inside the row), element by element otherwise -- coalesced along j either way --, widened to fp64 into the padded LDS tile, and
// written out along i: wavefront w takes the columns w, w + 4, ... of the tile, its 64 lanes the 64 rows, so the store of A is one
// contiguous run of 64 T and the two miss words of the run are one ballot.  Rows i >= n of the last row tile are written as zeros /
// not missing (gridDim.x covers npad); columns j >= m are not touched (the allocation zeroed them).
// partial: [gridDim.y * gridDim.x][3] as prep_convert_kernel leaves them, summed per block in a fixed order.
template <typename S, typename T>
__global__ __launch_bounds__(256) void ingest_rows_kernel(const S *__restrict__ src, size_t ld, int vec, int n, int m, T *__restrict__ dst,
                                                          int npad, uint32_t *__restrict__ miss, double *__restrict__ partial)
{
    constexpr int VEC = 16 / (int)sizeof(S);      // elements per 16-byte piece
    constexpr int PPR = INGEST_TILE / VEC;        // pieces per tile row
    __shared__ double tile[INGEST_TILE * INGEST_PITCH];
    __shared__ double red[3][4];
    struct alignas(16) Piece { S e[VEC]; };
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = blockIdx.x * INGEST_TILE;
    const int words = npad >> 5;
    const int tiles_j = (m + INGEST_TILE - 1) / INGEST_TILE;
    double cnt = 0.0, klc = 0.0, over = 0.0;
    for (int tj = blockIdx.y; tj < tiles_j; tj += gridDim.y) {
        const int j0 = tj * INGEST_TILE;
        for (int p = threadIdx.x; p < INGEST_TILE * PPR; p += 256) {
            const int ii = p / PPR, jj = (p % PPR) * VEC;
            const int i = i0 + ii, j = j0 + jj;
            double *t = tile + ii * INGEST_PITCH + jj;
            if (i < n && j + VEC <= m && vec) {
                const Piece pc = *reinterpret_cast<const Piece *>(src + ((size_t)i * ld + j));
#pragma unroll
                for (int e = 0; e < VEC; e++) t[e] = prep_load(&pc.e[e]);
            } else {
#pragma unroll
                for (int e = 0; e < VEC; e++) t[e] = (i < n && j + e < m) ? prep_load(src + ((size_t)i * ld + j + e)) : 0.0;
            }
        }
        __syncthreads();
        const int i = i0 + lane;
        for (int jj = wave; jj < INGEST_TILE && j0 + jj < m; jj += 4) {
            double v = tile[lane * INGEST_PITCH + jj];
            bool fin = true;
            if (i < n) {
                fin = isfinite(v);
                if (fin) {
                    cnt += 1.0;
                    klc += (v + NNLM_TINY) * log(v + NNLM_TINY) - v;
                    if (sizeof(T) == 4 && fabs(v) > 3.4028234663852886e38) over += 1.0;
                }
            }
            const size_t col = (size_t)(j0 + jj);
            dst[col * npad + i] = fin ? (T)v : (T)0;
            const unsigned long long b = __ballot(!fin);
            if (lane == 0) {
                miss[col * words + (i0 >> 5)] = (uint32_t)b;
                miss[col * words + (i0 >> 5) + 1] = (uint32_t)(b >> 32);
            }
        }
        __syncthreads();
    }
    cnt = wave_sum(cnt);
    klc = wave_sum(klc);
    over = wave_sum(over);
    if (lane == 0) {
        red[0][wave] = cnt;
        red[1][wave] = klc;
        red[2][wave] = over;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0, s = 0, o = 0;
        for (int w = 0; w < 4; w++) {
            c += red[0][w];
            s += red[1][w];
            o += red[2][w];
        }
        const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partial[3 * blk] = c;
        partial[3 * blk + 1] = s;
        partial[3 * blk + 2] = o;
    }
}

// Factor masters.  dst64: [KP][ld] fp64, row q = component q, column c = row of W / column of H; src: element (c, q) at
// src[c * sc + q * sq] (W n x k: sc = row_stride, sq = col_stride; H k x m: sc = col_stride, sq = row_stride).  Everything outside
// [0, ncols) x [0, k) is written as zero, as the host repack leaves it.  op32: the fp32 operand copy of W (F32 mode) or NULL.
// src == NULL: zeros.  grid (ld / 256, KP).
template <typename S>
__global__ __launch_bounds__(256) void factor_ingest_kernel(const S *__restrict__ src, long long sc, long long sq, int ncols, int k,
                                                            double *__restrict__ dst64, float *__restrict__ op32, int ld)
{
    const int c = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y;
    if (c >= ld) return;
    double v = 0.0;
    if (src && c < ncols && q < k) v = prep_load(src + ((size_t)c * (size_t)sc + (size_t)q * (size_t)sq));
    dst64[(size_t)q * ld + c] = v;
    if (op32) op32[(size_t)q * ld + c] = (float)v;
}

// The masters [.][ld] to the caller's strided n x k / k x m buffer of type D (double or float): element (c, q) to dst[c * sc + q * sq].
// Only the ncols x k entries are written: the gaps of a strided destination stay as they are.  grid (ceil(ncols / 256), k).
template <typename D>
__global__ __launch_bounds__(256) void factor_export_kernel(const double *__restrict__ src64, int ld, int ncols, D *__restrict__ dst,
                                                            long long sc, long long sq)
{
    const int c = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y;
    if (c >= ncols) return;
    dst[(size_t)c * (size_t)sc + (size_t)q * (size_t)sq] = (D)src64[(size_t)q * ld + c];
}

// check_k's bound for a matrix with missing entries: the fewest observed entries of any vector of a bit matrix.  bits: [nvec][words]
// (miss: the m columns, npad / 32 words each; missT: the n rows, mpad / 32 words each), len = entries of a vector (padding bits are 0).
// One wavefront per vector; out = min over the vectors of len - popcount (integer minimum: the order does not matter).  *out starts
// at INT_MAX.
__global__ __launch_bounds__(256) void observed_min_kernel(const uint32_t *__restrict__ bits, int nvec, int words, int len, int *__restrict__ out)
{
    const int v = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= nvec) return;
    long long c = 0;
    for (int w = lane; w < words; w += 64) c += __popc(bits[(size_t)v * words + w]);
    c = wave_sum_ll(c);
    if (lane == 0) atomicMin(out, len - (int)c);
}
