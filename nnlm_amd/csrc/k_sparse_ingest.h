// k_sparse_ingest.h -- the ingest of a sparse matrix that already lives in device memory (nnlm_set_matrix_sparse_device, DESIGN section
// 4.21): what set_matrix_csc_impl does on one host thread -- validate the compressed side, accumulate the range statistics and the KL
// constant, build the other side, convert the values -- as kernels over the caller's arrays.
//
// Ordering rule: no value read from the caller's arrays is used as an address before it has been checked, and the host learns the verdict
// of a stage before it launches the next one.
//   1. spi_ptr_kernel     reads the pointers alone (addresses: thread indices), writes their int64 copy and the first offending line;
//   2. spi_check_kernel   runs on pointers stage 1 has accepted (0 = ptr[0] <= ... <= ptr[lines] = nnz): entry numbers are in range by
//                         construction, the line of an entry comes from a search in the accepted pointers, idx[e] is COMPARED, never
//                         dereferenced.  Writes the narrowed indices, the converted values and the line of every entry;
//   3. spi_count_kernel,  run on indices stage 2 has accepted (0 <= idx < lines of the other side): the first kernels that use an
//      spi_hist_kernel,   index as an address.  The other side is a stable LSD radix sort of the entries by index (8-bit digits), the
//      spi_scatter_kernel line number and the value as payload; its pointers are the scan of the index histogram.
// Per-entry weights (nnlm_set_matrix_sparse_device_weighted) add, between stages 2 and 3 and under the same rule:
//   2a. spi_pattern_ptr_kernel, weights that bring a pattern of their own: their pointers, then (only when those are equal) their indices
//       spi_pattern_idx_kernel  are COMPARED with the accepted resident ones, never dereferenced;
//   2b. spi_wcheck_kernel       reads a weight per entry number (in range by construction), checks it, forms c a in fp64 and converts;
// and the sort carries the weights and the products as two more payloads of the same positions (spi_scatter_kernel<T, true>).
// Nothing here depends on scheduling: the only atomics are integer counters whose final value is order independent (the histograms), the
// rank of an entry inside a wavefront comes from ballots, the per-block results are reduced over a fixed tree and summed by the host in
// block order.
#pragma once
#include "common.h"
#include "k_prep.h"
#include <climits>

#define SPI_THREADS 256
#define SPI_CHECK_ITEMS 8
#define SPI_CHECK_SHARE (SPI_THREADS * SPI_CHECK_ITEMS) // entries per block of spi_check_kernel
#define SPI_SORT_ROUNDS 8
#define SPI_SORT_TILE (SPI_THREADS * SPI_SORT_ROUNDS)   // entries per block of spi_hist_kernel / spi_scatter_kernel
#define SPI_SCAN_ITEMS 8
#define SPI_SCAN_TILE (SPI_THREADS * SPI_SCAN_ITEMS)    // elements per block of the scan kernels
#define SPI_NONE LLONG_MAX                              // "no offender" of the per-block minima

// sh[0] = op over the block's values, fixed tree (SPI_THREADS threads); returns it to every thread
template <typename V, typename Op>
__device__ static inline V spi_block_reduce(V v, V *sh, Op op)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = SPI_THREADS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = op(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    const V r = sh[0];
    __syncthreads();
    return r;
}
struct SpiMin {
    __device__ long long operator()(long long a, long long b) const { return a < b ? a : b; }
};
struct SpiAdd {
    template <typename V> __device__ V operator()(V a, V b) const { return a + b; }
};
struct SpiMax {
    __device__ double operator()(double a, double b) const { return a > b ? a : b; }
};

// Stage 1.  ptr [lines + 1] in the caller's type -> out [lines + 1] int64; blockmin[b] = the smallest offence code of the block's
// pointers: 0 (ptr[0] != 0), 1 + j (ptr[j + 1] < ptr[j]), lines + 1 (ptr[lines] != nnz), SPI_NONE.  The smallest over all blocks is the
// host contract's first offender.
template <typename P>
__global__ __launch_bounds__(SPI_THREADS) void spi_ptr_kernel(const P *__restrict__ ptr, int lines, long long nnz, long long *__restrict__ out,
                                                              long long *__restrict__ blockmin)
{
    __shared__ long long sh[SPI_THREADS];
    const long long t = (long long)blockIdx.x * SPI_THREADS + threadIdx.x;
    long long bad = SPI_NONE;
    if (t <= lines) {
        const long long v = (long long)ptr[t];
        out[t] = v;
        if (t == lines && v != nnz) bad = (long long)lines + 1;
        if (t < lines && (long long)ptr[t + 1] < v) bad = 1 + t;
        if (t == 0 && v != 0) bad = 0;
    }
    bad = spi_block_reduce(bad, sh, SpiMin());
    if (threadIdx.x == 0) blockmin[blockIdx.x] = bad;
}

// The line j of [lo, hi) with ptr[j] <= e < ptr[j + 1]: the LAST line that starts at or before e (empty lines in front of it share its
// start and lose).  Needs ptr[lo] <= e < ptr[hi], ptr non-decreasing.
__device__ static inline int spi_line_of(const long long *__restrict__ ptr, int lo, int hi, long long e)
{
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (ptr[mid] <= e) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Stage 2 (and the conversions of stage 4: the values go to the mode's type T twice, into the given side's resident array and into the
// buffer the sort starts from).  Block b owns entries [b SPI_CHECK_SHARE, (b + 1) SPI_CHECK_SHARE): the
// work is split by entries, a line of any length costs what its entries cost.  Per entry the first violated rule in the host's order
// (csc_check): 0 index out of [0, other), 1 not above its predecessor in the line, 2 value not finite, 3 (kl) value negative;
// blockcode[b] = min(8 e + kind).  blockstat[b] = {entries with |v| > fp32 max, max |(float) v|, sum (v + eps) log(v + eps) - v}.
template <typename I, typename S, typename T>
__global__ __launch_bounds__(SPI_THREADS) void spi_check_kernel(const long long *__restrict__ ptr, int lines, const I *__restrict__ idx,
                                                                const S *__restrict__ val, long long nnz, long long other, int kl,
                                                                int *__restrict__ idx_out, T *__restrict__ val_out, T *__restrict__ val_sort,
                                                                int *__restrict__ line_out, long long *__restrict__ blockcode, double *__restrict__ blockstat)
{
    __shared__ long long shl[SPI_THREADS];
    __shared__ double shd[SPI_THREADS];
    __shared__ int sj[2];
    const long long e0 = (long long)blockIdx.x * SPI_CHECK_SHARE;
    const long long e1 = e0 + SPI_CHECK_SHARE < nnz ? e0 + SPI_CHECK_SHARE : nnz;
    if (threadIdx.x < 2) sj[threadIdx.x] = spi_line_of(ptr, 0, lines, threadIdx.x == 0 ? e0 : e1 - 1);
    __syncthreads();
    const int jlo = sj[0], jhi = sj[1];
    long long code = SPI_NONE;
    double over = 0.0, mx = 0.0, klc = 0.0;
    for (int it = 0; it < SPI_CHECK_ITEMS; it++) {
        const long long e = e0 + (long long)it * SPI_THREADS + threadIdx.x;
        if (e >= e1) continue;
        const int j = spi_line_of(ptr, jlo, jhi + 1, e);
        const long long i = (long long)idx[e];
        const double v = prep_load(val + e);
        int kind = -1;
        if (i < 0 || i >= other) kind = 0;
        else if (e > ptr[j] && i <= (long long)idx[e - 1]) kind = 1;
        else if (!isfinite(v)) kind = 2;
        else if (kl && v < 0.0) kind = 3;
        if (kind >= 0 && e * 8 + kind < code) code = e * 8 + kind;
        idx_out[e] = (int)i;
        val_out[e] = (T)v;
        val_sort[e] = (T)v;
        line_out[e] = j;
        if (fabs(v) > 3.4028234663852886e38) over += 1.0;
        const double fv = fabs((double)(float)v);
        if (fv > mx) mx = fv;
        klc += (v + NNLM_TINY) * log(v + NNLM_TINY) - v;
    }
    code = spi_block_reduce(code, shl, SpiMin());
    over = spi_block_reduce(over, shd, SpiAdd());
    mx = spi_block_reduce(mx, shd, SpiMax());
    klc = spi_block_reduce(klc, shd, SpiAdd());
    if (threadIdx.x == 0) {
        blockcode[blockIdx.x] = code;
        blockstat[3 * (size_t)blockIdx.x] = over;
        blockstat[3 * (size_t)blockIdx.x + 1] = mx;
        blockstat[3 * (size_t)blockIdx.x + 2] = klc;
    }
}

// The index and the value of entry e, widened: what the host needs to word a refusal
template <typename I, typename S>
__global__ void spi_fetch_kernel(const I *__restrict__ idx, const S *__restrict__ val, long long e, long long *__restrict__ i_out,
                                 double *__restrict__ v_out)
{
    *i_out = (long long)idx[e];
    *v_out = prep_load(val + e);
}

// Stage 2a.  The pointers of the weights' own pattern against the accepted ones (ref [lines + 1], int64), one thread per pointer:
// blockmin[b] = the smallest line whose extent differs -- pointer t > 0 differing means line t - 1 does (its start was equal or an
// earlier line already differs) -- or SPI_NONE.
template <typename P>
__global__ __launch_bounds__(SPI_THREADS) void spi_pattern_ptr_kernel(const P *__restrict__ ptr, const long long *__restrict__ ref, int lines,
                                                                      long long *__restrict__ blockmin)
{
    __shared__ long long sh[SPI_THREADS];
    const long long t = (long long)blockIdx.x * SPI_THREADS + threadIdx.x;
    long long bad = SPI_NONE;
    if (t <= lines && (long long)ptr[t] != ref[t]) bad = t > 0 ? t - 1 : 0;
    bad = spi_block_reduce(bad, sh, SpiMin());
    if (threadIdx.x == 0) blockmin[blockIdx.x] = bad;
}
// ... and, on equal pointers, its indices against the accepted resident int32 ones, one thread per entry: blockmin[b] = the smallest
// entry that differs, or SPI_NONE (the host finds its line in its copy of the pointers).
template <typename I>
__global__ __launch_bounds__(SPI_THREADS) void spi_pattern_idx_kernel(const I *__restrict__ idx, const int *__restrict__ ref, long long nnz,
                                                                      long long *__restrict__ blockmin)
{
    __shared__ long long sh[SPI_THREADS];
    const long long e = (long long)blockIdx.x * SPI_THREADS + threadIdx.x;
    long long bad = SPI_NONE;
    if (e < nnz && (long long)idx[e] != (long long)ref[e]) bad = e;
    bad = spi_block_reduce(bad, sh, SpiMin());
    if (threadIdx.x == 0) blockmin[blockIdx.x] = bad;
}

// Stage 2b: the weights, on entries stage 2 has accepted (every value finite).  Same shares as spi_check_kernel.  Per entry c = the weight
// and v = the value, each widened to fp64 from its own type, and c a = c * v, ONE fp64 multiply (the host's weight[e] * x[e]); c and c a
// go to the mode's type T twice, as the values do.  blockcode[b] = the first entry whose weight is not a finite number >= 0 (a code of
// its own: the host reads it only after stage 2 has found no offence of A), blockstat[b] = what the host loop adds for a weighted entry:
// {entries with |v| <= fp32 max and (|c a| > fp32 max or c > fp32 max), max |(float)(c a)|, sum c ((v + eps) log(v + eps) - v)}.
template <typename S, typename C, typename T>
__global__ __launch_bounds__(SPI_THREADS) void spi_wcheck_kernel(const S *__restrict__ val, const C *__restrict__ wgt, long long nnz,
                                                                 T *__restrict__ wt_out, T *__restrict__ wt_sort, T *__restrict__ wa_out,
                                                                 T *__restrict__ wa_sort, long long *__restrict__ blockcode,
                                                                 double *__restrict__ blockstat)
{
    __shared__ long long shl[SPI_THREADS];
    __shared__ double shd[SPI_THREADS];
    const long long e0 = (long long)blockIdx.x * SPI_CHECK_SHARE;
    const long long e1 = e0 + SPI_CHECK_SHARE < nnz ? e0 + SPI_CHECK_SHARE : nnz;
    long long code = SPI_NONE;
    double over = 0.0, wmx = 0.0, klc = 0.0;
    for (int it = 0; it < SPI_CHECK_ITEMS; it++) {
        const long long e = e0 + (long long)it * SPI_THREADS + threadIdx.x;
        if (e >= e1) continue;
        const double v = prep_load(val + e), c = prep_load(wgt + e);
        if ((!isfinite(c) || c < 0.0) && e < code) code = e;
        const double ca = c * v;
        wt_out[e] = (T)c;
        wt_sort[e] = (T)c;
        wa_out[e] = (T)ca;
        wa_sort[e] = (T)ca;
        if (fabs(v) <= 3.4028234663852886e38 && (fabs(ca) > 3.4028234663852886e38 || c > 3.4028234663852886e38)) over += 1.0;
        const double fca = fabs((double)(float)ca);
        if (fca > wmx) wmx = fca;
        klc += c * ((v + NNLM_TINY) * log(v + NNLM_TINY) - v);
    }
    code = spi_block_reduce(code, shl, SpiMin());
    over = spi_block_reduce(over, shd, SpiAdd());
    wmx = spi_block_reduce(wmx, shd, SpiMax());
    klc = spi_block_reduce(klc, shd, SpiAdd());
    if (threadIdx.x == 0) {
        blockcode[blockIdx.x] = code;
        blockstat[3 * (size_t)blockIdx.x] = over;
        blockstat[3 * (size_t)blockIdx.x + 1] = wmx;
        blockstat[3 * (size_t)blockIdx.x + 2] = klc;
    }
}

// Stage 3.  cnt[i] += entries with index i (cnt zeroed, [lines of the other side + 1]); its exclusive scan is the other side's pointers
__global__ __launch_bounds__(SPI_THREADS) void spi_count_kernel(const int *__restrict__ idx, long long nnz, unsigned long long *__restrict__ cnt)
{
    for (long long e = (long long)blockIdx.x * SPI_THREADS + threadIdx.x; e < nnz; e += (long long)gridDim.x * SPI_THREADS)
        atomicAdd(&cnt[idx[e]], 1ULL);
}

// Exclusive scan of x [len], in place, in three launches: bsum[b] = sum of tile b; bsum -> its exclusive scan (one block); every tile
// rescanned from its offset.
__global__ __launch_bounds__(SPI_THREADS) void spi_scan_sums_kernel(const long long *__restrict__ x, long long len, long long *__restrict__ bsum)
{
    __shared__ long long sh[SPI_THREADS];
    const long long b0 = (long long)blockIdx.x * SPI_SCAN_TILE + (long long)threadIdx.x * SPI_SCAN_ITEMS;
    long long s = 0;
    for (int q = 0; q < SPI_SCAN_ITEMS; q++)
        if (b0 + q < len) s += x[b0 + q];
    s = spi_block_reduce(s, sh, SpiAdd());
    if (threadIdx.x == 0) bsum[blockIdx.x] = s;
}
// exclusive prefix of v over the block's threads (Hillis-Steele in LDS)
__device__ static inline long long spi_block_exscan(long long v, long long *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < SPI_THREADS; d <<= 1) {
        const long long t = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += t;
        __syncthreads();
    }
    const long long r = sh[threadIdx.x] - v;
    __syncthreads();
    return r;
}
__global__ __launch_bounds__(SPI_THREADS) void spi_scan_top_kernel(long long *__restrict__ bsum, int nb)
{
    __shared__ long long sh[SPI_THREADS];
    const int per = (nb + SPI_THREADS - 1) / SPI_THREADS;
    const int q0 = (int)threadIdx.x * per, q1 = q0 + per < nb ? q0 + per : nb;
    long long s = 0;
    for (int q = q0; q < q1; q++) s += bsum[q];
    long long run = spi_block_exscan(s, sh);
    for (int q = q0; q < q1; q++) {
        const long long v = bsum[q];
        bsum[q] = run;
        run += v;
    }
}
__global__ __launch_bounds__(SPI_THREADS) void spi_scan_apply_kernel(long long *__restrict__ x, long long len, const long long *__restrict__ boff)
{
    __shared__ long long sh[SPI_THREADS];
    const long long b0 = (long long)blockIdx.x * SPI_SCAN_TILE + (long long)threadIdx.x * SPI_SCAN_ITEMS;
    long long v[SPI_SCAN_ITEMS], s = 0;
    for (int q = 0; q < SPI_SCAN_ITEMS; q++) {
        v[q] = b0 + q < len ? x[b0 + q] : 0;
        s += v[q];
    }
    long long run = boff[blockIdx.x] + spi_block_exscan(s, sh);
    for (int q = 0; q < SPI_SCAN_ITEMS; q++)
        if (b0 + q < len) {
            x[b0 + q] = run;
            run += v[q];
        }
}

// One radix pass over digit (key >> shift) & 255.  Block b owns entries [b SPI_SORT_TILE, (b + 1) SPI_SORT_TILE);
// ghist[d * nblocks + b] = its entries of digit d: scanned in that order (digit-major, block-minor) it is where the block's entries of
// digit d start in the output.
__global__ __launch_bounds__(SPI_THREADS) void spi_hist_kernel(const int *__restrict__ keys, long long nnz, int shift, long long *__restrict__ ghist,
                                                               int nblocks)
{
    __shared__ int hist[256];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * SPI_SORT_TILE;
    for (int r = 0; r < SPI_SORT_ROUNDS; r++) {
        const long long e = base + (long long)r * SPI_THREADS + threadIdx.x;
        if (e < nnz) atomicAdd(&hist[(keys[e] >> shift) & 255], 1);
    }
    __syncthreads();
    ghist[(size_t)threadIdx.x * nblocks + blockIdx.x] = hist[threadIdx.x];
}

// The stable scatter of the pass.  Wavefront w of the block owns SPI_SORT_ROUNDS rows of 64 consecutive entries; an entry of digit d lands
// at goff[d][b] + (entries of d in the wavefronts before w) + (entries of d in w's earlier rows) + (lanes below it in its row with d):
// input order within a digit, whatever the schedule.  The last term is a popcount over ballots.  kout == NULL: the last pass drops the keys.
// WT: the weights and the products c a (win, ain -> wout, aout) travel to the same positions as the values; otherwise the four are unused.
template <typename T, bool WT>
__global__ __launch_bounds__(SPI_THREADS) void spi_scatter_kernel(const int *__restrict__ kin, const int *__restrict__ lin, const T *__restrict__ vin,
                                                                  int *__restrict__ kout, int *__restrict__ lout, T *__restrict__ vout, long long nnz,
                                                                  int shift, const long long *__restrict__ goff, int nblocks,
                                                                  const T *__restrict__ win, const T *__restrict__ ain, T *__restrict__ wout,
                                                                  T *__restrict__ aout)
{
    constexpr int NW = SPI_THREADS / 64;
    __shared__ int wcnt[NW][256];
    __shared__ long long boff[256];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int q = 0; q < NW; q++) wcnt[q][threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * SPI_SORT_TILE + (long long)w * (64 * SPI_SORT_ROUNDS) + lane;
    int key[SPI_SORT_ROUNDS];
#pragma unroll
    for (int r = 0; r < SPI_SORT_ROUNDS; r++) {
        const long long e = base + r * 64;
        key[r] = e < nnz ? kin[e] : 0;
        if (e < nnz) atomicAdd(&wcnt[w][(key[r] >> shift) & 255], 1);
    }
    __syncthreads();
    {
        int run = 0;
        for (int q = 0; q < NW; q++) {
            const int c = wcnt[q][threadIdx.x];
            wcnt[q][threadIdx.x] = run;
            run += c;
        }
        boff[threadIdx.x] = goff[(size_t)threadIdx.x * nblocks + blockIdx.x];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SPI_SORT_ROUNDS; r++) {
        const long long e = base + r * 64;
        const bool valid = e < nnz;
        const int d = (key[r] >> shift) & 255;
        unsigned long long same = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1;
            const unsigned long long bal = __ballot(valid && bit);
            same &= bit ? bal : ~bal;
        }
        const int rank = __popcll(same & ((1ULL << lane) - 1ULL));
        long long pos = 0;
        if (valid) pos = boff[d] + wcnt[w][d] + rank;
        __syncthreads();
        if (valid && rank == 0) wcnt[w][d] += __popcll(same);
        __syncthreads();
        if (valid) {
            if (kout) kout[pos] = key[r];
            lout[pos] = lin[e];
            vout[pos] = vin[e];
            if constexpr (WT) {
                wout[pos] = win[e];
                aout[pos] = ain[e];
            }
        }
    }
}
