// tu_sparse.hip -- the instantiations of the sparse-A kernels (k_sparse.h, k_sparse_batch.h, k_sparse_na.h, k_sparse_na_batch.h, k_sparse_kl.h,
// k_sparse_kl_batch.h, k_sparse_ingest.h), see tu_sweepq.h.
#include "tu_sweepq.h"
#include "k_sparse.h"
#include "k_sparse_batch.h"
#include "k_sparse_na.h"
#include "k_sparse_na_batch.h"
#include "k_sparse_kl.h"
#include "k_sparse_kl_batch.h"
#include "k_sparse_ingest.h"
#include <cstdlib>

// Lanes per worker: KP = 16 -> four workers per wavefront, KP = 32 -> two, otherwise one (KP = 48 leaves 16 lanes idle; rank > 64 is
// launched once per 64 coordinates)
int nnlm_sp_lanes(int KP) { return KP == 16 ? 16 : (KP == 32 ? 32 : 64); }

// At least ~64 non-zeros per worker (the binary search that finds a worker's first column is then a small part of its time), at most
// 16 wavefronts per CU (four per SIMD: enough gathers in flight to cover the latency of the Infinity Cache)
int nnlm_sp_workers(long long nnz, int KP, int cus)
{
    const int ng = 64 / nnlm_sp_lanes(KP);
    long long waves = (nnz + 64LL * ng - 1) / (64LL * ng);
    const long long cap = 16LL * (cus > 0 ? cus : 256);
    if (waves > cap) waves = cap;
    if (waves < 1) waves = 1;
    return (int)waves * ng;
}

template <typename T, int LW> static void launch_spmm(const SpmmArgs &a, hipStream_t st)
{
    const int waves = a.nworkers / (64 / LW);
    spmm_kernel<T, LW><<<(waves + 3) / 4, 256, 0, st>>>(a);
    spmm_fixup_kernel<<<(a.nworkers + 3) / 4, 256, 0, st>>>(a);
}
template <typename T> static void launch_spmm_t(const SpmmArgs &a, hipStream_t st)
{
    switch (nnlm_sp_lanes(a.KP)) {
    case 16: launch_spmm<T, 16>(a, st); break;
    case 32: launch_spmm<T, 32>(a, st); break;
    default: launch_spmm<T, 64>(a, st); break;
    }
}
void nnlm_tu_spmm(const SpmmArgs &a, bool f64, hipStream_t st)
{
    if (f64) launch_spmm_t<double>(a, st);
    else launch_spmm_t<float>(a, st);
}

template <typename T, bool MISS>
static void launch_sp_errors_t(const long long *ptr, const int *idx, const void *val, int ncols, long long nnz, long long chunk, int nworkers,
                               const double *Wrow, int KP, int k, const double *H, int ldh, double *partial, int nblocks, hipStream_t st)
{
    const T *v = (const T *)val;
    switch (nnlm_sp_lanes(KP)) {
    case 16: sp_errors_kernel<T, 16, MISS><<<nblocks, 256, 0, st>>>(ptr, idx, v, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial); break;
    case 32: sp_errors_kernel<T, 32, MISS><<<nblocks, 256, 0, st>>>(ptr, idx, v, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial); break;
    default: sp_errors_kernel<T, 64, MISS><<<nblocks, 256, 0, st>>>(ptr, idx, v, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial); break;
    }
}
// nblocks = workgroups of four wavefronts covering the nworkers workers (the caller sizes `partial` from it: 3 doubles per workgroup)
void nnlm_tu_sp_errors(const long long *ptr, const int *idx, const void *val, bool f64, int ncols, long long nnz, long long chunk, int nworkers,
                       const double *Wrow, int KP, int k, const double *H, int ldh, double *partial, int nblocks, bool miss, hipStream_t st)
{
    if (f64 && miss) launch_sp_errors_t<double, true>(ptr, idx, val, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial, nblocks, st);
    else if (f64) launch_sp_errors_t<double, false>(ptr, idx, val, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial, nblocks, st);
    else if (miss) launch_sp_errors_t<float, true>(ptr, idx, val, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial, nblocks, st);
    else launch_sp_errors_t<float, false>(ptr, idx, val, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial, nblocks, st);
}

template <typename T>
static void launch_sp_errors_weighted_t(const long long *ptr, const int *idx, const void *val, const void *wt, int ncols, long long nnz, long long chunk,
                                        int nworkers, const double *Wrow, int KP, int k, const double *H, int ldh, double *partial, int nblocks,
                                        hipStream_t st)
{
    const T *v = (const T *)val, *c = (const T *)wt;
    switch (nnlm_sp_lanes(KP)) {
    case 16: sp_errors_weighted_kernel<T, 16><<<nblocks, 256, 0, st>>>(ptr, idx, v, c, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial); break;
    case 32: sp_errors_weighted_kernel<T, 32><<<nblocks, 256, 0, st>>>(ptr, idx, v, c, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial); break;
    default: sp_errors_weighted_kernel<T, 64><<<nblocks, 256, 0, st>>>(ptr, idx, v, c, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial); break;
    }
}
// (the caller sizes `partial`: 5 doubles per workgroup)
void nnlm_tu_sp_errors_weighted(const long long *ptr, const int *idx, const void *val, const void *wt, bool f64, int ncols, long long nnz,
                                long long chunk, int nworkers, const double *Wrow, int KP, int k, const double *H, int ldh, double *partial,
                                int nblocks, hipStream_t st)
{
    if (f64) launch_sp_errors_weighted_t<double>(ptr, idx, val, wt, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial, nblocks, st);
    else launch_sp_errors_weighted_t<float>(ptr, idx, val, wt, ncols, nnz, chunk, nworkers, Wrow, KP, k, H, ldh, partial, nblocks, st);
}
void nnlm_tu_sp_err_final_weighted(const double *s, const double *GW, const double *GH, const double *wsum, const double *hsum, int k, int KP,
                                   bool miss, double *out, hipStream_t st)
{
    sp_err_final_weighted_kernel<<<1, 256, 0, st>>>(s, GW, GH, wsum, hsum, k, KP, miss ? 1 : 0, out);
}

void nnlm_tu_sp_rowsums(const double *X, int ld, int ncols, int KP, double *partial, int nblocks, hipStream_t st)
{
    sp_rowsum_partial_kernel<<<nblocks, 256, 0, st>>>(X, ld, ncols, KP, partial);
}
void nnlm_tu_sp_err_final(const double *s, const double *GW, const double *GH, const double *wsum, const double *hsum, int k, int KP, double *out,
                          hipStream_t st)
{
    sp_err_final_kernel<<<1, 256, 0, st>>>(s, GW, GH, wsum, hsum, k, KP, out);
}

// ---- batched factorisation (k_sparse_batch.h) ----
// Wavefronts of sp_batch_errors_kernel: one per 64 x SPB_TILE non-zeros (rounded up), at most 16 per CU; nnlm_spb_chunk then gives each
// whole rows of 64, so the shares are not tiles (nnz = 257: two wavefronts, 192 + 65).  A function of nnz and the CU count only: the
// sums of a member do not depend on how many members or coordinates the batch holds.
int nnlm_spb_waves(long long nnz, int cus)
{
    long long waves = (nnz + 64LL * SPB_TILE - 1) / (64LL * SPB_TILE);
    const long long cap = 16LL * (cus > 0 ? cus : 256);
    if (waves > cap) waves = cap;
    if (waves < 1) waves = 1;
    return (int)waves;
}
// a wavefront's share of the non-zeros: whole rows of 64 (its lanes' reads stay aligned)
long long nnlm_spb_chunk(long long nnz, int nwaves)
{
    const long long c = (nnz + nwaves - 1) / nwaves;
    return c < 1 ? 64 : (c + 63) / 64 * 64;
}
// partial: [3 B][nblk], nblk = (nwaves + 3) / 4 workgroups
void nnlm_tu_sp_batch_errors(const long long *ptr, const int *idx, const void *val, bool f64, int ncols, long long nnz, long long chunk, int nwaves,
                             const double *Wrow, const double *Hrow, int KP, const int *off, int B, unsigned long long amask, double *partial,
                             hipStream_t st)
{
    const int nblk = (nwaves + 3) / 4;
    if (f64)
        sp_batch_errors_kernel<double><<<nblk, 256, 0, st>>>(ptr, idx, (const double *)val, ncols, nnz, chunk, nwaves, Wrow, Hrow, KP, off, B, amask,
                                                             partial, nblk);
    else
        sp_batch_errors_kernel<float><<<nblk, 256, 0, st>>>(ptr, idx, (const float *)val, ncols, nnz, chunk, nwaves, Wrow, Hrow, KP, off, B, amask,
                                                            partial, nblk);
}
void nnlm_tu_sp_batch_final(const double *s, const double *GW, const double *GH, const double *wsum, const double *hsum, const int *off, int B, int KP,
                            unsigned long long amask, double *out, hipStream_t st)
{
    sp_batch_final_kernel<<<B, 256, 0, st>>>(s, GW, GH, wsum, hsum, off, KP, amask, out);
}

// ---- absent entries missing (k_sparse_na.h) ----
int nnlm_spg_workers(long long nnz, int cus)
{
    long long w = (nnz + 255) / 256;
    const long long cap = 16LL * (cus > 0 ? cus : 256);
    if (w > cap) w = cap;
    if (w < 1) w = 1;
    return (int)w;
}

template <int NT> static void launch_sp_gram(const SpGramArgs &a, bool f64, hipStream_t st)
{
    const int nb = (a.nworkers + 3) / 4;
    if (a.wt) { // (per-entry weights: the WT form)
        if (f64) sp_gram_kernel<double, NT, true><<<nb, 256, 0, st>>>(a);
        else sp_gram_kernel<float, NT, true><<<nb, 256, 0, st>>>(a);
        return;
    }
    if (f64) sp_gram_kernel<double, NT><<<nb, 256, 0, st>>>(a);
    else sp_gram_kernel<float, NT><<<nb, 256, 0, st>>>(a);
}
void nnlm_tu_sp_gram(const SpGramArgs &a, int NKQ, bool f64, hipStream_t st)
{
    switch (NKQ) {
    case 1: launch_sp_gram<1>(a, f64, st); break;
    case 2: launch_sp_gram<2>(a, f64, st); break;
    case 3: launch_sp_gram<3>(a, f64, st); break;
    default: launch_sp_gram<4>(a, f64, st); break;
    }
}
void nnlm_tu_sp_gram_fixup(const SpGramArgs &a, const int *longc, int nlong, int KP, hipStream_t st)
{
    if (nlong <= 0) return;
    switch (KP) {
    case 16: sp_gram_fixup_kernel<16><<<nlong, 256, 0, st>>>(a, longc); break;
    case 32: sp_gram_fixup_kernel<32><<<nlong, 256, 0, st>>>(a, longc); break;
    case 48: sp_gram_fixup_kernel<48><<<nlong, 256, 0, st>>>(a, longc); break;
    default: sp_gram_fixup_kernel<64><<<nlong, 256, 0, st>>>(a, longc); break;
    }
}
void nnlm_tu_sp_err_final_missing(const double *s, double *out, hipStream_t st) { sp_err_final_missing_kernel<<<1, 64, 0, st>>>(s, out); }

// ---- batched factorisation, absent entries missing (k_sparse_na_batch.h) ----
template <int NT> static void launch_sp_gram_batch(const SpGramBatchArgs &a, bool f64, hipStream_t st)
{
    const int nb = (a.g.nworkers + 3) / 4;
    if (f64) sp_gram_batch_kernel<double, NT><<<nb, 256, 0, st>>>(a);
    else sp_gram_batch_kernel<float, NT><<<nb, 256, 0, st>>>(a);
}
void nnlm_tu_sp_gram_batch(const SpGramBatchArgs &a, int NT, bool f64, hipStream_t st)
{
    switch (NT) {
    case 1: launch_sp_gram_batch<1>(a, f64, st); break;
    case 2: launch_sp_gram_batch<2>(a, f64, st); break;
    case 3: launch_sp_gram_batch<3>(a, f64, st); break;
    default: launch_sp_gram_batch<4>(a, f64, st); break;
    }
}
void nnlm_tu_sp_gram_batch_fixup(const SpGramBatchArgs &a, const int *longc, int nlong, int KP, hipStream_t st)
{
    if (nlong <= 0) return;
    sp_gram_batch_fixup_kernel<<<nlong, 256, 0, st>>>(a, longc, KP);
}
void nnlm_tu_sp_batch_errors_missing(const long long *ptr, const int *idx, const void *val, bool f64, int ncols, long long nnz, long long chunk,
                                     int nwaves, const double *Wrow, const double *Hrow, int KP, const int *off, int B, unsigned long long amask,
                                     double *partial, hipStream_t st)
{
    const int nblk = (nwaves + 3) / 4;
    if (f64)
        sp_batch_errors_kernel<double, true><<<nblk, 256, 0, st>>>(ptr, idx, (const double *)val, ncols, nnz, chunk, nwaves, Wrow, Hrow, KP, off, B,
                                                                   amask, partial, nblk);
    else
        sp_batch_errors_kernel<float, true><<<nblk, 256, 0, st>>>(ptr, idx, (const float *)val, ncols, nnz, chunk, nwaves, Wrow, Hrow, KP, off, B,
                                                                  amask, partial, nblk);
}
void nnlm_tu_sp_batch_final_missing(const double *s, int B, unsigned long long amask, double *out, hipStream_t st)
{
    sp_batch_final_missing_kernel<<<(B + 63) / 64, 64, 0, st>>>(s, B, amask, out);
}

// ---- KL loss, absent entries zeros (k_sparse_kl.h) ----
int nnlm_spkl_short_max(void) { return SPKL_SHORT_MAX; }

template <int METHOD, typename T> static void launch_sp_kl(const SpKlArgs &a, int nshort, hipStream_t st)
{
    if (nshort > 0) sp_kl_solve_kernel<METHOD, T><<<(a.ncols + 3) / 4, 256, 0, st>>>(a);
    if (a.nlong > 0) sp_kl_solve_long_kernel<METHOD, T><<<a.nlong, 256, 0, st>>>(a);
}
void nnlm_tu_sp_kl(const SpKlArgs &a, int method, bool f64, int nshort, hipStream_t st)
{
    if (method == 3) {
        if (f64) launch_sp_kl<3, double>(a, nshort, st);
        else launch_sp_kl<3, float>(a, nshort, st);
    } else {
        if (f64) launch_sp_kl<4, double>(a, nshort, st);
        else launch_sp_kl<4, float>(a, nshort, st);
    }
}

void nnlm_tu_sp_kl_long(const SpKlArgs &a, int method, bool f64, hipStream_t st)
{
    if (a.nlong <= 0) return;
    if (method == 3) {
        if (f64) sp_kl_solve_long_kernel<3, double><<<a.nlong, 256, 0, st>>>(a);
        else sp_kl_solve_long_kernel<3, float><<<a.nlong, 256, 0, st>>>(a);
    } else {
        if (f64) sp_kl_solve_long_kernel<4, double><<<a.nlong, 256, 0, st>>>(a);
        else sp_kl_solve_long_kernel<4, float><<<a.nlong, 256, 0, st>>>(a);
    }
}

// ---- KL loss, batched (k_sparse_kl_batch.h) ----
int nnlm_spkl_batch_group(void)
{
    const char *e = getenv("NNLM_SPKL_BATCH_GROUP");
    const int g = e ? atoi(e) : SPKL_BATCH_G;
    return (g == 1 || g == 2 || g == 4) ? g : SPKL_BATCH_G;
}

template <int METHOD, typename T> static void launch_sp_kl_batch(const SpKlBatchArgs &a, int group, hipStream_t st)
{
    const int nb = (a.a.ncols + 3) / 4;
    switch (group) {
    case 1: sp_kl_batch_kernel<METHOD, T, 1><<<nb, 256, 0, st>>>(a); break;
    case 2: sp_kl_batch_kernel<METHOD, T, 2><<<nb, 256, 0, st>>>(a); break;
    default: sp_kl_batch_kernel<METHOD, T, 4><<<nb, 256, 0, st>>>(a); break;
    }
}
void nnlm_tu_sp_kl_batch(const SpKlBatchArgs &a, int method, bool f64, int group, hipStream_t st)
{
    if (method == 3) {
        if (f64) launch_sp_kl_batch<3, double>(a, group, st);
        else launch_sp_kl_batch<3, float>(a, group, st);
    } else {
        if (f64) launch_sp_kl_batch<4, double>(a, group, st);
        else launch_sp_kl_batch<4, float>(a, group, st);
    }
}

// ---- ingest of a sparse matrix in device memory (k_sparse_ingest.h) ----
int nnlm_spi_check_share(void) { return SPI_CHECK_SHARE; }
int nnlm_spi_sort_tile(void) { return SPI_SORT_TILE; }
int nnlm_spi_scan_tile(void) { return SPI_SCAN_TILE; }

void nnlm_tu_spi_ptr(const void *ptr, bool i64, int lines, long long nnz, long long *out, long long *blockmin, hipStream_t st)
{
    const int nb = (lines + SPI_THREADS) / SPI_THREADS; // lines + 1 pointers
    if (i64) spi_ptr_kernel<long long><<<nb, SPI_THREADS, 0, st>>>((const long long *)ptr, lines, nnz, out, blockmin);
    else spi_ptr_kernel<int><<<nb, SPI_THREADS, 0, st>>>((const int *)ptr, lines, nnz, out, blockmin);
}

// f(I{}, S{}) for the caller's index and value types
template <typename F> static void spi_with_types(bool i64, int dtype, F &&f)
{
    auto g = [&](auto i) {
        switch (dtype) {
        case 0: f(i, double{}); break;
        case 1: f(i, float{}); break;
        case 2: f(i, nnlm_f16{}); break;
        default: f(i, nnlm_bf16{}); break;
        }
    };
    if (i64) g((long long)0);
    else g((int)0);
}

void nnlm_tu_spi_check(const long long *ptr, int lines, const void *idx, bool i64, const void *val, int dtype, bool f64, long long nnz, long long other,
                       bool kl, int *idx_out, void *val_out, void *val_sort, int *line_out, long long *blockcode, double *blockstat, hipStream_t st)
{
    const int nb = (int)((nnz + SPI_CHECK_SHARE - 1) / SPI_CHECK_SHARE);
    spi_with_types(i64, dtype, [&](auto i, auto s) {
        typedef decltype(i) I;
        typedef decltype(s) S;
        if (f64)
            spi_check_kernel<I, S, double><<<nb, SPI_THREADS, 0, st>>>(ptr, lines, (const I *)idx, (const S *)val, nnz, other, kl ? 1 : 0, idx_out,
                                                                       (double *)val_out, (double *)val_sort, line_out, blockcode, blockstat);
        else
            spi_check_kernel<I, S, float><<<nb, SPI_THREADS, 0, st>>>(ptr, lines, (const I *)idx, (const S *)val, nnz, other, kl ? 1 : 0, idx_out,
                                                                      (float *)val_out, (float *)val_sort, line_out, blockcode, blockstat);
    });
}

void nnlm_tu_spi_fetch(const void *idx, bool i64, const void *val, int dtype, long long e, long long *i_out, double *v_out, hipStream_t st)
{
    spi_with_types(i64, dtype, [&](auto i, auto s) {
        typedef decltype(i) I;
        typedef decltype(s) S;
        spi_fetch_kernel<I, S><<<1, 1, 0, st>>>((const I *)idx, (const S *)val, e, i_out, v_out);
    });
}

void nnlm_tu_spi_count(const int *idx, long long nnz, long long *cnt, hipStream_t st)
{
    long long nb = (nnz + SPI_THREADS - 1) / SPI_THREADS;
    if (nb > 16384) nb = 16384;
    spi_count_kernel<<<(int)nb, SPI_THREADS, 0, st>>>(idx, nnz, (unsigned long long *)cnt);
}

void nnlm_tu_spi_scan(long long *x, long long len, long long *bsum, hipStream_t st)
{
    const int nb = (int)((len + SPI_SCAN_TILE - 1) / SPI_SCAN_TILE);
    spi_scan_sums_kernel<<<nb, SPI_THREADS, 0, st>>>(x, len, bsum);
    spi_scan_top_kernel<<<1, SPI_THREADS, 0, st>>>(bsum, nb);
    spi_scan_apply_kernel<<<nb, SPI_THREADS, 0, st>>>(x, len, bsum);
}

template <typename T>
static void spi_scatter(const int *kin, const int *lin, const void *vin, int *kout, int *lout, void *vout, long long nnz, int shift,
                        const long long *goff, int nb, const void *win, const void *ain, void *wout, void *aout, hipStream_t st)
{
    if (win)
        spi_scatter_kernel<T, true><<<nb, SPI_THREADS, 0, st>>>(kin, lin, (const T *)vin, kout, lout, (T *)vout, nnz, shift, goff, nb, (const T *)win,
                                                                (const T *)ain, (T *)wout, (T *)aout);
    else
        spi_scatter_kernel<T, false><<<nb, SPI_THREADS, 0, st>>>(kin, lin, (const T *)vin, kout, lout, (T *)vout, nnz, shift, goff, nb, nullptr, nullptr,
                                                                 nullptr, nullptr);
}

void nnlm_tu_spi_sort_pass(const int *kin, const int *lin, const void *vin, int *kout, int *lout, void *vout, bool f64, long long nnz, int shift,
                           long long *ghist, long long *bsum, hipStream_t st, const void *win, const void *ain, void *wout, void *aout)
{
    const int nb = (int)((nnz + SPI_SORT_TILE - 1) / SPI_SORT_TILE);
    spi_hist_kernel<<<nb, SPI_THREADS, 0, st>>>(kin, nnz, shift, ghist, nb);
    nnlm_tu_spi_scan(ghist, 256LL * nb, bsum, st);
    if (f64) spi_scatter<double>(kin, lin, vin, kout, lout, vout, nnz, shift, ghist, nb, win, ain, wout, aout, st);
    else spi_scatter<float>(kin, lin, vin, kout, lout, vout, nnz, shift, ghist, nb, win, ain, wout, aout, st);
}

void nnlm_tu_spi_pattern_ptr(const void *ptr, bool i64, const long long *ref, int lines, long long *blockmin, hipStream_t st)
{
    const int nb = (lines + SPI_THREADS) / SPI_THREADS; // lines + 1 pointers
    if (i64) spi_pattern_ptr_kernel<long long><<<nb, SPI_THREADS, 0, st>>>((const long long *)ptr, ref, lines, blockmin);
    else spi_pattern_ptr_kernel<int><<<nb, SPI_THREADS, 0, st>>>((const int *)ptr, ref, lines, blockmin);
}

void nnlm_tu_spi_pattern_idx(const void *idx, bool i64, const int *ref, long long nnz, long long *blockmin, hipStream_t st)
{
    const int nb = (int)((nnz + SPI_THREADS - 1) / SPI_THREADS);
    if (i64) spi_pattern_idx_kernel<long long><<<nb, SPI_THREADS, 0, st>>>((const long long *)idx, ref, nnz, blockmin);
    else spi_pattern_idx_kernel<int><<<nb, SPI_THREADS, 0, st>>>((const int *)idx, ref, nnz, blockmin);
}

void nnlm_tu_spi_wcheck(const void *val, int dtype, const void *wgt, int wdtype, bool f64, long long nnz, void *wt_out, void *wt_sort, void *wa_out,
                        void *wa_sort, long long *blockcode, double *blockstat, hipStream_t st)
{
    const int nb = (int)((nnz + SPI_CHECK_SHARE - 1) / SPI_CHECK_SHARE);
    spi_with_types(false, dtype, [&](auto, auto s) {
        spi_with_types(false, wdtype, [&](auto, auto c) {
            typedef decltype(s) S;
            typedef decltype(c) Cw;
            if (f64)
                spi_wcheck_kernel<S, Cw, double><<<nb, SPI_THREADS, 0, st>>>((const S *)val, (const Cw *)wgt, nnz, (double *)wt_out, (double *)wt_sort,
                                                                             (double *)wa_out, (double *)wa_sort, blockcode, blockstat);
            else
                spi_wcheck_kernel<S, Cw, float><<<nb, SPI_THREADS, 0, st>>>((const S *)val, (const Cw *)wgt, nnz, (float *)wt_out, (float *)wt_sort,
                                                                            (float *)wa_out, (float *)wa_sort, blockcode, blockstat);
        });
    });
}
