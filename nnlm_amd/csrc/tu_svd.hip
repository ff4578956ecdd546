// tu_svd.hip -- the instantiations of the kernels of k_svd.h, see tu_svd.h.
#include "k_svd.h"
#include "tu_svd.h"

// LDS of a workgroup: 64 KB without asking, the 160 KB of a CU at most.  The columns of X take LP * CB doubles; T's rows take the rest,
// all of them when everything fits 64 KB (ranks up to 64 at CB = 32: 48 KB), else as many as the larger grant holds (a multiple of 8).
static const size_t SVD_LDS_CAP = 160 * 1024;

int nnlm_svd_rotate_rows(int LP, int CB)
{
    const size_t xs = (size_t)LP * CB * 8, row = (size_t)LP * 8;
    if (xs + (size_t)LP * row <= 65536) return LP;
    if (xs + 8 * row > SVD_LDS_CAP) return 0;
    size_t rb = (SVD_LDS_CAP - xs) / row / 8 * 8;
    if (rb > (size_t)LP) rb = LP;
    return (int)rb;
}

size_t nnlm_svd_rotate_lds(int LP, int CB) { return ((size_t)LP * CB + (size_t)nnlm_svd_rotate_rows(LP, CB) * LP) * 8; }

int nnlm_svd_rotate_form(int LP)
{
    for (int cb = SVD_ROT_COLS; cb >= 8; cb >>= 1)
        if (nnlm_svd_rotate_rows(LP, cb) > 0) return cb;
    return 0;
}

hipError_t nnlm_tu_svd_rotate(double *X, int ld, int ncols, int LP, const double *T, int form, double *tmp, hipStream_t st)
{
    if (form == 0) {
        if (!tmp) return hipErrorInvalidValue;
        svd_rotate_global_kernel<<<dim3((ld + 255) / 256, LP), 256, 0, st>>>(X, ld, ncols, LP, T, tmp);
        return hipMemcpyAsync(X, tmp, (size_t)LP * ld * 8, hipMemcpyDeviceToDevice, st);
    }
    if (form != 32 && form != 16 && form != 8) return hipErrorInvalidValue;
    const int rb = nnlm_svd_rotate_rows(LP, form);
    const size_t lds = nnlm_svd_rotate_lds(LP, form);
    if (rb < 1 || ld % form) return hipErrorInvalidValue;
    if (lds > 65536) {
        const hipError_t e = hipFuncSetAttribute((const void *)svd_rotate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    svd_rotate_kernel<<<ld / form, SVD_ROT_THREADS, lds, st>>>(X, ld, ncols, LP, rb, form, T);
    return hipSuccess;
}

int nnlm_nndsvd_norm_blocks(int n, int m)
{
    const int len = n > m ? n : m;
    return len < 1 ? 1 : (len + SVD_CHUNK - 1) / SVD_CHUNK;
}

void nnlm_tu_nndsvd_norms(const double *U, int ldu, int n, const double *Vt, int ldv, int m, int k, double *part, double *out, hipStream_t st)
{
    const int nb = nnlm_nndsvd_norm_blocks(n, m);
    nndsvd_norms_kernel<<<dim3(nb, k), 256, 0, st>>>(U, ldu, n, Vt, ldv, m, part);
    svd_fold_kernel<<<(4 * k + 255) / 256, 256, 0, st>>>(part, nb, 4, 4 * k, out);
}

void nnlm_tu_nndsvd_build(const double *U, int ldu, const double *Vt, int ldv, const NndsvdRow *rows, int nrows, double fill, double *W64, float *Wop,
                          int ldw, int n, double *H64, int ldh, int m, hipStream_t st)
{
    const int ld = ldw > ldh ? ldw : ldh;
    nndsvd_build_kernel<<<dim3((ld + 255) / 256, nrows), 256, 0, st>>>(U, ldu, Vt, ldv, rows, fill, W64, Wop, ldw, n, H64, ldh, m);
}

static size_t svd_sum_blocks(size_t cnt) { return cnt < 1 ? 1 : (cnt + SVD_SUM_CHUNK - 1) / SVD_SUM_CHUNK; }

size_t nnlm_svd_sum_scratch(size_t cnt) { return svd_sum_blocks(cnt) + svd_sum_blocks(svd_sum_blocks(cnt)); }

// Two levels of per-block sums (4096 values each, the same tree in every block), then one thread folds the few that remain in block
// order: 2e8 values -> 50 000 -> 13 partial sums.  Every level has a fixed order.
void nnlm_tu_svd_sum(const void *x, bool f64, size_t cnt, double *part, double *out, hipStream_t st)
{
    const size_t nb = svd_sum_blocks(cnt), nb2 = svd_sum_blocks(nb);
    if (f64) svd_sum_kernel<double><<<(unsigned)nb, 256, 0, st>>>((const double *)x, cnt, part);
    else svd_sum_kernel<float><<<(unsigned)nb, 256, 0, st>>>((const float *)x, cnt, part);
    svd_sum_kernel<double><<<(unsigned)nb2, 256, 0, st>>>(part, nb, part + nb);
    svd_fold_kernel<<<1, 256, 0, st>>>(part + nb, (int)nb2, 1, 1, out);
}
