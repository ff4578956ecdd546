// tu_svd.h -- launch entries of the kernels of k_svd.h (tu_svd.hip): the factor rotations, NNDSVD norms and build, and the sum of A behind
// nnlm_svd / nnlm_set_factors_nndsvd.
#pragma once
#include <hip/hip_runtime.h>

// One row of the start.  src: the triplet it is built from, -1 = a zero row (rank padding); side: 0 = |x| (component 0), 1 = the positive
// part, -1 = the negative part; su / sv: the scales of the W and the H entries (0: a zero component)
struct NndsvdRow {
    int src, side;
    double su, sv;
};

// The form of a rotation at padded rank LP: the widest column tile of svd_rotate_kernel (32, 16 or 8) whose columns of X plus eight rows
// of T fit the 160 KB LDS of a CU (32 up to LP = 512, 16 up to 853, 8 up to 1280), or 0: out of place through a second buffer
// (svd_rotate_global_kernel) -- no width is refused.
int nnlm_svd_rotate_form(int LP);
// Rows of T the tile width CB holds in LDS at a time (all LP when everything fits 64 KB; 0: CB does not fit), and the dynamic LDS bytes
int nnlm_svd_rotate_rows(int LP, int CB);
size_t nnlm_svd_rotate_lds(int LP, int CB);
// X [LP][ld] <- T X, padding columns (>= ncols) zero; T [LP][LP] on the device; form as above; tmp [LP][ld]: needed by form 0 only.
// Returns the hipFuncSetAttribute / argument error, if any.
hipError_t nnlm_tu_svd_rotate(double *X, int ld, int ncols, int LP, const double *T, int form, double *tmp, hipStream_t st);
// blocks per component of nnlm_tu_nndsvd_norms for lines of n and m entries
int nnlm_nndsvd_norm_blocks(int n, int m);
// out[4 j + {0: |u+|^2, 1: |u-|^2, 2: |v+|^2, 3: |v-|^2}] for j < k; part: [k][blocks][4] doubles
void nnlm_tu_nndsvd_norms(const double *U, int ldu, int n, const double *Vt, int ldv, int m, int k, double *part, double *out, hipStream_t st);
void nnlm_tu_nndsvd_build(const double *U, int ldu, const double *Vt, int ldv, const NndsvdRow *rows, int nrows, double fill, double *W64, float *Wop,
                          int ldw, int n, double *H64, int ldh, int m, hipStream_t st);
// doubles of partial sums nnlm_tu_svd_sum needs for cnt values (one per block of 4096 values, then one per 4096 of those); *out = the sum
size_t nnlm_svd_sum_scratch(size_t cnt);
void nnlm_tu_svd_sum(const void *x, bool f64, size_t cnt, double *part, double *out, hipStream_t st);
