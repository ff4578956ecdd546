// k_sparse_kl.h -- the KL-divergence half-step on a sparse A whose absent entries are zeros (nnlm_set_matrix_csc_kl): scd_kl_update
// (reference src/base_algorithms.cpp:71-116) and lee_kl_update (:119-151) over the STORED entries of a line only.
//
// Every sum over the contraction in the two reference loops is weighted by the data: a = sum_i Aj_i mu_i^2, b = sum_i Aj_i mu_i - sumW_q
// (SCD), Wt.row(q) . (Aj / (wh + eps)) (Lee).  A row with Aj_i = 0 adds an exact 0 (Ajt + 1e-16 > 0, so mu is finite and 0 * mu = 0);
// only sumW sees every row, and that is the k column sums of the fixed factor (kl_sumw_kernel, k_kl.h).  The state vector Ajt / wh is
// therefore needed at the stored entries only, and a half-step is O(nnz k): per stored entry e of line c and coordinate q one gather of
// Yrow[idx[e]][q], one quotient and two to three multiply-adds.  The result differs from the dense computation by summation order only.
//
// Line = column of A for the H half-step (CSC), row of A for the W half-step (the CSR the handle keeps).  Two forms by the line's
// stored count L (nnlm_get_info "sparse_kl_form_h" / "_w": bit 0 = the short form ran, bit 1 = the long form ran):
//   L <= SPKL_SHORT_MAX  sp_kl_solve_kernel       a wavefront per line, four lines per workgroup; lane l holds entries l, l + 64, ...
//                                                 (index, value, state: SPKL_EPL of each in registers), sums by a 64-lane butterfly
//   L >  SPKL_SHORT_MAX  sp_kl_solve_long_kernel  a workgroup per line (the list of long lines is made when the matrix is set), 256
//                                                 entries per pass, the state of entry e in a per-entry buffer state[e] (type T); the
//                                                 rank-1 refresh step q - 1 owes an entry is applied while the sums of step q are formed
//                                                 (kl_stream_kernel's arrangement); sums: butterfly per wavefront, then LDS in wave order
// Starting states p_e = sum_q Yrow[i_e][q] x_q (fp64 multiply-adds, q ascending, rounded to T) are formed in the prologue of both.
// T: fp32 in the fp32-operand mode (state, row copy, values; the quotient is w * v_rcp_f32(|p + 1e-16|) as in kl_tile_kernel, DESIGN 4.7;
// the sums are fp64), fp64 in the strict mode (the reference's arithmetic, correctly rounded quotients).  A state that returns to exactly
// 0 is divided as 0 + 1e-16: no 0 * rcp(0).  An empty line has empty sums: SCD gets b = -sumW_q - ... <= 0, the coordinate is clamped to
// 0; Lee gets tmp = 0 / (sumW_q + ...) = 0 (0 / 0 only where the reference has it too: a zero column of the fixed factor without penalty).
// No atomics on data (the integer sweep counter is one atomic add per line): two runs are bit-identical.
#pragma once
#include "common.h"
#include "tu_sweepq.h"

#define SPKL_EPL 4                       // stored entries per lane of the short form
#define SPKL_SHORT_MAX (64 * SPKL_EPL)   // the longest line the short form takes (tests/sparse_kl_cases.py restates it)

__device__ static inline double spkl_readlane(double v, int src)
{
    int2 p = __builtin_bit_cast(int2, v);
    p.x = __builtin_amdgcn_readlane(p.x, src);
    p.y = __builtin_amdgcn_readlane(p.y, src);
    return __builtin_bit_cast(double, p);
}

// The refreshed state wh + coef * w, rounded to T.  The state is a sum of non-negative terms x_q w_q; in fp32 its rounding residue can be
// negative and of the size of the 1e-16 in the quotient (a coordinate that went to 1e-16 and back), where |p + 1e-16| cancels and the
// reciprocal overflows: the fp32 state is kept at >= 0 (the strict mode keeps the reference's arithmetic as it is)
template <typename T> __device__ static inline T spkl_refresh(double coef, T w, T p)
{
    const T v = (T)__builtin_fma(coef, (double)w, (double)p);
    if constexpr (sizeof(T) == 4) return v > 0.0f ? v : 0.0f;
    else return v;
}

__device__ static inline bool spkl_all_masked(unsigned long long mword, int k)
{
    const unsigned long long km = k >= 64 ? ~0ull : ((1ull << k) - 1ull);
    return (mword & km) == km;
}

// one stored entry's share of the sums of coordinate step q: w = Yrow[i][q], p = state, b = data
template <int METHOD, typename T> __device__ static inline void spkl_entry(T w, T p, T b, double &s0, double &s1)
{
    if constexpr (sizeof(T) == 8) {
        if (METHOD == 4) {
            s0 += w * (b / (p + NNLM_TINY));
        } else {
            const double u = w / (p + NNLM_TINY);
            s0 += b * (u * u);
            s1 += b * u;
        }
    } else {
        const float r = __builtin_amdgcn_rcpf(__builtin_fabsf(p + 1e-16f));
        if (METHOD == 4) {
            s0 += (double)(w * (b * r));
        } else {
            const float u = w * r, bu = b * u;
            s0 += (double)bu * (double)u;
            s1 += (double)bu;
        }
    }
}

// The scalar update of coordinate q from the reduced sums (every lane computes the same): returns the new x_q, *coef = what the
// states owe (new wh = wh + coef * row q), and updates S = sum of x and the sweep's largest relative change.
template <int METHOD>
__device__ static inline double spkl_update(const SpKlArgs &a, double s0, double s1, double sumw, double xq, double &S, double &rel, double *coef)
{
    *coef = 0.0;
    if (METHOD == 4) { // src/base_algorithms.cpp:141-147
        double tmp = s0 / (sumw + a.r0 * xq + a.r1 * (S - xq) + a.r2);
        *coef = (tmp - 1) * xq;
        S = __builtin_fma(tmp - 1, xq, S); // (one rounding, written out: the contraction every instantiation had chosen must not depend on the caller)
        const double xn = xq * tmp;
        tmp = 2 * fabs(tmp - 1) / (tmp + 1);
        if (tmp > rel) rel = tmp;
        return xn;
    }
    double aa = s0, bb = s1 - sumw; // :98-111
    aa += a.r0;
    bb += aa * xq - a.r2 - a.r1 * (S - xq);
    double tmp = bb / (aa + NNLM_TINY);
    if (tmp < 0) tmp = 0;
    if (tmp != xq) {
        *coef = tmp - xq;
        const double er = 2 * fabs(xq - tmp) / (tmp + xq + NNLM_TINY);
        if (er > rel) rel = er;
        S += tmp - xq;
        return tmp;
    }
    return xq;
}

__device__ static inline void spkl_store(const SpKlArgs &a, int q, int col, double xv)
{
    a.Xout[(size_t)q * a.ldx + col] = xv;
    if (a.op_mode == 1) ((float *)a.op)[(size_t)q * a.op_ld + col] = (float)xv; // (fp32-operand mode only: the strict mode's operand IS the master)
}

// ---- short form: a wavefront per line, k <= 64 (lane q holds x_q) ----
template <int METHOD, typename T>
__global__ __launch_bounds__(256) void sp_kl_solve_kernel(const SpKlArgs a)
{
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= a.ncols) return; // (wave-uniform; no workgroup barrier below)
    const long long s = a.ptr[col];
    const long long len64 = a.ptr[col + 1] - s;
    if (len64 > SPKL_SHORT_MAX) return; // the long form's
    const int len = (int)len64, k = a.k;
    const T *val = (const T *)a.val, *Y = (const T *)a.Y;
    const unsigned long long mword = a.mask ? a.mask[(size_t)col * a.mw] : 0ull;
    const bool skipcol = spkl_all_masked(mword, k); // (update() passes such a line by: no sweep is counted, src/update_with_missing.cpp:32)

    double xv = lane < k ? a.X[(size_t)lane * a.ldx + col] : 0.0;
    const double sw = lane < k ? a.sumw[lane] : 0.0;
    double S = 0.0;
    for (int q = 0; q < k; q++) S += spkl_readlane(xv, q);

    const T *yr[SPKL_EPL];
    T bv[SPKL_EPL], pv[SPKL_EPL];
    bool ok[SPKL_EPL];
#pragma unroll
    for (int u = 0; u < SPKL_EPL; u++) {
        const int e = lane + 64 * u;
        ok[u] = e < len;
        const int i = ok[u] ? a.idx[s + e] : 0;
        bv[u] = ok[u] ? val[s + e] : (T)0;
        yr[u] = Y + (size_t)i * a.KP;
        pv[u] = (T)0;
    }
    if (a.max_iter > 0 && !skipcol) { // starting states (src/base_algorithms.cpp:82, :133) at the stored entries
        double pd[SPKL_EPL];
#pragma unroll
        for (int u = 0; u < SPKL_EPL; u++) pd[u] = 0.0;
        for (int q = 0; q < k; q++) {
            const double xq = spkl_readlane(xv, q);
#pragma unroll
            for (int u = 0; u < SPKL_EPL; u++)
                if (ok[u]) pd[u] = __builtin_fma((double)yr[u][q], xq, pd[u]);
        }
#pragma unroll
        for (int u = 0; u < SPKL_EPL; u++) pv[u] = (T)pd[u];
    }
    double rel = 1.0 + a.rel_tol;
    unsigned t = 0;
    for (; !skipcol && t < a.max_iter && rel > a.rel_tol; t++) {
        rel = 0.0;
        for (int q = 0; q < k; q++) {
            if ((mword >> q) & 1ull) continue;
            const double xq = spkl_readlane(xv, q), sumw = spkl_readlane(sw, q);
            T w[SPKL_EPL];
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int u = 0; u < SPKL_EPL; u++) {
                w[u] = ok[u] ? yr[u][q] : (T)0;
                if (ok[u]) spkl_entry<METHOD, T>(w[u], pv[u], bv[u], s0, s1);
            }
            s0 = wave_sum(s0);
            if (METHOD == 3) s1 = wave_sum(s1);
            double coef;
            const double xn = spkl_update<METHOD>(a, s0, s1, sumw, xq, S, rel, &coef);
            if (lane == q) xv = xn;
            if (coef != 0.0) { // (:106, :143)
#pragma unroll
                for (int u = 0; u < SPKL_EPL; u++) pv[u] = spkl_refresh<T>(coef, w[u], pv[u]);
            }
        }
    }
    if (lane < k) spkl_store(a, lane, col, xv);
    if (lane == 0 && t) atomicAdd(a.sweeps, (unsigned long long)t);
}

// ---- long form: a workgroup per line of the list longc, any stored count ----
template <int METHOD, typename T>
__global__ __launch_bounds__(256) void sp_kl_solve_long_kernel(const SpKlArgs a)
{
    __shared__ double xs[NNLM_KQ_MAX];
    __shared__ double red[2][2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = a.longc[blockIdx.x], k = a.k;
    const long long s = a.ptr[col], len = a.ptr[col + 1] - s;
    const T *val = (const T *)a.val + s, *Y = (const T *)a.Y;
    const int *idx = a.idx + s;
    T *ps = (T *)a.state + s; // (entries of distinct lines are distinct: no two workgroups share a slot)
    const unsigned long long mword = a.mask ? a.mask[(size_t)col * a.mw] : 0ull;
    const bool skipcol = spkl_all_masked(mword, k); // (update() passes such a line by: no sweep is counted, src/update_with_missing.cpp:32)

    if (tid < k) xs[tid] = a.X[(size_t)tid * a.ldx + col];
    __syncthreads();
    double S = 0.0;
    for (int q = 0; q < k; q++) S += xs[q];
    if (a.max_iter > 0 && !skipcol)
        for (long long e = tid; e < len; e += 256) {
            const T *yr = Y + (size_t)idx[e] * a.KP;
            double pd = 0.0;
            for (int q = 0; q < k; q++) pd = __builtin_fma((double)yr[q], xs[q], pd);
            ps[e] = (T)pd;
        }
    double rel = 1.0 + a.rel_tol, cprev = 0.0;
    unsigned t = 0;
    int par = 0, qprev = -1;
    for (; !skipcol && t < a.max_iter && rel > a.rel_tol; t++) {
        rel = 0.0;
        for (int q = 0; q < k; q++) {
            if ((mword >> q) & 1ull) continue;
            const double xq = xs[q];
            double s0 = 0.0, s1 = 0.0;
            for (long long e = tid; e < len; e += 256) { // (a thread meets the same entries in every step: the state needs no barrier)
                const T *yr = Y + (size_t)idx[e] * a.KP;
                T pv = ps[e];
                if (cprev != 0.0) { // the refresh step qprev owes this entry (:106, :143)
                    pv = spkl_refresh<T>(cprev, yr[qprev], pv);
                    ps[e] = pv;
                }
                spkl_entry<METHOD, T>(yr[q], pv, val[e], s0, s1);
            }
            s0 = wave_sum(s0);
            if (METHOD == 3) s1 = wave_sum(s1);
            if (lane == 0) red[par][0][wave] = s0, red[par][1][wave] = s1;
            __syncthreads();
            s0 = (red[par][0][0] + red[par][0][1]) + (red[par][0][2] + red[par][0][3]);
            s1 = (red[par][1][0] + red[par][1][1]) + (red[par][1][2] + red[par][1][3]);
            par ^= 1;
            const double xn = spkl_update<METHOD>(a, s0, s1, a.sumw[q], xq, S, rel, &cprev);
            if (tid == 0) xs[q] = xn;
            qprev = q;
        }
        __syncthreads();
    }
    __syncthreads();
    if (tid < k) spkl_store(a, tid, col, xs[tid]);
    if (tid == 0 && t) atomicAdd(a.sweeps, (unsigned long long)t);
}
