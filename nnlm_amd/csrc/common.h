// common.h -- shared device helpers for libnnlm_mi355x (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define NNLM_TINY 1e-16 // TINY_NUM, reference src/nnlm.h:17

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// Geometry of the resident layouts (see DESIGN.md "Data layout in HBM").
//   A_dev  : [mpad][npad] elements of T, column j of A starts at j*npad (zero padded)
//   npad   : n rounded up to NNLM_PAD_N (tile of the A*H^T kernel along i)
//   mpad   : m rounded up to NNLM_PAD_M (tile of the W^T*A kernel along j)
#define NNLM_PAD_N 256
#define NNLM_PAD_M 128
#define NNLM_KQ_MAX 64 // fast path: rank padded to KP = 16*NKQ <= 64

static inline int round_up_i(int x, int q) { return (x + q - 1) / q * q; }

// ---- MFMA wrappers: 16x16x4, one element of A and B per lane ---------------------------------
//   A operand: lane l holds A[M = l&15][K = l>>4];  B operand: lane l holds B[K = l>>4][N = l&15]
//   f32 C/D: lane l, reg r -> D[M = 4*(l>>4)+r][N = l&15]
//   f64 C/D: lane l, reg r -> D[M = (l>>4)+4*r][N = l&15]   (cdna_hip_programming.md section 3)
template <typename T> struct Mfma;
template <> struct Mfma<float> {
    typedef f32x4 acc_t;
    static constexpr int EPV = 4; // elements per 16-byte LDS read
    __device__ static inline acc_t mma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    __device__ static inline int row_of(int lane, int r) { return 4 * (lane >> 4) + r; }
};
template <> struct Mfma<double> {
    typedef f64x4 acc_t;
    static constexpr int EPV = 2;
    __device__ static inline acc_t mma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    __device__ static inline int row_of(int lane, int r) { return (lane >> 4) + 4 * r; }
};

// 16-byte direct global->LDS copy (global_load_lds_dwordx4): per-lane global source, LDS
// destination = wave-uniform base + lane*16.
__device__ static inline void glds16(const void *gsrc, void *lds_wave_base)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)gsrc,
                                     (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

// ln x for a NORMAL positive fp32 x: v_log_f32 (log2, 1 ulp, one quarter-rate instruction) times ln 2.  logf() / __logf() compile
// to a ~20-instruction sequence here (denormal rescaling, two-term ln 2 product, special cases) -- measured as half of the error
// block's time.  The error sums take ln(ahat + 1e-16): never denormal; a relative error of 1e-7 per term averages out over 2e8.
#define NNLM_LN2F 0.69314718055994531f
__device__ static inline float log2_native(float x) { return __builtin_amdgcn_logf(x); }

// The reference's relative-change test  2|x_new - x| / (x_new + x + eps) > rel_tol  (src/base_algorithms.cpp:29-35), decided exactly
// like its rounded quotient without a division on the common path: away from the boundary  2|d| > tol * s  is the same decision (both
// roundings are below 2 ulp); inside a band of 1e-15 relative the IEEE quotient is formed and compared, as the reference does.
__device__ static inline bool rel_change_exceeds(double d2, double s, double tol)
{
    const double rhs = tol * s;
    if (__builtin_expect(fabs(d2 - rhs) <= 1e-15 * fabs(rhs), 0)) return d2 / s > tol;
    return d2 > rhs;
}

__device__ static inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ static inline long long wave_sum_ll(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ln x for a positive, finite, NORMAL double (the error sums take ln(ahat + 1e-16): never zero, never denormal) in ~28 fp64
// instructions: x = m 2^e with m in [sqrt(1/2), sqrt 2), ln m = 2 atanh(s), s = (m - 1) / (m + 1) (|s| <= 0.1716: ten terms of the
// odd series leave 6e-19), the quotient correctly rounded (reciprocal, two Newton steps, one residual correction).  libm's log()
// compiles to ~55 instructions here and was two thirds of errors_kernel<double>'s arithmetic.  Error < 2 ulp of the result.
// (The series coefficients live in constant memory, NOT as literals: gfx950's VOP3 encoding has no 64-bit literal operand, so each
// literal costs a VGPR pair -- 30 registers of a kernel that needs them for occupancy; loaded from a non-const __constant__ array
// they arrive by s_load and stay in SGPR pairs, one scalar source per fma.)
static __constant__ double NNLM_LOGC[19] = {1.0 / 21.0, 1.0 / 19.0, 1.0 / 17.0, 1.0 / 15.0, 1.0 / 13.0, 1.0 / 11.0, 1.0 / 9.0, 1.0 / 7.0,
                                            1.0 / 5.0,  1.0 / 3.0,  1.9082149292705877e-10, 0.693147180369123816490,
                                            1.0 / 7.0, -1.0 / 6.0, 1.0 / 5.0, -1.0 / 4.0, 1.0 / 3.0, -0.5, 0.69314718055994530942}; // [12..18]: nnlm_log_tab
__device__ static inline double nnlm_log_pos(double x)
{
    double m = __builtin_amdgcn_frexp_mant(x); // [0.5, 1)
    int e = __builtin_amdgcn_frexp_exp(x);
    const bool lo = m < 0.70710678118654752;
    m = lo ? 2.0 * m : m;
    e = lo ? e - 1 : e;
    const double num = m - 1.0, den = m + 1.0;
    double r = __builtin_amdgcn_rcp(den);
    r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
    r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
    double sq = num * r;
    sq = __builtin_fma(__builtin_fma(-den, sq, num), r, sq);
    const double z = sq * sq;
    double p = NNLM_LOGC[0];
#pragma unroll
    for (int c = 1; c < 10; c++) p = __builtin_fma(p, z, NNLM_LOGC[c]);
    // ln m = 2 s + 2 s z p;  e ln 2 in two pieces (the high one has 11 trailing zero bits: e * LN2_HI is exact for |e| < 2048)
    const double ed = (double)e;
    const double t = __builtin_fma(2.0 * sq * z, p, ed * NNLM_LOGC[10]);
    return __builtin_fma(ed, NNLM_LOGC[11], 2.0 * sq + t);
}
