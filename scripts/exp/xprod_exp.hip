// Ablation micro-benchmark of xprod_tn_kernel (not part of the product).
// -DXPROD_BLOCKS: instead of the round-5 ablations, time the PRODUCT's xprod16_tn_kernel (nnlm_amd/csrc/k_xprod16.h) at config 2's two
// launches for {8, 10} wavefronts per block x {all 16, the 13 needed at k = 50} factor pieces, each at the slab counts that fill the
// device best, and print the weight of a factor byte against a byte of A that the four times imply (XPLAN_Y_WEIGHT in nnlm_mi355x.hip).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form -DXPROD_BLOCKS scripts/exp/xprod_exp.hip -o scripts/exp/xprod_blocks_exp
// `xprod_blocks_exp loop`: the shipped plans on two alternating split copies, one row per cache policy of the stream of A (loop_mode below).
#ifdef XPROD_BLOCKS
#include "../../nnlm_amd/csrc/k_xprod16.h"
#include <cstdio>
#include <cmath>
#include <algorithm>
#include <string>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
struct Times { float mean, sd, mn; };
template <int NWV, int YP> static Times run16b(const uint32_t *A, int lda, const uint32_t *Y, int ldy, double *Cx, int ldc, int S, int stages, int reps, const int *sc)
{
    const int lds = xprod16_lds_bytes(NWV, 4, YP), tiles = (ldc + 16 * NWV - 1) / (16 * NWV), sps = (stages + S - 1) / S;
    hipFuncSetAttribute((const void *)xprod16_tn_kernel<4, NWV, YP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    dim3 grid(tiles, (stages + sps - 1) / sps);
    std::vector<hipEvent_t> ev(reps + 1);
    for (auto &e : ev) hipEventCreate(&e);
    for (int i = 0; i < 3; i++) xprod16_tn_kernel<4, NWV, YP><<<grid, 64 * NWV, lds>>>(A, lda, Y, ldy, Cx, ldc, ldc, (size_t)64 * ldc, 0, stages, sps, sc);
    hipDeviceSynchronize();
    hipEventRecord(ev[0]);
    for (int i = 0; i < reps; i++) {
        xprod16_tn_kernel<4, NWV, YP><<<grid, 64 * NWV, lds>>>(A, lda, Y, ldy, Cx, ldc, ldc, (size_t)64 * ldc, 0, stages, sps, sc);
        hipEventRecord(ev[i + 1]);
    }
    hipEventSynchronize(ev[reps]);
    std::vector<float> t(reps);
    for (int i = 0; i < reps; i++) hipEventElapsedTime(&t[i], ev[i], ev[i + 1]);
    for (auto &e : ev) hipEventDestroy(e);
    double m = 0, v = 0;
    for (float x : t) m += x;
    m /= reps;
    for (float x : t) v += (x - m) * (x - m);
    return {(float)m, (float)std::sqrt(v / (reps - 1)), *std::min_element(t.begin(), t.end())};
}
// `xprod_blocks_exp loop`: the cache state of the iteration loop instead of a single-buffer replay.  Two separate split copies (818 MB each,
// as A16 and A16T); the benchmark's H launch (160-column blocks, 4 slabs) runs on one and its W launch (160-column blocks, 2 slabs) on the
// other, alternately, 30 timed pairs after 3 warm-up pairs, once per cache policy of the stream of A: nt_from_stage = INT_MAX (default
// policy), 0 (all of A non-temporal) and R in between (the stages < R of slab 0 keep the default policy: 256 R bytes of every column).
static int loop_mode()
{
    const int npad = 20224, mpad = 10112, pairs = 30, warm = 3;
    const size_t abytes = (size_t)npad * mpad * 4;
    uint32_t *A[2], *Y; double *Cx; int *sc;
    CK(hipMalloc(&A[0], abytes)); CK(hipMalloc(&A[1], abytes)); CK(hipMalloc(&Y, (size_t)64 * npad * 4)); CK(hipMalloc(&Cx, (size_t)4 * 64 * npad * 8));
    CK(hipMemset(A[0], 0x3c, abytes)); CK(hipMemset(A[1], 0x3c, abytes)); CK(hipMemset(Y, 0x3c, (size_t)64 * npad * 4));
    CK(hipMalloc(&sc, 8)); CK(hipMemset(sc, 0, 8));
    constexpr int NWV = 10, YP = 13;
    const int lds = xprod16_lds_bytes(NWV, 4, YP);
    CK(hipFuncSetAttribute((const void *)xprod16_tn_kernel<4, NWV, YP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    struct { const char *name; int len, cols, S; } L[2] = {{"H half-step (10112 cols x 316 stages, S = 4)", npad, mpad, 4}, {"W half-step (20224 cols x 158 stages, S = 2)", mpad, npad, 2}};
    auto launch = [&](int l, int nt_from) {
        const int stages = L[l].len / 64, sps = (stages + L[l].S - 1) / L[l].S, tiles = (L[l].cols + 16 * NWV - 1) / (16 * NWV);
        xprod16_tn_kernel<4, NWV, YP><<<dim3(tiles, (stages + sps - 1) / sps), 64 * NWV, lds>>>(A[l], L[l].len, Y, L[l].len, Cx, L[l].cols, L[l].cols, (size_t)64 * L[l].cols, 0,
                                                                                             stages, sps, sc, nt_from);
    };
    const double gb = (double)abytes / 1e9;
    std::vector<hipEvent_t> ev(2 * pairs + 1);
    for (auto &evt : ev) CK(hipEventCreate(&evt));
    printf("| launch | nt_from_stage | mean ms | sd | min ms | TB/s of A (mean) |\n|---|---|---|---|---|---|\n");
    for (int nt_from : {0x7fffffff, 0, 4, 8, 12, 16, 32, 64}) {
        for (int i = 0; i < warm; i++) launch(0, nt_from), launch(1, nt_from);
        CK(hipDeviceSynchronize());
        CK(hipEventRecord(ev[0]));
        for (int i = 0; i < pairs; i++) {
            launch(0, nt_from);
            CK(hipEventRecord(ev[2 * i + 1]));
            launch(1, nt_from);
            CK(hipEventRecord(ev[2 * i + 2]));
        }
        CK(hipEventSynchronize(ev[2 * pairs]));
        CK(hipGetLastError());
        for (int l = 0; l < 2; l++) {
            std::vector<float> t(pairs);
            for (int i = 0; i < pairs; i++) CK(hipEventElapsedTime(&t[i], ev[2 * i + l], ev[2 * i + l + 1]));
            double m = 0, v = 0;
            for (float x : t) m += x;
            m /= pairs;
            for (float x : t) v += (x - m) * (x - m);
            char nm[16];
            if (nt_from == 0x7fffffff) snprintf(nm, sizeof nm, "INT_MAX");
            else snprintf(nm, sizeof nm, "%d", nt_from);
            printf("| %s | %s | %.4f | %.4f | %.4f | %.2f |\n", L[l].name, nm, m, std::sqrt(v / (pairs - 1)), *std::min_element(t.begin(), t.end()), gb / m);
        }
    }
    return 0;
}
int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "loop") return loop_mode();
    const int npad = 20224, mpad = 10112, reps = 30;
    uint32_t *A, *Y; double *Cx; int *sc;
    CK(hipMalloc(&A, (size_t)npad * mpad * 4)); CK(hipMalloc(&Y, (size_t)64 * npad * 4)); CK(hipMalloc(&Cx, (size_t)16 * 64 * npad * 8));
    CK(hipMemset(A, 0x3c, (size_t)npad * mpad * 4)); CK(hipMemset(Y, 0x3c, (size_t)64 * npad * 4));
    CK(hipMalloc(&sc, 8)); CK(hipMemset(sc, 0, 8));
    const double gb = (double)npad * mpad * 4 / 1e9;
    // {name, lda = contraction length, ldc = columns}
    struct { const char *name; int len, cols; } L[2] = {{"H half-step (10112 cols x 316 stages)", npad, mpad}, {"W half-step (20224 cols x 158 stages)", mpad, npad}};
    printf("| launch | waves | pieces | S | blocks | mean ms | sd | min ms | TB/s of A (mean) |\n|---|---|---|---|---|---|---|---|---|\n");
    for (int l = 0; l < 2; l++) {
        const int len = L[l].len, cols = L[l].cols, stages = len / 64;
        double t8[2] = {0, 0}, t10[2] = {0, 0};
        auto row = [&](int w, int yp, int S, Times t) {
            const int tiles = (cols + 16 * w - 1) / (16 * w), sps = (stages + S - 1) / S;
            printf("| %s | %d | %d | %d | %d | %.4f | %.4f | %.4f | %.2f |\n", L[l].name, w, yp, S, tiles * ((stages + sps - 1) / sps), t.mean, t.sd, t.mn, gb / t.mean);
        };
        for (int S : {2, 3, 4}) {
            Times a = run16b<8, 16>(A, len, Y, len, Cx, cols, S, stages, reps, sc), b = run16b<8, 13>(A, len, Y, len, Cx, cols, S, stages, reps, sc);
            Times c = run16b<10, 13>(A, len, Y, len, Cx, cols, S, stages, reps, sc);
            row(8, 16, S, a), row(8, 13, S, b), row(10, 13, S, c);
            if (S == 3) t8[0] = a.mean, t8[1] = b.mean;
            if ((l == 0 && S == 4) || (l == 1 && S == 2)) t10[0] = c.mean;
        }
        // T ~ A bytes + w * factor bytes per stage at fixed geometry:  T(8,16) / T(8,13) = (32768 + 16384 w) / (32768 + 13312 w)
        const double r = t8[0] / t8[1], w = 32768.0 * (r - 1.0) / (16384.0 - 13312.0 * r);
        printf("%s: factor-byte weight implied by 8 waves, 16 vs 13 pieces at S = 3: %.3f; best 10-wave / 8-wave trimmed = %.4f\n", L[l].name, w, t10[0] / t8[1]);
    }
    return 0;
}
#else
#include "csrc_r5/k_xprod.h"
#include "csrc_r5/k_xprod16.h"
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
template <int EXP, int NKQ = 4, int KT = 0> static float run(const float *A, int lda, const float *Y, int ldy, double *Cx, int ldc, int tiles, int S, int sps, int stages, int reps)
{
    const int lds = xprod_tn_lds_bytes(64);
    hipFuncSetAttribute((const void *)xprod_tn_kernel<float, NKQ, KT, EXP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    dim3 grid(tiles, S);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    xprod_tn_kernel<float, NKQ, KT, EXP><<<grid, XPROD_THREADS, lds>>>(A, lda, Y, ldy, Cx, ldc, (size_t)64 * ldc, 0, stages, sps);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    for (int i = 0; i < reps; i++) xprod_tn_kernel<float, NKQ, KT, EXP><<<grid, XPROD_THREADS, lds>>>(A, lda, Y, ldy, Cx, ldc, (size_t)64 * ldc, 0, stages, sps);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    return ms / reps;
}
template <int EXP> static float run16(const uint32_t *A, int lda, const uint32_t *Y, int ldy, double *Cx, int ldc, int tiles, int S, int sps, int stages, int reps, const int *sc)
{
    const int lds = xprod_tn_lds_bytes(64);
    hipFuncSetAttribute((const void *)xprod16_tn_kernel<4, EXP>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    dim3 grid(tiles, S);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    xprod16_tn_kernel<4, EXP><<<grid, XPROD_THREADS, lds>>>(A, lda, Y, ldy, Cx, ldc, (size_t)64 * ldc, 0, stages, sps, sc);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    for (int i = 0; i < reps; i++) xprod16_tn_kernel<4, EXP><<<grid, XPROD_THREADS, lds>>>(A, lda, Y, ldy, Cx, ldc, (size_t)64 * ldc, 0, stages, sps, sc);
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    return ms / reps;
}
int main()
{
    const int npad = 20224, mpad = 10112;
    float *A, *Y; double *Cx;
    CK(hipMalloc(&A, (size_t)npad * mpad * 4)); CK(hipMalloc(&Y, (size_t)64 * npad * 4)); CK(hipMalloc(&Cx, (size_t)8 * 64 * mpad * 8));
    CK(hipMemset(A, 0x3c, (size_t)npad * mpad * 4)); CK(hipMemset(Y, 0x3c, (size_t)64 * npad * 4));
    const int stages = npad / 64, tiles = mpad / 128;
    int *sc; CK(hipMalloc(&sc, 8)); CK(hipMemset(sc, 0, 8));
    for (int S : {3, 6}) {
        const int sps = (stages + S - 1) / S;
        printf("S=%d (%d blocks): full %.3f | no-Y %.3f | no-MFMA %.3f | cached A %.3f | cached A+Y %.3f | loads only %.3f | cached, no LDS reads %.3f | MFMA only (no loads/barriers/LDS) %.3f | LDS+MFMA no loads/barriers %.3f ms\n", S, tiles * S,
               run<0>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10), run<1>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10),
               run<2>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10), run<4>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10),
               run<5>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10), run<3>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10),
               run<13>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10), run<24>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10),
               run<16>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10));
        printf("   tail NKQ=3 KT=2: full %.3f | cached A+Y %.3f | MFMA only %.3f | LDS+MFMA %.3f | cached no LDS reads %.3f | NKQ=3 KT=0 (k=48): full %.3f\n",
               run<0, 3, 2>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10), run<5, 3, 2>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10),
               run<24, 3, 2>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10), run<16, 3, 2>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10),
               run<13, 3, 2>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10), run<0, 3, 0>(A, npad, Y, npad, Cx, mpad, tiles, S, sps, stages, 10));
        printf("   split-fp16 (4 tiles): full %.3f | no MFMA %.3f | cached A %.3f\n", run16<0>((const uint32_t *)A, npad, (const uint32_t *)Y, npad, Cx, mpad, tiles, S, sps, stages, 10, sc),
               run16<2>((const uint32_t *)A, npad, (const uint32_t *)Y, npad, Cx, mpad, tiles, S, sps, stages, 10, sc),
               run16<4>((const uint32_t *)A, npad, (const uint32_t *)Y, npad, Cx, mpad, tiles, S, sps, stages, 10, sc));
    }
    return 0;
}
#endif
