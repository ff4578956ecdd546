// k_sparse_kl_batch.h -- the KL half-step of a BATCH of models on a sparse A whose absent entries are zeros (nnlm_set_matrix_csc_kl_batch,
// DESIGN section 4.20): the short form of k_sparse_kl.h for all active members of the stack in one launch.
//
// A wavefront owns a line (four lines per workgroup); the index, value and row pointer of the line's stored entries are loaded once
// (SPKL_EPL per lane) and serve every member.  Lane q holds x_q and sumw_q of STACKED coordinate q (the ranks sum to at most 64).  The
// members come in groups of G (a compile-time constant; the host lists the active members, larger ranks first, so that a group's ranks
// are close): within a group the coordinate loops run in lock step -- step q of the group is ONE straight-line block that gathers,
// divides, reduces (G interleaved 64-lane butterflies) and updates for its G members, so the G dependent chains of k_sparse_kl.h's solo
// kernel (gather -> quotient -> butterfly -> scalar division -> refresh) fill each other's issue slots.  A member that has fewer
// coordinates than the step, or that has left its inner-sweep loop, is predicated wavefront-uniformly: the block still runs for it on a
// valid address (its first coordinate) and its results are dropped.
//
// A member's arithmetic is the solo kernel's, call for call (spkl_entry, wave_sum, spkl_update, spkl_refresh; the starting state over its
// own coordinates, q ascending from off_b; its own S, rel and sweep count t): nothing depends on its neighbours, its position in the
// stack or G, so member b equals sp_kl_solve_kernel at rank k_b on the same line bit for bit.  A line is read and written by its one
// wavefront, so the factor may be solved in place (Xout == X); only the rows of the listed members are written.  No atomics on data; one
// integer atomic per line and member into its sweep counter.
#pragma once
#include "k_sparse_kl.h"

// every lane holds the same S, rel and t of a member: the flag in a scalar register, so that what hangs on it (the step's coordinate, the
// lane spkl_readlane reads) is wavefront-uniform for the compiler too
__device__ static inline bool spklb_uniform(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }

template <int METHOD, typename T, int G>
__global__ __launch_bounds__(256) void sp_kl_batch_kernel(const SpKlBatchArgs ba)
{
    const SpKlArgs &a = ba.a;
    const int lane = threadIdx.x & 63;
    const int col = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (col >= a.ncols) return; // (wave-uniform; no workgroup barrier below)
    const long long s = a.ptr[col];
    const long long len64 = a.ptr[col + 1] - s;
    if (len64 > SPKL_SHORT_MAX) return; // the long form's (per member, sp_kl_solve_long_kernel)
    const int len = (int)len64, K = a.k;
    const T *val = (const T *)a.val, *Y = (const T *)a.Y;

    double xv = lane < K ? a.X[(size_t)lane * a.ldx + col] : 0.0;
    const double sw = lane < K ? a.sumw[lane] : 0.0;

    const T *yr[SPKL_EPL];
    T bv[SPKL_EPL];
    bool ok[SPKL_EPL];
#pragma unroll
    for (int u = 0; u < SPKL_EPL; u++) {
        const int e = lane + 64 * u;
        ok[u] = e < len;
        const int i = ok[u] ? a.idx[s + e] : 0;
        bv[u] = ok[u] ? val[s + e] : (T)0;
        yr[u] = Y + (size_t)i * a.KP;
    }

    for (int m0 = 0; m0 < ba.nmem; m0 += G) {
        int mb[G], off[G], kk[G], kmax = 0;
#pragma unroll
        for (int g = 0; g < G; g++) { // (a short last group: the missing members have no coordinates and never run)
            const bool have = m0 + g < ba.nmem;
            mb[g] = ba.mem[have ? m0 + g : m0];
            off[g] = ba.off[mb[g]];
            kk[g] = have ? ba.kb[mb[g]] : 0;
            kmax = kk[g] > kmax ? kk[g] : kmax;
        }
        double S[G];
        T pv[G][SPKL_EPL];
#pragma unroll
        for (int g = 0; g < G; g++) {
            S[g] = 0.0;
            for (int q = 0; q < kk[g]; q++) S[g] += spkl_readlane(xv, off[g] + q);
#pragma unroll
            for (int u = 0; u < SPKL_EPL; u++) pv[g][u] = (T)0;
        }
        if (a.max_iter > 0) { // starting states (src/base_algorithms.cpp:82, :133) at the stored entries, member by member
            double pd[G][SPKL_EPL];
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int u = 0; u < SPKL_EPL; u++) pd[g][u] = 0.0;
            for (int q = 0; q < kmax; q++) {
#pragma unroll
                for (int g = 0; g < G; g++) {
                    if (q >= kk[g]) continue;
                    const double xq = spkl_readlane(xv, off[g] + q);
#pragma unroll
                    for (int u = 0; u < SPKL_EPL; u++)
                        if (ok[u]) pd[g][u] = __builtin_fma((double)yr[u][off[g] + q], xq, pd[g][u]);
                }
            }
#pragma unroll
            for (int g = 0; g < G; g++)
#pragma unroll
                for (int u = 0; u < SPKL_EPL; u++) pv[g][u] = (T)pd[g][u];
        }
        double rel[G];
        unsigned t[G];
        bool run[G], any = false;
#pragma unroll
        for (int g = 0; g < G; g++) {
            rel[g] = 1.0 + a.rel_tol;
            t[g] = 0;
            run[g] = spklb_uniform(kk[g] > 0 && t[g] < a.max_iter && rel[g] > a.rel_tol);
            any = any || run[g];
        }
        while (any) {
#pragma unroll
            for (int g = 0; g < G; g++)
                if (run[g]) rel[g] = 0.0;
            for (int q = 0; q < kmax; q++) {
                // one step of the group: every phase below is straight-line over its G members
                bool on[G];
                int c[G];
                double xq[G], sumw[G], s0[G], s1[G], coef[G];
                T w[G][SPKL_EPL];
#pragma unroll
                for (int g = 0; g < G; g++) {
                    on[g] = run[g] && q < kk[g];
                    c[g] = off[g] + (on[g] ? q : 0); // (always a coordinate of the stack: the gather below stays inside the row)
                    xq[g] = spkl_readlane(xv, c[g]);
                    sumw[g] = spkl_readlane(sw, c[g]);
#pragma unroll
                    for (int u = 0; u < SPKL_EPL; u++) w[g][u] = ok[u] ? yr[u][c[g]] : (T)0;
                }
#pragma unroll
                for (int g = 0; g < G; g++) {
                    s0[g] = 0.0, s1[g] = 0.0;
#pragma unroll
                    for (int u = 0; u < SPKL_EPL; u++)
                        if (ok[u]) spkl_entry<METHOD, T>(w[g][u], pv[g][u], bv[u], s0[g], s1[g]);
                }
#pragma unroll
                for (int g = 0; g < G; g++) {
                    s0[g] = wave_sum(s0[g]);
                    if (METHOD == 3) s1[g] = wave_sum(s1[g]);
                }
#pragma unroll
                for (int g = 0; g < G; g++) {
                    double Sn = S[g], reln = rel[g], cf;
                    const double xn = spkl_update<METHOD>(a, s0[g], s1[g], sumw[g], xq[g], Sn, reln, &cf);
                    coef[g] = on[g] ? cf : 0.0; // (a member that is not in this step: its sums are dropped)
                    S[g] = on[g] ? Sn : S[g];
                    rel[g] = on[g] ? reln : rel[g];
                    if (on[g] && lane == c[g]) xv = xn;
                }
#pragma unroll
                for (int g = 0; g < G; g++)
                    if (coef[g] != 0.0) { // (:106, :143)
#pragma unroll
                        for (int u = 0; u < SPKL_EPL; u++) pv[g][u] = spkl_refresh<T>(coef[g], w[g][u], pv[g][u]);
                    }
            }
            any = false;
#pragma unroll
            for (int g = 0; g < G; g++)
                if (run[g]) {
                    t[g]++;
                    run[g] = spklb_uniform(t[g] < a.max_iter && rel[g] > a.rel_tol);
                    any = any || run[g];
                }
        }
#pragma unroll
        for (int g = 0; g < G; g++) {
            if (lane >= off[g] && lane < off[g] + kk[g]) spkl_store(a, lane, col, xv);
            if (lane == 0 && t[g]) atomicAdd(ba.sweeps + mb[g], (unsigned long long)t[g]);
        }
    }
}
