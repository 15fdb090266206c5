// Serra09: EVERY matched section of a pair, not only the best one.
//
//   S1 qmax_sections_kernel<EQG>  qmax_locate_kernel's sweep, run per FREE INTERVAL of the plot's rows: section 0 is section 16's
//                                 alignment; the rows of a section found (and `pad` rows on either side, clipped to the free interval
//                                 it lies in) become excluded, Q is 0 on them, and the next section is the alignment of what is left.
//                                 One wave per pair, 32 columns per lane, strips of 2048 columns; the loop over sections runs inside
//                                 the launch.
//
// The contract is section 16's (serra09_locate_kernels.hpp) on the masked matrix Q': the same f32 values, end = row-major first
// maximum, the same predecessor chains.  Q' = 0 on a stretch of at least two rows cuts the recursion (it reaches back two rows at
// most), so Q' on a free interval [a, b] is the recursion run over rows a..b from two zero rows -- independent of every other
// interval.  Hence
//   * a sweep per free interval, its register rows and seam state zeroed at row a: no test of the row inside the unrolled row pair;
//   * one best record (value, end, start) per free interval; a section splits ONE interval, and only its two remainders are swept
//     again -- every other record still holds;
//   * the next section is the best of the records by (value, then smaller end cell): the row-major rule across intervals.
// An interval of fewer than 2 DP rows holds no value above 1 and is not swept (the host refuses min_score <= 1).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/acx.h"
#include "serra09_kernels.hpp"          // PairDesc, BAND, lane_prev_*
#include "serra09_locate_kernels.hpp"   // LocSeam, loc_strips, loc_sel_gt, loc_sel_eq0

namespace acx {

constexpr int SEC_MAX = 16;                    // sections of one pair, at most (acx_section_opts.max_sections)

template <bool EQG>
__global__ __launch_bounds__(64) void qmax_sections_kernel(const PairDesc *__restrict__ pd,
                                                           const unsigned long long *__restrict__ bits,
                                                           LocSeam *__restrict__ seam, const int64_t *__restrict__ seam_off,
                                                           acx_alignment *__restrict__ out, int32_t *__restrict__ n_out,
                                                           float go, float ge, int dp_start,
                                                           int max_sections, int pad, float min_score, float min_ratio)
{
    constexpr int CPL = LOC_CPL;
    constexpr int NP = EQG ? 1 : CPL;
    // the free intervals [a, b] of the plot's rows (either may be empty: a > b) and the best record of each; wave-uniform
    __shared__ int iv_a[SEC_MAX + 1], iv_b[SEC_MAX + 1];
    __shared__ float iv_v[SEC_MAX + 1];
    __shared__ unsigned iv_e[SEC_MAX + 1], iv_s[SEC_MAX + 1];
    const int lane = threadIdx.x;
    const PairDesc P = pd[blockIdx.x];
    int Me = P.Mq, Ne = P.Mr;
    if (dp_start == 3) { Me -= 1; Ne -= 1; }       // as in qmax_locate_kernel: the same DP on the plot less its last row / column
    const int ndw = 2 * P.nw;
    const unsigned *rows = reinterpret_cast<const unsigned *>(bits + P.offT);
    const unsigned W = (unsigned)P.Mr;             // S = i * W + j
    const int nstrips = loc_strips(Ne);
    LocSeam *bnd = nstrips > 1 ? seam + seam_off[blockIdx.x] : nullptr;
    const int S = min(max(max_sections, 1), SEC_MAX);
    pad = min(max(pad, 0), P.Mq);                  // (q1 + pad stays an int)
    acx_alignment *rec = out + (size_t)blockIdx.x * S;

    if (lane == 0) { iv_a[0] = 0; iv_b[0] = P.Mq - 1; }
    __syncthreads();
    int n_iv = 1, found = 0;
    int npend = 1, pend0 = 0, pend1 = 0;           // the intervals whose records the next round computes
    float score0 = 0.0f;

    for (;;) {
        for (int t = 0; t < npend; ++t) {
            const int idx = t == 0 ? pend0 : pend1;
            const int lo = max(__builtin_amdgcn_readfirstlane(iv_a[idx]), 2);             // rows 0 and 1 of Q stay zero
            const int hi = min(__builtin_amdgcn_readfirstlane(iv_b[idx]), Me - 1);
            float best = 0.0f;                     // this lane's first maximum so far, its cell and its path start
            unsigned bend = 0u, bstart = 0u;
            if (hi - lo >= 1) {
                for (int s = 0; s < nstrips; ++s) {
                    const int cbase = s * LOC_STRIP;
                    const LocSeam *bin = bnd + (size_t)((s + 1) & 1) * P.Mq;      // records of strip s - 1 (read for s > 0 only)
                    LocSeam *bout = bnd + (size_t)(s & 1) * P.Mq;
                    const bool more = s + 1 < nstrips;
                    unsigned colmask = 0u;         // columns of this lane that exist and are >= 2 (the first two columns of Q stay 0)
#pragma unroll
                    for (int e = 0; e < CPL; ++e) {
                        const int j = cbase + CPL * lane + e;
                        if (j >= 2 && j < Ne) colmask |= (1u << e);
                    }
                    float Q1[CPL], Q2[CPL], P1[NP], P2[NP];                       // rows lo - 1 and lo - 2 of Q' are zero
                    unsigned S1[CPL], S2[CPL];
#pragma unroll
                    for (int e = 0; e < CPL; ++e) {
                        Q1[e] = 0.0f; Q2[e] = 0.0f; S1[e] = 0u; S2[e] = 0u;
                        if constexpr (!EQG) { P1[e] = 0.0f; P2[e] = 0.0f; }
                    }
                    const int dw0 = (cbase + CPL * lane) >> 5;
                    const bool has0 = dw0 < ndw, has1 = dw0 + 1 < ndw;
                    auto load_row = [&](int i, unsigned &d0, unsigned &d1) {
                        d0 = 0u; d1 = 0u;
                        if (i < Me) {
                            const unsigned *r = rows + (size_t)i * ndw;
                            if (has0) d0 = r[dw0];
                            if (has1) d1 = r[dw0 + 1];
                        }
                    };
                    // the left strip's rows i - 1 and i - 2: zero above the interval, its records cover rows lo..hi only
                    LocSeam recA = {0.0f, 0.0f, 0.0f, 0.0f, 0u, 0u, 0u, 0u}, recB = recA;

                    // One DP row, as in qmax_locate_kernel: QA / SA / PA = row i-1, QB / SB / PB = row i-2 (overwritten with row i)
                    auto dp_row = [&](int i, unsigned d0, unsigned d1, float (&QA)[CPL], float (&QB)[CPL], unsigned (&SA)[CPL],
                                      unsigned (&SB)[CPL], float (&PA)[NP], float (&PB)[NP]) {
                        LocSeam recN = recA;       // the left strip's row i, for row i + 1 (one row ahead of its use)
                        if (s > 0) recN = bin[i];
                        const int sh = (BAND - 1) - (i & (BAND - 1));              // bit position of column 0 in the row bitmap
                        const unsigned w = __builtin_amdgcn_alignbit(d1, d0, sh) & colmask;
                        float l1a = lane_prev_f(QA[CPL - 1]), l1b = lane_prev_f(QA[CPL - 2]), l2a = lane_prev_f(QB[CPL - 1]);
                        unsigned t1a = lane_prev_u(SA[CPL - 1]), t1b = lane_prev_u(SA[CPL - 2]), t2a = lane_prev_u(SB[CPL - 1]);
                        float p1a = 0.f, p1b = 0.f, p2a = 0.f;
                        if constexpr (!EQG) {
                            p1a = lane_prev_f(PA[NP - 1]); p1b = lane_prev_f(PA[NP - 2]); p2a = lane_prev_f(PB[NP - 1]);
                        }
                        if (lane == 0) {           // (strip 0: the zeros of the matrix edge)
                            l1a = recA.q1; l1b = recA.q2; l2a = recB.q1;
                            t1a = recA.s1; t1b = recA.s2; t2a = recB.s1;
                            p1a = recA.p1; p1b = recA.p2; p2a = recB.p1;
                        }
                        const unsigned self0 = (unsigned)i * W + (unsigned)(cbase + CPL * lane);
#pragma unroll
                        for (int e = CPL - 1; e >= 0; --e) {
                            const bool r = (w >> e) & 1u;
                            const float c2 = (e >= 1) ? QA[e - 1] : l1a;                          // (i-1, j-1)
                            const float c3 = (e >= 1) ? QB[e - 1] : l2a;                          // (i-2, j-1)
                            const float c4 = (e >= 2) ? QA[e - 2] : (e == 1 ? l1a : l1b);         // (i-1, j-2)
                            const unsigned s2 = (e >= 1) ? SA[e - 1] : t1a;
                            const unsigned s3 = (e >= 1) ? SB[e - 1] : t2a;
                            const unsigned s4 = (e >= 2) ? SA[e - 2] : (e == 1 ? t1a : t1b);
                            const float m23 = fmaxf(c2, c3), mx = fmaxf(m23, c4);
                            float q;
                            unsigned sn;
                            if constexpr (EQG) {
                                const unsigned sc = loc_sel_gt(c4, m23, s4, loc_sel_gt(c3, c2, s3, s2));      // the first of c2, c3, c4 equal to mx
                                const int rm = __builtin_amdgcn_sbfe((int)w, e, 1);
                                const float tt = __int_as_float((rm & __float_as_int(1.0f)) | (~rm & __float_as_int(-go)));
                                q = fmaxf(mx + tt, 0.0f);
                                sn = loc_sel_eq0((unsigned)__float_as_int(mx) | (unsigned)~rm, self0 + (unsigned)e, sc);
                            } else {
                                unsigned sc = (c3 > c2) ? s3 : s2;                                // the first of c2, c3, c4 equal to mx
                                sc = (c4 > m23) ? s4 : sc;
                                const unsigned smatch = (mx == 0.0f) ? self0 + (unsigned)e : sc;  // no predecessor: the path starts here
                                const float a2 = (e >= 1) ? PA[e - 1] : p1a;
                                const float a3 = (e >= 1) ? PB[e - 1] : p2a;
                                const float a4 = (e >= 2) ? PA[e - 2] : (e == 1 ? p1a : p1b);
                                const float n23 = fmaxf(a2, a3), amx = fmaxf(n23, a4);
                                unsigned sa = (a3 > a2) ? s3 : s2;
                                sa = (a4 > n23) ? s4 : sa;
                                q = r ? (mx + 1.0f) : fmaxf(amx, 0.0f);
                                sn = r ? smatch : sa;
                            }
                            // (columns 0, 1 and the columns right of the matrix: as in qmax_locate_kernel, never the first maximum)
                            QB[e] = q;
                            SB[e] = sn;
                            if constexpr (!EQG) PB[e] = q - (r ? go : ge);
                        }
                        float rowmax = 0.0f;
#pragma unroll
                        for (int e = 0; e < CPL; e += 2) rowmax = fmaxf(rowmax, fmaxf(QB[e], QB[e + 1]));
                        if (rowmax > best || (rowmax == best && self0 < bend)) {
                            best = rowmax;
#pragma unroll
                            for (int e = CPL - 1; e >= 0; --e)
                                if (QB[e] == rowmax) { bend = self0 + (unsigned)e; bstart = SB[e]; }
                        }
                        if (more && lane == 63) {
                            LocSeam o;
                            o.q1 = QB[CPL - 1]; o.q2 = QB[CPL - 2];
                            o.p1 = EQG ? 0.0f : PB[NP - 1]; o.p2 = EQG ? 0.0f : PB[EQG ? 0 : NP - 2];
                            o.s1 = SB[CPL - 1]; o.s2 = SB[CPL - 2]; o.pad0 = 0u; o.pad1 = 0u;
                            bout[i] = o;
                        }
                        recB = recA; recA = recN;
                    };

                    unsigned a0, a1, b0, b1;       // the interval may begin on either row parity: the register rows only alternate
                    load_row(lo, a0, a1); load_row(lo + 1, b0, b1);
                    for (int i = lo; i <= hi; i += 2) {
                        unsigned n0, n1;
                        load_row(i + 2, n0, n1);
                        dp_row(i, a0, a1, Q1, Q2, S1, S2, P1, P2);
                        a0 = n0; a1 = n1;
                        if (i + 1 <= hi) {
                            load_row(i + 3, n0, n1);
                            dp_row(i + 1, b0, b1, Q2, Q1, S2, S1, P2, P1);
                            b0 = n0; b1 = n1;
                        }
                    }
                    // the next strip (and the next sweep, which writes the same records) goes through memory: same wave
                    __threadfence();
                }
                // the wave's row-major first maximum of the interval: larger value, then smaller cell index
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) {
                    const float ov = __shfl_xor(best, m, 64);
                    const unsigned oe = loc_shfl_xor_u(bend, m), os = loc_shfl_xor_u(bstart, m);
                    if (ov > best || (ov == best && oe < bend)) { best = ov; bend = oe; bstart = os; }
                }
            }
            if (lane == 0) { iv_v[idx] = best; iv_e[idx] = bend; iv_s[idx] = bstart; }
        }
        __syncthreads();

        // the next section: the best of the interval records
        float bv = 0.0f;
        unsigned be = 0u, bs = 0u;
        int bi = -1;
        for (int t = 0; t < n_iv; ++t) {
            const float v = iv_v[t];
            const unsigned e = iv_e[t];
            if (v > bv || (v == bv && bi >= 0 && e < be)) { bv = v; be = e; bs = iv_s[t]; bi = t; }
        }
        bi = __builtin_amdgcn_readfirstlane(bi);
        if (bi < 0) break;
        const float thr = found == 0 ? min_score : fmaxf(min_score, min_ratio * score0);
        if (!(bv >= thr)) break;
        if (found == 0) score0 = bv;
        const int q0 = (int)(__builtin_amdgcn_readfirstlane(bs) / W), q1 = (int)(__builtin_amdgcn_readfirstlane(be) / W);
        if (lane == 0) {
            acx_alignment a;
            a.score = bv;
            a.q0 = q0; a.r0 = (int32_t)(bs % W);
            a.q1 = q1; a.r1 = (int32_t)(be % W);
            rec[found] = a;
        }
        if (++found == S) break;
        // rows [max(a, q0 - pad), min(b, q1 + pad)] of the section's interval [a, b] become excluded; what is left above and below
        const int a = __builtin_amdgcn_readfirstlane(iv_a[bi]), b = __builtin_amdgcn_readfirstlane(iv_b[bi]);
        __syncthreads();
        if (lane == 0) {
            iv_b[bi] = max(a, q0 - pad) - 1;
            iv_a[n_iv] = min(b, q1 + pad) + 1; iv_b[n_iv] = b;
        }
        __syncthreads();
        pend0 = bi; pend1 = n_iv; npend = 2;
        ++n_iv;
    }

    if (lane == 0) {
        n_out[blockIdx.x] = found;
        acx_alignment none;
        none.score = 0.0f; none.q0 = -1; none.r0 = -1; none.q1 = -1; none.r1 = -1;
        for (int k = found; k < S; ++k) rec[k] = none;
    }
}

}  // namespace acx
