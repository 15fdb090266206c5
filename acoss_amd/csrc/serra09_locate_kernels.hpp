// Serra09: WHERE the Qmax alignment lies.
//
//   A1 qmax_locate_kernel<EQG>  the Qmax row sweep over the recurrence bitmap that carries, beside every Q value, the cell
//                               at which the path through it began; reports max Q, the row-major first cell that attains it
//                               and that cell's path start.  One wave per pair, 32 columns per lane, strips of 2048 columns.
//
// The contract (the f32 values are those of oracle/acx_oracle.c step 6; Qmax only):
//   end    the first cell in row-major order with Q == max Q (the oracle's strict `v > best`)
//   pred   of a match cell: the first of c2 = Q[i-1][j-1], c3 = Q[i-2][j-1], c4 = Q[i-1][j-2] equal to their maximum (the oracle's
//          strict `>` chain); none when that maximum is 0 -- a path starts at the cell.  Of a gap cell with Q > 0: the first of the
//          penalised a2, a3, a4 equal to their maximum (gamma_o == gamma_e: the same choice as among c2, c3, c4, the penalty
//          being one monotone subtraction).
//   start  S[i][j] = (i, j) where a path starts, S[pred] elsewhere; reported: S[end].
// S is ONE u32 per cell, i * Mr + j: the host refuses a pair whose cells, plus one strip, reach 2^32.
//
// The sweep itself is qmax_locate_sweep: this kernel runs it once over rows 2 .. Me - 1, qmax_sections_kernel
// (serra09_sections_kernels.hpp) once per free interval of rows.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/acx.h"
#include "serra09_kernels.hpp"      // PairDesc, BAND, lane_prev_*

namespace acx {

constexpr int LOC_CPL = 32;                    // bitmap columns a lane owns
constexpr int LOC_STRIP = 64 * LOC_CPL;        // columns of one strip

// What a strip leaves for the next one, per row: Q, the penalised Q and S of its two rightmost columns
// (x1 = column c - 1, x2 = column c - 2; c = first column of the next strip).
struct alignas(16) LocSeam {
    float q1, q2, p1, p2;
    unsigned s1, s2, pad0, pad1;
};

// strips of a pair whose DP has Ne columns, and the seam records it needs (two buffers of one record per row)
__host__ __device__ inline int loc_strips(int Ne) { return Ne <= 0 ? 0 : (Ne + LOC_STRIP - 1) / LOC_STRIP; }
inline int64_t loc_seam_records(int Mq, int Mr, int dp_start)
{
    return loc_strips(dp_start == 3 ? Mr - 1 : Mr) > 1 ? 2 * (int64_t)Mq : 0;
}

__device__ __forceinline__ unsigned loc_shfl_xor_u(unsigned v, int m) { return (unsigned)__shfl_xor((int)v, m, 64); }

// a > b ? x : y and k == 0 ? x : y as ONE compare into vcc with its select right behind it.  Written as plain C++ the 3 x 32 selects
// of a row's S values are all placed behind the row's Q chain, their 96 lane masks kept in SGPRs until then: 402 SGPR spills to VGPR
// lanes in qmax_locate_kernel<true> (about 400 v_writelane / v_readlane per row of ~700 instructions).
__device__ __forceinline__ unsigned loc_sel_gt(float a, float b, unsigned x, unsigned y)
{
    unsigned r;
    asm("v_cmp_gt_f32_e32 vcc, %1, %2\n\tv_cndmask_b32_e32 %0, %4, %3, vcc" : "=v"(r) : "v"(a), "v"(b), "v"(x), "v"(y) : "vcc");
    return r;
}
__device__ __forceinline__ unsigned loc_sel_eq0(unsigned k, unsigned x, unsigned y)
{
    unsigned r;
    asm("v_cmp_eq_u32_e32 vcc, 0, %1\n\tv_cndmask_b32_e32 %0, %3, %2, vcc" : "=v"(r) : "v"(k), "v"(x), "v"(y) : "vcc");
    return r;
}

// The sweep of qmax_locate_kernel and qmax_sections_kernel: rows lo .. hi (2 <= lo, hi <= Me - 1) of the pair's recurrence bitmap in
// strips of 2048 columns, started from two ZERO rows and zero seam records -- rows 0 and 1 of Q, and every excluded row of a sections
// run, are zero.  Me x Ne: the DP's extent; bnd: the pair's seam records (two buffers of P.Mq; unused with one strip).  Returns, the
// same in every lane, max Q over these rows, the row-major first cell that attains it and that cell's path start (all 0 where no
// cell is positive).  A strip ends in __threadfence(): the next strip, and a later sweep over the same records, go through memory.
struct LocBest { float best; unsigned end, start; };

template <bool EQG>
__device__ __forceinline__ LocBest qmax_locate_sweep(const PairDesc &P, const unsigned long long *bits, LocSeam *bnd, int Me, int Ne,
                                                     float go, float ge, int lo, int hi)
{
    constexpr int CPL = LOC_CPL;
    constexpr int NP = EQG ? 1 : CPL;
    const int lane = threadIdx.x;
    const int ndw = 2 * P.nw;
    const unsigned *rows = reinterpret_cast<const unsigned *>(bits + P.offT);
    const unsigned W = (unsigned)P.Mr;             // S = i * W + j
    const int nstrips = loc_strips(Ne);
    float best = 0.0f;                             // this lane's first maximum so far, its cell and its path start
    unsigned bend = 0u, bstart = 0u;

    for (int s = 0; s < nstrips; ++s) {
        const int cbase = s * LOC_STRIP;
        const LocSeam *bin = bnd + (size_t)((s + 1) & 1) * P.Mq;      // records of strip s - 1 (read for s > 0 only)
        LocSeam *bout = bnd + (size_t)(s & 1) * P.Mq;
        const bool more = s + 1 < nstrips;
        unsigned colmask = 0u;                     // columns of this lane that exist and are >= 2 (the first two columns of Q stay 0)
#pragma unroll
        for (int e = 0; e < CPL; ++e) {
            const int j = cbase + CPL * lane + e;
            if (j >= 2 && j < Ne) colmask |= (1u << e);
        }
        float Q1[CPL], Q2[CPL], P1[NP], P2[NP];
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
        // the left strip's rows i - 1 and i - 2: zero above row lo, its records cover rows lo .. hi only
        LocSeam recA = {0.0f, 0.0f, 0.0f, 0.0f, 0u, 0u, 0u, 0u}, recB = recA;

        // One DP row: QA / SA / PA = row i-1, QB / SB / PB = row i-2 (overwritten with row i), descending column order
        auto dp_row = [&](int i, unsigned d0, unsigned d1, float (&QA)[CPL], float (&QB)[CPL], unsigned (&SA)[CPL], unsigned (&SB)[CPL],
                          float (&PA)[NP], float (&PB)[NP]) {
            LocSeam recN = recA;                   // the left strip's row i, for row i + 1 (one row ahead of its use)
            if (s > 0) recN = bin[i];
            const int sh = (BAND - 1) - (i & (BAND - 1));                  // bit position of column 0 in the row bitmap
            const unsigned w = __builtin_amdgcn_alignbit(d1, d0, sh) & colmask;
            float l1a = lane_prev_f(QA[CPL - 1]), l1b = lane_prev_f(QA[CPL - 2]), l2a = lane_prev_f(QB[CPL - 1]);
            unsigned t1a = lane_prev_u(SA[CPL - 1]), t1b = lane_prev_u(SA[CPL - 2]), t2a = lane_prev_u(SB[CPL - 1]);
            float p1a = 0.f, p1b = 0.f, p2a = 0.f;
            if constexpr (!EQG) {
                p1a = lane_prev_f(PA[NP - 1]); p1b = lane_prev_f(PA[NP - 2]); p2a = lane_prev_f(PB[NP - 1]);
            }
            if (lane == 0) {                       // (strip 0: the zeros of the matrix edge)
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
                    // match: mx + 1; gap: max(mx - g, 0): max(mx + t, 0) with t = +1 / -g blended by the sign-extended recurrence bit
                    // (qmax_cells: the same f32 operations on the same values)
                    const int rm = __builtin_amdgcn_sbfe((int)w, e, 1);
                    const float t = __int_as_float((rm & __float_as_int(1.0f)) | (~rm & __float_as_int(-go)));
                    q = fmaxf(mx + t, 0.0f);
                    // a match cell whose predecessors are all 0 (mx >= 0 is never -0: its bits are 0) has none: the path starts here
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
                // Columns 0, 1 and the columns right of the matrix take the gap branch (their recurrence bit is masked): in columns 0 / 1
                // the predecessors are all 0, so the cell is; a cell right of the matrix feeds only cells further right, and it is no
                // larger than its predecessor in an EARLIER row, so that, followed back into the matrix, some cell of the matrix holds
                // at least its value in an earlier row: it is never the row-major first maximum, whatever lane records it meanwhile.
                QB[e] = q;
                SB[e] = sn;
                if constexpr (!EQG) PB[e] = q - (r ? go : ge);
            }
            float rowmax = 0.0f;
#pragma unroll
            for (int e = 0; e < CPL; e += 2) rowmax = fmaxf(rowmax, fmaxf(QB[e], QB[e + 1]));
            // strict: an earlier row keeps a tie, and within the row the smallest column wins.  A later strip visits the rows again:
            // there a tie in an EARLIER row (self0 < bend; in the same row the later strip's columns are larger) takes over.
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

        unsigned a0, a1, b0, b1;                   // lo may have either parity: the register rows only alternate
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
        // the next strip reads this one's records: same wave, but through memory
        __threadfence();
    }

    // the wave's row-major first maximum: larger value, then smaller cell index (row, then column).  A strip visits its rows
    // again, so a lane of a later strip may hold an EARLIER row than a lane of an earlier one: the cell index decides, not the order.
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(best, m, 64);
        const unsigned oe = loc_shfl_xor_u(bend, m), os = loc_shfl_xor_u(bstart, m);
        if (ov > best || (ov == best && oe < bend)) { best = ov; bend = oe; bstart = os; }
    }
    return {best, bend, bstart};
}

template <bool EQG>
__global__ __launch_bounds__(64) void qmax_locate_kernel(const PairDesc *__restrict__ pd,
                                                         const unsigned long long *__restrict__ bits,
                                                         LocSeam *__restrict__ seam, const int64_t *__restrict__ seam_off,
                                                         acx_alignment *__restrict__ out,
                                                         float go, float ge, int dp_start)
{
    const PairDesc P = pd[blockIdx.x];
    int Me = P.Mq, Ne = P.Mr;
    if (dp_start == 3) { Me -= 1; Ne -= 1; }       // cell (i, j) of the oracle reads R[i-1][j-1]: the same DP on the plot less its last row / column
    LocSeam *bnd = loc_strips(Ne) > 1 ? seam + seam_off[blockIdx.x] : nullptr;
    const LocBest r = qmax_locate_sweep<EQG>(P, bits, bnd, Me, Ne, go, ge, 2, Me - 1);
    if (threadIdx.x == 0) {
        const unsigned W = (unsigned)P.Mr;
        acx_alignment a;
        a.score = r.best;
        if (r.best > 0.0f) {
            a.q0 = (int32_t)(r.start / W); a.r0 = (int32_t)(r.start % W);
            a.q1 = (int32_t)(r.end / W); a.r1 = (int32_t)(r.end % W);
        } else {
            a.q0 = -1; a.r0 = -1; a.q1 = -1; a.r1 = -1;
        }
        out[blockIdx.x] = a;
    }
}

}  // namespace acx
