// LateFusionChen: WHERE the Dmax alignment lies, and its PATH.
//
//   D1 dmax_locate_kernel<EQG>  qmax_locate_kernel's row sweep with the Dmax bonus bits: reports max Q, the row-major first cell that
//                               attains it and that cell's path start.  One wave per pair, 32 columns per lane, strips of 2048 columns.
//   D2 dmax_path_kernel<EQG>    qmax_path_kernel's box pass with the Dmax bonus bits: one 2-bit predecessor code per box cell, then the
//                               traceback.  Same direction plane, seam records, boxes and budget (serra09_path_kernels.hpp).
//
// The contract (the f32 values are those of oracle/acx_oracle.c step 6 with dmax = 1):
//   c2 = Q[i-1][j-1], c3 = Q[i-2][j-1] + R[i-1][j], c4 = Q[i-1][j-2] + R[i][j-1]          (the bonus bits are RAW bits of the plot)
//   match  max(c2, c3, c4) + 1; gap  max(0, c2 - g(R[i-1][j-1]), c3 - g(R[i-2][j-1]), c4 - g(R[i-1][j-2]))
//   end    the first cell in row-major order with Q == max Q
//   pred   the cell of the first of the three candidates (bonus included; penalised in a gap cell) equal to their maximum -- unless
//          that cell's own Q is 0: then the path starts here.  (Qmax: "their maximum is 0".  Dmax: c3 can be 1 over a Q of 0.)
//   start  S[i][j] = (i, j) where a path starts, S[pred] elsewhere; reported: S[end].
// What does not carry over from the Qmax kernels:
//   * R[i][j-1] of a lane's first column is the left lane's last bit; of a strip's first column it is read from the bitmap.
//   * R[i-1][j] is the previous row's word, extracted with THAT row's phase (i & 7).
//   * "no predecessor" needs the chosen candidate's own Q.  The locating sweep carries it in S: a cell whose Q is 0 holds LOC_NONE, which
//     is no cell's index (the host refuses a plot whose cells, plus one strip, reach 2^32: every index is at most 2^32 - 3).  The path
//     pass has no S and selects the chosen candidate's Q beside its code.
//   * Columns 0, 1 and the columns right of the matrix are FORCED to 0 in the locating sweep, as the Dmax score sweeps force them
//     (qmax_cells): R[i][1] is a bonus of column 2's c4, so a masked column is not 0 by itself.  The path pass needs none: the box lies
//     inside the DP's cells, left of it Q reads 0 by construction and a column right of it feeds only columns further right.
//   * gamma_o != gamma_e: a penalised value of a cell with Q = 0 is -g(R[cell]), and 1 - g can be positive.  Rows 0 / 1 (the box pass:
//     the two rows above and the two columns left of the box) carry those penalties, read from the plot as it is.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/acx.h"
#include "serra09_kernels.hpp"          // PairDesc, BAND, lane_prev_*
#include "serra09_locate_kernels.hpp"   // LOC_CPL, LOC_STRIP, LocSeam, loc_strips, loc_sel_*
#include "serra09_path_kernels.hpp"     // PATH_CPL, PATH_STRIP, PathSeam, PathBox, path_words, path_strips

namespace acx {

constexpr unsigned LOC_NONE = 0xffffffffu;     // S of a cell whose Q is 0

// a == b ? x : y as one compare into vcc with its select right behind it (loc_sel_gt's reason)
__device__ __forceinline__ unsigned loc_sel_eq(unsigned a, unsigned b, unsigned x, unsigned y)
{
    unsigned r;
    asm("v_cmp_eq_u32_e32 vcc, %1, %2\n\tv_cndmask_b32_e32 %0, %4, %3, vcc" : "=v"(r) : "v"(a), "v"(b), "v"(x), "v"(y) : "vcc");
    return r;
}
// 1.0f where bit e of w is set, 0.0f elsewhere (the sign-extended bit opaque: seen through, a row's 64 bonus bits become 64 bit tests
// into SGPR lane masks, kept there until their selects)
__device__ __forceinline__ float loc_bonus(unsigned w, int e)
{
    int m = __builtin_amdgcn_sbfe((int)w, e, 1);
    asm("" : "+v"(m));
    return __int_as_float(m & __float_as_int(1.0f));
}

// (x & m) | (y & ~m) for a sign-extended bit m, opaque: seen through, the blend becomes a bit test into an SGPR lane mask and a select
__device__ __forceinline__ unsigned loc_blend(int m, unsigned x, unsigned y)
{
    asm("" : "+v"(m));
    return (x & (unsigned)m) | (y & ~(unsigned)m);
}

template <bool EQG>
__global__ __launch_bounds__(64) void dmax_locate_kernel(const PairDesc *__restrict__ pd,
                                                         const unsigned long long *__restrict__ bits,
                                                         LocSeam *__restrict__ seam, const int64_t *__restrict__ seam_off,
                                                         acx_alignment *__restrict__ out,
                                                         float go, float ge, int dp_start)
{
    constexpr int CPL = LOC_CPL;
    constexpr int NP = EQG ? 1 : CPL;
    const int lane = threadIdx.x;
    const PairDesc P = pd[blockIdx.x];
    int Me = P.Mq, Ne = P.Mr;
    if (dp_start == 3) { Me -= 1; Ne -= 1; }       // the same DP on the plot less its last row / column (bonus bits included)
    const int ndw = 2 * P.nw;
    const unsigned *rows = reinterpret_cast<const unsigned *>(bits + P.offT);
    const unsigned W = (unsigned)P.Mr;             // S = i * W + j
    const int nstrips = loc_strips(Ne);
    LocSeam *bnd = nstrips > 1 ? seam + seam_off[blockIdx.x] : nullptr;
    float best = 0.0f;
    unsigned bend = 0u, bstart = 0u;

    for (int s = 0; s < nstrips; ++s) {
        const int cbase = s * LOC_STRIP;
        const LocSeam *bin = bnd + (size_t)((s + 1) & 1) * P.Mq;
        LocSeam *bout = bnd + (size_t)(s & 1) * P.Mq;
        const bool more = s + 1 < nstrips;
        unsigned colmask = 0u;                     // columns of this lane that exist and are >= 2: every other cell is forced to 0
#pragma unroll
        for (int e = 0; e < CPL; ++e) {
            const int j = cbase + CPL * lane + e;
            if (j >= 2 && j < Ne) colmask |= (1u << e);
        }
        float Q1[CPL], Q2[CPL], P1[NP], P2[NP];
        unsigned S1[CPL], S2[CPL];
#pragma unroll
        for (int e = 0; e < CPL; ++e) { Q1[e] = 0.0f; Q2[e] = 0.0f; S1[e] = LOC_NONE; S2[e] = LOC_NONE; }
        // d0 / d1: the lane's dwords of row i; dm: the dword left of them (lane 0 of a strip behind the first finds R[i][cbase - 1] there).
        // No branch: a row behind the plot is its last row again (loaded, never used: no DP row reads a row >= Me but through the
        // prefetch), and a dword outside the row is the row's first / last again -- it would hold columns left or right of the
        // matrix, whose cells are forced to 0 whatever their own and their bonus bits say.
        const int dw0 = (cbase + CPL * lane) >> 5;
        const int ia = min(dw0, ndw - 1), ib = min(dw0 + 1, ndw - 1), im = min(max(dw0 - 1, 0), ndw - 1);
        auto load_row = [&](int i, unsigned &d0, unsigned &d1, unsigned &dm) {
            const unsigned *r = rows + (size_t)min(i, P.Mq - 1) * ndw;
            d0 = r[ia];
            d1 = r[ib];
            dm = r[im];
        };
        auto row_bits = [&](int i, unsigned d0, unsigned d1) {
            return __builtin_amdgcn_alignbit(d1, d0, (BAND - 1) - (i & (BAND - 1)));      // (that row's phase)
        };
        // rows 0 and 1: Q = 0; their raw bits are row 2's bonus bits and, with distinct penalties, their penalised values
        unsigned wprev;
        {
            unsigned p0, p1, pm;
            load_row(1, p0, p1, pm);
            wprev = row_bits(1, p0, p1);
            if constexpr (!EQG) {
                load_row(0, p0, p1, pm);
                const unsigned w0 = row_bits(0, p0, p1);
#pragma unroll
                for (int e = 0; e < CPL; ++e) {
                    P1[e] = ((wprev >> e) & 1u) ? -go : -ge;
                    P2[e] = ((w0 >> e) & 1u) ? -go : -ge;
                }
            }
        }
        if (more && lane == 63) {
            LocSeam z;
            z.q1 = 0.0f; z.q2 = 0.0f; z.p1 = 0.0f; z.p2 = 0.0f; z.s1 = LOC_NONE; z.s2 = LOC_NONE; z.pad0 = 0u; z.pad1 = 0u;
            if constexpr (!EQG) { z.p1 = P2[NP - 1]; z.p2 = P2[EQG ? 0 : NP - 2]; }
            if (Me > 0) bout[0] = z;
            if constexpr (!EQG) { z.p1 = P1[NP - 1]; z.p2 = P1[EQG ? 0 : NP - 2]; }
            if (Me > 1) bout[1] = z;
        }
        LocSeam recA;                              // the left strip's rows i - 1 and i - 2
        recA.q1 = 0.0f; recA.q2 = 0.0f; recA.p1 = 0.0f; recA.p2 = 0.0f; recA.s1 = LOC_NONE; recA.s2 = LOC_NONE; recA.pad0 = 0u; recA.pad1 = 0u;
        LocSeam recB = recA;
        if (s > 0 && Me > 2) { recB = bin[0]; recA = bin[1]; }

        // One DP row: QA / SA / PA = row i-1, QB / SB / PB = row i-2 (overwritten with row i), descending column order
        auto dp_row = [&](int i, unsigned d0, unsigned d1, unsigned dm, float (&QA)[CPL], float (&QB)[CPL], unsigned (&SA)[CPL],
                          unsigned (&SB)[CPL], float (&PA)[NP], float (&PB)[NP]) {
            LocSeam recN = recA;
            if (s > 0) recN = bin[i];
            const int sh = (BAND - 1) - (i & (BAND - 1));
            const unsigned wraw = __builtin_amdgcn_alignbit(d1, d0, sh);
            const unsigned w = wraw & colmask;
            unsigned cmrow = colmask;              // (opaque: hoisted out of the row loop, its 32 bit tests are 32 lane masks in SGPRs)
            asm("" : "+v"(cmrow));
            float l1a = lane_prev_f(QA[CPL - 1]), l1b = lane_prev_f(QA[CPL - 2]), l2a = lane_prev_f(QB[CPL - 1]);
            unsigned t1a = lane_prev_u(SA[CPL - 1]), t1b = lane_prev_u(SA[CPL - 2]), t2a = lane_prev_u(SB[CPL - 1]);
            unsigned carry = lane_prev_u(wraw >> (CPL - 1));       // R[i][j0 - 1]: the left lane's last bit
            float p1a = 0.f, p1b = 0.f, p2a = 0.f;
            if constexpr (!EQG) {
                p1a = lane_prev_f(PA[NP - 1]); p1b = lane_prev_f(PA[NP - 2]); p2a = lane_prev_f(PB[NP - 1]);
            }
            if (lane == 0) {
                l1a = recA.q1; l1b = recA.q2; l2a = recB.q1;
                t1a = recA.s1; t1b = recA.s2; t2a = recB.s1;
                p1a = recA.p1; p1b = recA.p2; p2a = recB.p1;
                // the bit left of the strip, from the bitmap: position sh - 1 of d0, or the last bit of dm (strip 0: column -1, whose
                // bit only reaches column 0, a forced cell)
                carry = (unsigned)(((((unsigned long long)d0) << 32) | dm) >> (31 + sh)) & 1u;
            }
            const unsigned wleft = (wraw << 1) | carry;            // bit e = R[i][j-1]
            const unsigned self0 = (unsigned)i * W + (unsigned)(cbase + CPL * lane);
#pragma unroll
            for (int e = CPL - 1; e >= 0; --e) {
                const float x3 = loc_bonus(wprev, e), x4 = loc_bonus(wleft, e);
                const float c2 = (e >= 1) ? QA[e - 1] : l1a;                                  // (i-1, j-1)
                const float c3 = ((e >= 1) ? QB[e - 1] : l2a) + x3;                           // (i-2, j-1) + R[i-1][j]
                const float c4 = ((e >= 2) ? QA[e - 2] : (e == 1 ? l1a : l1b)) + x4;          // (i-1, j-2) + R[i][j-1]
                const unsigned s2 = (e >= 1) ? SA[e - 1] : t1a;
                const unsigned s3 = (e >= 1) ? SB[e - 1] : t2a;
                const unsigned s4 = (e >= 2) ? SA[e - 2] : (e == 1 ? t1a : t1b);
                const float m23 = fmaxf(c2, c3), mx = fmaxf(m23, c4);
                int cm = __builtin_amdgcn_sbfe((int)cmrow, e, 1);
                asm("" : "+v"(cm));
                const int rm = __builtin_amdgcn_sbfe((int)w, e, 1);
                float q;
                unsigned sc;
                if constexpr (EQG) {
                    sc = loc_sel_gt(c4, m23, s4, loc_sel_gt(c3, c2, s3, s2));                 // the first of c2, c3, c4 equal to mx
                    const float t = __int_as_float((rm & __float_as_int(1.0f)) | (~rm & __float_as_int(-go)));
                    q = fmaxf(mx + t, 0.0f);      // (one monotone subtraction: the gap cell's choice is the choice among c2, c3, c4)
                } else {
                    const unsigned sm = loc_sel_gt(c4, m23, s4, loc_sel_gt(c3, c2, s3, s2));
                    const float a2 = (e >= 1) ? PA[e - 1] : p1a;
                    const float a3 = ((e >= 1) ? PB[e - 1] : p2a) + x3;
                    const float a4 = ((e >= 2) ? PA[e - 2] : (e == 1 ? p1a : p1b)) + x4;
                    const float n23 = fmaxf(a2, a3), amx = fmaxf(n23, a4);
                    const unsigned sa = loc_sel_gt(a4, n23, s4, loc_sel_gt(a3, a2, s3, s2));
                    q = __int_as_float((int)loc_blend(rm, (unsigned)__float_as_int(mx + 1.0f), (unsigned)__float_as_int(fmaxf(amx, 0.0f))));
                    sc = loc_blend(rm, sm, sa);
                }
                q = __int_as_float(__float_as_int(q) & cm);                                   // columns 0, 1 and right of the matrix: 0
                // the chosen candidate's own Q is 0 (its S says so): the path starts here; a cell that holds 0 lies on no path
                unsigned sn = loc_sel_eq(sc, LOC_NONE, self0 + (unsigned)e, sc);
                sn = loc_sel_eq0((unsigned)__float_as_int(q), LOC_NONE, sn);                  // (q >= 0 is never -0)
                QB[e] = q;
                SB[e] = sn;
                if constexpr (!EQG)                                                           // (a forced cell's penalty follows its raw bit)
                    PB[e] = q - __int_as_float((int)loc_blend(__builtin_amdgcn_sbfe((int)wraw, e, 1), (unsigned)__float_as_int(go), (unsigned)__float_as_int(ge)));
            }
            wprev = wraw;
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

        unsigned a0, a1, am, b0, b1, bm;
        load_row(2, a0, a1, am); load_row(3, b0, b1, bm);
        for (int i = 2; i < Me; i += 2) {
            unsigned n0, n1, nm;
            load_row(i + 2, n0, n1, nm);
            dp_row(i, a0, a1, am, Q1, Q2, S1, S2, P1, P2);
            a0 = n0; a1 = n1; am = nm;
            if (i + 1 < Me) {
                load_row(i + 3, n0, n1, nm);
                dp_row(i + 1, b0, b1, bm, Q2, Q1, S2, S1, P2, P1);
                b0 = n0; b1 = n1; bm = nm;
            }
        }
        __threadfence();       // the next strip reads this one's records: same wave, but through memory
    }

    // the wave's row-major first maximum (qmax_locate_kernel)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(best, m, 64);
        const unsigned oe = loc_shfl_xor_u(bend, m), os = loc_shfl_xor_u(bstart, m);
        if (ov > best || (ov == best && oe < bend)) { best = ov; bend = oe; bstart = os; }
    }
    if (lane == 0) {
        acx_alignment a;
        a.score = best;
        if (best > 0.0f) {
            a.q0 = (int32_t)(bstart / W); a.r0 = (int32_t)(bstart % W);
            a.q1 = (int32_t)(bend / W); a.r1 = (int32_t)(bend % W);
        } else {
            a.q0 = -1; a.r0 = -1; a.q1 = -1; a.r1 = -1;
        }
        out[blockIdx.x] = a;
    }
}

// The box pass.  A box starts at a cell with Q > 0, so q0 >= 2 and r0 >= 2: rows q0 - 1, q0 - 2 and columns r0 - 1, r0 - 2 exist in the plot,
// and their bits are read as they are (the bonus of the box's first row and column, and the penalties of the zeros around the box).
template <bool EQG>
__global__ __launch_bounds__(64) void dmax_path_kernel(const PairDesc *__restrict__ pd, const PathBox *__restrict__ boxes,
                                                       const unsigned long long *__restrict__ bits,
                                                       unsigned long long *__restrict__ dir, PathSeam *__restrict__ seam,
                                                       int32_t *__restrict__ cells, int32_t *__restrict__ n_cells,
                                                       float go, float ge)
{
    constexpr int CPL = PATH_CPL;
    constexpr int NP = EQG ? 1 : CPL;
    const int lane = threadIdx.x;
    const PathBox bx = boxes[blockIdx.x];
    const PairDesc P = pd[bx.pair];
    const int H = bx.q1 - bx.q0 + 1, Wd = bx.r1 - bx.r0 + 1;
    const int nwords = path_words(Wd);
    const int ndw = 2 * P.nw;
    const unsigned *rows = reinterpret_cast<const unsigned *>(bits + P.offT);
    unsigned long long *plane = dir + bx.dir_off;
    const int nstrips = path_strips(Wd);
    PathSeam *bnd = nstrips > 1 ? seam + bx.seam_off : nullptr;

    for (int s = 0; s < nstrips; ++s) {
        const int cbase = s * PATH_STRIP + CPL * lane;
        const PathSeam *bin = bnd + (size_t)((s + 1) & 1) * H;
        PathSeam *bout = bnd + (size_t)(s & 1) * H;
        const bool more = s + 1 < nstrips;
        unsigned colmask = 0u;
#pragma unroll
        for (int e = 0; e < CPL; ++e)
            if (cbase + e < Wd) colmask |= (1u << e);
        const int word = s * 64 + lane;
        const bool has_word = word < nwords;
        float Q1[CPL], Q2[CPL], P1[NP], P2[NP];
#pragma unroll
        for (int e = 0; e < CPL; ++e) { Q1[e] = 0.0f; Q2[e] = 0.0f; }
        // The 34 bits of plot row i = q0 + y at plot columns r0 + cbase - 2 .. r0 + cbase + 31, in two dwords and the dword before them:
        // bit 0 / 1 of `lb` = the two columns left of the lane's, `wl` = columns - 1 .. + 30 (bit e = R[i][j-1]), `wr` = the lane's own.
        // y may be -1 and -2 (the rows above the box; q0 >= 2); a row behind the box is its last row again (loaded, never used).  A dword
        // behind the row's last is the last again: it would hold columns right of the plot, which are right of the box.
        auto load_row = [&](int y, unsigned &dl, unsigned &d0, unsigned &d1) {
            const int i = max(bx.q0 + min(y, H - 1), 0);                              // (the max: a record that broke q0 >= 2 reads inside)
            const int pos = bx.r0 + cbase - 2 + (BAND - 1) - (i & (BAND - 1));       // (>= 0: r0 >= 2)
            const int dw0 = max(pos, 0) >> 5;
            const unsigned *r = rows + (size_t)i * ndw;
            dl = r[min(dw0, ndw - 1)];
            d0 = r[min(dw0 + 1, ndw - 1)];
            d1 = r[min(dw0 + 2, ndw - 1)];
        };
        auto row_bits = [&](int y, unsigned dl, unsigned d0, unsigned d1, unsigned &lb, unsigned &wl, unsigned &wr) {
            const int i = bx.q0 + y;
            const int sh = (bx.r0 + cbase - 2 + (BAND - 1) - (i & (BAND - 1))) & 31;
            const unsigned lo = __builtin_amdgcn_alignbit(d0, dl, sh), hi = __builtin_amdgcn_alignbit(d1, d0, sh);      // 64 bits from column - 2
            lb = lo & 3u;
            wl = __builtin_amdgcn_alignbit(hi, lo, 1);
            wr = __builtin_amdgcn_alignbit(hi, lo, 2);
        };
        auto pen = [&](unsigned bit) { return bit ? -go : -ge; };
        // the rows above the box: Q = 0; their raw bits are the first box row's bonus bits and, with distinct penalties, their penalised values
        unsigned wprev;
        PathSeam recA = {0.0f, 0.0f, 0.0f, 0.0f}, recB = recA;      // the cells left of the lane's, box rows y - 1 and y - 2 (lane 0 uses them)
        {
            unsigned dl, d0, d1, lb1, lb2, wl, w2;
            load_row(-1, dl, d0, d1);
            row_bits(-1, dl, d0, d1, lb1, wl, wprev);
            if constexpr (!EQG) {
                load_row(-2, dl, d0, d1);
                row_bits(-2, dl, d0, d1, lb2, wl, w2);
#pragma unroll
                for (int e = 0; e < CPL; ++e) { P1[e] = pen((wprev >> e) & 1u); P2[e] = pen((w2 >> e) & 1u); }
                recA.p1 = pen(lb1 & 2u); recA.p2 = pen(lb1 & 1u);
                recB.p1 = pen(lb2 & 2u); recB.p2 = pen(lb2 & 1u);
            }
        }

        auto dp_row = [&](int y, unsigned dl, unsigned d0, unsigned d1, float (&QA)[CPL], float (&QB)[CPL], float (&PA)[NP], float (&PB)[NP]) {
            unsigned lb, wleft, wraw;
            row_bits(y, dl, d0, d1, lb, wleft, wraw);
            // the cells left of the lane's in row y, for row y + 1: the left strip's record, or (strip 0) the zeros left of the box
            PathSeam recN = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (!EQG) { recN.p1 = pen(lb & 2u); recN.p2 = pen(lb & 1u); }
            if (s > 0) recN = bin[y];
            const unsigned w = wraw & colmask;
            float l1a = lane_prev_f(QA[CPL - 1]), l1b = lane_prev_f(QA[CPL - 2]), l2a = lane_prev_f(QB[CPL - 1]);
            float p1a = 0.f, p1b = 0.f, p2a = 0.f;
            if constexpr (!EQG) {
                p1a = lane_prev_f(PA[NP - 1]); p1b = lane_prev_f(PA[NP - 2]); p2a = lane_prev_f(PB[NP - 1]);
            }
            if (lane == 0) {
                l1a = recA.q1; l1b = recA.q2; l2a = recB.q1;
                p1a = recA.p1; p1b = recA.p2; p2a = recB.p1;
            }
            unsigned lo = 0u, hi = 0u;
#pragma unroll
            for (int e = CPL - 1; e >= 0; --e) {
                const float x3 = loc_bonus(wprev, e), x4 = loc_bonus(wleft, e);
                const float q2 = (e >= 1) ? QA[e - 1] : l1a;                                  // (i-1, j-1)
                const float q3 = (e >= 1) ? QB[e - 1] : l2a;                                  // (i-2, j-1)
                const float q4 = (e >= 2) ? QA[e - 2] : (e == 1 ? l1a : l1b);                 // (i-1, j-2)
                const float c2 = q2, c3 = q3 + x3, c4 = q4 + x4;
                const float m23 = fmaxf(c2, c3), mx = fmaxf(m23, c4);
                float q;
                unsigned code;
                if constexpr (EQG) {
                    // the first of c2, c3, c4 equal to mx, and that cell's own Q: 0 there, and a path starts here
                    code = loc_sel_gt(c4, m23, 3u, loc_sel_gt(c3, c2, 2u, 1u));
                    const unsigned cq = loc_sel_gt(c4, m23, (unsigned)__float_as_int(q4),
                                                   loc_sel_gt(c3, c2, (unsigned)__float_as_int(q3), (unsigned)__float_as_int(q2)));
                    code = loc_sel_eq0(cq, 0u, code);                                         // (Q >= 0 is never -0)
                    int rm = __builtin_amdgcn_sbfe((int)w, e, 1);
                    asm("" : "+v"(rm));
                    const float t = __int_as_float((rm & __float_as_int(1.0f)) | (~rm & __float_as_int(-go)));
                    q = fmaxf(mx + t, 0.0f);
                } else {
                    const unsigned u2 = (unsigned)__float_as_int(q2), u3 = (unsigned)__float_as_int(q3), u4 = (unsigned)__float_as_int(q4);
                    const unsigned cm = loc_sel_gt(c4, m23, 3u, loc_sel_gt(c3, c2, 2u, 1u));
                    const unsigned qm = loc_sel_gt(c4, m23, u4, loc_sel_gt(c3, c2, u3, u2));
                    const float a2 = (e >= 1) ? PA[e - 1] : p1a;
                    const float a3 = ((e >= 1) ? PB[e - 1] : p2a) + x3;
                    const float a4 = ((e >= 2) ? PA[e - 2] : (e == 1 ? p1a : p1b)) + x4;
                    const float n23 = fmaxf(a2, a3), amx = fmaxf(n23, a4);
                    const unsigned ca = loc_sel_gt(a4, n23, 3u, loc_sel_gt(a3, a2, 2u, 1u));
                    const unsigned qa = loc_sel_gt(a4, n23, u4, loc_sel_gt(a3, a2, u3, u2));
                    const int rm = __builtin_amdgcn_sbfe((int)w, e, 1);
                    q = __int_as_float((int)loc_blend(rm, (unsigned)__float_as_int(mx + 1.0f), (unsigned)__float_as_int(fmaxf(amx, 0.0f))));
                    code = loc_sel_eq0(loc_blend(rm, qm, qa), 0u, loc_blend(rm, cm, ca));     // (Q >= 0 is never -0)
                }
                QB[e] = q;
                if constexpr (!EQG)
                    PB[e] = q - __int_as_float((int)loc_blend(__builtin_amdgcn_sbfe((int)wraw, e, 1), (unsigned)__float_as_int(go), (unsigned)__float_as_int(ge)));
                if (e >= 16) hi |= code << (2 * (e - 16)); else lo |= code << (2 * e);
            }
            wprev = wraw;
            if (has_word) path_store_codes(plane, y, nwords, word, lo, hi);
            if (more && lane == 63) path_store_seam<EQG>(bout, y, QB, PB);
            recB = recA; recA = recN;
        };

        unsigned al, a0, a1, bl, b0, b1;
        load_row(0, al, a0, a1); load_row(1, bl, b0, b1);
        for (int y = 0; y < H; y += 2) {
            unsigned nl, n0, n1;
            load_row(y + 2, nl, n0, n1);
            dp_row(y, al, a0, a1, Q1, Q2, P1, P2);
            al = nl; a0 = n0; a1 = n1;
            if (y + 1 < H) {
                load_row(y + 3, nl, n0, n1);
                dp_row(y + 1, bl, b0, b1, Q2, Q1, P2, P1);
                bl = nl; b0 = n0; b1 = n1;
            }
        }
        __threadfence();       // the next strip reads this one's records, the traceback the whole plane: same wave, but through memory
    }

    if (lane == 0) n_cells[blockIdx.x] = path_traceback(plane, nwords, bx, H, Wd, cells + 2 * bx.cell_off);
}

}  // namespace acx
