// EarlyFusion: EVERY matched section of a pair, not only the best alignment.
//
//   ef_sections_kernel   ef_align_kernel's sweep, run per FREE INTERVAL of the plot's rows: section 0 is section 19's alignment; the
//                        rows of a section found (and `pad` rows on either side, clipped to the free interval it lies in) become
//                        excluded, T is 0 on them, and the next section is the alignment of what is left.  One wave per job (pair),
//                        16 columns per lane; the loop over sections and every traceback run inside the launch.
//
// The contract is section 19's (ef_align_kernels.hpp) on the masked matrix T': the same integer tenths, end = row-major first maximum,
// the same predecessor chains.  On an excluded row T' = 0 and U' = (B ? 0 : -7) -- what rows 0 and 1 hold.  A section scores more than
// 1.0 (the host refuses min_score <= 1), so it has two cells in two rows, every excluded stretch has at least two rows, and the
// recursion -- it reaches back two rows at most -- never crosses one.  Hence T' on a free interval [a, b] is the plain recursion over
// rows lo = max(a, 2) .. hi = min(b, M - 2) started from the BITS of rows lo - 1 and lo - 2, independent of every other interval:
//   * a sweep per free interval: no test of the row inside the unrolled row body, which is ef_align_kernel's (a copy: that kernel's
//     listing stays as it is);
//   * one best record (value, end cell) per free interval; a section splits ONE interval, and only its two remainders are swept
//     again -- their rows of the direction plane are overwritten, every other interval's codes and record still hold;
//   * the next section is the best of the records by (value, then smaller end cell): the row-major rule across intervals;
//   * the traceback of a section stays inside its interval: a predecessor in a row above lo has T' = 0 and ends the chain, and no
//     code of a row outside lo .. hi is read (the rows above may hold the codes of an earlier round).
// An interval of fewer than two counted rows holds no score above 1 and is not swept.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/acx.h"
#include "ef_align_kernels.hpp"    // EfAlignJob, EFA_CPL, EFA_REC, ef_align_store, ef_align_dir_words

namespace acx {

constexpr int EFS_MAX = 16;                       // sections of one pair, at most (acx_section_opts.max_sections)

// The cells all sections of an M x N plot can have together: their row ranges are disjoint and a path has at most one cell per row
// (M in all), and at most min(M, N) cells each.  A job's room in `cells` (EfAlignJob.max_cells).
__host__ __device__ __forceinline__ int64_t ef_sections_room(int M, int N, int S)
{
    const int64_t side = M < N ? M : N;
    return (int64_t)S * side < M ? (int64_t)S * side : (int64_t)M;
}

// ef_align_traceback with a lower row bound: the chain of a section in the free interval whose first swept row is `lo` -- rows
// lo - 1 and lo - 2 hold T' = 0 as rows 0 and 1 do, so a predecessor above lo ends the chain, and the rows above lo are never read.
__device__ __forceinline__ int ef_sections_traceback(const unsigned *plane, int64_t wpr, int lo, int hi, int N, int y1, int x1, int max_cells,
                                                     int32_t *dst, int &y0, int &x0)
{
    auto code_at = [&](int yy, int xx) -> unsigned {
        const unsigned wd = __hip_atomic_load(plane + (size_t)yy * wpr + (xx >> 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return (wd >> (2 * (xx & 15))) & 3u;
    };
    int x = x1, y = y1, n = 0;
    if (y >= lo && y <= hi && x >= 2 && x <= N - 2) {
        unsigned code = code_at(y, x);
        while (code != 0u && n < max_cells) {
            dst[2 * n] = y; dst[2 * n + 1] = x;
            ++n;
            const int py = y - (code == 2u ? 2 : 1), px = x - (code == 3u ? 2 : 1);
            if (py < lo || px < 2) break;                            // an excluded row (or rows / columns 0, 1): T' = 0
            code = code_at(py, px);                                  // 0: T' == 0 there, (y, x) was the start
            if (code != 0u) { y = py; x = px; }
        }
    }
    y0 = y; x0 = x;
    return n;
}

// res: the number of sections of every job (gridDim.x words), then max_sections records of EFA_REC words per job -- acx_alignment's
// five fields and the section's number of cells; the no-match record behind the count --, then the cells of all jobs: a job's
// sections behind one another from job.cell_off, each END FIRST, job.max_cells = ef_sections_room() in all.
__global__ __launch_bounds__(64) void ef_sections_kernel(const EfPair *__restrict__ pd, const EfAlignJob *__restrict__ jobs,
                                                         const unsigned *__restrict__ bits, unsigned *dir,
                                                         int32_t *__restrict__ res, int plane,
                                                         int max_sections, int pad, float min_score, float min_ratio)
{
    // the free intervals [a, b] of the plot's rows (either may be empty: a > b) and the best record of each; wave-uniform
    __shared__ int iv_a[EFS_MAX + 1], iv_b[EFS_MAX + 1];
    __shared__ int iv_v[EFS_MAX + 1], iv_e[EFS_MAX + 1];             // tenths, and the end cell row * EF_MAXNB + column
    constexpr int CPL = EFA_CPL;
    const int lane = threadIdx.x;
    const EfAlignJob job = jobs[blockIdx.x];
    const EfPair P = pd[job.pair];
    const int M = P.M, N = P.N, pitch = P.pitchC;
    const int S = min(max(max_sections, 1), EFS_MAX);
    pad = min(max(pad, 0), EF_MAXNB);                                // (q1 + pad stays small)
    int32_t *rec = res + gridDim.x + (size_t)EFA_REC * S * blockIdx.x;
    int32_t *cells = res + gridDim.x + (size_t)EFA_REC * S * gridDim.x + 2 * job.cell_off;
    const int side = min(M, N);
    int found = 0, used = 0;
    if (M >= 4 && N >= 4 && M <= EF_MAXNB && N <= EF_MAXNB) {
        const unsigned char *rows = reinterpret_cast<const unsigned char *>(bits + P.offB + (int64_t)plane * M * (pitch >> 5));
        const int rowbytes = pitch >> 3, wpr = pitch / CPL;
        unsigned *my_dir = dir + job.dir_off;
        const int j0 = CPL * lane;
        const bool inrow = j0 < pitch;
        auto load = [&](int row) -> unsigned {
            const int r = row < M ? row : M - 1;                     // (rows past the last one: a valid address, never used)
            return inrow ? (unsigned)*reinterpret_cast<const unsigned short *>(rows + (size_t)r * rowbytes + 2 * lane) : 0u;
        };
        // valid: bit e = column j0 + e is counted (2 <= j <= N - 2), as in ef_align_kernel
        unsigned valid = 0u;
#pragma unroll
        for (int e = 0; e < CPL; ++e) valid |= (j0 + e >= 2 && j0 + e <= N - 2) ? (1u << e) : 0u;

        if (lane == 0) { iv_a[0] = 0; iv_b[0] = M - 1; }
        __syncthreads();
        int n_iv = 1;
        int npend = 1, pend0 = 0, pend1 = 0;                         // the intervals whose records the next round computes
        float score0 = 0.0f;

        for (;;) {
            for (int t = 0; t < npend; ++t) {
                const int idx = t == 0 ? pend0 : pend1;
                const int lo = max(__builtin_amdgcn_readfirstlane(iv_a[idx]), 2);         // rows 0 and 1 of T stay zero
                const int hi = min(__builtin_amdgcn_readfirstlane(iv_b[idx]), M - 2);
                int best = 0, best_cell = 0x7fffffff;
                if (hi - lo >= 1) {
                    // A cell is held as V = 4 (U + 8), ef_align_kernel's way: key = max3(V + 2, V + 1, V + 0) of the three predecessors
                    // gives the maximum and which one it is; 4 T = max(0, (key & ~3) - 32 +- 40), new V = 4 T + (B ? 32 : 4).
                    int V1[CPL], V2[CPL];                            // rows i-1, i-2
                    {
                        const unsigned w0 = load(lo - 2), w1 = load(lo - 1);              // T' = 0 there, U' = delta(B)
#pragma unroll
                        for (int e = 0; e < CPL; ++e) {
                            V2[e] = 4 + 28 * (int)((w0 >> e) & 1u);
                            V1[e] = 4 + 28 * (int)((w1 >> e) & 1u);
                        }
                    }
                    // the running maximum of a lane as ONE integer, (4 T) << 14 | (1023 - i) << 4 | (15 - e)
                    int best_key = 0;
                    // one row: VA = row i-1, VB = row i-2 (overwritten with row i, from the right)
                    auto dp_row = [&](int i, unsigned wb, int (&VA)[CPL], int (&VB)[CPL]) {
                        const int a1 = lane_prev_i(VA[CPL - 1]), a2 = lane_prev_i(VA[CPL - 2]), b1 = lane_prev_i(VB[CPL - 1]);
                        const int row_key = (EF_MAXNB - 1 - i) << 4;
                        unsigned codes = 0u;
                        // (opaque per row: sixteen loop-invariant lane masks hoisted out of the row loop would take 32 SGPRs and spill)
                        int vm = (int)valid;
                        asm volatile("" : "+v"(vm));
#pragma unroll
                        for (int e = CPL - 1; e >= 0; --e) {
                            const int k2 = ((e >= 1) ? VA[e - 1] : a1) + 2;                           // (i-1, j-1)
                            const int k3 = ((e >= 1) ? VB[e - 1] : b1) + 1;                           // (i-2, j-1)
                            const int k4 = (e >= 2) ? VA[e - 2] : (e == 1 ? a1 : a2);                 // (i-1, j-2)
                            const int key = max(max(k2, k3), k4);
                            const int bit = (int)((wb >> e) & 1u);
                            int t4 = (key & ~3) - 72 + 80 * bit;
                            t4 = max(t4, 0) & __builtin_amdgcn_sbfe(vm, e, 1);                // (sbfe of one bit: 0 or -1)
                            VB[e] = t4 + 4 + 28 * bit;
                            const unsigned code = t4 > 0 ? 3u - (unsigned)(key & 3) : 0u;
                            codes |= code << (2 * e);
                            best_key = max(best_key, ((t4 << 14) | (15 - e)) | row_key);
                        }
                        if (inrow) my_dir[(size_t)i * wpr + lane] = codes;
                    };
                    // the 8-row ring starts at the interval's first row, whatever its row & 7; the register rows only alternate, so
                    // the interval may begin on either parity: row lo - 1 is V1, and 8 is even
                    constexpr int SW_PF = 8;
                    unsigned ring[SW_PF];
#pragma unroll
                    for (int sl = 0; sl < SW_PF; ++sl) ring[sl] = load(lo + sl);
                    for (int i0 = lo; i0 <= hi; i0 += SW_PF) {
#pragma unroll
                        for (int sl = 0; sl < SW_PF; ++sl) {
                            const int i = i0 + sl;
                            if (i <= hi) {                           // wave-uniform
                                const unsigned wb = ring[sl];
                                ring[sl] = load(i + SW_PF);
                                if (sl & 1) dp_row(i, wb, V2, V1); else dp_row(i, wb, V1, V2);
                            }
                        }
                    }
                    // the maximum and, among equal maxima, the smallest cell index
                    best = best_key >> 16;                           // tenths: (4 T) >> 2
                    best_cell = best > 0 ? (EF_MAXNB - 1 - ((best_key >> 4) & (EF_MAXNB - 1))) * EF_MAXNB + j0 + 15 - (best_key & 15) : 0x7fffffff;
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) {
                        const int ob = __shfl_xor(best, o, 64), oc = __shfl_xor(best_cell, o, 64);
                        if (ob > best || (ob == best && oc < best_cell)) { best = ob; best_cell = oc; }
                    }
                }
                if (lane == 0) { iv_v[idx] = best; iv_e[idx] = best_cell; }
            }
            // the tracebacks read the plane: same wave, but other lanes' stores, through memory
            __threadfence();
            __syncthreads();

            // the next section: the best of the interval records
            int bv = 0, be = 0x7fffffff, bi = -1;
            for (int t = 0; t < n_iv; ++t) {
                const int v = iv_v[t], e = iv_e[t];
                if (v > bv || (v == bv && v > 0 && e < be)) { bv = v; be = e; bi = t; }
            }
            bi = __builtin_amdgcn_readfirstlane(bi);
            bv = __builtin_amdgcn_readfirstlane(bv);
            be = __builtin_amdgcn_readfirstlane(be);
            if (bi < 0) break;
            const float score = (float)bv / 10.0f;                   // ef_align_kernel's expression: the same bits
            const float thr = found == 0 ? min_score : fmaxf(min_score, min_ratio * score0);
            if (!(score >= thr)) break;
            if (found == 0) score0 = score;
            const int a = __builtin_amdgcn_readfirstlane(iv_a[bi]), b = __builtin_amdgcn_readfirstlane(iv_b[bi]);
            const int q1 = be / EF_MAXNB, r1 = be % EF_MAXNB;
            int y = 0, x = 0, n = 0;
            if (lane == 0) {
                n = ef_sections_traceback(my_dir, wpr, max(a, 2), min(b, M - 2), N, q1, r1, min(side, job.max_cells - used),
                                          cells + 2 * used, y, x);
                acx_alignment al;
                al.score = score;                                    // (a positive score without a cell: the driver reports it)
                al.q0 = al.r0 = al.q1 = al.r1 = -1;
                if (n > 0) { al.q0 = y; al.r0 = x; al.q1 = q1; al.r1 = r1; }
                ef_align_store(rec + (size_t)EFA_REC * found, al, n);
            }
            n = __builtin_amdgcn_readfirstlane(n);
            const int q0 = __builtin_amdgcn_readfirstlane(y);
            used += n;
            ++found;
            if (found == S || n == 0) break;
            // rows [max(a, q0 - pad), min(b, q1 + pad)] of the section's interval [a, b] become excluded; what is left above and below
            __syncthreads();
            if (lane == 0) {
                iv_b[bi] = max(a, q0 - pad) - 1;
                iv_a[n_iv] = min(b, q1 + pad) + 1; iv_b[n_iv] = b;
            }
            __syncthreads();
            pend0 = bi; pend1 = n_iv; npend = 2;
            ++n_iv;
        }
    }
    if (lane == 0) {
        res[blockIdx.x] = found;
        acx_alignment none;
        none.score = 0.0f; none.q0 = none.r0 = none.q1 = none.r1 = -1;
        for (int k = found; k < S; ++k) ef_align_store(rec + (size_t)EFA_REC * k, none, 0);
    }
}

}  // namespace acx
