// EarlyFusion: EVERY matched section of a pair, not only the best alignment.
//
//   ef_sections_kernel   ef_align_kernel's sweep (ef_align_sweep), run per FREE INTERVAL of the plot's rows: section 0 is section 19's
//                        alignment; the rows of a section found (and `pad` rows on either side, clipped to the free interval it lies
//                        in) become excluded, T is 0 on them, and the next section is the alignment of what is left.  One wave per job
//                        (pair), 16 columns per lane; the loop over sections and every traceback run inside the launch.
//
// The contract is section 19's (ef_align_kernels.hpp) on the masked matrix T': the same integer tenths, end = row-major first maximum,
// the same predecessor chains.  On an excluded row T' = 0 and U' = (B ? 0 : -7) -- what rows 0 and 1 hold.  A section scores more than
// 1.0 (the host refuses min_score <= 1), so it has two cells in two rows, every excluded stretch has at least two rows, and the
// recursion -- it reaches back two rows at most -- never crosses one.  Hence T' on a free interval [a, b] is the plain recursion over
// rows lo = max(a, 2) .. hi = min(b, M - 2) started from the BITS of rows lo - 1 and lo - 2, independent of every other interval:
//   * a sweep per free interval: no test of the row inside the unrolled row body;
//   * one best record (value, end cell) per free interval; a section splits ONE interval, and only its two remainders are swept
//     again -- their rows of the direction plane are overwritten, every other interval's codes and record still hold;
//   * the next section is the best of the records by (value, then smaller end cell): the row-major rule across intervals;
//   * the traceback of a section stays inside its interval (ef_align_traceback's row bounds).
// An interval of fewer than two counted rows holds no score above 1 and is not swept.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/acx.h"
#include "ef_align_kernels.hpp"    // EfAlignJob, EFA_CPL, EFA_REC, ef_align_sweep, ef_align_traceback, ef_align_store
#include "sections_common.hpp"

namespace acx {

// The cells all sections of an M x N plot can have together: their row ranges are disjoint and a path has at most one cell per row
// (M in all), and at most min(M, N) cells each.  A job's room in `cells` (EfAlignJob.max_cells).
__host__ __device__ __forceinline__ int64_t ef_sections_room(int M, int N, int S)
{
    const int64_t side = M < N ? M : N;
    return (int64_t)S * side < M ? (int64_t)S * side : (int64_t)M;
}

// res: the number of sections of every job (gridDim.x words), then max_sections records of EFA_REC words per job -- acx_alignment's
// five fields and the section's number of cells; the no-match record behind the count --, then the cells of all jobs: a job's
// sections behind one another from job.cell_off, each END FIRST, job.max_cells = ef_sections_room() in all.
__global__ __launch_bounds__(64) void ef_sections_kernel(const EfPair *__restrict__ pd, const EfAlignJob *__restrict__ jobs,
                                                         const unsigned *__restrict__ bits, unsigned *dir,
                                                         int32_t *__restrict__ res, int plane,
                                                         int max_sections, int pad, float min_score, float min_ratio)
{
    __shared__ SecIntervals iv;
    __shared__ int iv_v[SEC_MAX + 1], iv_e[SEC_MAX + 1];             // an interval's best record: tenths, and the end cell row * EF_MAXNB + column
    const int lane = threadIdx.x;
    const EfAlignJob job = jobs[blockIdx.x];
    const EfPair P = pd[job.pair];
    const int M = P.M, N = P.N, pitch = P.pitchC;
    const int S = min(max(max_sections, 1), SEC_MAX);
    pad = min(max(pad, 0), EF_MAXNB);                                // (q1 + pad stays small)
    int32_t *rec = res + gridDim.x + (size_t)EFA_REC * S * blockIdx.x;
    int32_t *cells = res + gridDim.x + (size_t)EFA_REC * S * gridDim.x + 2 * job.cell_off;
    const int side = min(M, N);
    int found = 0, used = 0;
    if (M >= 4 && N >= 4 && M <= EF_MAXNB && N <= EF_MAXNB) {
        const unsigned char *rows = reinterpret_cast<const unsigned char *>(bits + P.offB + (int64_t)plane * M * (pitch >> 5));
        unsigned *my_dir = dir + job.dir_off;

        if (lane == 0) { iv.a[0] = 0; iv.b[0] = M - 1; }
        __syncthreads();
        int n_iv = 1;
        int npend = 1, pend0 = 0, pend1 = 0;                         // the intervals whose records the next round computes
        float score0 = 0.0f;

        for (;;) {
            for (int t = 0; t < npend; ++t) {
                const int idx = t == 0 ? pend0 : pend1;
                const int lo = max(__builtin_amdgcn_readfirstlane(iv.a[idx]), 2);         // rows 0 and 1 of T stay zero
                const int hi = min(__builtin_amdgcn_readfirstlane(iv.b[idx]), M - 2);
                EfBest best = {0, 0x7fffffff};
                if (hi - lo >= 1) best = ef_align_sweep(rows, M, N, pitch, my_dir, lo, hi);
                if (lane == 0) { iv_v[idx] = best.tenths; iv_e[idx] = best.cell; }
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
            if (!(score >= sec_threshold(found, score0, min_score, min_ratio))) break;
            if (found == 0) score0 = score;
            const int a = __builtin_amdgcn_readfirstlane(iv.a[bi]), b = __builtin_amdgcn_readfirstlane(iv.b[bi]);
            const int q1 = be / EF_MAXNB, r1 = be % EF_MAXNB;
            int y = 0, x = 0, n = 0;
            if (lane == 0) {
                n = ef_align_traceback(my_dir, pitch / EFA_CPL, max(a, 2), min(b, M - 2), N, q1, r1, min(side, job.max_cells - used),
                                       cells + 2 * used, y, x);
                acx_alignment al = sec_no_match();
                al.score = score;                                    // (a positive score without a cell: the driver reports it)
                if (n > 0) { al.q0 = y; al.r0 = x; al.q1 = q1; al.r1 = r1; }
                ef_align_store(rec + (size_t)EFA_REC * found, al, n);
            }
            n = __builtin_amdgcn_readfirstlane(n);
            const int q0 = __builtin_amdgcn_readfirstlane(y);
            used += n;
            ++found;
            if (found == S || n == 0) break;
            sec_split(iv, bi, n_iv, a, b, q0, q1, pad);
            pend0 = bi; pend1 = n_iv; npend = 2;
            ++n_iv;
        }
    }
    if (lane == 0) {
        res[blockIdx.x] = found;
        for (int k = found; k < S; ++k) ef_align_store(rec + (size_t)EFA_REC * k, sec_no_match(), 0);
    }
}

}  // namespace acx
