// Serra09: EVERY matched section of a pair, not only the best one.
//
//   S1 qmax_sections_kernel<EQG>  qmax_locate_kernel's sweep (qmax_locate_sweep), run per FREE INTERVAL of the plot's rows: section 0
//                                 is section 16's alignment; the rows of a section found (and `pad` rows on either side, clipped to
//                                 the free interval it lies in) become excluded, Q is 0 on them, and the next section is the alignment
//                                 of what is left.  One wave per pair, 32 columns per lane, strips of 2048 columns; the loop over
//                                 sections runs inside the launch.
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
#include "serra09_kernels.hpp"          // PairDesc
#include "serra09_locate_kernels.hpp"   // LocSeam, loc_strips, qmax_locate_sweep
#include "sections_common.hpp"

namespace acx {

template <bool EQG>
__global__ __launch_bounds__(64) void qmax_sections_kernel(const PairDesc *__restrict__ pd,
                                                           const unsigned long long *__restrict__ bits,
                                                           LocSeam *__restrict__ seam, const int64_t *__restrict__ seam_off,
                                                           acx_alignment *__restrict__ out, int32_t *__restrict__ n_out,
                                                           float go, float ge, int dp_start,
                                                           int max_sections, int pad, float min_score, float min_ratio)
{
    __shared__ SecIntervals iv;
    __shared__ float iv_v[SEC_MAX + 1];            // an interval's best record: max Q', its first cell and that cell's path start
    __shared__ unsigned iv_e[SEC_MAX + 1], iv_s[SEC_MAX + 1];
    const int lane = threadIdx.x;
    const PairDesc P = pd[blockIdx.x];
    int Me = P.Mq, Ne = P.Mr;
    if (dp_start == 3) { Me -= 1; Ne -= 1; }       // as in qmax_locate_kernel: the same DP on the plot less its last row / column
    const unsigned W = (unsigned)P.Mr;             // S = i * W + j
    LocSeam *bnd = loc_strips(Ne) > 1 ? seam + seam_off[blockIdx.x] : nullptr;
    const int S = min(max(max_sections, 1), SEC_MAX);
    pad = min(max(pad, 0), P.Mq);                  // (q1 + pad stays an int)
    acx_alignment *rec = out + (size_t)blockIdx.x * S;

    if (lane == 0) { iv.a[0] = 0; iv.b[0] = P.Mq - 1; }
    __syncthreads();
    int n_iv = 1, found = 0;
    int npend = 1, pend0 = 0, pend1 = 0;           // the intervals whose records the next round computes
    float score0 = 0.0f;

    for (;;) {
        for (int t = 0; t < npend; ++t) {
            const int idx = t == 0 ? pend0 : pend1;
            const int lo = max(__builtin_amdgcn_readfirstlane(iv.a[idx]), 2);             // rows 0 and 1 of Q stay zero
            const int hi = min(__builtin_amdgcn_readfirstlane(iv.b[idx]), Me - 1);
            LocBest best = {0.0f, 0u, 0u};
            if (hi - lo >= 1) best = qmax_locate_sweep<EQG>(P, bits, bnd, Me, Ne, go, ge, lo, hi);
            if (lane == 0) { iv_v[idx] = best.best; iv_e[idx] = best.end; iv_s[idx] = best.start; }
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
        if (!(bv >= sec_threshold(found, score0, min_score, min_ratio))) break;
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
        const int a = __builtin_amdgcn_readfirstlane(iv.a[bi]), b = __builtin_amdgcn_readfirstlane(iv.b[bi]);
        sec_split(iv, bi, n_iv, a, b, q0, q1, pad);
        pend0 = bi; pend1 = n_iv; npend = 2;
        ++n_iv;
    }

    if (lane == 0) {
        n_out[blockIdx.x] = found;
        for (int k = found; k < S; ++k) rec[k] = sec_no_match();
    }
}

}  // namespace acx
