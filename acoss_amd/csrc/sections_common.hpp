// What qmax_sections_kernel and ef_sections_kernel share (DESIGN.md sections 28 and 29): the FREE INTERVALS of a plot's rows, in LDS
// and wave-uniform, which a section splits.  An interval's best record, picking the best and emitting a section differ (f32 value and
// start cell; tenths and a traceback) and stay in the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/acx.h"

namespace acx {

constexpr int SEC_MAX = 16;                    // sections of one pair, at most (acx_section_opts.max_sections)

// the free intervals [a, b] of the plot's rows (either may be empty: a > b); a kernel declares one __shared__
struct SecIntervals { int a[SEC_MAX + 1], b[SEC_MAX + 1]; };

// what a section must score: min_score, and from the second section on min_ratio of the first one's score as well
__device__ __forceinline__ float sec_threshold(int found, float score0, float min_score, float min_ratio)
{
    return found == 0 ? min_score : fmaxf(min_score, min_ratio * score0);
}

// Rows [max(a, q0 - pad), min(b, q1 + pad)] of interval bi = [a, b], in which the section of rows q0 .. q1 lies, become excluded:
// what is left above stays interval bi, what is left below becomes interval n_iv.  Every lane calls it.
__device__ __forceinline__ void sec_split(SecIntervals &iv, int bi, int n_iv, int a, int b, int q0, int q1, int pad)
{
    __syncthreads();
    if (threadIdx.x == 0) { iv.b[bi] = max(a, q0 - pad) - 1; iv.a[n_iv] = min(b, q1 + pad) + 1; iv.b[n_iv] = b; }
    __syncthreads();
}

// the record behind a pair's last section
__device__ __forceinline__ acx_alignment sec_no_match() { return {0.0f, -1, -1, -1, -1}; }

}  // namespace acx
