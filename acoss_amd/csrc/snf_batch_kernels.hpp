// Fused query shortlists (acx_query_fused_lists): many small similarity network fusions side by side.
//
// A chunk holds P independent problems (fused_plan.hpp: FusedProb), problem p a neighbourhood of n_p tracks with its own
// matrices in the chunk's matrix arena.  Every stage of snf_prepare / snf_update (acx.hip) runs for ALL problems in one
// launch: the problem index is the last grid dimension, the leading dimensions cover the largest problem and a block
// beyond its problem's extent leaves at once (before any barrier).  The work of a block is the row body of
// snf_kernels.hpp, called with the problem's pointers and n: per problem the operations, their order and so the bits are
// those of the single-problem kernels.  A matrix is named by its slot in the problem's part of the arena (fused_plan.hpp).
//   B0  fused_stage_kernel       pair scores of the slab -> the m dense n x n f64 distance matrices of a fused type
//                                (mirrored, per-class transform), and the type's non-finite flag per problem
//   B1..B8  snf_batch_*_kernel   sym, localscale, affinity, knn, rownorm, mean, ast, sut
//   B9  fused_row_kernel         row q of the fused matrix, rounded once to f32, ranked by rank_select_sort: the first k
//                                tracks of the neighbourhood as collection indices
// A neighbourhood holds at most 1025 tracks: a row of doubles (8 KB) and a row of floats fit the default LDS.
// Every store is a plain C++ store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fused_plan.hpp"
#include "rank_kernels.hpp"
#include "snf_kernels.hpp"

namespace acx {

// the planes of one fused type, in fusion order: the pair kernels' plane index of each
struct FusedPlanes { int32_t p[FUSED_MAX_PLANES]; int32_t count; };
// matrices by slot: the sources of a mean
struct SnfSlots { int32_t s[8]; int32_t count; };

__device__ __forceinline__ double *snf_slot(double *mats, const FusedProb &pr, int slot)
{
    return mats + pr.mat + (int64_t)slot * pr.n * pr.n;
}

// B0.  grid: (ceil(max n^2 / 256), P).  slab[(pr.pair + pair index) W + e]: plane e of the pair (min, max).
// transform 1 (ChenFusion): D[i][j] = (double)(float)(col[T[j]] / (double)s) -- normalize_by_length's f32 value of column j,
// widened; 2 (EarlyFusion): 1 / (1 + (double)s).  The diagonal is 0 (snf_sym_kernel zeroes it whatever it holds).
// flag[p * flag_stride] = 1 where an off-diagonal distance is not finite (zeroed by the host before).
__global__ __launch_bounds__(256) void fused_stage_kernel(const FusedProb *__restrict__ probs, const float *__restrict__ slab, int W,
                                                          const double *__restrict__ col, const int32_t *__restrict__ tracks, FusedPlanes pl,
                                                          int transform, double *__restrict__ mats, uint8_t *__restrict__ flag, int flag_stride)
{
    const FusedProb pr = probs[blockIdx.y];
    const int n = pr.n;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)n * n) return;
    const int i = (int)(e / n), j = (int)(e - (int64_t)i * n);
    if (i == j) {
        for (int t = 0; t < pl.count; ++t) snf_slot(mats, pr, t)[e] = 0.0;
        return;
    }
    const int a = i < j ? i : j, b = i < j ? j : i;
    const float *s = slab + (pr.pair + fused_pair_index(n, a, b)) * W;
    const double cj = transform == 1 ? col[tracks[pr.tracks + j]] : 0.0;
    bool bad = false;
    for (int t = 0; t < pl.count; ++t) {
        const double sv = (double)s[pl.p[t]];
        const double d = transform == 1 ? (double)(float)(cj / sv) : 1.0 / (1.0 + sv);
        snf_slot(mats, pr, t)[e] = d;
        bad |= !(fabs(d) <= 1.79769313486231570815e+308);
    }
    if (bad) flag[(int64_t)blockIdx.y * flag_stride] = 1;
}

// B1.  grid: (ceil(max n / 32), ceil(max n / 32), P)
__global__ __launch_bounds__(256) void snf_batch_sym_kernel(const FusedProb *__restrict__ probs, double *__restrict__ mats, int src, int dst)
{
    __shared__ double tile[32][33];
    const FusedProb pr = probs[blockIdx.z];
    if ((int)blockIdx.x * 32 >= pr.n || (int)blockIdx.y * 32 >= pr.n) return;
    snf_sym_tile(snf_slot(mats, pr, src), snf_slot(mats, pr, dst), pr.n, (int)blockIdx.x, (int)blockIdx.y, tile);
}

// B2.  grid: (ceil(max n / 4), P)
__global__ __launch_bounds__(256) void snf_batch_localscale_kernel(const FusedProb *__restrict__ probs, double *__restrict__ mats, int S, int md, int K)
{
    const FusedProb pr = probs[blockIdx.y];
    if ((int)blockIdx.x * 4 >= pr.n) return;
    snf_localscale_rows(snf_slot(mats, pr, S), snf_slot(mats, pr, md), pr.n, K, (int)blockIdx.x);
}

// B3.  grid: (ceil(max n^2 / 256), P)
__global__ __launch_bounds__(256) void snf_batch_affinity_kernel(const FusedProb *__restrict__ probs, double *__restrict__ mats, int S, int md, double mu)
{
    const FusedProb pr = probs[blockIdx.y];
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)pr.n * pr.n) return;
    snf_affinity_cell(snf_slot(mats, pr, S), snf_slot(mats, pr, md), pr.n, mu, e);
}

// B4.  grid: (ceil(max n / 4), P).  The lists of plane `plane`: pr.list + plane n K entries into J and V.
__global__ __launch_bounds__(256) void snf_batch_knn_kernel(const FusedProb *__restrict__ probs, double *__restrict__ mats, int Wm, int32_t *__restrict__ J,
                                                            double *__restrict__ V, int plane, int K)
{
    __shared__ double cv[4][64];
    __shared__ int cj[4][64];
    const FusedProb pr = probs[blockIdx.y];
    if ((int)blockIdx.x * 4 >= pr.n) return;
    const int64_t at = pr.list + (int64_t)plane * pr.n * K;
    snf_knn_rows(snf_slot(mats, pr, Wm), J + at, V + at, pr.n, K, (int)blockIdx.x, cv, cj);
}

// B5.  grid: (max n, P)
__global__ __launch_bounds__(256) void snf_batch_rownorm_kernel(const FusedProb *__restrict__ probs, double *__restrict__ mats, int Wm, int Pm)
{
    __shared__ double part[256];
    const FusedProb pr = probs[blockIdx.y];
    if ((int)blockIdx.x >= pr.n) return;
    snf_rownorm_row(snf_slot(mats, pr, Wm), snf_slot(mats, pr, Pm), pr.n, (int)blockIdx.x, part);
}

// B6.  grid: (ceil(max n^2 / 256), P)
__global__ __launch_bounds__(256) void snf_batch_mean_kernel(const FusedProb *__restrict__ probs, double *__restrict__ mats, SnfSlots srcs, double scale,
                                                             int acc)
{
    const FusedProb pr = probs[blockIdx.y];
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)pr.n * pr.n) return;
    SnfSrc sp;
    sp.count = srcs.count;
    for (int k = 0; k < srcs.count; ++k) sp.p[k] = snf_slot(mats, pr, srcs.s[k]);
    snf_mean_cell(sp, scale, snf_slot(mats, pr, acc), e);
}

// B7.  grid: (max n, P); dynamic LDS: max n doubles (the row of A, as snf_ast_kernel<true> keeps it)
__global__ __launch_bounds__(256) void snf_batch_ast_kernel(const FusedProb *__restrict__ probs, double *__restrict__ mats, int A, int UT,
                                                            const int32_t *__restrict__ J, const double *__restrict__ V, int plane, int K)
{
    extern __shared__ double row[];
    const FusedProb pr = probs[blockIdx.y];
    if ((int)blockIdx.x >= pr.n) return;
    const int64_t at = pr.list + (int64_t)plane * pr.n * K;
    snf_ast_row<true>(snf_slot(mats, pr, A), J + at, V + at, snf_slot(mats, pr, UT), pr.n, K, (int)blockIdx.x, row);
}

// B8.  grid: (max n, P)
__global__ __launch_bounds__(256) void snf_batch_sut_kernel(const FusedProb *__restrict__ probs, double *__restrict__ mats, int UT, int Pm,
                                                            const int32_t *__restrict__ J, const double *__restrict__ V, int plane, int K, double reg_diag)
{
    const FusedProb pr = probs[blockIdx.y];
    if ((int)blockIdx.x >= pr.n) return;
    const int64_t at = pr.list + (int64_t)plane * pr.n * K;
    snf_sut_row(snf_slot(mats, pr, UT), J + at, V + at, snf_slot(mats, pr, Pm), pr.n, K, reg_diag, (int)blockIdx.x);
}

// B9.  grid: (P).  Row pr.qpos of the fused matrix in slot `F`: every value rounded ONCE to f32 into LDS, the query's own
// column left out, ranked in the order of rank_kernels.hpp with the collection index as tie rank (T ascends: the order of
// acx_topk_rows on the row), reported as collection indices.  out_idx / out_score: P x out_stride, this type's k at `out_at`.
// P2 = the power of two >= max(4, min(k, max n - 1)).  Dynamic LDS: 12 P2 + RANK_SELECT_LDS_FIXED + 4 max n.
__global__ __launch_bounds__(RANK_THREADS) void fused_row_kernel(const FusedProb *__restrict__ probs, const double *__restrict__ mats, int F,
                                                                 const int32_t *__restrict__ tracks, int k, int P2, int32_t *__restrict__ out_idx,
                                                                 float *__restrict__ out_score, int out_stride, int out_at)
{
    extern __shared__ float4 rank_lds4[];
    float *lrow = rank_select_row(rank_lds4, P2);
    const FusedProb pr = probs[blockIdx.x];
    const int n = pr.n, tid = threadIdx.x;
    const double *row = mats + pr.mat + (int64_t)F * n * n + (int64_t)pr.qpos * n;
    const int32_t *T = tracks + pr.tracks;
    for (int j = tid; j < n; j += RANK_THREADS) lrow[j] = (float)row[j];
    rank_select_sort(rank_lds4, n, n - 1, k, P2, [&](int j, int &pos, uint64_t &key) {
        if (j == pr.qpos) return false;
        pos = j;
        key = rank_key64(lrow[j], (uint32_t)T[j]);
        return true;
    });
    const int32_t *spos = rank_select_columns(rank_lds4, P2);
    const int64_t o = (int64_t)blockIdx.x * out_stride + out_at;
    for (int p = tid; p < k; p += RANK_THREADS) {
        const int j = p < P2 ? spos[p] : -1;
        out_idx[o + p] = j >= 0 ? T[j] : -1;
        out_score[o + p] = j >= 0 ? lrow[j] : __builtin_nanf("");
    }
}

}  // namespace acx
