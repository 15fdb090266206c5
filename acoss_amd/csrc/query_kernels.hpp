// Finish of a query band (acx_query_scores / acx_query_topk / acx_query_ranks, include/acx.h): from the band's score slab
// to finished rows, ranked candidate lists or the positions of listed tracks without leaving the device.
//
// The slab is what the pair kernels' scatter left behind: R rows (the band's queries) x N columns (every track of the
// pool) x W planes, plane fastest -- slab[(r N + c) W + e] = score plane e of the pair {query r, track c} in the
// orientation the call selected.  A query's own cell is never computed (it holds 0 from the band's memset and is never
// read as a score).
//   value of a cell   col_mode 0: s    1: (float)((double)s / col[c])    2: -(float)(col[c] / (double)s)
//                     one IEEE f64 division and one rounding to f32: the bits numpy's (D / norm).astype(float32) and
//                     -(norm / D).astype(float32) produce (normalize_by_length of Serra09 / ChenFusion)
//   Q1  query_rows_kernel   the finished rows, de-interleaved: out[e][r N + c], own cell 0
// The order of Q2 and Q3 is the one of rank_kernels.hpp, decided by its rank_select_sort and rank_count_positions:
// larger value first (-0.0 and +0.0 tie), ties by ascending tie rank, NaN after every number.  The kernels here add the
// band: which cells of the slab a row's candidates are, their finishing, and where the results go.
//   Q2  query_topk_kernel   one workgroup per (row, plane): the first k candidates, tie rank = track index.  The
//                           candidates are a strictly ascending track list (or every track); the own track is skipped
//                           also when listed.  Up to RANK_ROW_LDS candidates keep their finished values in LDS (the slab
//                           is read once); more are re-read -- and re-finished, the same operations on the same bits --
//                           per pass.
//   Q3  query_rank_kernel   one workgroup per (row, plane): the 1-based positions of listed tracks (a query's clique
//                           mates) among the row's finished values, ties by posn.  The own column is stored as NaN (no
//                           comparison counts it); a NaN or a -inf anywhere else flags the (row, plane) and its positions
//                           are -1.  Up to RANK_ROW_LDS tracks keep their finished values in LDS; more are re-read -- and
//                           re-finished, the same operations on the same bits -- per pass.
//   Q4  query_topk_lists_kernel   Q2 for a band whose rows each bring their own candidate list (acx_query_topk_lists): the
//                           slab is R x L x W by list position, candidates are positions, empty slots and the own
//                           track are skipped and the valid entries are counted.  Up to RANK_ROW_LDS positions keep
//                           their finished values in LDS; more are re-read and re-finished per pass.
// Every store is a plain C++ store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rank_kernels.hpp"

namespace acx {

__device__ __forceinline__ float query_value(float s, const double *__restrict__ col, int c, int mode)
{
    if (mode == 0) return s;
    if (mode == 1) return (float)((double)s / col[c]);
    return -(float)(col[c] / (double)s);
}

// Q1.  grid: (ceil(N / 256), R, W).  out: W planes of R x N floats.
__global__ __launch_bounds__(256) void query_rows_kernel(const float *__restrict__ slab, int N, int W, int R,
                                                         const int32_t *__restrict__ self_of, const double *__restrict__ col,
                                                         int mode, float *__restrict__ out)
{
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y, e = blockIdx.z;
    if (c >= N) return;
    const float s = slab[((int64_t)r * N + c) * W + e];
    out[((int64_t)e * R + r) * N + c] = c == self_of[r] ? 0.0f : query_value(s, col, c, mode);
}

// Q2.  grid: (R, W).  cands: ncand strictly ascending tracks, or NULL (candidate j is track j, ncand = N).
// out_idx / out_score: R x W x k.  P = the power of two >= max(4, min(k, ncand)) (<= RANK_KMAX): slots of the LDS sort.
// Dynamic LDS: 12 P + RANK_SELECT_LDS_FIXED + IN_LDS ? 4 ncand : 0.
template <bool IN_LDS>
__global__ __launch_bounds__(RANK_THREADS) void query_topk_kernel(const float *__restrict__ slab, int N, int W,
                                                                   const int32_t *__restrict__ self_of,
                                                                   const int32_t *__restrict__ cands, int ncand,
                                                                   const double *__restrict__ col, int mode, int k, int P,
                                                                   int32_t *__restrict__ out_idx, float *__restrict__ out_score)
{
    extern __shared__ float4 rank_lds4[];
    float *lrow = rank_select_row(rank_lds4, P);
    const int r = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
    const float *row = slab + (int64_t)r * N * W + e;
    const int self = self_of[r];
    auto track_of = [&](int j) { return cands ? cands[j] : j; };
    auto value_of = [&](int c) { return query_value(row[(int64_t)c * W], col, c, mode); };
    int mine_self = 0;
    for (int j = tid; j < ncand; j += RANK_THREADS) {
        const int c = track_of(j);
        if (c == self) { mine_self = 1; continue; }
        if (IN_LDS) lrow[j] = value_of(c);
    }
    const int nvalid = ncand - (__syncthreads_or(mine_self) ? 1 : 0);       // candidates there are to list
    rank_select_sort(rank_lds4, ncand, nvalid, k, P, [&](int j, int &c, uint64_t &key) {
        c = track_of(j);
        if (c == self) return false;
        key = rank_key64(IN_LDS ? lrow[j] : value_of(c), (uint32_t)c);      // (the keys are distinct: exactly min(k, nvalid) <= P are taken)
        return true;
    });
    const int32_t *scol = rank_select_columns(rank_lds4, P);
    const int64_t o = ((int64_t)r * W + e) * k;
    for (int p = tid; p < k; p += RANK_THREADS) {
        const int c = p < P ? scol[p] : -1;
        out_idx[o + p] = c;
        out_score[o + p] = c >= 0 ? value_of(c) : __builtin_nanf("");
    }
}

// Q3.  grid: (R, W).  mates[moff[r] - mate_base .. moff[r + 1] - mate_base): the listed tracks of row r (none is the row's
// own track: checked by the host); posn: N distinct tie ranks or NULL (the track index).
// out_pos[e * plane_stride + moff[r] - mate_base + j]: position of the j-th listed track in plane e, or -1 where the
// (row, plane) is flagged; out_flag[r W + e] in {0, 1}.
// Dynamic LDS: RANK_COUNT_LDS_FIXED + IN_LDS ? 16 * ((N + 3) / 4) : 0 (the counters in front: the quads stay on 16 bytes).
template <bool IN_LDS>
__global__ __launch_bounds__(RANK_THREADS) void query_rank_kernel(const float *__restrict__ slab, int N, int W,
                                                                   const int32_t *__restrict__ self_of,
                                                                   const double *__restrict__ col, int mode,
                                                                   const int32_t *__restrict__ posn,
                                                                   const int64_t *__restrict__ moff,
                                                                   const int32_t *__restrict__ mates, int64_t mate_base,
                                                                   int64_t plane_stride, int32_t *__restrict__ out_pos,
                                                                   uint8_t *__restrict__ out_flag)
{
    extern __shared__ float4 rank_lds4[];
    float4 *lrow4 = rank_lds4 + RANK_COUNT_LDS_FIXED / 16;
    float *lrow = reinterpret_cast<float *>(lrow4);
    const int r = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
    const float *row = slab + (int64_t)r * N * W + e;
    const int self = self_of[r];
    const int nq = (N + 3) >> 2;
    // the finished value of column c; the own column and the padding of the last quad are NaN, which no comparison counts
    auto value_of = [&](int c) { return (c < N && c != self) ? query_value(row[(int64_t)c * W], col, c, mode) : __builtin_nanf(""); };
    int nans = 0, minf = 0;
    for (int c = tid; c < 4 * nq; c += RANK_THREADS) {     // (column by column: neighbouring lanes read neighbouring cells)
        const float v = value_of(c);
        if (IN_LDS) lrow[c] = v;
        nans += (v != v) ? 1 : 0;
        minf |= rank_bad(v) ? 1 : 0;
    }
    rank_count_positions(
        reinterpret_cast<int *>(rank_lds4), N, nq, nans, minf,
        [&](int q) { return IN_LDS ? lrow4[q] : make_float4(value_of(4 * q), value_of(4 * q + 1), value_of(4 * q + 2), value_of(4 * q + 3)); },
        value_of, posn, mates, moff[r] - mate_base, moff[r + 1] - mate_base, out_pos + (int64_t)e * plane_stride,
        out_flag + (int64_t)r * W + e);
}

// Q4.  grid: (R, W).  The band of acx_query_topk_lists: every row has its OWN candidate list, lists[r L .. r L + L) --
// tracks in any order, -1 = an empty slot, no track twice (checked by the host) --, and the slab is laid out by list
// POSITION: slab[(r L + j) W + e] = plane e of the pair {query r, lists[r L + j]}.  Candidate j is position j; empty slots
// and the row's own track take no part.  The select carries the POSITION where the other kernels carry the column (the
// key holds the track: rank_key64(value, track), the order of Q2), so that a listed track's score is read back at its
// position and nothing here is N wide.
// out_idx / out_score: R x W x k.  P = the power of two >= max(4, min(k, L)) (<= RANK_KMAX).
// Dynamic LDS: 12 P + RANK_SELECT_LDS_FIXED + 16 (the count of a row's valid entries) + IN_LDS ? 4 L : 0.
template <bool IN_LDS>
__global__ __launch_bounds__(RANK_THREADS) void query_topk_lists_kernel(const float *__restrict__ slab, int L, int W,
                                                                         const int32_t *__restrict__ self_of,
                                                                         const int32_t *__restrict__ lists,
                                                                         const double *__restrict__ col, int mode, int k, int P,
                                                                         int32_t *__restrict__ out_idx, float *__restrict__ out_score)
{
    extern __shared__ float4 rank_lds4[];
    int *cnt = reinterpret_cast<int *>(rank_select_row(rank_lds4, P));      // 16 bytes in front of the row: the valid entries
    float *lrow = reinterpret_cast<float *>(cnt + 4);
    const int r = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
    const float *row = slab + (int64_t)r * L * W + e;
    const int32_t *list = lists + (int64_t)r * L;
    const int self = self_of[r];
    // query_value's bits with ONE division for both col_modes (a single path through the re-finishing of a pass)
    auto value_at = [&](int j, int c) {
        const float s = row[(int64_t)j * W];
        if (mode == 0) return s;
        const double d = col[c];
        const float q = (float)((mode == 1 ? (double)s : d) / (mode == 1 ? d : (double)s));
        return mode == 1 ? q : -q;
    };
    if (tid == 0) *cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int j = tid; j < L; j += RANK_THREADS) {
        const int c = list[j];
        if (c < 0 || c == self) continue;
        ++mine;
        if (IN_LDS) lrow[j] = value_at(j, c);
    }
    mine = rank_wave_sum(mine);
    if ((tid & 63) == 0 && mine) atomicAdd(cnt, mine);
    __syncthreads();
    const int nvalid = *cnt;                              // candidates there are to list: counted, a list may hold any number
    rank_select_sort(rank_lds4, L, nvalid, k, P, [&](int j, int &pos, uint64_t &key) {
        const int c = list[j];
        if (c < 0 || c == self) return false;
        pos = j;
        key = rank_key64(IN_LDS ? lrow[j] : value_at(j, c), (uint32_t)c);    // (no track twice in a row: the keys are distinct)
        return true;
    });
    const int32_t *spos = rank_select_columns(rank_lds4, P);
    const int64_t o = ((int64_t)r * W + e) * k;
    for (int p = tid; p < k; p += RANK_THREADS) {
        const int j = p < P ? spos[p] : -1;
        const int c = j >= 0 ? list[j] : -1;
        out_idx[o + p] = c;
        out_score[o + p] = j >= 0 ? value_at(j, c) : __builtin_nanf("");
    }
}

}  // namespace acx
