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
//   Q2  query_topk_kernel   one workgroup per (row, plane): the first k candidates of the order of rank_kernels.hpp --
//                           larger value first (-0.0 and +0.0 tie), ties by ascending track index, NaN after every
//                           number -- by the same radix select over rank_key64(value, track) and the same bitonic sort
//                           as topk_rows_kernel, so the order is that kernel's by construction.  The candidates are a
//                           strictly ascending track list (or every track); the own track is skipped also when listed.
//                           Up to RANK_ROW_LDS candidates keep their finished values in LDS (the slab is read once);
//                           more are re-read -- and re-finished, the same operations on the same bits -- per pass.
//   Q3  query_rank_kernel   one workgroup per (row, plane): the 1-based positions of listed tracks (a query's clique
//                           mates) among the row's finished values, by the counting of rank_columns_kernel -- plain
//                           float comparisons, ties by posn --, eight mates per pass over the row.  The own column is
//                           stored as NaN (no comparison counts it); a NaN or a -inf anywhere else flags the (row, plane)
//                           and its positions are -1.  Up to RANK_ROW_LDS tracks keep their finished values in LDS; more
//                           are re-read -- and re-finished, the same operations on the same bits -- per pass.
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
// Dynamic LDS: 12 P bytes (keys, tracks) + QUERY_LDS_FIXED (histogram, scan, three counters) + IN_LDS ? 4 ncand : 0.
constexpr int QUERY_LDS_FIXED = 4 * (256 + 256 + 4);
template <bool IN_LDS>
__global__ __launch_bounds__(RANK_THREADS) void query_topk_kernel(const float *__restrict__ slab, int N, int W,
                                                                   const int32_t *__restrict__ self_of,
                                                                   const int32_t *__restrict__ cands, int ncand,
                                                                   const double *__restrict__ col, int mode, int k, int P,
                                                                   int32_t *__restrict__ out_idx, float *__restrict__ out_score)
{
    // (all LDS in the dynamic region: static variables in front of it would move its base off 16 bytes and the 64-bit
    //  key accesses off their natural alignment)
    extern __shared__ float4 rank_lds4[];
    uint64_t *skey = reinterpret_cast<uint64_t *>(rank_lds4);
    int32_t *scol = reinterpret_cast<int32_t *>(skey + P);
    int *hist = reinterpret_cast<int *>(scol + P), *scan = hist + 256;
    int &sel_digit = scan[256], &sel_below = scan[257], &n_taken = scan[258];
    float *lrow = reinterpret_cast<float *>(scan + 260);
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
    for (int s = tid; s < P; s += RANK_THREADS) { skey[s] = ~0ull; scol[s] = -1; }
    if (tid == 0) n_taken = 0;
    const int nvalid = ncand - (__syncthreads_or(mine_self) ? 1 : 0);       // candidates there are to list
    const int kk = min(k, nvalid);
    auto key_of = [&](int j, int c) { return rank_key64(IN_LDS ? lrow[j] : value_of(c), (uint32_t)c); };
    // the kk-th smallest key (1-based) among the candidates: most significant byte first
    uint64_t prefix = 0, mask = 0;
    if (kk > 0 && kk < nvalid) {
        int want = kk;
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int j = tid; j < ncand; j += RANK_THREADS) {
                const int c = track_of(j);
                if (c == self) continue;
                const uint64_t key = key_of(j, c);
                if ((key & mask) == prefix) atomicAdd(&hist[(int)((key >> shift) & 255)], 1);
            }
            __syncthreads();
            const int mine = hist[tid];
            int x = mine;                             // inclusive scan over the 256 bins
            for (int o = 1; o < 256; o <<= 1) {
                scan[tid] = x;
                __syncthreads();
                if (tid >= o) x += scan[tid - o];
                __syncthreads();
            }
            if (x - mine < want && want <= x) { sel_digit = tid; sel_below = x - mine; }
            __syncthreads();
            prefix |= (uint64_t)sel_digit << shift;
            mask |= (uint64_t)255 << shift;
            want -= sel_below;
            __syncthreads();
        }
    } else {
        prefix = ~0ull;                               // everything (kk == nvalid); kk == 0 takes nothing below
    }
    if (kk > 0) {
        for (int j = tid; j < ncand; j += RANK_THREADS) {
            const int c = track_of(j);
            if (c == self) continue;
            const uint64_t key = key_of(j, c);
            if (key <= prefix) {
                const int s = atomicAdd(&n_taken, 1);
                if (s < P) { skey[s] = key; scol[s] = c; }        // (the keys are distinct: exactly kk <= P are taken)
            }
        }
    }
    __syncthreads();
    // bitonic sort of the P slots, ascending by key (unused slots hold ~0: last)
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (P >> 1); t += RANK_THREADS) {
                const int lo = ((t / stride) * stride << 1) + (t % stride), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t a = skey[lo], b = skey[hi];
                if ((a > b) == up) {
                    skey[lo] = b; skey[hi] = a;
                    const int32_t ca = scol[lo]; scol[lo] = scol[hi]; scol[hi] = ca;
                }
            }
            __syncthreads();
        }
    }
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
// Dynamic LDS: QUERY_RANK_LDS_FIXED (the RANK_MB counters) + IN_LDS ? 16 * ((N + 3) / 4) : 0.
constexpr int QUERY_RANK_LDS_FIXED = 16 * ((4 * RANK_MB + 15) / 16);
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
    // (all LDS in the dynamic region, the counters in front: the row's quads stay on 16 bytes)
    extern __shared__ float4 rank_lds4[];
    int *acc = reinterpret_cast<int *>(rank_lds4);
    float4 *lrow4 = rank_lds4 + QUERY_RANK_LDS_FIXED / 16;
    float *lrow = reinterpret_cast<float *>(lrow4);
    const int r = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
    const float *row = slab + (int64_t)r * N * W + e;
    const int self = self_of[r];
    const int nq = (N + 3) >> 2;
    // the finished value of column c; the own column and the padding of the last quad are NaN, which no comparison counts
    auto value_of = [&](int c) { return (c < N && c != self) ? query_value(row[(int64_t)c * W], col, c, mode) : __builtin_nanf(""); };
    // pass 0: the finished row (into LDS).  A NaN anywhere else, or a -inf, flags the (row, plane): with the own column
    // and the padding as the only NaNs allowed, a clean row holds exactly 4 nq - N + 1 of them.
    int nans = 0, minf = 0;
    for (int c = tid; c < 4 * nq; c += RANK_THREADS) {
        const float v = value_of(c);
        if (IN_LDS) lrow[c] = v;
        nans += (v != v) ? 1 : 0;
        minf |= rank_bad(v) ? 1 : 0;
    }
    if (tid < RANK_MB) acc[tid] = 0;
    __syncthreads();
    nans = rank_wave_sum(nans);
    if ((tid & 63) == 0 && nans) atomicAdd(&acc[0], nans);
    const bool any_minf = __syncthreads_or(minf) != 0;
    const bool flagged = any_minf || acc[0] != 4 * nq - N + 1;
    __syncthreads();
    const int64_t m0 = moff[r] - mate_base, m1 = moff[r + 1] - mate_base;
    int32_t *pos = out_pos + (int64_t)e * plane_stride;
    if (tid == 0) out_flag[(int64_t)r * W + e] = flagged ? 1 : 0;
    if (flagged) {
        for (int64_t j = m0 + tid; j < m1; j += RANK_THREADS) pos[j] = -1;
        return;
    }
    for (int64_t b0 = m0; b0 < m1; b0 += RANK_MB) {
        float mv[RANK_MB];
        int mp[RANK_MB], cnt[RANK_MB];
#pragma unroll
        for (int j = 0; j < RANK_MB; ++j) {      // wave-uniform: the mates' values and tie ranks
            const bool on = b0 + j < m1;
            const int m = on ? mates[b0 + j] : 0;
            mv[j] = on ? value_of(m) : __builtin_nanf("");
            mp[j] = on ? (posn ? posn[m] : m) : 0;
            cnt[j] = 0;
        }
        if (tid < RANK_MB) acc[tid] = 0;
        for (int q = tid; q < nq; q += RANK_THREADS) {
            float v[4];
            if (IN_LDS) {
                const float4 v4 = lrow4[q];
                v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = value_of(4 * q + i);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bool have = false;
                int pc = 0;
#pragma unroll
                for (int j = 0; j < RANK_MB; ++j) {
                    if (v[i] > mv[j]) {
                        ++cnt[j];
                    } else if (v[i] == mv[j]) {       // a tie (the mate's own cell included): the tie order decides
                        if (!have) { const int c = 4 * q + i; pc = posn ? posn[c] : c; have = true; }
                        cnt[j] += pc < mp[j] ? 1 : 0;
                    }
                }
            }
        }
        __syncthreads();                              // acc zeroed
#pragma unroll
        for (int j = 0; j < RANK_MB; ++j) {
            const int s = rank_wave_sum(cnt[j]);
            if ((tid & 63) == 0 && s) atomicAdd(&acc[j], s);
        }
        __syncthreads();
        if (tid < RANK_MB && b0 + tid < m1) pos[b0 + tid] = 1 + acc[tid];
        __syncthreads();
    }
}

}  // namespace acx
