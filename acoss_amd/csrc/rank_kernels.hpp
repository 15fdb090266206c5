// Ranking of finished score rows (the reference's getEvalStatistics, algorithm_template.py:205-290, and candidate lists).
//
// ONE order, defined in this file and nowhere else: column a comes before column b iff
//     s[a] > s[b],  or  s[a] == s[b] and posn[a] < posn[b]            (IEEE comparison: -0.0 and +0.0 tie)
// with posn[c] = c when no tie order is given.  Two device functions decide it; every kernel that ranks calls them:
//   rank_count_positions   the 1-based position of every listed column (a row's clique mates) in that order:
//                          1 + #{c != self: s[c] > s[m]} + #{c != self: s[c] == s[m], posn[c] < posn[m]}, by counting --
//                          plain float comparisons, no key --, RANK_MB mates per pass over the row.  A row with a NaN or a
//                          -inf outside its own cell is flagged and gets -1: the host decides what such a row means.
//   rank_select_sort       the first k columns of the order.  NaN is defined here as np.argsort(-row, kind="stable")
//                          defines it: after every number, among themselves by posn.  The k-th key by a radix select
//                          (8 passes of 8 bits) over the 64-bit composite key rank_key64 (descending score key << 32 |
//                          posn), which has no ties; compaction; bitonic sort in LDS.
// The kernels add where a row comes from and where its result goes: their row load, their functors, their stores.
//   R1  rank_columns_kernel   positions in a row slab            (query_kernels.hpp Q3: in a query band's finished values)
//   R2  topk_rows_kernel      first k of a row slab, with scores (query_kernels.hpp Q2: of a band's candidates)
// A row slab is n_rows rows of n f32 scores with leading dimension ld; row r is the score row of track self[r], whose own
// cell takes no part.  Every row starts on 16 bytes (a 16-byte aligned slab and ld % 4 == 0: the host stages rows that
// way, rank_for_pieces), so a quad is columns 4 q .. 4 q + 3 and whole quads are one 16-byte load.
// One workgroup of 256 threads per row.  A row of up to RANK_ROW_LDS cells is read ONCE from global memory into LDS (own
// cell and padding as NaN, which no comparison counts); a longer row is re-read per pass (L2).  All LDS is dynamic: static
// variables in front of it would move its base off 16 bytes.  Every store is a plain C++ store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acx {

constexpr int RANK_THREADS = 256;
constexpr int RANK_ROW_LDS = 16384;      // cells of a row kept in LDS (64 KB: two workgroups per CU)
constexpr int RANK_MB = 8;               // mates counted per pass over the row
constexpr int RANK_KMAX = 1024;          // largest k of topk_rows_kernel (the reference's largest Top-k is 1000)

__device__ __forceinline__ int rank_wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Quad q of row `row` (n cells, own cell `self`, 16-byte aligned): columns 4 q .. 4 q + 3, a whole quad as one 16-byte
// load.  Cells from n on and the own cell come back NaN.
__device__ __forceinline__ float4 rank_quad_global(const float *__restrict__ row, int n, int self, int q)
{
    const int c0 = 4 * q;
    float4 v;
    if (c0 + 3 < n) {
        v = *reinterpret_cast<const float4 *>(row + c0);
    } else {
        v.x = c0 < n ? row[c0] : __builtin_nanf("");
        v.y = c0 + 1 < n ? row[c0 + 1] : __builtin_nanf("");
        v.z = c0 + 2 < n ? row[c0 + 2] : __builtin_nanf("");
        v.w = __builtin_nanf("");
    }
    const int d = self - c0;
    if (d == 0) v.x = __builtin_nanf("");
    if (d == 1) v.y = __builtin_nanf("");
    if (d == 2) v.z = __builtin_nanf("");
    if (d == 3) v.w = __builtin_nanf("");
    return v;
}

__device__ __forceinline__ bool rank_bad(float v) { return v == -__builtin_inff(); }      // (NaNs are counted)

// Positions by counting.  The row is nq quads of finished values, quad(q) = columns 4 q .. 4 q + 3, with the own cell and
// the columns from n on as NaN; mate(m) = the finished value of column m.  `nans` / `minf`: what this thread saw of its
// share of the row while it loaded it -- how many NaNs, whether a -inf.  A NaN anywhere but in the own cell and the
// padding, or a -inf, flags the row: a clean row holds exactly 4 nq - n + 1 NaNs.
// acc: RANK_MB counters in LDS (RANK_COUNT_LDS_FIXED bytes).  mates[m0 .. m1): the listed columns (none is the own one).
// out_pos[j]: the position of mates[j], or -1 in a flagged row; *out_flag in {0, 1}.
constexpr int RANK_COUNT_LDS_FIXED = 16 * ((4 * RANK_MB + 15) / 16);
template <typename Quad, typename Mate>
__device__ __forceinline__ void rank_count_positions(int *acc, int n, int nq, int nans, int minf, Quad quad, Mate mate,
                                                     const int32_t *__restrict__ posn, const int32_t *__restrict__ mates,
                                                     int64_t m0, int64_t m1, int32_t *__restrict__ out_pos,
                                                     uint8_t *__restrict__ out_flag)
{
    const int tid = threadIdx.x;
    if (tid < RANK_MB) acc[tid] = 0;
    __syncthreads();
    nans = rank_wave_sum(nans);
    if ((tid & 63) == 0 && nans) atomicAdd(&acc[0], nans);
    const bool any_minf = __syncthreads_or(minf) != 0;
    const bool flagged = any_minf || acc[0] != 4 * nq - n + 1;
    __syncthreads();
    if (tid == 0) *out_flag = flagged ? 1 : 0;
    if (flagged) {
        for (int64_t j = m0 + tid; j < m1; j += RANK_THREADS) out_pos[j] = -1;
        return;
    }
    for (int64_t b0 = m0; b0 < m1; b0 += RANK_MB) {
        float mv[RANK_MB];
        int mp[RANK_MB], cnt[RANK_MB];
#pragma unroll
        for (int j = 0; j < RANK_MB; ++j) {      // wave-uniform: the mates' values and tie ranks
            const bool on = b0 + j < m1;
            const int m = on ? mates[b0 + j] : 0;
            mv[j] = on ? mate(m) : __builtin_nanf("");
            mp[j] = on ? (posn ? posn[m] : m) : 0;
            cnt[j] = 0;
        }
        if (tid < RANK_MB) acc[tid] = 0;
        for (int q = tid; q < nq; q += RANK_THREADS) {
            const float4 v4 = quad(q);
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bool have = false;
                int pc = 0;
#pragma unroll
                for (int j = 0; j < RANK_MB; ++j) {
                    if (v[e] > mv[j]) {
                        ++cnt[j];
                    } else if (v[e] == mv[j]) {       // a tie (the mate's own cell included): the tie order decides
                        if (!have) { const int c = 4 * q + e; pc = posn ? posn[c] : c; have = true; }
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
        if (tid < RANK_MB && b0 + tid < m1) out_pos[b0 + tid] = 1 + acc[tid];
        __syncthreads();
    }
}

// R1.  slab: n_rows x ld; mates[moff[r] .. moff[r + 1]) the listed columns of row r (none is self[r]: checked by the host).
// out_pos[moff[r] + j]: position of the j-th listed column, or -1 in a flagged row; out_flag[r] in {0, 1}.
// Dynamic LDS: RANK_COUNT_LDS_FIXED + IN_LDS ? 16 * ((n + 3) / 4) : 0 (the counters in front: the quads stay on 16 bytes).
template <bool IN_LDS>
__global__ __launch_bounds__(RANK_THREADS) void rank_columns_kernel(const float *__restrict__ slab, int64_t ld, int n,
                                                                     const int32_t *__restrict__ self_of,
                                                                     const int32_t *__restrict__ posn,
                                                                     const int64_t *__restrict__ moff,
                                                                     const int32_t *__restrict__ mates, int64_t mate_base,
                                                                     int32_t *__restrict__ out_pos,
                                                                     uint8_t *__restrict__ out_flag)
{
    extern __shared__ float4 rank_lds4[];
    float4 *lrow4 = rank_lds4 + RANK_COUNT_LDS_FIXED / 16;
    const int r = blockIdx.x, tid = threadIdx.x;
    const float *row = slab + (int64_t)r * ld;
    const int self = self_of[r];
    const int nq = (n + 3) >> 2;
    int nans = 0, minf = 0;
    for (int q = tid; q < nq; q += RANK_THREADS) {
        const float4 v = rank_quad_global(row, n, self, q);
        if (IN_LDS) lrow4[q] = v;
        nans += (v.x != v.x) + (v.y != v.y) + (v.z != v.z) + (v.w != v.w);
        minf |= (rank_bad(v.x) || rank_bad(v.y) || rank_bad(v.z) || rank_bad(v.w)) ? 1 : 0;
    }
    rank_count_positions(
        reinterpret_cast<int *>(rank_lds4), n, nq, nans, minf,
        [&](int q) { return IN_LDS ? lrow4[q] : rank_quad_global(row, n, self, q); }, [&](int m) { return row[m]; }, posn, mates,
        moff[r] - mate_base, moff[r + 1] - mate_base, out_pos, out_flag + r);
}

// The composite key of a cell: smaller = earlier in the order.  High word: the descending score key (-0.0 canonicalised
// to +0.0 first, so that the zeros tie; every NaN 0xffffffff, behind -inf's 0xff800000); low word: the tie rank.
__device__ __forceinline__ uint64_t rank_key64(float v, uint32_t p)
{
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0;
    const uint32_t asc = (u >> 31) ? ~u : (u | 0x80000000u);
    const uint32_t desc = (v != v) ? 0xffffffffu : ~asc;
    return ((uint64_t)desc << 32) | p;
}

// LDS of rank_select_sort: P keys | P columns | RANK_SELECT_LDS_FIXED (histogram, scan, three counters) | the caller's
// row.  P = the power of two >= max(4, min(k, nvalid)) (<= RANK_KMAX): slots of the sort.
constexpr int RANK_SELECT_LDS_FIXED = 4 * (256 + 256 + 4);
__device__ __forceinline__ int32_t *rank_select_columns(float4 *lds, int P) { return reinterpret_cast<int32_t *>(reinterpret_cast<uint64_t *>(lds) + P); }
__device__ __forceinline__ float *rank_select_row(float4 *lds, int P) { return reinterpret_cast<float *>(rank_select_columns(lds, P) + P + RANK_SELECT_LDS_FIXED / 4); }

// The first min(k, nvalid) columns of the order among candidates 0 .. ncand - 1, of which nvalid are not the row's own:
// cell(j, c, key) gives candidate j's column and rank_key64, or returns false when j is the row's own track.  On return
// rank_select_columns(lds, P)[0 .. P) holds them in order, -1 behind the last.  What the caller wrote to its row in LDS
// needs no barrier of its own: cell is first called behind the one that follows the initialisation of the slots.
template <typename Cell>
__device__ __forceinline__ void rank_select_sort(float4 *lds, int ncand, int nvalid, int k, int P, Cell cell)
{
    uint64_t *skey = reinterpret_cast<uint64_t *>(lds);
    int32_t *scol = rank_select_columns(lds, P);
    int *hist = scol + P, *scan = hist + 256;
    int &sel_digit = scan[256], &sel_below = scan[257], &n_taken = scan[258];
    const int tid = threadIdx.x;
    const int kk = min(k, nvalid);                    // columns there are to list
    for (int s = tid; s < P; s += RANK_THREADS) { skey[s] = ~0ull; scol[s] = -1; }
    if (tid == 0) n_taken = 0;
    __syncthreads();
    // the kk-th smallest key (1-based) among the candidates: most significant byte first
    uint64_t prefix = 0, mask = 0;
    if (kk > 0 && kk < nvalid) {
        int want = kk;
        for (int shift = 56; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int j = tid; j < ncand; j += RANK_THREADS) {
                int c;
                uint64_t key;
                if (!cell(j, c, key)) continue;
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
            int c;
            uint64_t key;
            if (!cell(j, c, key)) continue;
            if (key <= prefix) {
                const int s = atomicAdd(&n_taken, 1);
                if (s < P) { skey[s] = key; scol[s] = c; }        // (s >= P only with a tie order that repeats values)
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
}

// R2.  out_idx / out_score: n_rows x k (the scores are bit copies); candidate j is column j, P as above with nvalid = n - 1.
// Dynamic LDS: 12 P + RANK_SELECT_LDS_FIXED + IN_LDS ? 16 * ((n + 3) / 4) : 0.
template <bool IN_LDS>
__global__ __launch_bounds__(RANK_THREADS) void topk_rows_kernel(const float *__restrict__ slab, int64_t ld, int n,
                                                                  const int32_t *__restrict__ self_of,
                                                                  const int32_t *__restrict__ posn, int k, int P,
                                                                  int32_t *__restrict__ out_idx, float *__restrict__ out_score)
{
    extern __shared__ float4 rank_lds4[];
    float *lrow = rank_select_row(rank_lds4, P);
    const int r = blockIdx.x, tid = threadIdx.x;
    const float *row = slab + (int64_t)r * ld;
    const int self = self_of[r];
    if (IN_LDS) {
        // 16-byte loads and stores where the quad is whole
        for (int q = tid; q < ((n + 3) >> 2); q += RANK_THREADS) {
            const int c0 = 4 * q;
            if (c0 + 3 < n) {
                reinterpret_cast<float4 *>(lrow)[q] = *reinterpret_cast<const float4 *>(row + c0);
            } else {
                for (int e = 0; c0 + e < n; ++e) lrow[c0 + e] = row[c0 + e];
            }
        }
    }
    const float *src = IN_LDS ? lrow : row;
    rank_select_sort(rank_lds4, n, n - 1, k, P, [&](int j, int &c, uint64_t &key) {
        if (j == self) return false;
        c = j;
        key = rank_key64(src[j], (uint32_t)(posn ? posn[j] : j));
        return true;
    });
    const int32_t *scol = rank_select_columns(rank_lds4, P);
    for (int p = tid; p < k; p += RANK_THREADS) {
        const int c = p < P ? scol[p] : -1;
        out_idx[(int64_t)r * k + p] = c;
        out_score[(int64_t)r * k + p] = c >= 0 ? row[c] : __builtin_nanf("");
    }
}

}  // namespace acx
