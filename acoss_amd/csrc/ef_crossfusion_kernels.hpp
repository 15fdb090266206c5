// The full cross-diffusion early fusion of one pair of tracks (Tralie, ISMIR 2017; the "Step 3" that
// earlyfusion_traile.py:142-148 disables): per feature the (M + N) x (M + N) affinity matrix
//     [ getW(S^A, k1)        getWCSM(C, k1, k2) ]
//     [ getWCSM(C, k1, k2)^T getW(S^B, k2)      ]          (similarity_fusion.py:38-99)
// the three of them cross-diffused by the kernels of snf_kernels.hpp, X = the two cross blocks of the result summed, the
// kappa N LARGEST cells of every row of X set in the bitmap that sw_bits_h16_kernel walks.
// The kernels here are the pieces around the SNF stages: the means of the smallest cells of the rows and the columns of a
// cross block, the cross block's affinity, widening and placement of the diagonal blocks, X, and the selection on f64.
// f64 throughout, like the reference; rows and columns of at most XF_MAXN cells (a line sits in one wave's registers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acx {

constexpr int XF_MAXN = 1024;     // cells per row / column: XF_PER_LANE values in each of 64 lanes
constexpr int XF_PER_LANE = 16;

__device__ __forceinline__ unsigned xf_key32(float v)
{
    const unsigned b = __float_as_uint(v);
    return (b >> 31) ? ~b : (b | 0x80000000u);               // monotone: smaller float -> smaller key
}
__device__ __forceinline__ float xf_unkey32(unsigned k)
{
    return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}
// -0.0 ranks WITH +0.0 (numpy's comparisons, which the stable argsort of the specification uses, do not tell them apart)
__device__ __forceinline__ unsigned long long xf_key64(double v)
{
    if (v == 0.0) v = 0.0;
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// The k-th smallest (0-based, k < count) of the keys a wave holds, XF_PER_LANE per lane (slot t of lane l is valid when
// valid(t)): built from the top bit down, one ballot count per bit and slot -- the largest T with |{key < T}| <= k.
template <typename KeyT, int BITS, typename Valid>
__device__ __forceinline__ KeyT xf_kth_smallest(const KeyT (&key)[XF_PER_LANE], int nslots, Valid valid, int k)
{
    KeyT T = 0;
    for (int bit = BITS - 1; bit >= 0; --bit) {
        const KeyT cand = T | ((KeyT)1 << bit);
        int below = 0;
#pragma unroll
        for (int t = 0; t < XF_PER_LANE; ++t)
            if (t < nslots) below += __popcll(__ballot(valid(t) && key[t] < cand));
        if (below <= k) T = cand;
    }
    return T;
}

// r[i] = mean of the k_row smallest cells of row i, c[j] = mean of the k_col smallest cells of column j of the f32 matrix
// C (M rows of pitch ld, N columns), as f64 (getWCSM, similarity_fusion.py:47-51: np.partition and np.mean).  One wave per
// line, rows first; a column is read with stride ld straight from C (no transposed copy) into the same registers.  The
// cells below the k-th smallest value are added in f64 (exactly widened), the ties at the cut contribute their common value.
// Needs 1 <= k_row <= N <= XF_MAXN and 1 <= k_col <= M <= XF_MAXN (host).
__global__ __launch_bounds__(256) void xf_means_kernel(const float *__restrict__ C, int M, int N, int64_t ld, int k_row, int k_col,
                                                       double *__restrict__ r, double *__restrict__ c)
{
    const int line = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (line >= M + N) return;                                // (wave-uniform)
    const bool is_row = line < M;
    const int len = is_row ? N : M, k = is_row ? k_row : k_col;
    const float *src = is_row ? C + (int64_t)line * ld : C + (line - M);
    const int64_t stride = is_row ? 1 : ld;
    const int nslots = (len + 63) >> 6;
    unsigned key[XF_PER_LANE];
#pragma unroll
    for (int t = 0; t < XF_PER_LANE; ++t) {
        const int e = t * 64 + lane;
        key[t] = (t < nslots && e < len) ? xf_key32(src[(int64_t)e * stride]) : 0xffffffffu;
    }
    auto valid = [&](int t) { return t * 64 + lane < len; };
    const unsigned tk = xf_kth_smallest<unsigned, 32>(key, nslots, valid, k - 1);
    const double tv = (double)xf_unkey32(tk);
    double s = 0.0;
    int below = 0;
#pragma unroll
    for (int t = 0; t < XF_PER_LANE; ++t)
        if (t < nslots && valid(t) && key[t] < tk) { s += (double)xf_unkey32(key[t]); ++below; }
    for (int off = 32; off >= 1; off >>= 1) { s += __shfl_xor(s, off, 64); below += __shfl_xor(below, off, 64); }
    if (lane == 0) {
        const double m = (s + (double)(k - below) * tv) / (double)k;
        if (is_row) r[line] = m; else c[line - M] = m;
    }
}

// The cross block of W (getWCSM, similarity_fusion.py:52-54): Eps = (r_i + c_j + C) / 3, W = exp(-C^2 / (2 (mu Eps)^2)), in
// numpy's operation order (no guard on the denominator: 0 / 0 is NaN there too).  Written to W[i][M + j] and, turned through
// an LDS tile so that both stores are coalesced, to W[M + j][i] (setupWCSMSSM, :70-73); W is (M + N) x (M + N).
__global__ __launch_bounds__(256) void xf_cross_affinity_kernel(const float *__restrict__ C, int M, int N, int64_t ld,
                                                                const double *__restrict__ r, const double *__restrict__ c,
                                                                double mu, double *__restrict__ W)
{
    __shared__ double tile[32][33];
    const int n = M + N;
    const int j0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
    for (int rr = ty; rr < 32; rr += 8) {
        const int i = i0 + rr, j = j0 + tx;
        double w = 0.0;
        if (i < M && j < N) {
            const double d = (double)C[(int64_t)i * ld + j];
            double eps = r[i] + c[j] + d;
            eps = eps / 3.0;
            const double me = mu * eps;
            w = exp(-(d * d) / (2.0 * (me * me)));
            W[(size_t)i * n + M + j] = w;
        }
        tile[rr][tx] = w;
    }
    __syncthreads();
    for (int rr = ty; rr < 32; rr += 8) {
        const int j = j0 + rr, i = i0 + tx;
        if (i < M && j < N) W[(size_t)(M + j) * n + i] = tile[tx][rr];
    }
}

// dst (m x m, dense, f64) = src (m rows of pitch ld, f32), widened exactly: the input of snf_sym_kernel for a diagonal block
__global__ __launch_bounds__(256) void xf_widen_kernel(const float *__restrict__ src, int64_t ld, int m, double *__restrict__ dst)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)m * m) return;
    const int i = (int)(e / m), j = (int)(e - (int64_t)i * m);
    dst[e] = (double)src[(int64_t)i * ld + j];
}

// W[at + i][at + j] = src[i][j] (src m x m dense; W n x n): a diagonal block takes its place (setupWCSMSSM, :70, :73)
__global__ __launch_bounds__(256) void xf_place_kernel(const double *__restrict__ src, int m, double *__restrict__ W, int n, int at)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)m * m) return;
    const int i = (int)(e / m), j = (int)(e - (int64_t)i * m);
    W[(size_t)(at + i) * n + at + j] = src[e];
}

// X[i][j] = D[i][M + j] + D[M + j][i]: the fused matrix is not symmetric, both cross blocks count.  The lower block is read
// row by row (coalesced) into an LDS tile and taken from there transposed.  X is M x N dense.
__global__ __launch_bounds__(256) void xf_x_kernel(const double *__restrict__ D, int M, int N, double *__restrict__ X)
{
    __shared__ double tile[32][33];
    const int n = M + N;
    const int j0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int rr = ty; rr < 32; rr += 8) {
        const int j = j0 + rr, i = i0 + tx;
        tile[rr][tx] = (i < M && j < N) ? D[(size_t)(M + j) * n + i] : 0.0;
    }
    __syncthreads();
    for (int rr = ty; rr < 32; rr += 8) {
        const int i = i0 + rr, j = j0 + tx;
        if (i < M && j < N) X[(size_t)i * N + j] = D[(size_t)i * n + M + j] + tile[tx][rr];
    }
}

// csm_to_binary(exp(-X), kappa) without the exponential: row i of the bitmap holds the k columns with the LARGEST X[i][:], ties
// at the cut in ascending column order (the first k of a stable descending argsort).  One wave per row, N <= XF_MAXN, the
// 64-bit keys 16 per lane (column 64 t + lane in slot t).  bits: M rows of pitch / 32 words, pitch = N rounded up to 64, bit
// j % 32 of word j / 32 (the layout sw_bits_h16_kernel and ef_align_kernel read); every word of a row is written, pad bits zero.
__global__ __launch_bounds__(256) void xf_select_kernel(const double *__restrict__ X, int M, int N, int k, unsigned *__restrict__ bits)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= M) return;                                       // (wave-uniform)
    const double *row = X + (size_t)i * N;
    const int nslots = (N + 63) >> 6;
    unsigned long long key[XF_PER_LANE];
#pragma unroll
    for (int t = 0; t < XF_PER_LANE; ++t) {
        const int j = t * 64 + lane;
        key[t] = (t < nslots && j < N) ? xf_key64(row[j]) : 0ull;
    }
    auto valid = [&](int t) { return t * 64 + lane < N; };
    unsigned *out = bits + (size_t)i * (2 * nslots);
    const bool none = k <= 0, all = k >= N;
    unsigned long long tk = 0ull;
    int neq_left = 0;
    if (!none && !all) {
        tk = xf_kth_smallest<unsigned long long, 64>(key, nslots, valid, N - k);       // the k-th largest
        int ngt = 0;
#pragma unroll
        for (int t = 0; t < XF_PER_LANE; ++t)
            if (t < nslots) ngt += __popcll(__ballot(valid(t) && key[t] > tk));
        neq_left = k - ngt;
    }
#pragma unroll
    for (int t = 0; t < XF_PER_LANE; ++t) {
        if (t >= nslots) continue;                            // (wave-uniform)
        unsigned long long m;
        if (none) m = 0ull;
        else if (all) m = __ballot(valid(t));
        else {
            const bool ok = valid(t);
            const unsigned long long meq = __ballot(ok && key[t] == tk);
            const int eq_rank = __popcll(meq & ((1ull << lane) - 1ull));
            m = __ballot(ok && (key[t] > tk || (key[t] == tk && eq_rank < neq_left)));
            const int neq = __popcll(meq);
            neq_left -= neq < neq_left ? neq : neq_left;
        }
        if (lane < 2) out[2 * t + lane] = (unsigned)(m >> (32 * lane));
    }
}

}  // namespace acx
