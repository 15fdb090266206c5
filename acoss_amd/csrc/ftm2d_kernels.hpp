// FTM2D (Bertin-Mahieux & Ellis 2012: 2D Fourier transform magnitudes of beat-synchronous chroma), reference
// acoss/algorithms/ftm2d.py.  Per track (load_features, :52-64):
//   F1  beat sync   librosa.util.sync(X.T, onsets, aggregate=np.median): f32 median of every bin over every segment
//                   [b_k, b_k+1) of unique(clip(onsets, 0, T) + {0, T}) -- bit-identical to np.median on f32
//   F2  chrompwr    (:100-117) per beat, f64
//       + the 12-point DFT along chroma of every beat (real input: bins 0..6)
//   F3  windows     (:120-139) |fft2| of every WIN-beat window as the WIN-point DFT along time of those 7 rows (rows
//                   7..11 by conjugate symmetry), in fftshift order; / window L2 norm, log(C x + 1) (:59-61)
//   F4  median      per dimension over the windows, exact f64 np.median (:62)
//   F5  normalise   / L2 norm of the median (:63; an all-zero median gives NaN like the reference)
// Per pair (similarity, :85-97): exp(-sum((s1 - s2)^2)) in f64, rounded to f32 -- ftm2d_tile_kernel for the pair grid,
// ftm2d_pairs_kernel for pair lists, both summing d^2 over k = 0 .. D-1 in order in ONE accumulator (same bits).
// Every store is a plain C++ store.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "prep_kernels.hpp"     // track_of

namespace acx {

constexpr int FTM_MAXWIN = 256;       // WIN supported on the device
constexpr int FTM_NW = 8;             // windows per workgroup of ftm2d_window_kernel (at most; the host picks what fits LDS)
constexpr int FTM_LDS = 64 * 1024;    // dynamic LDS of ftm2d_window_kernel
constexpr int FTM_SEG_REG = 4;        // F1: segments of up to 4 x 64 frames are selected in registers
constexpr int FTM_TM = 64;            // pair tile: 64 x 64 pairs per workgroup, 4 x 4 per thread
constexpr int FTM_KS = 16;            // dims per LDS slab of the pair tile

// ---- order-preserving keys: a < b (floats, no NaN) <=> key(a) < key(b) as unsigned integers --------------------------
__device__ __forceinline__ uint32_t ftm_key32(float v)
{
    const uint32_t u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ftm_unkey32(uint32_t k)
{
    return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ uint64_t ftm_key64(double v)
{
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ftm_unkey64(uint64_t k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ int ftm_wave_sum(int v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint64_t ftm_wave_min(uint64_t v)
{
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}

// The k1-th and k2-th (k2 = k1 or k1 + 1) smallest of n keys, a WAVE-level selection on the bit patterns: the largest
// key K with #(keys < K) <= k is built bit by bit from the top (one counting pass per bit), then the next order
// statistic is the same key (if it repeats) or the smallest key above it.  KEY(i) yields key i < n (any lane).
// Exact for any n; no sort, no LDS.  REG = keys held in registers (n <= 64 REG), else re-read through KEY each pass.
template <typename U, int E, typename KeyFn>
__device__ void ftm_wave_select(KeyFn key, int n, int k1, int k2, bool in_regs, U &v1, U &v2)
{
    const int lane = threadIdx.x & 63;
    constexpr int BITS = 8 * (int)sizeof(U);
    U reg[E];
    if (in_regs) {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = lane + 64 * e;
            reg[e] = i < n ? key(i) : (U)~(U)0;       // padding: the largest key, never counted below a candidate
        }
    }
    auto count_lt = [&](U cand) -> int {
        int cnt = 0;
        if (in_regs) {
#pragma unroll
            for (int e = 0; e < E; ++e) cnt += (lane + 64 * e < n && reg[e] < cand) ? 1 : 0;
        } else {
            for (int i = lane; i < n; i += 64) cnt += key(i) < cand ? 1 : 0;
        }
        return ftm_wave_sum(cnt);
    };
    U prefix = 0;
    for (int b = BITS - 1; b >= 0; --b) {
        const U cand = prefix | ((U)1 << b);
        if (count_lt(cand) <= k1) prefix = cand;
    }
    v1 = prefix;
    if (k2 == k1) { v2 = v1; return; }
    // #(keys <= v1) > k2: v1 again; else the smallest key above v1
    int le = 0;
    uint64_t mn = ~0ull;
    if (in_regs) {
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (lane + 64 * e < n) {
                le += reg[e] <= v1 ? 1 : 0;
                if (reg[e] > v1 && (uint64_t)reg[e] < mn) mn = reg[e];
            }
    } else {
        for (int i = lane; i < n; i += 64) {
            const U x = key(i);
            le += x <= v1 ? 1 : 0;
            if (x > v1 && (uint64_t)x < mn) mn = x;
        }
    }
    le = ftm_wave_sum(le);
    mn = ftm_wave_min(mn);
    v2 = le > k2 ? v1 : (U)mn;
}

// ------------------------------------------------------------------------------------
// F1: beat-synchronous medians.  One wave per beat (segment); the 12 bins one after the other.  ch holds the batch's
// raw chroma (rows, 12) f32; bnd the segment boundaries as batch rows: beat j of track t (boff[t] <= j < boff[t + 1])
// spans rows bnd[j + t] .. bnd[j + t + 1].  sync (beats, 12) f32: np.median -- the middle value, or the f32 mean of
// the two middle values for an even count.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ftm2d_sync_kernel(const float *__restrict__ ch, const int64_t *__restrict__ bnd,
                                                         const int64_t *__restrict__ boff, int n_tracks, int64_t n_beats,
                                                         float *__restrict__ sync)
{
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n_beats) return;
    const int t = track_of(boff, n_tracks, j);
    const int64_t r0 = bnd[j + t];
    const int n = (int)(bnd[j + t + 1] - r0);
    const float *x = ch + r0 * 12;
    const int k1 = (n - 1) >> 1, k2 = n >> 1;
    const bool in_regs = n <= 64 * FTM_SEG_REG;
    for (int b = 0; b < 12; ++b) {
        uint32_t a, c;
        ftm_wave_select<uint32_t, FTM_SEG_REG>([&](int i) { return ftm_key32(x[(int64_t)i * 12 + b]); }, n, k1, k2, in_regs, a, c);
        if ((threadIdx.x & 63) == 0) {
            const float lo = ftm_unkey32(a), hi = ftm_unkey32(c);
            sync[j * 12 + b] = (k1 == k2) ? lo : (lo + hi) / 2.0f;
        }
    }
}

// ------------------------------------------------------------------------------------
// F2: per beat (one thread): chrompwr in f64 -- norm (0 -> 1), (x / norm)^P, renormalise (0 -> 1), scale back
// (ftm2d.py:100-117) -- and the 12-point DFT along chroma: G[j][k1] = sum_c y_c exp(-2 pi i k1 c / 12), k1 = 0..6
// (tw12[m] = exp(-2 pi i m / 12) from the host).  pwr (beats, 12) f64, G (beats, 7) complex as (re, im) pairs.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ftm2d_beat_kernel(const float *__restrict__ sync, int64_t n_beats, double P,
                                                         const double *__restrict__ tw12, double *__restrict__ pwr,
                                                         double *__restrict__ G)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n_beats) return;
    double x[12], s = 0.0;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        x[c] = (double)sync[j * 12 + c];
        s = s + x[c] * x[c];
    }
    double cmn = __builtin_sqrt(s);
    if (cmn == 0.0) cmn = 1.0;
    double sp = 0.0;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        x[c] = pow(x[c] / cmn, P);
        sp = sp + x[c] * x[c];
    }
    double cmpn = __builtin_sqrt(sp);
    if (cmpn == 0.0) cmpn = 1.0;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
        x[c] = cmn * (x[c] / cmpn);
        pwr[j * 12 + c] = x[c];
    }
#pragma unroll
    for (int k = 0; k <= 6; ++k) {
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int c = 0; c < 12; ++c) {
            const int m = (k * c) % 12;
            re = __builtin_fma(x[c], tw12[2 * m], re);
            im = __builtin_fma(x[c], tw12[2 * m + 1], im);
        }
        G[(j * 7 + k) * 2] = re;
        G[(j * 7 + k) * 2 + 1] = im;
    }
}

// ------------------------------------------------------------------------------------
// F3: a block of nw consecutive windows of one track per workgroup.  LDS: the 7 DFT rows of the beats the block
// covers, the WIN twiddles exp(-2 pi i m / WIN) (host f64 table), the 7 x WIN magnitudes of every window, the window
// norms.  Thread per (k1, k2), k1 <= 6: F[k1, k2] = sum_t G[k1][w + t] tw[(k2 t) mod WIN] for the nw windows at once.
// Then norm^2 = sum over all 12 rows (rows 1..5 stand for 11..7 too: |F[12 - k1, -k2]| = |F[k1, k2]| for real input),
// and out[d] in fftshift order (row r = F row (r + 6) mod 12, column s = F column (s - WIN/2) mod WIN) as
// log(C x / norm + 1) (norm 0 -> 1).  logwin: track t's (D, nwin_t) matrix DIMENSION-major at woff[t] * D.
// blk[b] = {track, first window}.
// ------------------------------------------------------------------------------------
struct FtmBlock { int32_t track, w0; };

__global__ __launch_bounds__(256) void ftm2d_window_kernel(const double *__restrict__ G, const int64_t *__restrict__ boff,
                                                           const int64_t *__restrict__ woff, const FtmBlock *__restrict__ blk,
                                                           const double *__restrict__ twW, int win, int nw, double C,
                                                           double *__restrict__ logwin)
{
    extern __shared__ double ftm_lds[];
    const FtmBlock bk = blk[blockIdx.x];
    const int t = bk.track, w0 = bk.w0;
    const int nwin = (int)(woff[t + 1] - woff[t]);
    const int nwb = nwin - w0 < nw ? nwin - w0 : nw;          // windows of this block
    const int span = nw + win - 1;                              // beats staged per row
    const int nbt = nwb + win - 1;                              // beats of the block that exist
    double *g = ftm_lds;                                        // [7][span] complex
    double *tw = g + 2 * 7 * span;                              // [win] complex
    double *mag = tw + 2 * win;                                 // [nw][7 * win]
    double *nrm = mag + (size_t)nw * 7 * win;                   // [nw]
    const int tid = threadIdx.x;
    const double *Gt = G + (boff[t] + w0) * 14;
    for (int e = tid; e < 7 * span; e += 256) {
        const int k = e / span, u = e - k * span;
        const bool ok = u < nbt;
        g[2 * e] = ok ? Gt[u * 14 + 2 * k] : 0.0;
        g[2 * e + 1] = ok ? Gt[u * 14 + 2 * k + 1] : 0.0;
    }
    for (int e = tid; e < 2 * win; e += 256) tw[e] = twW[e];
    __syncthreads();
    for (int o = tid; o < 7 * win; o += 256) {
        const int k1 = o / win, k2 = o - k1 * win;
        const double *gk = g + 2 * k1 * span;
        double re[FTM_NW], im[FTM_NW];
#pragma unroll
        for (int r = 0; r < FTM_NW; ++r) { re[r] = 0.0; im[r] = 0.0; }
        int m = 0;
        for (int u = 0; u < win; ++u) {
            const double wr = tw[2 * m], wi = tw[2 * m + 1];
#pragma unroll
            for (int r = 0; r < FTM_NW; ++r) {
                if (r < nw) {
                    const double gr = gk[2 * (r + u)], gi = gk[2 * (r + u) + 1];
                    re[r] = __builtin_fma(gr, wr, re[r]);
                    re[r] = __builtin_fma(-gi, wi, re[r]);
                    im[r] = __builtin_fma(gr, wi, im[r]);
                    im[r] = __builtin_fma(gi, wr, im[r]);
                }
            }
            m += k2;
            if (m >= win) m -= win;
        }
#pragma unroll
        for (int r = 0; r < FTM_NW; ++r)
            if (r < nw) mag[(size_t)r * 7 * win + o] = __builtin_sqrt(re[r] * re[r] + im[r] * im[r]);
    }
    __syncthreads();
    // window norms: one wave per window, fixed-order lane sums + shuffle tree (reproducible)
    const int wave = tid >> 6, lane = tid & 63;
    for (int r = wave; r < nwb; r += 4) {
        const double *mr = mag + (size_t)r * 7 * win;
        double s = 0.0;
        for (int o = lane; o < 7 * win; o += 64) {
            const int k1 = o / win;
            const double v = mr[o] * mr[o];
            s = s + ((k1 == 0 || k1 == 6) ? v : 2.0 * v);
        }
        for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64);
        if (lane == 0) {
            const double q = __builtin_sqrt(s);
            nrm[r] = q == 0.0 ? 1.0 : q;
        }
    }
    __syncthreads();
    const int D = 12 * win, half = win / 2;
    double *out = logwin + woff[t] * D;
    for (int e = tid; e < nw * D; e += 256) {
        const int d = e / nw, r = e - d * nw;
        if (r >= nwb) continue;
        const int row = d / win, col = d - row * win;
        int k1 = row + 6;
        if (k1 >= 12) k1 -= 12;
        int k2 = col - half;
        if (k2 < 0) k2 += win;
        if (k1 > 6) {
            k1 = 12 - k1;
            k2 = k2 == 0 ? 0 : win - k2;
        }
        const double x = mag[(size_t)r * 7 * win + k1 * win + k2];
        out[(int64_t)d * nwin + w0 + r] = log(C * x / nrm[r] + 1.0);
    }
}

// ------------------------------------------------------------------------------------
// F4: one wave per (track, dimension): the exact f64 np.median of the nwin window values (contiguous in logwin);
// NaN anywhere -> NaN (np.median).  med (tracks, D).
// ------------------------------------------------------------------------------------
template <int E>
__global__ __launch_bounds__(256) void ftm2d_median_kernel(const double *__restrict__ logwin, const int64_t *__restrict__ woff,
                                                           int D, double *__restrict__ med)
{
    const int t = blockIdx.y;
    const int d = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (d >= D) return;
    const int n = (int)(woff[t + 1] - woff[t]);
    const double *x = logwin + woff[t] * D + (int64_t)d * n;
    bool nan = false;
    for (int i = threadIdx.x & 63; i < n; i += 64) nan = nan || !(x[i] == x[i]);
    if (__any(nan)) {
        if ((threadIdx.x & 63) == 0) med[(int64_t)t * D + d] = __builtin_nan("");
        return;
    }
    const int k1 = (n - 1) >> 1, k2 = n >> 1;
    uint64_t a, b;
    ftm_wave_select<uint64_t, E>([&](int i) { return ftm_key64(x[i]); }, n, k1, k2, n <= 64 * E, a, b);
    if ((threadIdx.x & 63) == 0) {
        const double lo = ftm_unkey64(a), hi = ftm_unkey64(b);
        med[(int64_t)t * D + d] = (k1 == k2) ? lo : (lo + hi) / 2.0;
    }
}

// F5: one wave per track: shingle = med / sqrt(sum med^2) (fixed-order lane sums + shuffle tree) into out (tracks, D).
__global__ __launch_bounds__(64) void ftm2d_normalize_kernel(const double *__restrict__ med, int D, double *__restrict__ out)
{
    const int t = blockIdx.x, lane = threadIdx.x;
    const double *m = med + (int64_t)t * D;
    double s = 0.0;
    for (int d = lane; d < D; d += 64) s = s + m[d] * m[d];
    for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64);
    const double q = __builtin_sqrt(s);
    for (int d = lane; d < D; d += 64) out[(int64_t)t * D + d] = m[d] / q;
}

// ------------------------------------------------------------------------------------
// Pairs.  score = (float) exp(-sum_k (a_k - b_k)^2), the sum in f64 FMAs over k = 0 .. D-1 in order (the difference
// form: no cancellation).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ftm2d_pairs_kernel(const double *__restrict__ S, int D, const int32_t *__restrict__ pairs,
                                                          int64_t K, float *__restrict__ out)
{
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const double *a = S + (int64_t)pairs[2 * k] * D, *b = S + (int64_t)pairs[2 * k + 1] * D;
    double acc = 0.0;
    for (int i = 0; i < D; ++i) {
        const double d = a[i] - b[i];
        acc = __builtin_fma(d, d, acc);
    }
    out[k] = (float)exp(-acc);
}

// One 64 x 64 block of a grid tile per workgroup (the tile's score layout: rows x cols floats at `offset`, one plane).
// Slabs of FTM_KS dimensions of both sides' shingles go through LDS (k-major, so a thread's 4 rows / 4 columns are
// contiguous); thread (tx, ty) owns rows 4 ty .. 4 ty + 3 and columns 4 tx .. 4 tx + 3.  Dimensions past D read as 0
// on both sides (an exact + 0 to the sum).  Diagonal tiles: i < j (symmetric) or i != j only.
struct FtmTileItem {
    int32_t row0, col0, rows, cols;     // the tile
    int32_t r0, c0;                     // first row / column of this 64 x 64 block inside the tile
    int32_t diagonal, pad;
    int64_t offset;
};

__global__ __launch_bounds__(256) void ftm2d_tile_kernel(const double *__restrict__ S, int D, const FtmTileItem *__restrict__ items,
                                                         int symmetric, float *__restrict__ scores)
{
    __shared__ double As[FTM_KS][FTM_TM + 2];
    __shared__ double Bs[FTM_KS][FTM_TM + 2];
    const FtmTileItem it = items[blockIdx.x];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int nr = it.rows - it.r0 < FTM_TM ? it.rows - it.r0 : FTM_TM;
    const int nc = it.cols - it.c0 < FTM_TM ? it.cols - it.c0 : FTM_TM;
    const double *A = S + (int64_t)(it.row0 + it.r0) * D;
    const double *B = S + (int64_t)(it.col0 + it.c0) * D;
    double acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
    for (int k0 = 0; k0 < D; k0 += FTM_KS) {
#pragma unroll
        for (int q = 0; q < FTM_TM * FTM_KS / 256; ++q) {
            const int e = tid + 256 * q, r = e / FTM_KS, k = e - r * FTM_KS;
            const bool kin = k0 + k < D;
            As[k][r] = (kin && r < nr) ? A[(int64_t)r * D + k0 + k] : 0.0;
            Bs[k][r] = (kin && r < nc) ? B[(int64_t)r * D + k0 + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FTM_KS; ++k) {
            double a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { a[i] = As[k][4 * ty + i]; b[i] = Bs[k][4 * tx + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = a[i] - b[j];
                    acc[i][j] = __builtin_fma(d, d, acc[i][j]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int a = it.r0 + 4 * ty + i, b = it.c0 + 4 * tx + j;
            if (4 * ty + i >= nr || 4 * tx + j >= nc) continue;
            if (it.diagonal && (symmetric ? a >= b : a == b)) continue;
            scores[it.offset + (int64_t)a * it.cols + b] = (float)exp(-acc[i][j]);
        }
}

}  // namespace acx
