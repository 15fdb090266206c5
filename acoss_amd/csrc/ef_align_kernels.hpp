// EarlyFusion: WHERE the constrained Smith-Waterman alignment of a binarised matrix lies, and its path.
//
// The recursion is E4's (ef_kernels.hpp), in integer tenths on the bitmaps the selection kernels leave in d_efbits:
//   T[i][j] = max(0, (B[i][j] ? 10 : -10) + max(U[i-1][j-1], U[i-2][j-1], U[i-1][j-2])),  U = T + (B ? 0 : -7),
//   T = 0 in rows / columns 0, 1;  the cells 2 <= i <= M-2, 2 <= j <= N-2 count.
// Reported in this T frame (rows = blocks of the query, columns = blocks of the reference):
//   end    the counted cell, first in row-major order, at which T attains its maximum
//   pred   of a cell with T > 0: the first of (i-1, j-1), (i-2, j-1), (i-1, j-2) whose U equals the maximum of the three
//   start  the last cell with T > 0 on the chain of predecessors from the end (its chosen predecessor has T == 0)
//   path   the cells from start to end; at most min(M, N) (every step lowers row and column by at least one)
//
// One wave per job (pair), ONE width for every class: a lane owns 16 contiguous columns, 64 lanes cover the 1024 a row may have.
// Rows i-1 and i-2 are plain i32 registers (sw_kernel<16>), the left neighbour's edge values come by DPP.  Every cell gets two
// bits of direction code -- 0: T == 0 (or not counted), 1 / 2 / 3: which predecessor -- so a lane's row is one u32, stored into
// the job's direction plane: M rows of pitch / 16 words (pitch / 4 bytes a row, at most 256 bytes).  A lane's running
// maximum is ONE packed integer -- the value, then the earlier row, then the smaller column -- updated by a plain max, so that an
// earlier row keeps a tie and within a row the smallest column wins; the wave reduction compares the value, then the cell index.  Behind a __threadfence lane 0 walks the codes back from the end
// (qmax_path_kernel's way): cells are written END FIRST, the driver reverses them.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/acx.h"
#include "ef_kernels.hpp"      // EfPair, lane_prev_i

namespace acx {

constexpr int EFA_CPL = 16;                       // columns per lane: 64 lanes x 16 = EF_MAXNB
constexpr int EFA_REC = 6;                        // int32 words of a job's result: acx_alignment's five fields and the cell count
static_assert(64 * EFA_CPL == EF_MAXNB, "a wave covers the longest row of the bit path");

struct EfAlignJob {
    int32_t pair;          // index into the batch's EfPair descriptors
    int32_t max_cells;     // min(M, N): the room of this job in `cells`
    int64_t dir_off;       // first u32 word of the job's direction plane
    int64_t cell_off;      // first cell (x 2 int32) of the job in `cells`
};

__host__ __device__ __forceinline__ int64_t ef_align_dir_words(int M, int pitch) { return (int64_t)M * (pitch / EFA_CPL); }

// The traceback of every kernel here and of ef_sections_kernel, on ONE lane behind the fence that makes the other lanes' codes
// visible: from the end cell (y1, x1) along the codes of `plane` (wpr words a row, word j / 16 of a row holds column j) while a cell
// has one, at most max_cells cells, written to dst END FIRST.  Returns the number of cells and the start in (y0, x0).  lo .. hi are the
// rows the sweep behind the codes ran over (2 .. M - 2 for a whole plot; a free interval's for a section): rows lo - 1 and lo - 2 hold
// T = 0, so a predecessor above lo ends the chain, and no row outside lo .. hi is read (in a sections run the rows above may hold the
// codes of an earlier round).  The path stays inside rows [lo, hi] x columns [2, N-2] (every step lowers row and column), and the
// bounds keep a plane that broke that promise from being read outside, or the job's cells from being written outside.
__device__ __forceinline__ int ef_align_traceback(const unsigned *plane, int64_t wpr, int lo, int hi, int N, int y1, int x1, int max_cells,
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
            if (py < lo || px < 2) break;                            // above the swept rows, or columns 0, 1: T = 0
            code = code_at(py, px);                                  // 0: T == 0 there, (y, x) was the start
            if (code != 0u) { y = py; x = px; }
        }
    }
    y0 = y; x0 = x;
    return n;
}

// A job's result: the acx_alignment record (score's bits, q0, r0, q1, r1) and the number of cells.
__device__ __forceinline__ void ef_align_store(int32_t *rec, const acx_alignment a, int n)
{
    rec[0] = __float_as_int(a.score); rec[1] = a.q0; rec[2] = a.r0; rec[3] = a.q1; rec[4] = a.r1; rec[5] = n;
}

// The sweep of ef_align_kernel and of ef_sections_kernel (ef_sections_kernels.hpp): rows lo .. hi of a job's bitmap (`rows`: M rows of
// pitch / 8 bytes), started from the BITS of rows lo - 1 and lo - 2 -- T = 0 there, U = delta(B): what rows 0 and 1 hold, and what an
// excluded row of a sections run holds.  Writes rows lo .. hi of the direction plane `my_dir` and returns, the same in every lane, the
// maximum in tenths and the counted cell, first in row-major order, that attains it (row * EF_MAXNB + column; 0x7fffffff with a
// maximum of 0).  2 <= lo, hi <= M - 2; no row at all (hi < lo) gives (0, 0x7fffffff).
struct EfBest { int tenths, cell; };

__device__ __forceinline__ EfBest ef_align_sweep(const unsigned char *rows, int M, int N, int pitch, unsigned *my_dir, int lo, int hi)
{
    constexpr int CPL = EFA_CPL;
    const int lane = threadIdx.x;
    const int rowbytes = pitch >> 3, wpr = pitch / CPL;
    const int j0 = CPL * lane;
    const bool inrow = j0 < pitch;
    auto load = [&](int row) -> unsigned {
        const int r = row < M ? row : M - 1;                         // (rows past the last one: a valid address, never used)
        return inrow ? (unsigned)*reinterpret_cast<const unsigned short *>(rows + (size_t)r * rowbytes + 2 * lane) : 0u;
    };
    // A cell is held as V = 4 (U + 8) (U >= -7: positive; the two low bits are free), so that the maximum of the three
    // predecessors AND which one it is come from one v_max3 of V + 2, V + 1, V + 0 in the order (i-1, j-1), (i-2, j-1),
    // (i-1, j-2): equal U's leave the first with the largest key.  With base = key & ~3 = 4 (max U + 8):
    //   4 T = max(0, base - 32 +- 40),  new V = 4 T + (B ? 32 : 4),  code = 3 - (key & 3) where T > 0.
    // valid: bit e = column j0 + e is counted (2 <= j <= N - 2).  T is forced to 0 elsewhere: columns 0, 1 by the recursion's
    // definition, columns right of N - 2 because they feed only columns further right -- so a cell with T > 0 is a counted one.
    unsigned valid = 0u;
#pragma unroll
    for (int e = 0; e < CPL; ++e) valid |= (j0 + e >= 2 && j0 + e <= N - 2) ? (1u << e) : 0u;
    int V1[CPL], V2[CPL];                                            // rows i-1, i-2
    {
        const unsigned w0 = load(lo - 2), w1 = load(lo - 1);         // T = 0 there, U = delta(B)
#pragma unroll
        for (int e = 0; e < CPL; ++e) {
            V2[e] = 4 + 28 * (int)((w0 >> e) & 1u);
            V1[e] = 4 + 28 * (int)((w1 >> e) & 1u);
        }
    }
    // The running maximum of a lane as ONE integer, (4 T) << 14 | (1023 - i) << 4 | (15 - e): larger T first, then the earlier
    // row, then the smaller column (4 T <= 40 960 < 2^16: 30 bits).
    int best_key = 0;
    // one row: VA = row i-1, VB = row i-2 (overwritten with row i, from the right: cell e reads VB[e - 1] before it is replaced)
    auto dp_row = [&](int i, unsigned wb, int (&VA)[CPL], int (&VB)[CPL]) {
        const int a1 = lane_prev_i(VA[CPL - 1]), a2 = lane_prev_i(VA[CPL - 2]), b1 = lane_prev_i(VB[CPL - 1]);
        const int row_key = (EF_MAXNB - 1 - i) << 4;
        unsigned codes = 0u;
        // (opaque per row: sixteen loop-invariant lane masks hoisted out of the row loop would take 32 SGPRs and spill)
        int vm = (int)valid;
        asm volatile("" : "+v"(vm));
#pragma unroll
        for (int e = CPL - 1; e >= 0; --e) {
            const int k2 = ((e >= 1) ? VA[e - 1] : a1) + 2;                               // (i-1, j-1)
            const int k3 = ((e >= 1) ? VB[e - 1] : b1) + 1;                               // (i-2, j-1)
            const int k4 = (e >= 2) ? VA[e - 2] : (e == 1 ? a1 : a2);                     // (i-1, j-2)
            const int key = max(max(k2, k3), k4);
            const int bit = (int)((wb >> e) & 1u);
            int t4 = (key & ~3) - 72 + 80 * bit;
            t4 = max(t4, 0) & __builtin_amdgcn_sbfe(vm, e, 1);                    // (sbfe of one bit: 0 or -1)
            VB[e] = t4 + 4 + 28 * bit;
            const unsigned code = t4 > 0 ? 3u - (unsigned)(key & 3) : 0u;
            codes |= code << (2 * e);
            best_key = max(best_key, ((t4 << 14) | (15 - e)) | row_key);
        }
        if (inrow) my_dir[(size_t)i * wpr + lane] = codes;
    };
    // rows in flight ahead of the recursion, as in sw_bits_h16_kernel.  The ring starts at row lo, whatever its row & 7, and the
    // register rows only alternate, so lo may have either parity: row lo - 1 is V1, and SW_PF is even
    constexpr int SW_PF = 8;
    unsigned ring[SW_PF];
#pragma unroll
    for (int sl = 0; sl < SW_PF; ++sl) ring[sl] = load(lo + sl);
    for (int i0 = lo; i0 <= hi; i0 += SW_PF) {
#pragma unroll
        for (int sl = 0; sl < SW_PF; ++sl) {
            const int i = i0 + sl;
            if (i <= hi) {                                           // wave-uniform
                const unsigned wb = ring[sl];
                ring[sl] = load(i + SW_PF);
                if (sl & 1) dp_row(i, wb, V2, V1); else dp_row(i, wb, V1, V2);
            }
        }
    }
    // the maximum and, among equal maxima, the smallest cell index (a plain maximum would lose which lane's cell comes first)
    EfBest r;
    r.tenths = best_key >> 16;                                       // (4 T) >> 2
    r.cell = r.tenths > 0 ? (EF_MAXNB - 1 - ((best_key >> 4) & (EF_MAXNB - 1))) * EF_MAXNB + j0 + 15 - (best_key & 15) : 0x7fffffff;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const int ob = __shfl_xor(r.tenths, o, 64), oc = __shfl_xor(r.cell, o, 64);
        if (ob > r.tenths || (ob == r.tenths && oc < r.cell)) { r.tenths = ob; r.cell = oc; }
    }
    return r;
}

__global__ __launch_bounds__(64) void ef_align_kernel(const EfPair *__restrict__ pd, const EfAlignJob *__restrict__ jobs,
                                                      const unsigned *__restrict__ bits, unsigned *dir,
                                                      int32_t *__restrict__ res, int plane)
{
    // res: EFA_REC words per job -- the acx_alignment record (score's bits, q0, r0, q1, r1) and the number of cells -- then the
    // cells of all jobs (job.cell_off), so that one copy brings a chunk's results back
    int32_t *cells = res + (size_t)EFA_REC * gridDim.x;
    const int lane = threadIdx.x;
    const EfAlignJob job = jobs[blockIdx.x];
    const EfPair P = pd[job.pair];
    const int M = P.M, N = P.N, pitch = P.pitchC;
    acx_alignment a;
    a.score = 0.0f; a.q0 = a.r0 = a.q1 = a.r1 = -1;
    int n = 0;
    if (M >= 4 && N >= 4) {
        const unsigned char *rows = reinterpret_cast<const unsigned char *>(bits + P.offB + (int64_t)plane * M * (pitch >> 5));
        unsigned *my_dir = dir + job.dir_off;
        const EfBest b = ef_align_sweep(rows, M, N, pitch, my_dir, 2, M - 2);
        // the traceback reads the whole plane: same wave, but other lanes' stores, through memory
        __threadfence();
        if (lane == 0 && b.tenths > 0) {
            int y = b.cell / EF_MAXNB, x = b.cell % EF_MAXNB;
            n = ef_align_traceback(my_dir, pitch / EFA_CPL, 2, M - 2, N, y, x, job.max_cells, cells + 2 * job.cell_off, y, x);
            a.score = (float)b.tenths / 10.0f;                       // (a positive score without a cell: the driver reports it)
            if (n > 0) {
                a.q1 = b.cell / EF_MAXNB; a.r1 = b.cell % EF_MAXNB;
                a.q0 = y; a.r0 = x;
            }
        }
    }
    if (lane == 0) ef_align_store(res + (size_t)EFA_REC * blockIdx.x, a, n);
}

// The same alignment on the FLOAT path, for plots of any size: a batch that holds a track of more than
// EF_MAXNB blocks keeps no bitmaps, so a cell of the plot is what sw_long_kernel::load_b reads off the pair's float matrix, its row's
// threshold t and tie column jcut.  One wave per job again, a lane owns 16 contiguous columns, and a plot of N columns runs in
// ceil(N / 1024) STRIPS as sw_long_kernel's does: for every row lane 63 leaves U[i][c-1], U[i][c-2] (c: the next strip's first column)
// in the pair's record area -- sw_long_kernel's own records, free once the batch's score launch has finished on the stream -- double
// buffered by strip, and lane 0 of the next strip reads them in place of its left neighbour.  A strip ends in __threadfence().
//   direction plane   M rows of 64 * nstrips words (word j / 16 of a row holds column j); EVERY word of rows 2 .. M-2 is written in
//                     every strip, zeros included: the traceback stops on a 0, and the plane is reused between calls
//   running best      T, row and column as three integers per lane (T passes 16 bits and rows pass 1023 here; a pair may hold more
//                     than 2^32 cells): replaced by a larger T, or by an equal T in an EARLIER row -- strip 2 meets row 3 after
//                     strip 1 met row 300 -- and within a row by the smaller column; the wave reduction compares T, row, column
//   traceback         lane 0, behind the last strip's fence, bounded by min(M, N) cells and by the counted rectangle
constexpr int EFA_STRIP = 64 * EFA_CPL;           // columns of one strip

__host__ __device__ __forceinline__ int ef_align_long_strips(int N) { return (N + EFA_STRIP - 1) / EFA_STRIP; }
__host__ __device__ __forceinline__ int64_t ef_align_long_dir_words(int M, int N) { return (int64_t)M * 64 * ef_align_long_strips(N); }

__global__ __launch_bounds__(64) void ef_align_long_kernel(const EfPair *__restrict__ pd, const EfAlignJob *__restrict__ jobs,
                                                           const float *__restrict__ scratch, float *stat, unsigned *dir,
                                                           int32_t *__restrict__ res, int plane)
{
    int32_t *cells = res + (size_t)EFA_REC * gridDim.x;              // the result block of ef_align_kernel
    constexpr int CPL = EFA_CPL;
    const int lane = threadIdx.x;
    const EfAlignJob job = jobs[blockIdx.x];
    const EfPair P = pd[job.pair];
    const int M = P.M, N = P.N, pitch = P.pitchC;
    acx_alignment a;
    a.score = 0.0f; a.q0 = a.r0 = a.q1 = a.r1 = -1;
    int n = 0;
    if (M >= 4 && N >= 4) {
        const float *C = scratch + (plane < 3 ? ef_c_off(P, plane) : ef_f_off(P));
        const float *thr = stat + P.offS + plane * ef_s_stride(P);
        const int *jcut = reinterpret_cast<const int *>(thr) + ef_jcut_off(P, plane);
        unsigned long long *rec = reinterpret_cast<unsigned long long *>(stat + P.offS + ef_rec_off(P, plane));     // int2 {U[c-1], U[c-2]}
        const int nstrips = ef_align_long_strips(N);
        const int64_t wpr = 64 * (int64_t)nstrips;
        unsigned *my_dir = dir + job.dir_off;
        int bT = 0, bRow = 0, bCol = 0;                              // the lane's running best (bT == 0: none yet)
        for (int st = 0; st < nstrips; ++st) {
            const int j0 = st * EFA_STRIP + CPL * lane;
            const unsigned long long *rin = rec + (size_t)((st + 1) & 1) * P.pitchT;
            unsigned long long *rout = rec + (size_t)(st & 1) * P.pitchT;
            const bool more = st + 1 < nstrips, seam = st > 0;
            // the plot's row as 16 bits: sw_long_kernel::load_b.  j >= N reads no memory and is 0: such a column reads column N - 1
            // in its place, and `have` drops its bit
            const int nv = min(max(N - j0, 0), CPL);
            const unsigned have = (1u << nv) - 1u;
            auto load_b = [&](int row) -> unsigned {
                const int r = row < M ? row : M - 1;                 // (rows past the last one: a valid address, never used)
                const float t = thr[r];
                const int jc = jcut[r];
                const float *Cr = C + (size_t)r * pitch;
                float d[CPL];
#pragma unroll
                for (int e = 0; e < CPL; ++e) d[e] = Cr[(unsigned)min(j0 + e, N - 1)];
                // ties: bit e = column j0 + e <= jcut.  jcut is clamped into [j0 - 1, j0 + 15] BEFORE the subtraction: the selection
                // kernels write 0x7fffffff for a row whose every tie counts, and jcut - j0 + 1 would overflow in lane 0 of strip 0
                const int ec = min(max(jc, j0 - 1), j0 + CPL - 1) - j0 + 1;
                const unsigned tie = (1u << ec) - 1u;
                unsigned w = 0u;
#pragma unroll
                for (int e = 0; e < CPL; ++e) w |= (d[e] < t ? 1u : (d[e] == t ? ((tie >> e) & 1u) : 0u)) << e;
                return w & have;
            };
            // a record: the two values as one 8-byte word, so that a row's record is one store and one load (relaxed, agent scope:
            // the other lanes' stores of the strip before, read through memory behind its fence)
            auto put_rec = [&](int row, int u1, int u2) {
                if (more && lane == 63) rout[row] = (unsigned long long)(unsigned)u1 | ((unsigned long long)(unsigned)u2 << 32);
            };
            auto get_rec = [&](int row) -> unsigned long long {
                return seam ? __hip_atomic_load(rin + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            };
            // valid: bit e = column j0 + e is counted (2 <= j <= N - 2); T is forced to 0 elsewhere, as in ef_align_kernel
            unsigned valid = 0u;
#pragma unroll
            for (int e = 0; e < CPL; ++e) valid |= (j0 + e >= 2 && j0 + e <= N - 2) ? (1u << e) : 0u;
            int U1[CPL], U2[CPL];                                    // rows i-1, i-2
            {
                const unsigned w0 = load_b(0), w1 = load_b(1);       // rows 0 and 1: T = 0, U = delta(B)
#pragma unroll
                for (int e = 0; e < CPL; ++e) {
                    U2[e] = ((w0 >> e) & 1u) ? 0 : -7;
                    U1[e] = ((w1 >> e) & 1u) ? 0 : -7;
                }
                put_rec(0, U2[CPL - 1], U2[CPL - 2]);
                put_rec(1, U1[CPL - 1], U1[CPL - 2]);
            }
            unsigned long long recB = get_rec(0), recA = get_rec(1); // records of rows i-2, i-1
            // one row: UA = row i-1, UB = row i-2 (overwritten with row i, from the right: cell e reads UB[e - 1] before it is replaced)
            auto dp_row = [&](int i, unsigned wb, int (&UA)[CPL], int (&UB)[CPL]) {
                int a1 = lane_prev_i(UA[CPL - 1]), a2 = lane_prev_i(UA[CPL - 2]), b1 = lane_prev_i(UB[CPL - 1]);
                if (lane == 0) { a1 = (int)(unsigned)recA; a2 = (int)(unsigned)(recA >> 32); b1 = (int)(unsigned)recB; }
                unsigned codes = 0u;
                int rT = 0, rE = 0;                                  // the row's maximum in this lane, at its smallest column
#pragma unroll
                for (int e = CPL - 1; e >= 0; --e) {
                    const int c2 = (e >= 1) ? UA[e - 1] : a1;                             // (i-1, j-1)
                    const int c3 = (e >= 1) ? UB[e - 1] : b1;                             // (i-2, j-1)
                    const int c4 = (e >= 2) ? UA[e - 2] : (e == 1 ? a1 : a2);             // (i-1, j-2)
                    int mx = c2;
                    unsigned code = 1u;
                    if (c3 > mx) { mx = c3; code = 2u; }
                    if (c4 > mx) { mx = c4; code = 3u; }
                    const int bit = (int)((wb >> e) & 1u);
                    int t = mx - 10 + 20 * bit;
                    t = max(t, 0) & __builtin_amdgcn_sbfe((int)valid, e, 1);              // (sbfe of one bit: 0 or -1)
                    UB[e] = t - 7 + 7 * bit;
                    codes |= (t > 0 ? code : 0u) << (2 * e);
                    if (t >= rT) { rT = t; rE = e; }                 // (from the right: an equal value further left wins)
                }
                my_dir[i * wpr + 64 * st + lane] = codes;
                put_rec(i, UB[CPL - 1], UB[CPL - 2]);
                if (rT > bT || (rT == bT && rT > 0 && i < bRow)) { bT = rT; bRow = i; bCol = j0 + rE; }
            };
            unsigned wb = load_b(2);
            for (int i = 2; i <= M - 2; ++i) {
                const unsigned wn = load_b(i + 1);                   // the next row and its record, ahead of their use
                const unsigned long long recN = get_rec(i);
                dp_row(i, wb, U1, U2);
#pragma unroll
                for (int e = 0; e < CPL; ++e) { const int u = U1[e]; U1[e] = U2[e]; U2[e] = u; }
                wb = wn;
                recB = recA; recA = recN;
            }
            __threadfence();                                         // the next strip reads this one's records, the traceback every strip's codes
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const int oT = __shfl_xor(bT, o, 64), oR = __shfl_xor(bRow, o, 64), oC = __shfl_xor(bCol, o, 64);
            if (oT > bT || (oT == bT && (oR < bRow || (oR == bRow && oC < bCol)))) { bT = oT; bRow = oR; bCol = oC; }
        }
        if (lane == 0 && bT > 0) {
            int y = bRow, x = bCol;
            n = ef_align_traceback(my_dir, wpr, 2, M - 2, N, y, x, job.max_cells, cells + 2 * job.cell_off, y, x);
            a.score = (float)bT / 10.0f;                             // sw_long_kernel's expression: the same bits
            if (n > 0) {
                a.q1 = bRow; a.r1 = bCol;
                a.q0 = y; a.r0 = x;
            }
        }
    }
    if (lane == 0) ef_align_store(res + (size_t)EFA_REC * blockIdx.x, a, n);
}

}  // namespace acx
