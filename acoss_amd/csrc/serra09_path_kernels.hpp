// Serra09: the PATH of the Qmax alignment between its start and its end.
//
//   P1 qmax_path_kernel<EQG>  the Qmax recursion over the cells of the box [q0, q1] x [r0, r1] that qmax_locate_kernel reported, with 0
//                             for every Q outside it, storing one 2-bit predecessor code per cell; then a traceback over the codes from
//                             the box's last cell.  One wave per pair with a match, 32 box columns per lane, strips of 2048 box columns.
//
// The contract is section 16's (serra09_locate_kernels.hpp): the same f32 values, the same strict `>` chains.  The BOX PROPERTY makes the
// box enough: the recursion is monotone in its inputs, so Q_box <= Q_full everywhere; the path's first cell is a match cell with Q = 1 in
// both; by induction every path cell keeps its value; a predecessor that ties the chosen one in the box would tie or beat it in the full
// matrix and would have been chosen there; every step lowers row and column by at least 1, so the path lies inside the box.
//   code   0: no predecessor (a path starts here, or the cell holds 0 and lies on no path); 1 / 2 / 3: (i-1, j-1) / (i-2, j-1) / (i-1, j-2)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/acx.h"
#include "serra09_kernels.hpp"      // PairDesc, BAND, lane_prev_*
#include "serra09_locate_kernels.hpp"   // loc_sel_gt, loc_sel_eq0

namespace acx {

constexpr int PATH_CPL = 32;                     // box columns a lane owns: one 64-bit code word per lane and row
constexpr int PATH_STRIP = 64 * PATH_CPL;        // box columns of one strip

// What a strip leaves for the next one, per box row: Q and the penalised Q of its two rightmost columns
// (x1 = box column c - 1, x2 = box column c - 2; c = first box column of the next strip).
struct alignas(16) PathSeam {
    float q1, q2, p1, p2;
};

// One wave's work: the box of a pair of the batch, and where its direction plane, seam records and cells lie.
struct PathBox {
    int32_t pair;          // the pair's descriptor (index into the batch's PairDesc array)
    int32_t q0, r0, q1, r1;
    int32_t max_cells;     // min(q1 - q0, r1 - r0) + 1: no path is longer
    int64_t dir_off;       // first u64 word of the direction plane: rows x path_words(width) words
    int64_t seam_off;      // first seam record: two buffers of one record per box row (boxes wider than one strip only)
    int64_t cell_off;      // first cell (two int32 each) of the pair's path in the cell buffer, written END FIRST
};

__host__ __device__ inline int path_words(int width) { return (width + PATH_CPL - 1) / PATH_CPL; }
__host__ __device__ inline int path_strips(int width) { return (width + PATH_STRIP - 1) / PATH_STRIP; }
// bytes of device memory a box takes in the chunk: direction plane + seam records
inline int64_t path_box_bytes(int rows, int width)
{
    return (int64_t)rows * path_words(width) * 8 + (path_strips(width) > 1 ? 2 * (int64_t)rows * (int64_t)sizeof(PathSeam) : 0);
}

// A lane's codes of box row y (column e at bits [2 e, 2 e + 2) of hi : lo), as one word of the row's plane.
__device__ __forceinline__ void path_store_codes(unsigned long long *plane, int y, int nwords, int word, unsigned lo, unsigned hi)
{
    plane[(size_t)y * nwords + word] = ((unsigned long long)hi << 32) | lo;
}

// What lane 63 leaves of box row y for the next strip (EQG: no penalised values, PB has one element that is not read).
template <bool EQG, int NP>
__device__ __forceinline__ void path_store_seam(PathSeam *bout, int y, const float (&QB)[PATH_CPL], const float (&PB)[NP])
{
    PathSeam o;
    o.q1 = QB[PATH_CPL - 1]; o.q2 = QB[PATH_CPL - 2];
    o.p1 = EQG ? 0.0f : PB[NP - 1]; o.p2 = EQG ? 0.0f : PB[EQG ? 0 : NP - 2];
    bout[y] = o;
}

// The traceback of a box of H rows and Wd columns, on one lane behind the last strip's fence: from the box's last cell along the codes
// until a cell has none; the cells are written END FIRST, their number is returned.  It never leaves the box (every step lowers row and
// column, and a cell of the path has its predecessor in the box: the box property); the bounds keep a plane that broke that promise
// from being read or written outside.  (n, x, y are declared in this order: the four kernels' listings follow it.)
__device__ __forceinline__ int path_traceback(const unsigned long long *plane, int nwords, const PathBox &bx, int H, int Wd, int32_t *out)
{
    int n = 0, x = Wd - 1, y = H - 1;
    while (n < bx.max_cells && y >= 0 && x >= 0) {
        out[2 * n] = bx.q0 + y; out[2 * n + 1] = bx.r0 + x;
        ++n;
        const unsigned long long wd = __hip_atomic_load(plane + (size_t)y * nwords + (x >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned code = (unsigned)(wd >> (2 * (x & 31))) & 3u;
        if (code == 0u) break;
        y -= (code == 2u) ? 2 : 1;
        x -= (code == 3u) ? 2 : 1;
    }
    return n;
}

template <bool EQG>
__global__ __launch_bounds__(64) void qmax_path_kernel(const PairDesc *__restrict__ pd, const PathBox *__restrict__ boxes,
                                                       const unsigned long long *__restrict__ bits,
                                                       unsigned long long *__restrict__ dir, PathSeam *__restrict__ seam,
                                                       int32_t *__restrict__ cells, int32_t *__restrict__ n_cells,
                                                       float go, float ge)
{
    constexpr int CPL = PATH_CPL;
    constexpr int NP = EQG ? 1 : CPL;
    const int lane = threadIdx.x;
    const PathBox bx = boxes[blockIdx.x];
    const PairDesc P = pd[bx.pair];
    const int H = bx.q1 - bx.q0 + 1, Wd = bx.r1 - bx.r0 + 1;        // rows and columns of the box
    const int nwords = path_words(Wd);
    const int ndw = 2 * P.nw;
    const unsigned *rows = reinterpret_cast<const unsigned *>(bits + P.offT);
    unsigned long long *plane = dir + bx.dir_off;
    const int nstrips = path_strips(Wd);
    PathSeam *bnd = nstrips > 1 ? seam + bx.seam_off : nullptr;

    for (int s = 0; s < nstrips; ++s) {
        const int cbase = s * PATH_STRIP + CPL * lane;               // this lane's first box column
        const PathSeam *bin = bnd + (size_t)((s + 1) & 1) * H;       // records of strip s - 1 (read for s > 0 only)
        PathSeam *bout = bnd + (size_t)(s & 1) * H;
        const bool more = s + 1 < nstrips;
        unsigned colmask = 0u;                                       // box columns of this lane that exist
#pragma unroll
        for (int e = 0; e < CPL; ++e)
            if (cbase + e < Wd) colmask |= (1u << e);
        const int word = s * 64 + lane;                              // this lane's code word in a plane row
        const bool has_word = word < nwords;
        float Q1[CPL], Q2[CPL], P1[NP], P2[NP];                      // box rows above the box are 0
#pragma unroll
        for (int e = 0; e < CPL; ++e) {
            Q1[e] = 0.0f; Q2[e] = 0.0f;
            if constexpr (!EQG) { P1[e] = 0.0f; P2[e] = 0.0f; }
        }
        // The lane's 32 recurrence bits of box row y: plot row i = q0 + y, plot columns r0 + cbase ..; bit position of plot column j in
        // the row's bitmap is j + (BAND - 1) - (i & (BAND - 1)), so the dwords that hold them move with the row.
        // No branch: a row behind the box is the box's last row again (loaded, never used), and a dword behind the row's last is the last
        // again -- it would hold columns right of the plot, which colmask clears whatever is loaded for them.
        auto load_row = [&](int y, unsigned &d0, unsigned &d1) {
            const int i = bx.q0 + min(y, H - 1);
            const int pos = bx.r0 + cbase + (BAND - 1) - (i & (BAND - 1));
            const int dw0 = pos >> 5;
            const unsigned *r = rows + (size_t)i * ndw;
            d0 = r[min(dw0, ndw - 1)];
            d1 = r[min(dw0 + 1, ndw - 1)];
        };
        PathSeam recA = {0.0f, 0.0f, 0.0f, 0.0f}, recB = recA;      // the left strip's box rows y - 1 and y - 2

        // One box row: QA / PA = row y-1, QB / PB = row y-2 (overwritten with row y), descending column order
        auto dp_row = [&](int y, unsigned d0, unsigned d1, float (&QA)[CPL], float (&QB)[CPL], float (&PA)[NP], float (&PB)[NP]) {
            PathSeam recN = recA;                                    // the left strip's row y, for row y + 1
            if (s > 0) recN = bin[y];
            const int i = bx.q0 + y;
            const int sh = (bx.r0 + cbase + (BAND - 1) - (i & (BAND - 1))) & 31;
            const unsigned w = __builtin_amdgcn_alignbit(d1, d0, sh) & colmask;
            float l1a = lane_prev_f(QA[CPL - 1]), l1b = lane_prev_f(QA[CPL - 2]), l2a = lane_prev_f(QB[CPL - 1]);
            float p1a = 0.f, p1b = 0.f, p2a = 0.f;
            if constexpr (!EQG) {
                p1a = lane_prev_f(PA[NP - 1]); p1b = lane_prev_f(PA[NP - 2]); p2a = lane_prev_f(PB[NP - 1]);
            }
            if (lane == 0) {                                         // (strip 0: the zeros left of the box)
                l1a = recA.q1; l1b = recA.q2; l2a = recB.q1;
                p1a = recA.p1; p1b = recA.p2; p2a = recB.p1;
            }
            unsigned lo = 0u, hi = 0u;                               // the row's codes: column e at bits [2 e, 2 e + 2)
#pragma unroll
            for (int e = CPL - 1; e >= 0; --e) {
                [[maybe_unused]] const bool r = (w >> e) & 1u;
                const float c2 = (e >= 1) ? QA[e - 1] : l1a;                          // (i-1, j-1)
                const float c3 = (e >= 1) ? QB[e - 1] : l2a;                          // (i-2, j-1)
                const float c4 = (e >= 2) ? QA[e - 2] : (e == 1 ? l1a : l1b);         // (i-1, j-2)
                const float m23 = fmaxf(c2, c3), mx = fmaxf(m23, c4);
                float q;
                unsigned code;
                if constexpr (EQG) {
                    // the first of c2, c3, c4 equal to mx; mx == 0: a match cell starts a path, a gap cell holds 0 and lies on none
                    // (each select ONE compare into vcc with its v_cndmask right behind it, and the two branches of q blended by the
                    // sign-extended recurrence bit, as in qmax_locate_kernel<true>: written as plain C++ the row's 96 lane masks are
                    // kept in SGPRs behind the Q chain -- 49 SGPR spills to VGPR lanes)
                    code = loc_sel_gt(c4, m23, 3u, loc_sel_gt(c3, c2, 2u, 1u));
                    code = loc_sel_eq0((unsigned)__float_as_int(mx), 0u, code);       // (mx >= 0 is never -0: its bits are 0)
                    int rm = __builtin_amdgcn_sbfe((int)w, e, 1);
                    asm("" : "+v"(rm));      // (opaque: seen through, the blend becomes 32 bit tests into SGPR lane masks and their selects)
                    const float t = __int_as_float((rm & __float_as_int(1.0f)) | (~rm & __float_as_int(-go)));
                    q = fmaxf(mx + t, 0.0f);
                } else {
                    unsigned cm = (c3 > c2) ? 2u : 1u;
                    cm = (c4 > m23) ? 3u : cm;
                    cm = (mx == 0.0f) ? 0u : cm;
                    const float a2 = (e >= 1) ? PA[e - 1] : p1a;
                    const float a3 = (e >= 1) ? PB[e - 1] : p2a;
                    const float a4 = (e >= 2) ? PA[e - 2] : (e == 1 ? p1a : p1b);
                    const float n23 = fmaxf(a2, a3), amx = fmaxf(n23, a4);
                    unsigned ca = (a3 > a2) ? 2u : 1u;                                // (a gap cell with amx <= 0 holds 0: on no path)
                    ca = (a4 > n23) ? 3u : ca;
                    q = r ? (mx + 1.0f) : fmaxf(amx, 0.0f);
                    code = r ? cm : ca;
                }
                // A column right of the box takes the gap branch (its bit is masked) and feeds only columns further right: no cell of
                // the box reads it, and its code word bits are never visited (the traceback stays inside the box).
                QB[e] = q;
                if constexpr (!EQG) PB[e] = q - (r ? go : ge);
                if (e >= 16) hi |= code << (2 * (e - 16)); else lo |= code << (2 * e);
            }
            if (has_word) path_store_codes(plane, y, nwords, word, lo, hi);
            if (more && lane == 63) path_store_seam<EQG>(bout, y, QB, PB);
            recB = recA; recA = recN;
        };

        unsigned a0, a1, b0, b1;
        load_row(0, a0, a1); load_row(1, b0, b1);
        for (int y = 0; y < H; y += 2) {
            unsigned n0, n1;
            load_row(y + 2, n0, n1);
            dp_row(y, a0, a1, Q1, Q2, P1, P2);
            a0 = n0; a1 = n1;
            if (y + 1 < H) {
                load_row(y + 3, n0, n1);
                dp_row(y + 1, b0, b1, Q2, Q1, P2, P1);
                b0 = n0; b1 = n1;
            }
        }
        // the next strip reads this one's records, the traceback the whole plane: same wave, but through memory
        __threadfence();
    }

    if (lane == 0) n_cells[blockIdx.x] = path_traceback(plane, nwords, bx, H, Wd, cells + 2 * bx.cell_off);
}

}  // namespace acx
