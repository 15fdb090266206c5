// The EarlyFusion batch plan (host code, no device work): how a pair list is checked, sized, packed into scratch-sized
// batches of equal size, put into run order, and which kernels a batch launches.  A pure function of (block counts per
// track, pair list, parameters, scratch limit, the per-process switch): run_ef_impl (acx.hip) follows it, launch_ef_batch
// switches on its answer, and acx_ef_plan reports it without a device, which is what tests/test_ef_plan.py reads.  A
// limit, the sizing formula or a kernel choice is changed HERE and nowhere else.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/acx.h"
#include "ef_kernels.hpp"      // EfPair, EF_MAXNB, EF_COLSTAT_MAXK, ef_s_total (the struct the kernels read: its layout lives with them)

namespace acx {

// block counts as the run sees them: the uploaded pool's block offsets
struct EfLengths {
    const int64_t *off;
    int n_tracks;
    int64_t blocks(int t) const { return off[t + 1] - off[t]; }
};

// The whole list before the first launch: the first pair with an index out of range (ACX_ERR_INVALID), else the first pair
// with a track without blocks (ACX_ERR_SHORT); `k` is that pair.  Whether a pool is up at all is the caller's to say first.
struct EfCheck { int code; int64_t k; };
inline EfCheck ef_check_pairs(const EfLengths &len, const int32_t *pairs, int64_t K)
{
    int64_t first_short = -1;
    for (int64_t k = 0; k < K; ++k) {
        const int32_t q = pairs[2 * k], r = pairs[2 * k + 1];
        if (q < 0 || r < 0 || q >= len.n_tracks || r >= len.n_tracks) return EfCheck{ACX_ERR_INVALID, k};
        if (first_short < 0 && (len.blocks(q) < 1 || len.blocks(r) < 1)) first_short = k;
    }
    return first_short >= 0 ? EfCheck{ACX_ERR_SHORT, first_short} : EfCheck{ACX_OK, K};
}

// csm_to_binary's neighbours per row (cross_recurrence.py:149-154): kappa == 0 -> all ones; kappa < 1 ->
// int(round(kappa * ncols)) (numpy: half to even, in f64); else kappa neighbours
inline int ef_kbin(double kappa, int N)
{
    if (kappa == 0.0) return N;
    if (kappa < 1.0) return (int)std::nearbyint(kappa * (double)N);
    return (int)kappa;
}

inline int ef_pitch(int n) { return (n + 63) / 64 * 64; }

// The descriptor of a pair of M x N blocks but for its arena offsets (0 here: a pair alone in every arena).
inline EfPair ef_pair_desc(int32_t q, int32_t r, int M, int N, double kappa, bool keep_ct)
{
    EfPair d;
    d.q = q; d.r = r; d.M = M; d.N = N; d.oti = 0;
    d.pitchC = ef_pitch(N); d.pitchT = ef_pitch(M);
    d.kbin = ef_kbin(kappa, N);
    d.ctN = keep_ct ? N : 0;
    d.pad = 0; d.offB = 0; d.offC = 0; d.offS = 0;
    return d;
}

// ---- what a list keeps per pair -----------------------------------------------------------------
//   keep_ct    the transposed matrices: the column statistics (mean of the K smallest of every column) come from C itself up to
//              K = EF_COLSTAT_MAXK (ef_colstat_kernel); larger neighbourhoods take the row kernels on C^T
//   bits_path  tracks of up to EF_MAXNB blocks (rows that fit a wave's registers): the selection kernels leave the BINARISED
//              rows behind, the fused matrix is made and binarised in registers and the Smith-Waterman kernel walks bits.  ONE
//              longer track in the list: every batch keeps the streaming kernels' float matrices
//   keep_f     the fused matrix is stored: the float path, or the debug entry asks for it
struct EfMode { bool keep_ct, bits_path, keep_f; };
// (a CHECKED list of the pool)
inline EfMode ef_mode(const EfLengths &len, const int32_t *pairs, int64_t K, int Kn, bool want_fused)
{
    EfMode m{Kn > EF_COLSTAT_MAXK, true, false};
    for (int64_t k = 0; k < K && m.bits_path; ++k)
        m.bits_path = len.blocks(pairs[2 * k]) <= EF_MAXNB && len.blocks(pairs[2 * k + 1]) <= EF_MAXNB;
    m.keep_f = !m.bits_path || want_fused;
    return m;
}
// (a caller's matrix of M x N: no column statistics at all)
inline EfMode ef_mode_matrix(int M, int N, bool want_fused)
{
    const bool bits = M <= EF_MAXNB && N <= EF_MAXNB;
    return EfMode{false, bits, !bits || want_fused};
}

// floats of the scratch arena a pair takes: [C x3][C^T x3 (ctN rows each)][F]
inline int64_t ef_pair_floats(const EfPair &d, bool keep_f) { return (int64_t)(keep_f ? 4 : 3) * d.M * d.pitchC + (int64_t)3 * d.ctN * d.pitchT; }

inline EfPair ef_list_pair(const EfLengths &len, const int32_t *pairs, int64_t k, double kappa, const EfMode &mode)
{
    const int32_t q = pairs[2 * k], r = pairs[2 * k + 1];
    return ef_pair_desc(q, r, (int)len.blocks(q), (int)len.blocks(r), kappa, mode.keep_ct);
}

// ---- batches ---------------------------------------------------------------------------------------
// The sizes of a CHECKED list: the first pair that cannot fit the limit on its own (-1: none), and the floats of a batch.
// Batches of EQUAL size: a list that needs 1.3 limits runs as 0.65 + 0.65, not 1.0 + 0.3 (the last kernels of a batch run
// on a draining device; a small trailing batch pays that for little work -- a 128 x 128 grid tile of 400-block tracks is
// 16 384 pairs = 31 GB of matrices): total / ceil(total / limit), 2 % and 2^22 floats of slack for the greedy fill.
struct EfSizes { int64_t too_big; int64_t batch_floats; };
inline EfSizes ef_batch_floats(const EfLengths &len, const int32_t *pairs, int64_t K, double kappa, const EfMode &mode, int64_t limit_floats)
{
    double total = 0.0;
    for (int64_t k = 0; k < K; ++k) {
        const int64_t need = ef_pair_floats(ef_list_pair(len, pairs, k, kappa, mode), mode.keep_f);
        if (need > limit_floats) return EfSizes{k, limit_floats};
        total += (double)need;
    }
    if (K <= 1 || total <= (double)limit_floats) return EfSizes{-1, limit_floats};
    const double nb = std::ceil(total / (double)limit_floats);
    return EfSizes{-1, std::min<int64_t>(limit_floats, (int64_t)(total / nb * 1.02) + ((int64_t)1 << 22))};
}

// what a batch takes of the arenas and spans: floats of d_scratch and d_thr, words of d_efbits; cells (its profile records)
// and the longest sides (its grids, its kernels)
struct EfArena {
    int64_t used = 0, used_s = 0, used_b = 0, cells = 0;
    int maxM = 0, maxN = 0;
};
// the next pair of a batch: its offsets, then the arenas grow by it
inline void ef_arena_add(EfArena &a, EfPair &d, bool keep_f)
{
    d.offC = a.used;
    d.offS = a.used_s;
    d.offB = a.used_b;
    a.used += ef_pair_floats(d, keep_f);
    a.used_s += ef_s_total(d);
    a.used_b += (int64_t)4 * d.M * (d.pitchC / 32);
    a.maxM = std::max(a.maxM, d.M);
    a.maxN = std::max(a.maxN, d.N);
    a.cells += (int64_t)d.M * d.N;
}

// The batch that starts at pair k_from of a CHECKED and SIZED list: greedily, in list order, as many pairs as fit
// batch_floats -- the first is always taken -- and at most 65535 (a grid dimension).  Fills `pd` with their descriptors,
// arena offsets included, `used` with the arenas' extents, and returns the end of the batch.
inline int64_t ef_pack_batch(const EfLengths &len, const int32_t *pairs, int64_t k_from, int64_t K, const acx_ef_params &p, const EfMode &mode,
                             int64_t batch_floats, std::vector<EfPair> &pd, EfArena &used)
{
    pd.clear();
    used = EfArena();
    int64_t k = k_from;
    for (; k < K && pd.size() < 65535; ++k) {
        EfPair d = ef_list_pair(len, pairs, k, p.kappa, mode);
        if (used.used + ef_pair_floats(d, mode.keep_f) > batch_floats && !pd.empty()) break;
        ef_arena_add(used, d, mode.keep_f);
        pd.push_back(d);
    }
    return k;
}

// ---- the kernels of a batch --------------------------------------------------------------------------
//   ACX_EF_ROWSTAT2=0   rows of <= 512 cells keep the one-row selection kernel (read once per process)
struct EfSwitches { bool two_rows; };
inline const EfSwitches &ef_switches()
{
    static const EfSwitches s = [] { const char *e = getenv("ACX_EF_ROWSTAT2"); return EfSwitches{!(e && e[0] == '0')}; }();
    return s;
}

// The limits: rows of more than 512 cells take the wide variants (16 values / columns per lane); more than EF_MAXNB: a row no
// longer fits a wave's registers -- the streaming variants (any length).  The row kernels go by the batch's longest side either
// way (they also run on C^T and on the fused matrix), the Smith-Waterman kernels by its longest row.
struct EfBatchKernels {
    int row;        // ACX_EF_ROW_*: the statistics of C (mode 0)
    int row1;       // ... of C^T (mode 1) and of a stored fused matrix (mode 2): always a one-row kernel
    int col;        // ACX_EF_COL_*
    int fuse;       // ACX_EF_FUSE_* (exact or fast arithmetic: the context's setting)
    int sw;         // ACX_EF_SW_*
};
inline EfBatchKernels ef_batch_kernels(int maxM, int maxN, int Kn, const EfMode &mode, bool ext_matrix)
{
    const int longest = std::max(maxM, maxN);
    EfBatchKernels kn;
    kn.row1 = longest > EF_MAXNB ? ACX_EF_ROW_LONG : (longest > 512 ? ACX_EF_ROW_4 : ACX_EF_ROW_2);
    // rows of <= 512 cells: two rows per wave (ef_rowstat2_kernels.hpp)
    kn.row = ef_switches().two_rows && longest <= EF_MAXNB && maxN <= 512 ? ACX_EF_ROW_TWO : kn.row1;
    if (ext_matrix) kn.col = ACX_EF_COL_NONE;
    else if (mode.keep_ct) kn.col = ACX_EF_COL_ROWPASS;
    else kn.col = Kn <= 10 ? ACX_EF_COL_10 : ACX_EF_COL_16;
    if (ext_matrix) kn.fuse = ACX_EF_FUSE_NONE;
    else if (!mode.bits_path) kn.fuse = ACX_EF_FUSE_FLOAT;
    else kn.fuse = longest > 512 ? ACX_EF_FUSE_WIDE : ACX_EF_FUSE_NARROW;
    // (packed 16-bit integers on the bit path: rows of <= 1024 cells keep every score below 10 240 tenths)
    if (mode.bits_path) kn.sw = maxN > 512 ? ACX_EF_SW_H16_16 : ACX_EF_SW_H16_8;
    else kn.sw = maxN > EF_MAXNB ? ACX_EF_SW_LONG : (maxN > 512 ? ACX_EF_SW_16 : ACX_EF_SW_8);
    return kn;
}

// stage 0..3: row statistics, column statistics, fused selection, Smith-Waterman
inline const char *ef_kernel_name(int stage, int kernel)
{
    static const char *const names[4][5] = {
        {"ef_rowstat2_kernel", "ef_rowstat_kernel<2, false>", "ef_rowstat_kernel<4, false>", "ef_rowstat_long_kernel", nullptr},
        {"ef_rowstat_kernel on C^T", "ef_colstat_kernel<10>", "ef_colstat_kernel<16>", "none", nullptr},
        {"ef_rowstat_kernel<2, true>", "ef_rowstat_kernel<4, true>", "ef_fuse_kernel", "none", nullptr},
        {"sw_bits_h16_kernel<8>", "sw_bits_h16_kernel<16>", "sw_kernel<8>", "sw_kernel<16>", "sw_long_kernel"},
    };
    return stage >= 0 && stage < 4 && kernel >= 0 && kernel < 5 ? names[stage][kernel] : nullptr;
}

// ---- run order -----------------------------------------------------------------------------------------
// An arbitrary pair list is processed sorted by (first track, second track): pairs that share a track then fall into the
// same rectangle of the GEMMs (shared operands) and neighbouring pairs read neighbouring memory.  Returns true for a list
// that is sorted already (a grid tile, np.triu_indices ...): it goes through as it is, nothing is filled.  Else
// sorted_pairs[k] = pairs[order[k]], a stable sort.
inline bool ef_pair_before(const int32_t *a, const int32_t *b) { return a[0] != b[0] ? a[0] < b[0] : a[1] < b[1]; }
inline bool ef_in_run_order(const int32_t *pairs, int64_t K)
{
    for (int64_t k = 1; k < K; ++k)
        if (ef_pair_before(pairs + 2 * k, pairs + 2 * k - 2)) return false;
    return true;
}
inline bool ef_run_order(const int32_t *pairs, int64_t K, std::vector<int64_t> &order, std::vector<int32_t> &sorted_pairs)
{
    if (ef_in_run_order(pairs, K)) return true;
    order.resize((size_t)K);
    for (int64_t k = 0; k < K; ++k) order[(size_t)k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return ef_pair_before(pairs + 2 * a, pairs + 2 * b); });
    sorted_pairs.resize((size_t)2 * K);
    for (int64_t k = 0; k < K; ++k) {
        sorted_pairs[(size_t)2 * k] = pairs[2 * order[(size_t)k]];
        sorted_pairs[(size_t)2 * k + 1] = pairs[2 * order[(size_t)k] + 1];
    }
    return false;
}

}  // namespace acx
