// The Serra09 batch plan (host code, no device work): how a pair list is sized, packed into scratch-sized batches,
// sorted by size class, and which band and sweep kernel each class runs.  A pure function of (pooled track lengths,
// pair list, parameters, scratch limit, the three per-process switches): run_serra09_impl (acx.hip) follows it,
// launch_band_kernel (acx_band.hip) switches on its answer, and acx_serra09_plan reports it without a device, which is
// what tests/test_serra09_shapes_design.py and tests/test_serra09_plan.py read.  A class limit or a kernel choice is
// changed HERE and nowhere else.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/acx.h"
#include "serra09_kernels.hpp"      // PairDesc, pct_position, BAND, MAX_M (the struct the kernels read: its layout lives with them)

namespace acx {

// Tiles of 64 columns in the band of a row of M cells: the band kernels sweep BAND = 8 rows whose diagonals start
// up to 7 columns left of the matrix, so 64 n tiles hold rows of up to 64 n - 7 cells.
inline int serra09_tiles(int M) { return (M + BAND - 1 + 63) / 64; }

inline int64_t serra09_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// Number of embedded frames of a track of T pooled frames (oracle embed_len): the stack at base
// frame i = 0, tau, 2 tau, ... holds frames i, i + tau, ..., i + (m - 1) tau.
inline int serra09_embed_len(int T, int m, int tau, int embed_full)
{
    const int span = embed_full ? (m - 1) * tau : m * tau;
    const int L = T - span;
    if (L <= 0) return 0;
    return (L + tau - 1) / tau;
}

// ---- size classes ----------------------------------------------------------------------
// A pass whose rows hold <= 249 / 505 / 761 / 1017 / 2041 cells (4 / 8 / 12 / 16 / 32 tiles) runs the band kernel that fits:
// band2_kernel with four rows per wave, with two rows per wave at 16 / 24 positions per lane (stack sizes m <= 9 only),
// band_kernel with 8 / 16 / 32 values per lane.  The alignment sweep behind the row pass gives a lane 8 / 8 / 16 / 16 / 32
// bitmap columns and, for the default penalties, packs four / two pairs of the two narrow classes into a wave.
// Class NC: a side beyond the last limit, or m > MAX_M -- the streaming kernels (serra09_long_kernels.hpp).
constexpr int SERRA09_NC = 5;
struct Serra09Class {
    int tiles;                         // the class holds rows of up to this many tiles
    int band_m9, band_m10, band_f16;   // ACX_SERRA09_FAMILY_*: exact arithmetic m <= 9 / m >= 10, the f16x2 Gram (m = 9)
    int cols, pack;                    // the sweep: bitmap columns per lane, pairs per wave (default penalties)
};
constexpr Serra09Class SERRA09_CLASS[SERRA09_NC] = {
    {4, ACX_SERRA09_FAMILY_BAND2_4ROWS, ACX_SERRA09_FAMILY_BAND_2, ACX_SERRA09_FAMILY_BAND_2, 8, 4},
    {8, ACX_SERRA09_FAMILY_BAND2_2ROWS, ACX_SERRA09_FAMILY_BAND_2, ACX_SERRA09_FAMILY_BAND_2, 8, 2},
    {12, ACX_SERRA09_FAMILY_BAND2_MID, ACX_SERRA09_FAMILY_BAND_4, ACX_SERRA09_FAMILY_BAND_4, 16, 1},
    {16, ACX_SERRA09_FAMILY_BAND_4, ACX_SERRA09_FAMILY_BAND_4, ACX_SERRA09_FAMILY_BAND_4, 16, 1},
    {32, ACX_SERRA09_FAMILY_BAND_8, ACX_SERRA09_FAMILY_BAND_8, ACX_SERRA09_FAMILY_BAND_8, 32, 1},
};

// class of a row of M cells by its length alone (the stack size is the caller's: serra09_pair_key)
inline int serra09_row_class(int M)
{
    const int nd = serra09_tiles(M);
    int cl = 0;
    while (cl < SERRA09_NC && nd > SERRA09_CLASS[cl].tiles) ++cl;
    return cl;
}

// ---- the per-process switches (A/B aids; read once) ---------------------------------------
//   ACX_BAND2=2 | 1 | 0   peel the band2 classes off one by one: the four-row class onto the two-row kernel; also the
//                         24-position class onto band_kernel<M, 4>; also the two-row classes onto band_kernel<M, 2>
//   ACX_QMAX_MULTI=0      one wave per pair in every sweep
//   ACX_QMAX_STREAM=0     the sweeps run on the main stream
//   ACX_PLANES=0          the wide class reads its column operands from the rotated pool: no per-rotation planes (576 B per frame)
struct Serra09Switches {
    int band2;          // band2 classes kept: 3 (default) .. 0
    bool multi, qstream, planes;
};
inline const Serra09Switches &serra09_switches()
{
    static const Serra09Switches s = [] {
        auto off = [](const char *name) { const char *e = getenv(name); return e && e[0] == '0'; };
        const char *b = getenv("ACX_BAND2");
        return Serra09Switches{(b && b[0] >= '0' && b[0] <= '2') ? b[0] - '0' : 3, !off("ACX_QMAX_MULTI"), !off("ACX_QMAX_STREAM"), !off("ACX_PLANES")};
    }();
    return s;
}

// the band kernel of a pass whose longest row is of class cl (< NC)
inline int serra09_band_family(int cl, int m, int arith)
{
    const Serra09Class &c = SERRA09_CLASS[cl];
    if (arith == ACX_ARITH_F16X2) return c.band_f16;
    if (m > 9) return c.band_m10;
    const int keep = serra09_switches().band2;
    switch (c.band_m9) {
    case ACX_SERRA09_FAMILY_BAND2_4ROWS: return keep >= 3 ? c.band_m9 : (keep >= 1 ? ACX_SERRA09_FAMILY_BAND2_2ROWS : ACX_SERRA09_FAMILY_BAND_2);
    case ACX_SERRA09_FAMILY_BAND2_2ROWS: return keep >= 1 ? c.band_m9 : ACX_SERRA09_FAMILY_BAND_2;
    case ACX_SERRA09_FAMILY_BAND2_MID: return keep >= 2 ? c.band_m9 : ACX_SERRA09_FAMILY_BAND_4;
    default: return c.band_m9;
    }
}

// the sweep of class cl: columns per lane (0: the streaming sweep, any length) and pairs per wave
struct Serra09Sweep { int cols, pack; };
inline Serra09Sweep serra09_sweep(int cl)
{
    if (cl >= SERRA09_NC) return Serra09Sweep{0, 1};
    return Serra09Sweep{SERRA09_CLASS[cl].cols, serra09_switches().multi ? SERRA09_CLASS[cl].pack : 1};
}

inline const char *serra09_family_name(int family, int m)
{
    const bool lo = m <= 9;
    switch (family) {
    case ACX_SERRA09_FAMILY_BAND2_4ROWS: return "band2_kernel<M, B2_NV, 16>";
    case ACX_SERRA09_FAMILY_BAND2_2ROWS: return "band2_kernel<M, B2_NV, 32>";
    case ACX_SERRA09_FAMILY_BAND2_MID: return "band2_kernel<M, B2_NV_MID, 32>";
    case ACX_SERRA09_FAMILY_BAND_2: return lo ? "band_kernel<M<=9, 2>" : "band_kernel<M>=10, 2>";
    case ACX_SERRA09_FAMILY_BAND_4: return lo ? "band_kernel<M<=9, 4>" : "band_kernel<M>=10, 4>";
    case ACX_SERRA09_FAMILY_BAND_8: return lo ? "band_kernel<M<=9, 8>" : "band_kernel<M>=10, 8>";
    case ACX_SERRA09_FAMILY_STREAMING: return "csm_long_kernel + rowsel_long_kernel";
    default: return nullptr;
    }
}

// ---- pair sizing -------------------------------------------------------------------------
// Pooled lengths as the run sees them: the uploaded pool's offsets decimated by the stack stride tau (ensure_tau), i.e.
// ceil(T / tau) frames; tau = 1 over the decimated pool's own offsets gives the same.  (serra09_one_batch and the report
// ask before any pool has been decimated.)
struct Serra09Lengths {
    const int64_t *off;
    int32_t n_tracks;
    int tau;
    int operator()(int t) const
    {
        const int64_t T = off[t + 1] - off[t];
        return (int)(tau == 1 ? T : (T + tau - 1) / tau);
    }
};

// What a pair takes of the three arenas.  The band pipeline keeps D2 out of HBM: only the debug entry point (dbg) makes a
// band-class pair need it; a streaming pair needs D2, D2^T and the DP's strip records (2 x 4 floats per row).
struct Serra09Need {
    int64_t D, L;       // floats of the scratch arena: D2; D2^T + strip records
    int64_t bits;       // u64 words of the bitmap arena (Mq rows x nw words)
    int64_t thr;        // floats of the threshold arena (the thresholds and eps of every row and column: PairDesc::offX)
    int64_t floats() const { return D + L + 2 * bits; }      // against the scratch limit: a bitmap word counts as two floats
};

// The descriptor of pair (qi, ri) but for its arena offsets, and its needs.  ACX_ERR_INVALID: an index out of range;
// ACX_ERR_SHORT: a track shorter than the delay-embedding stack.  `p`: its tau is the Lengths', the embedding here has stride 1.
inline int serra09_size_pair(const Serra09Lengths &len, int qi, int ri, const acx_serra09_params &p, bool dbg, PairDesc &d, Serra09Need &need)
{
    if (qi < 0 || ri < 0 || qi >= len.n_tracks || ri >= len.n_tracks) return ACX_ERR_INVALID;
    d.q = qi; d.r = ri;
    d.Tq = len(qi);
    d.Tr = len(ri);
    d.Mq = serra09_embed_len(d.Tq, p.m, 1, p.embed_full);
    d.Mr = serra09_embed_len(d.Tr, p.m, 1, p.embed_full);
    if (d.Mq <= 0 || d.Mr <= 0) return ACX_ERR_SHORT;
    d.oti = 0;
    d.pitchD = (int32_t)serra09_round_up(d.Mr, 64);
    d.pitchT = (int32_t)serra09_round_up(d.Mq, 64);
    d.nw = serra09_tiles(d.Mr);
    d.pos_q = pct_position(d.Mq, p.kappa, p.pct_mode);
    d.pos_r = pct_position(d.Mr, p.kappa, p.pct_mode);
    const bool is_long = p.m > MAX_M || serra09_row_class(std::max(d.Mq, d.Mr)) == SERRA09_NC;
    need.D = (dbg || is_long) ? (int64_t)d.Mq * d.pitchD : 0;
    need.L = is_long ? (int64_t)d.Mr * d.pitchT + 8 * (int64_t)d.Mq : 0;
    need.bits = (int64_t)d.Mq * d.nw;
    need.thr = 3 * ((int64_t)d.pitchD + d.pitchT);
    return ACX_OK;
}

// The whole list before the first launch: the first pair the run refuses (its position to *bad) and the code for it --
// an index, a short track, or a pair that does not fit the scratch limit on its own (ACX_ERR_NOMEM).
inline int serra09_check_pairs(const Serra09Lengths &len, const int32_t *pairs, int64_t K, const acx_serra09_params &p, bool dbg,
                               int64_t limit_floats, int64_t *bad)
{
    PairDesc d;
    Serra09Need need;
    for (int64_t k = 0; k < K; ++k) {
        int rc = serra09_size_pair(len, pairs[2 * k], pairs[2 * k + 1], p, dbg, d, need);
        if (rc == ACX_OK && need.floats() > limit_floats) rc = ACX_ERR_NOMEM;
        if (rc != ACX_OK) { *bad = k; return rc; }
    }
    return ACX_OK;
}

// ---- batches -------------------------------------------------------------------------------
struct Serra09Arena { int64_t scratch = 0, bits = 0, thr = 0; };      // floats, u64 words, floats in use

// The batch that starts at pair k0 of a CHECKED list: greedily as many pairs as fit -- at most 65535 (a grid dimension),
// and scratch floats + 2 x bitmap words within the limit.  Fills `pd` with their descriptors, arena offsets included, in
// list order, `used` with the arenas' extents, and returns the end of the batch (k0: the list was not checked).
inline int64_t serra09_pack_batch(const Serra09Lengths &len, const int32_t *pairs, int64_t k0, int64_t K, const acx_serra09_params &p,
                                  bool dbg, int64_t limit_floats, std::vector<PairDesc> &pd, Serra09Arena &used)
{
    pd.clear();
    used = Serra09Arena();
    int64_t k = k0;
    for (; k < K && pd.size() < 65535; ++k) {
        PairDesc d;
        Serra09Need need;
        if (serra09_size_pair(len, pairs[2 * k], pairs[2 * k + 1], p, dbg, d, need) != ACX_OK) break;
        if (used.scratch + need.D + need.L + 2 * (used.bits + need.bits) > limit_floats) break;
        d.offD = used.scratch;
        d.offL = used.scratch + need.D;
        d.offT = used.bits;
        d.offX = used.thr;
        used.scratch += need.D + need.L;
        used.bits += need.bits;
        used.thr += need.thr;
        pd.push_back(d);
    }
    return k;
}

// Pairs are processed in size classes PER PASS.  The row pass (and the alignment sweep behind it) has rows of Mr cells, the
// column pass rows of Mq cells, so a pair carries two classes (cr, cq) and the batch is sorted by the key NC cr + cq: the row
// pass and the sweep take the NC keys of one cr in ONE launch, the column pass one launch per key -- a short track paired
// with a long one does not drag BOTH passes through the wider kernel.  Key NC * NC: the streaming class, last.
constexpr int SERRA09_NKEY = SERRA09_NC * SERRA09_NC + 1;
inline int serra09_pair_key(const PairDesc &d, int m)
{
    const int cr = serra09_row_class(d.Mr), cq = serra09_row_class(d.Mq);
    return (m > MAX_M || cr == SERRA09_NC || cq == SERRA09_NC) ? SERRA09_NC * SERRA09_NC : SERRA09_NC * cr + cq;
}

struct Serra09Sort {
    int key_begin[SERRA09_NKEY + 1];        // sorted pairs [key_begin[k], key_begin[k + 1]) have key k
    int cls_begin[SERRA09_NC + 2];          // ... [cls_begin[cl], cls_begin[cl + 1]) row class cl; cl = NC: the streaming class
};

// Counting sort of a batch by key, stable; `perm[k]` = position in the batch of sorted pair k.  `tmp`: a vector to sort through.
inline Serra09Sort serra09_sort_batch(std::vector<PairDesc> &pd, std::vector<PairDesc> &tmp, std::vector<int> &perm, int m)
{
    const int B = (int)pd.size();
    Serra09Sort s;
    int fill[SERRA09_NKEY];
    for (int kk = 0; kk < SERRA09_NKEY; ++kk) fill[kk] = 0;
    for (const PairDesc &d : pd) fill[serra09_pair_key(d, m)]++;
    s.key_begin[0] = 0;
    for (int kk = 0; kk < SERRA09_NKEY; ++kk) s.key_begin[kk + 1] = s.key_begin[kk] + fill[kk];
    for (int kk = 0; kk < SERRA09_NKEY; ++kk) fill[kk] = s.key_begin[kk];
    perm.resize(B);
    tmp.resize(B);
    for (int k2 = 0; k2 < B; ++k2) {
        const int kk = serra09_pair_key(pd[k2], m);
        perm[fill[kk]] = k2;
        tmp[fill[kk]++] = pd[k2];
    }
    pd.swap(tmp);
    for (int cl = 0; cl <= SERRA09_NC; ++cl) s.cls_begin[cl] = s.key_begin[SERRA09_NC * cl];
    s.cls_begin[SERRA09_NC + 1] = B;
    return s;
}

// ---- the product-path tail -------------------------------------------------------------------
// band_kernel<M, 8> has a second copy of its row tail (band_row_tail's FAST flag, serra09_kernels.hpp) in which everything the
// host knows about a pass is a constant.  It is taken when ALL of this holds: the wide class of the exact arithmetic; pct_mode 0 (the
// interpolating percentile) with the inclusive comparison; no eps and no D2 wanted (the debug entry point wants both); the row pass
// writes a bitmap; and for every row length n of the launch, i.e. for every pair of it: the position falls strictly between two
// ranks (ihi == ilo + 1) with both interpolation weights at least 2^-8 and at least one full rank below (band_row_tail's
// `weights_ok`), and the pivot-filtered selection applies ((ihi + 2) * 9 <= n: its `use_pivot`).  A length whose position is an
// integer ((n - 1) kappa: every 200th length at the default 0.095) does not qualify; serra09_fast_tail_runs cuts the pass around it.
inline bool serra09_fast_tail_row(const PctPos &pp, int n)
{
    return pp.ihi == pp.ilo + 1 && pp.fl >= 1.0f && (pp.ce - pp.kf) >= 0.00390625f && (pp.kf - pp.fl) >= 0.00390625f && (pp.ihi + 2) * 9 <= n;
}
// (role 1: the column pass, rows of Mq cells; role 0: the row pass, rows of Mr cells, `have_bits`: it writes the bitmap)
inline bool serra09_fast_tail_params(const acx_serra09_params &p, int family, int role, bool write_d2, bool want_eps, bool have_bits)
{
    return family == ACX_SERRA09_FAMILY_BAND_8 && p.arith == ACX_ARITH_EXACT && p.pct_mode == 0 && p.inclusive != 0 && !write_d2 && !want_eps &&
           (role != 0 || have_bits);
}
// One band pass over sorted pairs [b0, b1) as launches: maximal runs of neighbouring pairs that all qualify (fast) or all do not, so
// that a pair of an odd length sends only its own run through the generic copy, not the whole class.  Pairs are independent (one
// grid row each), so the cut changes no result.  More than 2 + B / 32 runs (lengths that alternate): one generic launch, as before.
struct Serra09Run { int begin, end; bool fast; };
inline std::vector<Serra09Run> serra09_fast_tail_runs(const acx_serra09_params &p, int family, int role, bool write_d2, bool want_eps,
                                                       bool have_bits, const std::vector<PairDesc> &pd, int b0, int b1)
{
    std::vector<Serra09Run> runs;
    if (b1 <= b0) return runs;
    if (!serra09_fast_tail_params(p, family, role, write_d2, want_eps, have_bits)) return {Serra09Run{b0, b1, false}};
    auto ok = [&](int k2) { return role ? serra09_fast_tail_row(pd[k2].pos_q, pd[k2].Mq) : serra09_fast_tail_row(pd[k2].pos_r, pd[k2].Mr); };
    for (int k2 = b0; k2 < b1; ++k2) {
        const bool f = ok(k2);
        if (!runs.empty() && runs.back().fast == f) runs.back().end = k2 + 1;
        else runs.push_back(Serra09Run{k2, k2 + 1, f});
    }
    if ((int)runs.size() > 2 + (b1 - b0) / 32) return {Serra09Run{b0, b1, false}};
    return runs;
}

// what one launch over sorted pairs [b0, b1) spans: the longest side each way (its grid) and the cells (its profile record)
struct Serra09Extent { int Mq = 0, Mr = 0; int64_t cells = 0; };
inline Serra09Extent serra09_extent(const std::vector<PairDesc> &pd, int b0, int b1)
{
    Serra09Extent e;
    for (int k2 = b0; k2 < b1; ++k2) {
        e.Mq = std::max(e.Mq, pd[k2].Mq); e.Mr = std::max(e.Mr, pd[k2].Mr);
        e.cells += (int64_t)pd[k2].Mq * pd[k2].Mr;
    }
    return e;
}

}  // namespace acx
