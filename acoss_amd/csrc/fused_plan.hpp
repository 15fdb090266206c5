// Fused query shortlists (acx_query_fused_lists), the host side (no device work): the neighbourhood of a query, the pairs
// it costs and where their scores lie, the device memory of one fusion problem, which queries share a chunk and where the
// parts of a chunk's one device block lie.  acx.hip issues the copies and launches; everything here is a pure function of
// its arguments.  FusedProb and fused_pair_index are also read by the kernels of snf_batch_kernels.hpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "query_plan.hpp"

#if defined(__HIPCC__)
#define ACX_FUSED_HD __host__ __device__
#else
#define ACX_FUSED_HD
#endif

namespace acx {

static const int FUSED_MAX_LIST = 1024;                    // list_len: a neighbourhood holds at most 1025 tracks
static const int FUSED_MAX_K = 64;                         // neighbours of the SNF kernels (one wave ranks them)
static const int FUSED_MAX_TYPES = 2, FUSED_MAX_PLANES = 4;
static const int64_t FUSED_CHUNK_PAIRS = (int64_t)1 << 20; // pairs per chunk (the host's pair list stays at 8 MB); one problem always fits
static const int FUSED_CHUNK_PROBLEMS = 4096;              // problems per chunk: the problem index is a grid dimension

// One fusion problem of a chunk as the kernels read it.  Offsets count elements of the chunk's arenas: `mat` doubles into
// the matrix arena, `list` entries into the two list arenas (V doubles, J ints), `pair` pairs into the slab, `tracks` ints
// into the track arena.
struct FusedProb {
    int32_t n;          // tracks of the neighbourhood T
    int32_t qpos;       // position of the query in T
    int64_t mat, list, pair, tracks;
};

// Pairs of a neighbourhood of n tracks: its upper triangle.
ACX_FUSED_HD inline int64_t fused_pairs(int64_t n) { return n * (n - 1) / 2; }

// Where the pair of positions a < b lies in the upper triangle of n tracks, row by row.
ACX_FUSED_HD inline int64_t fused_pair_index(int64_t n, int64_t a, int64_t b) { return a * (2 * n - a - 1) / 2 + (b - a - 1); }

// The matrices of a problem in its part of the matrix arena, n^2 doubles each, M = the most planes of the call's fused
// types:  D_0 .. D_{M-1} | cur_0 .. | nxt_0 .. | acc | ut | md (n doubles).
inline int fused_slot_dist(int /*M*/, int i) { return i; }
inline int fused_slot_cur(int M, int i) { return M + i; }
inline int fused_slot_nxt(int M, int i) { return 2 * M + i; }
inline int fused_slot_acc(int M) { return 3 * M; }
inline int fused_slot_ut(int M) { return 3 * M + 1; }
inline int fused_slot_md(int M) { return 3 * M + 2; }
inline int64_t fused_mat_doubles(int64_t n, int M) { return (3 * (int64_t)M + 2) * n * n + n; }
inline int64_t fused_list_entries(int64_t n, int M, int K) { return (int64_t)M * n * K; }

// T = sorted({q} U valid(row)): row holds L entries, -1 = an empty slot, no track twice (checked by the caller).
inline void fused_neighbourhood(int32_t q, const int32_t *row, int L, std::vector<int32_t> &T)
{
    T.clear();
    T.push_back(q);
    for (int j = 0; j < L; ++j)
        if (row[j] >= 0 && row[j] != q) T.push_back(row[j]);
    std::sort(T.begin(), T.end());
}

// Device bytes of one problem: its pair scores (W planes of f32), matrices, lists, tracks, descriptor and results
// (k indices, k scores and a flag per fused type).
inline int64_t fused_problem_bytes(int64_t n, int W, int M, int K, int n_types, int k)
{
    return fused_pairs(n) * W * 4 + 8 * fused_mat_doubles(n, M) + 12 * fused_list_entries(n, M, K) + 4 * n + (int64_t)sizeof(FusedProb) +
           (int64_t)n_types * (8 * (int64_t)k + 1);
}

// Queries [first, end) per chunk: consecutive queries while their problems fit `half` bytes, FUSED_CHUNK_PAIRS pairs and
// FUSED_CHUNK_PROBLEMS problems.  ns[i]: the size of query i's neighbourhood.  Returns the chunk ends (ascending, the last
// is the number of queries); *unfit = the first query whose problem alone exceeds `half`, -1 if none (then the ends are
// complete).
inline std::vector<int> fused_chunks(const std::vector<int32_t> &ns, int W, int M, int K, int n_types, int k, int64_t half, int *unfit)
{
    std::vector<int> ends;
    *unfit = -1;
    int64_t bytes = 0, pairs = 0;
    int first = 0;
    for (int i = 0; i < (int)ns.size(); ++i) {
        const int64_t b = fused_problem_bytes(ns[i], W, M, K, n_types, k), p = fused_pairs(ns[i]);
        if (b > half) { *unfit = i; return ends; }
        if (i > first && (bytes + b > half || pairs + p > FUSED_CHUNK_PAIRS || i - first >= FUSED_CHUNK_PROBLEMS)) {
            ends.push_back(i);
            first = i; bytes = 0; pairs = 0;
        }
        bytes += b; pairs += p;
    }
    if (!ns.empty()) ends.push_back((int)ns.size());
    return ends;
}

// The descriptors of a chunk's problems: running offsets into the arenas, in the order of the queries.
struct FusedChunk {
    std::vector<FusedProb> probs;
    std::vector<int32_t> tracks;          // the neighbourhoods, one behind the other
    int64_t mat = 0, list = 0, pairs = 0; // arena sizes: doubles, entries, pairs
    int max_n = 0;
};

inline FusedChunk fused_chunk(const int32_t *queries, const int32_t *lists, int L, int first, int end, int M, int K)
{
    FusedChunk ch;
    std::vector<int32_t> T;
    for (int i = first; i < end; ++i) {
        fused_neighbourhood(queries[i], lists + (size_t)i * L, L, T);
        FusedProb p;
        p.n = (int32_t)T.size();
        p.qpos = (int32_t)(std::lower_bound(T.begin(), T.end(), queries[i]) - T.begin());
        p.mat = ch.mat; p.list = ch.list; p.pair = ch.pairs; p.tracks = (int64_t)ch.tracks.size();
        ch.mat += fused_mat_doubles(p.n, M);
        ch.list += fused_list_entries(p.n, M, K);
        ch.pairs += fused_pairs(p.n);
        ch.tracks.insert(ch.tracks.end(), T.begin(), T.end());
        ch.max_n = std::max(ch.max_n, (int)p.n);
        ch.probs.push_back(p);
    }
    return ch;
}

// The pairs of a chunk, (min, max) of every unordered pair of every neighbourhood, and where their scores go in the slab
// (slab[(pair slot) W + e]).  Enumerated grouped by the pair's second track (then its first), as query_list_pairs does:
// neighbouring pairs share a track.  A pair two neighbourhoods hold is computed twice.
inline void fused_chunk_pairs(const FusedChunk &ch, int W, std::vector<int32_t> &pairs, std::vector<int64_t> &idx)
{
    struct Cell { int32_t a, b; int64_t at; };
    std::vector<Cell> cells;
    cells.reserve((size_t)ch.pairs);
    for (const FusedProb &p : ch.probs) {
        const int32_t *T = ch.tracks.data() + p.tracks;
        for (int a = 0; a < p.n; ++a)
            for (int b = a + 1; b < p.n; ++b) cells.push_back({T[a], T[b], (p.pair + fused_pair_index(p.n, a, b)) * W});
    }
    std::sort(cells.begin(), cells.end(), [](const Cell &x, const Cell &y) { return x.b != y.b ? x.b < y.b : x.a != y.a ? x.a < y.a : x.at < y.at; });
    pairs.resize(2 * cells.size()); idx.resize(cells.size());
    for (size_t k = 0; k < cells.size(); ++k) { pairs[2 * k] = cells[k].a; pairs[2 * k + 1] = cells[k].b; idx[k] = cells[k].at; }
}

// A call's one device block, sized for its largest chunk:
// slab | col (doubles; n_col = 0: none) | matrices | V | J | descriptors | tracks | indices | scores | flags
struct FusedLayout { size_t slab, col, mat, V, J, probs, tracks, idx, score, flag, total; };

inline FusedLayout fused_layout(size_t slab_floats, size_t n_col, size_t mat_doubles, size_t list_entries, size_t n_probs, size_t n_tracks, size_t res,
                                size_t n_flags)
{
    BlockLayout b;
    return {b.take(4 * slab_floats, 4), b.take(8 * n_col, 8), b.take(8 * mat_doubles, 8), b.take(8 * list_entries, 8), b.take(4 * list_entries, 4),
            b.take(sizeof(FusedProb) * n_probs, 8), b.take(4 * n_tracks, 4), b.take(4 * res, 4), b.take(4 * res, 4), b.take(n_flags, 1), b.total()};
}

}  // namespace acx
