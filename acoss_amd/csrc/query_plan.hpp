// Query bands, the host side (no device work): how many query rows a band holds, where the parts of a call's one
// device block lie, which pairs a band holds, in which order, and where each score goes in the slab.  acx.hip issues
// the copies and launches; everything here is a pure function of its arguments.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/acx.h"

namespace acx {

// Dense bands hold at most QUERY_BAND_ROWS rows: with EarlyFusion a band x 128 collection tracks is then one dense
// rectangle.  A list band is not capped by rows -- with lists of a few hundred entries that would hand Serra09 a fraction
// of one 65535-pair batch per band -- but by QUERY_LIST_BAND_CELLS cells: four full Serra09 batches, so that the two
// result slots of run_serra09 overlap within a band, while the host's pair list and destinations of a band stay at 4 MB.
// A design parameter: no measurement rests on it.
static const int QUERY_BAND_ROWS = 128;
static const int64_t QUERY_LIST_BAND_CELLS = (int64_t)1 << 18;

inline int64_t query_list_band_cap(int L) { return std::max<int64_t>(1, QUERY_LIST_BAND_CELLS / std::max(L, 1)); }

// Rows per band: `per_row` bytes of device memory per query row within `half` (half of the scratch limit), at most
// `cap` rows.  0: not even one row fits.
inline int query_band_rows(int n_queries, int64_t per_row, int64_t half, int64_t cap)
{
    if (half < per_row) return 0;
    return (int)std::min(std::min<int64_t>(n_queries, cap), half / per_row);
}

// The parts of one device block, in the order they are taken: byte offsets, every part at a multiple of its alignment.
struct BlockLayout {
    size_t end = 0;
    size_t take(size_t bytes, size_t align)
    {
        const size_t at = (end + align - 1) / align * align;
        end = at + bytes;
        return at;
    }
    size_t total() const { return end; }
};

// Every call's block begins slab | col (doubles; n_col = 0: none) | queries, then its own parts.  A part is aligned to
// its element size; the padding is not part of `per_row`, so it moves no band size and no refusal.  (The layouts below
// are braced lists: their parts are taken left to right.)
struct QueryHead { size_t slab, col, queries; };

inline QueryHead query_head(BlockLayout &b, size_t slab_floats, size_t n_col, size_t n_queries)
{
    return {b.take(4 * slab_floats, 4), b.take(8 * n_col, 8), b.take(4 * n_queries, 4)};
}

// acx_query_scores: ... | the band's finished rows
struct QueryScoresLayout { QueryHead head; size_t fin, total; };

inline QueryScoresLayout query_scores_layout(size_t slab_floats, size_t n_col, size_t n_queries)
{
    BlockLayout b;
    return {query_head(b, slab_floats, n_col, n_queries), b.take(4 * slab_floats, 4), b.total()};
}

// acx_query_topk / acx_query_topk_lists: ... | candidates or lists (n_list ints) | the band's `res` indices | its scores
struct QueryTopkLayout { QueryHead head; size_t list, idx, score, total; };

inline QueryTopkLayout query_topk_layout(size_t slab_floats, size_t n_col, size_t n_queries, size_t n_list, size_t res)
{
    BlockLayout b;
    return {query_head(b, slab_floats, n_col, n_queries), b.take(4 * n_list, 4), b.take(4 * res, 4), b.take(4 * res, 4), b.total()};
}

// acx_query_ranks: ... | moff (n_queries + 1) | mates | posn (n_posn = 0: none) | the band's positions | its flags
struct QueryRanksLayout { QueryHead head; size_t moff, mates, posn, pos, flag, total; };

inline QueryRanksLayout query_ranks_layout(size_t slab_floats, size_t n_col, size_t n_queries, size_t n_mates, size_t n_posn, size_t n_pos,
                                           size_t n_flag)
{
    BlockLayout b;
    return {query_head(b, slab_floats, n_col, n_queries), b.take(8 * (n_queries + 1), 8), b.take(4 * n_mates, 4), b.take(4 * n_posn, 4),
            b.take(4 * n_pos, 4), b.take(n_flag, 1), b.total()};
}

// The pairs of a band (queries q[0 .. nr) x the columns) and where their scores go in the slab.  Columns come in
// blocks of 128, so that an EarlyFusion rectangle is one block x the band.  Pass 0: the cells computed as (query,
// column) -- all of an ordered band, the columns above the query of a symmetric one --, column by column: neighbouring
// pairs share their second track (what simple_kernel wants).  Pass 1 (symmetric): the cells computed as (column,
// query), query by query.  A query's own column is left out.
inline void query_band_pairs(const int32_t *q, int nr, const int32_t *cols, int ncols, int n, int w, int symmetric,
                             std::vector<int32_t> &pairs, std::vector<int64_t> &idx)
{
    pairs.clear(); idx.clear();
    const int CB = 128;
    for (int j0 = 0; j0 < ncols; j0 += CB) {
        const int j1 = std::min(ncols, j0 + CB);
        for (int j = j0; j < j1; ++j) {
            const int col = cols ? cols[j] : j;
            for (int r = 0; r < nr; ++r) {
                if (col == q[r] || (symmetric && col < q[r])) continue;
                pairs.push_back(q[r]); pairs.push_back(col);
                idx.push_back(((int64_t)r * n + col) * w);
            }
        }
        if (!symmetric) continue;
        for (int r = 0; r < nr; ++r)
            for (int j = j0; j < j1; ++j) {
                const int col = cols ? cols[j] : j;
                if (col >= q[r]) break;
                pairs.push_back(col); pairs.push_back(q[r]);
                idx.push_back(((int64_t)r * n + col) * w);
            }
    }
}

// The cells of a list band -- rows q[0 .. nr) with their lists -- as pairs and slab destinations.  Cell (r, j) with
// c = lists[r][j], c >= 0, c != q[r] is the pair (min, max) of a symmetric call, (q, c) of an ordered one; a pair two rows
// want is computed twice.  The cells are enumerated grouped by the pair's second track (then by its first): neighbouring
// pairs share a track (what simple_kernel wants), and the queries of one work share shortlist entries.  No pair kernel's
// score depends on its place in the list.
inline void query_list_pairs(const int32_t *q, int nr, const int32_t *lists, int L, int w, int symmetric, std::vector<int32_t> &pairs,
                             std::vector<int64_t> &idx)
{
    struct Cell { int32_t a, b; int64_t at; };
    std::vector<Cell> cells;
    for (int r = 0; r < nr; ++r)
        for (int j = 0; j < L; ++j) {
            const int32_t cnd = lists[(size_t)r * L + j];
            if (cnd < 0 || cnd == q[r]) continue;
            const bool swap = symmetric && cnd < q[r];
            cells.push_back({swap ? cnd : q[r], swap ? q[r] : cnd, ((int64_t)r * L + j) * w});
        }
    std::sort(cells.begin(), cells.end(), [](const Cell &x, const Cell &y) {
        return x.b != y.b ? x.b < y.b : x.a != y.a ? x.a < y.a : x.at < y.at;
    });
    pairs.resize(2 * cells.size()); idx.resize(cells.size());
    for (size_t k = 0; k < cells.size(); ++k) { pairs[2 * k] = cells[k].a; pairs[2 * k + 1] = cells[k].b; idx[k] = cells[k].at; }
}

// FTM2D: the band as tiles of the tile kernel -- per query row and run of consecutive columns, the columns above the
// query as a 1 x cols tile (query, column); those below it as a rows x 1 tile (column, query) when symmetric, as a
// second 1 x cols tile otherwise.  A tile's scores are rows x cols floats at its offset: both shapes fill the slab row.
inline std::vector<acx_grid_tile> query_ftm2d_band_tiles(const int32_t *q, int nr, const int32_t *cols, int ncols, int n, int symmetric)
{
    std::vector<acx_grid_tile> tiles;
    auto add = [&](int r, int a, int b) {             // columns [a, b) of slab row r, none of them the query
        if (a >= b) return;
        acx_grid_tile t;
        t.rank = 0; t.diagonal = 0; t.cost = 0.0;
        t.offset = (int64_t)r * n + a;
        if (symmetric && b <= q[r]) { t.row0 = a; t.rows = b - a; t.col0 = q[r]; t.cols = 1; }
        else { t.row0 = q[r]; t.rows = 1; t.col0 = a; t.cols = b - a; }
        tiles.push_back(t);
    };
    for (int j0 = 0; j0 < ncols;) {
        int j1 = j0 + 1;
        const int a = cols ? cols[j0] : 0;
        if (cols) { while (j1 < ncols && cols[j1] == cols[j1 - 1] + 1) ++j1; } else j1 = ncols;
        const int b = a + (j1 - j0);
        for (int r = 0; r < nr; ++r) {
            add(r, a, std::min(b, q[r]));
            add(r, std::max(a, q[r] + 1), b);
        }
        j0 = j1;
    }
    return tiles;
}

}  // namespace acx
