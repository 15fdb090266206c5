// Host-only checks of acoss_amd/csrc/query_plan.hpp (tests/test_query_plan_host.py builds this with the address and
// undefined-behaviour sanitizers and runs it): block layouts, the pairs and destinations of dense and list bands, the
// FTM2D band tiles and the rows per band.  Every expectation is written out here or derived from the rules in the
// header's comments, none from the functions under test.  Exit status 0: every check held.
#include <cstdio>
#include <map>
#include <tuple>
#include <utility>
#include <vector>

#include "../acoss_amd/csrc/query_plan.hpp"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

struct Part { size_t at, bytes, align; };

// every part at a multiple of its alignment, no two overlapping, the first (the slab) at 0, sum <= total <= sum + 7 per part
static void check_parts(const std::vector<Part> &parts, size_t total)
{
    size_t sum = 0;
    CHECK(parts[0].at == 0);
    for (size_t i = 0; i < parts.size(); ++i) {
        CHECK(parts[i].at % parts[i].align == 0);
        CHECK(parts[i].at + parts[i].bytes <= total);
        sum += parts[i].bytes;
        for (size_t j = 0; j < i; ++j)
            if (parts[i].bytes > 0 && parts[j].bytes > 0)
                CHECK(parts[i].at + parts[i].bytes <= parts[j].at || parts[j].at + parts[j].bytes <= parts[i].at);
    }
    CHECK(total >= sum && total <= sum + 7 * parts.size());
}

static std::vector<Part> head_parts(const acx::QueryHead &h, size_t slab_floats, size_t n_col, size_t nq)
{
    return {{h.slab, 4 * slab_floats, 4}, {h.col, 8 * n_col, 8}, {h.queries, 4 * nq, 4}};
}

static void check_layouts()
{
    acx::BlockLayout b;
    CHECK(b.take(5, 1) == 0 && b.take(8, 8) == 8 && b.take(0, 4) == 16 && b.take(3, 4) == 16 && b.take(1, 1) == 19 && b.total() == 20);
    // SiMPle's 23 tracks, one row, one plane: 92 bytes of slab, the doubles start at 96
    CHECK(acx::query_topk_layout(23, 23, 5, 0, 10).head.col == 96);
    for (size_t R : {1, 3, 128})
        for (size_t n : {23, 37, 300})
            for (size_t w : {1, 2, 4})
                for (size_t nq : {1, 3, 5})
                    for (size_t n_col : {(size_t)0, n}) {
                        const size_t slab = R * n * w;
                        const acx::QueryScoresLayout s = acx::query_scores_layout(slab, n_col, nq);
                        std::vector<Part> p = head_parts(s.head, slab, n_col, nq);
                        p.push_back({s.fin, 4 * slab, 4});
                        check_parts(p, s.total);
                        for (size_t k : {1, 7}) {
                            const size_t res = R * w * k;
                            for (size_t n_cands : {0, 3}) {       // acx_query_topk: no candidates (or an empty list), three
                                const acx::QueryTopkLayout t = acx::query_topk_layout(slab, n_col, nq, n_cands, res);
                                p = head_parts(t.head, slab, n_col, nq);
                                p.push_back({t.list, 4 * n_cands, 4}); p.push_back({t.idx, 4 * res, 4}); p.push_back({t.score, 4 * res, 4});
                                check_parts(p, t.total);
                            }
                            for (size_t L : {0, 5}) {             // acx_query_topk_lists: the slab is R x L x planes
                                const acx::QueryTopkLayout t = acx::query_topk_layout(R * L * w, n_col, nq, nq * L, res);
                                p = head_parts(t.head, R * L * w, n_col, nq);
                                p.push_back({t.list, 4 * nq * L, 4}); p.push_back({t.idx, 4 * res, 4}); p.push_back({t.score, 4 * res, 4});
                                check_parts(p, t.total);
                            }
                        }
                        for (size_t M : {0, 5})
                            for (size_t n_posn : {(size_t)0, n}) {
                                const acx::QueryRanksLayout r = acx::query_ranks_layout(slab, n_col, nq, M, n_posn, w * M, R * w);
                                p = head_parts(r.head, slab, n_col, nq);
                                p.push_back({r.moff, 8 * (nq + 1), 8}); p.push_back({r.mates, 4 * M, 4}); p.push_back({r.posn, 4 * n_posn, 4});
                                p.push_back({r.pos, 4 * w * M, 4}); p.push_back({r.flag, R * w, 1});
                                check_parts(p, r.total);
                            }
                    }
}

typedef std::vector<std::tuple<int, int, int64_t>> Seq;      // (first, second, destination)

static Seq seq_of(const std::vector<int32_t> &pairs, const std::vector<int64_t> &idx)
{
    Seq s;
    CHECK(pairs.size() == 2 * idx.size());
    for (size_t k = 0; k < idx.size() && 2 * k + 1 < pairs.size(); ++k) s.push_back(std::make_tuple(pairs[2 * k], pairs[2 * k + 1], idx[k]));
    return s;
}

static void check_band_pairs()
{
    std::vector<int32_t> pairs = {9, 9};                     // (whatever they held is gone)
    std::vector<int64_t> idx = {1};
    const int32_t q[2] = {3, 1};
    // n = 5, two planes, all columns.  Symmetric: pass 0 column by column holds the columns above each query -- column 2:
    // (1, 2); column 3: (1, 3); column 4: (3, 4), (1, 4) --, pass 1 query by query the columns below it -- 3: 0, 1, 2; 1: 0.
    acx::query_band_pairs(q, 2, nullptr, 5, 5, 2, 1, pairs, idx);
    const Seq sym = {{1, 2, 14}, {1, 3, 16}, {3, 4, 8}, {1, 4, 18}, {0, 3, 0}, {1, 3, 2}, {2, 3, 4}, {0, 1, 10}};
    CHECK(seq_of(pairs, idx) == sym);
    // Ordered: every column but the query's own, column by column, the queries in their order
    acx::query_band_pairs(q, 2, nullptr, 5, 5, 2, 0, pairs, idx);
    const Seq ord = {{3, 0, 0}, {1, 0, 10}, {3, 1, 2}, {3, 2, 4}, {1, 2, 14}, {1, 3, 16}, {3, 4, 8}, {1, 4, 18}};
    CHECK(seq_of(pairs, idx) == ord);
    // 130 candidates of 200 tracks (0 .. 59 and 130 .. 199): the second block of 128 columns holds two
    const int n = 200, w = 4;
    std::vector<int32_t> cols;
    for (int j = 0; j < 130; ++j) cols.push_back(j < 60 ? j : j + 70);
    const int32_t qs[5] = {150, 0, 199, 59, 100};           // in either run, at both ends, and outside the candidates
    for (int symmetric = 0; symmetric < 2; ++symmetric) {
        acx::query_band_pairs(qs, 5, cols.data(), 130, n, w, symmetric, pairs, idx);
        std::map<int64_t, int> seen;
        int block = 0;
        for (const auto &t : seq_of(pairs, idx)) {
            const int64_t at = std::get<2>(t);
            CHECK(at % w == 0 && at >= 0 && at < (int64_t)5 * n * w);
            const int r = (int)(at / w / n), col = (int)(at / w % n);
            ++seen[at];
            CHECK((col < 60 ? col : col - 70) / 128 >= block);      // both passes of a block of 128 columns before the next block
            block = (col < 60 ? col : col - 70) / 128;
            if (r < 0 || r >= 5) continue;
            const int a = symmetric ? std::min(qs[r], col) : qs[r], b = symmetric ? std::max(qs[r], col) : col;
            CHECK(std::get<0>(t) == a && std::get<1>(t) == b);
        }
        size_t want = 0;
        for (int r = 0; r < 5; ++r)
            for (int32_t col : cols) {
                if (col == qs[r]) continue;
                ++want;
                CHECK(seen[((int64_t)r * n + col) * w] == 1);
            }
        CHECK(idx.size() == want && seen.size() == want);
    }
}

static void check_list_pairs()
{
    const int L = 4, w = 2;
    const int32_t q[3] = {4, 2, 7};
    // -1 entries, row 0 lists its own track, track 7 is listed by rows 0 and 1, rows 0 and 2 list each other
    const int32_t lists[12] = {7, -1, 4, 1, /**/ 7, 5, -1, 0, /**/ 2, 4, 9, -1};
    std::vector<int32_t> pairs;
    std::vector<int64_t> idx;
    for (int symmetric = 0; symmetric < 2; ++symmetric) {
        acx::query_list_pairs(q, 3, lists, L, w, symmetric, pairs, idx);
        const Seq s = seq_of(pairs, idx);
        std::map<int64_t, int> seen;
        int both = 0;
        for (size_t k = 0; k < s.size(); ++k) {
            const int64_t at = std::get<2>(s[k]);
            CHECK(at % w == 0 && at >= 0 && at < 3 * L * w);
            if (at < 0 || at >= 3 * L * w) continue;
            const int r = (int)(at / w / L), c = lists[at / w];
            ++seen[at];
            const bool swap = symmetric && c < q[r];
            CHECK(std::get<0>(s[k]) == (swap ? c : q[r]) && std::get<1>(s[k]) == (swap ? q[r] : c));
            both += std::get<0>(s[k]) == 4 && std::get<1>(s[k]) == 7;
            if (k > 0) CHECK(std::make_tuple(std::get<1>(s[k - 1]), std::get<0>(s[k - 1]), std::get<2>(s[k - 1])) < std::make_tuple(std::get<1>(s[k]), std::get<0>(s[k]), at));
        }
        for (int r = 0; r < 3; ++r)
            for (int j = 0; j < L; ++j) {
                const int32_t c = lists[r * L + j];
                CHECK(seen[((int64_t)r * L + j) * w] == ((c < 0 || c == q[r]) ? 0 : 1));
            }
        CHECK(s.size() == 8);                                // 12 cells less three -1 and one own track
        CHECK(both == (symmetric ? 2 : 1));                  // (4, 7) for row 0 and, symmetric, for row 2 as well: computed twice
    }
    acx::query_list_pairs(q, 3, nullptr, 0, w, 1, pairs, idx);
    CHECK(pairs.empty() && idx.empty());
}

static void check_ftm2d_tiles()
{
    const int n = 12;
    const int32_t q[5] = {0, 11, 7, 5, 2};                   // column 0, column n - 1, inside a run, in the gap, at a run's end
    const std::vector<int32_t> gap = {0, 1, 2, 6, 7, 8, 11};
    for (int symmetric = 0; symmetric < 2; ++symmetric)
        for (int all = 0; all < 2; ++all) {
            std::vector<int32_t> cols = gap;
            if (all) { cols.clear(); for (int j = 0; j < n; ++j) cols.push_back(j); }
            const std::vector<acx_grid_tile> tiles = acx::query_ftm2d_band_tiles(q, 5, all ? nullptr : cols.data(), (int)cols.size(), n, symmetric);
            std::vector<int> cover(5 * n, 0);
            for (const acx_grid_tile &t : tiles) {
                CHECK(t.diagonal == 0 && t.rows >= 1 && t.cols >= 1 && t.offset >= 0 && t.offset < 5 * n);
                if (t.offset < 0 || t.offset >= 5 * n) continue;
                const int r = (int)(t.offset / n), a = (int)(t.offset % n);
                const bool below = symmetric && a < q[r];
                if (below) CHECK(t.cols == 1 && t.col0 == q[r] && t.row0 == a && a + t.rows <= q[r]);      // rows x 1: (column, query)
                else CHECK(t.rows == 1 && t.row0 == q[r] && t.col0 == a && (a > q[r] || a + t.cols <= q[r]));      // 1 x cols: (query, column)
                const int len = t.rows * t.cols;
                CHECK(a + len <= n);
                for (int i = 0; i < len && a + i < n; ++i) ++cover[r * n + a + i];
            }
            for (int r = 0; r < 5; ++r) {
                std::vector<int> want(n, 0);
                for (int32_t c : cols) want[c] = c != q[r];
                for (int c = 0; c < n; ++c) CHECK(cover[r * n + c] == want[c]);
            }
        }
}

static void check_rows()
{
    const int64_t topk = 4 * 300 + 8 * 7, scores = 2 * 4 * 300;      // the rows of test_band_splitting (300 tracks, k = 7)
    CHECK(acx::query_band_rows(10, topk, 4 * topk, acx::QUERY_BAND_ROWS) == 4);
    CHECK(acx::query_band_rows(10, scores, 3 * scores, acx::QUERY_BAND_ROWS) == 3);
    CHECK(acx::query_band_rows(10, topk, (2 * topk - 8) / 2, acx::QUERY_BAND_ROWS) == 0);
    CHECK(acx::query_band_rows(10, scores, (2 * topk - 8) / 2, acx::QUERY_BAND_ROWS) == 0);
    CHECK(acx::query_band_rows(10, topk, topk, acx::QUERY_BAND_ROWS) == 1);
    CHECK(acx::query_band_rows(10, topk, topk - 1, acx::QUERY_BAND_ROWS) == 0);
    CHECK(acx::query_band_rows(10, topk, (int64_t)1 << 40, acx::QUERY_BAND_ROWS) == 10);
    CHECK(acx::QUERY_BAND_ROWS == 128 && acx::query_band_rows(1000, topk, (int64_t)1 << 40, acx::QUERY_BAND_ROWS) == 128);
    CHECK(acx::query_band_rows(1000, topk, 127 * topk + topk - 1, acx::QUERY_BAND_ROWS) == 127);
    // list bands: 2^18 cells; an empty list counts as one cell per row
    CHECK(acx::query_list_band_cap(0) == 262144 && acx::query_list_band_cap(1) == 262144);
    CHECK(acx::query_list_band_cap(300) == 873 && acx::query_list_band_cap(262145) == 1);
    CHECK(acx::query_band_rows(1 << 20, 8, (int64_t)1 << 40, acx::query_list_band_cap(0)) == 262144);
    CHECK(acx::query_band_rows(1 << 20, 12, (int64_t)1 << 40, acx::query_list_band_cap(1)) == 262144);
    CHECK(acx::query_band_rows(1000, 1208, (int64_t)1 << 40, acx::query_list_band_cap(300)) == 873);
    CHECK(acx::query_band_rows(1000, 1208, 5 * 1208, acx::query_list_band_cap(300)) == 5);
}

int main()
{
    check_layouts();
    check_band_pairs();
    check_list_pairs();
    check_ftm2d_tiles();
    check_rows();
    if (failures) std::fprintf(stderr, "query_plan_check: %d check(s) failed\n", failures);
    else std::printf("query_plan_check: ok\n");
    return failures ? 1 : 0;
}
