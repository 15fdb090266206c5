// Host check of acoss_amd/csrc/fused_plan.hpp (no GPU): reads one case from the file named on the command line --
//   Q L W M K n_types k half
//   Q queries
//   Q x L list entries
// -- and prints the plan the host driver of acx_query_fused_lists would follow: the chunks, every problem's descriptor
// and neighbourhood, the pair list with its slab destinations, the bytes per problem and the block layout.
// tests/test_fused_plan_host.py compares the text with a few lines of numpy.  The invariants that need no second
// opinion are asserted here.
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../acoss_amd/csrc/fused_plan.hpp"

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    using namespace acx;
    CHECK(argc == 2);
    FILE *f = fopen(argv[1], "r");
    CHECK(f);
    int Q, L, W, M, K, nt, k;
    long long half;
    CHECK(fscanf(f, "%d %d %d %d %d %d %d %lld", &Q, &L, &W, &M, &K, &nt, &k, &half) == 8);
    std::vector<int32_t> queries((size_t)Q), lists((size_t)Q * L);
    for (auto &v : queries) CHECK(fscanf(f, "%d", &v) == 1);
    for (auto &v : lists) CHECK(fscanf(f, "%d", &v) == 1);
    fclose(f);

    // the pair index walks the upper triangle row by row, without gaps
    for (int n = 2; n <= 40; ++n) {
        int64_t at = 0;
        for (int a = 0; a < n; ++a)
            for (int b = a + 1; b < n; ++b) CHECK(fused_pair_index(n, a, b) == at++);
        CHECK(at == fused_pairs(n));
    }
    CHECK(fused_pair_index(1025, 1023, 1024) == fused_pairs(1025) - 1);
    // slots: distances, two generations, two work matrices, the local scales -- distinct, in (3 M + 2) n^2 + n doubles
    for (int m = 2; m <= 4; ++m) {
        std::set<int> slots;
        for (int i = 0; i < m; ++i) { slots.insert(fused_slot_dist(m, i)); slots.insert(fused_slot_cur(m, i)); slots.insert(fused_slot_nxt(m, i)); }
        slots.insert(fused_slot_acc(m)); slots.insert(fused_slot_ut(m)); slots.insert(fused_slot_md(m));
        CHECK((int)slots.size() == 3 * m + 3 && *slots.rbegin() == 3 * m + 2 && fused_slot_md(m) == 3 * m + 2);
        CHECK(fused_mat_doubles(7, m) == (int64_t)fused_slot_md(m) * 49 + 7);
    }

    std::vector<int32_t> ns((size_t)Q), T;
    for (int i = 0; i < Q; ++i) {
        fused_neighbourhood(queries[i], lists.data() + (size_t)i * L, L, T);
        ns[i] = (int32_t)T.size();
    }
    printf("bytes");
    for (int i = 0; i < Q; ++i) printf(" %lld", (long long)fused_problem_bytes(ns[i], W, M, K, nt, k));
    printf("\n");
    int unfit = -1;
    const std::vector<int> ends = fused_chunks(ns, W, M, K, nt, k, half, &unfit);
    printf("unfit %d\nends", unfit);
    for (int e : ends) printf(" %d", e);
    printf("\n");
    if (unfit >= 0) return 0;
    CHECK(Q == 0 || (!ends.empty() && ends.back() == Q));
    std::vector<int32_t> pairs;
    std::vector<int64_t> idx;
    size_t first = 0;
    for (size_t ci = 0; ci < ends.size(); first = (size_t)ends[ci++]) {
        const FusedChunk ch = fused_chunk(queries.data(), lists.data(), L, (int)first, ends[ci], M, K);
        printf("chunk %zu %zu %d %lld %lld %lld\n", ci, ch.probs.size(), ch.max_n, (long long)ch.mat, (long long)ch.list, (long long)ch.pairs);
        int64_t bytes = 0;
        for (size_t p = 0; p < ch.probs.size(); ++p) {
            const FusedProb &pr = ch.probs[p];
            printf("prob %d %d %lld %lld %lld %lld\nT", pr.n, pr.qpos, (long long)pr.mat, (long long)pr.list, (long long)pr.pair, (long long)pr.tracks);
            for (int j = 0; j < pr.n; ++j) printf(" %d", ch.tracks[(size_t)pr.tracks + j]);
            printf("\n");
            CHECK(ch.tracks[(size_t)pr.tracks + pr.qpos] == queries[first + p]);
            bytes += fused_problem_bytes(pr.n, W, M, K, nt, k);
        }
        CHECK(ch.probs.size() == 1 || bytes <= half);
        CHECK(ch.probs.size() == 1 || ch.pairs <= FUSED_CHUNK_PAIRS);
        CHECK((int)ch.probs.size() <= FUSED_CHUNK_PROBLEMS);
        fused_chunk_pairs(ch, W, pairs, idx);
        CHECK((int64_t)idx.size() == ch.pairs && pairs.size() == 2 * idx.size());
        std::set<int64_t> seen(idx.begin(), idx.end());
        CHECK(seen.size() == idx.size());                      // every slab slot exactly once
        printf("pairs");
        for (size_t t = 0; t < idx.size(); ++t) {
            CHECK(pairs[2 * t] < pairs[2 * t + 1] && idx[t] % W == 0 && idx[t] / W < ch.pairs);
            printf(" %d %d %lld", pairs[2 * t], pairs[2 * t + 1], (long long)idx[t]);
        }
        printf("\n");
        const FusedLayout lay = fused_layout((size_t)ch.pairs * W, 5, (size_t)ch.mat, (size_t)ch.list, ch.probs.size(), ch.tracks.size(),
                                             ch.probs.size() * nt * k, ch.probs.size() * nt);
        CHECK(lay.col % 8 == 0 && lay.mat % 8 == 0 && lay.V % 8 == 0 && lay.J % 4 == 0 && lay.probs % 8 == 0 && lay.tracks % 4 == 0 && lay.idx % 4 == 0);
        CHECK(lay.slab == 0 && lay.col >= 4 * (size_t)ch.pairs * W && lay.mat >= lay.col + 40 && lay.V >= lay.mat + 8 * (size_t)ch.mat &&
              lay.J >= lay.V + 8 * (size_t)ch.list && lay.probs >= lay.J + 4 * (size_t)ch.list && lay.tracks >= lay.probs + sizeof(FusedProb) * ch.probs.size() &&
              lay.idx >= lay.tracks + 4 * ch.tracks.size() && lay.score >= lay.idx + 4 * ch.probs.size() * nt * k &&
              lay.flag >= lay.score + 4 * ch.probs.size() * nt * k && lay.total == lay.flag + ch.probs.size() * nt);
        printf("layout %zu\n", lay.total);
    }
    return 0;
}
