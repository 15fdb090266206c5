"""
CPU-only: the shape sets of tests/_serra09_shapes.py reach what tests/test_gpu_serra09_shapes.py says they reach -- every (cr, cq) class
key of the product path's batch sort, both sides of every inner class edge as rows AND as columns, every band kernel family in both
roles -- and the recurrence plots they give the kernels are neither empty nor full.  S.cls / S.key / S.family are the library's own
answers (acx_serra09_plan: the table of acoss_amd/csrc/serra09_plan.hpp, no device needed), so the literals below pin that table.
The second half does the same for the streaming class's sets (tests/test_gpu_serra09_streaming.py): every pair of class 5 in one batch,
the residues of the 64 x 64 tiles and the strip counts of the 2048-column sweep, alignments that need both sides of a strip seam, and
distance rows whose ties make the streaming selector descend.
"""
import numpy as np
import pytest

from tests import _serra09_shapes as S


def _dims(d):
    return [(int(d["M"][i]), int(d["M"][j])) for i, j in d["pairs"]]


@pytest.mark.parametrize("m", [1, 9, 10, 16])
def test_edge_set_hits_every_key_and_both_sides_of_every_edge(m):
    import oracle
    d = S.edge_set(m)
    p = oracle.serra09_params(m=m)
    lens = np.diff(d["offsets"])
    assert [oracle.serra09_embed_len(int(T), p) for T in lens] == d["M"].tolist()
    dims = _dims(d)
    assert len(dims) == 45 and sum(a * b for a, b in dims) == 26_822_817
    assert {S.key(a, b) for a, b in dims} == {(cr, cq) for cr in range(S.NC) for cq in range(S.NC)}
    Mqs, Mrs = {a for a, _ in dims}, {b for _, b in dims}
    for lo, up in zip(S.LOWER, S.UPPER):
        assert lo == up + 1 and S.cls(lo) == S.cls(up) + 1
        assert {lo, up} <= Mqs and {lo, up} <= Mrs, (lo, up)
    assert S.cls(2041) == 4 and S.cls(2042) == 5 and S.cls(1) == 0
    # two versions per length, from the two ends of the work
    assert sorted(d["M"].tolist()) == sorted(2 * (list(S.UPPER) + list(S.LOWER) + [3, 40]))


def test_every_band_family_is_named_in_both_roles():
    # the row pass of a pair runs the kernel of class cr (role 0), its column pass that of class cq (role 1); the edge set holds every key
    seen = {(S.family(m, c), role) for m in range(1, 17) for c in range(S.NC) for role in (0, 1)}
    assert {f for f, _ in seen} == set(S.FAMILIES) and len(S.FAMILIES) == 8
    assert seen == {(f, role) for f in S.FAMILIES for role in (0, 1)}
    assert [S.family(9, c) for c in range(5)] == ["band2_kernel<M, B2_NV, 16>", "band2_kernel<M, B2_NV, 32>", "band2_kernel<M, B2_NV_MID, 32>",
                                                  "band_kernel<M<=9, 4>", "band_kernel<M<=9, 8>"]
    assert [S.family(10, c) for c in range(5)] == ["band_kernel<M>=10, 2>"] * 2 + ["band_kernel<M>=10, 4>"] * 2 + ["band_kernel<M>=10, 8>"]
    # per m, the keys of the edge set put every class on both passes
    for m in (1, 9, 10, 16):
        dims = _dims(S.edge_set(m))
        assert {(S.family(m, S.key(a, b)[0]), 0) for a, b in dims} | {(S.family(m, S.key(a, b)[1]), 1) for a, b in dims} == \
            {(S.family(m, c), role) for c in range(S.NC) for role in (0, 1)}


def test_tile_edge_and_row_residue_sets():
    for m in (9, 12):
        d = S.tile_edge_set(m)
        dims = _dims(d)
        assert len(dims) == 126
        tiles = lambda M: (M + S.BAND - 1 + 63) // 64
        for side in (0, 1):         # every tile count 1 .. 32 from its last length, 2 .. 32 from its first, as Mq and as Mr
            other = [x[1 - side] for x in dims if x[side] != 300]
            assert set(other) == {300}
            Ms = sorted(x[side] for x in dims if x[side] != 300)
            assert Ms == sorted([57 + 64 * k for k in range(32)] + [58 + 64 * k for k in range(31)])
            assert {tiles(M) for M in Ms if M % 64 == 57} == set(range(1, 33))
            assert {tiles(M) for M in Ms if M % 64 == 58} == set(range(2, 33))
    for m in (4, 9, 13):
        dims = _dims(S.row_residue_set(m))
        assert len(dims) == 105
        assert {a for a, _ in dims} == set(range(1, 18)) | {248, 249, 250, 251}
        assert {a % 8 for a, _ in dims} == set(range(8))
        assert sorted({S.cls(b) for _, b in dims}) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("kappa", [0.095, 0.4])
def test_plots_are_neither_empty_nor_full(kappa):
    for d in (S.edge_set(9), S.tile_edge_set(9)):
        scores, Rs = S.oracle_plots(d, m=9, kappa=kappa)
        dens = np.array([R.mean() for R in Rs])
        print("kappa %g: densities %.4f .. %.4f, scores %g .. %g" % (kappa, dens.min(), dens.max(), scores.min(), scores.max()))
        for k, R in enumerate(Rs):
            assert 0 < int(R.sum()) < R.size, S.describe(d, k, 9)
            assert 0.01 <= dens[k] <= 0.6, (S.describe(d, k, 9), dens[k])


# ---- the streaming class: tests/test_gpu_serra09_streaming.py ------------------------------------------------------------------------
STACK_MS = tuple(range(17, 34))
LONG_MS = (1, 9, 16, 17, 33)


def _streams(d, m, **kw):
    """The library's plan of the set's pair list: every pair of class 5 with the streaming family and the strip sweep, all in batch 0."""
    from acoss_amd import _lib
    rec = _lib.serra09_plan(np.diff(d["offsets"]), d["pairs"], _lib.serra09_params(m=m, **kw))
    assert len(rec) == len(d["pairs"])
    assert np.all(rec["cr"] == S.NC) and np.all(rec["cq"] == S.NC) and np.all(rec["batch"] == 0) and np.all(rec["sweep_cols"] == 0)
    names = {_lib.serra09_family_name(f, m) for f in rec["row_family"]} | {_lib.serra09_family_name(f, m) for f in rec["col_family"]}
    assert names == {"csm_long_kernel + rowsel_long_kernel"}
    if not kw:
        assert [(int(r["Mq"]), int(r["Mr"])) for r in rec] == _dims(d)
    return rec


@pytest.mark.parametrize("m", STACK_MS)
def test_stack_set_streams_and_sits_on_every_tile_edge(m):
    d = S.stack_set(m)
    _streams(d, m)
    dims = _dims(d)
    assert len(dims) == 121 and sum(a * b for a, b in dims) == 1_515_361
    for side in (0, 1):
        Ms = {x[side] for x in dims}
        assert Ms == set(S.STACK_SIDES)
        assert {1, 2, 3, 63, 0} <= {M % 64 for M in Ms}         # a last tile of 1, 2, 3, 63 and 64 cells
        assert {M % 4 for M in Ms} == {0, 1, 2, 3}               # four rows to a workgroup (rowsel_long_kernel, binarise_long_kernel)
        assert {1, 2, 3} <= Ms and {(M + 63) // 64 for M in Ms} == {1, 2, 3, 4, 8}
    assert sorted(d["M"].tolist()) == sorted(2 * list(S.STACK_SIDES))


@pytest.mark.parametrize("m", LONG_MS)
def test_long_set_streams_and_sits_on_every_strip_edge(m):
    d = S.long_set(m)
    _streams(d, m)
    dims = _dims(d)
    assert len(dims) == 103 and sum(a * b for a, b in dims) == 18_639_749
    assert S.cls(2041, m) == (4 if m <= 16 else 5) and S.cls(2042, m) == 5
    strips = lambda Ne: (Ne + S.STRIP - 1) // S.STRIP
    for drop in (0, 1):              # dp_start = 3 drops a row and a column
        for n in (1, 2):             # the last length of n strips and the first or second of n + 1, as the sweep's columns
            Ne = {b - drop for _, b in dims}
            assert n * S.STRIP in Ne and Ne & {n * S.STRIP + 1, n * S.STRIP + 2}, (drop, n)
        assert {strips(b - drop) for _, b in dims if b > 2041} == {1, 2, 3}       # (a one-cell row and dp_start = 3: no strip at all)
    for side in (0, 1):              # every long side against every short one, both ways round
        other = 1 - side
        assert {(x[side], x[other]) for x in dims if x[other] in S.SHORT_SIDES} == {(L, s) for L in S.LONG_SIDES for s in S.SHORT_SIDES}
        assert {0, 1} <= {x[side] % 64 for x in dims if x[side] > 2041}
    assert set(S.LONG_SQUARES) <= set(dims)
    sub = _dims(S.long_subset(d))
    assert len(sub) == 20 and {max(x) for x in sub} == {2042, 2049} and {min(x) for x in sub} == set(S.SHORT_SIDES)


def test_other_embeddings_of_the_streaming_sets():
    """tau = 2 and embed_full = 1 (tests of the parameter switches): still one batch of streaming pairs, the lengths by the oracle."""
    import oracle
    for d, m in ((S.stack_set(17, tau=2), 17), (S.long_subset(S.long_set(9, tau=2)), 9)):
        rec = _streams(d, m, tau=2)
        assert [(int(r["Mq"]), int(r["Mr"])) for r in rec] == _dims(d) == _dims(S.relabel(d, m, tau=2))
    for d, m in ((S.stack_set(17), 17), (S.long_subset(S.long_set(9)), 9)):
        rec = _streams(d, m, embed_full=1)
        assert [(int(r["Mq"]), int(r["Mr"])) for r in rec] == _dims(S.relabel(d, m, embed_full=1)) == [(a + 1, b + 1) for a, b in _dims(d)]
    assert oracle.serra09_embed_len(S.frames_for(2049, 9, 2), oracle.serra09_params(tau=2)) == 2049


@pytest.mark.parametrize("m,kappa", [(17, 0.095), (24, 0.095), (33, 0.095), (9, 0.095), (9, 0.4)])
def test_streaming_plots_are_neither_empty_nor_full(m, kappa):
    sets = [S.long_set(9)] if m == 9 else [S.stack_set(m)] + ([S.long_set(m)] if m in LONG_MS else [])
    for d in sets:
        scores, Rs = S.oracle_plots(d, m=m, kappa=kappa)
        dims = _dims(d)
        dens = np.array([R.mean() for R in Rs])
        big = np.array([min(x) >= 8 for x in dims])
        print("m=%d kappa %g: densities %.4f .. %.4f (shorter side >= 8 cells), scores %g .. %g" % (
            m, kappa, dens[big].min(), dens[big].max(), scores.min(), scores.max()))
        for k in np.nonzero(big)[0]:
            assert 0 < int(Rs[k].sum()) < Rs[k].size, S.describe(d, k, m)
            assert 0.01 <= dens[k] <= 0.6, (S.describe(d, k, m), dens[k])


def test_seam_set_needs_both_strips():
    """The best path of each (300-cell query, 4300-cell reference) pair crosses a strip seam: the plot cut at the seam scores less on
    either side than the whole plot, for Qmax and for Dmax."""
    import oracle
    m = 9
    d = S.seam_set(m)
    _streams(d, m)
    assert _dims(d) == [(300, 4300), (300, 4300), (4300, 300), (4300, 300)] and sum(a * b for a, b in _dims(d)) == 5_160_000
    _, Rs = S.oracle_plots(d, m=m)
    for k, seam in ((0, 2048), (1, 4096)):
        R = Rs[k]
        for dmax in (False, True):
            whole, left, right = (oracle.qmax_binary(X, 0.5, 0.5, dmax) for X in (R, R[:, :seam], R[:, seam:]))
            print("seam %d dmax=%d: whole %g, cut %g | %g" % (seam, dmax, whole, left, right))
            assert left < whole and right < whole, (seam, dmax, whole, left, right)
            assert whole >= 250 and min(left, right) >= 100          # a path along the whole query, about half of it on either side


@pytest.mark.parametrize("m", [9, 17])
def test_tie_set_makes_the_selector_descend(m):
    """Rows of the tie set by what the streaming selector (wave_select_stream) has to do with them: all values equal (the shortcut), more
    than 64 values equal to the one at the percentile's rank (no bin of <= 64 candidates before the range has narrowed to that value:
    several passes), all values distinct (the i.i.d. case the suite had)."""
    import oracle
    from acoss_amd import _lib
    d = S.tie_set(m)
    dims = _dims(d)
    assert len(dims) == 127 and sum(a * b for a, b in dims) == 12_331_089
    rec = _lib.serra09_plan(np.diff(d["offsets"]), d["pairs"], _lib.serra09_params(m=m))
    assert [(int(r["Mq"]), int(r["Mr"])) for r in rec] == dims and np.all(rec["batch"] == 0)
    streams = rec["cr"] == S.NC
    assert np.array_equal(streams, rec["cq"] == S.NC)
    want = np.ones(127, bool) if m > 16 else np.array([max(x) == S.TIE_LONG for x in dims])
    assert np.array_equal(streams, want) and streams.sum() == (127 if m > 16 else 6)
    p = oracle.serra09_params(m=m)
    count = dict(all_equal=0, heavy=0, distinct=0, rows=0)
    def rows_of(k):
        i, j = d["pairs"][k]
        _, it = oracle.serra09_pair(S.track(d, i), S.track(d, j), p, want_intermediates=True)
        out = dict(all_equal=0, heavy=0, distinct=0, rows=0)
        for D in (it["d"], it["d"].T):
            n = D.shape[1]
            srt = np.sort(D, axis=1)
            kth = srt[:, int(np.floor(np.float32(max(n - 1, 1)) * np.float32(0.095)))]
            same = (D == kth[:, None]).sum(axis=1)
            out["rows"] += len(D)
            out["all_equal"] += int(np.sum(srt[:, 0] == srt[:, -1]))
            out["heavy"] += int(np.sum((same > 64) & (srt[:, 0] != srt[:, -1])))
            out["distinct"] += int(np.sum(np.all(srt[:, 1:] != srt[:, :-1], axis=1))) if n > 1 else 0
        return out
    for out in S.pool_map(rows_of, np.nonzero(streams)[0]):
        for name in count:
            count[name] += out[name]
    print("tie set m=%d: %s" % (m, count))
    assert count["all_equal"] >= 100 and count["heavy"] >= 1000 and count["distinct"] >= 100, count
