"""
GPU tests of the rerank path (run with -m gpu on a real MI355X): acx_query_topk_lists and CoverAlgorithm.rerank /
identify_cascade / rerank_tracks.  Every expectation comes from paths that existed before them -- the pair-list entry
points, acx_query_topk, identify -- or from numpy (tests/_query_lists_ref.py, proved in tests/test_query_lists_host.py);
none comes from the code under test.  Every comparison is equality of indices and of score BITS.  Pools, helpers and
sizes are those of tests/test_gpu_query.py and tests/test_gpu_append.py.
"""
import ctypes

import numpy as np
import pytest

from . import _query_lists_ref as lref
from . import test_gpu_append as ta
from . import test_gpu_query as tq
from .test_gpu_query import ctx  # noqa: F401  (the fixture: one fresh context per test)

pytestmark = pytest.mark.gpu

QUERIES = tq.QUERIES               # [7, 2, 9, 2, 5]
L = 8
KERNEL = "query_topk_lists_kernel"


def _lists(n):
    """Five rows of L = 8 for QUERIES over a pool of n >= 11 tracks: unsorted everywhere; tracks below AND above the query
    in rows 0, 1, 3, 4 (both orientations of a symmetric class); -1 in the middle and at the end (rows 0, 3); row 1
    lists its own track 2; row 2 is empty; rows 1 and 3 are the same query with different lists."""
    t = n - 1
    lists = np.array([[t, 3, 8, -1, 0, 9, 1, -1],
                      [2, 9, 0, 4, 1, 6, 3, 5],
                      [-1, -1, -1, -1, -1, -1, -1, -1],
                      [10, 0, -1, 7, t - 1 if t > 10 else 8, -1, -1, -1],
                      [0, t, 4, 6, 8, 2, -1, 3]], np.int32)
    assert lists.shape == (len(QUERIES), L)
    return lists


def _check(got, want, what):
    gi, gs = got
    wi, ws = want
    assert gi.shape == wi.shape and np.array_equal(gi, wi), what
    assert tq._same(gs, ws), what


@pytest.mark.parametrize("name", tq.ALGOS)
def test_lists_equal_reference(ctx, name):  # noqa: F811
    """All five classes x col_mode 0 / 1 / 2 x k in {1, 10, L + 5} against numpy on raw rows of the pair-list entry
    points; the other orientation rule once; and (FTM2D) no tile kernel: only the listed cells are pairs."""
    algo, sym, params, pair_fn, n, w, col, _ = tq._setup(ctx, name)
    lists = _lists(n)
    raw = tq._raw_rows(pair_fn, n, QUERIES, sym, w)
    ctx.profile_enable(True)
    ctx.profile_reset()
    calls = 0
    for mode, cl in ((0, None), (1, col), (2, col)):
        for k in (1, 10, L + 5):
            gi, gs = ctx.query_topk_lists(algo, sym, params, QUERIES, lists, k, col=cl, col_mode=mode)
            calls += 1
            assert gi.shape == (len(QUERIES), w, k) and gi.dtype == np.int32 and gs.dtype == np.float32
            for e in range(w):
                _check((gi[:, e], gs[:, e]), lref.topk_lists(raw[e], QUERIES, lists, k, col=cl, col_mode=mode), (name, mode, k, e))
            assert np.all(gi[2] == -1) and np.all(np.isnan(gs[2])), "an empty row"
            assert 2 not in gi[1] and 2 not in gi[3], "the own track is skipped, also when listed"
    prof = ctx.profile()
    assert prof[KERNEL]["launches"] == calls
    assert prof["query_topk_kernel"]["launches"] == 0 and prof["ftm2d_tile_kernel"]["launches"] == 0
    if name == "ftm2d":
        assert prof["ftm2d_pairs_kernel"]["launches"] == calls
    ctx.profile_enable(False)
    other = tq._raw_rows(pair_fn, n, QUERIES, not sym, w)
    gi, gs = ctx.query_topk_lists(algo, not sym, params, QUERIES, lists, 10)
    for e in range(w):
        _check((gi[:, e], gs[:, e]), lref.topk_lists(other[e], QUERIES, lists, 10), (name, "other orientation", e))
    # no list at all
    gi, gs = ctx.query_topk_lists(algo, sym, params, QUERIES, np.zeros((len(QUERIES), 0), np.int32), 3)
    assert gi.shape == (len(QUERIES), w, 3) and np.all(gi == -1) and np.all(np.isnan(gs))
    gi, gs = ctx.query_topk_lists(algo, sym, params, [], np.zeros((0, 4), np.int32), 3)
    assert gi.shape == (0, w, 3)


@pytest.mark.parametrize("name", tq.ALGOS)
def test_same_ascending_list_equals_query_topk(ctx, name):  # noqa: F811
    algo, sym, params, pair_fn, n, w, col, _ = tq._setup(ctx, name)
    cand = np.array(sorted(set(range(1, n, 2)) | {2, 7}), np.int32)
    lists = np.tile(cand, (len(QUERIES), 1))
    for mode, cl in ((0, None), (1, col)):
        for k in (4, len(cand) + 2):
            want = ctx.query_topk(algo, sym, params, QUERIES, k, candidates=cand, col=cl, col_mode=mode)
            _check(ctx.query_topk_lists(algo, sym, params, QUERIES, lists, k, col=cl, col_mode=mode), want, (name, mode, k))


def test_constructed_ties_serra09(ctx):  # noqa: F811
    """Two bit-identical copies of a track, built as tests/test_gpu_query.py builds them, listed in DESCENDING index
    order: they come out in ascending index order with equal score bits."""
    from acoss_amd import _lib, synth
    d = synth.cover_set(clique_sizes=[2] * 6, seed=9, t_range=(60, 300))
    off = d["offsets"]
    n0 = len(off) - 1
    twin = d["frames"][off[3]:off[4]]
    frames = np.concatenate([d["frames"], twin, twin])
    offsets = np.concatenate([off, [off[-1] + len(twin), off[-1] + 2 * len(twin)]]).astype(np.int64)
    ctx.upload_pool(frames, offsets)
    n, a, b = n0 + 2, n0, n0 + 1
    queries = [4, 0, 3]
    p = _lib.serra09_params()
    raw = tq._raw_rows(lambda pr: ctx.serra09_pairs(pr, p), n, queries, True, 1)
    assert np.array_equal(tq._bits(raw[0][:, a]), tq._bits(raw[0][:, b])), "the construction itself: equal raw scores"
    lists = np.array([[b, 9, a, 1, -1, 6], [b, a, 2, 11, 5, 7], [10, b, 8, -1, a, 0]], np.int32)
    col = np.sqrt(np.diff(offsets).astype(np.float64))
    for mode, cl in ((0, None), (1, col), (2, col)):
        gi, gs = ctx.query_topk_lists(_lib.ALGO_SERRA09, True, p, queries, lists, 6, col=cl, col_mode=mode)
        _check((gi[:, 0], gs[:, 0]), lref.topk_lists(raw[0], queries, lists, 6, col=cl, col_mode=mode), mode)
        for i in range(len(queries)):
            pa, pb = list(gi[i, 0]).index(a), list(gi[i, 0]).index(b)
            assert pb == pa + 1, "equal scores: ascending track index"
            assert tq._bits(gs[i, 0, pa]) == tq._bits(gs[i, 0, pb])


def _random_lists(rng, n, Q, length, filled):
    lists = np.full((Q, length), -1, np.int32)
    for i in range(Q):
        slots = rng.choice(length, size=filled, replace=False)
        lists[i, slots] = rng.choice(n, size=filled, replace=False)
    return lists


def test_band_splitting(ctx):  # noqa: F811
    """A scratch limit that leaves 4 rows per band for 10 queries gives the results of the one-band run, in three
    launches; a limit under one row is ACX_ERR_NOMEM and leaves the context usable.  SiMPle in bands of 2; Serra09 under a
    caller's limit that the band shares with its pair kernels."""
    from acoss_amd import _lib
    rng = np.random.default_rng(11)
    n, k, ll = 300, 7, 40
    ctx.ftm2d_upload_shingles(0.3 * rng.standard_normal((n, 12)))
    queries = rng.integers(0, n, size=10)
    lists = _random_lists(rng, n, 10, ll, 33)
    raw = tq._raw_rows(lambda pr: ctx.ftm2d_pairs(pr), n, queries, True, 1)
    want = lref.topk_lists(raw[0], queries, lists, k)
    one_i, one_s = ctx.query_topk_lists(_lib.ALGO_FTM2D, True, None, queries, lists, k)
    _check((one_i[:, 0], one_s[:, 0]), want, "one band")
    per_row = 4 * ll + 8 * k
    ctx.profile_enable(True)
    ctx.profile_reset()
    ctx.set_scratch_limit(2 * 4 * per_row)               # half of it holds 4 rows: 10 queries = 3 bands
    _check(ctx.query_topk_lists(_lib.ALGO_FTM2D, True, None, queries, lists, k), (one_i, one_s), "three bands")
    assert ctx.profile()[KERNEL]["launches"] == 3
    ctx.set_scratch_limit(2 * per_row)                   # one row per band
    _check(ctx.query_topk_lists(_lib.ALGO_FTM2D, True, None, queries, lists, k), (one_i, one_s), "ten bands")
    assert ctx.profile()[KERNEL]["launches"] == 13
    ctx.profile_enable(False)
    ctx.set_scratch_limit(2 * per_row - 8)
    with pytest.raises(MemoryError, match="one query row"):
        ctx.query_topk_lists(_lib.ALGO_FTM2D, True, None, queries, lists, k)
    ctx.set_scratch_limit(0)
    _check(ctx.query_topk_lists(_lib.ALGO_FTM2D, True, None, queries, lists, k), (one_i, one_s), "afterwards")
    # SiMPle, 7 queries in bands of 2
    algo, sym, params, pair_fn, ns, w, col, _ = tq._setup(ctx, "simple")
    qs = [3, 20, 3, 11, 0, 22, 8]
    sl = _random_lists(rng, ns, len(qs), 9, 7)
    one = ctx.query_topk_lists(algo, sym, params, qs, sl, 5, col=col, col_mode=1)
    raw = tq._raw_rows(pair_fn, ns, qs, sym, w)
    _check((one[0][:, 0], one[1][:, 0]), lref.topk_lists(raw[0], qs, sl, 5, col=col, col_mode=1), "simple")
    ctx.set_scratch_limit(2 * 2 * (4 * 9 + 8 * 5))
    _check(ctx.query_topk_lists(algo, sym, params, qs, sl, 5, col=col, col_mode=1), one, "simple, bands of 2")
    ctx.set_scratch_limit(0)
    algo, sym, params, pair_fn, ns, w, col, _ = tq._setup(ctx, "serra09")
    sl = _lists(ns)
    one = ctx.query_topk_lists(algo, sym, params, QUERIES, sl, 6)
    ctx.set_scratch_limit(64 << 20)
    _check(ctx.query_topk_lists(algo, sym, params, QUERIES, sl, 6), one, "serra09 under a caller's limit")
    ctx.set_scratch_limit(0)


def test_rows_per_band_follow_cells_not_128(ctx):  # noqa: F811
    """600 queries with lists of 5 are ONE band (the 128-row cap of the dense bands does not apply); with lists of 500
    they are 300 000 cells, over the budget of 2^18: two bands.  Both against numpy on ftm2d_pairs rows."""
    from acoss_amd import _lib
    rng = np.random.default_rng(17)
    n = 600
    ctx.ftm2d_upload_shingles(0.3 * rng.standard_normal((n, 12)))
    queries = rng.permutation(n)
    raw = tq._raw_rows(lambda pr: ctx.ftm2d_pairs(pr), n, queries, True, 1)
    ctx.profile_enable(True)
    for length, filled, bands in ((5, 4, 1), (500, 480, 2)):
        lists = _random_lists(rng, n, n, length, filled)
        ctx.profile_reset()
        gi, gs = ctx.query_topk_lists(_lib.ALGO_FTM2D, True, None, queries, lists, 6)
        assert ctx.profile()[KERNEL]["launches"] == bands, length
        _check((gi[:, 0], gs[:, 0]), lref.topk_lists(raw[0], queries, lists, 6), length)
    ctx.profile_enable(False)


def test_lists_beyond_the_lds_budget(ctx):  # noqa: F811
    """Lists of 17 000 positions no longer fit the LDS and are re-read per pass (as the rows of
    test_rows_beyond_the_lds_budget).  The FIRST query's expectation is numpy on its ftm2d_pairs row; the second uses
    query_topk with the sorted list, as that test permits itself."""
    from acoss_amd import _lib
    rng = np.random.default_rng(21)
    n, length = 20000, 17000
    S = 0.25 * rng.standard_normal((n, 24))
    S[15000:15040] = S[100:140]                           # exact ties far apart
    ctx.ftm2d_upload_shingles(S)
    queries = [120, 19999]
    lists = _random_lists(rng, n, 2, length, 16400)
    raw0 = tq._raw_rows(lambda pr: ctx.ftm2d_pairs(pr), n, queries[:1], True, 1)
    col = 1.0 + rng.random(n)
    for k in (10, 1024):
        for mode, cl in ((0, None), (2, col)):
            gi, gs = ctx.query_topk_lists(_lib.ALGO_FTM2D, True, None, queries, lists, k, col=cl, col_mode=mode)
            _check((gi[:1, 0], gs[:1, 0]), lref.topk_lists(raw0[0], queries[:1], lists[:1], k, col=cl, col_mode=mode), (k, mode))
            wi, ws = ctx.query_topk(_lib.ALGO_FTM2D, True, None, queries[1:], k, candidates=np.sort(lists[1][lists[1] >= 0]),
                                    col=cl, col_mode=mode)
            _check((gi[1:], gs[1:]), (wi, ws), (k, mode, "second query"))


def test_only_listed_cells_run(ctx):  # noqa: F811
    """A Serra09 pool with a 12-frame track (index a) and a 6-frame track (index b).  At the default m = 9 the 6-frame
    track is shorter than the delay-embedding stack, the 12-frame track an ordinary tiny one; at m = 16 both are short.
    Lists that omit the short tracks succeed -- their cells are never pairs --; a list that names one raises before any
    launch, and the pool answers the next call normally."""
    from acoss_amd import _lib, synth
    d = synth.cover_set(clique_sizes=[2] * 6, seed=9, t_range=(60, 300))
    off = d["offsets"]
    a, b = len(off) - 1, len(off)
    frames = np.concatenate([d["frames"], d["frames"][:12], d["frames"][20:26]])
    offsets = np.concatenate([off, [off[-1] + 12, off[-1] + 18]]).astype(np.int64)
    ctx.upload_pool(frames, offsets)
    n = b + 1
    queries = [4, 0, 9]
    for p, short in ((_lib.serra09_params(), [b]), (_lib.serra09_params(m=16), [a, b])):
        ok = [c for c in range(n) if c not in short]
        lists = np.array([[ok[-1], 3, 1, -1], [7, ok[-1], 2, 5], [-1, 0, 11, 10]], np.int32)
        pairs = np.array([(min(q, c), max(q, c)) for q in queries for c in ok if c != q], np.int32)
        sc = np.asarray(ctx.serra09_pairs(pairs, p), np.float32).reshape(-1)
        raw = np.zeros((1, len(queries), n), np.float32)
        raw[0, np.repeat(np.arange(3), len(pairs) // 3), [c for q in queries for c in ok if c != q]] = sc
        want = lref.topk_lists(raw[0], queries, lists, 4)
        got = ctx.query_topk_lists(_lib.ALGO_SERRA09, True, p, queries, lists, 4)
        _check((got[0][:, 0], got[1][:, 0]), want, "lists without the short tracks")
        ctx.profile_enable(True)
        ctx.profile_reset()
        for s in short:
            bad = lists.copy()
            bad[2, 0] = s
            with pytest.raises(_lib.AcxError, match="shorter than the delay-embedding stack"):
                ctx.query_topk_lists(_lib.ALGO_SERRA09, True, p, queries, bad, 4)
        assert tq._launches(ctx) == 0, "the pair list of the band is checked before its first launch"
        ctx.profile_enable(False)
        got = ctx.query_topk_lists(_lib.ALGO_SERRA09, True, p, queries, lists, 4)
        _check((got[0][:, 0], got[1][:, 0]), want, "the next call")


def test_error_paths(ctx):  # noqa: F811
    """Invalid arguments only.  Each rule returns its code, names its argument, and launches nothing."""
    from acoss_amd import _lib
    rng = np.random.default_rng(2)
    n = 30
    ctx.ftm2d_upload_shingles(0.3 * rng.standard_normal((n, 12)))
    ctx.profile_enable(True)
    ctx.profile_reset()
    F = _lib.ALGO_FTM2D
    good = np.array([[4, -1, 7], [9, 2, -1]], np.int32)
    cases = [
        (ValueError, r"lists\[1\]\[2\] = 30 is neither a track in \[0, 30\) nor -1", dict(lists=[[1, 2, 3], [4, 5, 30]])),
        (ValueError, r"lists\[0\]\[1\] = -2", dict(lists=[[1, -2, 3], [4, 5, 6]])),
        (ValueError, r"lists row 1 holds track 4 twice \(positions 0 and 2\)", dict(lists=[[1, 2, 3], [4, 5, 4]])),
        (ValueError, r"queries\[1\] = 30", dict(queries=[0, 30])),
        (ValueError, "col must not be NULL", dict(col_mode=1)),
        (ValueError, "k must be >= 1", dict(k=0)),
        (NotImplementedError, "k = 1025 is over the limit of 1024", dict(k=1025)),
    ]
    for exc, pattern, kw in cases:
        args = dict(queries=[1, 2], k=3, lists=good, col=None, col_mode=0)
        args.update(kw)
        with pytest.raises(exc, match=pattern):
            ctx.query_topk_lists(F, True, None, args["queries"], args["lists"], args["k"], col=args["col"], col_mode=args["col_mode"])
    with pytest.raises(ValueError, match=r"lists must be \(len\(queries\), L\)"):
        ctx.query_topk_lists(F, True, None, [1, 2], good[:1], 3)
    # NULL lists, a negative list_len, a missing pool: through the raw ABI
    q = np.array([1, 2], np.int32)
    idx, sc = np.zeros(6, np.int32), np.zeros(6, np.float32)
    spec = _lib.QuerySpec(F, 1, 0, 0)

    def call(spec, params, lists, list_len, k=3):
        return ctx._L.acx_query_topk_lists(ctx._h, ctypes.byref(spec), params, _lib._iptr(q), 2, lists, list_len, None, k,
                                           _lib._iptr(idx), _lib._fptr(sc))
    ta._code(ctx, call(spec, None, None, 3), _lib.ACX_ERR_INVALID, "lists must not be NULL", "list_len > 0")
    ta._code(ctx, call(spec, None, _lib._iptr(good), -1), _lib.ACX_ERR_INVALID, "list_len must be >= 0", "-1")
    ta._code(ctx, call(spec, None, _lib._iptr(good), 3, k=1025), _lib.ACX_ERR_UNSUPPORTED, "k = 1025")
    ta._code(ctx, call(_lib.QuerySpec(F, 1, 0, 7), None, _lib._iptr(good), 3), _lib.ACX_ERR_INVALID, "spec.reserved")
    ta._code(ctx, call(_lib.QuerySpec(_lib.ALGO_SERRA09, 1, 0, 0), _lib._params_ptr(_lib.serra09_params()), _lib._iptr(good), 3),
             _lib.ACX_ERR_STATE, "not uploaded")
    assert tq._launches(ctx) == 0, "the arguments are validated before the first launch"
    assert call(spec, None, None, 0) == _lib.ACX_OK and np.all(idx == -1) and np.all(np.isnan(sc)), "list_len == 0 needs no lists"
    # ... and the context is as usable as before
    gi, gs = ctx.query_topk_lists(F, True, None, [1, 2], good, 3)
    raw = tq._raw_rows(lambda pr: ctx.ftm2d_pairs(pr), n, [1, 2], True, 1)
    _check((gi[:, 0], gs[:, 0]), lref.topk_lists(raw[0], [1, 2], good, 3), "afterwards")
    prof = ctx.profile()
    assert prof[KERNEL]["launches"] == 2 and prof["ftm2d_pairs_kernel"]["launches"] == 1 and prof["ftm2d_tile_kernel"]["launches"] == 0
    ctx.profile_enable(False)


def _by_hand(algo, queries, lists, k):
    """rerank through paths that existed before it: identify of ONE query against the sorted valid entries of its row."""
    out = {}
    for i, q in enumerate(queries):
        row = np.asarray(lists[i])
        one = algo.identify([q], k=k, candidates=np.sort(row[row >= 0]))
        for t, (ii, ss) in one.items():
            out.setdefault(t, ([], []))
            out[t][0].append(ii[0])
            out[t][1].append(ss[0])
    return {t: (np.stack(v[0]), np.stack(v[1])) for t, v in out.items()}


def _check_types(got, want, what):
    assert sorted(got) == sorted(want), what
    for t in want:
        _check(got[t], want[t], (what, t))


def test_identify_cascade(tmp_path, monkeypatch):
    """Serra09 over an FTM2D first stage on twelve tracks: the by-hand composition, and with shortlist = N - 1 identify()."""
    monkeypatch.chdir(tmp_path)
    n = 12
    csv = tq._dataset(tmp_path, ["w%d" % (i // 2) for i in range(n)])
    second, first = tq._make("Serra09", csv, "second"), tq._make("FTM2D", csv, "first")
    queries = [8, 3, 10, 3, 0]
    for shortlist, k in ((5, 3), (5, 8), (4, 1)):
        lists = first.identify(queries, k=shortlist)["main"][0]
        assert lists.shape == (len(queries), shortlist) and np.all(lists >= 0)
        got = second.identify_cascade(first, queries, k=k, shortlist=shortlist)
        _check_types(got, _by_hand(second, queries, lists, k), (shortlist, k))
        for i in range(len(queries)):
            assert set(got["main"][0][i][got["main"][0][i] >= 0]) <= set(lists[i])
        _check_types(second.rerank(queries, [list(r) for r in lists], k=k), got, "rerank of the same lists, ragged")
    _check_types(second.identify_cascade(first, queries, k=4, shortlist=n - 1, first_type="main"), second.identify(queries, k=4),
                 "every other track shortlisted")
    # ragged shortlists with empty rows, any order
    ragged = [[11, 0, 5], [], [9], [4, 3, 7, 1], [0, 2]]
    padded = np.array([[11, 0, 5, -1], [-1, -1, -1, -1], [9, -1, -1, -1], [4, 3, 7, 1], [0, 2, -1, -1]])
    got = second.rerank(queries, ragged, k=3)
    _check_types(got, _by_hand(second, queries, padded, 3), "ragged")
    assert np.all(got["main"][0][1] == -1) and list(got["main"][0][4]) == [2, -1, -1], "the own track 0 is skipped"
    for t in second.Ds:
        assert not np.any(np.asarray(second.Ds[t])), "rerank must not write Ds"
    second.cleanup_memmap()
    first.cleanup_memmap()


@pytest.mark.parametrize("cls_name", ["Serra09", "Simple"])
def test_rerank_tracks(tmp_path, monkeypatch, cls_name):
    """rerank_tracks of an object over N tracks against rerank(queries=[N ..]) -- and identify, row by row -- of a SECOND
    object over the N + Q tracks; Ds, N and the pool are unchanged, also after a call that raised in the library."""
    from acoss_amd import _lib
    monkeypatch.chdir(tmp_path)
    N, Q = 9, 3
    tracks = ta._class_tracks(cls_name, N + Q)
    ident, full = ta._make(cls_name, tmp_path, "ident", tracks[:N]), ta._make(cls_name, tmp_path, "full", tracks)
    new, queries = tracks[N:], list(range(N, N + Q))
    types = list(full._identify_planes)
    lists = [[8, 0, 3, 5], [2], [7, 1, -1, 4, 6, 0]]
    padded = np.array([[8, 0, 3, 5, -1, -1], [2, -1, -1, -1, -1, -1], [7, 1, -1, 4, 6, 0]])
    before = ident.identify([0, 4, 7], k=5)
    plen = None if getattr(ident, "_pooled_len", None) is None else ident._pooled_len.copy()
    for k in (1, 3, 8):
        got = ident.rerank_tracks(new, lists, k=k)
        _check_types(got, _by_hand(full, queries, padded, k), ("by hand", k))
        _check_types(got, full.rerank(queries, lists, k=k), ("rerank on the larger collection", k))
    got = ident.rerank_tracks(new, padded, k=2, similarity_types=types[-1:])
    assert list(got) == types[-1:]

    def unchanged():
        ctx_, algo = ident._grid()[0], ident._grid()[1]
        assert len(ctx_.pool_lengths(algo)) == N and ident.N == N
        after = ident.identify([0, 4, 7], k=5)
        _check_types(after, before, "identify afterwards")
        if plen is not None:
            assert np.array_equal(ident._pooled_len, plen)
        for t in ident.Ds:
            assert not np.any(np.asarray(ident.Ds[t])), "rerank_tracks must not write Ds"
    unchanged()
    with pytest.raises(_lib.AcxError):
        ident.rerank_tracks([new[0], ta._too_short(cls_name, new[1])], [[1, 2], [3, 4]], k=2)
    unchanged()
    if cls_name == "Serra09":
        from acoss_amd.algorithms.rqa_serra09 import pool_median
        raw = ta._raw_tracks()
        pooled = [pool_median(t, 4) for t in raw]
        a = ta._make("Serra09", tmp_path, "raw", pooled[:6])
        a.downsample_fac = 4
        sl = [[5, 0, 2]] * len(raw[6:])
        _check_types(a.rerank_tracks(raw[6:], sl, k=2, raw=True), a.rerank_tracks(pooled[6:], sl, k=2), "raw=True")
        a.cleanup_memmap()
    ident.cleanup_memmap()
    full.cleanup_memmap()
