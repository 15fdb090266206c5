"""
GPU tests of the query path (run with -m gpu on a real MI355X): acx_query_scores / acx_query_topk and
CoverAlgorithm.identify / query_rows.  Every expectation comes from paths that existed before them -- the pair-list
entry points, all_pairwise + normalize_by_length + top_matches, the CPU oracle -- or from numpy (tests/_query_ref.py,
proved against tests/_rank_ref.py in tests/test_query_host.py); none comes from the code under test, with the one
exception the large-row test states.  Every comparison is equality of indices and of score BITS.
"""
import ctypes
import os

import numpy as np
import pytest

from . import _query_ref as qref

pytestmark = pytest.mark.gpu

QUERIES = [7, 2, 9, 2, 5]          # non-contiguous, unsorted, one duplicate


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _launches(ctx):
    return sum(v["launches"] for v in ctx.profile().values())


@pytest.fixture()
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _raw_rows(pair_fn, n, queries, symmetric, planes):
    """(planes, Q, N) raw score rows from a pair-list entry point: the cell (q, c) is the pair (min, max) of a symmetric
    call and (q, c) of an ordered one; a query's own cell stays 0."""
    pairs, where = [], []
    for i, q in enumerate(queries):
        for c in range(n):
            if c == q:
                continue
            pairs.append((min(q, c), max(q, c)) if symmetric else (q, c))
            where.append((i, c))
    sc = np.asarray(pair_fn(np.array(pairs, np.int32)), dtype=np.float32).reshape(len(pairs), planes)
    rows = np.zeros((planes, len(queries), n), np.float32)
    where = np.array(where)
    for e in range(planes):
        rows[e, where[:, 0], where[:, 1]] = sc[:, e]
    return rows


def _setup(ctx, name):
    """Uploads the small pool of algorithm `name`: -> (algo, symmetric, params, pair_fn, n, planes, col)."""
    from acoss_amd import _lib, synth
    rng = np.random.default_rng(77)
    if name in ("serra09", "chenfusion"):
        d = synth.cover_set(clique_sizes=[2] * 9 + [3, 1], seed=31, t_range=(60, 420))
        ctx.upload_pool(d["frames"], d["offsets"])
        n = len(d["offsets"]) - 1
        col = np.sqrt(np.diff(d["offsets"]).astype(np.float64))
        assert len(np.unique(col)) > n // 2, "the lengths must differ"
        p = _lib.serra09_params()
        if name == "serra09":
            return _lib.ALGO_SERRA09, True, p, lambda pr: ctx.serra09_pairs(pr, p), n, 1, col, d
        return _lib.ALGO_CHENFUSION, True, p, lambda pr: ctx.chenfusion_pairs(pr, p), n, 2, col, d
    if name == "simple":
        feats = [rng.random((int(rng.integers(30, 90)), 12)) for _ in range(23)]
        feats = [f / np.linalg.norm(f, axis=1, keepdims=True) for f in feats]
        offs = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int64)
        ctx.upload_pool_f64(np.concatenate(feats), offs)
        col = np.sqrt(np.diff(offs).astype(np.float64))
        return _lib.ALGO_SIMPLE, False, _lib.SimpleParams(10, 1), lambda pr: ctx.simple_pairs(pr, 10).astype(np.float32), 23, 1, col, None
    if name == "earlyfusion":
        tracks = synth.earlyfusion_set(11, seed=4, nb_range=(20, 70))
        ctx.ef_upload_pool(tracks)
        col = 1.0 + rng.random(11)
        return (_lib.ALGO_EARLYFUSION, True, _lib.EfParams(0.1, 10), lambda pr: ctx.earlyfusion_pairs(pr, kappa=0.1, K=10), 11, 4,
                col, None)
    if name == "ftm2d":
        S = 0.3 * rng.standard_normal((37, 24))
        ctx.ftm2d_upload_shingles(S)
        col = 1.0 + rng.random(37)
        return _lib.ALGO_FTM2D, True, None, lambda pr: ctx.ftm2d_pairs(pr), 37, 1, col, None
    raise KeyError(name)


ALGOS = ["serra09", "chenfusion", "simple", "earlyfusion", "ftm2d"]


@pytest.mark.parametrize("name", ALGOS)
def test_rows_equal_pair_list(ctx, name):
    algo, sym, params, pair_fn, n, w, col, d = _setup(ctx, name)
    want = _raw_rows(pair_fn, n, QUERIES, sym, w)
    got = ctx.query_scores(algo, sym, params, QUERIES)
    assert got.shape == (w, len(QUERIES), n) and got.dtype == np.float32
    assert _same(got, want)
    assert np.all(got[:, np.arange(len(QUERIES)), QUERIES] == 0.0)
    # the other orientation rule: ordered cells (q, c) / symmetric cells (min, max)
    other = _raw_rows(pair_fn, n, QUERIES, not sym, w)
    assert _same(ctx.query_scores(algo, not sym, params, QUERIES), other)
    for mode in (1, 2):
        got = ctx.query_scores(algo, sym, params, QUERIES, col=col, col_mode=mode)
        for e in range(w):
            assert _same(got[e], qref.scores(want[e], QUERIES, col, mode)), (mode, e)
    if name == "serra09":
        import oracle
        pairs = np.array([(min(q, c), max(q, c)) for q in QUERIES for c in range(n) if c != q], np.int32)
        ref = oracle.serra09_pairs(d["frames"], d["offsets"], pairs)
        k = 0
        for i, q in enumerate(QUERIES):
            for c in range(n):
                if c != q:
                    assert _bits(want[0, i, c]) == _bits(ref[k]), (q, c)
                    k += 1


def _assert_topk_rows_agrees(ctx, fin, n, k, gi, gs, what):
    """The two APIs on the same finished rows: acx_topk_rows over the rows of query_scores, placed in an (n, n) matrix,
    gives the indices of query_topk and the bits of its scores (NaN compared as bits)."""
    for e in range(fin.shape[0]):
        D = np.zeros((n, n), np.float32)
        D[np.asarray(QUERIES)] = fin[e]
        ri, rs = ctx.topk_rows(D, k, rows=QUERIES)
        assert np.array_equal(gi[:, e], ri), ("topk_rows", k, e, what)
        assert _same(gs[:, e], rs), ("topk_rows", k, e, what)


@pytest.mark.parametrize("name", ALGOS)
def test_topk_equals_reference(ctx, name):
    algo, sym, params, pair_fn, n, w, col, _ = _setup(ctx, name)
    raw = _raw_rows(pair_fn, n, QUERIES, sym, w)
    fin = {0: ctx.query_scores(algo, sym, params, QUERIES)}
    for mode in (1, 2):
        fin[mode] = ctx.query_scores(algo, sym, params, QUERIES, col=col, col_mode=mode)
    cand = np.array(sorted(set(range(1, n, 2)) | {2, 7}), np.int32)      # holds two of the queries (7 and 2) and misses others
    for k in (1, 10, n - 1, n + 5):
        for cands in (None, cand):
            gi, gs = ctx.query_topk(algo, sym, params, QUERIES, k, candidates=cands)
            assert gi.shape == (len(QUERIES), w, k) and gi.dtype == np.int32 and gs.dtype == np.float32
            for e in range(w):
                wi, ws = qref.topk(raw[e], QUERIES, k, candidates=cands)
                assert np.array_equal(gi[:, e], wi), (k, e, cands is not None)
                assert _same(gs[:, e], ws), (k, e, cands is not None)
            for i, q in enumerate(QUERIES):
                assert q not in gi[i]
            if cands is None:
                _assert_topk_rows_agrees(ctx, fin[0], n, k, gi, gs, 0)
    gi, _ = ctx.query_topk(algo, sym, params, QUERIES, n + 5)
    assert np.all(gi[:, :, n - 1:] == -1) and np.all(gi[:, :, :n - 1] >= 0)
    for mode in (1, 2):
        for cands in (None, cand):
            gi, gs = ctx.query_topk(algo, sym, params, QUERIES, 10, candidates=cands, col=col, col_mode=mode)
            for e in range(w):
                wi, ws = qref.topk(raw[e], QUERIES, 10, candidates=cands, col=col, col_mode=mode)
                assert np.array_equal(gi[:, e], wi) and _same(gs[:, e], ws), (mode, e)
            if cands is None:
                _assert_topk_rows_agrees(ctx, fin[mode], n, 10, gi, gs, mode)
    gi, gs = ctx.query_topk(algo, sym, params, QUERIES, 3, candidates=np.zeros(0, np.int32))
    assert np.all(gi == -1) and np.all(np.isnan(gs))


def test_constructed_ties_serra09(ctx):
    """Two bit-identical copies of a track at indices above every query: both are computed in the same orientation
    (query, copy), get the same score and are listed in index order."""
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
    raw = _raw_rows(lambda pr: ctx.serra09_pairs(pr, p), n, queries, True, 1)
    assert np.array_equal(_bits(raw[0][:, a]), _bits(raw[0][:, b])), "the construction itself: equal raw scores"
    col = np.sqrt(np.diff(offsets).astype(np.float64))
    for mode, cl in ((0, None), (1, col), (2, col)):
        gi, gs = ctx.query_topk(_lib.ALGO_SERRA09, True, p, queries, n + 1, col=cl, col_mode=mode)
        wi, ws = qref.topk(raw[0], queries, n + 1, col=cl, col_mode=mode)
        assert np.array_equal(gi[:, 0], wi) and _same(gs[:, 0], ws)
        for i in range(len(queries)):
            pa, pb = list(gi[i, 0]).index(a), list(gi[i, 0]).index(b)
            assert pb == pa + 1, "equal scores: ascending track index"
            assert _bits(gs[i, 0, pa]) == _bits(gs[i, 0, pb])


def test_constructed_ties_and_minus_inf_ftm2d(ctx):
    """Identical shingles tie; a shingle far from everything scores exactly 0, which col_mode 2 turns into -inf: an
    ordinary value that ranks after every other number."""
    from acoss_amd import _lib
    rng = np.random.default_rng(5)
    S = 0.3 * rng.standard_normal((20, 16))
    S[17] = S[11]
    S[18] = S[11]
    S[19] = 100.0                                        # exp(-|s - t|^2) underflows to 0 against every other track
    ctx.ftm2d_upload_shingles(S)
    queries = [6, 1, 11]
    raw = _raw_rows(lambda pr: ctx.ftm2d_pairs(pr), 20, queries, True, 1)
    assert np.all(raw[0][:, 19] == 0.0) and np.array_equal(_bits(raw[0][:2, 17]), _bits(raw[0][:2, 18]))
    col = 1.0 + rng.random(20)
    gi, gs = ctx.query_topk(_lib.ALGO_FTM2D, True, None, queries, 19, col=col, col_mode=2)
    wi, ws = qref.topk(raw[0], queries, 19, col=col, col_mode=2)
    assert np.array_equal(gi[:, 0], wi) and _same(gs[:, 0], ws)
    assert np.all(gi[:, 0, 18] == 19) and np.all(gs[:, 0, 18] == -np.inf) and np.all(np.isfinite(gs[:, 0, :18]))
    gi, gs = ctx.query_topk(_lib.ALGO_FTM2D, True, None, queries, 19)
    for i in range(2):
        pa, pb = list(gi[i, 0]).index(17), list(gi[i, 0]).index(18)
        assert pb == pa + 1 and _bits(gs[i, 0, pa]) == _bits(gs[i, 0, pb])
    assert list(gi[2, 0, :2]) == [17, 18] and np.all(gs[2, 0, :2] == 1.0)      # the query's own twins: score 1, index order
    rows = ctx.query_scores(_lib.ALGO_FTM2D, True, None, queries, col=col, col_mode=2)
    assert np.all(rows[0][:, 19] == -np.inf) and np.all(rows[0][np.arange(3), queries] == 0.0)


def _dataset(tmp_path, labels):
    path = os.path.join(str(tmp_path), "ds.csv")
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i, l in enumerate(labels):
            f.write("%s,t%d\n" % (l, i))
    return path


def _make(cls_name, csv, tag):
    from acoss_amd import algorithms, synth
    rng = np.random.default_rng(3)
    cls = getattr(algorithms, cls_name)
    a = cls(csv, "feat/", shortname=tag)
    labels = ["w%d" % (i // 2) for i in range(a.N)]
    if cls_name in ("Serra09", "ChenFusion"):
        d = synth.cover_set(clique_sizes=[2] * (a.N // 2), seed=12, t_range=(60, 200))
        a.set_pooled_features([d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for i in range(a.N)], labels)
    elif cls_name == "Simple":
        feats = [rng.random((12, int(rng.integers(30, 80)))) for _ in range(a.N)]
        a.set_features([f / np.linalg.norm(f, axis=0, keepdims=True) for f in feats], labels)
    elif cls_name == "EarlyFusion":
        a.set_block_features(synth.earlyfusion_set(a.N, seed=6, nb_range=(20, 60)), labels)
    else:
        a.set_features(list(0.3 * rng.standard_normal((a.N, 36))), labels)
    return a


@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion", "Simple", "EarlyFusion", "FTM2D"])
def test_identify_equals_benchmark_sequence(tmp_path, monkeypatch, cls_name):
    """identify / query_rows of one object against all_pairwise + normalize_by_length (+ ChenFusion's sign flip, the
    `*= -1` of do_late_fusion) + top_matches(rows=queries) of a SECOND object of the same class."""
    monkeypatch.chdir(tmp_path)
    n = 12
    csv = _dataset(tmp_path, ["w%d" % (i // 2) for i in range(n)])
    queries = [8, 3, 10, 3, 0]
    cand = np.array([0, 1, 3, 4, 6, 9, 10, 11])
    ident, full = _make(cls_name, csv, "ident"), _make(cls_name, csv, "full")
    full.all_pairwise(symmetric=full._identify_symmetric)
    if hasattr(full, "normalize_by_length"):
        full.normalize_by_length()
    if cls_name == "ChenFusion":
        for key in ("qmax", "dmax"):
            full.Ds[key] *= -1
    types = list(full._identify_planes)
    assert types == [k for k in full.Ds.keys()]
    for k in (1, 5, n + 3):
        got = ident.identify(queries, k=k)
        assert sorted(got) == sorted(types)
        for t in types:
            wi, ws = full.top_matches(t, k, rows=queries)
            assert np.array_equal(got[t][0], wi) and _same(got[t][1], ws), (t, k)
    got = ident.identify(queries, k=4, candidates=cand, similarity_types=types[-1:])
    assert list(got) == types[-1:]
    D = np.array(full.Ds[types[-1]])
    wi, ws = qref.topk(D[queries], queries, 4, candidates=cand)
    assert np.array_equal(got[types[-1]][0], wi) and _same(got[types[-1]][1], ws)
    rows = ident.query_rows(queries)
    for t in types:
        want = np.array(full.Ds[t])[queries]
        want[np.arange(len(queries)), queries] = 0.0
        assert _same(rows[t], want), t
    for t in ident.Ds:
        assert not np.any(np.asarray(ident.Ds[t])), "identify must not write Ds"
    for fused in ident._identify_fused:
        with pytest.raises(NotImplementedError):
            ident.identify(queries, similarity_types=[fused])
    ident.cleanup_memmap()
    full.cleanup_memmap()


def test_band_splitting(ctx):
    """A scratch limit that forces at least three bands gives the results of the one-band run; a limit under one row is
    ACX_ERR_NOMEM and leaves the context usable.  (FTM2D and SiMPle: their pair kernels need no scratch arena, so the
    limit can go down to a few rows; a Serra09 pair alone needs more than a band of this size.)"""
    from acoss_amd import _lib
    rng = np.random.default_rng(11)
    n, k = 300, 7
    ctx.ftm2d_upload_shingles(0.3 * rng.standard_normal((n, 12)))
    queries = rng.integers(0, n, size=10)
    one_i, one_s = ctx.query_topk(_lib.ALGO_FTM2D, True, None, queries, k)
    one_rows = ctx.query_scores(_lib.ALGO_FTM2D, True, None, queries)
    per_row = 4 * n + 8 * k
    ctx.set_scratch_limit(2 * 4 * per_row)               # half of it holds 4 rows: 10 queries = 3 bands
    gi, gs = ctx.query_topk(_lib.ALGO_FTM2D, True, None, queries, k)
    assert np.array_equal(gi, one_i) and _same(gs, one_s)
    ctx.set_scratch_limit(2 * 3 * (2 * 4 * n))           # query_scores: 3 rows per band, 4 bands
    assert _same(ctx.query_scores(_lib.ALGO_FTM2D, True, None, queries), one_rows)
    ctx.set_scratch_limit(2 * per_row - 8)
    with pytest.raises(MemoryError, match="one query row"):
        ctx.query_topk(_lib.ALGO_FTM2D, True, None, queries, k)
    with pytest.raises(MemoryError, match="one query row"):
        ctx.query_scores(_lib.ALGO_FTM2D, True, None, queries)
    ctx.set_scratch_limit(0)
    gi, gs = ctx.query_topk(_lib.ALGO_FTM2D, True, None, queries, k)
    assert np.array_equal(gi, one_i) and _same(gs, one_s)
    # SiMPle, 7 queries in bands of 2
    algo, sym, params, pair_fn, ns, w, col, _ = _setup(ctx, "simple")
    qs = [3, 20, 3, 11, 0, 22, 8]
    one_i, one_s = ctx.query_topk(algo, sym, params, qs, 5, col=col, col_mode=1)
    ctx.set_scratch_limit(2 * 2 * (4 * ns + 8 * 5))
    gi, gs = ctx.query_topk(algo, sym, params, qs, 5, col=col, col_mode=1)
    assert np.array_equal(gi, one_i) and _same(gs, one_s)
    ctx.set_scratch_limit(0)
    # a caller's limit with room for everything: the pair kernels of Serra09 run under what the band leaves of it
    algo, sym, params, pair_fn, ns, w, col, _ = _setup(ctx, "serra09")
    one_i, one_s = ctx.query_topk(algo, sym, params, QUERIES, 6)
    ctx.set_scratch_limit(64 << 20)
    gi, gs = ctx.query_topk(algo, sym, params, QUERIES, 6)
    assert np.array_equal(gi, one_i) and _same(gs, one_s)
    ctx.set_scratch_limit(0)


def test_column_values_behind_an_odd_slab(ctx):
    """One and three queries of 23 (SiMPle) and 37 (FTM2D) tracks, one plane: R * n and R * L are odd, the slab ends
    4 bytes past a multiple of 8 and the f64 column values behind it have to move up to their alignment.  Every query
    export with col given, against _query_ref on the rows of the pair-list entry points: a list row is query_topk of
    its sorted valid entries, a position is the place in the full ranking (no tie, NaN or -inf in these rows)."""
    for name in ("simple", "ftm2d"):
        algo, sym, params, pair_fn, n, w, col, _ = _setup(ctx, name)
        assert w == 1 and n % 2 == 1
        cand = np.array([1, 8, n - 1], np.int32)
        for queries in ([7], [7, 2, 9]):
            raw = _raw_rows(pair_fn, n, queries, sym, w)[0]
            rng = np.random.default_rng(n + len(queries))
            lists = np.stack([rng.permutation(np.delete(np.arange(n), q))[:5] for q in queries]).astype(np.int32)
            lists[0, 2] = -1
            lists[-1, 0] = queries[-1]                        # the own track
            moff = 2 * np.arange(len(queries) + 1)
            mates = np.array([[(q + 1) % n, (q + 5) % n] for q in queries], np.int32).reshape(-1)
            for mode in (1, 2):
                what = (name, len(queries), mode)
                fin = qref.scores(raw, queries, col, mode)
                off_own = np.ones(fin.shape, bool)
                off_own[np.arange(len(queries)), queries] = False
                assert np.all(np.isfinite(fin[off_own])), what
                assert _same(ctx.query_scores(algo, sym, params, queries, col=col, col_mode=mode)[0], fin), what
                for cands in (None, cand):
                    gi, gs = ctx.query_topk(algo, sym, params, queries, 4, candidates=cands, col=col, col_mode=mode)
                    wi, ws = qref.topk(raw, queries, 4, candidates=cands, col=col, col_mode=mode)
                    assert np.array_equal(gi[:, 0], wi) and _same(gs[:, 0], ws), what + (cands is not None,)
                gi, gs = ctx.query_topk_lists(algo, sym, params, queries, lists, 4, col=col, col_mode=mode)
                for i, q in enumerate(queries):
                    wi, ws = qref.topk(raw[i:i + 1], [q], 4, candidates=np.sort(lists[i][lists[i] >= 0]), col=col, col_mode=mode)
                    assert np.array_equal(gi[i, 0], wi[0]) and _same(gs[i, 0], ws[0]), what + (i,)
                full, fs = qref.topk(raw, queries, n - 1, col=col, col_mode=mode)
                assert np.all(fs[:, 1:] != fs[:, :-1]), "the rows hold no tie"
                pos, flag = ctx.query_ranks(algo, sym, params, queries, moff, mates, col=col, col_mode=mode)
                want = [1 + list(full[i]).index(m) for i in range(len(queries)) for m in mates[moff[i]:moff[i + 1]]]
                assert pos.shape == (1, len(mates)) and np.array_equal(pos[0], want) and not flag.any(), what


def test_rows_beyond_the_lds_budget(ctx):
    """20 000 tracks: a row no longer fits the LDS and is re-read per pass.  The rows are checked against the pair-list
    entry point; the lists against _query_ref on those rows (the one place where the new query_scores feeds the
    yardstick -- after it has been checked itself)."""
    from acoss_amd import _lib
    rng = np.random.default_rng(21)
    n = 20000
    S = 0.25 * rng.standard_normal((n, 8))
    S[15000:15040] = S[100:140]                           # exact ties far apart
    ctx.ftm2d_upload_shingles(S)
    queries = [19999, 120, 7]
    rows = ctx.query_scores(_lib.ALGO_FTM2D, True, None, queries)
    want = _raw_rows(lambda pr: ctx.ftm2d_pairs(pr), n, queries, True, 1)
    assert _same(rows, want)
    col = 1.0 + rng.random(n)
    big = np.sort(rng.choice(n, size=17000, replace=False)).astype(np.int32)
    small = np.sort(rng.choice(n, size=5000, replace=False)).astype(np.int32)
    for k in (10, 1024):
        for cands in (None, big, small):
            for mode, cl in ((0, None), (2, col)):
                gi, gs = ctx.query_topk(_lib.ALGO_FTM2D, True, None, queries, k, candidates=cands, col=cl, col_mode=mode)
                wi, ws = qref.topk(rows[0], queries, k, candidates=cands, col=cl, col_mode=mode)
                assert np.array_equal(gi[:, 0], wi) and _same(gs[:, 0], ws), (k, mode)


def test_error_paths(ctx):
    """Invalid arguments only.  Each rule returns its error, names its argument, and launches nothing."""
    from acoss_amd import _lib
    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.AcxError, match="not uploaded"):
            fresh.query_topk(_lib.ALGO_FTM2D, True, None, [0], 1)
    finally:
        fresh.close()
    rng = np.random.default_rng(2)
    n = 30
    ctx.ftm2d_upload_shingles(0.3 * rng.standard_normal((n, 12)))
    ctx.profile_enable(True)
    ctx.profile_reset()
    col = 1.0 + rng.random(n)
    bad_col = col.copy()
    bad_col[3] = np.inf
    F = _lib.ALGO_FTM2D
    cases = [
        (ValueError, r"queries\[1\] = 30", dict(queries=[0, 30])),
        (ValueError, r"queries\[0\] = -1", dict(queries=[-1])),
        (ValueError, r"cands\[2\] = 30", dict(candidates=[1, 2, 30])),
        (ValueError, r"cands must be strictly ascending \(cands\[2\]\)", dict(candidates=[1, 5, 5])),
        (ValueError, r"cands must be strictly ascending \(cands\[1\]\)", dict(candidates=[4, 2])),
        (ValueError, "col must not be NULL", dict(col_mode=1)),
        (ValueError, "col must be NULL", dict(col=col, col_mode=0)),
        (ValueError, r"col\[3\] is not finite", dict(col=bad_col, col_mode=2)),
        (ValueError, "spec.col_mode", dict(col=col, col_mode=3)),
        (ValueError, "k must be >= 1", dict(k=0)),
        (NotImplementedError, "k = 1025", dict(k=1025)),
    ]
    for exc, pattern, kw in cases:
        args = dict(queries=[1, 2], k=3, candidates=None, col=None, col_mode=0)
        args.update(kw)
        with pytest.raises(exc, match=pattern):
            ctx.query_topk(F, True, None, args["queries"], args["k"], candidates=args["candidates"], col=args["col"],
                           col_mode=args["col_mode"])
    for exc, pattern, kw in cases[:2] + cases[5:9]:
        args = dict(queries=[1, 2], col=None, col_mode=0)
        args.update({k_: v for k_, v in kw.items() if k_ in args})
        with pytest.raises(exc, match=pattern):
            ctx.query_scores(F, True, None, args["queries"], col=args["col"], col_mode=args["col_mode"])
    # reserved != 0, an unknown algorithm, a missing params struct, a missing pool: through the raw ABI
    q = np.array([1, 2], np.int32)
    idx, sc = np.zeros(6, np.int32), np.zeros(6, np.float32)
    spec = _lib.QuerySpec(9, 1, 0, 0)
    rc = ctx._L.acx_query_topk(ctx._h, ctypes.byref(spec), None, _lib._iptr(q), 2, None, 0, None, 3, _lib._iptr(idx), _lib._fptr(sc))
    assert rc == _lib.ACX_ERR_INVALID and b"spec.algo" in ctx._L.acx_last_error(ctx._h)
    spec = _lib.QuerySpec(F, 2, 0, 0)
    rc = ctx._L.acx_query_topk(ctx._h, ctypes.byref(spec), None, _lib._iptr(q), 2, None, 0, None, 3, _lib._iptr(idx), _lib._fptr(sc))
    assert rc == _lib.ACX_ERR_INVALID and b"spec.symmetric" in ctx._L.acx_last_error(ctx._h)
    spec = _lib.QuerySpec(F, 1, 0, 7)
    rc = ctx._L.acx_query_topk(ctx._h, ctypes.byref(spec), None, _lib._iptr(q), 2, None, 0, None, 3, _lib._iptr(idx), _lib._fptr(sc))
    assert rc == _lib.ACX_ERR_INVALID and b"spec.reserved" in ctx._L.acx_last_error(ctx._h)
    spec = _lib.QuerySpec(_lib.ALGO_SERRA09, 1, 0, 0)
    rc = ctx._L.acx_query_topk(ctx._h, ctypes.byref(spec), None, _lib._iptr(q), 2, None, 0, None, 3, _lib._iptr(idx), _lib._fptr(sc))
    assert rc == _lib.ACX_ERR_INVALID and b"params" in ctx._L.acx_last_error(ctx._h)
    spec = _lib.QuerySpec(_lib.ALGO_SERRA09, 1, 0, 0)
    p = _lib.serra09_params()
    rc = ctx._L.acx_query_topk(ctx._h, ctypes.byref(spec), _lib._params_ptr(p), _lib._iptr(q), 2, None, 0, None, 3, _lib._iptr(idx), _lib._fptr(sc))
    assert rc == _lib.ACX_ERR_STATE and b"not uploaded" in ctx._L.acx_last_error(ctx._h)
    assert _launches(ctx) == 0, "the arguments are validated before the first launch"
    # ... and the context is as usable as before
    gi, gs = ctx.query_topk(F, True, None, [1, 2], 3)
    raw = _raw_rows(lambda pr: ctx.ftm2d_pairs(pr), n, [1, 2], True, 1)
    wi, ws = qref.topk(raw[0], [1, 2], 3)
    assert np.array_equal(gi[:, 0], wi) and _same(gs[:, 0], ws)
    prof = ctx.profile()
    assert prof["query_topk_kernel"]["launches"] == 1 and prof["ftm2d_tile_kernel"]["launches"] == 1
    ctx.query_scores(F, True, None, [1, 2])
    assert ctx.profile()["query_rows_kernel"]["launches"] == 1
    ctx.profile_enable(False)
