"""
GPU tests of the evaluation of a query set (run with -m gpu on a real MI355X): acx_query_ranks through ctypes and
CoverAlgorithm.evaluate.  Every expectation comes from paths that existed before them -- the pair-list entry points,
all_pairwise + normalize_by_length + getEvalStatistics(engine="device") -- or from numpy (tests/_rank_ref.py,
tests/_query_ref.py, tests/_evalq_ref.py); none comes from the code under test.  Positions, flags and the integer
statistics are compared for equality; MAP and MRR of a query subset to 1e-12 relative (the yardstick sums in another
order), of the whole collection bit for bit against the route through the matrix.
"""
import ctypes
import os

import numpy as np
import pytest

from . import _evalq_ref as eref
from . import _query_ref as qref
from . import _rank_ref as rref
from .test_gpu_query import ALGOS, _launches, _raw_rows, _setup

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _matrix(fin, queries, n):
    """The finished rows of `queries` as rows of an (n, n) matrix for tests/_rank_ref.py (other rows are never read)."""
    D = np.zeros((n, n), np.float32)
    D[np.asarray(queries)] = fin
    return D


def _mate_lists(lists):
    moff = np.concatenate([[0], np.cumsum([len(m) for m in lists])]).astype(np.int64)
    mates = np.array([t for m in lists for t in m], np.int32)
    return moff, mates


def _positions(fin, queries, moff, mates, posn):
    """The definition once more, on rows alone (no (n, n) matrix: for the 20 000-track test)."""
    n = fin.shape[1]
    posn = np.arange(n) if posn is None else np.asarray(posn)
    pos = np.full(len(mates), -1, np.int32)
    flag = np.zeros(len(queries), np.uint8)
    for i, q in enumerate(queries):
        s, other = fin[i], np.arange(n) != q
        if np.isnan(s[other]).any() or (s[other] == -np.inf).any():
            flag[i] = 1
            continue
        for j in range(int(moff[i]), int(moff[i + 1])):
            m = int(mates[j])
            pos[j] = 1 + np.count_nonzero(other & (s > s[m])) + np.count_nonzero(other & (s == s[m]) & (posn < posn[m]))
    return pos, flag


@pytest.mark.parametrize("name", ALGOS)
def test_query_ranks_equal_reference(ctx, name):
    """Positions and flags for all five algorithms, col_mode 0 / 1 / 2, posn given and None: tests/_rank_ref.py on the
    raw rows of the pair-list entry points finished by tests/_query_ref.py.  One query lists every other track, one
    lists nothing, one comes twice with different lists.  acx_rank_columns on the same finished rows must agree."""
    algo, sym, params, pair_fn, n, w, col, _ = _setup(ctx, name)
    queries = [7, 2, 9, 7, 5]
    lists = [[c for c in range(n) if c != 7], [], [1, 3], [0, 10], [8, 4, 6]]
    moff, mates = _mate_lists(lists)
    raw = _raw_rows(pair_fn, n, queries, sym, w)
    perm = np.random.default_rng(8).permutation(n).astype(np.int32)
    flagged = 0
    for mode, cl in ((0, None), (1, col), (2, col)):
        for posn in (None, perm, 3 * perm + 1):              # (tie ranks need not be a permutation: distinct is enough)
            pos, flag = ctx.query_ranks(algo, sym, params, queries, moff, mates, posn=posn, col=cl, col_mode=mode)
            assert pos.shape == (w, len(mates)) and pos.dtype == np.int32
            assert flag.shape == (len(queries), w) and flag.dtype == np.uint8
            for e in range(w):
                fin = qref.finish(raw[e], cl, mode)
                wp, wf = rref.rank_columns(_matrix(fin, queries, n), queries, moff, mates, posn=posn)
                print(name, mode, e, "flagged rows", int(wf.sum()))
                assert np.array_equal(flag[:, e], wf), (mode, e)
                assert np.array_equal(pos[e], wp), (mode, e)
                # the two APIs on the same finished rows: acx_rank_columns gives these positions and flags
                rp, rf = ctx.rank_columns(_matrix(fin, queries, n), queries, moff, mates, posn=posn)
                assert np.array_equal(pos[e], rp) and np.array_equal(flag[:, e], rf), ("rank_columns", mode, e)
                p2, f2 = _positions(fin, queries, moff, mates, posn)
                assert np.array_equal(p2, wp) and np.array_equal(f2, wf), "the two numpy statements agree"
                flagged += int(wf.sum())
                ok = np.repeat(wf == 0, np.diff(moff))
                assert np.all(pos[e][~ok] == -1) and np.all(pos[e][ok] >= 1) and np.all(pos[e][ok] <= n - 1)
                if wf[0] == 0:                               # every other track listed: a permutation of 1 .. n - 1
                    assert sorted(pos[e][:n - 1].tolist()) == list(range(1, n))
    # the other orientation rule
    other = _raw_rows(pair_fn, n, queries, not sym, w)
    pos, flag = ctx.query_ranks(algo, not sym, params, queries, moff, mates)
    for e in range(w):
        wp, wf = rref.rank_columns(_matrix(other[e], queries, n), queries, moff, mates)
        assert np.array_equal(pos[e], wp) and np.array_equal(flag[:, e], wf)
    # no queries at all
    pos, flag = ctx.query_ranks(algo, sym, params, [], [0], [])
    assert pos.shape == (w, 0) and flag.shape == (0, w)


def test_constructed_ties_serra09(ctx):
    """Two bit-identical copies of a track above every query get the same score in every row: their positions are
    neighbours, and which comes first follows posn -- not the track index."""
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
    assert np.array_equal(raw[0][:, a].view(np.uint32), raw[0][:, b].view(np.uint32)), "the construction itself: equal raw scores"
    col = np.sqrt(np.diff(offsets).astype(np.float64))
    moff, mates = _mate_lists([[a, b, 1], [b, a], [a, 5, b]])
    rev = np.arange(n, dtype=np.int32)[::-1].copy()           # posn[b] < posn[a]
    for mode, cl in ((0, None), (1, col), (2, col)):
        for posn, first, second in ((None, a, b), (rev, b, a)):
            pos, flag = ctx.query_ranks(_lib.ALGO_SERRA09, True, p, queries, moff, mates, posn=posn, col=cl, col_mode=mode)
            wp, wf = rref.rank_columns(_matrix(qref.finish(raw[0], cl, mode), queries, n), queries, moff, mates, posn=posn)
            assert np.array_equal(pos[0], wp) and np.array_equal(flag[:, 0], wf) and not flag.any()
            for i in range(len(queries)):
                got = dict(zip(mates[moff[i]:moff[i + 1]].tolist(), pos[0][moff[i]:moff[i + 1]].tolist()))
                assert got[second] == got[first] + 1, "equal scores: the tie rank decides"


def test_constructed_minus_inf_ftm2d(ctx):
    """A shingle far from everything scores exactly 0 against every other track, which col_mode 2 turns into -inf:
    exactly the (query, plane)s the yardstick flags are flagged, with positions -1; under col_mode 0 and 1 the 0 is an
    ordinary value and nothing is flagged."""
    from acoss_amd import _lib
    rng = np.random.default_rng(5)
    S = 0.3 * rng.standard_normal((20, 16))
    S[17] = S[11]
    S[18] = S[11]
    S[19] = 100.0                                        # exp(-|s - t|^2) underflows to 0 against every other track
    ctx.ftm2d_upload_shingles(S)
    queries = [6, 1, 11, 19]
    moff, mates = _mate_lists([[19, 2, 17], [18, 17], [17, 18, 19], [0, 5]])
    raw = _raw_rows(lambda pr: ctx.ftm2d_pairs(pr), 20, queries, True, 1)
    assert np.all(raw[0][:3, 19] == 0.0) and np.all(raw[0][3] == 0.0)
    col = 1.0 + rng.random(20)
    for mode, cl in ((0, None), (1, col), (2, col)):
        pos, flag = ctx.query_ranks(_lib.ALGO_FTM2D, True, None, queries, moff, mates, col=cl, col_mode=mode)
        wp, wf = rref.rank_columns(_matrix(qref.finish(raw[0], cl, mode), queries, 20), queries, moff, mates)
        assert np.array_equal(pos[0], wp) and np.array_equal(flag[:, 0], wf), mode
        if mode == 2:
            assert flag[:, 0].tolist() == [1, 1, 1, 1] and np.all(pos == -1)      # every row sees column 19 (row 19: all of them)
        else:
            assert not flag.any()
            assert pos[0][0] == 19 and pos[0][7] == 19                            # the 0 is last of 19 columns
            if mode == 0:
                assert pos[0][5:7].tolist() == [1, 2]                             # the query's own twins: score 1, index order


def _dataset(tmp_path, n):
    path = os.path.join(str(tmp_path), "ds.csv")
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i, i))
    return path


CLIQUE_SIZES = [2, 1, 3, 2, 1, 4, 1, 2, 3, 1, 2, 1, 1]       # 24 tracks: cliques of 2 to 4 and six singletons


def _make(cls_name, csv, tag):
    """An object of the class with a 24-track pool injected.  Serra09 / ChenFusion: a synthetic cover set whose labels
    are its works (clique mates score above 0, so no mate sits at -inf under ChenFusion's normalisation); the others:
    random features with the same labels."""
    from acoss_amd import algorithms, synth
    rng = np.random.default_rng(3)
    cls = getattr(algorithms, cls_name)
    a = cls(csv, "feat/", shortname=tag)
    assert a.N == sum(CLIQUE_SIZES)
    labels = ["w%d" % w for w, k in enumerate(CLIQUE_SIZES) for _ in range(k)]
    if cls_name in ("Serra09", "ChenFusion"):
        d = synth.cover_set(clique_sizes=CLIQUE_SIZES, seed=12, t_range=(60, 200))
        assert list(d["labels"]) == labels
        a.set_pooled_features([d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for i in range(a.N)], labels)
    elif cls_name == "Simple":
        feats = [rng.random((12, int(rng.integers(30, 80)))) for _ in range(a.N)]
        a.set_features([f / np.linalg.norm(f, axis=0, keepdims=True) for f in feats], labels)
    elif cls_name == "EarlyFusion":
        a.set_block_features(synth.earlyfusion_set(a.N, seed=6, nb_range=(20, 60)), labels)
    else:
        a.set_features(list(0.3 * rng.standard_normal((a.N, 36))), labels)
    return a


def _benchmark_sequence(full, cls_name):
    full.all_pairwise(symmetric=full._identify_symmetric)
    if hasattr(full, "normalize_by_length"):
        full.normalize_by_length()
    if cls_name == "ChenFusion":
        for key in ("qmax", "dmax"):
            full.Ds[key] *= -1


def _same_tuple(got, want):
    return all(np.float64(got[i]).tobytes() == np.float64(want[i]).tobytes() for i in range(4)) and np.array_equal(got[4], want[4])


@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion", "Simple", "EarlyFusion", "FTM2D"])
def test_evaluate_equals_benchmark_sequence(tmp_path, monkeypatch, cls_name):
    """evaluate() of one object against all_pairwise + normalize_by_length (+ ChenFusion's sign flip) +
    getEvalStatistics(engine="device") of a SECOND object of the same class: bit for bit with queries=None, CSV line
    included; a shuffled subset with singletons against tests/_evalq_ref.py on the second object's matrices."""
    monkeypatch.chdir(tmp_path)
    n = sum(CLIQUE_SIZES)
    csv = _dataset(tmp_path, n)
    tops = [1, 5, 10]
    ev, full = _make(cls_name, csv, "ev"), _make(cls_name, csv, "full")
    _benchmark_sequence(full, cls_name)
    types = list(full._identify_planes)
    cliques = [sorted(full.cliques[s]) for s in full.cliques]
    want = {t: full.getEvalStatistics(t, topsidx=tops, engine="device") for t in types}
    info = {}
    got = ev.evaluate(topsidx=tops, report=True, info=info)
    assert list(got) == types
    for t in types:
        print(cls_name, t, "evaluate", got[t], "matrix route", want[t], info[t])
        assert _same_tuple(got[t], want[t]), t
        D = np.array(full.Ds[t])
        n_flag = eref.flagged_rows(D, cliques)
        if cls_name != "ChenFusion":
            assert n_flag == 0, "these classes produce finite matrices"
        assert info[t]["host_rows"] == n_flag and info[t]["device_rows"] == sum(k for k in CLIQUE_SIZES if k > 1) - n_flag
    lines_ev = open("results_ev_%s.csv" % ev.name).read()
    lines_full = open("results_full_%s.csv" % full.name).read()
    assert lines_ev == lines_full and lines_ev.count("\n") == 1 + len(types)
    # a shuffled subset that includes singletons
    subset = np.random.default_rng(17).permutation(n)[:15]
    singles = [c[0] for c in cliques if len(c) == 1]
    assert set(subset) & set(singles) and set(subset) - set(singles)
    info = {}
    got = ev.evaluate(queries=subset, topsidx=tops, info=info)
    for t in types:
        D = np.array(full.Ds[t])
        w = eref.statistics(D, cliques, subset, tops)
        print(cls_name, t, "subset", got[t], "yardstick", w, info[t])
        assert got[t][0] == w[0] and got[t][2] == w[2] and np.array_equal(got[t][4], w[4]), t
        assert got[t][1] == pytest.approx(w[1], rel=1e-12) and got[t][3] == pytest.approx(w[3], rel=1e-12), t
        assert info[t]["host_rows"] == eref.flagged_rows(D, cliques, subset)
        if cls_name != "ChenFusion":
            assert info[t]["host_rows"] == 0
    # one similarity type, a subset of singletons only: nothing to rank, MRR 0 over the queries given
    with pytest.warns(UserWarning, match="no clique"):
        got = ev.evaluate(queries=singles[:3], similarity_types=types[-1:], topsidx=tops)
    assert list(got) == types[-1:] and np.isnan(got[types[-1]][0]) and got[types[-1]][1] == 0.0 and not got[types[-1]][4].any()
    for t in ev.Ds:
        assert not np.any(np.asarray(ev.Ds[t])), "evaluate must not write Ds"
    for fused in ev._identify_fused:
        with pytest.raises(NotImplementedError):
            ev.evaluate(similarity_types=[fused])
    ev.cleanup_memmap()
    full.cleanup_memmap()


def test_evaluate_with_minus_inf_rows(tmp_path, monkeypatch):
    """FTM2D shingles under a col_mode 2 normalisation (a subclass states it, as ChenFusion does): track 23 scores 0
    against everything, so every finished row holds a -inf outside its own cell, every evaluated row is flagged by the
    device and ranked on the host from query_rows() -- and the tuple is still the yardstick's."""
    from acoss_amd import algorithms
    monkeypatch.chdir(tmp_path)
    n = sum(CLIQUE_SIZES)                                  # track 23 is a singleton
    rng = np.random.default_rng(14)
    S = 0.3 * rng.standard_normal((n, 16))
    S[23] = 100.0
    colv = 1.0 + rng.random(n)

    class Mode2(algorithms.FTM2D):
        def _identify_norm(self):
            return 2, colv

    a = Mode2(_dataset(tmp_path, n), "feat/", shortname="minf")
    labels = ["w%d" % w for w, k in enumerate(CLIQUE_SIZES) for _ in range(k)]
    a.set_features(list(S), labels)
    cliques = [sorted(a.cliques[s]) for s in a.cliques]
    ctx, algo, params, keys = a._grid()
    raw = _raw_rows(lambda pr: ctx.ftm2d_pairs(pr), n, list(range(n)), True, 1)
    D = qref.finish(raw[0], colv, 2)
    assert np.all(D[:23, 23] == -np.inf)
    for queries in (None, [20, 3, 23, 8, 9, 1]):
        info = {}
        got = a.evaluate(queries=queries, topsidx=[1, 5], info=info)["main"]
        want = eref.statistics(D, cliques, queries, [1, 5])
        n_flag = eref.flagged_rows(D, cliques, queries)
        print("evaluate", got, "yardstick", want, info)
        assert n_flag > 0 and info["main"] == {"device_rows": 0, "host_rows": n_flag}
        assert got[0] == want[0] and got[2] == want[2] and np.array_equal(got[4], want[4])
        assert got[1] == pytest.approx(want[1], rel=1e-12) and got[3] == pytest.approx(want[3], rel=1e-12)
    a.cleanup_memmap()


def test_band_splitting(ctx):
    """A scratch limit that forces at least three bands gives the result of the one-band run; a limit under one row is
    ACX_ERR_NOMEM and leaves the context usable."""
    from acoss_amd import _lib
    rng = np.random.default_rng(11)
    n = 300
    ctx.ftm2d_upload_shingles(0.3 * rng.standard_normal((n, 12)))
    queries = rng.permutation(n)[:10]
    lists = [[int(c) for c in rng.permutation(n)[:int(k)] if c != q] for q, k in zip(queries, rng.integers(0, 9, size=10))]
    lists[4] = [c for c in range(20) if c != queries[4]]       # the longest list sets the row's charge
    moff, mates = _mate_lists(lists)
    posn = rng.permutation(n).astype(np.int32)
    one_p, one_f = ctx.query_ranks(_lib.ALGO_FTM2D, True, None, queries, moff, mates, posn=posn)
    raw = _raw_rows(lambda pr: ctx.ftm2d_pairs(pr), n, queries, True, 1)
    wp, wf = _positions(raw[0], queries, moff, mates, posn)
    assert np.array_equal(one_p[0], wp) and np.array_equal(one_f[:, 0], wf)
    per_row = 4 * n + 4 * max(len(m) for m in lists) + 1
    ctx.set_scratch_limit(2 * 4 * per_row)                # half of it holds 4 rows: 10 queries = 3 bands
    ctx.profile_enable(True)
    ctx.profile_reset()
    p, f = ctx.query_ranks(_lib.ALGO_FTM2D, True, None, queries, moff, mates, posn=posn)
    assert ctx.profile()["query_rank_kernel"]["launches"] == 3
    ctx.profile_enable(False)
    assert np.array_equal(p, one_p) and np.array_equal(f, one_f)
    ctx.set_scratch_limit(2 * per_row - 8)
    with pytest.raises(MemoryError, match="one query row"):
        ctx.query_ranks(_lib.ALGO_FTM2D, True, None, queries, moff, mates, posn=posn)
    ctx.set_scratch_limit(0)
    p, f = ctx.query_ranks(_lib.ALGO_FTM2D, True, None, queries, moff, mates, posn=posn)
    assert np.array_equal(p, one_p) and np.array_equal(f, one_f)
    # SiMPle (ordered, col_mode 1), 7 queries in bands of 2
    algo, sym, params, pair_fn, ns, w, col, _ = _setup(ctx, "simple")
    qs = [3, 20, 5, 11, 0, 22, 8]
    moff, mates = _mate_lists([[(q + d) % ns for d in (1, 4, 9)] for q in qs])
    one_p, one_f = ctx.query_ranks(algo, sym, params, qs, moff, mates, col=col, col_mode=1)
    ctx.set_scratch_limit(2 * 2 * (4 * ns + 4 * 3 + 1))
    p, f = ctx.query_ranks(algo, sym, params, qs, moff, mates, col=col, col_mode=1)
    assert np.array_equal(p, one_p) and np.array_equal(f, one_f)
    ctx.set_scratch_limit(0)
    # a caller's limit with room for everything: the pair kernels of ChenFusion run under what the band leaves of it
    algo, sym, params, pair_fn, ns, w, col, _ = _setup(ctx, "chenfusion")
    moff, mates = _mate_lists([[(q + d) % ns for d in (1, 2)] for q in qs[:5]])
    qs = [q % ns for q in qs[:5]]
    one_p, one_f = ctx.query_ranks(algo, sym, params, qs, moff, mates)
    ctx.set_scratch_limit(64 << 20)
    p, f = ctx.query_ranks(algo, sym, params, qs, moff, mates)
    assert np.array_equal(p, one_p) and np.array_equal(f, one_f)
    ctx.set_scratch_limit(0)


def test_rows_beyond_the_lds_budget(ctx):
    """20 000 tracks: a row no longer fits the LDS and is re-read and re-finished on every pass.  The raw rows come from
    the pair-list entry point."""
    from acoss_amd import _lib
    rng = np.random.default_rng(21)
    n = 20000
    S = 0.25 * rng.standard_normal((n, 8))
    S[15000:15040] = S[100:140]                           # exact ties far apart
    ctx.ftm2d_upload_shingles(S)
    queries = [19999, 120, 7, 15010]
    lists = [[0, 19998, 15000, 100], [15020, 15000 + 21, 121, 3, 4, 5, 6, 8, 9, 10, 11], [], [110, 15011, 15039, 139]]
    moff, mates = _mate_lists(lists)
    raw = _raw_rows(lambda pr: ctx.ftm2d_pairs(pr), n, queries, True, 1)
    col = 1.0 + rng.random(n)
    perm = rng.permutation(n).astype(np.int32)
    for mode, cl in ((0, None), (2, col)):
        fin = qref.finish(raw[0], cl, mode)
        for posn in (None, perm):
            pos, flag = ctx.query_ranks(_lib.ALGO_FTM2D, True, None, queries, moff, mates, posn=posn, col=cl, col_mode=mode)
            wp, wf = _positions(fin, queries, moff, mates, posn)
            print("mode", mode, "flags", wf.tolist(), "positions", wp.tolist())
            assert np.array_equal(flag[:, 0], wf) and np.array_equal(pos[0], wp), (mode, posn is not None)
    assert not _positions(raw[0], queries, moff, mates, None)[1].any(), "the mode-0 rows are finite: positions were counted"


def test_error_paths(ctx):
    """Invalid arguments only.  Each rule returns its error, names its argument, and launches nothing."""
    from acoss_amd import _lib
    fresh = _lib.Context(0)
    try:
        with pytest.raises(_lib.AcxError, match="not uploaded"):
            fresh.query_ranks(_lib.ALGO_FTM2D, True, None, [0], [0, 1], [1])
    finally:
        fresh.close()
    rng = np.random.default_rng(2)
    n = 30
    ctx.ftm2d_upload_shingles(0.3 * rng.standard_normal((n, 12)))
    ctx.profile_enable(True)
    ctx.profile_reset()
    col = 1.0 + rng.random(n)
    dup = np.arange(n, dtype=np.int32)
    dup[9] = dup[4]
    neg = np.arange(n, dtype=np.int32)
    neg[6] = -2
    F = _lib.ALGO_FTM2D
    cases = [
        (ValueError, r"mates\[1\] is queries\[1\] itself", dict(mates=[5, 2])),
        (ValueError, r"mates\[0\] = 30", dict(mates=[30, 3])),
        (ValueError, r"mates\[1\] = -1", dict(mates=[3, -1])),
        (ValueError, r"moff must be non-decreasing \(moff\[2\]\)", dict(moff=[0, 3, 2])),
        (ValueError, r"moff\[0\] must be 0", dict(moff=[1, 1, 2])),
        (ValueError, r"posn must hold distinct tie ranks \(posn\[9\] = posn\[4\] = 4\)", dict(posn=dup)),
        (ValueError, r"posn\[6\] = -2 is negative", dict(posn=neg)),
        (ValueError, r"queries\[1\] = 30", dict(queries=[0, 30])),
        (ValueError, "col must not be NULL", dict(col_mode=1)),
        (ValueError, "col must be NULL", dict(col=col, col_mode=0)),
        (ValueError, "spec.col_mode", dict(col=col, col_mode=3)),
    ]
    for exc, pattern, kw in cases:
        args = dict(queries=[1, 2], moff=[0, 1, 2], mates=[5, 6], posn=None, col=None, col_mode=0)
        args.update(kw)
        with pytest.raises(exc, match=pattern):
            ctx.query_ranks(F, True, None, args["queries"], args["moff"], args["mates"], posn=args["posn"], col=args["col"],
                            col_mode=args["col_mode"])
    # the shim's own checks of the list lengths
    with pytest.raises(ValueError, match="moff"):
        ctx.query_ranks(F, True, None, [1, 2], [0, 1], [5])
    with pytest.raises(ValueError, match="posn"):
        ctx.query_ranks(F, True, None, [1, 2], [0, 1, 2], [5, 6], posn=np.arange(n - 1))
    # NULL arguments and a missing pool: through the raw ABI
    q = np.array([1, 2], np.int32)
    moff, mates = np.array([0, 1, 2], np.int64), np.array([5, 6], np.int32)
    pos, flag = np.zeros(2, np.int32), np.zeros(2, np.uint8)
    fp = flag.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    spec = _lib.QuerySpec(F, 1, 0, 0)
    rc = ctx._L.acx_query_ranks(ctx._h, ctypes.byref(spec), None, _lib._iptr(q), 2, None, None, None, _lib._iptr(mates), _lib._iptr(pos), fp)
    assert rc == _lib.ACX_ERR_INVALID and b"moff" in ctx._L.acx_last_error(ctx._h)
    rc = ctx._L.acx_query_ranks(ctx._h, ctypes.byref(spec), None, _lib._iptr(q), 2, None, None, _lib._lptr(moff), None, _lib._iptr(pos), fp)
    assert rc == _lib.ACX_ERR_INVALID and b"mates" in ctx._L.acx_last_error(ctx._h)
    rc = ctx._L.acx_query_ranks(ctx._h, ctypes.byref(spec), None, _lib._iptr(q), 2, None, None, _lib._lptr(moff), _lib._iptr(mates), _lib._iptr(pos), None)
    assert rc == _lib.ACX_ERR_INVALID and b"out_flag" in ctx._L.acx_last_error(ctx._h)
    spec = _lib.QuerySpec(_lib.ALGO_SERRA09, 1, 0, 0)
    p = _lib.serra09_params()
    rc = ctx._L.acx_query_ranks(ctx._h, ctypes.byref(spec), _lib._params_ptr(p), _lib._iptr(q), 2, None, None, _lib._lptr(moff), _lib._iptr(mates),
                                _lib._iptr(pos), fp)
    assert rc == _lib.ACX_ERR_STATE and b"not uploaded" in ctx._L.acx_last_error(ctx._h)
    assert _launches(ctx) == 0, "the arguments are validated before the first launch"
    # ... and the context is as usable as before
    pos, flag = ctx.query_ranks(F, True, None, [1, 2], [0, 1, 2], [5, 6])
    raw = _raw_rows(lambda pr: ctx.ftm2d_pairs(pr), n, [1, 2], True, 1)
    wp, wf = rref.rank_columns(_matrix(raw[0], [1, 2], n), [1, 2], [0, 1, 2], [5, 6])
    assert np.array_equal(pos[0], wp) and np.array_equal(flag[:, 0], wf)
    prof = ctx.profile()
    assert prof["query_rank_kernel"]["launches"] == 1 and prof["ftm2d_tile_kernel"]["launches"] == 1
    ctx.profile_enable(False)
