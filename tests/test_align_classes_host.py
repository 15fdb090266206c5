"""
Host-side checks of the alignment methods of Serra09, ChenFusion and EarlyFusion (align, align_paths, align_matches,
align_match_paths, align_sections, align_match_sections) and of the one-call forms above them: which method of the class's libacx
context each reaches, with which arguments, what it makes of the records that come back -- every field, the spans, the no-match
rows, the paths, the lists of sections -- and every refusal, with its text, before the first library call.  No GPU and no library:
the context is tests/_align_host.py's recording stand-in.
"""
import re

import numpy as np
import pytest

from tests import _align_host as H
from tests._align_host import N, Q, SERRA

ALIGN_DTYPE = np.dtype([("score", "<f4"), ("q0", "<i4"), ("r0", "<i4"), ("q1", "<i4"), ("r1", "<i4"),
                        ("q_span", "<i4", (2,)), ("r_span", "<i4", (2,))])

# (class, the similarity_type keyword, the context's method family, its plane)
CASES = [("Serra09", {}, "serra09", None),
         ("ChenFusion", {}, "serra09", None),
         ("ChenFusion", {"similarity_type": "qmax"}, "serra09", None),
         ("ChenFusion", {"similarity_type": "dmax"}, "chenfusion", 1),
         ("EarlyFusion", {}, "ef", 3),
         ("EarlyFusion", {"similarity_type": "early"}, "ef", 3),
         ("EarlyFusion", {"similarity_type": "mfccs"}, "ef", 0),
         ("EarlyFusion", {"similarity_type": "chromas"}, "ef", 2)]
SECTION_CASES = [c for c in CASES if c[3] != 1]
IDS = lambda c: "%s-%s" % (c[0], c[1].get("similarity_type")) if isinstance(c, tuple) else None


@pytest.fixture
def make(tmp_path, monkeypatch):
    """make(cls_name, **attributes) -> (object over N injected tracks whose context is a RecordingCtx with the pool 'uploaded',
    that context, Q well-formed new tracks)."""
    from acoss_amd import _lib, algorithms
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a context was created")))
    made = []

    def _make(cls_name, blocks=None, long=False, **attrs):
        algo = getattr(algorithms, cls_name)(H.csv(tmp_path, N), "feat/", shortname="al")
        tracks = H.tracks(cls_name, N + Q)
        if cls_name in SERRA:
            algo.set_pooled_features(tracks[:N])
            algo._pooled_len = H.lengths(N)
        else:
            algo.set_block_features(tracks[:N])
        for k, v in attrs.items():
            setattr(algo, k, v)
        ctx = H.RecordingCtx(blocks, long)
        monkeypatch.setattr(algo, "_context", lambda: ctx)
        algo._ctx, algo._pool_ready = ctx, True
        made.append(algo)
        return algo, ctx, tracks[N:]
    yield _make
    for algo in made:
        algo._ctx = None
        algo.cleanup_memmap()


# ---------------------------------------------------------------------- what the class must make of the library's records
def expected_rows(algo, al, pairs, T=None):
    """The class's rows for the library's records `al` of `pairs`, one record at a time from the documented formulas.
    T: the pooled lengths an index may name (Serra09 / ChenFusion)."""
    al, pairs = np.asarray(al), np.asarray(pairs).reshape(-1, 2)
    out = np.zeros(len(al), ALIGN_DTYPE)
    for k, r in enumerate(al):
        out[k]["score"] = r["score"]
        for f in ("q0", "r0", "q1", "r1"):
            out[k][f] = r[f]
        if r["q0"] < 0:
            assert tuple(r) == H.NO_MATCH
            out[k]["q_span"] = out[k]["r_span"] = -1
            continue
        for side, col in (("q", 0), ("r", 1)):
            if T is not None:       # [tau q0, min(tau (q1 + m - 1), T - 1)]
                span = [algo.tau * int(r[side + "0"]), min(algo.tau * (int(r[side + "1"]) + algo.m - 1), int(T[pairs[k, col]]) - 1)]
            else:                   # [q0, q1 + blocksize - 1], unclipped
                span = [int(r[side + "0"]), int(r[side + "1"]) + algo.blocksize - 1]
            out[k][side + "_span"] = span
    return out


def same_rows(got, exp):
    assert isinstance(got, np.ndarray) and got.dtype == ALIGN_DTYPE and got.shape == exp.shape
    for f in ALIGN_DTYPE.names:
        assert np.array_equal(got[f], exp[f]), f
    return True


def same_paths(got, exp):
    assert isinstance(got, list) and len(got) == len(exp)
    for g, e in zip(got, exp):
        assert isinstance(g, np.ndarray) and g.dtype == np.int32 and g.ndim == 2 and g.shape[1] == 2 and np.array_equal(g, e)
    return True


def path_list(off, cells):
    return [cells[off[k]:off[k + 1]] for k in range(len(off) - 1)]


def T_of(cls_name, n=N):
    return H.lengths(n) if cls_name in SERRA else None


def expected_call(algo, family, plane, paths, pairs, long=False):
    """(the context's method, its arguments by name) for a records / paths call."""
    pairs = np.asarray(pairs).reshape(-1, 2).tolist()
    if family == "ef":
        return ("ef_align_long" if long else "ef_align"), dict(pairs=pairs, kappa=algo.kappa, K=algo.K, plane=plane, paths=paths)
    args = dict(pairs=pairs, params=dict(m=algo.m, tau=algo.tau, kappa=pytest.approx(algo.kappa), oti=int(algo.oti), dmax=0))
    if family == "chenfusion":
        args["plane"] = plane
    return family + ("_align_paths" if paths else "_align"), args


def expected_sections_call(algo, family, plane, paths, pairs, opts):
    pairs = np.asarray(pairs).reshape(-1, 2).tolist()
    o = dict(zip(("max_sections", "min_score", "min_ratio", "pad"), opts))
    if family == "ef":
        return "ef_align_sections", dict(pairs=pairs, kappa=algo.kappa, K=algo.K, plane=plane, opts=o, paths=paths)
    return "serra09_align_sections", dict(pairs=pairs, params=dict(m=algo.m, tau=algo.tau, kappa=pytest.approx(algo.kappa), oti=int(algo.oti), dmax=0),
                                          opts=o, paths=paths)


PAIRS = np.array([[0, 1], [3, 3], [4, 0], [2, 4], [1, 0], [0, 2]])           # canned: hit, no match, clipped, short, hit, no match
QUERIES = [0, 3, 2]
INDICES = np.array([[1, -1, 4], [-1, -1, -1], [0, 2, -1]])                  # an all-empty row; filled: (0, 1) (0, 4) (2, 0) (2, 2)
MATCH_PAIRS = [[0, 1], [0, 4], [2, 0], [2, 2]]
MATCH_AT = [(0, 0), (0, 2), (2, 0), (2, 1)]


def serra_variants(cls_name):
    return [dict(tau=tau, m=m) for tau in (1, 2) for m in (1, 9)] if cls_name in SERRA else [dict(blocksize=20), dict(blocksize=3)]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_align_and_align_paths(make, case):
    cls_name, kw, family, plane = case
    for attrs in serra_variants(cls_name):
        for long in ((False, True) if family == "ef" else (False,)):
            algo, ctx, _ = make(cls_name, long=long, **attrs)
            al = H.canned_records(len(PAIRS))
            exp = expected_rows(algo, al, PAIRS, T_of(cls_name))
            if cls_name in SERRA:           # the canned records hold a span that is clipped and one that is not
                clipped = exp["q_span"][:, 1] == H.lengths(N)[PAIRS[:, 0]] - 1
                assert clipped[exp["q0"] >= 0].any() and not clipped[exp["q0"] >= 0].all()
            else:
                assert exp["q_span"][0].tolist() == [2, 20 + algo.blocksize - 1] and exp["r_span"][2].tolist() == [5, 70 + algo.blocksize - 1]
            assert (exp[1]["q0"], exp[1]["q_span"].tolist(), exp[1]["r_span"].tolist(), exp[1]["score"]) == (-1, [-1, -1], [-1, -1], 0)
            got = algo.align(PAIRS, **kw)
            assert ctx.calls == [expected_call(algo, family, plane, False, PAIRS, long)]
            assert same_rows(got, exp)
            got, paths = algo.align_paths(PAIRS.tolist(), **kw)
            assert ctx.calls[1:] == [expected_call(algo, family, plane, True, PAIRS, long)]
            assert same_rows(got, exp) and same_paths(paths, path_list(*H.canned_paths(al)))
            assert paths[1].shape == (0, 2) and paths[3].shape == (4, 2)
            # empty input: no call
            for empty in ([], np.zeros((0, 2), np.int32)):
                got = algo.align(empty, **kw)
                assert same_rows(got, np.zeros(0, ALIGN_DTYPE))
                got, paths = algo.align_paths(empty, **kw)
                assert same_rows(got, np.zeros(0, ALIGN_DTYPE)) and paths == []
            assert len(ctx.calls) == 2 and ctx.asked == (2 if family == "ef" else 0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_align_matches_and_align_match_paths(make, case):
    cls_name, kw, family, plane = case
    for attrs in serra_variants(cls_name)[1:3]:
        for long in ((False, True) if family == "ef" else (False,)):
            algo, ctx, _ = make(cls_name, long=long, **attrs)
            al = H.canned_records(4)
            rows = expected_rows(algo, al, MATCH_PAIRS, T_of(cls_name))
            exp = np.zeros((3, 3), ALIGN_DTYPE)
            for f in ("q0", "r0", "q1", "r1", "q_span", "r_span"):
                exp[f] = -1
            exp_paths = [[np.zeros((0, 2), np.int32) for _ in range(3)] for _ in range(3)]
            for t, (r, s) in enumerate(MATCH_AT):
                exp[r, s] = rows[t]
                exp_paths[r][s] = path_list(*H.canned_paths(al))[t]
            got = algo.align_matches(QUERIES, INDICES, **kw)
            assert ctx.calls == [expected_call(algo, family, plane, False, MATCH_PAIRS, long)]
            assert same_rows(got, exp)
            got, paths = algo.align_match_paths(np.array(QUERIES), INDICES.tolist(), **kw)
            assert ctx.calls[1:] == [expected_call(algo, family, plane, True, MATCH_PAIRS, long)]
            assert same_rows(got, exp)
            assert isinstance(paths, list) and len(paths) == 3 and all(same_paths(p, e) for p, e in zip(paths, exp_paths))
            assert paths[0][1].shape == (0, 2) and paths[0][1].dtype == np.int32 and paths[0][2].shape == (0, 2) and paths[2][1].shape == (4, 2)
            # nothing but empty slots, and no queries at all: no call
            none = np.full((2, 3), -1)
            got = algo.align_matches([1, 2], none, **kw)
            assert same_rows(got, exp[1:2].repeat(2, axis=0))
            got, paths = algo.align_match_paths([1, 2], none, **kw)
            assert same_rows(got, exp[1:2].repeat(2, axis=0)) and [[p.shape for p in row] for row in paths] == [[(0, 2)] * 3] * 2
            got = algo.align_matches([], np.zeros((0, 3), np.int32), **kw)
            assert same_rows(got, np.zeros((0, 3), ALIGN_DTYPE))
            got, paths = algo.align_match_paths([], np.zeros((0, 3), np.int32), **kw)
            assert same_rows(got, np.zeros((0, 3), ALIGN_DTYPE)) and paths == []
            assert len(ctx.calls) == 2


def expected_sections(algo, cls_name, pairs, S, T=None):
    """-> (the list of (n_k,) arrays, the list of lists of paths) for the canned sections of `pairs`."""
    al, n, off, cells = H.canned_sections(len(pairs), S)
    T = T_of(cls_name) if T is None and cls_name in SERRA else T
    sections = [expected_rows(algo, al[k, :n[k]], np.repeat(np.asarray(pairs)[k:k + 1], n[k], axis=0), T) for k in range(len(pairs))]
    return sections, [[cells[off[k * S + s]:off[k * S + s + 1]] for s in range(n[k])] for k in range(len(pairs))]


def same_sections(got, exp):
    assert isinstance(got, list) and len(got) == len(exp)
    return all(same_rows(g, e) for g, e in zip(got, exp))


@pytest.mark.parametrize("case", SECTION_CASES, ids=IDS)
def test_align_sections(make, case):
    cls_name, kw, family, plane = case
    pairs = PAIRS[:5]
    for attrs in serra_variants(cls_name)[1:3]:
        algo, ctx, _ = make(cls_name, blocks=np.arange(5, 5 + N), **attrs)
        # the defaults: four sections, min_score 2, min_ratio 0, pad 0, no paths
        exp, exp_paths = expected_sections(algo, cls_name, pairs, 4)
        assert [len(e) for e in exp] == [0, 1, 2, 0, 1] and exp[2]["q0"].tolist() == [4, 2]
        got = algo.align_sections(pairs, **kw)
        assert ctx.calls == [expected_sections_call(algo, family, plane, False, pairs, (4, 2.0, 0.0, 0))]
        assert same_sections(got, exp)
        # by keyword, with the paths; one section at most
        got = algo.align_sections(pairs.tolist(), max_sections=1, min_score=2.5, min_ratio=0.5, pad=3, paths=True, **kw)
        assert ctx.calls[1:] == [expected_sections_call(algo, family, plane, True, pairs, (1, 2.5, 0.5, 3))]
        exp, exp_paths = expected_sections(algo, cls_name, pairs, 1)
        assert isinstance(got, tuple) and len(got) == 2 and same_sections(got[0], exp)
        assert all(same_paths(g, e) for g, e in zip(got[1], exp_paths)) and [len(p) for p in got[1]] == [0, 1, 1, 0, 1]
        # by position, in the class's own order
        args = (3, 4.0, 0.25, 1, 1)
        pos = ((kw["similarity_type"],) if "similarity_type" in kw else ("early",)) + args if family == "ef" else args
        got = algo.align_sections(pairs, *pos, **({} if family == "ef" else kw))
        assert ctx.calls[2:] == [expected_sections_call(algo, family, plane, True, pairs, (3, 4.0, 0.25, 1))]
        exp, exp_paths = expected_sections(algo, cls_name, pairs, 3)
        assert same_sections(got[0], exp) and all(same_paths(g, e) for g, e in zip(got[1], exp_paths))
        assert [p.shape for p in got[1][2]] == [(1, 2), (2, 2)]
        # empty input: no call
        assert algo.align_sections([], **kw) == [] and algo.align_sections(np.zeros((0, 2), np.int64), paths=True, **kw) == ([], [])
        assert len(ctx.calls) == 3


@pytest.mark.parametrize("case", SECTION_CASES, ids=IDS)
def test_align_match_sections(make, case):
    cls_name, kw, family, plane = case
    for attrs in serra_variants(cls_name)[1:3]:
        algo, ctx, _ = make(cls_name, blocks=np.arange(5, 5 + N), **attrs)
        sec, sec_paths = expected_sections(algo, cls_name, MATCH_PAIRS, 4)
        got = algo.align_match_sections(QUERIES, INDICES, **kw)
        assert ctx.calls == [expected_sections_call(algo, family, plane, False, MATCH_PAIRS, (4, 2.0, 0.0, 0))]
        assert isinstance(got, list) and [len(row) for row in got] == [3, 3, 3]
        for r in range(3):
            for s in range(3):
                t = MATCH_AT.index((r, s)) if (r, s) in MATCH_AT else None
                assert same_rows(got[r][s], np.zeros(0, ALIGN_DTYPE) if t is None else sec[t])
        args = (2, 3.0, 1.0, 5, True)
        pos = ((kw["similarity_type"],) if "similarity_type" in kw else ("early",)) + args if family == "ef" else args
        got = algo.align_match_sections(QUERIES, INDICES, *pos, **({} if family == "ef" else kw))
        assert ctx.calls[1:] == [expected_sections_call(algo, family, plane, True, MATCH_PAIRS, (2, 3.0, 1.0, 5))]
        sec, sec_paths = expected_sections(algo, cls_name, MATCH_PAIRS, 2)
        assert isinstance(got, tuple) and len(got) == 2 and [len(row) for row in got[1]] == [3, 3, 3]
        for r in range(3):
            for s in range(3):
                t = MATCH_AT.index((r, s)) if (r, s) in MATCH_AT else None
                assert same_rows(got[0][r][s], np.zeros(0, ALIGN_DTYPE) if t is None else sec[t])
                assert got[1][r][s] == [] if t is None else same_paths(got[1][r][s], sec_paths[t])
        assert [len(p) for p in got[1][2]] == [2, 0, 0] and [len(p) for p in got[1][0]] == [0, 0, 1]
        # nothing but empty slots, and no queries: no call
        got = algo.align_match_sections([1], [[-1, -1]], paths=True, **kw)
        assert [[g.shape for g in row] for row in got[0]] == [[(0,), (0,)]] and got[0][0][0].dtype == ALIGN_DTYPE and got[1] == [[[], []]]
        assert algo.align_match_sections([], np.zeros((0, 2), np.int32), **kw) == []
        assert algo.align_match_sections([], np.zeros((0, 2), np.int32), paths=True, **kw) == ([], [])
        assert len(ctx.calls) == 2


def test_earlyfusion_sections_for_a_pool_the_context_did_not_see(make):
    """ef_has_long_track() answers True for such a pool: the sections call goes to the library, which refuses a long track itself."""
    algo, ctx, _ = make("EarlyFusion", blocks=None, long=True)
    got = algo.align_sections(PAIRS[:2])
    assert ctx.calls == [expected_sections_call(algo, "ef", 3, False, PAIRS[:2], (4, 2.0, 0.0, 0))] and [len(g) for g in got] == [0, 1]


# ---------------------------------------------------------------------- inside a session
@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion", "EarlyFusion"])
def test_spans_inside_a_session(make, cls_name):
    """Indices in [0, N + Q); Serra09's spans clip to the session's pooled lengths behind the collection's."""
    algo, ctx, new = make(cls_name, **(dict(tau=1, m=1) if cls_name in SERRA else {}))
    pairs = np.array([[N + 1, 0], [N, N], [0, N + 1]])
    with algo.appended(new) as s:
        if cls_name in SERRA:
            assert algo._track_lengths().tolist() == H.lengths(N + Q).tolist()
        exp = expected_rows(algo, H.canned_records(3), pairs, T_of(cls_name, N + Q))
        got = algo.align(pairs)
        assert same_rows(got, exp)
        if cls_name in SERRA:       # HITS[1] ends at (60, 70): row 60 - 1 + 1 is beyond track N + Q - 1 (58 frames) as well
            assert exp[2]["q_span"].tolist() == [0, 39] and exp[2]["r_span"].tolist() == [5, 57]
        got = algo.align_matches(s.indices, [[0, -1], [N, 1]])
        assert ctx.calls[-1][1]["pairs"] == [[N, 0], [N + 1, N], [N + 1, 1]]
        rows = expected_rows(algo, H.canned_records(3), ctx.calls[-1][1]["pairs"], T_of(cls_name, N + Q))
        assert same_rows(got[[0, 1, 1], [0, 0, 1]], rows) and got[0, 1]["q0"] == -1
        secs = algo.align_sections(pairs)
        assert same_sections(secs, expected_sections(algo, cls_name, pairs, 4, T_of(cls_name, N + Q))[0])
    assert ctx.session == [("append", Q), ("truncate", N)]
    with pytest.raises(ValueError, match=r"^align: idxs must be track indices in \[0, %d\)$" % N):
        algo.align(pairs)


# ---------------------------------------------------------------------- every refusal, before the first library call
def raises(exc, text):
    return pytest.raises(exc, match="^" + re.escape(text) + "$")


PAIR_METHODS = ("align", "align_paths", "align_sections")
MATCH_METHODS = ("align_matches", "align_match_paths", "align_match_sections")


@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion", "EarlyFusion"])
def test_index_refusals(make, cls_name):
    algo, ctx, new = make(cls_name)
    for who in PAIR_METHODS:
        fn = getattr(algo, who)
        with raises(ValueError, "%s: track indices must be integers, got dtype float64" % who):
            fn(np.array([[0.0, 1.0]]))
        for bad in (np.arange(3), np.zeros((2, 3), np.int32), np.zeros((1, 2, 2), np.int32)):
            with raises(ValueError, "%s: idxs must be (K, 2) (query, reference) track indices, got shape %s" % (who, bad.shape)):
                fn(bad)
        for bad in ([[0, N]], [[-1, 0]]):
            with raises(ValueError, "%s: idxs must be track indices in [0, %d)" % (who, N)):
                fn(bad)
    for who in MATCH_METHODS:
        fn = getattr(algo, who)
        with raises(ValueError, "%s: track indices must be integers, got dtype float64" % who):
            fn([0.5], [[1]])
        with raises(ValueError, "%s: track indices must be integers, got dtype float64" % who):
            fn([0], [[1.0]])
        for bad in (np.zeros(2, np.int32), np.zeros((1, 2), np.int32), np.zeros((2, 1, 1), np.int32)):
            with raises(ValueError, "%s: indices must be (Q, k) with one row per query (2), got shape %s" % (who, bad.shape)):
                fn([0, 1], bad)
        for bad in ([N], [-1]):
            with raises(ValueError, "%s: queries must be track indices in [0, %d)" % (who, N)):
                fn(bad, [[0, 1]])
        for bad in ([[0, N]], [[-2, 0]]):
            with raises(ValueError, "%s: indices must be track indices in [0, %d) or -1" % (who, N)):
                fn([0], bad)
    with algo.appended(new) as s:
        with raises(ValueError, "align: idxs must be track indices in [0, %d)" % s.total):
            algo.align([[0, s.total]])
        with raises(ValueError, "align_matches: queries must be track indices in [0, %d)" % s.total):
            algo.align_matches([s.total], [[0]])
    assert ctx.calls == [] and ctx.asked == 0


@pytest.mark.parametrize("cls_name", ["ChenFusion", "EarlyFusion"])
def test_similarity_type_refusals(make, cls_name):
    algo, ctx, _ = make(cls_name)
    planes = list(algo._identify_planes)
    for who in PAIR_METHODS + MATCH_METHODS:
        args = ([[0, 1]],) if who in PAIR_METHODS else ([0], [[1]])
        for bad in ("nope", 3):
            with raises(ValueError, "%s: unknown similarity type %r; similarity_type must be one of %s" % (who, bad, planes)):
                getattr(algo, who)(*args, similarity_type=bad)
        for fused in algo._identify_fused:
            with raises(ValueError, "%s: '%s' is fused from whole score matrices and has no alignment of its own; similarity_type must be one of %s"
                        % (who, fused, planes)):
                getattr(algo, who)(*args, similarity_type=fused)
        # ... before the indices are looked at
        with raises(ValueError, "%s: unknown similarity type 'nope'; similarity_type must be one of %s" % (who, planes)):
            getattr(algo, who)(*(([[0, N]],) if who in PAIR_METHODS else ([N], [[1]])), similarity_type="nope")
    assert algo._identify_fused and ctx.calls == [] and ctx.asked == 0


def test_serra09_type_refusal_of_the_one_call_forms(make):
    algo, ctx, new = make("Serra09")
    for who in ("align_tracks", "align_track_paths"):
        with raises(ValueError, "%s: unknown similarity type 'qmax'; similarity_type must be one of ['main']" % who):
            getattr(algo, who)(new, np.zeros((Q, 1), np.int32), similarity_type="qmax")
    with raises(ValueError, "locate_tracks: unknown similarity type 'qmax'; similarity_type must be one of ['main']"):
        algo.locate_tracks(new, similarity_type="qmax")
    assert ctx.calls == [] and ctx.session == []


@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion"])
def test_dmax_engine_refusal(make, cls_name):
    """Serra09's alignment is the Qmax one: with engine dmax set the scores are Dmax's and align*() refuses -- ChenFusion's plane 0
    likewise, its plane 1 (which does not read the switch) not."""
    algo, ctx, new = make(cls_name, _engine={"dmax": 1})
    for kw in ({},) if cls_name == "Serra09" else ({}, {"similarity_type": "qmax"}):
        for who in PAIR_METHODS + MATCH_METHODS:
            with raises(ValueError, "%s: the Qmax alignment only (engine dmax must be 0)" % who):
                getattr(algo, who)(*(([[0, N]],) if who in PAIR_METHODS else ([N], [[1.5]])), **kw)       # (before the indices)
        for who in ("align_tracks", "align_track_paths", "locate_tracks"):
            with raises(ValueError, "%s: the Qmax alignment only (engine dmax must be 0)" % who):
                getattr(algo, who)(new, *(() if who == "locate_tracks" else (np.zeros((Q, 1), np.int32),)), **kw)
    assert ctx.calls == [] and ctx.session == []
    if cls_name == "ChenFusion":
        kw = {"similarity_type": "dmax"}
        algo.align([[0, 1]], **kw), algo.align_paths([[0, 1]], **kw), algo.align_matches([0], [[1]], **kw), algo.align_match_paths([0], [[1]], **kw)
        assert [c[0] for c in ctx.calls] == ["chenfusion_align", "chenfusion_align_paths"] * 2
        assert all(c[1]["plane"] == 1 and c[1]["params"]["dmax"] == 1 for c in ctx.calls)
        algo.align_tracks(new, np.zeros((Q, 1), np.int32), **kw)
        assert ctx.calls[-1][0] == "chenfusion_align" and ctx.session == [("append", Q), ("truncate", N)]


def test_chenfusion_sections_are_qmax_only(make):
    algo, ctx, _ = make("ChenFusion")
    for who, args in (("align_sections", ([[0, 1]],)), ("align_match_sections", ([0], [[1]]))):
        with raises(ValueError, "%s: the sections are those of the Qmax alignment; similarity_type must be 'qmax', got 'dmax'" % who):
            getattr(algo, who)(*args, similarity_type="dmax")
        with raises(ValueError, "%s: the sections are those of the Qmax alignment; similarity_type must be 'qmax', got 'dmax'" % who):
            getattr(algo, who)(*args, max_sections=0, similarity_type="dmax")
    assert ctx.calls == []


BAD_OPTIONS = [(dict(max_sections=0), "max_sections must be in [1, 16], got 0"), (dict(max_sections=17), "max_sections must be in [1, 16], got 17"),
               (dict(max_sections=2.0), "max_sections must be an integer, got 2.0"), (dict(max_sections=True), "max_sections must be an integer, got True"),
               (dict(pad=-1), "pad must be >= 0, got -1"), (dict(pad=1.5), "pad must be an integer, got 1.5"),
               (dict(min_score=1.0), "min_score must be > 1 (a section has at least two cells), got 1.0"),
               (dict(min_score=float("nan")), "min_score must be > 1 (a section has at least two cells), got nan"),
               (dict(min_ratio=-0.5), "min_ratio must be in [0, 1], got -0.5"), (dict(min_ratio=1.25), "min_ratio must be in [0, 1], got 1.25")]


@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion", "EarlyFusion"])
def test_section_option_refusals(make, cls_name):
    algo, ctx, _ = make(cls_name, blocks=np.arange(5, 5 + N))
    for who, args in (("align_sections", ([[0, 1]],)), ("align_match_sections", ([0], [[1, -1]]))):
        for kw, text in BAD_OPTIONS:
            with raises(ValueError, "%s: %s" % (who, text)):
                getattr(algo, who)(*args, **kw)
            with raises(ValueError, "%s: %s" % (who, text)):
                getattr(algo, who)(*args, paths=True, **kw)
    assert ctx.calls == [] and ctx.asked == 0


def test_earlyfusion_sections_refuse_a_long_track(make):
    algo, ctx, _ = make("EarlyFusion", blocks=np.array([5, 6, 2000, 8, 9]), long=True)
    text = "%s: sections need the bit path: tracks of at most 1024 blocks (align() serves longer ones)"
    for paths in (False, True):
        with raises(NotImplementedError, text % "align_sections"):
            algo.align_sections([[0, 2]], paths=paths)
        with raises(NotImplementedError, text % "align_match_sections"):
            algo.align_match_sections([2], [[-1, 1]], "ssms", paths=paths)
    assert ctx.calls == [] and ctx.asked == 4
    # the options and the indices come first, and an empty list names no long track
    with raises(ValueError, "align_sections: pad must be >= 0, got -1"):
        algo.align_sections([[0, 2]], pad=-1)
    with raises(ValueError, "align_sections: idxs must be track indices in [0, %d)" % N):
        algo.align_sections([[0, N]])
    assert algo.align_sections([]) == [] and [len(g) for g in algo.align_match_sections([2], [[-1]])[0]] == [0]
    assert ctx.calls == [] and ctx.asked == 4


# ---------------------------------------------------------------------- the one-call forms above the class methods
IDX = np.array([[1, -1, 4], [0, 2, -1]], np.int32)                         # what identify() lists for the Q new tracks
SCORE = np.array([[3.0, np.nan, 1.0], [2.0, 1.5, np.nan]], np.float32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_align_tracks_and_align_track_paths(make, case):
    cls_name, kw, family, plane = case
    algo, ctx, new = make(cls_name)
    pairs = [[N, 1], [N, 4], [N + 1, 0], [N + 1, 2]]
    with algo.appended(new) as s:
        exp = algo.align_matches(s.indices, IDX, **kw)
        exp_paths = algo.align_match_paths(s.indices, IDX, **kw)[1]
    del ctx.calls[:], ctx.session[:]
    got = algo.align_tracks(new, IDX, **kw)
    assert ctx.calls == [expected_call(algo, family, plane, False, pairs)] and ctx.session == [("append", Q), ("truncate", N)]
    assert same_rows(got, exp) and same_rows(exp[[0, 0, 1, 1], [0, 2, 0, 1]], expected_rows(algo, H.canned_records(4), pairs, T_of(cls_name, N + Q)))
    got, paths = algo.align_track_paths(new, IDX, **kw)
    assert ctx.calls[1:] == [expected_call(algo, family, plane, True, pairs)] and ctx.session == [("append", Q), ("truncate", N)] * 2
    assert same_rows(got, exp) and all(same_paths(p, e) for p, e in zip(paths, exp_paths))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_locate_tracks(make, case, monkeypatch):
    """idx / score from identify() over the session's tracks, then align_matches / align_match_paths of (new track, hit) -- EarlyFusion:
    align / align_paths of (hit, new track), the pair the listed score belongs to."""
    cls_name, kw, family, plane = case
    algo, ctx, new = make(cls_name)
    t = kw.get("similarity_type", {"Serra09": "main", "ChenFusion": "qmax", "EarlyFusion": "early"}[cls_name])
    asked = []

    def identify(queries, k=10, candidates=None, similarity_types=None):
        asked.append((np.asarray(queries).tolist(), k, np.asarray(candidates).tolist(), similarity_types, algo._n_tracks()))
        return {t: (IDX.copy(), SCORE.copy())}
    monkeypatch.setattr(algo, "identify", identify)
    if family == "ef":
        pairs = [[1, N], [4, N], [0, N + 1], [2, N + 1]]
    else:
        pairs = [[N, 1], [N, 4], [N + 1, 0], [N + 1, 2]]
    rows = expected_rows(algo, H.canned_records(4), pairs, T_of(cls_name, N + Q))
    got = algo.locate_tracks(new, k=3, **kw)
    assert asked == [([N, N + 1], 3, list(range(N)), [t], N + Q)]
    assert ctx.calls == [expected_call(algo, family, plane, False, pairs)] and ctx.session == [("append", Q), ("truncate", N)]
    assert len(got) == 3 and np.array_equal(got[0], IDX) and np.array_equal(got[1], SCORE, equal_nan=True)
    assert got[2].shape == (Q, 3) and same_rows(got[2][[0, 0, 1, 1], [0, 2, 0, 1]], rows)
    assert got[2][0, 1]["q0"] == -1 and got[2][1, 2]["r_span"].tolist() == [-1, -1]
    got = algo.locate_tracks(new, k=3, candidates=[0, 2], paths=True, **kw)
    assert asked[1:] == [([N, N + 1], 3, [0, 2], [t], N + Q)]
    assert ctx.calls[1:] == [expected_call(algo, family, plane, True, pairs)]
    assert len(got) == 4 and same_rows(got[2][[0, 0, 1, 1], [0, 2, 0, 1]], rows)
    al = H.canned_records(4)
    flat = [got[3][r][s] for r, s in ((0, 0), (0, 2), (1, 0), (1, 1))]
    assert same_paths(flat, path_list(*H.canned_paths(al))) and got[3][0][1].shape == (0, 2) and got[3][1][2].shape == (0, 2)


# ---------------------------------------------------------------------- what changed when the six methods became one body each
def test_accepted_consequences_of_the_shared_methods(make):
    """NOT part of the pinned behaviour: the three differences the shared methods brought, and nothing else.
    1. Serra09's methods take similarity_type as the other classes' do: None or 'main', anything else is an unknown type.
    2. An explicit similarity_type=None means the class's default in ChenFusion and EarlyFusion too.
    3. The sections methods of every class check the similarity type, then the options, then the indices."""
    algo, ctx, _ = make("Serra09")
    for st in (None, "main"):
        algo.align(PAIRS, similarity_type=st), algo.align_paths(PAIRS, similarity_type=st)
        algo.align_matches(QUERIES, INDICES, similarity_type=st), algo.align_match_paths(QUERIES, INDICES, st)
        algo.align_sections(PAIRS, similarity_type=st), algo.align_match_sections(QUERIES, INDICES, similarity_type=st)
    assert [c[0] for c in ctx.calls] == ["serra09_align", "serra09_align_paths"] * 2 + ["serra09_align_sections"] * 2 \
        + ["serra09_align", "serra09_align_paths"] * 2 + ["serra09_align_sections"] * 2
    del ctx.calls[:]
    for who in PAIR_METHODS + MATCH_METHODS:
        with raises(ValueError, "%s: unknown similarity type 'qmax'; similarity_type must be one of ['main']" % who):
            getattr(algo, who)(*(([[0, N]],) if who in PAIR_METHODS else ([N], [[1]])), similarity_type="qmax")
    assert ctx.calls == []
    for cls_name, family, plane in (("ChenFusion", "serra09", None), ("EarlyFusion", "ef", 3)):
        algo, ctx, _ = make(cls_name, blocks=np.arange(5, 5 + N))
        algo.align(PAIRS, None), algo.align_paths(PAIRS, None), algo.align_matches(QUERIES, INDICES, None)
        algo.align_match_paths(QUERIES, INDICES, None)
        algo.align_sections(PAIRS, similarity_type=None), algo.align_match_sections(QUERIES, INDICES, similarity_type=None)
        assert ctx.calls[:2] == [expected_call(algo, family, plane, False, PAIRS), expected_call(algo, family, plane, True, PAIRS)]
        assert ctx.calls[2:4] == [expected_call(algo, family, plane, False, MATCH_PAIRS), expected_call(algo, family, plane, True, MATCH_PAIRS)]
        assert ctx.calls[4:] == [expected_sections_call(algo, family, plane, False, PAIRS, (4, 2.0, 0.0, 0)),
                                 expected_sections_call(algo, family, plane, False, MATCH_PAIRS, (4, 2.0, 0.0, 0))]
    for cls_name in ("Serra09", "ChenFusion", "EarlyFusion"):
        algo, ctx, _ = make(cls_name)
        with raises(ValueError, "align_sections: pad must be >= 0, got -1"):
            algo.align_sections([[0, N]], pad=-1)
        with raises(ValueError, "align_match_sections: pad must be >= 0, got -1"):
            algo.align_match_sections([N], [[0.5]], pad=-1)
        assert ctx.calls == []
