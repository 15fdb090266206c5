"""
Host-side checks of appended() sessions and their one-call forms (align_tracks / align_track_paths / locate_tracks): every
argument error comes before the library call it guards, and a session leaves the object exactly as it found it.  No GPU: the
class's libacx context is a fake that records the append and the truncate and fails the test on any other use.
"""
import copy

import numpy as np
import pytest

CLASSES = ["Serra09", "ChenFusion", "Simple", "EarlyFusion", "FTM2D"]
N, Q = 8, 3


class _Reached(Exception):
    """The fake library was called: every Python-side check before that call has passed."""


class _FakeCtx(object):
    """Stands where the class's libacx context would be.  calls: ("append", n_new) / ("truncate", n_tracks), in order."""

    def __init__(self):
        self.calls = []

    def pool_append(self, frames, offsets):
        self.calls.append(("append", len(offsets) - 1))

    def pool_append_raw(self, raw, raw_offsets, fac=40):
        self.calls.append(("append", len(raw_offsets) - 1))
        return np.concatenate([[0], np.cumsum(-(-np.diff(raw_offsets) // fac))]).astype(np.int64)

    pool_append_f64 = pool_append

    def ef_pool_append(self, tracks):
        self.calls.append(("append", len(tracks)))

    def ftm2d_append_shingles(self, shingles):
        self.calls.append(("append", len(shingles)))

    def pool_truncate(self, algo, n_tracks):
        self.calls.append(("truncate", int(n_tracks)))

    def __getattr__(self, name):
        def call(*a, **k):
            raise _Reached(name)
        return call


def _csv(tmp_path, n):
    path = tmp_path / "ds.csv"
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


def _tracks(cls_name, n, seed=5):
    rng = np.random.default_rng(seed)
    if cls_name in ("Serra09", "ChenFusion"):
        return [rng.random((40 + 3 * i, 12)).astype(np.float32) for i in range(n)]
    if cls_name == "Simple":
        return [rng.random((12, 40 + i)) for i in range(n)]
    if cls_name == "EarlyFusion":
        return [dict(mfccs=rng.random((5 + i, 650)).astype(np.float32), ssms=rng.random((5 + i, 1225)).astype(np.float32),
                     chromas=rng.random((5 + i, 480)).astype(np.float32), chroma_med=rng.random(12)) for i in range(n)]
    return [rng.standard_normal(36) for _ in range(n)]


def _bad_track(cls_name):
    """-> (a list of tracks in a wrong format, the message's pattern)"""
    if cls_name in ("Serra09", "ChenFusion"):
        return [np.zeros((40, 11), np.float32)], r"\(T, 12\)"
    if cls_name == "Simple":
        return [np.zeros((40, 12))], r"\(12, n\)"
    if cls_name == "EarlyFusion":
        t = _tracks("EarlyFusion", 1)[0]
        return [dict(t, ssms=t["ssms"][:-1])], "same number of blocks"
    return [np.zeros(24)], r"\(36,\) shingle"


def _cache(algo):
    """The feature cache of the class (the dict its set_* method fills)."""
    for name in ("all_block_feats", "shingles", "all_feats"):
        if hasattr(algo, name):
            return getattr(algo, name)
    raise AssertionError("no feature cache")


@pytest.fixture
def make(tmp_path, monkeypatch):
    """make(cls_name) -> (object over N injected tracks whose context is a _FakeCtx with the pool 'uploaded', that context,
    Q well-formed new tracks)."""
    from acoss_amd import _lib, algorithms
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a context was created")))
    made = []

    def _make(cls_name):
        cls = getattr(algorithms, cls_name)
        algo = cls(_csv(tmp_path, N), "feat/", shortname="sess", **(dict(WIN=3) if cls_name == "FTM2D" else {}))
        tracks = _tracks(cls_name, N + Q)
        labels = ["w%d" % (i // 2) for i in range(N)]
        if cls_name in ("Serra09", "ChenFusion"):
            algo.set_pooled_features(tracks[:N], labels)
            algo._pooled_len = np.array([len(t) for t in tracks[:N]], np.int64)
        elif cls_name == "EarlyFusion":
            algo.set_block_features(tracks[:N], labels)
        else:
            algo.set_features(tracks[:N], labels)
        algo._ctx, algo._pool_ready = _FakeCtx(), True
        made.append(algo)
        return algo, algo._ctx, tracks[N:]
    yield _make
    for algo in made:
        algo._ctx = None
        algo.cleanup_memmap()


def test_session_object_and_bound(make):
    algo, ctx, new = make("Serra09")
    assert algo._n_tracks() == N
    with algo.appended(new) as s:
        assert s.first == N and s.count == Q and s.total == N + Q and algo.N == N
        assert s.indices.dtype == np.int32 and s.indices.tolist() == list(range(N, N + Q))
        assert algo._n_tracks() == N + Q
        assert algo._track_lengths().tolist() == algo._pooled_len.tolist() + [len(t) for t in new]
        assert ctx.calls == [("append", Q)]
    assert algo._n_tracks() == N and ctx.calls == [("append", Q), ("truncate", N)]
    with pytest.raises(ValueError, match=r"\[0, %d\)" % N):
        algo.identify([N])


def test_raw_session_takes_the_librarys_lengths(make):
    algo, ctx, _ = make("Serra09")
    algo.downsample_fac = 4
    raw = [np.zeros((T0, 12), np.float32) for T0 in (203, 240, 9)]
    with algo.appended(raw, raw=True):
        assert algo._track_lengths()[N:].tolist() == [51, 60, 3]
    assert ctx.calls == [("append", 3), ("truncate", N)]


@pytest.mark.parametrize("cls_name", CLASSES)
def test_argument_errors_before_the_append(make, cls_name):
    algo, ctx, new = make(cls_name)
    bad, pattern = _bad_track(cls_name)
    with pytest.raises(ValueError, match=pattern):
        algo.appended(bad)
    with pytest.raises(ValueError, match="at least one track"):
        algo.appended([])
    for labels in (["a"] * (Q - 1), ["a"] * (Q + 1)):
        with pytest.raises(ValueError, match=r"one clique label per track \(%d\)" % Q):
            algo.appended(new, labels=labels)
    if cls_name == "FTM2D":
        for fn in (algo.align_tracks, algo.align_track_paths):
            with pytest.raises(NotImplementedError, match="no alignment"):
                fn(new, np.zeros((Q, 2), np.int32))
        with pytest.raises(NotImplementedError, match="no alignment"):
            algo.locate_tracks(new)
    else:
        idx = np.zeros((Q, 2), np.int32)
        with pytest.raises(ValueError, match=pattern):
            algo.align_tracks(bad, idx[:1])
        with pytest.raises(ValueError, match=pattern):
            algo.locate_tracks(bad)
        with pytest.raises(ValueError, match=r"one row per query \(%d\)" % Q):
            algo.align_tracks(new, idx[:2])
        for entry in (N + Q, -2):
            with pytest.raises(ValueError, match=r"\[0, %d\) or -1" % (N + Q)):
                algo.align_tracks(new, np.full((Q, 2), entry, np.int32))
        with pytest.raises(ValueError, match="unknown similarity type"):
            algo.align_tracks(new, idx, similarity_type="nope")
        with pytest.raises(ValueError, match="unknown similarity type"):
            algo.locate_tracks(new, similarity_type="nope")
        for fused in algo._identify_fused:
            for call in (lambda: algo.locate_tracks(new, similarity_type=fused), lambda: algo.align_tracks(new, idx, similarity_type=fused)):
                with pytest.raises(ValueError, match="no alignment of its own"):
                    call()
        with pytest.raises(ValueError, match="k must be >= 1"):
            algo.locate_tracks(new, k=0)
        with pytest.raises(ValueError, match=r"candidates must be tracks of the collection, indices in \[0, %d\)" % N):
            algo.locate_tracks(new, candidates=[1, N])
        if cls_name == "Simple":
            with pytest.raises(NotImplementedError, match="no alignment paths"):
                algo.align_track_paths(new, idx)
            with pytest.raises(NotImplementedError, match="no alignment paths"):
                algo.locate_tracks(new, paths=True)
    assert ctx.calls == []


def _refused(cls_name, algo, new):
    """-> [(method name, a call of it with well-formed arguments)]"""
    main = list(algo.Ds)[0]
    pair = np.array([[0, 1]])
    calls = [("similarity", lambda: algo.similarity(pair)), ("all_pairwise", lambda: algo.all_pairwise()),
             ("getEvalStatistics", lambda: algo.getEvalStatistics(main)), ("top_matches", lambda: algo.top_matches(main, k=2)),
             ("identify_tracks", lambda: algo.identify_tracks(new)), ("score_tracks", lambda: algo.score_tracks(new)),
             ("rerank_tracks", lambda: algo.rerank_tracks(new, [[0]] * Q)), ("appended", lambda: algo.appended(new))]
    if cls_name in ("Serra09", "ChenFusion"):
        calls += [("normalize_by_length", algo.normalize_by_length), ("set_pooled_features", lambda: algo.set_pooled_features(_tracks(cls_name, N)))]
    if cls_name in ("ChenFusion", "EarlyFusion"):
        calls += [("do_late_fusion", algo.do_late_fusion)]
    if cls_name == "EarlyFusion":
        calls += [("set_block_features", lambda: algo.set_block_features(_tracks(cls_name, N)))]
    if cls_name in ("Simple", "FTM2D"):
        calls += [("set_features", lambda: algo.set_features(_tracks(cls_name, N)))]
    if cls_name != "FTM2D":
        calls += [("align_tracks", lambda: algo.align_tracks(new, np.zeros((Q, 1), np.int32))), ("locate_tracks", lambda: algo.locate_tracks(new))]
    return calls


@pytest.mark.parametrize("cls_name", CLASSES)
def test_refused_inside_a_session(make, cls_name):
    algo, ctx, new = make(cls_name)
    cache = _cache(algo)
    before = (id(cache), sorted(cache), copy.deepcopy(algo.cliques))
    with algo.appended(new):
        for name, call in _refused(cls_name, algo, new):
            with pytest.raises(RuntimeError, match=name):
                call()
        assert ctx.calls == [("append", Q)]
    assert ctx.calls == [("append", Q), ("truncate", N)]
    assert (id(_cache(algo)), sorted(_cache(algo)), algo.cliques) == before
    for t in algo.Ds:
        assert not np.any(np.asarray(algo.Ds[t]))


def _index_calls(cls_name, algo, i):
    """Every read-only method of the class with the track index i in each place an index can stand."""
    pair, q = np.array([[0, i]]), np.array([i])
    calls = [lambda: algo.identify(q), lambda: algo.identify([0], candidates=[1, i] if i > 1 else [i, 1]), lambda: algo.query_rows(q),
             lambda: algo.rerank([0], [[1, i]]), lambda: algo.rerank(q, [[1]]), lambda: algo.evaluate(queries=q)]
    if cls_name != "FTM2D":
        calls += [lambda: algo.align(pair), lambda: algo.align(pair[:, ::-1]), lambda: algo.align_matches(q, [[0]]),
                  lambda: algo.align_matches([0], [[i]])]
    if cls_name in ("Serra09", "ChenFusion", "EarlyFusion"):
        calls += [lambda: algo.align_paths(pair), lambda: algo.align_match_paths([0], [[i]]), lambda: algo.align_match_paths(q, [[0]])]
    if cls_name == "ChenFusion":
        calls += [lambda: algo.align(pair, "dmax"), lambda: algo.align_matches([0], [[i]], "dmax")]
    if cls_name == "EarlyFusion":
        calls += [lambda: algo.align(pair, "mfccs"), lambda: algo.full_fusion(pair), lambda: algo.rerank_full(q, [[0]]),
                  lambda: algo.rerank_full([0], [[i]])]
    if cls_name == "Simple":
        calls += [lambda: algo.profile(pair)]
    return calls


@pytest.mark.parametrize("cls_name", CLASSES)
def test_index_bounds_inside_a_session(make, cls_name):
    """[0, N + Q) is accepted wherever [0, N) is outside (the call reaches the library), N + Q and negative indices are refused
    before it."""
    algo, ctx, new = make(cls_name)
    labels = ["w0", "new", "new"]
    with algo.appended(new, labels=labels) as s:
        for bad in (s.total, -2):
            for call in _index_calls(cls_name, algo, bad):
                with pytest.raises(ValueError, match=r"\[0, %d\)" % s.total):
                    call()
        for call in _index_calls(cls_name, algo, s.total - 1):
            with pytest.raises(_Reached):
                call()
        assert ctx.calls == [("append", Q)]
    for call in _index_calls(cls_name, algo, N):
        with pytest.raises(ValueError, match=r"\[0, %d\)" % N):
            call()
    assert ctx.calls == [("append", Q), ("truncate", N)]


def test_evaluate_needs_labels_and_extends_the_cliques(make):
    algo, ctx, new = make("Simple")
    with algo.appended(new) as s:
        with pytest.raises(ValueError, match="opened without labels"):
            algo.evaluate(queries=s.indices)
        assert ctx.calls == [("append", Q)]
    cliques = copy.deepcopy(algo.cliques)
    with algo.appended(new, labels=["w1", "x", "x"]):
        assert algo._cliques_now() == [[0, 1], [2, 3, N], [4, 5], [6, 7], [N + 1, N + 2]]
        assert algo.cliques == cliques
    assert algo._cliques_now() == [[0, 1], [2, 3], [4, 5], [6, 7]]


@pytest.mark.parametrize("cls_name", CLASSES)
def test_restoration(make, cls_name):
    """After a session, after an exception in its body and after a failing library call in it: N, the cliques, the pooled
    lengths, the bound and the feature cache are as before, and the context saw one append and one truncate to N each time."""
    algo, ctx, new = make(cls_name)

    def state():
        cache = _cache(algo)
        plen = getattr(algo, "_pooled_len", None)
        return (algo.N, algo._n_tracks(), copy.deepcopy(algo.cliques), None if plen is None else plen.tolist(), id(cache), sorted(cache),
                list(algo.filepaths), algo._session)
    before = state()
    with algo.appended(new, labels=["a", "b", "c"]):
        pass
    assert state() == before
    with pytest.raises(KeyError, match="from the body"):
        with algo.appended(new):
            raise KeyError("from the body")
    assert state() == before
    with pytest.raises(_Reached):
        with algo.appended(new) as s:
            algo.identify(s.indices)
    assert state() == before
    assert ctx.calls == [("append", Q), ("truncate", N)] * 3


def test_a_failed_append_still_truncates_and_closes(make):
    algo, ctx, new = make("Serra09")

    def failing(frames, offsets):
        ctx.calls.append(("append", len(offsets) - 1))
        raise _Reached("pool_append")
    ctx.pool_append = failing
    with pytest.raises(_Reached):
        with algo.appended(new):
            raise AssertionError("the body must not run")
    assert ctx.calls == [("append", Q), ("truncate", N)] and algo._session is None and algo._n_tracks() == N
