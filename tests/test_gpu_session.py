"""
GPU tests of appended() sessions and their one-call forms (run with -m gpu on a real MI355X).  The rule: inside
`with A.appended(new) as s`, every permitted call returns, bit for bit, what the same call with the same indices returns on a
fresh object B of the same class and parameters built over the N + Q tracks in ONE upload.  Every comparison is equality of
shapes, dtypes and bytes: indices, score bits, every field of every record, every cell of every path, every profile value,
every evaluation number.  A holds N = 6 tracks, Q = 3 are new; the shapes are the smallest at which each class's kernels
still do all their work: Serra09 / ChenFusion pooled tracks of 40 to 130 frames at (m, tau) = (9, 1) and (5, 2) and once as
raw chroma with downsample_fac = 4 (raw lengths no multiples of 4), EarlyFusion 24 to 70 blocks with the feature widths of
tests/test_gpu_sw_align.py, SiMPle (12, 60..150) at SSLEN = 10, FTM2D shingles at WIN = 8.
EarlyFusion's locate_tracks() is held against the alignment of the pair (hit, new track) -- the cell whose score identify()
lists for that symmetric class --, not against align_tracks(), which aligns (new track, hit).
"""
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, Q = 6, 3
EF_DIMS = (40, 100, 96)                    # the feature widths of tests/test_gpu_sw_align.py
# the collection's clique labels and the new tracks': new track 0 has two mates (track 0 and new track 1), new track 1 has a mate
# among the new tracks, new track 2 has none
LABELS, NEW_LABELS = ["A", "B", "B", "C", "C", "D"], ["A", "A", "E"]
CONFIGS = ["serra09", "serra09_m5t2", "serra09_raw", "chen", "chen_m5t2", "earlyfusion", "simple", "ftm2d"]


def _flat(x):
    """Any result -> nested lists of arrays (dict values in key order)."""
    if isinstance(x, dict):
        return [_flat(x[k]) for k in sorted(x)]
    if isinstance(x, (list, tuple)):
        return [_flat(v) for v in x]
    return np.ascontiguousarray(x)


def _eq(a, b):
    """Same structure, shapes, dtypes and bytes (NaN and signed zeros included)."""
    a, b = _flat(a), _flat(b)
    if isinstance(a, list) or isinstance(b, list):
        return isinstance(a, list) and isinstance(b, list) and len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _serra_tracks(seed):
    """9 pooled tracks of 40 to 130 frames from four works; collection: tracks 0 .. 5, new: 6 .. 8."""
    from acoss_amd import synth
    d = synth.cover_set(clique_sizes=[3, 2, 2, 1, 1], seed=seed, t_range=(50, 104))
    t = [np.ascontiguousarray(d["frames"][d["offsets"][i]:d["offsets"][i + 1]]) for i in range(9)]
    t = [t[0], t[3], t[4], t[5], t[6], t[7], t[1], t[2], t[8]]
    assert all(40 <= len(x) <= 130 for x in t), [len(x) for x in t]
    return t


def _raw_tracks():
    """Raw chroma for downsample_fac = 4: no length a multiple of 4; pooled 40 to 130 frames."""
    rng = np.random.default_rng(19)
    return [rng.random((int(T0), 12)).astype(np.float32) for T0 in (203, 161, 322, 281, 247, 518, 290, 399, 173)]


def _ef_tracks():
    rng = np.random.default_rng(52999)
    tracks = []
    for k, nb in enumerate((24, 70, 33, 48, 57, 41, 64, 29, 52)):
        r = np.random.default_rng(52000 + k)
        tracks.append(dict(mfccs=r.standard_normal((nb, EF_DIMS[0])).astype(np.float32), ssms=(2 * r.random((nb, EF_DIMS[1]))).astype(np.float32),
                           chromas=(r.random((nb, EF_DIMS[2])).astype(np.float32) ** 3 + 1e-3), chroma_med=r.random(12) ** 2))
    for a, b, at_a, at_b, m in ((1, 6, 10, 30, 25), (4, 7, 20, 2, 20), (6, 8, 5, 25, 22), (3, 1, 8, 40, 24)):
        for key in ("mfccs", "ssms", "chromas"):              # shared excerpts: alignments longer than noise gives
            tracks[b][key][at_b:at_b + m] = tracks[a][key][at_a:at_a + m] + 0.02 * rng.standard_normal((m, tracks[a][key].shape[1])).astype(np.float32)
    return tracks


class _Built(object):
    """One configuration: A over the N tracks, B over the N + Q, the new tracks as appended() takes them."""

    def __init__(self, cfg, root):
        from acoss_amd import algorithms
        from acoss_amd.algorithms.rqa_serra09 import pool_median
        self.cfg, self.how, kw = cfg, {}, {}
        rng = np.random.default_rng(3)
        if cfg.startswith("serra09") or cfg.startswith("chen"):
            cls = algorithms.Serra09 if cfg.startswith("serra09") else algorithms.ChenFusion
            kw = dict(m=5, tau=2) if cfg.endswith("m5t2") else {}
            if cfg == "serra09_raw":
                raw = _raw_tracks()
                tracks, self.new, self.how, kw = [pool_median(t, 4) for t in raw], raw[N:], dict(raw=True), dict(downsample_fac=4)
            else:
                tracks = _serra_tracks(12 if cls is algorithms.Serra09 else 14)
                self.new = tracks[N:]
            inject = "set_pooled_features"
        elif cfg == "earlyfusion":
            cls, tracks, inject = algorithms.EarlyFusion, _ef_tracks(), "set_block_features"
            self.new = tracks[N:]
        elif cfg == "simple":
            cls, inject = algorithms.Simple, "set_features"
            feats = [rng.random((12, int(n))) for n in (60, 150, 97, 71, 133, 88, 64, 121, 149)]
            tracks = [f / np.linalg.norm(f, axis=0, keepdims=True) for f in feats]
            self.new = tracks[N:]
        else:
            cls, inject, kw = algorithms.FTM2D, "set_features", dict(WIN=8)
            tracks = list(0.3 * rng.standard_normal((N + Q, 96)))
            self.new = tracks[N:]
        self.planes = list(cls._identify_planes)
        self.objs = []
        for tag, n, labels in (("A", N, LABELS), ("B", N + Q, LABELS + NEW_LABELS)):
            path = os.path.join(root, "%s_%s.csv" % (cfg, tag))
            with open(path, "w") as f:
                f.write("work_id,track_id\n")
                for i in range(n):
                    f.write("w%d,t%d\n" % (i, i))
            obj = cls(path, "feat/", shortname="%s_%s" % (cfg, tag), **kw)
            getattr(obj, inject)(tracks[:n], labels)
            self.objs.append(obj)
        self.A, self.B = self.objs

    def session(self, labels=NEW_LABELS):
        return self.A.appended(self.new, labels=labels, **self.how)

    def close(self):
        for obj in self.objs:
            obj.cleanup_memmap()
            if getattr(obj, "_ctx", None) is not None:
                obj._ctx.close()
                obj._ctx = None


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """built(cfg) -> the _Built of a configuration, made once and shared; its objects are only read."""
    root, cwd, made = str(tmp_path_factory.mktemp("session")), os.getcwd(), {}
    os.chdir(root)

    def get(cfg):
        if cfg not in made:
            made[cfg] = _Built(cfg, root)
        return made[cfg]
    yield get
    for b in made.values():
        b.close()
    os.chdir(cwd)


# new against old, old against new, new against new (both orders), old against old
PAIRS = np.array([(6, 0), (1, 7), (7, 8), (8, 6), (2, 3), (8, 5)])
QUERIES = [6, 7, 8, 0, 3]
SHORT_Q, SHORTLISTS = [6, 1, 8], [[0, 7, -1], [8, -1, 2], [3, 4, 5]]


def _identify_then(method, **kw):
    """align_matches / align_match_paths on identify()'s own output: three candidates for k = 4 leave a -1 slot, and a new track
    is among the candidates."""
    def call(o):
        t = kw.get("similarity_type", o._identify_planes[0])
        idx = o.identify([6, 2, 8], k=4, candidates=[0, 3, 7], similarity_types=[t])[t][0]
        assert np.any(idx == -1) and np.any(idx == 7)
        return idx, getattr(o, method)([6, 2, 8], idx, **kw)
    return call


def _methods(cfg):
    """{case: call(object)}: every permitted method of the configuration's class with the index lists that matter."""
    m = {"identify": lambda o: o.identify(QUERIES, k=4),
         "identify_candidates_with_new": lambda o: o.identify(QUERIES, k=3, candidates=[1, 2, 6, 8]),
         "identify_k_beyond": lambda o: o.identify([7, 2], k=N + Q + 2),
         "query_rows": lambda o: o.query_rows([7, 2, 8]),
         "rerank": lambda o: o.rerank(SHORT_Q, SHORTLISTS, k=2),
         "evaluate_new": lambda o: o.evaluate(queries=np.arange(N, N + Q)),
         "evaluate_all": lambda o: o.evaluate(),
         "evaluate_mixed": lambda o: o.evaluate(queries=[7, 0, 3], topsidx=[1, 2])}
    if cfg == "ftm2d":
        return m
    types = {"chen": ["qmax", "dmax"], "chen_m5t2": ["qmax", "dmax"], "earlyfusion": ["mfccs", "ssms", "chromas", "early"]}.get(cfg, [None])
    for t in types:
        kw, tag = ({}, "") if t is None else (dict(similarity_type=t), "_" + t)
        m["align" + tag] = lambda o, kw=kw: o.align(PAIRS, **kw)
        m["align_matches" + tag] = _identify_then("align_matches", **kw)
        if cfg != "simple":
            m["align_paths" + tag] = lambda o, kw=kw: o.align_paths(PAIRS, **kw)
            m["align_match_paths" + tag] = _identify_then("align_match_paths", **kw)
    if cfg == "simple":
        m["profile"] = lambda o: o.profile(PAIRS)
    if cfg == "earlyfusion":
        m["full_fusion"] = lambda o: o.full_fusion(PAIRS)
        m["rerank_full"] = lambda o: o.rerank_full(SHORT_Q, SHORTLISTS, k=2)
    return m


CASES = [(cfg, name) for cfg in CONFIGS for name in _methods(cfg)]


@pytest.mark.parametrize("cfg,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_rule(built, cfg, name):
    b = built(cfg)
    call = _methods(cfg)[name]
    with b.session() as s:
        assert s.first == N and s.count == Q and s.total == N + Q and b.A.N == N and s.indices.tolist() == [6, 7, 8]
        got = call(b.A)
    want = call(b.B)
    assert _eq(got, want), (cfg, name)
    if name == "evaluate_new":
        # the labels give new track 0 two mates, new track 1 a mate among the new tracks and new track 2 none: two rows are ranked
        info = {}
        b.B.evaluate(queries=np.arange(N, N + Q), info=info)
        assert all(v["device_rows"] + v["host_rows"] == 2 for v in info.values()), info


ALIGNING = [c for c in CONFIGS if c != "ftm2d"]
INDICES = np.array([[0, -1, 7], [3, 2, 6], [5, -1, -1]], np.int32)          # a -1 slot and a new track in a row


def _types(cfg):
    return {"chen": [None, "dmax"], "chen_m5t2": [None, "dmax"], "earlyfusion": [None, "chromas"]}.get(cfg, [None])


@pytest.mark.parametrize("cfg", ALIGNING)
def test_align_tracks(built, cfg):
    """align_tracks / align_track_paths equal the session calls, and B's answers."""
    b = built(cfg)
    new_q = np.arange(N, N + Q)
    for t in _types(cfg):
        kw = {} if t is None else dict(similarity_type=t)
        got = b.A.align_tracks(b.new, INDICES, **kw, **b.how)
        with b.session(None) as s:
            inside = b.A.align_matches(s.indices, INDICES, **kw)
        assert _eq(got, inside) and _eq(got, b.B.align_matches(new_q, INDICES, **kw)), (cfg, t)
        assert got.shape == INDICES.shape and np.all(got["q0"][INDICES < 0] == -1)
        if cfg == "simple":
            continue
        got = b.A.align_track_paths(b.new, INDICES, **kw, **b.how)
        with b.session(None) as s:
            inside = b.A.align_match_paths(s.indices, INDICES, **kw)
        assert _eq(got, inside) and _eq(got, b.B.align_match_paths(new_q, INDICES, **kw)), (cfg, t)
        assert _eq(got[0], b.A.align_tracks(b.new, INDICES, **kw, **b.how))


@pytest.mark.parametrize("cfg", ALIGNING)
def test_locate_tracks(built, cfg):
    """locate_tracks equals identify_tracks + align_tracks, field for field; three candidates for k = 4 leave a -1 slot.
    EarlyFusion: + the alignment of (hit, new track), whose score bits are the listed score's."""
    b = built(cfg)
    A, cands = b.A, [0, 2, 5]
    for t in _types(cfg):
        kw = {} if t is None else dict(similarity_type=t)
        plane = t or {"earlyfusion": "early"}.get(cfg, b.planes[0])
        for c in (cands, None):
            idx, score, al = A.locate_tracks(b.new, k=4, candidates=c, **kw, **b.how)
            want = A.identify_tracks(b.new, k=4, candidates=c, similarity_types=[plane], **b.how)[plane]
            assert _eq(idx, want[0]) and _eq(score, want[1]), (cfg, t)
            assert (c is None) or np.all(idx[:, 3] == -1)
            if cfg == "simple":
                assert _eq(al, A.align_tracks(b.new, idx))
                continue
            idx2, score2, al2, paths = A.locate_tracks(b.new, k=4, candidates=c, paths=True, **kw, **b.how)
            assert _eq((idx2, score2, al2), (idx, score, al)) and len(paths) == Q and all(len(p) == 4 for p in paths)
            if cfg != "earlyfusion":
                assert _eq(al, A.align_tracks(b.new, idx, **kw, **b.how))
                assert _eq((al, paths), A.align_track_paths(b.new, idx, **kw, **b.how))
                continue
            rows, slots = np.nonzero(idx >= 0)
            pairs = np.stack([idx[rows, slots], N + rows], axis=1)
            ref, ref_paths = b.B.align_paths(pairs, **kw)
            assert _eq(al[rows, slots], ref) and _eq([paths[r][s] for r, s in zip(rows, slots)], ref_paths)
            assert np.all(al["q0"][idx < 0] == -1) and all(len(paths[r][s]) == 0 for r, s in zip(*np.nonzero(idx < 0)))
            assert _eq(al["score"][rows, slots].view(np.uint32), score[rows, slots].view(np.uint32)), "the record's score is the listed score"


def _state(b):
    """What a session must leave alone, as bytes."""
    A = b.A
    ctx, algo = A._grid()[:2]
    lengths = ctx.pool_lengths(algo)
    assert len(lengths) == N and A.N == N and A._n_tracks() == N and A._session is None
    plen = getattr(A, "_pooled_len", None)
    return _flat([A.identify(range(N), k=3), lengths, [zlib.crc32(np.asarray(A.Ds[t]).tobytes()) for t in sorted(A.Ds)],
                  [] if plen is None else plen, sorted(A.cliques), [sorted(A.cliques[c]) for c in sorted(A.cliques)]])


@pytest.mark.parametrize("cfg", ["serra09", "serra09_raw", "chen", "earlyfusion", "simple", "ftm2d"])
def test_state(built, cfg):
    b = built(cfg)
    before = _state(b)
    with b.session() as s:
        b.A.identify(s.indices, k=2)
        b.A.evaluate(queries=s.indices)
    assert _eq(_state(b), before)
    with pytest.raises(KeyError, match="from the body"):
        with b.session() as s:
            b.A.query_rows(s.indices)
            raise KeyError("from the body")
    assert _eq(_state(b), before)
    for fn in (lambda: b.A.identify_tracks(b.new, k=2, **b.how), lambda: b.A.locate_tracks(b.new, k=2, **b.how) if cfg != "ftm2d" else None):
        fn()
        assert _eq(_state(b), before)


def test_library_error_inside_a_session(built):
    """A new Serra09 track shorter than the delay-embedding stack: the append takes it, the first call that names it fails in
    the library (ACX_ERR_SHORT) -- the state is as before, and a following valid session succeeds."""
    from acoss_amd import _lib
    b = built("serra09")
    before = _state(b)
    short = [b.new[0], np.ascontiguousarray(b.new[1][:5])]
    with pytest.raises(_lib.AcxError, match="shorter than the delay-embedding stack"):
        with b.A.appended(short) as s:
            assert s.total == N + 2
            b.A.align([(0, s.first)])                          # (the well-formed one works)
            b.A.identify(s.indices, k=2)
    assert _eq(_state(b), before)
    with pytest.raises(_lib.AcxError, match="shorter than the delay-embedding stack"):
        b.A.locate_tracks(short, k=2)
    assert _eq(_state(b), before)
    with b.session() as s:
        got = b.A.identify(s.indices, k=3)
    assert _eq(got, b.B.identify([6, 7, 8], k=3))
    assert _eq(_state(b), before)


def test_launch_count(built):
    """One append's preparation per one-call form: with the event clocks on, the norm table's tail (norms_kernel) is built as
    often by locate_tracks as by identify_tracks alone, and twice as often by identify_tracks followed by align_tracks."""
    b = built("serra09")
    A = b.A
    ctx = A._context()
    A.identify([0], k=1)                                        # (the norm table exists: an append extends it)

    def launches(fn):
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            fn()
            return ctx.profile()["norms_kernel"]["launches"]
        finally:
            ctx.profile_enable(False)
    one = launches(lambda: A.identify_tracks(b.new, k=3))
    assert one >= 1
    assert launches(lambda: A.locate_tracks(b.new, k=3)) == one

    def two_calls():
        idx = A.identify_tracks(b.new, k=3)["main"][0]
        A.align_tracks(b.new, idx)
    assert launches(two_calls) == 2 * one


def test_planted_excerpt(built):
    """40 pooled frames of collection track 2 (from frame 10) stand 30 frames into a new track: locate_tracks ranks track 2
    first and its spans cover the planted ranges.  The rest of the new track are track 2's other 60 frames in a shuffled
    order: no run of them lines up with the original, and the new track's chroma profile is track 2's, so the optimal
    transposition between the two is none and the copy is compared as it stands.  Prints what it found; asserts only the
    rank and the coverage."""
    b = built("serra09")
    src = b.A.all_feats[2]
    assert len(src) == 100
    rest = np.random.default_rng(8).permutation(np.concatenate([np.arange(10), np.arange(50, 100)]))
    new = np.ascontiguousarray(np.concatenate([src[rest[:30]], src[10:50], src[rest[30:]]]))
    idx, score, al, paths = b.A.locate_tracks([new], k=3, paths=True)
    print("planted excerpt (frames 10..49 of track 2 = 30..69 of the new track): hits %s, scores %s, q_span %s, r_span %s, %d cells"
          % (idx[0].tolist(), score[0].tolist(), al["q_span"][0, 0].tolist(), al["r_span"][0, 0].tolist(), len(paths[0][0])))
    assert idx[0, 0] == 2
    q, r = al["q_span"][0, 0], al["r_span"][0, 0]
    assert q[0] <= 30 and q[1] >= 69, q
    assert r[0] <= 10 and r[1] >= 49, r
