"""
GPU tests of the append path (run with -m gpu on a real MI355X): acx_pool_append & co., acx_pool_truncate and
CoverAlgorithm.identify_tracks / score_tracks.  Every expectation comes from the path that existed before them: a
FRESH context that uploaded the final track list in one call (and, for Serra09, the CPU oracle).  Every comparison
is equality of indices and of score BITS.  The pools are those of tests/test_gpu_query.py::_setup: 22 tracks of 60-420
frames (Serra09 / ChenFusion), 23 of 30-90 frames (SiMPle), 11 of 20-70 blocks (EarlyFusion), 37 shingles of 24 values.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALGOS = ["serra09", "chenfusion", "simple", "earlyfusion", "ftm2d"]


def _eq(a, b):
    """Same shape, dtype and bytes (NaN and signed zeros included); lists element by element."""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class _Pool(object):
    """The small pool of one algorithm as a list of tracks, and the calls that differ between the pool types."""

    def __init__(self, name):
        from acoss_amd import _lib, synth
        rng = np.random.default_rng(77)
        self.name = name
        self.sym, self.planes, self.params = True, 1, None
        if name in ("serra09", "chenfusion"):
            d = synth.cover_set(clique_sizes=[2] * 9 + [3, 1], seed=31, t_range=(60, 420))
            self.tracks = [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for i in range(len(d["offsets"]) - 1)]
            self.algo = _lib.ALGO_SERRA09 if name == "serra09" else _lib.ALGO_CHENFUSION
            self.planes = 1 if name == "serra09" else 2
            self.params = _lib.serra09_params()
        elif name == "simple":
            feats = [rng.random((int(rng.integers(30, 90)), 12)) for _ in range(23)]
            self.tracks = [f / np.linalg.norm(f, axis=1, keepdims=True) for f in feats]
            self.algo, self.sym, self.params = _lib.ALGO_SIMPLE, False, _lib.SimpleParams(10, 1)
        elif name == "earlyfusion":
            self.tracks = synth.earlyfusion_set(11, seed=4, nb_range=(20, 70))
            self.algo, self.planes, self.params = _lib.ALGO_EARLYFUSION, 4, _lib.EfParams(0.1, 10)
        else:
            self.tracks = list(0.3 * rng.standard_normal((37, 24)))
            self.algo = _lib.ALGO_FTM2D
        assert len(self.tracks) == {"serra09": 22, "chenfusion": 22, "simple": 23, "earlyfusion": 11, "ftm2d": 37}[name]

    def length(self, t):
        """frames / blocks of a track as acx_pool_lengths counts them"""
        return 1 if self.name == "ftm2d" else (len(t["mfccs"]) if self.name == "earlyfusion" else len(t))

    @staticmethod
    def pack(tracks):
        offs = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
        return np.concatenate(tracks, axis=0), offs

    def upload(self, ctx, tracks):
        if self.name in ("serra09", "chenfusion"):
            ctx.upload_pool(*self.pack(tracks))
        elif self.name == "simple":
            ctx.upload_pool_f64(*self.pack(tracks))
        elif self.name == "earlyfusion":
            ctx.ef_upload_pool(tracks)
        else:
            ctx.ftm2d_upload_shingles(np.stack(tracks))

    def append(self, ctx, tracks):
        if self.name in ("serra09", "chenfusion"):
            ctx.pool_append(*self.pack(tracks))
        elif self.name == "simple":
            ctx.pool_append_f64(*self.pack(tracks))
        elif self.name == "earlyfusion":
            ctx.ef_pool_append(tracks)
        else:
            ctx.ftm2d_append_shingles(np.stack(tracks))

    def all_pairs(self, n):
        return np.array([(i, j) for i in range(n) for j in range(n) if (i < j if self.sym else i != j)], np.int32)

    def pairs(self, ctx, pairs, params=None):
        p = params if params is not None else self.params
        if self.name == "serra09":
            return ctx.serra09_pairs(pairs, p)
        if self.name == "chenfusion":
            return ctx.chenfusion_pairs(pairs, p)
        if self.name == "simple":
            return ctx.simple_pairs(pairs, p.sslen)
        if self.name == "earlyfusion":
            return ctx.earlyfusion_pairs(pairs, kappa=p.kappa, K=p.K)
        return ctx.ftm2d_pairs(pairs)

    def download(self, ctx, n_rows):
        if self.name in ("serra09", "chenfusion"):
            return ctx.download_pool(n_rows)
        if self.name == "simple":
            return ctx.download_pool_f64(n_rows)
        if self.name == "ftm2d":
            return ctx.ftm2d_download_shingles()
        return None                                  # (the block-feature pool has no download call)

    def snapshot(self, ctx, tracks, params=None):
        """Everything the defining property names, for a pool that should hold `tracks`."""
        n = len(tracks)
        lengths = ctx.pool_lengths(self.algo)
        grid = [np.zeros((n, n), np.float32) for _ in range(self.planes)]
        ctx.pair_grid(self.algo, self.sym, params if params is not None else self.params, grid, mirror=self.sym)
        return dict(lengths=lengths, pool=self.download(ctx, sum(self.length(t) for t in tracks)), scores=self.pairs(ctx, self.all_pairs(n), params),
                    grid=grid)


def _same_state(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert _eq(a[key], b[key]), key


def _context(**kw):
    from acoss_amd import _lib
    return _lib.Context(0, **kw)


_FRESH = {}


def _fresh(name, key, tracks, params=None, prepare=None):
    """The reference: a fresh context, ONE upload of `tracks`, a snapshot; computed once per (name, key) and shared."""
    if (name, key) not in _FRESH:
        P = _Pool(name)
        ctx = _context()
        try:
            if prepare:
                prepare(ctx)
            P.upload(ctx, tracks)
            _FRESH[(name, key)] = P.snapshot(ctx, tracks, params)
        finally:
            ctx.close()
    return _FRESH[(name, key)]


def _first(name):
    """Tracks of the first upload: 10, as far as the pool leaves three appends (EarlyFusion has 11 tracks: 8)."""
    return 8 if name == "earlyfusion" else 10


@pytest.mark.parametrize("name", ALGOS)
def test_growth_path(name):
    """upload, append 1 (the exact blocks reallocate), append 1 (fits the new capacity), append the rest (reallocates)."""
    P = _Pool(name)
    n0, T = _first(name), P.tracks
    want = _fresh(name, "all", T)
    ctx = _context()
    try:
        P.upload(ctx, T[:n0])
        P.append(ctx, T[n0:n0 + 1])
        assert len(ctx.pool_lengths(P.algo)) == n0 + 1
        P.append(ctx, T[n0 + 1:n0 + 2])
        P.append(ctx, T[n0 + 2:])
        got = P.snapshot(ctx, T)
    finally:
        ctx.close()
    _same_state(got, want)
    if name == "serra09":
        import oracle
        frames, offs = P.pack(T)
        pairs = np.array([(i, j) for i in (0, 9, 10, 11) for j in range(i + 1, len(T)) if j >= 10], np.int32)
        ref = oracle.serra09_pairs(frames, offs, pairs)
        ap = {tuple(p): s for p, s in zip(P.all_pairs(len(T)).tolist(), got["scores"])}
        assert _eq(np.array([ap[tuple(p)] for p in pairs.tolist()], np.float32), ref)


def _serra_cases():
    from acoss_amd import _lib
    sp = _lib.serra09_params
    # key: (pool, params used BEFORE the append -- what they built gets extended --, params compared after it, in order)
    return {"normtab": ("serra09", sp(), [sp(), sp(m=5, embed_full=1), sp()]),
            "tau2": ("serra09", sp(tau=2), [sp(tau=2), sp(tau=1), sp(tau=3, m=4)]),
            "f16x2": ("serra09", sp(arith="f16x2"), [sp(arith="f16x2"), sp()]),
            "embed_full": ("serra09", sp(embed_full=1), [sp(embed_full=1), sp(m=16)]),
            "chen": ("chenfusion", sp(), [sp(), sp(m=5, embed_full=1)])}


@pytest.mark.parametrize("case", ["normtab", "tau2", "f16x2", "embed_full", "chen"])
def test_derived_data_serra09(case):
    """Derived data that exists when the append comes -- norm table, decimated active pool, f16 operand pool -- is extended;
    what a later parameter set needs is rebuilt over the grown pool.  ChenFusion: both planes."""
    name, before, after = _serra_cases()[case]
    P = _Pool(name)
    T, n0 = P.tracks, 10
    ctx = _context()
    try:
        P.upload(ctx, T[:n0])
        P.pairs(ctx, P.all_pairs(n0), before)
        P.append(ctx, T[n0:n0 + 4])
        P.pairs(ctx, P.all_pairs(n0 + 4)[-5:], before)         # (used between two appends, too)
        P.append(ctx, T[n0 + 4:])
        for i, p in enumerate(after):
            want = _fresh(name, (case, i), T, params=p)
            _same_state(P.snapshot(ctx, T, p), want)
    finally:
        ctx.close()


def test_derived_data_simple():
    """SiMPle's window norms exist for one SSLEN when the append comes and are asked for another afterwards."""
    from acoss_amd import _lib
    P = _Pool("simple")
    T, n0 = P.tracks, 10
    ctx = _context()
    try:
        P.upload(ctx, T[:n0])
        P.pairs(ctx, P.all_pairs(n0), _lib.SimpleParams(10, 1))
        P.append(ctx, T[n0:])
        for sslen in (10, 7, 10):
            p = _lib.SimpleParams(sslen, 1)
            _same_state(P.snapshot(ctx, T, p), _fresh("simple", ("sslen", sslen), T, params=p))
    finally:
        ctx.close()


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3"])
def test_derived_data_earlyfusion(mode):
    """Row norms, row scales and splits in the pool's current format are extended row by row; the other format is built
    over the grown pool when the mode is switched after the append."""
    P = _Pool("earlyfusion")
    T, n0 = P.tracks, 8
    other = "bf16x3" if mode == "f16x2" else "f16x2"
    ctx = _context()
    try:
        ctx.set_ef_gemm(mode)
        P.upload(ctx, T[:n0])
        P.pairs(ctx, P.all_pairs(n0))
        P.append(ctx, T[n0:])
        for m in (mode, other, mode):
            ctx.set_ef_gemm(m)
            _same_state(P.snapshot(ctx, T), _fresh("earlyfusion", ("gemm", m), T, prepare=lambda c, m=m: c.set_ef_gemm(m)))
    finally:
        ctx.close()


def test_size_classes_and_pool_edges():
    """Appended tracks of 12 frames (shorter than the stack from m = 12 on), 0 frames, 1100 frames (widest band class) and 2100 frames
    (streaming class), the long ones LAST: their edge tiles read the slack behind the pool.  Scores and recurrence plots."""
    from acoss_amd import _lib, synth
    P = _Pool("serra09")
    base = P.tracks[:6]
    long_ = synth.cover_set(clique_sizes=[1, 1], seed=5, t_range=(1100, 1100))
    t1100 = long_["frames"][:1100]
    t2100 = np.concatenate([long_["frames"], long_["frames"][:1000][::-1]])[:2100]
    assert t1100.shape == (1100, 12) and t2100.shape == (2100, 12)
    tail = [P.tracks[6][:12], np.zeros((0, 12), np.float32), np.ascontiguousarray(t1100), np.ascontiguousarray(t2100)]
    allt = base + tail
    wide = np.array([(i, 8) for i in range(6)], np.int32)
    stream = np.array([(0, 9), (1, 9)], np.int32)
    res = []
    for appended in (False, True):
        ctx = _context()
        try:
            if appended:
                P.upload(ctx, base)
                ctx.serra09_pairs(P.all_pairs(6))                 # (a norm table to extend)
                P.append(ctx, tail[:2])
                P.append(ctx, tail[2:])
            else:
                P.upload(ctx, allt)
            r = dict(lengths=ctx.pool_lengths(P.algo), pool=ctx.download_pool(sum(len(t) for t in allt)))
            for key, pr in (("wide", wide), ("stream", stream)):
                r[key] = ctx.serra09_pairs(pr)
                sc, plots = ctx.serra09_debug_bits(pr)
                r[key + "_dbg"], r[key + "_plots"], r[key + "_outside"] = sc, plots, np.int64(ctx.outside_bits)
            # 12 frames leave 3 embedded frames at the default m = 9: an ordinary, tiny pair; at m = 16 the track is shorter
            # than the stack, as the track without frames is at any m -- the answer an uploaded one gets
            r["tiny"] = ctx.serra09_pairs(np.array([(0, 6), (6, 8)], np.int32))
            for short, p in ((7, _lib.serra09_params()), (6, _lib.serra09_params(m=16)), (7, _lib.serra09_params(m=16))):
                with pytest.raises(_lib.AcxError, match="shorter than the delay-embedding stack"):
                    ctx.serra09_pairs(np.array([(0, short)], np.int32), p)
            r["m16"] = ctx.serra09_pairs(wide, _lib.serra09_params(m=16))
            r["after"] = ctx.serra09_pairs(P.all_pairs(6))
            res.append(r)
        finally:
            ctx.close()
    _same_state(res[1], res[0])
    assert res[0]["lengths"].tolist()[6:] == [12, 0, 1100, 2100]
    assert np.any(res[0]["wide"] > 0) and np.any(res[0]["stream"] > 0)


def _different(name, tracks):
    """Tracks of other content AND other lengths than `tracks`."""
    if name == "ftm2d":
        return [-t[::-1] for t in tracks[::-1]][:-1]
    if name == "earlyfusion":
        return [{k: (np.ascontiguousarray(v[::-1][:-3]) if k != "chroma_med" else v[::-1].copy()) for k, v in t.items()} for t in tracks[::-1]]
    return [np.ascontiguousarray(t[::-1][:-7]) for t in tracks[::-1]]


@pytest.mark.parametrize("name", ALGOS)
def test_truncate(name):
    P = _Pool(name)
    T, n0 = P.tracks, _first(name)
    other = T[:n0] + _different(name, T[n0:])
    ctx = _context()
    try:
        P.upload(ctx, T[:n0])
        P.pairs(ctx, P.all_pairs(n0))                             # (derived data exists)
        P.append(ctx, T[n0:])
        P.pairs(ctx, P.all_pairs(len(T))[-3:])
        ctx.pool_truncate(P.algo, n0)
        _same_state(P.snapshot(ctx, T[:n0]), _fresh(name, "first", T[:n0]))
        ctx.pool_truncate(P.algo, n0)                             # to the current count: nothing happens
        assert len(ctx.pool_lengths(P.algo)) == n0
        # different tracks behind the same end: nothing of the first append's frames, norms or row scales may show
        P.append(ctx, other[n0:])
        _same_state(P.snapshot(ctx, other), _fresh(name, "other", other))
        ctx.pool_truncate(P.algo, 1)
        assert ctx.pool_lengths(P.algo).tolist() == [P.length(T[0])]
        P.append(ctx, T[1:n0])
        _same_state(P.snapshot(ctx, T[:n0]), _fresh(name, "first", T[:n0]))
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ALGOS)
def test_upload_over_grown_pool(name):
    """A new upload into a context whose pool has been grown (every block at 1.5 x its capacity, derived data included) and
    truncated: the pool is the new list's alone, its blocks are exactly as large as their contents again -- so the first
    append behind it reallocates -- and, Serra09, an upload that fails over a grown pool leaves no pool."""
    from acoss_amd import _lib
    P = _Pool(name)
    T, n0 = P.tracks, _first(name)
    few = P.all_pairs(n0)[:4]
    prepare, tag = None, "default"
    ctx = _context()
    try:
        if name == "earlyfusion":
            prepare, tag = (lambda c: c.set_ef_gemm("f16x2")), "f16x2"
            prepare(ctx)
        P.upload(ctx, T[:n0])
        if name in ("serra09", "chenfusion"):                     # decimated pool, norm table and (Serra09) f16 operand pool exist
            P.pairs(ctx, few, _lib.serra09_params(tau=2))
        if name == "serra09":
            P.pairs(ctx, few, _lib.serra09_params(tau=2, arith="f16x2"))
        if name == "earlyfusion":                                 # row scales and two-term splits exist
            P.pairs(ctx, few)
        P.append(ctx, T[n0:])
        ctx.pool_truncate(P.algo, n0 + 1)
        assert len(ctx.pool_lengths(P.algo)) == n0 + 1
        P.upload(ctx, T[3:9])
        _same_state(P.snapshot(ctx, T[3:9]), _fresh(name, ("reupload", tag, "3:9"), T[3:9], prepare=prepare))
        P.append(ctx, T[9:12])
        _same_state(P.snapshot(ctx, T[3:12]), _fresh(name, ("reupload", tag, "3:12"), T[3:12], prepare=prepare))
        if name == "serra09":
            # the decimated copy in the same lifecycle: rebuilt over the new pool (exact again), grown by an append, truncated
            p2 = _lib.serra09_params(tau=2)
            ctx.pool_truncate(P.algo, 6)
            _same_state(P.snapshot(ctx, T[3:9], p2), _fresh(name, ("reupload", "tau2", "3:9"), T[3:9], params=p2))
            P.append(ctx, T[9:12])
            _same_state(P.snapshot(ctx, T[3:12], p2), _fresh(name, ("reupload", "tau2", "3:12"), T[3:12], params=p2))
            bad = [T[0], T[1].copy(), T[2]]
            bad[1][3, 5] = np.nan
            with pytest.raises(ValueError, match=r"track 1 holds a non-finite value"):
                P.upload(ctx, bad)
            with pytest.raises(_lib.AcxError, match="not uploaded"):
                ctx.serra09_pairs(P.all_pairs(3))
    finally:
        ctx.close()


def _raw_tracks():
    """Raw chroma for fac = 4: lengths that are and are not multiples of 4, and one track whose bins b and b + 6 are equal --
    its chroma profile has period 6, so two transpositions tie in every OTI it takes part in, bit for bit."""
    rng = np.random.default_rng(19)
    tracks = [rng.random((int(T0), 12)).astype(np.float32) for T0 in (240, 203, 322, 280, 261, 247, 400, 318)]
    half = rng.random((290, 6)).astype(np.float32)
    tracks[6] = np.ascontiguousarray(np.concatenate([half, half], axis=1))
    return tracks


def test_raw_append():
    P = _Pool("serra09")
    raw = _raw_tracks()
    n0 = 5
    oti_pairs = [(0, 6), (6, 7), (5, 6), (2, 7), (5, 7)]
    res, offs = [], []
    for appended in (False, True):
        ctx = _context()
        try:
            if appended:
                ctx.upload_raw_pool(*P.pack(raw[:n0]), fac=4)
                p1 = ctx.pool_append_raw(*P.pack(raw[n0:n0 + 1]), fac=4)
                p2 = ctx.pool_append_raw(*P.pack(raw[n0 + 1:]), fac=4)
                offs.append(np.concatenate([p1, p1[-1] + p2[1:]]))
            else:
                poff = ctx.upload_raw_pool(*P.pack(raw), fac=4)
                ctx.lengths = np.diff(poff)
                offs.append(poff[n0:] - poff[n0])
            lengths = ctx.pool_lengths(P.algo)
            r = dict(lengths=lengths, pool=ctx.download_pool(int(lengths.sum())), scores=ctx.serra09_pairs(P.all_pairs(len(raw))),
                     oti=np.array([ctx.serra09_debug_pair(i, j)["oti"] for i, j in oti_pairs]))
            res.append(r)
        finally:
            ctx.close()
    assert _eq(offs[1], offs[0]) and offs[0].tolist()[:3] == [0, 62, 135]        # ceil(247 / 4), + ceil(290 / 4)
    _same_state(res[1], res[0])
    # the pooled track keeps the period, so its profile does: the tie is real
    pooled6 = res[0]["pool"][res[0]["lengths"][:6].sum():res[0]["lengths"][:7].sum()]
    assert np.array_equal(pooled6[:, :6], pooled6[:, 6:])


def _dataset(tmp_path, tag, n):
    path = os.path.join(str(tmp_path), "%s.csv" % tag)
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return path


def _class_tracks(cls_name, n):
    from acoss_amd import synth
    rng = np.random.default_rng(3)
    if cls_name in ("Serra09", "ChenFusion"):
        d = synth.cover_set(clique_sizes=[2] * (n // 2), seed=12, t_range=(60, 200))
        return [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for i in range(n)]
    if cls_name == "Simple":
        feats = [rng.random((12, int(rng.integers(30, 80)))) for _ in range(n)]
        return [f / np.linalg.norm(f, axis=0, keepdims=True) for f in feats]
    if cls_name == "EarlyFusion":
        return synth.earlyfusion_set(n, seed=6, nb_range=(20, 60))
    return list(0.3 * rng.standard_normal((n, 36)))


def _make(cls_name, tmp_path, tag, tracks):
    from acoss_amd import algorithms
    cls = getattr(algorithms, cls_name)
    kw = dict(WIN=3) if cls_name == "FTM2D" else {}
    a = cls(_dataset(tmp_path, tag, len(tracks)), "feat/", shortname=tag, **kw)
    labels = ["w%d" % (i // 2) for i in range(a.N)]
    if cls_name in ("Serra09", "ChenFusion"):
        a.set_pooled_features(tracks, labels)
    elif cls_name == "EarlyFusion":
        a.set_block_features(tracks, labels)
    else:
        a.set_features(tracks, labels)
    return a


def _too_short(cls_name, track):
    if cls_name in ("Serra09", "ChenFusion"):
        return track[:5]
    if cls_name == "Simple":
        return track[:, :4]
    if cls_name == "EarlyFusion":
        return {k: (v[:0] if k != "chroma_med" else v) for k, v in track.items()}
    return None                                      # (a shingle has one length: FTM2D has no too-short track)


@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion", "Simple", "EarlyFusion", "FTM2D"])
def test_identify_tracks(tmp_path, monkeypatch, cls_name):
    """identify_tracks / score_tracks of an object over N tracks against identify(queries=[N ..], candidates=range(N)) /
    query_rows[:, :N] of a SECOND object built over the N + Q tracks."""
    from acoss_amd import _lib
    monkeypatch.chdir(tmp_path)
    N, Q = 9, 3
    tracks = _class_tracks(cls_name, N + Q)
    ident, full = _make(cls_name, tmp_path, "ident", tracks[:N]), _make(cls_name, tmp_path, "full", tracks)
    new, queries = tracks[N:], list(range(N, N + Q))
    types = list(full._identify_planes)
    before = ident.identify([0, 4, 7], k=5)
    plen = None if getattr(ident, "_pooled_len", None) is None else ident._pooled_len.copy()
    for k in (1, 4, N + 3):
        got, want = ident.identify_tracks(new, k=k), full.identify(queries, k=k, candidates=np.arange(N))
        assert sorted(got) == sorted(types)
        for t in types:
            assert _eq(got[t][0], want[t][0]) and _eq(got[t][1], want[t][1]), (t, k)
        if k > N:
            assert np.all(got[types[0]][0][:, N:] == -1) and np.all(np.isnan(got[types[0]][1][:, N:]))
    cand = np.array([0, 2, 3, 7])
    got = ident.identify_tracks(new, k=6, candidates=cand, similarity_types=types[-1:])
    want = full.identify(queries, k=6, candidates=cand, similarity_types=types[-1:])
    assert list(got) == types[-1:]
    assert _eq(got[types[-1]][0], want[types[-1]][0]) and _eq(got[types[-1]][1], want[types[-1]][1])
    assert np.all(got[types[-1]][0][:, 4:] == -1) and np.all(np.isnan(got[types[-1]][1][:, 4:]))
    rows, wrows = ident.score_tracks(new), full.query_rows(queries)
    for t in types:
        assert rows[t].shape == (Q, N) and _eq(rows[t], wrows[t][:, :N]), t

    def unchanged():
        ctx, algo = ident._grid()[0], ident._grid()[1]
        assert len(ctx.pool_lengths(algo)) == N and ident.N == N
        after = ident.identify([0, 4, 7], k=5)
        for t in types:
            assert _eq(after[t][0], before[t][0]) and _eq(after[t][1], before[t][1]), t
        if plen is not None:
            assert np.array_equal(ident._pooled_len, plen)
        for t in ident.Ds:
            assert not np.any(np.asarray(ident.Ds[t])), "identify_tracks must not write Ds"
    unchanged()
    short = _too_short(cls_name, new[1])
    if short is not None:
        with pytest.raises(_lib.AcxError):
            ident.identify_tracks([new[0], short], k=3)
        with pytest.raises(_lib.AcxError):
            ident.score_tracks([short])
        unchanged()
    ident.cleanup_memmap()
    full.cleanup_memmap()


def test_identify_tracks_raw(tmp_path, monkeypatch):
    """Serra09 with raw=True: raw chroma pooled on the device by downsample_fac equals the pooled tracks handed in."""
    from acoss_amd.algorithms.rqa_serra09 import pool_median
    monkeypatch.chdir(tmp_path)
    raw = _raw_tracks()
    pooled = [pool_median(t, 4) for t in raw]
    a = _make("Serra09", tmp_path, "raw", pooled[:6])
    a.downsample_fac = 4
    want = a.identify_tracks(pooled[6:], k=4)
    got = a.identify_tracks(raw[6:], k=4, raw=True)
    assert _eq(got["main"][0], want["main"][0]) and _eq(got["main"][1], want["main"][1])
    assert _eq(a.score_tracks(raw[6:], raw=True)["main"], a.score_tracks(pooled[6:])["main"])
    a.cleanup_memmap()


def _code(ctx, rc, code, *words):
    msg = ctx._L.acx_last_error(ctx._h).decode()
    assert rc == code, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_error_codes():
    """Every error of the append calls: its code, and the argument by name."""
    from acoss_amd import _lib
    P = _Pool("serra09")
    frames, offs = P.pack(P.tracks[:3])
    fp, lp, dp = _lib._fptr, _lib._lptr, _lib._dptr
    S = np.zeros((2, 24))
    ctx = _context()
    try:
        L, h = ctx._L, ctx._h
        # no pool of that kind
        _code(ctx, L.acx_pool_append(h, fp(frames), lp(offs), 3, 12), _lib.ACX_ERR_STATE, "pool_append", "not uploaded")
        _code(ctx, L.acx_pool_append_raw(h, fp(frames), lp(offs), 3, 12, 4, None), _lib.ACX_ERR_STATE, "pool_append_raw")
        _code(ctx, L.acx_pool_append_f64(h, dp(frames.astype(np.float64)), lp(offs), 3, 12), _lib.ACX_ERR_STATE, "pool_append_f64")
        _code(ctx, L.acx_ftm2d_append_shingles(h, dp(S), 2, 24), _lib.ACX_ERR_STATE, "ftm2d_append_shingles")
        for algo in range(5):
            _code(ctx, L.acx_pool_truncate(h, algo, 1), _lib.ACX_ERR_STATE, "pool_truncate")
        _code(ctx, L.acx_pool_truncate(h, 9, 1), _lib.ACX_ERR_INVALID, "algo")
        # a pool that is still open
        ctx.ef_pool_begin([3, 4])
        z = [np.zeros((2, d), np.float32) for d in (650, 1225, 480)]
        o2 = np.array([0, 2], np.int64)
        _code(ctx, L.acx_ef_pool_append(h, fp(z[0]), fp(z[1]), fp(z[2]), dp(np.zeros(12)), lp(o2), 1), _lib.ACX_ERR_STATE, "still being filled")
        _code(ctx, L.acx_pool_truncate(h, _lib.ALGO_EARLYFUSION, 1), _lib.ACX_ERR_STATE)
        ctx.ftm2d_pool_begin(4, win=2)
        _code(ctx, L.acx_ftm2d_append_shingles(h, dp(S), 2, 24), _lib.ACX_ERR_STATE, "still being filled")
        _code(ctx, L.acx_pool_truncate(h, _lib.ALGO_FTM2D, 1), _lib.ACX_ERR_STATE)
        # arguments, with pools in place
        P.upload(ctx, P.tracks[:4])
        want = ctx.serra09_pairs(P.all_pairs(4))
        bad0, dec = offs.copy(), offs.copy()
        bad0[0] = 1
        dec[2] = dec[1] - 1
        _code(ctx, L.acx_pool_append(h, fp(frames), lp(offs), 3, 11), _lib.ACX_ERR_INVALID, "dim")
        _code(ctx, L.acx_pool_append(h, fp(frames), lp(bad0), 3, 12), _lib.ACX_ERR_INVALID, "offsets[0]")
        _code(ctx, L.acx_pool_append(h, fp(frames), lp(dec), 3, 12), _lib.ACX_ERR_INVALID, "offsets")
        _code(ctx, L.acx_pool_append(h, fp(frames), lp(offs), 0, 12), _lib.ACX_ERR_INVALID, "n_new")
        _code(ctx, L.acx_pool_append(h, fp(frames), lp(offs), 2 ** 31 - 1, 12), _lib.ACX_ERR_INVALID, "n_new", "2^31")
        _code(ctx, L.acx_pool_append(h, None, lp(offs), 3, 12), _lib.ACX_ERR_INVALID)
        _code(ctx, L.acx_pool_append_raw(h, fp(frames), lp(offs), 3, 12, 0, None), _lib.ACX_ERR_INVALID, "fac")
        _code(ctx, L.acx_pool_append_raw(h, fp(frames), lp(offs), 3, 12, 65, None), _lib.ACX_ERR_UNSUPPORTED, "fac")
        _code(ctx, L.acx_pool_append_raw(h, fp(frames), lp(offs), 3, 11, 4, None), _lib.ACX_ERR_INVALID, "dim")
        _code(ctx, L.acx_pool_append_raw(h, fp(frames), lp(bad0), 3, 12, 4, None), _lib.ACX_ERR_INVALID, "offsets[0]")
        for n in (0, 5, -1):
            _code(ctx, L.acx_pool_truncate(h, _lib.ALGO_SERRA09, n), _lib.ACX_ERR_INVALID, "n_tracks")
        _code(ctx, L.acx_pool_truncate(h, _lib.ALGO_CHENFUSION, 4), _lib.ACX_OK)
        assert len(ctx.pool_lengths(_lib.ALGO_SERRA09)) == 4 and _eq(ctx.serra09_pairs(P.all_pairs(4)), want)
        ctx.upload_pool_f64(frames.astype(np.float64), offs)
        _code(ctx, L.acx_pool_append_f64(h, dp(frames.astype(np.float64)), lp(offs), 3, 11), _lib.ACX_ERR_INVALID, "dim")
        _code(ctx, L.acx_pool_append_f64(h, dp(frames.astype(np.float64)), lp(dec), 3, 12), _lib.ACX_ERR_INVALID, "offsets")
        _code(ctx, L.acx_pool_truncate(h, _lib.ALGO_SIMPLE, 4), _lib.ACX_ERR_INVALID, "n_tracks")
        ctx.ftm2d_upload_shingles(np.zeros((3, 24)))
        _code(ctx, L.acx_ftm2d_append_shingles(h, dp(S), 2, 12), _lib.ACX_ERR_INVALID, "dim")
        _code(ctx, L.acx_ftm2d_append_shingles(h, dp(S), 0, 24), _lib.ACX_ERR_INVALID, "n_new")
        assert ctx.ftm2d_download_shingles().shape == (3, 24)
        E = _Pool("earlyfusion")
        ctx.ef_upload_pool(E.tracks[:2])
        _code(ctx, L.acx_ef_pool_append(h, fp(z[0]), fp(z[1]), fp(z[2]), dp(np.zeros(12)), lp(np.array([1, 2], np.int64)), 1), _lib.ACX_ERR_INVALID, "offsets[0]")
        _code(ctx, L.acx_ef_pool_append(h, fp(z[0]), None, fp(z[2]), dp(np.zeros(12)), lp(o2), 1), _lib.ACX_ERR_INVALID, "ssms")
        with pytest.raises(ValueError, match="dims"):
            ctx.ef_pool_append([dict(E.tracks[3], mfccs=E.tracks[3]["mfccs"][:, :600])])
        assert len(ctx.pool_lengths(_lib.ALGO_EARLYFUSION)) == 2
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["serra09", "simple", "earlyfusion"])
def test_nonfinite_append(name):
    """REJECT: the append fails naming the track by its FINAL index and the pool is as it was.  ZERO: the values are zeroed
    and counted, and the scores are those of the zeroed track."""
    P = _Pool(name)
    T, n0 = P.tracks, 6
    good, bad, zeroed = T[n0], None, None
    if name == "earlyfusion":
        bad = dict(T[n0 + 1], ssms=T[n0 + 1]["ssms"].copy())
        bad["ssms"][3, 5], bad["ssms"][4, 0], bad["ssms"][7, 9] = np.nan, np.inf, -np.inf
        zeroed = dict(bad, ssms=np.where(np.isfinite(bad["ssms"]), bad["ssms"], 0).astype(np.float32))
    else:
        bad = T[n0 + 1].copy()
        bad[3, 5], bad[4, 0], bad[20, 11] = np.nan, np.inf, -np.inf
        zeroed = np.where(np.isfinite(bad), bad, 0).astype(bad.dtype)
    ctx = _context()
    try:
        P.upload(ctx, T[:n0])
        want = P.snapshot(ctx, T[:n0])
        with pytest.raises(ValueError, match=r"track %d holds a non-finite value" % (n0 + 1)):
            P.append(ctx, [good, bad])
        _same_state(P.snapshot(ctx, T[:n0]), want)
        P.append(ctx, [good])                                     # and the pool still takes an append
        assert len(ctx.pool_lengths(P.algo)) == n0 + 1
    finally:
        ctx.close()
    final = T[:n0] + [good, zeroed]
    ctx = _context(nonfinite="zero")
    try:
        P.upload(ctx, T[:n0])
        P.pairs(ctx, P.all_pairs(n0))
        P.append(ctx, [good, bad])
        assert ctx.nonfinite_zeroed() == 3
        got = P.snapshot(ctx, final)
    finally:
        ctx.close()
    _same_state(got, _fresh(name, "zeroed", final))


def test_f16x2_pool_through_truncates():
    """The f16 operand pool exists when the appends come.  A truncate to an end that no append ever stopped at, but which keeps
    every track the operand pool's range check was made for, keeps it; a shorter one drops it, and the next f16x2 call
    rebuilds it.  When the tracks that remain are too quiet for the range check, the call refuses them as after an upload."""
    from acoss_amd import _lib
    P = _Pool("serra09")
    T, n0 = P.tracks, 10
    p = _lib.serra09_params(arith="f16x2")
    ctx = _context()
    try:
        P.upload(ctx, T[:n0])
        P.pairs(ctx, P.all_pairs(n0), p)
        P.append(ctx, T[n0:n0 + 4])
        P.append(ctx, T[n0 + 4:])
        for n in (12, 7):
            ctx.pool_truncate(P.algo, n)
            _same_state(P.snapshot(ctx, T[:n], p), _fresh("serra09", ("f16x2", n), T[:n], params=p))
        P.append(ctx, T[7:12])
        _same_state(P.snapshot(ctx, T[:12], p), _fresh("serra09", ("f16x2", 12), T[:12], params=p))
    finally:
        ctx.close()
    quiet = [np.ascontiguousarray(t * np.float32(2.0 ** -12)) for t in T[:2]]      # largest magnitude below 2^-8
    ctx = _context()
    try:
        P.upload(ctx, quiet)
        P.append(ctx, T[2:6])
        P.pairs(ctx, P.all_pairs(6), p)                              # (built, and checked, over the six tracks)
        ctx.pool_truncate(P.algo, 2)
        with pytest.raises(NotImplementedError, match="f16x2 needs features"):
            P.pairs(ctx, P.all_pairs(2), p)
        assert _eq(P.pairs(ctx, P.all_pairs(2)), _fresh("serra09", "quiet", quiet)["scores"])
    finally:
        ctx.close()


def test_rejected_append_on_recycled_memory():
    """A rejected append leaves the pool as it was also when the blocks it had replaced by then are recycled device memory.
    The first append after an upload always reallocates, and the band kernel's edge tiles of the last track read the slack
    behind the rotated pool and the norm table unclamped, so what an append keeps of a block includes that slack: the
    new block is sealed like the old one before anything can fail.  Device memory freed just before, full of NaN patterns
    (as a freed norm table is full of +inf), is there for the allocator to hand back: where it does, a block that was NOT
    sealed shows as NaN scores instead of the pool's.  Which block an allocation gets is the allocator's choice, so this
    test can catch the fault and cannot prove its absence; the copy of the slack in s09_append_begin is what does."""
    import torch
    P = _Pool("serra09")
    T, n0 = P.tracks, 6
    bad = T[n0 + 1].copy()
    bad[3, 5] = np.nan
    ctx = _context()
    try:
        P.upload(ctx, T[:n0])
        want = P.snapshot(ctx, T[:n0])                                # (rotated pool and norm table exist)
        dev = ctx.torch_device()
        junk = [torch.full((1 << s,), float("nan"), dtype=torch.float32, device=dev) for s in range(12, 22) for _ in range(3)]
        torch.cuda.synchronize(dev)
        del junk
        torch.cuda.empty_cache()
        with pytest.raises(ValueError, match=r"track %d holds a non-finite value" % (n0 + 1)):
            P.append(ctx, [T[n0], bad])
        _same_state(P.snapshot(ctx, T[:n0]), want)
        P.append(ctx, T[n0:])
        _same_state(P.snapshot(ctx, T), _fresh("serra09", "all", T))
    finally:
        ctx.close()
