"""
GPU tests of fused scores for query shortlists (run with -m gpu on a real MI355X): acx_query_fused_lists and
CoverAlgorithm.rerank_fused / rerank_tracks_fused / identify_cascade_fused.  Every comparison is equality of
indices, of score BITS and of flags.  The yardstick is the composition of exports that existed before it, per neighbourhood
(tests/_fused_ref.py with the library's own entry points handed in): acx_chenfusion_pairs / acx_earlyfusion_pairs, the host
mirror and transform, acx_snf_fuse_dists, the row, acx_topk_rows.  None comes from the code under test.
Sizes: with K = 20 the neighbourhoods run over n in {22, 23, 31..33, 63..65, 129, 257} -- n = K + 2, the (n + 3) / 4 rows per
workgroup of the wave kernels, the 32 x 32 tile, the 64-lane wave, the 256-thread row loops --, with K = 2 over {4, 5};
one query has n = 257.  Tracks are synthetic and short.
"""
import os

import numpy as np
import pytest

from . import _fused_ref as fref
from .test_gpu_query import _bits, _launches

pytestmark = pytest.mark.gpu

NS = [22, 23, 31, 32, 33, 63, 64, 65, 129, 257]
N_CHEN = 260                       # ordinary tracks of the ChenFusion pool; two planted ones behind them
PLANTED = (N_CHEN, N_CHEN + 1)
N_EF = 130
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "snf_fuse_dists_n257_m3.npy")


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("idx", "score", "flag")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        if name == "score":
            assert np.array_equal(_bits(g), _bits(w)), (what, name)
        else:
            assert np.array_equal(g, w), (what, name)


def _chen_tracks():
    """260 short cover tracks and two planted tracks of 210 frames: with pct_mode = 1 and kappa = 0.095 the percentile position
    of a row of 200 other cells is the integer 19 and both interpolation weights are 0 (tests/test_oracle_serra09.py) -- every
    plot with such a track is empty, its raw scores are 0."""
    from acoss_amd import synth
    d = synth.cover_set(clique_sizes=[2] * (N_CHEN // 2), seed=41, t_range=(60, 150))
    rng = np.random.default_rng(200)
    tracks = [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for i in range(N_CHEN)]
    tracks += [synth._frame_max_normalise(rng.random((210, 12))) for _ in PLANTED]
    return tracks


class _Pool(object):
    """One context with an uploaded pool and the yardstick over it; pair scores and fusions of a neighbourhood are computed
    once and shared among the tests."""

    def __init__(self, name):
        from acoss_amd import _lib, synth
        self.ctx = _lib.Context(0)
        self.name = name
        self._cache = {}
        if name == "chen":
            frames, offsets = synth.pack(_chen_tracks())
            self.ctx.upload_pool(frames, offsets)
            self.algo, self.params = _lib.ALGO_CHENFUSION, _lib.serra09_params(pct_mode=1)
            self.col, self.mode, self.transform = np.sqrt(np.diff(offsets).astype(np.float64)), 2, _lib.FUSED_SQRTLEN
            self.pair_fn = lambda pr: self.ctx.chenfusion_pairs(pr, self.params)
            self.types = {"Late": (0, 1)}
            self.n = len(offsets) - 1
        else:
            self.ctx.ef_upload_pool(synth.earlyfusion_set(N_EF, seed=8, nb_range=(20, 32)))
            self.algo, self.params = _lib.ALGO_EARLYFUSION, _lib.EfParams(0.1, 10)
            self.col, self.mode, self.transform = None, 0, _lib.FUSED_INV1P
            self.pair_fn = lambda pr: self.ctx.earlyfusion_pairs(pr, kappa=0.1, K=10)
            self.types = {"late": (2, 1, 0), "early+late": (2, 1, 0, 3)}          # chromas, ssms, mfccs (, early) as planes
            self.n = N_EF

    def call(self, queries, lists, k, types=None, K=20, niters=20):
        from acoss_amd import _lib
        types = list(self.types) if types is None else types
        spec = _lib.fused_spec([self.types[t] for t in types], self.transform, K=K, niters=niters)
        return self.ctx.query_fused_lists(self.algo, True, self.params, queries, lists, k, spec, col=self.col, col_mode=self.mode)

    def want(self, queries, lists, k, types=None, K=20, niters=20):
        types = list(self.types) if types is None else types
        ctx = self.ctx

        def scores(pairs):
            key = ("s", pairs.tobytes())
            if key not in self._cache:
                self._cache[key] = np.asarray(self.pair_fn(pairs), np.float32)
            return self._cache[key]

        def fuse(Ds, K_, niters_):
            key = ("f", K_, niters_) + tuple(D.tobytes() for D in Ds)
            if key not in self._cache:
                self._cache[key] = ctx.snf_fuse_dists(Ds, K=K_, niters=niters_, reg_diag=1.0, mu=0.5)[1]
            return self._cache[key]

        def rank(row32, qpos, T, k_):
            M = np.zeros((len(T), len(T)), np.float32)
            M[qpos] = row32
            i, s = ctx.topk_rows(M, k_, rows=[qpos])
            return np.where(i[0] >= 0, T[np.maximum(i[0], 0)], -1).astype(np.int32), s[0]

        return fref.rerank_fused(scores, fuse, queries, lists, k, [self.types[t] for t in types], self.transform, col=self.col,
                                 K=K, niters=niters, rank=rank)


@pytest.fixture(scope="module")
def chen():
    p = _Pool("chen")
    yield p
    p.ctx.close()


@pytest.fixture(scope="module")
def ef():
    p = _Pool("ef")
    yield p
    p.ctx.close()


def _ragged(rng, n_pool, ns, L, own_rows=(), queries=None):
    """One query and one row of L slots per entry of ns: n - 1 other tracks at random slots, -1 elsewhere (at any position); in
    own_rows the query is listed in its own row as well."""
    Q = len(ns)
    if queries is None:
        queries = rng.integers(0, n_pool, Q)
    lists = np.full((Q, L), -1, np.int32)
    for i, n in enumerate(ns):
        others = rng.choice(np.setdiff1d(np.arange(n_pool), [queries[i]]), n - 1, replace=False)
        entries = np.concatenate([others, [queries[i]]]) if i in own_rows else others
        lists[i, rng.choice(L, len(entries), replace=False)] = entries
    return np.asarray(queries, np.int32), lists


@pytest.fixture(scope="module")
def chen_case():
    rng = np.random.default_rng(17)
    queries = rng.integers(0, N_CHEN, len(NS))
    queries[1] = queries[0]                                   # the same query twice, with different lists
    order = [0, 1, 2, 3, 9, 4, 5, 6, 7, 8]                   # n = 257 in the middle of the call
    ns = [NS[i] for i in order]
    q, lists = _ragged(rng, N_CHEN, ns, 260, own_rows=(2, 4, 7), queries=queries)
    return q, lists, ns


def test_chenfusion_late_every_size_in_one_call(chen, chen_case):
    """m = 2.  Ragged lists, -1 anywhere, the query listed in its own row, a duplicate query, neighbourhoods of every size in
    one call, k below and above the list."""
    q, lists, ns = chen_case
    assert q[0] == q[1] and not np.array_equal(lists[0], lists[1])
    assert [len(fref.neighbourhood(a, r)[0]) for a, r in zip(q, lists)] == ns
    for k in (10, 300):
        got = chen.call(q, lists, k)
        assert got[0].shape == (len(q), 1, k) and got[2].shape == (len(q), 1)
        _same(got, chen.want(q, lists, k), k)
        assert not got[2].any() and not np.isnan(got[1][:, :, :min(k, 21)]).any()
        for i, n in enumerate(ns):
            assert q[i] not in got[0][i] and np.all(got[0][i, 0, :min(k, n - 1)] >= 0)
            assert np.all(got[0][i, 0, n - 1:] == -1) and np.all(np.isnan(got[1][i, 0, n - 1:])), "k larger than the list"


def test_rows_and_entries_in_any_order(chen, chen_case):
    q, lists, _ = chen_case
    rng = np.random.default_rng(3)
    base = chen.call(q, lists, 12)
    perm = rng.permutation(len(q))
    shuffled = np.stack([rng.permutation(lists[i]) for i in perm])
    got = chen.call(q[perm], shuffled, 12)
    _same(got, tuple(a[perm] for a in base), "shuffled")


def test_two_chunks_equal_one(chen, chen_case):
    """Half of the lowered limit holds the n = 257 problem alone: the call takes three chunks (before it, it, behind it) and
    returns the bits of the one-chunk call; a limit below that problem is refused with nothing launched, and the context goes on."""
    q, lists, ns = chen_case
    ctx = chen.ctx
    base = chen.call(q, lists, 10)
    n, W, M, K, nt, k = 257, 2, 2, 20, 1, 10
    one = n * (n - 1) // 2 * W * 4 + 8 * ((3 * M + 2) * n * n + n) + 12 * M * n * K + 4 * n + 40 + nt * (8 * k + 1)
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        chen.call(q, lists, 10)
        assert ctx.profile()["fused_row_kernel"]["launches"] == 1
        ctx.set_scratch_limit(2 * one + 8)
        ctx.profile_reset()
        _same(chen.call(q, lists, 10), base, "chunks")
        prof = ctx.profile()
        assert prof["fused_row_kernel"]["launches"] == 3 and prof["fused_stage_kernel"]["launches"] == 3
        assert prof["snf_batch_prepare_kernels"]["launches"] == 3 and prof["snf_batch_update_kernels"]["launches"] == 3
        ctx.set_scratch_limit(2 * one - 2)
        ctx.profile_reset()
        with pytest.raises(MemoryError, match="lists row 4"):
            chen.call(q, lists, 10)
        assert _launches(ctx) == 0
    finally:
        ctx.set_scratch_limit(0)
        ctx.profile_enable(False)
    _same(chen.call(q, lists, 10), base, "after the refusal")


def test_small_K(chen):
    """K = 2, niters = 2: n in {4, 5} (n = K + 2 and one more)."""
    rng = np.random.default_rng(5)
    q, lists = _ragged(rng, N_CHEN, [4, 5, 5, 4], 6, own_rows=(1,))
    got = chen.call(q, lists, 6, K=2, niters=2)
    _same(got, chen.want(q, lists, 6, K=2, niters=2))
    assert not got[2].any()


def test_planted_zero_score(chen):
    """The planted pair has raw score 0 on the CPU oracle; on the device a neighbourhood that holds a planted track has an
    infinite distance: its flag is set and its row is NaN (ranked by index), the other queries keep their bits."""
    import oracle
    tracks = _chen_tracks()
    for dmax in (0, 1):
        assert oracle.serra09_pair(tracks[PLANTED[0]], tracks[PLANTED[1]], oracle.serra09_params(pct_mode=1, dmax=dmax)) == 0.0
    assert np.all(chen.pair_fn(np.array([[PLANTED[0], PLANTED[1]], [5, PLANTED[0]]], np.int32)) == 0.0)
    rng = np.random.default_rng(9)
    q, lists = _ragged(rng, N_CHEN, [24, 30, 26], 40)
    clean = chen.call(q, lists, 8)
    assert not clean[2].any()
    lists2 = lists.copy()
    lists2[1, np.nonzero(lists2[1] < 0)[0][:2]] = PLANTED
    got = chen.call(q, lists2, 8)
    _same(got, chen.want(q, lists2, 8), "planted")
    assert got[2][:, 0].tolist() == [0, 1, 0] and np.all(np.isnan(got[1][1]))
    others = np.sort(np.setdiff1d(lists2[1][lists2[1] >= 0], [q[1]]))
    assert np.array_equal(got[0][1, 0], others[:8]), "a NaN row lists its tracks in index order"
    for i in (0, 2):
        _same(tuple(a[i] for a in got), tuple(a[i] for a in clean), "untouched")


def test_refusals_launch_nothing(chen):
    from acoss_amd import _lib
    ctx = chen.ctx
    rng = np.random.default_rng(2)
    q, lists = _ragged(rng, N_CHEN, [25, 22], 30)
    spec = lambda **kw: _lib.fused_spec([(0, 1)], _lib.FUSED_SQRTLEN, **kw)
    call = lambda f=None, lists=lists, sym=True, mode=2, col=chen.col, k=5: ctx.query_fused_lists(
        _lib.ALGO_CHENFUSION, sym, chen.params, q, lists, k, f or spec(), col=col, col_mode=mode)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        twice = lists.copy()
        twice[0, np.nonzero(twice[0] < 0)[0][0]] = twice[0][twice[0] >= 0][0]
        with pytest.raises(ValueError, match="twice"):
            call(lists=twice)
        short = lists.copy()
        short[1, np.nonzero(short[1] >= 0)[0][0]] = -1
        with pytest.raises(ValueError, match=r"lists row 1 .* 21 tracks"):
            call(lists=short)
        with pytest.raises(NotImplementedError, match="64 neighbours"):
            call(spec(K=65))
        with pytest.raises(ValueError, match="niters"):
            call(spec(niters=0))
        with pytest.raises(ValueError, match="K must be"):
            call(spec(K=0))
        with pytest.raises(NotImplementedError, match="list_len"):
            call(lists=np.full((2, 1025), -1, np.int32))
        bad = spec()
        bad.reserved = 1
        with pytest.raises(ValueError, match="reserved"):
            call(bad)
        bad = spec()
        bad.planes[0][1] = 2
        with pytest.raises(ValueError, match="planes"):
            call(bad)
        with pytest.raises(ValueError, match="symmetric"):
            call(sym=False)
        with pytest.raises(ValueError, match="col_mode"):
            call(mode=1)
        with pytest.raises(NotImplementedError, match="over the limit"):
            call(k=1025)
        with pytest.raises(ValueError, match="ACX_ALGO"):
            ctx.query_fused_lists(_lib.ALGO_SERRA09, True, chen.params, q, lists, 5, spec(), col=chen.col, col_mode=2)
        assert _launches(ctx) == 0, "a refused call launches nothing"
        got = call()
        assert _launches(ctx) > 0
    finally:
        ctx.profile_enable(False)
    _same(got, chen.want(q, lists, 5), "after the refusals")
    empty = ctx.query_fused_lists(_lib.ALGO_CHENFUSION, True, chen.params, [], np.zeros((0, 4), np.int32), 3, spec(), col=chen.col, col_mode=2)
    assert empty[0].shape == (0, 1, 3) and empty[2].shape == (0, 1)


def test_earlyfusion_both_types_one_call_and_separately(ef):
    """m = 3 and m = 4: 'late' and 'early+late' from one call (the pairs scored once: the pair kernels run as often as for one
    type) equal each on its own and the yardstick."""
    rng = np.random.default_rng(23)
    ns = [22, 23, 31, 32, 33, 63, 64, 65, 129]
    q, lists = _ragged(rng, N_EF, ns, 129, own_rows=(0, 5))
    ctx = ef.ctx
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        both = ef.call(q, lists, 9)
        p2 = ctx.profile()
        ctx.profile_reset()
        late = ef.call(q, lists, 9, types=["late"])
        p1 = ctx.profile()
    finally:
        ctx.profile_enable(False)
    assert both[0].shape == (len(q), 2, 9)
    assert p2["fused_row_kernel"]["launches"] == 2 and p1["fused_row_kernel"]["launches"] == 1
    mine = ("fused_stage_kernel", "snf_batch_prepare_kernels", "snf_batch_update_kernels", "fused_row_kernel")
    pair_launches = lambda p: sum(v["launches"] for name, v in p.items() if name not in mine)
    assert pair_launches(p2) == pair_launches(p1) > 0, "scored once, fused twice"
    el = ef.call(q, lists, 9, types=["early+late"])
    _same(tuple(a[:, :1] for a in both), late, "late")
    _same(tuple(a[:, 1:] for a in both), el, "early+late")
    _same(both, ef.want(q, lists, 9), "yardstick")
    assert not both[2].any() and not np.isnan(both[1]).any()
    swapped = ef.call(q, lists, 9, types=["early+late", "late"])
    _same(tuple(a[:, ::-1] for a in swapped), both, "the order of the types")


def test_snf_fuse_dists_keeps_the_parent_bits():
    """acx_snf_fuse_dists on the whole-run case of tests/test_gpu_snf.py at n = 257, m = 3 (K = 7, 5 sweeps), against the bits
    recorded from the build before the kernels' row bodies became shared device functions."""
    from acoss_amd import _lib
    from .test_gpu_snf import _scores
    rng = np.random.default_rng(257 + 3)
    Scores = _scores(rng, 257, 3)
    c = _lib.Context(0)
    try:
        got = c.snf_fuse_dists(Scores, K=7, niters=5, reg_diag=1)[1]
    finally:
        c.close()
    want = np.load(GOLDEN)
    assert want.shape == (257, 257) and want.dtype == np.float64
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


# ------------------------------------------------------------------------------------------------ the classes
def _make(cls_name, tmp_path, tag, tracks):
    from acoss_amd import algorithms
    csv = os.path.join(str(tmp_path), tag + ".csv")
    with open(csv, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(len(tracks)):
            f.write("w%d,%s%d\n" % (i // 2, tag, i))
    a = getattr(algorithms, cls_name)(csv, "feat/", shortname=tag)
    labels = ["w%d" % (i // 2) for i in range(len(tracks))]
    (a.set_pooled_features if cls_name == "ChenFusion" else a.set_block_features)(tracks, labels)
    return a


def _class_tracks(cls_name, n):
    from acoss_amd import synth
    if cls_name == "ChenFusion":
        d = synth.cover_set(clique_sizes=[2] * (n // 2), seed=12, t_range=(60, 150))
        return [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for i in range(n)]
    return synth.earlyfusion_set(n, seed=6, nb_range=(20, 40))


@pytest.mark.parametrize("cls_name", ["ChenFusion", "EarlyFusion"])
def test_class_equals_the_sequence_on_the_subcollection(tmp_path, monkeypatch, cls_name):
    """rerank_fused on a 40-track collection against an object built over the sub-collection T and run through the existing
    sequence: all_pairwise, normalize_by_length where the class has one, do_late_fusion, top_matches(type, k, rows=[position])."""
    monkeypatch.chdir(tmp_path)
    tracks = _class_tracks(cls_name, 40)
    algo = _make(cls_name, tmp_path, "all", tracks)
    rng = np.random.default_rng(1)
    q, lists = _ragged(rng, 40, [22, 27, 40], 39, own_rows=())
    got = algo.rerank_fused(q, lists, k=7)
    assert sorted(got) == sorted(algo._identify_fused)
    for i in range(len(q)):
        T, pos = fref.neighbourhood(q[i], lists[i])
        sub = _make(cls_name, tmp_path, "sub%d" % i, [tracks[t] for t in T])
        sub.all_pairwise(symmetric=True)
        if hasattr(sub, "normalize_by_length"):
            sub.normalize_by_length()
        sub.do_late_fusion()
        for t in algo._identify_fused:
            wi, ws = sub.top_matches(t, 7, rows=[pos])
            assert np.array_equal(got[t][0][i], np.where(wi[0] >= 0, T[np.maximum(wi[0], 0)], -1)), (t, i)
            assert np.array_equal(_bits(got[t][1][i]), _bits(ws[0])), (t, i)
        sub.cleanup_memmap()
    for t in algo.Ds:
        assert not np.any(np.asarray(algo.Ds[t])), "rerank_fused must not write Ds"
    one = algo.rerank_fused(q, lists, k=7, similarity_types=[algo._identify_fused[-1]])
    t = algo._identify_fused[-1]
    assert list(one) == [t] and np.array_equal(one[t][0], got[t][0]) and np.array_equal(_bits(one[t][1]), _bits(got[t][1]))
    algo.cleanup_memmap()


@pytest.mark.parametrize("cls_name", ["ChenFusion", "EarlyFusion"])
def test_session_and_tracks_forms(tmp_path, monkeypatch, cls_name):
    """Inside appended(), rerank_fused over [0, N + Q) equals the call on an object built over the N + Q tracks;
    rerank_tracks_fused equals the session form; identify_cascade_fused is rerank_fused on the first stage's lists."""
    monkeypatch.chdir(tmp_path)
    tracks = _class_tracks(cls_name, 30)
    N, Q = 27, 3
    part, whole = _make(cls_name, tmp_path, "part", tracks[:N]), _make(cls_name, tmp_path, "whole", tracks)
    rng = np.random.default_rng(4)
    q, lists = _ragged(rng, 30, [23, 22, 25, 24], 29, queries=np.array([N + 1, 3, N, 11]))
    assert lists.max() >= N, "shortlists reach into the appended tracks"
    want = whole.rerank_fused(q, lists, k=6)
    with part.appended(tracks[N:]) as s:
        assert s.total == 30
        got = part.rerank_fused(q, lists, k=6)
        with pytest.raises(RuntimeError, match="rerank_tracks_fused"):
            part.rerank_tracks_fused(tracks[N:], lists[:Q])
    for t in want:
        assert np.array_equal(got[t][0], want[t][0]) and np.array_equal(_bits(got[t][1]), _bits(want[t][1])), t
    _, short = _ragged(rng, N, [22, 24, 23], N - 1, queries=np.arange(N, N + Q))
    with part.appended(tracks[N:]) as s:
        want2 = part.rerank_fused(s.indices, short, k=5)
    got2 = part.rerank_tracks_fused(tracks[N:], short, k=5)
    for t in want2:
        assert np.array_equal(got2[t][0], want2[t][0]) and np.array_equal(_bits(got2[t][1]), _bits(want2[t][1])), t
    # the cascade: the class itself as its own first stage
    first_type = whole._identify_planes[0]
    qs = [4, 19]
    shortlists = whole.identify(qs, k=25, similarity_types=[first_type])[first_type][0]
    casc = whole.identify_cascade_fused(whole, qs, k=5, shortlist=25)
    direct = whole.rerank_fused(qs, shortlists, k=5)
    for t in direct:
        assert np.array_equal(casc[t][0], direct[t][0]) and np.array_equal(_bits(casc[t][1]), _bits(direct[t][1])), t
    part.cleanup_memmap()
    whole.cleanup_memmap()
