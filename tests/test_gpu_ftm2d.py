"""
GPU tests of FTM2D (run with -m gpu on a real MI355X): the shingle chain stage by stage against numpy
(tests/_ftm2d_ref.py) on the device's own intermediates, the full shingle against the reference's goldens, pair scores,
the pair grid, streamed uploads, failure paths and the class end to end.

Bounds: stage 1 (beat sync) and stage 5's median are bit-identical to np.median; stages 2-4 (chrompwr, the 2D DFT
magnitudes, window norm, log) are f64 from the same inputs in another order, within 1e-10 absolute (values <= ~10);
the shingle within 1e-6 of the reference's f32-input run (which uses complex64 FFTs); pair scores within one f32 ulp
of f64 numpy on the downloaded shingles.
"""
import numpy as np
import pytest

from tests import _ftm2d_ref as ref

pytestmark = pytest.mark.gpu
STAGE_ATOL = 1e-10


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _track(rng, nbeats, intro=0, fpb=(1, 9), tail=3):
    """Chroma (T, 12) f32 and shuffled onsets giving exactly `nbeats` segments (intro frames before the first onset)."""
    lens = rng.integers(fpb[0], fpb[1] + 1, nbeats if intro == 0 else nbeats - 1)
    starts = intro + np.concatenate([[0], np.cumsum(lens)[:-1]])
    T = int(intro + lens.sum() + (0 if intro == 0 else tail))
    if intro == 0:
        T = int(lens.sum())
    X = (rng.random((T, 12)) ** 2).astype(np.float32)
    on = np.concatenate([starts, starts[:3], [T, T + 5]]).astype(np.int64)        # duplicates, T and beyond
    on = rng.permutation(on)
    assert len(ref.sync_bounds(T, on)) - 1 == nbeats
    return X, on


CASES = [(1, 1), (1, 2), (1, 2600), (2, 2), (2, 700), (3, 3), (3, 4), (16, 16), (16, 17), (16, 90), (37, 37), (37, 38),
         (74, 80), (75, 75), (75, 76), (75, 160), (76, 77), (128, 128), (128, 129), (256, 256), (256, 257), (256, 300)]


def _check_stages(got, X, on, pwr, win, C, nbeats):
    """What acx_ftm2d_debug_track returned for (X, on), stage by stage, each from the device's previous one, and the whole chain."""
    # stage 1: bit-identical to np.median per bin and segment
    np.testing.assert_array_equal(got["synced"], ref.beat_sync(X, on).T)
    # stage 2 from the device's stage 1
    want_pwr = ref.chrompwr(got["synced"].T.astype(np.float64), pwr).T
    assert np.max(np.abs(got["pwr"] - want_pwr)) <= STAGE_ATOL
    # stages 3-4 from the device's stage 2
    sh = ref.fftmat(got["pwr"].T, win).T
    nrm = np.sqrt(np.sum(sh ** 2, 1))
    nrm[nrm == 0] = 1
    want_lw = np.log(C * sh / nrm[:, None] + 1)
    assert got["logwin"].shape == (nbeats - win + 1, 12 * win)
    assert np.max(np.abs(got["logwin"] - want_lw)) <= STAGE_ATOL, np.max(np.abs(got["logwin"] - want_lw))
    # stage 5: the median bit-identical to np.median of the device's window matrix, then the norm
    np.testing.assert_array_equal(got["median"], np.median(got["logwin"], 0))
    want_sh = got["median"] / np.sqrt(np.sum(got["median"] ** 2))
    np.testing.assert_allclose(got["shingle"], want_sh, rtol=1e-14, atol=1e-15)
    # and the whole chain against the checker on the raw input
    full = ref.stages(X, on, pwr, win, C)
    assert np.max(np.abs(got["shingle"] - full["shingle"])) <= 1e-9


@pytest.mark.parametrize("win,nbeats", CASES)
def test_stages_against_numpy(ctx, win, nbeats):
    rng = np.random.default_rng(1000 * win + nbeats)
    pwr, C = ((0.5, 1.0), (1.96, 5.0))[(win + nbeats) % 2]
    X, on = _track(rng, nbeats, intro=5000 if nbeats == 90 else 0)
    _check_stages(ctx.ftm2d_debug_track(X, on, pwr, win, C), X, on, pwr, win, C, nbeats)


@pytest.mark.parametrize("k", [0, 1])
def test_shingles_match_reference_goldens(ctx, golden, k):
    g = golden("ftm2d")
    P, W, C = g["g%d_params" % k]
    tracks = [dict(chroma=g["g%d_X%d" % (k, i)], onsets=g["g%d_on%d" % (k, i)]) for i in range(3)]
    ctx.ftm2d_upload_raw_pool(tracks, P, int(W), C)
    S = ctx.ftm2d_download_shingles()
    assert np.max(np.abs(S - g["g%d_shingle_f32" % k])) <= 1e-6
    for i, t in enumerate(tracks):      # the debug entry runs the same kernels: the same bits
        np.testing.assert_array_equal(ctx.ftm2d_debug_track(t["chroma"], t["onsets"], P, int(W), C)["shingle"], S[i])
    got = ctx.ftm2d_pairs(np.array([(i, j) for i in range(3) for j in range(3)])).reshape(3, 3)
    np.testing.assert_allclose(got, g["g%d_sim_f32" % k], rtol=2e-6, atol=0)


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _random_shingles(rng, n, D=900):
    S = rng.random((n, D)) ** 4
    return S / np.linalg.norm(S, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, (n, 1))


def test_pairs_against_f64(ctx):
    from acoss_amd import synth
    tracks, _ = synth.ftm2d_cover_set(n_works=4, versions=3, seed=5)
    ctx.ftm2d_upload_raw_pool(tracks)
    S = ctx.ftm2d_download_shingles()
    n = len(S)
    pairs = np.array([(i, j) for i in range(n) for j in range(n)], np.int32)
    got = ctx.ftm2d_pairs(pairs)
    want = ref.pair_scores(S, pairs)
    assert _ulps(got, want.astype(np.float32)).max() <= 1
    assert np.all(got[pairs[:, 0] == pairs[:, 1]] == 1.0)
    assert ctx.ftm2d_pairs(np.zeros((0, 2), np.int32)).shape == (0,)


@pytest.mark.parametrize("n", [1, 2, 129, 257, 2100])
def test_pair_grid_equals_pairs(ctx, n):
    from acoss_amd import _lib
    rng = np.random.default_rng(n)
    S = _random_shingles(rng, n)
    S[n // 2] *= 0.2                                        # spread the scores
    ctx.ftm2d_upload_shingles(S)
    lengths = ctx.pool_lengths(_lib.ALGO_FTM2D)
    assert lengths.tolist() == [1] * n
    i, j = np.nonzero(~np.eye(n, dtype=bool))
    pairs = np.stack([i, j], 1).astype(np.int32)
    want = np.zeros((n, n), np.float32)
    if len(pairs):
        want[i, j] = ctx.ftm2d_pairs(pairs)
        sub = pairs[rng.permutation(len(pairs))[:20000]]
        assert _ulps(want[sub[:, 0], sub[:, 1]], ref.pair_scores(S, sub).astype(np.float32)).max() <= 1
    for sym in (True, False):
        D = np.zeros((n, n), np.float32)
        ctx.pair_grid(_lib.ALGO_FTM2D, sym, None, [D], mirror=sym)
        assert np.all(np.diag(D) == 0)
        np.testing.assert_array_equal(D, want)              # symmetric: the mirror of i < j equals the pair (j, i) bit for bit
        if sym:
            np.testing.assert_array_equal(D, D.T)
    if n in (129, 257):         # 3 ranks, whole and tile by tile, through device buffers and acx_grid_scatter
        for sym in (True, False):
            plan = _lib.grid_plan(lengths, _lib.ALGO_FTM2D, sym, world=3, tile=64, want_tiles=True)
            stride = int(plan["floats_per_rank"].max())
            for sliced in (False, True):
                bufs = []
                for r in range(3):
                    buf = ctx.dev_alloc(4 * stride)
                    if sliced:
                        for k in range(sum(1 for tl in plan["tiles"] if tl.rank == r)):
                            ctx.grid_run(plan["spec"], None, r, buf.ptr, first=k, count=1)
                    else:
                        ctx.grid_run(plan["spec"], None, r, buf.ptr)
                    bufs.append(buf.read(np.float32, stride))
                    buf.free()
                D = np.zeros((n, n), np.float32)
                _lib.grid_scatter(lengths, plan["spec"], np.concatenate(bufs), stride, [D], mirror=sym)
                np.testing.assert_array_equal(D, want)


def test_streamed_batches_are_bit_identical(ctx):
    from acoss_amd import synth
    tracks, _ = synth.ftm2d_cover_set(n_works=5, versions=3, seed=8)
    ctx.ftm2d_upload_raw_pool(tracks, batch=len(tracks))
    one = ctx.ftm2d_download_shingles()
    ctx.ftm2d_upload_raw_pool(tracks, batch=4)
    np.testing.assert_array_equal(ctx.ftm2d_download_shingles(), one)
    # out of order, a slice handed over twice, and sub-batches forced by a small scratch limit
    ctx.set_scratch_limit(3 * 900 * 8 * 100)
    try:
        n = len(tracks)
        ctx.ftm2d_pool_begin(n)
        ctx.ftm2d_pool_tracks(7, tracks[7:])
        ctx.ftm2d_pool_tracks(0, tracks[:7])
        ctx.ftm2d_pool_tracks(3, tracks[3:5])
        ctx.ftm2d_pool_end()
    finally:
        ctx.set_scratch_limit(0)
    np.testing.assert_array_equal(ctx.ftm2d_download_shingles(), one)


def test_failure_paths_leave_the_context_usable(ctx):
    from acoss_amd import _lib, synth
    tracks, _ = synth.ftm2d_cover_set(n_works=2, versions=2, seed=3)
    ctx.ftm2d_upload_raw_pool(tracks)
    good = ctx.ftm2d_download_shingles()
    short = [dict(t) for t in tracks]
    short[2] = dict(chroma=tracks[2]["chroma"], onsets=tracks[2]["onsets"][:50])
    with pytest.raises(ValueError, match="track 2 has"):
        ctx.ftm2d_upload_raw_pool(short)
    neg = [dict(t) for t in tracks]
    neg[3] = dict(chroma=tracks[3]["chroma"], onsets=np.concatenate([tracks[3]["onsets"], [-4]]))
    with pytest.raises(ValueError, match="track 3 has a negative onset"):
        ctx.ftm2d_upload_raw_pool(neg)
    with pytest.raises(ValueError, match="WIN"):
        ctx.ftm2d_pool_begin(4, win=257)
    with pytest.raises(ValueError, match="WIN"):
        ctx.ftm2d_pool_begin(4, win=0)
    # the pool left open by the failures: pool_end names the first missing track
    ctx.ftm2d_pool_begin(len(tracks))
    ctx.ftm2d_pool_tracks(0, tracks[:1])
    with pytest.raises(_lib.AcxError, match="track 1 was never handed over"):
        ctx.ftm2d_pool_end()
    # NaN chroma: rejected naming the track, or zeroed
    bad = [dict(t) for t in tracks]
    ch = tracks[1]["chroma"].copy()
    ch[17, 4] = np.nan
    bad[1] = dict(chroma=ch, onsets=tracks[1]["onsets"])
    with pytest.raises(ValueError, match="track 1 holds a non-finite"):
        ctx.ftm2d_upload_raw_pool(bad)
    ctx.set_nonfinite_policy("zero")
    try:
        ctx.ftm2d_upload_raw_pool(bad)
        assert ctx.nonfinite_zeroed() == 1
        ch0 = ch.copy()
        ch0[17, 4] = 0
        np.testing.assert_array_equal(ctx.ftm2d_download_shingles()[1], ctx.ftm2d_debug_track(ch0, tracks[1]["onsets"])["shingle"])
    finally:
        ctx.set_nonfinite_policy("raise")
    # the context still works and gives the same shingles as before
    ctx.ftm2d_upload_raw_pool(tracks)
    np.testing.assert_array_equal(ctx.ftm2d_download_shingles(), good)
    with pytest.raises(ValueError, match="out of range in pair 1"):
        ctx.ftm2d_pairs(np.array([[0, 1], [0, len(tracks)]]))
    with pytest.raises(ValueError, match="out of range"):
        ctx.ftm2d_pairs(np.array([[-1, 0]]))
    assert ctx.ftm2d_pairs(np.array([[0, 0]]))[0] == 1.0
    # a silent track: NaN shingle, NaN scores (as the reference)
    silent = [dict(t) for t in tracks]
    silent[0] = dict(chroma=np.zeros_like(tracks[0]["chroma"]), onsets=tracks[0]["onsets"])
    ctx.ftm2d_upload_raw_pool(silent)
    S = ctx.ftm2d_download_shingles()
    assert np.all(np.isnan(S[0])) and np.all(np.isfinite(S[1:]))
    sc = ctx.ftm2d_pairs(np.array([[0, 1], [1, 0], [0, 0], [1, 2]]))
    assert np.isnan(sc[:3]).all() and np.isfinite(sc[3])
    assert np.isnan(ref.shingle(silent[0]["chroma"], silent[0]["onsets"])).all()
    D = np.zeros((len(tracks), len(tracks)), np.float32)
    ctx.pair_grid(_lib.ALGO_FTM2D, True, None, [D], mirror=True)
    assert np.isnan(D[0, 1:]).all() and np.isfinite(D[1:, 1:]).all()


def test_end_to_end_from_feature_files(tmp_path, monkeypatch):
    from acoss_amd import synth
    from acoss_amd.algorithms import FTM2D
    from acoss_amd.algorithms.algorithm_template import eval_statistics
    from acoss_amd.featurestore import save_track
    tracks, labels = synth.ftm2d_cover_set(n_works=12, versions=4, seed=21)
    csv = tmp_path / "ftm.csv"
    root = str(tmp_path) + "/feat/"
    with open(csv, "w") as f:
        f.write("work_id,track_id\n")
        for k, (t, l) in enumerate(zip(tracks, labels)):
            f.write("%s,t%d\n" % (l, k))
            save_track(root + "%s/t%d.h5" % (l, k), {"label": l, "track_id": "t%d" % k, "hpcp": t["chroma"],
                                                      "madmom_features": {"onsets": t["onsets"]}})
    monkeypatch.chdir(tmp_path)
    algo = FTM2D(str(csv), root, shortname="synth")
    algo.upload_batch = 10           # several streamed batches
    algo.all_pairwise(symmetric=True)
    MR, MRR, MDR, MAP, tops = algo.getEvalStatistics("main")
    # the checker: numpy shingles, f64 scores stored as float32, mirrored like all_pairwise
    S = np.stack([ref.shingle(t["chroma"], t["onsets"]) for t in tracks])
    n = len(tracks)
    i, j = np.triu_indices(n, 1)
    Dref = np.zeros((n, n), np.float32)
    Dref[i, j] = ref.pair_scores(S, np.stack([i, j], 1)).astype(np.float32)
    Dref += Dref.T
    cl = {}
    for k, l in enumerate(labels):
        cl.setdefault(l, []).append(k)
    MAP_ref = eval_statistics(Dref, list(cl.values()))[3]
    assert abs(MAP - MAP_ref) <= 1e-6, (MAP, MAP_ref)
    assert np.max(np.abs(np.asarray(algo.Ds["main"]) - Dref)) <= 1e-6
    assert MAP > 0.5                  # chance is ~ 3 / 47
    # load_features / similarity on the same object agree with the grid
    np.testing.assert_array_equal(algo.load_features(3), algo.shingles[3])
    algo.Ds["main"][:] = 0
    algo.similarity(np.array([[0, 5], [7, 2]]))
    assert abs(algo.Ds["main"][0, 5] - Dref[0, 5]) <= 1e-6 and abs(algo.Ds["main"][7, 2] - Dref[7, 2]) <= 1e-6
    algo.cleanup_memmap()
