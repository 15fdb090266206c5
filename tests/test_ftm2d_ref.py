"""
CPU suite for FTM2D: the numpy checker (tests/_ftm2d_ref.py) against the reference's own outputs
(tests/golden/ftm2d.npz, tests/golden/make_ftm2d_goldens.py), the beat-sync edge cases, mutant checkers that must
move the shingle far beyond the GPU tolerances, and the FTM2D class's surface (no GPU needed).
"""
import inspect

import numpy as np
import pytest

from tests import _ftm2d_ref as ref

GROUPS = 2
N_PER_GROUP = 3


def _group(g, k):
    P, W, C = g["g%d_params" % k]
    tracks = [(g["g%d_X%d" % (k, i)], g["g%d_on%d" % (k, i)]) for i in range(N_PER_GROUP)]
    return float(P), int(W), float(C), tracks


@pytest.mark.parametrize("k", range(GROUPS))
def test_reference_goldens_f64_input(golden, k):
    g = golden("ftm2d")
    P, W, C, tracks = _group(g, k)
    hp = ref.beat_sync(tracks[0][0].astype(np.float64), tracks[0][1])
    np.testing.assert_array_equal(hp, g["g%d_synced_f64" % k])
    np.testing.assert_allclose(ref.chrompwr(hp, P), g["g%d_chrompwr_f64" % k], rtol=0, atol=1e-14)
    if k == 0:
        np.testing.assert_allclose(ref.fftmat(ref.chrompwr(hp, P)[:, :W + 3], W), g["g0_fftmat_f64"], rtol=0, atol=1e-12)
    S = np.stack([ref.shingle(X.astype(np.float64), on, P, W, C) for X, on in tracks])
    np.testing.assert_allclose(S, g["g%d_shingle_f64" % k], rtol=0, atol=1e-12)
    pairs = np.array([(i, j) for i in range(N_PER_GROUP) for j in range(N_PER_GROUP)])
    sim = ref.pair_scores(S, pairs).astype(np.float32).reshape(N_PER_GROUP, N_PER_GROUP)
    np.testing.assert_allclose(sim, g["g%d_sim_f64" % k], rtol=1.2e-7, atol=0)


@pytest.mark.parametrize("k", range(GROUPS))
def test_reference_goldens_f32_input(golden, k):
    """The reference on f32 chroma runs complex64 FFTs: the f64 checker stays within 1e-6 of it."""
    g = golden("ftm2d")
    P, W, C, tracks = _group(g, k)
    hp = ref.beat_sync(tracks[0][0], tracks[0][1])
    assert hp.dtype == np.float32
    np.testing.assert_array_equal(hp, g["g%d_synced_f32" % k])
    np.testing.assert_allclose(ref.chrompwr(hp.astype(np.float64), P), g["g%d_chrompwr_f32" % k], rtol=0, atol=1e-6)
    S = np.stack([ref.shingle(X, on, P, W, C) for X, on in tracks])
    np.testing.assert_allclose(S, g["g%d_shingle_f32" % k], rtol=0, atol=1e-6)
    pairs = np.array([(i, j) for i in range(N_PER_GROUP) for j in range(N_PER_GROUP)])
    sim = ref.pair_scores(S, pairs).astype(np.float32).reshape(N_PER_GROUP, N_PER_GROUP)
    np.testing.assert_allclose(sim, g["g%d_sim_f32" % k], rtol=1e-6, atol=0)


def _brute_sync(X, bounds):
    return np.stack([np.median(X[a:b], axis=0) for a, b in zip(bounds[:-1], bounds[1:])])


def test_sync_edge_cases():
    rng = np.random.default_rng(3)
    X = rng.random((40, 12)).astype(np.float32)
    # unsorted, duplicates, 0, T and beyond T; segments of length 1 (7, 8, 9)
    on = np.array([30, 7, 9, 8, 7, 0, 40, 55, 12, 30])
    b = ref.sync_bounds(40, on)
    assert b.tolist() == [0, 7, 8, 9, 12, 30, 40]
    S = ref.beat_sync(X, on)
    assert S.dtype == np.float32 and S.shape == (12, 6)
    np.testing.assert_array_equal(S.T, _brute_sync(X, b))
    np.testing.assert_array_equal(S[:, 1], X[7])                   # length-1 segment: the frame itself
    # no onsets at all: one segment, the whole track
    np.testing.assert_array_equal(ref.beat_sync(X, [])[:, 0], np.median(X, axis=0))
    # an intro of 5000 frames before the first onset
    Y = rng.random((5600, 12)).astype(np.float32)
    on = 5000 + 10 * np.arange(60)
    S = ref.beat_sync(Y, on)
    assert S.shape == (12, 61)
    np.testing.assert_array_equal(S[:, 0], np.median(Y[:5000], axis=0))
    # an even count is the f32 mean of the two middle values
    Z = np.array([[1.0], [2.0], [4.0], [8.0]], np.float32) * np.ones((1, 12), np.float32)
    assert ref.beat_sync(Z, [])[0, 0] == np.float32(3.0)
    with pytest.raises(ValueError):
        ref.sync_bounds(40, [3, -1])


@pytest.mark.parametrize("mutant", ["no_fftshift", "shift_one_axis", "mean_sync", "no_log", "no_chrompwr", "win_minus_one"])
def test_mutants_move_the_shingle(golden, mutant):
    """Every plausible slip moves some shingle by far more than the GPU tolerance (1e-6 against the f32 goldens)."""
    g = golden("ftm2d")
    worst = 0.0
    for k in range(GROUPS):
        P, W, C, tracks = _group(g, k)
        for X, on in tracks:
            good = ref.shingle(X, on, P, W, C)
            bad = ref.shingle(X, on, P, W, C, mutant=mutant)
            worst = max(worst, float(np.max(np.abs(good - bad))))
    assert worst > 1e-3, (mutant, worst)


def test_ftm2d_class_surface(tmp_path, monkeypatch):
    """Signature, name, cache prefix and similarity types of the reference's FTM2D (ftm2d.py:23-36), without a GPU."""
    from acoss_amd.algorithms import FTM2D
    from acoss_amd.featurestore import save_track
    params = list(inspect.signature(FTM2D.__init__).parameters.items())
    assert [n for n, _ in params[:8]] == ["self", "dataset_csv", "datapath", "chroma_type", "shortname", "PWR", "WIN", "C"]
    assert [p.default for _, p in params[3:8]] == ["hpcp", "Covers80", 1.96, 75, 5]
    assert [(n, p.default) for n, p in params[8:]] == [("device", None), ("nonfinite", "raise")]
    csv = tmp_path / "toy.csv"
    csv.write_text("work_id,track_id\na,t0\nb,t1\n")
    root = str(tmp_path) + "/"
    for k, l in enumerate("ab"):
        save_track(root + "%s/t%d.h5" % (l, k), {"label": l, "track_id": "t%d" % k, "hpcp": np.zeros((3, 12), np.float32)})
    monkeypatch.chdir(tmp_path)
    f = FTM2D(str(csv), root, chroma_type="crema", shortname="toy")
    assert f.name == "FTM2D" and f.N == 2 and (f.PWR, f.WIN, f.C) == (1.96, 75, 5)
    assert f.get_cacheprefix() == "cache/FTM2D_toy_crema"
    assert list(f.Ds.keys()) == ["main"] and f.Ds["main"].shape == (2, 2) and f.Ds["main"].dtype == np.float32
    assert f.shingles == {}
    f.cleanup_memmap()


def test_ftm2d_algo_constants():
    from acoss_amd import _lib
    assert _lib.ALGO_FTM2D == 4 and _lib.GRID_PLANES[_lib.ALGO_FTM2D] == 1
    p = _lib.Ftm2dParams()
    _lib.load().acx_ftm2d_default_params(p)
    assert (p.pwr, p.win, p.c) == (1.96, 75, 5.0)
    # the grid of N tracks is planned on lengths 1: every pair costs the same
    plan = _lib.grid_plan(np.ones(300, np.int64), _lib.ALGO_FTM2D, True, world=3)
    assert plan["floats_per_rank"].sum() >= 300 * 299 // 2
