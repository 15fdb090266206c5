"""
CPU suite for the EarlyFusion block features: the independent longdouble reference (tests/_efprep_ref.py: the resize as
clip(L @ G @ x) with explicit operators) against
  - the reference project's own outputs with the real scikit-image (tests/golden/efprep_skimage.npz): all twelve
    resize_block cases within 1e-12 (a scipy.ndimage formulation differs from them by 8.4e-14: a tenfold margin for
    another summation order), and the four load_features tracks (f32) within the bounds the GPU tests use;
  - scipy.ndimage (gaussian_filter1d(mode='constant', truncate=4.0), then map_coordinates(order=1,
    mode='grid-constant')) at every shape the GPU tests run, and at the radii 512, 513 and 1198 -- past what the device
    evaluates -- within 1e-12;
  - oracle.ef_block_features at the same shapes, so that the oracle is pinned at the edges too.
"""
import numpy as np
import pytest

from tests import _efprep_ref as ref

LD = np.longdouble
ROWS = (40, 1, 50, 2, 64, 3)
# (n, rows) beyond the edge lengths: r = 512 / 514 at one row, 513 at two, 1198 (a 600-frame block to one row), the
# 1100-frame block to 4 and 2 rows, 10300 frames to 40 rows (r = 513)
WIDE = ((257, 1), (258, 1), (515, 2), (600, 1), (1100, 4), (1100, 2), (10300, 40))


def _shapes():
    out = [(n, rows) for rows in ROWS for n in ref.edge_lengths(rows)]
    return out + [s for s in WIDE if s not in out]


def test_the_wide_shapes_have_the_radii_they_are_there_for():
    assert [ref.radius(n, rows)[1] for n, rows in WIDE] == [512, 514, 513, 1198, 548, 1098, 513]
    for rows in ROWS:
        assert ref.radius(257 * rows, rows)[1] == ref.MAXRAD
        assert ref.radius(ref.first_blurred(rows), rows)[1] >= 1 and ref.radius(ref.first_blurred(rows) - 1, rows)[1] == 0
        n = ref.rounded_up(rows)
        assert (n is None) == (rows <= 2) and (n is None or ref.radius(n, rows)[1] == int(4.0 * ref.radius(n, rows)[0]) + 1 >= 3)


def test_operators_are_what_they_say():
    """L's rows sum to 1 inside the block; G's rows sum to 1 away from the block's ends and to less beside them."""
    L, taps = ref.interpolation_matrix(123, 40)
    assert np.all(np.abs(L.sum(axis=1) - 1) < 1e-18) and all(0 <= t0 and t0 + 1 < 123 for t0, _ in taps)
    L, _ = ref.interpolation_matrix(7, 40)          # upsampling: the outermost rows blend with the zeros outside
    assert L[0].sum() < 1 and L[-1].sum() < 1 and abs(L[20].sum() - 1) < 1e-18
    w, r = ref.gaussian_weights(400, 50)
    assert r == 14 and len(w) == 29 and abs(w.sum() - 1) < 1e-18
    assert abs(ref.gaussian_row(200, 400, w, r).sum() - 1) < 1e-18 and 0.8 < ref.gaussian_row(3, 400, w, r).sum() < 0.9
    assert not ref.gaussian_row(-1, 400, w, r).any() and not ref.gaussian_row(400, 400, w, r).any()


def test_resize_against_the_skimage_goldens(golden):
    g = golden("efprep_skimage")
    worst = 0.0
    for k, (which, i1, i2, rows) in enumerate(g["rb_cases"]):
        src = g["rb_C"] if which == 1 else g["rb_X"]
        got = ref.resize(src[i1:i2], int(rows))
        want = g["rb_out_%d" % k]
        assert got.shape == want.shape
        worst = max(worst, float(np.max(np.abs(got - want.astype(LD)))))
        assert np.max(np.abs(got - want.astype(LD))) <= 1e-12, "case %d" % k
    print("resize against skimage: max |diff| = %.3g" % worst)


def _check_f32(got, want, ncoef, what):
    """Block features rounded to f32 (`got`) against the unrounded reference (`want`) with the bounds of the GPU tests."""
    for key in ("mfccs", "chromas"):
        err = np.abs(got[key].astype(LD) - want[key])
        assert np.all(err <= ref.bound_rounded(want[key])), (what, key, float(np.max(err / ref.bound_rounded(want[key]))))
        assert not got[key][want[key] == 0].any(), (what, key)
    err = np.abs(got["ssms"].astype(LD) - want["ssms"])
    assert np.all(err <= ref.bound_ssm(want["ssms"], ncoef)), (what, "ssms", float(np.max(err / ref.bound_ssm(want["ssms"], ncoef))))


def test_block_features_against_the_load_features_goldens(golden):
    g = golden("efprep_skimage")
    for k in (0, 1, 2, 9):
        geo = (20, 50, 40) if k != 9 else (12, 32, 24)
        mfcc = np.ascontiguousarray(g["lf%d_mfcc_htk" % k].T)
        want = ref.block_features(g["lf%d_hpcp" % k], mfcc, g["lf%d_onsets" % k], *geo)
        got = {key: g["lf%d_%s" % (k, key)] for key in ("mfccs", "ssms", "chromas")}
        assert got["mfccs"].shape == want["mfccs"].shape and len(got["mfccs"]) > 0
        _check_f32(got, want, mfcc.shape[1], "lf%d" % k)
        assert np.array_equal(g["lf%d_chroma_med" % k].astype(np.float64), want["chroma_med"])


def _scipy_resize(x, rows):
    from scipy import ndimage
    x = np.array(x, dtype=np.float64)
    x[np.isnan(x)] = 0
    n, d = x.shape
    if n == 0:
        return np.zeros((rows, d))
    sigma = max(0.0, (n / float(rows) - 1.0) / 2.0)
    filt = ndimage.gaussian_filter1d(x, sigma, axis=0, mode="constant", cval=0.0, truncate=4.0) if sigma > 0 else x
    pos = (np.arange(rows) + 0.5) * (n / float(rows)) - 0.5
    coords = np.stack(np.meshgrid(pos, np.arange(d, dtype=np.float64), indexing="ij"))
    out = ndimage.map_coordinates(filt, coords, order=1, mode="grid-constant", cval=0.0)
    mn, mx = x.min(), x.max()
    zero = out == 0
    out = np.clip(out, mn, mx)
    if not (mn <= 0 <= mx):
        out[zero] = 0
    out[~np.isfinite(out)] = 0
    return out


def test_resize_against_scipy_ndimage():
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(31)
    worst = 0.0
    for n, rows in _shapes():
        for fam in ref.FAMILIES:
            x = ref.family(rng, fam, n, 3)
            if n > 4:
                x[n // 2, 1] = np.nan
            got, want = ref.resize(x, rows), _scipy_resize(x, rows)
            err = float(np.max(np.abs(got - want.astype(LD))))
            worst = max(worst, err)
            assert err <= 1e-12, (n, rows, fam, err)
            assert np.array_equal(got == 0, want == 0), (n, rows, fam)
    print("resize against scipy.ndimage: max |diff| = %.3g" % worst)


def test_oracle_resize_and_block_features_at_the_edge_shapes():
    import oracle
    rng = np.random.default_rng(32)
    worst = 0.0
    for n, rows in _shapes():
        for fam in ref.FAMILIES:
            x = ref.family(rng, fam, n, 3)
            got, want = oracle.ef_resize(x, rows), ref.resize(x, rows)
            err = float(np.max(np.abs(got.astype(LD) - want)))
            worst = max(worst, err)
            assert err <= 1e-12 and np.array_equal(got == 0, want == 0), (n, rows, fam, err)
    print("oracle.ef_resize against the reference: max |diff| = %.3g" % worst)
    # the whole chain on one-block tracks: MFCC span n_m, chroma span n_c (beats beyond the end and empty blocks included)
    for (R, C, Rc, bs, n_m, n_c, T) in ((50, 13, 40, 20, 63, 1100, 1200), (2, 13, 1, 2, 300, 40, 400), (64, 40, 40, 20, 0, 51, 60),
                                         (64, 1, 40, 20, 81, 2000, 90), (3, 40, 40, 1, 0, 39, 45), (50, 13, 40, 20, 49, 50, 50)):
        chroma = ref.family(rng, "positive", T, 12)
        mfcc = rng.standard_normal((T, C)).astype(np.float32)
        mfcc[min(T - 1, 5), 0] = np.nan
        on = np.full(bs + 1, 3, np.int64)
        on[bs - 1] = 3 + n_m if bs > 1 else 3
        on[bs] = 3 + n_c
        got = oracle.ef_block_features(chroma, mfcc, on, bs, R, Rc)
        want = ref.block_features(chroma, mfcc, on, bs, R, Rc)
        _check_f32(got, want, C, (R, C, Rc, bs, n_m, n_c))
        assert np.array_equal(np.asarray(got["chroma_med"], np.float64), want["chroma_med"])
