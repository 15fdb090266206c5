"""
GPU tests of the EarlyFusion block-feature kernels stage by stage (run with -m gpu): ef_blocks_kernel,
ef_chroma_median_kernel and ef_rownorm_kernel (acoss_amd/csrc/ef_prep_kernels.hpp) per value against the independent
longdouble reference tests/_efprep_ref.py (the resize as clip(L @ G @ x); pinned to scikit-image's goldens, to scipy.ndimage
and to the oracle by tests/test_efprep_ref.py), at the block lengths, geometries and data where a resize, a median or a
multi-track launch can go wrong.

Bounds -- derived, none tuned to the device:
  mfccs, chromas   both sides work in f64 or better and round once to f32: |got - want| <= ulp32(want) / 2 + 1e-12 with
                   `want` the unrounded longdouble value, ulp32 taken at max(|want|, 2^-126); 1e-12 is the allowance for
                   another f64 summation order (test_efprep_ref.py measures 8.4e-14 between two formulations).  Where want is
                   exactly 0, got is exactly 0.
  ssms             the device takes the Gram form |x_r|^2 + |x_c|^2 - 2 x_r.x_c on unit rows, clamped at 0; its f64 rounding
                   error in d^2 is at most e = 4 (2 ncoef + 4) 2^-53:
                   |got - want| <= ulp32(want) / 2 + min(sqrt(e), e / (2 want)) + 1e-12
  medians, block offsets, a track alone against the same track in a pool: bit-identical
  downloaded unit-norm chroma rows   2 ulp32(want): one rounding of the norm to f32 and one f32 division
  squared norms    1 f32 ulp of the f64 value
No cell is left out, but for the two rows of a one-frame MFCC block at 50 rows that are mathematically 0 (see
test_mfcc_chain_at_the_edge_lengths): rounding noise scaled to unit length has no value to compare.
"""
import numpy as np
import pytest

from tests import _efprep_ref as ref

pytestmark = pytest.mark.gpu
LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _one_block(blocksize, n_m, n_c, start=3):
    """blocksize + 1 beats, i.e. ONE block: MFCC frames [start, start + n_m), chroma frames [start, start + n_c).
    (blocksize 1: the MFCC block is x[on[b]:on[b]], always empty.)"""
    on = np.full(blocksize + 1, start, np.int64)
    if blocksize > 1:
        on[blocksize - 1] = start + n_m
    on[blocksize] = start + n_c
    return on


def _check(got, want, ncoef, what, noise_rows=()):
    """Every value of one track's block features against the unrounded reference; returns the largest error / bound.
    `noise_rows`: the (block, row) the caller EXPECTS to be mathematically 0 yet not exactly (ref.mfcc_chain): their unit
    rows are scaled rounding noise on both sides.  They must be exactly those the reference finds; of them only this is
    asserted: the row is finite and of length 1 (or 0), and so are the distances to it finite and at most 2."""
    assert sorted(want["noise_rows"]) == sorted(noise_rows), (what, want["noise_rows"])
    R = want["mfccs"].shape[1] // ncoef
    keep_m = np.ones(want["mfccs"].shape, bool).reshape(-1, R, ncoef)
    keep_s = np.ones((len(keep_m), R, R), bool)
    for b, r in noise_rows:
        keep_m[b, r], keep_s[b, r, :], keep_s[b, :, r] = False, False, False
        row = got["mfccs"].reshape(-1, R, ncoef)[b, r].astype(np.float64)
        assert np.all(np.isfinite(row)) and (not row.any() or abs(np.sqrt((row * row).sum()) - 1) < 1e-6), (what, b, r)
    keep = dict(mfccs=keep_m.reshape(want["mfccs"].shape), chromas=np.ones(want["chromas"].shape, bool),
                ssms=keep_s[:, np.tril_indices(R, -1)[0], np.tril_indices(R, -1)[1]])
    assert np.all(np.isfinite(got["ssms"])) and np.all(got["ssms"] >= 0) and np.all(got["ssms"] <= 2.0 + 1e-6), what
    worst = {}
    for key in ("mfccs", "chromas"):
        assert got[key].shape == want[key].shape and got[key].dtype == np.float32, (what, key)
        err, bound = np.abs(got[key].astype(LD) - want[key])[keep[key]], ref.bound_rounded(want[key])[keep[key]]
        worst[key] = float(np.max(err / bound, initial=0))
        assert np.all(err <= bound), (what, key, worst[key], float(np.max(err)))
        assert not got[key][keep[key] & (want[key] == 0)].any(), (what, key, "a value that is exactly 0 came back non-zero")
    assert got["ssms"].shape == want["ssms"].shape and got["ssms"].dtype == np.float32, what
    err = np.abs(got["ssms"].astype(LD) - want["ssms"])[keep["ssms"]]
    bound = ref.bound_ssm(want["ssms"], ncoef)[keep["ssms"]]
    worst["ssms"] = float(np.max(err / bound, initial=0))
    assert np.all(err <= bound), (what, "ssms", worst["ssms"], float(np.max(err)))
    np.testing.assert_array_equal(got["chroma_med"], want["chroma_med"], err_msg=str(what))
    return worst


def _raises_wide(ctx, chroma, mfcc, on, geo, which):
    with pytest.raises(NotImplementedError, match=r"block 0 of track 0 spans \d+ frames of %s.*radius \d+, at most 512" % which):
        ctx.ef_block_features(chroma, mfcc, on, *geo)


# ---- a. the resize at its edges, through the chroma output ----

@pytest.mark.parametrize("family", ref.FAMILIES)
@pytest.mark.parametrize("rows", [40, 1])
def test_resize_edges_through_the_chroma_block(ctx, rows, family):
    """Block lengths 0, 1, 2, rows - 1, rows, rows + 1, the first with a Gaussian and the one before, 257 rows (r = 512, the
    widest the device holds) and 1100 frames; a length whose radius passes 512 (1100 frames to one row) must be refused."""
    rng = np.random.default_rng(100 + rows)
    worst = 0.0
    for n in ref.edge_lengths(rows):
        chroma = ref.family(rng, family, n + 9, 12)
        mfcc = np.zeros((4, 13), np.float32)
        on = _one_block(20, 0, n)
        geo = (20, 50, rows)
        if ref.radius(n, rows)[1] > ref.MAXRAD:
            _raises_wide(ctx, chroma, mfcc, on, geo, "chroma")
            continue
        got = ctx.ef_block_features(chroma, mfcc, on, *geo)
        w = _check(got, ref.block_features(chroma, mfcc, on, *geo), 13, (rows, family, n))
        worst = max(worst, w["chromas"])
    print("chroma rows=%d %s: max err / bound = %.3f" % (rows, family, worst))


# ---- b. the MFCC chain ----

@pytest.mark.parametrize("blocksize", [20, 1, 2])
@pytest.mark.parametrize("R,C", [(50, 13), (2, 13), (64, 40), (64, 1), (3, 40)])
def test_mfcc_chain_at_the_edge_lengths(ctx, R, C, blocksize):
    rng = np.random.default_rng(200 + R + C)
    worst = dict(mfccs=0.0, ssms=0.0, chromas=0.0)
    for n in ref.edge_lengths(R) if blocksize > 1 else [7]:          # (blocksize 1: every MFCC block is empty)
        mfcc = rng.standard_normal((n + 9, C)).astype(np.float32)
        chroma = ref.family(rng, "positive", 50, 12)
        on = _one_block(blocksize, n, 37)
        geo = (blocksize, R, 40)
        if ref.radius(n, R)[1] > ref.MAXRAD:
            _raises_wide(ctx, chroma, mfcc, on, geo, "MFCCs")
            continue
        got = ctx.ef_block_features(chroma, mfcc, on, *geo)
        # A one-frame block resizes to MULTIPLES of that frame, weight 1 - |(o + 0.5) / R - 0.5| in row o, and the row whose
        # weight equals the mean weight 0.75 -- (o + 0.5) / R = 1 / 4 or 3 / 4: rows 12 and 37 of 50, none of 64 or 3 -- is
        # mathematically 0 after the mean: rounding noise that both sides scale to unit length, as with an inexact constant
        # block.  Those two rows are the ONLY values in this file that are not compared.  (2 rows: both have weight 0.75
        # exactly, so they are exactly 0 and are compared.)
        noise = [(0, 12), (0, 37)] if (n, R) == (1, 50) else []
        w = _check(got, ref.block_features(chroma, mfcc, on, *geo), C, (R, C, blocksize, n), noise)
        if blocksize == 1 or n == 0:
            assert not got["mfccs"].any() and not got["ssms"].any()
        worst = {k: max(worst[k], w[k]) for k in worst}
    print("mfcc chain R=%d C=%d blocksize=%d: max err / bound = %s" % (R, C, blocksize, worst))


def test_mfcc_chain_nan_samples(ctx):
    """A NaN sample counts as 0: inside an ordinary block, and inside a block that is otherwise all-positive, whose range
    then includes 0 (the fill value no longer lies outside it: the rows blended with the zeros outside are clipped)."""
    rng = np.random.default_rng(210)
    for n in (31, 49, 63, 400):
        for positive in (False, True):
            mfcc = rng.standard_normal((n + 9, 13)).astype(np.float32)
            if positive:
                mfcc = np.abs(mfcc) + np.float32(0.25)
            mfcc[3 + n // 2, 4] = np.nan
            chroma = ref.family(rng, "positive", n + 20, 12)
            on = _one_block(20, n, n + 11)
            got = ctx.ef_block_features(chroma, mfcc, on)
            _check(got, ref.block_features(chroma, mfcc, on), 13, ("nan", n, positive))


@pytest.mark.parametrize("value", [0.0, 0.5])
def test_mfcc_chain_constant_blocks_are_exact_zeros(ctx, value):
    """A constant block of 0 or 0.5: the clip to the block's range makes every resized value that constant, the column means
    are exact, and mfccs and ssms are exactly 0.  (A constant that is no dyadic fraction, 0.1 say, is NOT asserted: the mean
    subtraction leaves rounding noise there, which both sides then scale to unit length -- noise against noise.)"""
    rng = np.random.default_rng(220)
    for n in (1, 49, 50, 51, 63, 300):
        mfcc = np.full((n + 9, 13), value, np.float32)
        chroma = ref.family(rng, "positive", n + 20, 12)
        on = _one_block(20, n, n + 5)
        got = ctx.ef_block_features(chroma, mfcc, on)
        assert not got["mfccs"].any() and not got["ssms"].any(), (value, n)
        _check(got, ref.block_features(chroma, mfcc, on), 13, ("constant", value, n))


def test_feature_arrays_of_different_length_and_beats_at_and_beyond_the_end(ctx):
    rng = np.random.default_rng(230)
    # chroma longer than the MFCCs and the other way round: each slice clips at its own array's end
    for Tc, Tm in ((300, 180), (170, 320)):
        chroma = ref.family(rng, "positive", Tc, 12)
        mfcc = rng.standard_normal((Tm, 13)).astype(np.float32)
        on = np.sort(rng.choice(330, 24, replace=False)).astype(np.int64)
        got = ctx.ef_block_features(chroma, mfcc, on)
        _check(got, ref.block_features(chroma, mfcc, on), 13, ("lengths", Tc, Tm))
    # beats equal to each other, equal to T, beyond T, and descending (numpy: an empty slice); blocksize 3 keeps it readable
    T = 200
    chroma = ref.family(rng, "positive", T, 12)
    mfcc = rng.standard_normal((T, 13)).astype(np.float32)
    on = np.array([5, 40, 40, 90, 60, 200, 260, 100, 30, 200, 199, 200, 201], np.int64)
    got = ctx.ef_block_features(chroma, mfcc, on, 3, 50, 40)
    want = ref.block_features(chroma, mfcc, on, 3, 50, 40)
    _check(got, want, 13, "beats")
    empty_m = [b for b in range(10) if min(on[b + 2], T) <= min(on[b], T)]
    assert empty_m == [5, 6, 9] and not got["mfccs"][empty_m].any() and not got["ssms"][empty_m].any()
    empty_c = [b for b in range(10) if min(on[b + 3], T) <= min(on[b], T)]
    assert empty_c == [5, 6, 9] and not got["chromas"][empty_c].any()


# ---- c. the medians ----

MEDIAN_T = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 1000, 1001)


def _median_data(rng, name, T):
    if name == "distinct":
        return rng.random((T, 12)).astype(np.float32)
    if name == "quarters":                       # many ties at the middle
        return (np.round(rng.random((T, 12)) * 4) / 4).astype(np.float32)
    if name == "binary":                         # real HPCP is full of exact 0 and 1
        return rng.integers(0, 2, (T, 12)).astype(np.float32)
    if name == "signed_zeros":
        return rng.choice(np.array([-1.0, -0.25, -0.0, 0.0, 0.25, 1.0], np.float32), (T, 12))
    if name == "denormals":
        return (rng.integers(-200, 200, (T, 12)).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    assert name == "last_bit"                    # the two middle values differ in the last bit: their f32 mean rounds
    x = np.empty((T, 12), np.float32)
    for col in range(12):
        lo = np.nextafter(np.float32(1 + col / 16.0), np.float32(4), dtype=np.float32) if col % 2 else np.float32(1 + col / 16.0)
        hi = np.nextafter(lo, np.float32(4), dtype=np.float32)
        v = np.concatenate([np.full((T - 1) // 2, 0.5, np.float32), [lo], [hi] if T > 1 else [], np.full(max(0, T - 2 - (T - 1) // 2), 3.0, np.float32)])
        x[:, col] = rng.permutation(v[:T])
    return x


@pytest.mark.parametrize("name", ["distinct", "quarters", "binary", "signed_zeros", "denormals", "last_bit"])
def test_chroma_medians_equal_numpy(ctx, name):
    rng = np.random.default_rng(300)
    for T in MEDIAN_T:
        chroma = _median_data(rng, name, T)
        got = ctx.ef_block_features(chroma, np.zeros((4, 13), np.float32), np.zeros(1, np.int64))["chroma_med"]
        want = np.median(chroma, axis=0)
        assert want.dtype == np.float32
        if name == "signed_zeros":               # the sign of a zero median is not asserted
            assert np.array_equal(got, want.astype(np.float64)), (name, T)
        else:
            assert got.tobytes() == want.astype(np.float64).tobytes(), (name, T, got, want)
    if name == "last_bit":                       # the family does what it is there for: the f64 mean differs from the f32 one
        c = _median_data(rng, name, 64)
        s = np.sort(c.astype(np.float64), axis=0)
        assert np.any((s[31] + s[32]) / 2 != np.median(c, axis=0).astype(np.float64))


# ---- d. the multi-track launch and the pool ----

def _pool_tracks(rng):
    """12 short tracks: the first, the last and two in the middle have no block (fewer beats than blocksize + 1), one has no
    frame of features at all (its blocks are empty: all-zero rows), one has a single block."""
    T = [120, 200, 250, 300, 180, 0, 260, 240, 170, 400, 220, 130]
    beats = [7, 24, 23, 26, 21, 23, 20, 0, 25, 24, 22, 12]
    tracks = []
    for t, nb in zip(T, beats):
        on = np.sort(rng.choice(max(t, 30) + 15, nb, replace=False)).astype(np.int64)
        tracks.append(dict(chroma=ref.family(rng, "positive", t, 12), mfcc=rng.standard_normal((t, 13)).astype(np.float32), onsets=on))
    return tracks


def test_pool_of_many_tracks_equals_every_track_alone(ctx):
    """ef_upload_raw_pool (one launch over all blocks: blockIdx.x bisected over the block offsets) unsliced, and under a
    scratch limit of 500 frames that puts the slices {0 1} {2} {3 4 5} {6 7} {8} {9} {10 11} -- boundaries beside the tracks
    without blocks, one slice without any block --: for every track, mfccs, ssms and the median bit-identical to
    ef_block_features of the track alone; the pool's chroma rows and squared norms against the reference."""
    rng = np.random.default_rng(400)
    tracks = _pool_tracks(rng)
    alone = [ctx.ef_block_features(t["chroma"], t["mfcc"], t["onsets"]) for t in tracks]
    nblocks = [max(0, len(t["onsets"]) - 20) for t in tracks]
    assert nblocks == [0, 4, 3, 6, 1, 3, 0, 0, 5, 4, 2, 0]
    for t, a in zip(tracks, alone):              # (checked against the reference as well: the pool inherits it)
        _check(a, ref.block_features(t["chroma"], t["mfcc"], t["onsets"]), 13, "alone")
    assert not alone[5]["chromas"].any() and np.all(np.isnan(alone[5]["chroma_med"]))
    for limit in (0, 100 * 500):
        try:
            ctx.set_scratch_limit(limit)
            boff = ctx.ef_upload_raw_pool(tracks)
        finally:
            ctx.set_scratch_limit(0)
        pool = ctx.ef_download_pool()
        assert np.array_equal(boff, np.concatenate([[0], np.cumsum(nblocks)])) and np.array_equal(pool["offsets"], boff)
        for k, a in enumerate(alone):
            rows = slice(boff[k], boff[k + 1])
            assert pool["mfccs"][rows].tobytes() == a["mfccs"].tobytes(), (limit, k)
            assert pool["ssms"][rows].tobytes() == a["ssms"].tobytes(), (limit, k)
            assert pool["chroma_med"][k].tobytes() == a["chroma_med"].tobytes(), (limit, k)
        _check_pool_rows(pool, {key: np.concatenate([a[key] for a in alone]) for key in ("mfccs", "ssms", "chromas")})
        zero = slice(boff[5], boff[6])           # the rows of the track without frames: norm 0 -> 1, the row stays 0
        assert not pool["chromas"][zero].any() and not pool["mfcc_sq"][zero].any() and not pool["ssm_sq"][zero].any()


def _check_pool_rows(pool, feats):
    """ef_rownorm_kernel: the pool's unit-norm chroma rows and squared norms from the f32 block features it was given."""
    unit, msq, ssq = ref.pool_rows(feats)
    err = np.abs(pool["chromas"].astype(LD) - unit)
    assert np.all(err <= 2 * ref.ulp32(unit)), float(np.max(err / ref.ulp32(unit)))
    assert not pool["chromas"][unit == 0].any()
    for got, want in ((pool["mfcc_sq"], msq), (pool["ssm_sq"], ssq)):
        w64 = want.astype(np.float64)            # "1 f32 ulp of the f64 value"
        assert np.all(np.abs(got.astype(LD) - w64) <= ref.ulp32(w64)), float(np.max(np.abs(got.astype(LD) - w64) / ref.ulp32(w64)))


@pytest.mark.parametrize("nb", [1, 3, 4, 5])
def test_rownorm_at_block_counts_around_four(ctx, nb):
    """ef_rownorm_kernel works on four rows per workgroup: pools of 1, 3, 4 and 5 blocks, one of them an all-zero row."""
    rng = np.random.default_rng(410 + nb)
    T = 260
    on = np.sort(rng.choice(T - 30, 20 + nb, replace=False)).astype(np.int64)
    on[-1] = on[nb - 1]                          # the last block's chroma slice is empty: a row of zeros
    t = dict(chroma=ref.family(rng, "positive", T, 12), mfcc=rng.standard_normal((T, 13)).astype(np.float32), onsets=on)
    a = ctx.ef_block_features(t["chroma"], t["mfcc"], t["onsets"])
    assert len(a["chromas"]) == nb and not a["chromas"][-1].any() and (nb == 1 or a["chromas"][0].any())
    boff = ctx.ef_upload_raw_pool([t])
    pool = ctx.ef_download_pool()
    assert list(boff) == [0, nb] and pool["mfccs"].tobytes() == a["mfccs"].tobytes() and pool["ssms"].tobytes() == a["ssms"].tobytes()
    _check_pool_rows(pool, a)
    assert not pool["chromas"][-1].any()
    # the same pool handed in ready goes through the same kernel
    ctx.ef_upload_pool([a])
    again = ctx.ef_download_pool()
    for key in ("mfccs", "ssms", "chromas", "mfcc_sq", "ssm_sq", "chroma_med", "offsets"):
        assert again[key].tobytes() == pool[key].tobytes(), key


# ---- e. the failure paths ----

def test_download_needs_a_finished_pool():
    from acoss_amd import _lib
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.AcxError, match="ef_download_pool: no finished block-feature pool"):
            c.ef_download_pool()
        c.ef_pool_begin([2, 3])
        with pytest.raises(_lib.AcxError, match="ef_download_pool: no finished block-feature pool"):
            c.ef_download_pool()
    finally:
        c.close()


def test_wide_blocks_and_negative_onsets_are_refused_and_leave_the_pool_alone(ctx):
    """A block whose Gaussian would need a radius above 512 (it used to be filtered with a clamped, renormalised kernel, off by
    up to 3.4e-2) is NotImplementedError naming track, block and limit; a negative onset (it used to be clamped to 0 where numpy
    counts from the end) is ValueError naming the track -- both before anything is allocated: the pool that is up gives the
    same bits afterwards."""
    import oracle
    rng = np.random.default_rng(500)

    def track(T, nbeats):
        on = np.sort(rng.choice(T - 10, nbeats, replace=False)).astype(np.int64)
        return dict(chroma=ref.family(rng, "positive", T, 12), mfcc=rng.standard_normal((T, 13)).astype(np.float32), onsets=on)
    tracks = [track(1500, 60), track(1800, 66), track(1300, 55)]
    pairs = oracle.all_pairs(3, True).astype(np.int32)
    ctx.ef_upload_raw_pool(tracks)
    before, scores = ctx.ef_download_pool(), ctx.earlyfusion_pairs(pairs)

    # 10290 frames to 40 rows is the first length with r = 513 there; 258 frames to one row have r = 514; (1100, 2): r = 1098
    assert ref.radius(10289, 40)[1] == 512 and ref.radius(10290, 40)[1] == 513
    wide = track(10400, 21)
    wide["onsets"] = _one_block(20, 50, 10290, start=7)
    with pytest.raises(NotImplementedError, match=r"block 0 of track 1 spans 10290 frames of chroma: its resize to 40 rows needs a Gaussian of radius 513, at most 512"):
        ctx.ef_upload_raw_pool([tracks[0], wide, tracks[1]])
    with pytest.raises(NotImplementedError, match=r"block 0 of track 0 spans 10290 frames of chroma"):
        ctx.ef_block_features(wide["chroma"], wide["mfcc"], wide["onsets"])
    with pytest.raises(NotImplementedError, match=r"spans 258 frames of chroma: its resize to 1 rows needs a Gaussian of radius 514"):
        ctx.ef_block_features(wide["chroma"], wide["mfcc"], _one_block(20, 50, 258), 20, 50, 1)
    with pytest.raises(NotImplementedError, match=r"block 0 of track 0 spans 1100 frames of MFCCs: its resize to 2 rows needs a Gaussian of radius 1098"):
        ctx.ef_block_features(wide["chroma"], wide["mfcc"], _one_block(20, 1100, 40), 20, 2, 40)
    # one frame fewer is the widest the device holds, and right
    ok = _one_block(20, 50, 10289, start=7)
    _check(ctx.ef_block_features(wide["chroma"], wide["mfcc"], ok), ref.block_features(wide["chroma"], wide["mfcc"], ok), 13, "r = 512")

    neg = dict(tracks[2], onsets=tracks[2]["onsets"].copy())
    neg["onsets"][0] = -1
    with pytest.raises(ValueError, match=r"ef_upload_raw_pool: track 2 has a negative onset \(-1\)"):
        ctx.ef_upload_raw_pool([tracks[0], tracks[1], neg])
    with pytest.raises(ValueError, match=r"ef_block_features: track 0 has a negative onset \(-1\)"):
        ctx.ef_block_features(neg["chroma"], neg["mfcc"], neg["onsets"])

    after = ctx.ef_download_pool()
    for key in before:
        assert after[key].tobytes() == before[key].tobytes(), key
    assert ctx.earlyfusion_pairs(pairs).tobytes() == scores.tobytes()
