"""
GPU suite: ranking of finished score rows on the device (rank_kernels.hpp; acx_rank_columns / acx_topk_rows,
eval_statistics_device, getEvalStatistics(engine="device"), top_matches).  Every expectation is numpy's
(tests/_rank_ref.py, eval_statistics, the oracle), none comes from the code under test.  The failure tests hand over
invalid ARGUMENTS only; nothing here provokes a device fault.
"""
import numpy as np
import pytest

import oracle
from acoss_amd.algorithms.algorithm_template import eval_statistics, eval_statistics_device

from . import _rank_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _launches(ctx):
    return sum(v["launches"] for v in ctx.profile().values())


def _random_mates(rng, n, rows, max_mates, empty_every=0):
    moff, mates = [0], []
    for i, t in enumerate(rows):
        cnt = 0 if (empty_every and i % empty_every == 0) else int(rng.integers(1, max_mates + 1))
        cand = rng.choice(n - 1, size=min(cnt, n - 1), replace=False)
        mates += [int(c) + (1 if c >= t else 0) for c in cand]          # any column but the row's own
        moff.append(len(mates))
    return np.array(moff, np.int64), np.array(mates, np.int32)


def _check_rank(ctx, D, rows, moff, mates, posn, expect_flags=None):
    pos, flag = ctx.rank_columns(D, rows, moff, mates, posn=posn)
    want_pos, want_flag = ref.rank_columns(D, rows, moff, mates, posn)
    assert pos.dtype == np.int32 and flag.dtype == np.uint8
    assert np.array_equal(flag, want_flag)
    assert np.array_equal(pos, want_pos)
    if expect_flags is not None:
        assert np.nonzero(flag)[0].tolist() == sorted(expect_flags)
    return pos, flag


def _tied(rng, shape, levels):
    return (np.round(rng.random(shape) * levels) / levels).astype(np.float32)


@pytest.mark.parametrize("levels", [3, 8])
@pytest.mark.parametrize("use_posn", [False, True])
def test_rank_columns_with_heavy_ties(ctx, levels, use_posn):
    rng = np.random.default_rng(100 + levels + int(use_posn))
    n = 257
    D = _tied(rng, (n, n), levels)
    D[rng.random((n, n)) < 0.05] = -0.0                 # the zeros tie whatever their sign
    D[rng.random((n, n)) < 0.05] = 0.0
    D[rng.random((n, n)) < 0.02] = np.inf               # an ordinary value
    rows = np.arange(n, dtype=np.int32)
    moff, mates = _random_mates(rng, n, rows, 9, empty_every=7)          # rows with no mates at all among them
    posn = rng.permutation(n).astype(np.int32) if use_posn else None
    _check_rank(ctx, D, rows, moff, mates, posn, expect_flags=[])


@pytest.mark.parametrize("n", [2, 63, 64, 65, 4097])
def test_rank_columns_row_lengths(ctx, n):
    rng = np.random.default_rng(n)
    R = min(n, 24)
    D = _tied(rng, (R, n), 8)                           # row t = the scores of track t: its own cell is D[t, t]
    rows = np.arange(R, dtype=np.int32)
    moff, mates = _random_mates(rng, n, rows, min(n - 1, 12))
    _check_rank(ctx, D, rows, moff, mates, rng.permutation(n).astype(np.int32), expect_flags=[])
    _check_rank(ctx, D, rows, moff, mates, None, expect_flags=[])


def test_rank_columns_leading_dimension_and_scattered_rows(ctx):
    rng = np.random.default_rng(9)
    n = 130
    wide = _tied(rng, (n, n + 7), 8)
    D = wide[:, :n]                                     # rows 4 (n + 7) bytes apart: handed over as it lies, ld > n
    assert not D.flags["C_CONTIGUOUS"]
    rows = np.arange(n, dtype=np.int32)
    moff, mates = _random_mates(rng, n, rows, 5)
    _check_rank(ctx, D, rows, moff, mates, None, expect_flags=[])
    rows = rng.permutation(n)[:40].astype(np.int32)     # any order, not a run: gathered slab by slab
    moff, mates = _random_mates(rng, n, rows, 5)
    _check_rank(ctx, D, rows, moff, mates, rng.permutation(n).astype(np.int32), expect_flags=[])
    old = ctx.RANK_SLAB_BYTES
    ctx.RANK_SLAB_BYTES = 4 * n * 7                     # several slabs of 7 rows
    try:
        _check_rank(ctx, D, rows, moff, mates, None, expect_flags=[])
    finally:
        ctx.RANK_SLAB_BYTES = old


def test_rank_columns_a_clique_of_300_in_700_tracks(ctx):
    rng = np.random.default_rng(300)
    n = 700
    D = _tied(rng, (n, n), 1000)
    members = np.sort(rng.permutation(n)[:300])
    rows = members.astype(np.int32)
    mates = np.concatenate([members[members != t] for t in members]).astype(np.int32)
    moff = (np.arange(301) * 299).astype(np.int64)
    _check_rank(ctx, D, rows, moff, mates, rng.permutation(n).astype(np.int32), expect_flags=[])


def test_rank_columns_rows_beyond_the_lds(ctx):
    rng = np.random.default_rng(8)
    R, n = 8, 100000
    D = _tied(rng, (R, n), 1000)                        # ~100 cells per level
    rows = np.arange(R, dtype=np.int32)
    moff, mates = _random_mates(rng, n, rows, 13, empty_every=5)
    _check_rank(ctx, D, rows, moff, mates, rng.permutation(n).astype(np.int32), expect_flags=[])
    _check_rank(ctx, D, rows, moff, mates, None, expect_flags=[])
    D[3, 99999] = np.nan
    D[6, 0] = -np.inf
    _check_rank(ctx, D, rows, moff, mates, None, expect_flags=[3, 6])


def test_rank_columns_flags_exactly_the_planted_rows(ctx):
    rng = np.random.default_rng(77)
    n = 300
    D = _tied(rng, (n, n), 8)
    rows = np.arange(n, dtype=np.int32)
    moff, mates = _random_mates(rng, n, rows, 6)
    clean, _ = _check_rank(ctx, D, rows, moff, mates, None, expect_flags=[])
    planted = {5: np.nan, 64: -np.inf, 65: np.nan, 199: -np.inf, 299: np.nan}
    for t, v in planted.items():
        D[t, (t * 7 + 3) % n if (t * 7 + 3) % n != t else 0] = v
    D[10, 10] = np.nan                                  # a row's OWN cell may hold anything
    D[11, 11] = -np.inf
    pos, flag = _check_rank(ctx, D, rows, moff, mates, None, expect_flags=list(planted))
    for i in range(n):                                  # every other row of the same call is unaffected
        sl = slice(moff[i], moff[i + 1])
        assert np.array_equal(pos[sl], clean[sl]) if i not in planted else (pos[sl] == -1).all()


def _topk_matrix(rng, R, n, levels):
    D = _tied(rng, (R, n), levels)
    for v in (-0.0, 0.0, np.inf, -np.inf, np.nan):
        D[rng.random((R, n)) < 0.03] = v
    D[0, : n // 2] = np.nan                             # more NaN than numbers behind the k-th place
    return D


def _check_topk(ctx, D, k, rows=None, posn=None):
    idx, score = ctx.topk_rows(D, k, rows=rows, posn=posn)
    want_idx, want_score = ref.topk_rows(D, k, rows=rows, posn=posn)
    assert idx.dtype == np.int32 and score.dtype == np.float32 and idx.shape == want_idx.shape
    assert np.array_equal(idx, want_idx)
    ok = idx >= 0
    assert np.array_equal(score.view(np.uint32)[ok], want_score.view(np.uint32)[ok])      # bit copies, NaN payloads included
    assert np.isnan(score[~ok]).all()
    return idx, score


@pytest.mark.parametrize("n, ks", [(300, ["1", "10", "n-1", "n+5"]), (2500, ["1", "10", "1000"]), (20000, ["10", "1000"])])
@pytest.mark.parametrize("use_posn", [False, True])
def test_topk_rows(ctx, n, ks, use_posn):
    rng = np.random.default_rng(n + int(use_posn))
    R = 40 if n <= 2500 else 6
    D = _topk_matrix(rng, R, n, 8)
    posn = rng.permutation(n).astype(np.int32) if use_posn else None
    for kname in ks:
        k = {"n-1": n - 1, "n+5": n + 5}.get(kname) or int(kname)
        idx, _ = _check_topk(ctx, D, k, posn=posn)
        if kname == "n+5":
            assert (idx[:, n - 1:] == -1).all() and (idx[:, :n - 1] >= 0).all()
    rows = rng.permutation(R)[:5].astype(np.int32)
    _check_topk(ctx, D, 10, rows=rows, posn=posn)


def test_topk_rows_tiny(ctx):
    D = np.array([[5.0, 1.0], [2.0, 7.0]], np.float32)
    idx, score = _check_topk(ctx, D, 3)
    assert idx.tolist() == [[1, -1, -1], [0, -1, -1]] and score[:, 0].tolist() == [1.0, 2.0]
    one = np.array([[3.0]], np.float32)                  # no other column at all
    idx, score = _check_topk(ctx, one, 2)
    assert idx.tolist() == [[-1, -1]]


def test_rank_and_topk_agree(ctx):
    """The position acx_rank_columns reports for the column at place p of the top-k list is p + 1."""
    rng = np.random.default_rng(5)
    n, k = 900, 50
    D = _tied(rng, (n, n), 8)
    D[rng.random((n, n)) < 0.05] = -0.0
    D[rng.random((n, n)) < 0.02] = np.inf
    posn = rng.permutation(n).astype(np.int32)
    idx, _ = ctx.topk_rows(D, k, posn=posn)
    moff = (np.arange(n + 1) * k).astype(np.int64)
    pos, flag = ctx.rank_columns(D, None, moff, idx.reshape(-1), posn=posn)
    assert not flag.any()
    assert np.array_equal(pos.reshape(n, k), np.tile(np.arange(1, k + 1, dtype=np.int32), (n, 1)))


def _assert_stats(got, want, exact_map):
    assert (got[0], got[1], got[2]) == (want[0], want[1], want[2]), (got, want)
    assert np.array_equal(got[4], want[4])
    if exact_map:
        assert got[3] == want[3], (got[3], want[3])
    else:
        np.testing.assert_allclose(got[3], want[3], rtol=1e-12)


def _check_eval(ctx, D, cliques, topsidx):
    info = {}
    got = eval_statistics_device(D, cliques, topsidx, ctx=ctx, info=info)
    _assert_stats(got, eval_statistics(D, cliques, topsidx, count_max_clique=10 ** 9), exact_map=True)
    for other in (eval_statistics(D, cliques, topsidx), oracle.eval_statistics(D, cliques, topsidx=topsidx, stable=True)):
        np.testing.assert_allclose(np.array(got[:4]), np.array(other[:4]), rtol=1e-12)
        assert np.array_equal(got[4], other[4])
    assert info["host_rows"] == 0, "a finite matrix is ranked on the device alone"
    assert info["device_rows"] == sum(len(c) for c in cliques if len(c) >= 2)
    return got


def test_eval_statistics_device_on_the_reference_goldens(ctx, golden):
    g = golden("harness")
    cl = ref.cliques_of(g["labels"])
    for tag in ("sym", "asym"):
        res = _check_eval(ctx, g["D_" + tag], cl, (1, 2, 5))
        np.testing.assert_allclose(np.array(list(res[:4]) + list(res[4])), g["stats_" + tag], rtol=1e-12)


@pytest.fixture(scope="module")
def datacos():
    cl, n = ref.datacos_cliques(200, 13, 400, seed=13)       # 3 000 tracks in the Da-TACOS shape
    rng = np.random.default_rng(14)
    D = np.round(rng.random((n, n)), 3).astype(np.float32)   # three decimals: ties in every row
    member = np.zeros((n, n), bool)
    for c in cl:
        member[np.ix_(c, c)] = True
    D[member] = np.round(np.minimum(1.0, D[member] + 0.25), 3)      # covers score higher, not always
    return D, cl


def test_eval_statistics_device_datacos_shape(ctx, datacos):
    D, cl = datacos
    _check_eval(ctx, D, cl, (1, 10, 100, 1000))


def test_eval_statistics_device_planted_rows(ctx, datacos):
    D, cl = datacos
    D = D.copy()
    n = D.shape[0]
    evaluated = [t for c in cl if len(c) >= 2 for t in c]
    planted = evaluated[::97]
    for k, t in enumerate(planted):
        D[t, (t + 11) % n] = [np.nan, -np.inf][k % 2]
    info = {}
    got = eval_statistics_device(D, cl, (1, 10, 100, 1000), ctx=ctx, info=info)
    assert info["host_rows"] == len(planted) and info["device_rows"] == len(evaluated) - len(planted)
    _assert_stats(got, eval_statistics(D, cl, (1, 10, 100, 1000), count_max_clique=0), exact_map=False)


def test_eval_statistics_device_other_layouts(ctx, datacos):
    """A float64 matrix and a non-contiguous view give what their float32 copy gives."""
    D, cl = datacos
    want = eval_statistics_device(D, cl, (1, 10, 100), ctx=ctx)
    info = {}
    got = eval_statistics_device(D.astype(np.float64), cl, (1, 10, 100), ctx=ctx, info=info)
    _assert_stats(got, want, exact_map=True)
    assert info["host_rows"] == 0
    n = D.shape[0]
    big = np.zeros((2 * n, 2 * n), np.float32)
    big[::2, ::2] = D
    view = big[::2, ::2]
    assert view.strides == (16 * n, 8)
    _assert_stats(eval_statistics_device(view, cl, (1, 10, 100), ctx=ctx), want, exact_map=True)
    F = np.asfortranarray(D)
    _assert_stats(eval_statistics_device(F, cl, (1, 10, 100), ctx=ctx), want, exact_map=True)
    idx, score = ctx.topk_rows(view, 7)
    idx32, score32 = ctx.topk_rows(D, 7)
    assert np.array_equal(idx, idx32) and np.array_equal(score, score32)


def test_ftm2d_end_to_end(tmp_path, monkeypatch):
    from acoss_amd import synth
    from acoss_amd.algorithms import FTM2D
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
    algo.all_pairwise(symmetric=True)
    host = algo.getEvalStatistics("main")
    dev = algo.getEvalStatistics("main", engine="device")
    assert dev[:4] == host[:4] and np.array_equal(dev[4], host[4])
    rows = open("results_synth_FTM2D.csv").read().splitlines()
    assert len(rows) == 3 and rows[1] == rows[2]
    D = np.array(algo.Ds["main"])
    n = len(labels)
    idx, score = algo.top_matches("main", k=3)
    assert idx.shape == (n, 3) and score.shape == (n, 3)
    hits = 0
    for t in range(n):
        cols = np.array([c for c in range(n) if c != t])
        best = cols[np.argsort(-D[t, cols], kind="stable")[:3]]
        assert idx[t].tolist() == best.tolist()
        assert np.array_equal(score[t], D[t, best])
        hits += labels[best[0]] == labels[t]
        assert (labels[idx[t, 0]] == labels[t]) == (labels[best[0]] == labels[t])
    assert hits > n // 2                               # (chance is ~ 3 / 47)
    some = algo.top_matches("main", k=2, rows=[5, 2])
    assert np.array_equal(some[0], idx[[5, 2], :2])


# ---------------------------------------------------------------- failure paths: invalid arguments only
def test_invalid_arguments_launch_nothing(ctx):
    rng = np.random.default_rng(2)
    n = 50
    D = _tied(rng, (n, n), 8)
    rows = np.arange(n, dtype=np.int32)
    moff, mates = _random_mates(rng, n, rows, 4)
    want = ref.rank_columns(D, rows, moff, mates)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        bad = mates.copy()
        bad[17] = n
        with pytest.raises(ValueError, match=r"mates\[17\]"):
            ctx.rank_columns(D, rows, moff, bad)
        bad[17] = -1
        with pytest.raises(ValueError, match=r"mates\[17\]"):
            ctx.rank_columns(D, rows, moff, bad)
        bad = mates.copy()
        r = int(np.searchsorted(moff, 30, side="right") - 1)
        bad[30] = rows[r]
        with pytest.raises(ValueError, match=r"mates\[30\].*own column"):
            ctx.rank_columns(D, rows, moff, bad)
        posn = np.arange(n, dtype=np.int32)
        posn[3] = -2
        with pytest.raises(ValueError, match=r"posn\[3\]"):
            ctx.rank_columns(D, rows, moff, mates, posn=posn)
        with pytest.raises(ValueError, match=r"posn\[3\]"):
            ctx.topk_rows(D, 5, posn=posn)
        with pytest.raises(ValueError, match="rows"):
            ctx.topk_rows(D, 5, rows=[0, n])
        with pytest.raises(ValueError, match=r"self\[1\]"):          # a row whose track is no column of the slab
            ctx.topk_rows(D[:, :20], 5, rows=[0, 30])
        with pytest.raises(NotImplementedError, match="k = 1025 is over the limit"):
            ctx.topk_rows(D, 1025)
        with pytest.raises(ValueError, match="k must be"):
            ctx.topk_rows(D, 0)
        assert _launches(ctx) == 0, "the arguments are validated before the first launch"
        # the context stays usable, and the profile sees the two kernel families
        pos, flag = ctx.rank_columns(D, rows, moff, mates)
        assert np.array_equal(pos, want[0]) and np.array_equal(flag, want[1])
        idx, _ = ctx.topk_rows(D, 5)
        assert np.array_equal(idx, ref.topk_rows(D, 5)[0])
        prof = ctx.profile()
        assert prof["rank_columns_kernel"]["launches"] == 1 and prof["topk_rows_kernel"]["launches"] == 1
        assert prof["rank_columns_kernel"]["cells"] == n * n
    finally:
        ctx.profile_enable(False)


def test_scratch_limit_bounds_the_staging(ctx):
    rng = np.random.default_rng(3)
    n = 600
    D = _tied(rng, (n, n), 8)
    rows = np.arange(n, dtype=np.int32)
    moff, mates = _random_mates(rng, n, rows, 4)
    want = ref.rank_columns(D, rows, moff, mates)
    ctx.set_scratch_limit(256 << 10)                    # ~ 50 rows per piece: a dozen pieces through the two slots
    try:
        pos, flag = ctx.rank_columns(D, rows, moff, mates)
        assert np.array_equal(pos, want[0]) and not flag.any()
        idx, _ = ctx.topk_rows(D, 9)
        assert np.array_equal(idx, ref.topk_rows(D, 9)[0])
        ctx.set_scratch_limit(4 << 10)                  # not even two rows
        with pytest.raises(MemoryError, match="scratch limit"):
            ctx.rank_columns(D, rows, moff, mates)
        with pytest.raises(MemoryError, match="scratch limit"):
            ctx.topk_rows(D, 9)
    finally:
        ctx.set_scratch_limit(0)
    pos, _ = ctx.rank_columns(D, rows, moff, mates)
    assert np.array_equal(pos, want[0])
