"""
GPU tests (run with -m gpu on a real MI355X): WHERE the Qmax alignment lies -- qmax_locate_kernel<EQG>
(acoss_amd/csrc/serra09_locate_kernels.hpp) through acx_qmax_locate_binary (the DP alone on a given plot) and acx_serra09_align (the
product chain), Serra09.align and Serra09.align_matches.

Every comparison is exact: all five fields (score, q0, r0, q1, r1) against the forward restatement of the contract
(tests/_qmax_locate_ref.py locate_forward; tests/test_qmax_locate_ref.py holds it against an independent traceback and the CPU
oracle), and the score also against the score sweep on the same plot (acx_qmax_binary / acx_serra09_pairs), bit for bit.

The kernel gives a lane C = 32 columns, a wave a strip of 64 C = 2048; the shapes below sit on both sides of a lane, of a
strip and of two and three strips.
"""
import numpy as np
import pytest

from tests import _qmax_locate_ref as ref
from tests import _serra09_shapes as S

pytestmark = pytest.mark.gpu

C = 32                         # columns per lane (LOC_CPL)
STRIP = 64 * C
SETTINGS = [(go, ge, st) for st in (2, 3) for go, ge in ((0.5, 0.5), (1.0, 0.25), (0.25, 1.0))]
FIELDS = ("score", "q0", "r0", "q1", "r1")


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _rec(a):
    """One acx_alignment record as the reference's tuple."""
    return (float(a["score"]),) + tuple(int(a[f]) for f in FIELDS[1:])


def _bits(x):
    return np.float32(x).view(np.uint32)


def _check_dp(ctx, R, setting, tag):
    """qmax_locate_binary on R against the reference, its score against qmax_binary; returns the record."""
    from acoss_amd import _lib
    go, ge, st = setting
    p = _lib.serra09_params(gamma_o=go, gamma_e=ge, dp_start=st)
    got = ctx.qmax_locate_binary(R, p)
    assert got.shape == (1,) and got.dtype == _lib.ALIGNMENT_DTYPE
    want = ref.locate_forward(R, go, ge, st)
    assert _rec(got[0]) == want, "%s, %s plot, gammas (%s, %s), dp_start %d: device %s, reference %s" % (
        tag, R.shape, go, ge, st, _rec(got[0]), want)
    assert _bits(got[0]["score"]) == _bits(ctx.qmax_binary(R, p)), (tag, setting)
    return want


def _diag(R, end, length, step=(1, 1)):
    """Ones on `length` cells ending in `end`, `step` apart."""
    for t in range(length):
        R[end[0] - t * step[0], end[1] - t * step[1]] = 1


# ---- the DP alone ---------------------------------------------------------------------------------------------------------------------------
def test_hand_checked_plots(ctx):
    assert _check_dp(ctx, np.eye(8, dtype=np.uint8), (0.5, 0.5, 2), "eye(8)") == (6.0, 2, 2, 7, 7)
    R = np.eye(10, dtype=np.uint8)
    R[5, 5] = 0
    assert _check_dp(ctx, R, (0.5, 0.5, 2), "one gap") == (6.5, 2, 2, 9, 9)
    R = np.eye(12, dtype=np.uint8)
    R[5, 5] = R[6, 6] = 0
    assert _check_dp(ctx, R, (0.5, 0.5, 2), "two gaps") == (7.5, 2, 2, 11, 11)
    assert _check_dp(ctx, R, (1.0, 0.25, 2), "two gaps") == (7.0, 2, 2, 11, 11)
    R = np.zeros((40, 40), np.uint8)
    _diag(R, (5, 5), 4)
    _diag(R, (28, 33), 4)
    assert _check_dp(ctx, R, (0.5, 0.5, 2), "two equal diagonals") == (4.0, 2, 2, 5, 5)
    R = np.zeros((9, 9), np.uint8)
    for c in ((4, 4), (5, 5), (3, 4), (4, 5), (6, 6)):
        R[c] = 1
    assert _check_dp(ctx, R, (0.5, 0.5, 2), "c2 and c3 tie") == (3.0, 4, 4, 6, 6)
    for setting in SETTINGS:
        assert _check_dp(ctx, np.zeros((7, 9), np.uint8), setting, "all zero") == ref.NO_MATCH
        for shape in ((2, 5), (5, 2), (1, 1), (2, 2)):
            assert _check_dp(ctx, np.ones(shape, np.uint8), setting, "smaller than 3 x 3") == ref.NO_MATCH


@pytest.mark.parametrize("N", [1, 2, 3, C - 1, C, C + 1, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 1, 3 * STRIP + 5])
def test_random_plots(ctx, N):
    """Both sides of a lane's columns, of one strip, two and three strips, with one to 64 rows; every penalty setting and dp_start."""
    rng = np.random.default_rng(N)
    for M in (1, 2, 3, 4, 5, 9, 64):
        R = (rng.random((M, N)) < rng.choice([0.05, 0.3, 0.6])).astype(np.uint8)
        for setting in SETTINGS:
            _check_dp(ctx, R, setting, "random plot")


def _random_path(rng, R, i, j):
    """Ones along a path from (i, j) that takes (1, 1), (1, 2) and (2, 1) steps, to the plot's edge; returns its cells."""
    steps = ((1, 2), (1, 2), (1, 1), (2, 1))
    cells = 0
    while i < R.shape[0] and j < R.shape[1]:
        R[i, j] = 1
        cells += 1
        di, dj = steps[int(rng.integers(0, 4))]
        i, j = i + di, j + dj
    return cells


def test_paths_across_every_lane_edge_and_both_seams(ctx):
    """Planted paths of (1, 1), (1, 2) and (2, 1) steps in sparse noise -- the start travels through the DPP neighbour values and the seam
    records: one from column 3 across every lane edge of the first strip's wave and on into the second strip; two short ones across the
    seams at 2048 and 4096."""
    rng = np.random.default_rng(7)
    R = (rng.random((1800, STRIP + 60)) < 0.01).astype(np.uint8)
    cells = _random_path(rng, R, 5, 3)
    assert cells > 1300 and R[:, STRIP:].sum(axis=0).min() > 0, "the path reaches the plot's right edge, behind the seam"
    for setting in ((0.5, 0.5, 2), (1.0, 0.25, 3)):
        rec = _check_dp(ctx, R, setting, "a path across every lane edge")
        assert rec[0] >= cells - 2 and rec[1] <= 6 and rec[2] <= 5 and rec[4] >= STRIP, (cells, rec)
    R = (rng.random((150, 2 * STRIP + 120)) < 0.01).astype(np.uint8)
    _random_path(rng, R, 2, STRIP - 70)
    _random_path(rng, R, 20, 2 * STRIP - 60)
    for setting in SETTINGS:
        rec = _check_dp(ctx, R, setting, "paths across the seams")
        assert rec[0] > 90 and (rec[2] < STRIP <= rec[4] or rec[2] < 2 * STRIP <= rec[4]), rec


def _two_diagonals(M, N, ra, ca, di, dj):
    """Ones on the diagonal that ends in (ra, ca) and on the one that starts in (ra + di, ca + dj)."""
    R = np.zeros((M, N), np.uint8)
    t = np.arange(0, min(ra, ca) + 1)
    R[ra - t, ca - t] = 1
    t = np.arange(0, min(M - ra - di, N - ca - dj))
    R[ra + di + t, ca + dj + t] = 1
    return R


def test_strip_seam_on_diagonals_that_jump(ctx):
    """As tests/test_gpu_serra09_streaming.py's test of the same name: the only best path enters the strip's first or second column by a
    (1, 2) or a (2, 1) step (Q and S of column c - 2 of the row above, of column c - 1 two rows up), or by two such steps through one
    missing cell (the penalised halves).  The start must be the first diagonal's, (2, .), carried over the seam."""
    M = 64
    for s, (seam, N) in enumerate(((STRIP, 2 * STRIP + 2), (2 * STRIP, 3 * STRIP + 1))):
        for (di, dj), (hi, hj) in (((1, 2), (1, 2)), ((2, 1), (2, 1)), ((2, 4), (1, 2)), ((4, 2), (2, 1))):
            for col in (seam, seam + 1):
                row = 30 + (s + col) % 2
                ra, ca = row - hi, col - hj
                R = _two_diagonals(M, N, ra, ca, di, dj)
                tag = "diagonal that jumps by (%d, %d) from (%d, %d), seam %d" % (di, dj, ra, ca, seam)
                for setting in ((0.5, 0.5, 2), (0.5, 0.5, 3), (1.0, 0.25, 2), (0.25, 1.0, 3)):
                    got = _check_dp(ctx, R, setting, tag)
                    assert (got[1], got[2]) == (2, ca - ra + 2) and got[4] > seam, (tag, setting, got)


def test_ties_between_lanes_and_between_strips(ctx):
    """Two diagonals of equal score: the row-major first END wins -- the earlier row even in a higher lane or a later strip (whose rows the
    wave visits after all rows of the earlier strip), the smaller column in the same row -- which a plain maximum over the lanes does not."""
    L = 6
    cases = [((20, 40), (12, 500), 1), ((20, 40), (20, 500), 0),                     # different lanes of one strip
             ((20, 40), (12, 50), 1), ((20, 37), (20, 60), 0),                       # the same lane
             ((20, 100), (12, STRIP + 900), 1), ((20, 100), (20, STRIP + 900), 0),   # different strips
             ((20, STRIP + 5), (12, 2 * STRIP + 40), 1), ((12, 70), (20, 2 * STRIP + 40), 0),
             ((13, STRIP - 1), (12, STRIP + 9), 1), ((12, STRIP - 1), (12, STRIP + 9), 0)]
    for a, b, winner in cases:
        R = np.zeros((40, 2 * STRIP + 100), np.uint8)
        _diag(R, a, L)
        _diag(R, b, L)
        for setting in SETTINGS[:4]:
            got = _check_dp(ctx, R, setting, "ties %s %s" % (a, b))
            end = (a, b)[winner]
            assert got == (float(L), end[0] - L + 1, end[1] - L + 1, end[0], end[1]), (a, b, setting, got)


def test_dp_argument_errors(ctx):
    from acoss_amd import _lib
    R = np.eye(8, dtype=np.uint8)
    with pytest.raises(NotImplementedError, match="Qmax alignment only"):
        ctx.qmax_locate_binary(R, _lib.serra09_params(dmax=1))
    R[3, 3] = 2
    with pytest.raises(ValueError, match="non-binary"):
        ctx.qmax_locate_binary(R)
    assert _check_dp(ctx, np.eye(8, dtype=np.uint8), (0.5, 0.5, 2), "after the errors") == (6.0, 2, 2, 7, 7)


# ---- the product path -----------------------------------------------------------------------------------------------------------------------
M9 = 9
LONG = 2100                    # cells: beyond the last band class (2041), the streaming kernels
SIDES = S.UPPER + (300, LONG)


@pytest.fixture(scope="module")
def pool():
    """Two versions (the start and the end of one work) of a track at the upper edge of every band size class, of 300 and of 2100 cells."""
    rng = np.random.default_rng([9, 16])
    tracks, Ms, start, end, _ = S._two_ends(rng, SIDES, M9, 1)
    d = S._pack(tracks, Ms, [(start[a], end[a]) for a in S.UPPER] + [(end[300], end[LONG])], start=start, end=end)
    for c, a in enumerate(S.UPPER):                        # one pair per band class, at the class edge as the plan reports it
        assert S.key(a, a, M9) == (c, c) and S.cls(a + 1, M9) == c + 1
    assert S.key(300, LONG, M9) == (S.NC, S.NC)
    return d


def _align_against_plots(ctx, d, pairs, tag, **kw):
    """serra09_align over `pairs` against the reference on the device's own plots (serra09_debug_bits) and serra09_pairs' scores."""
    from acoss_amd import _lib
    p = _lib.serra09_params(**kw)
    got = ctx.serra09_align(pairs, p)
    scores, Rs = ctx.serra09_debug_bits(pairs, p)
    assert got.shape == (len(pairs),)
    for k, R in enumerate(Rs):
        want = ref.locate_forward(R, p.gamma_o, p.gamma_e, p.dp_start)
        assert _rec(got[k]) == want, "%s pair %d %s, %s plot: device %s, reference %s" % (tag, k, tuple(pairs[k]), R.shape, _rec(got[k]), want)
    assert np.array_equal(got["score"].view(np.uint32), ctx.serra09_pairs(pairs, p).view(np.uint32)), tag
    assert np.array_equal(got["score"].view(np.uint32), scores.view(np.uint32)), tag
    return got


def test_one_pair_per_class_streaming_and_mixed(ctx, pool):
    ctx.upload_pool(pool["frames"], pool["offsets"])
    pairs = pool["pairs"]
    each = np.concatenate([_align_against_plots(ctx, pool, pairs[k:k + 1], "class %d alone" % k, m=M9) for k in range(len(pairs))])
    assert np.all(each["score"] > 0)
    k = len(pairs) - 1                                     # the streaming pair: the last 300 cells of a 2100-cell version of the same work
    assert each[k]["r1"] >= STRIP > each[k]["r0"], "the streaming pair's alignment crosses the strip seam: %s" % (each[k],)
    mixed = _align_against_plots(ctx, pool, pairs, "mixed list", m=M9)
    assert np.array_equal(mixed, each)
    assert np.array_equal(_align_against_plots(ctx, pool, pairs[::-1].copy(), "mixed list reversed", m=M9), each[::-1])
    _align_against_plots(ctx, pool, pairs, "mixed list, gammas (1, 0.25), dp_start 3", m=M9, gamma_o=1.0, gamma_e=0.25, dp_start=3)
    # a stack of 17 frames: every pair streams, however short
    short = np.array([[pool["start"][249], pool["end"][505]]], np.int32)
    _align_against_plots(ctx, pool, short, "m = 17", m=17)


def test_two_batches_give_the_records_of_one(ctx, pool):
    from acoss_amd import _lib
    st, en = pool["start"], pool["end"]
    pairs = np.array([(st[a], en[b]) for a in (249, 300, 505) for b in (249, 300, 505)] + [(en[300], en[LONG]), (st[LONG], st[300])], np.int32)
    p = _lib.serra09_params(m=M9)
    lens = np.diff(pool["offsets"])
    limit = 6 << 20                                        # bytes: either streaming pair alone takes 5.3 MB of D2, D2^T and strip records
    assert np.all(_lib.serra09_plan(lens, pairs, p)["batch"] == 0)
    assert _lib.serra09_plan(lens, pairs, p, scratch_limit=limit)["batch"].max() >= 1
    ctx.upload_pool(pool["frames"], pool["offsets"])
    one = ctx.serra09_align(pairs, p)
    ctx.set_scratch_limit(limit)
    try:
        assert np.array_equal(ctx.serra09_align(pairs, p), one)
        assert np.array_equal(ctx.serra09_align(pairs[::-1].copy(), p), one[::-1])
    finally:
        ctx.set_scratch_limit(0)
    assert np.array_equal(one["score"].view(np.uint32), ctx.serra09_pairs(pairs, p).view(np.uint32))


def test_refused_lists_launch_nothing(ctx, pool):
    """The codes of acx_serra09_pairs, for the whole list before the first launch; the next valid call succeeds."""
    from acoss_amd import _lib
    ctx.upload_pool(pool["frames"], pool["offsets"])
    n = len(pool["M"])
    p = _lib.serra09_params(m=M9)
    good = pool["pairs"][:2]
    want = ctx.serra09_align(good, p)
    for bad in ([n, 0], [0, -1]):
        with pytest.raises(ValueError, match="track index out of range in pair 2"):
            ctx.serra09_align(np.concatenate([good, [bad]]), p)
        with pytest.raises(ValueError, match="track index out of range in pair 2"):
            ctx.serra09_pairs(np.concatenate([good, [bad]]), p)
    with pytest.raises(NotImplementedError, match="Qmax alignment only"):
        ctx.serra09_align(good, _lib.serra09_params(m=M9, dmax=1))
    # a stack longer than the 249-cell tracks (258 frames): ACX_ERR_SHORT from both entries
    for call in (ctx.serra09_align, ctx.serra09_pairs):
        with pytest.raises(_lib.AcxError, match="shorter than the delay-embedding stack"):
            call(good, _lib.serra09_params(m=30, tau=9))
    assert np.array_equal(ctx.serra09_align(good, p), want)


def test_profile_names_the_kernel(ctx, pool):
    from acoss_amd import _lib
    ctx.upload_pool(pool["frames"], pool["offsets"])
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        ctx.serra09_align(pool["pairs"][:2], _lib.serra09_params(m=M9))
        prof = ctx.profile()
    finally:
        ctx.profile_enable(False)
    assert prof["qmax_locate_kernel"]["launches"] == 1 and prof["qmax_locate_kernel"]["ms"] > 0
    assert prof["qmax_bits_kernel"]["launches"] == 0, "the score sweep does not run for an alignment call"


# ---- Serra09.align / align_matches ----------------------------------------------------------------------------------------------------------
def _dataset(tmp_path, tag, n):
    path = tmp_path / ("%s.csv" % tag)
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


def _serra09(tmp_path, tag, tracks, **kw):
    from acoss_amd.algorithms import Serra09
    a = Serra09(_dataset(tmp_path, tag, len(tracks)), "feat/", shortname=tag, **kw)
    a.set_pooled_features(tracks, ["w%d" % (i // 2) for i in range(len(tracks))])
    return a


def test_planted_excerpt(tmp_path, monkeypatch):
    """Track B is random chroma with pooled frames [50, 130) copied from track A's [20, 100): with m = 9, tau = 1 the 72 embedded frames
    50 .. 121 of B are identical to A's 20 .. 91, their distance is 0 and, the threshold being inclusive, those 72 cells recur on one
    diagonal away from the first two rows and columns: score >= 72.  The overlap of the reported spans with the planted ones is printed."""
    from acoss_amd import synth
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(11)
    A = synth._frame_max_normalise(rng.random((150, 12))).astype(np.float32)
    B = synth._frame_max_normalise(rng.random((200, 12))).astype(np.float32)
    B[50:130] = A[20:100]
    algo = _serra09(tmp_path, "excerpt", [A, B], oti=False, m=9, tau=1)
    try:
        got = algo.align([[1, 0], [0, 1]])
        assert got.shape == (2,) and np.all(got["score"] >= 72), got
        _, Rs = algo._context().serra09_debug_bits(np.array([[1, 0], [0, 1]], np.int32), algo._params())
        for k, R in enumerate(Rs):
            assert _rec(got[k]) == ref.locate_forward(R), (k, got[k])
        for k, (qs, rs) in enumerate((((50, 129), (20, 99)), ((20, 99), (50, 129)))):
            for name, (lo, hi), span in (("query", qs, got[k]["q_span"]), ("reference", rs, got[k]["r_span"])):
                assert 0 <= span[0] <= span[1] < (200 if (name == "query") == (k == 0) else 150)
                both = max(0, min(hi, int(span[1])) - max(lo, int(span[0])) + 1)
                print("pair %d %s: planted [%d, %d], reported [%d, %d]: %d of %d planted frames covered, %d reported outside" % (
                    k, name, lo, hi, span[0], span[1], both, hi - lo + 1, int(span[1]) - int(span[0]) + 1 - both))
            assert tuple(got[k]["q_span"]) == (int(got[k]["q0"]), int(got[k]["q1"]) + 8)
    finally:
        algo._ctx.close()
        algo._ctx = None
        algo.cleanup_memmap()


def test_align_matches_on_identify_output(tmp_path, monkeypatch):
    from acoss_amd import synth
    monkeypatch.chdir(tmp_path)
    d = synth.cover_set(n_works=6, versions=2, seed=5, t_range=(60, 120))
    n = len(d["offsets"]) - 1
    assert n == 12
    algo = _serra09(tmp_path, "matches", [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for i in range(n)])
    try:
        queries = [0, 7, 3, 7]
        idx, _ = algo.identify(queries, k=12)["main"]      # eleven candidates: the last slot of every row is empty
        assert idx.shape == (4, 12) and np.all(idx[:, -1] == -1) and np.all(idx[:, :-1] >= 0)
        got = algo.align_matches(queries, idx)
        assert got.shape == (4, 12) and got.dtype == algo.ALIGN_DTYPE
        empty = got[idx < 0]
        assert np.all(empty["score"] == 0)
        for f in ("q0", "r0", "q1", "r1", "q_span", "r_span"):
            assert np.all(empty[f] == -1)
        for i, q in enumerate(queries):
            row = algo.align([[q, j] for j in idx[i, :-1]])
            assert np.array_equal(got[i, :-1], row), i
        assert np.array_equal(got[1], got[3])
        scores = algo._context().serra09_pairs(np.array([[queries[0], j] for j in idx[0, :-1]], np.int32), algo._params())
        assert np.array_equal(got[0, :-1]["score"].view(np.uint32), scores.view(np.uint32))
        hit = got["q0"] >= 0
        T = np.diff(d["offsets"])
        assert np.all(got["q_span"][hit][:, 0] == got["q0"][hit]) and np.all(got["q_span"][hit][:, 1] == got["q1"][hit] + 8)
        assert np.all(got["r_span"][hit][:, 1] < T[idx[hit]])
        assert np.all(got["q_span"][~hit] == -1) and np.all((got["score"] == 0) == ~hit)
    finally:
        algo._ctx.close()
        algo._ctx = None
        algo.cleanup_memmap()
