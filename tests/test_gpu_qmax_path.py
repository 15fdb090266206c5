"""
GPU tests (run with -m gpu on a real MI355X): the PATH of the Qmax alignment -- qmax_path_kernel<EQG>
(acoss_amd/csrc/serra09_path_kernels.hpp) through acx_qmax_path_binary (the DP alone on a given plot) and acx_serra09_align_paths
(the product chain), Serra09.align_paths and Serra09.align_match_paths.

Every comparison is exact: the record, the offsets and every cell against the full-matrix restatement of the contract
(tests/_qmax_path_ref.py path_full; tests/test_qmax_path_ref.py holds it against the DP on the box alone and against
locate_forward), and the record also against the locating sweep's on the same arguments, bit for bit.

The kernel gives a lane 32 BOX columns, a wave a strip of 2048 of them; the box starts at any plot column r0, so the lane's bits
come through a funnel shift by (7 - (i & 7) + r0) mod 32 from dwords that move with the row.
"""
import numpy as np
import pytest

from tests import _qmax_path_ref as ref
from tests import _serra09_shapes as S

pytestmark = pytest.mark.gpu

C = 32                         # box columns per lane (PATH_CPL)
STRIP = 64 * C
GAMMAS = ((0.5, 0.5), (1.0, 0.25), (0.25, 1.0))
SETTINGS = [(go, ge, st) for st in (2, 3) for go, ge in GAMMAS]
FIELDS = ("score", "q0", "r0", "q1", "r1")


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _rec(a):
    return (float(a["score"]),) + tuple(int(a[f]) for f in FIELDS[1:])


def _check_dp(ctx, R, setting, tag):
    """qmax_path_binary on R against path_full: record and cells; the record against qmax_locate_binary's bytes.  Returns the reference."""
    from acoss_amd import _lib
    go, ge, st = setting
    p = _lib.serra09_params(gamma_o=go, gamma_e=ge, dp_start=st)
    got, cells = ctx.qmax_path_binary(R, p)
    assert got.shape == (1,) and got.dtype == _lib.ALIGNMENT_DTYPE and cells.dtype == np.int32 and cells.ndim == 2 and cells.shape[1] == 2
    want, wcells, _ = ref.path_full(R, go, ge, st)
    label = "%s, %s plot, gammas (%s, %s), dp_start %d" % (tag, R.shape, go, ge, st)
    assert _rec(got[0]) == want, "%s: device %s, reference %s" % (label, _rec(got[0]), want)
    assert got.tobytes() == ctx.qmax_locate_binary(R, p).tobytes(), label
    if not np.array_equal(cells, wcells):
        n = min(len(cells), len(wcells))
        first = int(np.argmax(np.any(cells[:n] != wcells[:n], axis=1))) if n and np.any(cells[:n] != wcells[:n]) else n
        raise AssertionError("%s: %d cells, reference %d; they part at cell %d: device %s, reference %s" % (
            label, len(cells), len(wcells), first, cells[first:first + 3].tolist(), wcells[first:first + 3].tolist()))
    return want, wcells


# ---- the DP alone ---------------------------------------------------------------------------------------------------------------------------
def test_hand_checked_plots(ctx):
    for name, R, setting, rec, cells in ref.HAND:
        want, wcells = _check_dp(ctx, R, setting, name)
        assert want == rec and [tuple(c) for c in wcells] == cells, name


@pytest.mark.parametrize("N", [1, 2, 3, 31, 32, 33, 34, 63, 64, 65, 2047, 2048, 2049, 4097])
def test_random_plots(ctx, N):
    rng = np.random.default_rng([23, N])
    for M in (1, 2, 3, 4, 5, 9, 64):
        R = (rng.random((M, N)) < rng.choice([0.05, 0.3, 0.6])).astype(np.uint8)
        for setting in SETTINGS:
            _check_dp(ctx, R, setting, "random plot")


def plant(R, i, j, steps, rng=None, n=None):
    """Ones along a path from (i, j): `steps` is a sequence of (di, dj) taken in turn (cyclically), or with `rng` drawn from; up to n
    cells or the plot's edge.  Returns the cells."""
    cells = []
    t = 0
    while i < R.shape[0] and j < R.shape[1] and (n is None or len(cells) < n):
        R[i, j] = 1
        cells.append((i, j))
        di, dj = steps[int(rng.integers(0, len(steps)))] if rng is not None else steps[t % len(steps)]
        i, j, t = i + di, j + dj, t + 1
    return cells


MIXED = ((1, 1), (1, 2), (2, 1), (1, 2))


@pytest.mark.parametrize("r0m", [0, 1, 31, 32, 33, 63])
def test_planted_paths_at_the_funnel_shift_and_skew_edges(ctx, r0m):
    """A path of mixed steps planted alone, so that the box starts exactly where it does: r0 mod 64 on both sides of a dword and of a
    bitmap word, q0 mod 8 at both ends of the bitmap's skew; 150 cells cross several lane edges of the box."""
    rng = np.random.default_rng([29, r0m])
    for q0m in (0, 1, 7):
        q0, r0 = 8 + q0m, 64 + r0m
        R = np.zeros((q0 + 260, r0 + 300), np.uint8)
        cells = plant(R, q0, r0, MIXED, rng, n=150)
        for setting in ((0.5, 0.5, 2), (1.0, 0.25, 2), (0.25, 1.0, 3)):
            want, wcells = _check_dp(ctx, R, setting, "planted at (%d, %d)" % (q0, r0))
            assert want[1:3] == (q0, r0) and [tuple(c) for c in wcells] == cells and want[4] - want[2] > 4 * C


def test_planted_path_across_every_lane_edge(ctx):
    """One box of 2040 columns inside one strip: a path of mixed steps, in sparse noise below and right of its start, from lane 0 to lane 63."""
    rng = np.random.default_rng(31)
    R = np.zeros((1500, 2060), np.uint8)
    R[12:, 20:] = rng.random((1488, 2040)) < 0.01
    plant(R, 11, 19, ((1, 2), (1, 1), (1, 2), (2, 1), (1, 2)), rng)
    for setting in ((0.5, 0.5, 2), (1.0, 0.25, 3)):
        want, wcells = _check_dp(ctx, R, setting, "a path across every lane edge")
        assert want[1:3] == (11, 19) and STRIP - 3 * C < want[4] - want[2] + 1 <= STRIP, want
        assert len(set((wcells[:, 1] - 19) // C)) == 64, "the path has a cell in every lane's columns"


@pytest.mark.parametrize("variant", ["a (1, 2) step onto the seam column", "a (1, 2) step over the seam column", "a missing cell at the seam"])
def test_one_wide_box(ctx, variant):
    """A box wider than 2048 columns on a plot of 1200 x 2400: a path planted from column 5 mostly in (1, 2) steps.  The box's strip seam
    lies at r0 + 2048 = 2053, not at plot column 2048; the path crosses it by a (1, 2) step that lands on the second strip's first column
    (from its left neighbour's column c - 2), by one that lands on its second (from c - 1), or along a diagonal with the cell at c - 1
    missing (the penalised values of the seam record)."""
    R = np.zeros((1200, 2400), np.uint8)
    seam = 5 + STRIP
    pre = plant(R, 3, 5, ((1, 2),) * 19 + ((1, 1),) + ((1, 2),) * 19 + ((2, 1),), n=1100)
    pre = [c for c in pre if c[1] < seam - 12]
    R[:] = 0
    for c in pre:
        R[c] = 1
    i, j = pre[-1]
    run = []
    while j + 1 < seam - 8:                              # a diagonal up to the neighbourhood of the seam
        i, j = i + 1, j + 1
        run.append((i, j))
    if variant == "a (1, 2) step onto the seam column":
        land = seam
    elif variant == "a (1, 2) step over the seam column":
        land = seam + 1
    else:
        land = None
    while j < (land - 2 if land is not None else seam - 2):
        i, j = i + 1, j + 1
        run.append((i, j))
    if land is not None:
        i, j = i + 1, j + 2                              # the (1, 2) step
        assert j == land
        run.append((i, j))
    else:
        assert j == seam - 2                             # (i + 1, seam - 1) stays 0; the diagonal goes on at (i + 2, seam)
        i, j = i + 2, j + 2
        run.append((i, j))
    for c in run:
        R[c] = 1
    tail = plant(R, i + 1, j + 1, ((1, 1), (1, 2), (1, 2)), n=80)
    assert tail[-1][1] < 2399 and tail[-1][0] < 1199
    for setting in ((0.5, 0.5, 2), (1.0, 0.25, 3), (0.25, 1.0, 2)):
        want, wcells = _check_dp(ctx, R, setting, "wide box, " + variant)
        assert want[1:3] == (3, 5) and want[4] - want[2] + 1 > STRIP, want
        cols = set(wcells[:, 1].tolist())
        assert min(cols) == 5 and max(cols) > seam + 100, "the path crosses the seam of the BOX at column %d" % seam
        if land is not None:
            assert land in cols and land - 2 in cols and land - 1 not in cols
        else:
            gap = [tuple(c) for c in wcells if c[1] == seam - 1]
            assert seam - 2 in cols and seam in cols and len(gap) == 1 and R[gap[0]] == 0, "the path runs THROUGH the missing cell"


def test_ties_among_the_three_predecessors(ctx):
    """Dense plots: ties among c2, c3, c4 in match cells and among the penalised a2, a3, a4 in gap cells, with gamma_o != gamma_e too."""
    rng = np.random.default_rng(37)
    plots = [np.ones((20, 80), np.uint8), np.ones((70, 9), np.uint8)]
    R = np.ones((24, 70), np.uint8)
    R[::3, ::4] = 0
    plots.append(R)
    R = np.ones((30, 100), np.uint8)
    R[5::2] = 0                                          # every second row empty: every step a (2, 1) step through gap rows
    plots.append(R)
    for _ in range(4):
        plots.append((rng.random((int(rng.integers(10, 40)), int(rng.integers(40, 130)))) < 0.85).astype(np.uint8))
    for R in plots:
        for setting in SETTINGS + [(0.5, 0.7, 2), (0.0, 0.0, 2)]:
            _check_dp(ctx, R, setting, "ties")


def test_empty_plot_and_capacity(ctx):
    from acoss_amd import _lib
    for setting in SETTINGS:
        want, cells = _check_dp(ctx, np.zeros((7, 9), np.uint8), setting, "all zero")
        assert want == ref.NO_MATCH and cells.shape == (0, 2)
        for shape in ((2, 5), (5, 2), (1, 1)):
            assert _check_dp(ctx, np.ones(shape, np.uint8), setting, "smaller than 3 x 3")[0] == ref.NO_MATCH
    R = np.eye(12, 20, dtype=np.uint8)
    with pytest.raises(ValueError, match="cap 11 is too small: 12 cells required"):
        ctx.qmax_path_binary(R, cap=11)
    with pytest.raises(NotImplementedError, match="Qmax alignment only"):
        ctx.qmax_path_binary(R, _lib.serra09_params(dmax=1))
    bad = R.copy()
    bad[3, 3] = 2
    with pytest.raises(ValueError, match="non-binary"):
        ctx.qmax_path_binary(bad)
    rec, cells = ctx.qmax_path_binary(R, cap=12)
    assert _rec(rec[0]) == (10.0, 2, 2, 11, 11) and cells.tolist() == [[t, t] for t in range(2, 12)]


# ---- the product path -----------------------------------------------------------------------------------------------------------------------
M9 = 9
LONG = 2100                    # cells: beyond the last band class (2041), the streaming kernels
SIDES = S.UPPER + (300, LONG)


@pytest.fixture(scope="module")
def pool():
    """The pool of tests/test_gpu_qmax_locate.py: two versions (the start and the end of one work) of a track at the upper edge of every
    band size class, of 300 and of 2100 cells."""
    rng = np.random.default_rng([9, 16])
    tracks, Ms, start, end, _ = S._two_ends(rng, SIDES, M9, 1)
    d = S._pack(tracks, Ms, [(start[a], end[a]) for a in S.UPPER] + [(end[300], end[LONG])], start=start, end=end)
    for c, a in enumerate(S.UPPER):                        # one pair per band class, at the class edge as the plan reports it
        assert S.key(a, a, M9) == (c, c) and S.cls(a + 1, M9) == c + 1
    assert S.key(300, LONG, M9) == (S.NC, S.NC)
    return d


_REFS = {}


def _reference(R, p):
    """path_full of a device plot, computed once per (plot, penalties, dp_start)."""
    key = (R.shape, R.tobytes(), float(p.gamma_o), float(p.gamma_e), int(p.dp_start))
    if key not in _REFS:
        _REFS[key] = ref.path_full(R, p.gamma_o, p.gamma_e, p.dp_start)
    return _REFS[key]


def _paths_against_plots(ctx, pairs, tag, **kw):
    """serra09_align_paths over `pairs` against the reference on the device's own plots (serra09_debug_bits); the records against
    serra09_align's bytes."""
    from acoss_amd import _lib
    p = _lib.serra09_params(**kw)
    got, off, cells = ctx.serra09_align_paths(pairs, p)
    assert got.tobytes() == ctx.serra09_align(pairs, p).tobytes(), tag
    _, Rs = ctx.serra09_debug_bits(pairs, p)
    assert got.shape == (len(pairs),) and off.shape == (len(pairs) + 1,) and off[0] == 0 and cells.shape == (off[-1], 2)
    for k, R in enumerate(Rs):
        want, wcells, _ = _reference(R, p)
        label = "%s pair %d %s, %s plot" % (tag, k, tuple(pairs[k]), R.shape)
        assert _rec(got[k]) == want, "%s: device %s, reference %s" % (label, _rec(got[k]), want)
        assert off[k + 1] - off[k] == len(wcells), label
        assert np.array_equal(cells[off[k]:off[k + 1]], wcells), label
    return got, off, cells


def test_one_pair_per_class_streaming_and_mixed(ctx, pool):
    ctx.upload_pool(pool["frames"], pool["offsets"])
    pairs = pool["pairs"]
    each = [_paths_against_plots(ctx, pairs[k:k + 1], "class %d alone" % k, m=M9) for k in range(len(pairs))]
    assert all(len(e[2]) > 0 for e in each)
    mixed = _paths_against_plots(ctx, pairs, "mixed list", m=M9)
    assert np.array_equal(mixed[0], np.concatenate([e[0] for e in each])) and np.array_equal(mixed[2], np.concatenate([e[2] for e in each]))
    rev = _paths_against_plots(ctx, pairs[::-1].copy(), "mixed list reversed", m=M9)
    assert np.array_equal(rev[0], mixed[0][::-1]) and np.array_equal(rev[2], np.concatenate([e[2] for e in each[::-1]]))
    _paths_against_plots(ctx, pairs, "mixed list, gammas (1, 0.25), dp_start 3", m=M9, gamma_o=1.0, gamma_e=0.25, dp_start=3)
    # a stack of 17 frames: every pair streams, however short
    short = np.array([[pool["start"][249], pool["end"][505]]], np.int32)
    _paths_against_plots(ctx, short, "m = 17", m=17)


def _launches(ctx, call):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        out = call()
        prof = ctx.profile()
    finally:
        ctx.profile_enable(False)
    return out, prof["qmax_locate_kernel"]["launches"], prof["qmax_path_kernel"]["launches"], prof


def test_batches_chunks_and_the_budget(ctx, pool):
    """Two batches under a scratch limit give the paths of one; under a smaller limit the boxes of a batch run in more than one chunk
    of the direction plane (half the limit); a box beyond that budget is ACX_ERR_NOMEM and the next valid call succeeds."""
    from acoss_amd import _lib
    st, en = pool["start"], pool["end"]
    p = _lib.serra09_params(m=M9)
    lens = np.diff(pool["offsets"])
    ctx.upload_pool(pool["frames"], pool["offsets"])
    # two batches: the list of tests/test_gpu_qmax_locate.py (either streaming pair alone takes 5.3 MB of the 6 MB)
    pairs = np.array([(st[a], en[b]) for a in (249, 300, 505) for b in (249, 300, 505)] + [(en[300], en[LONG]), (st[LONG], st[300])], np.int32)
    limit = 6 << 20
    assert np.all(_lib.serra09_plan(lens, pairs, p)["batch"] == 0)
    assert _lib.serra09_plan(lens, pairs, p, scratch_limit=limit)["batch"].max() >= 1
    one, nloc, npath, prof = _launches(ctx, lambda: _paths_against_plots(ctx, pairs, "one batch", m=M9))
    ctx.set_scratch_limit(limit)
    try:
        two = ctx.serra09_align_paths(pairs, p)
        assert all(np.array_equal(a, b) for a, b in zip(one, two))
        rev = ctx.serra09_align_paths(pairs[::-1].copy(), p)
        assert np.array_equal(rev[0], one[0][::-1]) and rev[1][-1] == one[1][-1]
    finally:
        ctx.set_scratch_limit(0)
    # chunks: versions of the SAME start of the work, so that the boxes cover most of the plots; band classes only
    pairs = np.array([(st[a], st[b]) for a in (249, 300, 505) for b in (249, 300, 505) if a != b], np.int32)
    want = _paths_against_plots(ctx, pairs, "chunk list, no limit", m=M9)
    al = want[0]
    assert np.all(al["q0"] >= 0)
    plane = (al["q1"] - al["q0"] + 1).astype(np.int64) * ((al["r1"] - al["r0"] + 1 + 31) // 32) * 8      # bytes: one u64 per 32 box columns
    limit = 2 * int(plane.max())                           # budget = half the limit: the largest plane alone fills a chunk
    plan = _lib.serra09_plan(lens, pairs, p, scratch_limit=limit)
    print("direction planes %s bytes, scratch limit %d, batches %s" % (plane.tolist(), limit, plan["batch"].tolist()))
    assert np.bincount(plan["batch"]).max() >= 2, "a batch of at least two pairs, whose planes exceed the budget together"
    ctx.set_scratch_limit(limit)
    try:
        got, nloc, npath, prof = _launches(ctx, lambda: ctx.serra09_align_paths(pairs, p))
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert nloc == plan["batch"].max() + 1 and npath > nloc, "more chunks (%d) than batches (%d)" % (npath, nloc)
        assert prof["qmax_path_kernel"]["ms"] > 0 and prof["qmax_bits_kernel"]["launches"] == 0
        ctx.set_scratch_limit(limit - 16)                  # the largest plane no longer fits half the limit
        with pytest.raises(MemoryError, match="beyond the path budget"):
            ctx.serra09_align_paths(pairs, p)
    finally:
        ctx.set_scratch_limit(0)
    assert all(np.array_equal(a, b) for a, b in zip(ctx.serra09_align_paths(pairs, p), want))


def test_refused_lists_launch_nothing(ctx, pool):
    """The codes of acx_serra09_align, for the whole list before the first launch; cap below the bound; the next valid call succeeds."""
    from acoss_amd import _lib
    ctx.upload_pool(pool["frames"], pool["offsets"])
    n = len(pool["M"])
    p = _lib.serra09_params(m=M9)
    good = pool["pairs"][:2]
    want = ctx.serra09_align_paths(good, p)

    def launches_nothing(exc, match, call):
        ctx.profile_enable(True)
        try:
            ctx.profile_reset()
            with pytest.raises(exc, match=match):
                call()
            prof = ctx.profile()
        finally:
            ctx.profile_enable(False)
        assert sum(v["launches"] for v in prof.values()) == 0, {k: v["launches"] for k, v in prof.items() if v["launches"]}

    for bad in ([n, 0], [0, -1]):
        launches_nothing(ValueError, "track index out of range in pair 2", lambda: ctx.serra09_align_paths(np.concatenate([good, [bad]]), p))
    launches_nothing(NotImplementedError, "Qmax alignment only", lambda: ctx.serra09_align_paths(good, _lib.serra09_params(m=M9, dmax=1)))
    launches_nothing(_lib.AcxError, "shorter than the delay-embedding stack", lambda: ctx.serra09_align_paths(good, _lib.serra09_params(m=30, tau=9)))
    bound = sum(min(int(pool["M"][i]), int(pool["M"][j])) for i, j in good)
    launches_nothing(ValueError, "cap %d is too small: %d cells required" % (bound - 1, bound), lambda: ctx.serra09_align_paths(good, p, cap=bound - 1))
    got = ctx.serra09_align_paths(good, p, cap=bound)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_profile_names_the_kernel(ctx, pool):
    from acoss_amd import _lib
    ctx.upload_pool(pool["frames"], pool["offsets"])
    _, nloc, npath, prof = _launches(ctx, lambda: ctx.serra09_align_paths(pool["pairs"][:2], _lib.serra09_params(m=M9)))
    assert (nloc, npath) == (1, 1) and prof["qmax_path_kernel"]["ms"] > 0 and prof["qmax_path_kernel"]["cells"] > 0
    print("locate %.3f ms, path %.3f ms for two pairs" % (prof["qmax_locate_kernel"]["ms"], prof["qmax_path_kernel"]["ms"]))


# ---- Serra09.align_paths / align_match_paths ------------------------------------------------------------------------------------------------
def _dataset(tmp_path, tag, n):
    path = tmp_path / ("%s.csv" % tag)
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


def _serra09(tmp_path, tag, tracks, cls=None, **kw):
    from acoss_amd.algorithms import Serra09
    a = (cls or Serra09)(_dataset(tmp_path, tag, len(tracks)), "feat/", shortname=tag, **kw)
    a.set_pooled_features(tracks, ["w%d" % (i // 2) for i in range(len(tracks))])
    return a


def _close(algo):
    algo._ctx.close()
    algo._ctx = None
    algo.cleanup_memmap()


def test_align_paths_on_the_planted_excerpt(tmp_path, monkeypatch):
    """The planted excerpt of tests/test_gpu_qmax_locate.py: B's pooled frames [50, 130) are A's [20, 100), so with m = 9, tau = 1 the
    embedded frames 50 .. 121 of B equal A's 20 .. 91: the copy's diagonal is r - q = -30 for (B, A) and +30 for (A, B).  The share of
    path cells on it is printed, not asserted."""
    from acoss_amd import synth
    from acoss_amd.algorithms import ChenFusion
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(11)
    A = synth._frame_max_normalise(rng.random((150, 12))).astype(np.float32)
    B = synth._frame_max_normalise(rng.random((200, 12))).astype(np.float32)
    B[50:130] = A[20:100]
    idxs = [[1, 0], [0, 1]]
    algo = _serra09(tmp_path, "pathexcerpt", [A, B], oti=False, m=9, tau=1)
    try:
        al, paths = algo.align_paths(idxs)
        plain = algo.align(idxs)
        assert al.dtype == plain.dtype == algo.ALIGN_DTYPE and al.tobytes() == plain.tobytes()
        for f in algo.ALIGN_DTYPE.names:
            assert np.array_equal(al[f], plain[f]), f
        _, Rs = algo._context().serra09_debug_bits(np.array(idxs, np.int32), algo._params())
        assert len(paths) == 2
        for k, (R, diag) in enumerate(zip(Rs, (-30, 30))):
            want, wcells, _ = ref.path_full(R)
            assert paths[k].dtype == np.int32 and np.array_equal(paths[k], wcells), k
            assert tuple(paths[k][0]) == (al[k]["q0"], al[k]["r0"]) and tuple(paths[k][-1]) == (al[k]["q1"], al[k]["r1"])
            on = int(np.sum(paths[k][:, 1] - paths[k][:, 0] == diag))
            print("pair %d: %d path cells, %d (%.0f %%) on the copy's diagonal r - q = %d" % (k, len(paths[k]), on, 100.0 * on / len(paths[k]), diag))
        assert algo.align_paths(np.zeros((0, 2), np.int64))[1] == []
    finally:
        _close(algo)
    chen = _serra09(tmp_path, "pathchen", [A, B], cls=ChenFusion, oti=False, m=9, tau=1)
    try:
        cal, cpaths = chen.align_paths(idxs)                # the Qmax path of ChenFusion's plot: the same plot, the same path
        assert cal.tobytes() == al.tobytes() and all(np.array_equal(a, b) for a, b in zip(cpaths, paths))
    finally:
        _close(chen)


def test_align_match_paths_on_identify_output(tmp_path, monkeypatch):
    from acoss_amd import synth
    monkeypatch.chdir(tmp_path)
    d = synth.cover_set(n_works=6, versions=2, seed=5, t_range=(60, 120))
    n = len(d["offsets"]) - 1
    algo = _serra09(tmp_path, "pathmatches", [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for i in range(n)])
    try:
        queries = [0, 7, 3, 7]
        idx, _ = algo.identify(queries, k=12)["main"]      # eleven candidates: the last slot of every row is empty
        assert idx.shape == (4, 12) and np.all(idx[:, -1] == -1) and np.all(idx[:, :-1] >= 0)
        got, paths = algo.align_match_paths(queries, idx)
        assert got.tobytes() == algo.align_matches(queries, idx).tobytes()
        assert len(paths) == 4 and all(len(row) == 12 for row in paths)
        for i, q in enumerate(queries):
            assert paths[i][-1].shape == (0, 2) and paths[i][-1].dtype == np.int32, "an empty slot has an empty path"
            row_al, row_paths = algo.align_paths([[q, j] for j in idx[i, :-1]])
            assert np.array_equal(got[i, :-1], row_al)
            for s in range(11):
                assert np.array_equal(paths[i][s], row_paths[s]), (i, s)
                if got[i, s]["q0"] >= 0:
                    assert tuple(paths[i][s][0]) == (got[i, s]["q0"], got[i, s]["r0"]) and tuple(paths[i][s][-1]) == (got[i, s]["q1"], got[i, s]["r1"])
                else:
                    assert len(paths[i][s]) == 0
        _, Rs = algo._context().serra09_debug_bits(np.array([[queries[0], j] for j in idx[0, :-1]], np.int32), algo._params())
        for s, R in enumerate(Rs):
            assert np.array_equal(paths[0][s], ref.path_full(R)[1]), s
    finally:
        _close(algo)
