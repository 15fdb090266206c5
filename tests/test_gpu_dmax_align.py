"""
GPU tests (run with -m gpu on a real MI355X): WHERE the Dmax alignment lies and its PATH -- dmax_locate_kernel<EQG> and dmax_path_kernel<EQG>
(acoss_amd/csrc/chen_align_kernels.hpp) through acx_dmax_locate_binary / acx_dmax_path_binary (the DP alone on a given plot),
acx_chenfusion_align / acx_chenfusion_align_paths (the product chain) and ChenFusion.align*(similarity_type="dmax").

Every comparison is exact, against the full-matrix restatement of the contract (tests/_dmax_align_ref.py dmax_full;
tests/test_dmax_align_ref.py holds it against the forward propagation, the DP on the box alone and the oracle's Dmax).

Both kernels give a lane 32 columns and a wave a strip of 2048: plot columns in the locating sweep, BOX columns in the path pass.  What
Dmax adds, and what the shapes below sit on: the bonus bit R[i][j-1] of a lane's first column lies in the left lane's word, of a strip's
first column across the seam; the bonus bit R[i-1][j] lies in the previous row's word, whose phase (i & 7) differs; the box's first row and
column take their values from bits OUTSIDE the box.
"""
import numpy as np
import pytest

from tests import _dmax_align_ref as ref
from tests import _serra09_shapes as S

pytestmark = pytest.mark.gpu

C = 32                         # columns per lane (LOC_CPL, PATH_CPL)
STRIP = 64 * C
SETTINGS = [(go, ge, st) for st in (2, 3) for go, ge in ref.GAMMAS]
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
    """dmax_path_binary on R against dmax_full: record and cells; the record against dmax_locate_binary's bytes.  Returns the reference."""
    from acoss_amd import _lib
    go, ge, st = setting
    p = _lib.serra09_params(gamma_o=go, gamma_e=ge, dp_start=st)
    got, cells = ctx.dmax_path_binary(R, p)
    assert got.shape == (1,) and got.dtype == _lib.ALIGNMENT_DTYPE and cells.dtype == np.int32 and cells.ndim == 2 and cells.shape[1] == 2
    want, wcells, wq = ref.dmax_full(R, go, ge, st)
    label = "%s, %s plot, gammas (%s, %s), dp_start %d" % (tag, R.shape, go, ge, st)
    loc = ctx.dmax_locate_binary(R, p)
    assert _rec(loc[0]) == want, "%s: locating sweep %s, reference %s" % (label, _rec(loc[0]), want)
    assert got.tobytes() == loc.tobytes(), label
    if not np.array_equal(cells, wcells):
        n = min(len(cells), len(wcells))
        first = int(np.argmax(np.any(cells[:n] != wcells[:n], axis=1))) if n and np.any(cells[:n] != wcells[:n]) else n
        raise AssertionError("%s: %d cells, reference %d; they part at cell %d: device %s, reference %s" % (
            label, len(cells), len(wcells), first, cells[first:first + 3].tolist(), wcells[first:first + 3].tolist()))
    return want, wcells, wq


# ---- the DP alone ---------------------------------------------------------------------------------------------------------------------------
def test_hand_checked_plots(ctx):
    for name, R, setting, rec, cells, qs in ref.HAND:
        want, wcells, wq = _check_dp(ctx, R, setting, name)
        assert want == rec and [tuple(c) for c in wcells] == cells and wq.tolist() == [float(v) for v in qs], name


@pytest.mark.parametrize("N", [1, 2, 3, 31, 32, 33, 34, 63, 64, 65, STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 1])
def test_random_plots(ctx, N):
    rng = np.random.default_rng([41, N])
    for M in (1, 2, 3, 4, 5, 9, 64):
        R = ref.random_plot(rng, M, N, rng.choice([0.05, 0.3, 0.6]))
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


# 32 columns and 19 rows a period, from a multiple of 32 to the next, where it LANDS by a (1, 2) step; the odd number of rows takes the
# (2, 1) step through every i mod 8
LANE_PERIOD = ((1, 2),) * 13 + ((2, 1), (1, 1), (1, 1), (1, 1), (1, 2))


def lanes_and_seams_plot():
    """A path of mixed steps from (3, 32) over two strip seams of the plot (columns 2048, 4096) and of its box (2080, 4128), in sparse noise
    below and right of its start.  Every multiple of 32 is reached by a (1, 2) step from column - 2; the bonus bit of that step, R[i][column - 1]
    -- the left lane's last bit, the left strip's at a seam -- is set at every second landing."""
    rng = np.random.default_rng(44)
    R = np.zeros((2520, 2 * STRIP + 110), np.uint8)
    R[4:, 33:] = rng.random((R.shape[0] - 4, R.shape[1] - 33)) < 0.004
    cells = plant(R, 3, 32, LANE_PERIOD)
    landings = [c for c in cells if c[1] % C == 0 and c[1] > 32]
    for k, (i, j) in enumerate(landings):
        R[i, j - 1] = k & 1
    return R, cells, landings


def test_planted_path_lands_on_every_lane_and_seam_column(ctx):
    """Also the box wider than a strip (three strips of the path pass), and (2, 1) steps at every row phase."""
    R, cells, landings = lanes_and_seams_plot()
    assert len(landings) == (R.shape[1] - 1) // C - 1 and {STRIP, 2 * STRIP, STRIP + 32, 2 * STRIP + 32} <= {c[1] for c in landings}
    for setting in ((0.5, 0.5, 3), (0.5, 0.7, 2)):
        want, wcells, _ = _check_dp(ctx, R, setting, "a path onto every lane's first column")
        got = {tuple(c) for c in wcells}
        assert want[1:3] == (3, 32) and want[4] - want[2] + 1 > 2 * STRIP, want
        steps = {tuple(b): tuple(b - a) for a, b in zip(wcells[:-1], wcells[1:])}
        lim = R.shape[1] - 1 - (setting[2] == 3)
        # (the noise is one in which the reference's path takes every landing: the seed of lanes_and_seams_plot was chosen for it)
        missed = [c for c in landings if c[1] < lim - 2 and not (c in got and steps.get(c) == (1, 2))]
        assert missed == [], "the path lands on every lane's and strip's first column by a (1, 2) step: %s" % missed
        assert {i % 8 for (i, j), d in steps.items() if d == (2, 1)} == set(range(8)), "(2, 1) steps at every row phase"


@pytest.mark.parametrize("r0m", [0, 1, 31, 32, 33, 63])
def test_boxes_whose_start_reads_a_bit_outside_the_box(ctx, r0m):
    """A path of mixed steps planted alone from (q0, r0), and ONE more bit: above the start, R[q0 - 1][r0] (the bonus of c3), or left of it,
    R[q0][r0 - 1] (the bonus of c4).  The start then holds 2, not 1, and every value on the path is one larger: the box pass must read row
    q0 - 1 and column r0 - 1 of the plot.  r0 mod 64 on both sides of a dword and of a bitmap word, q0 mod 8 at both ends of the skew."""
    rng = np.random.default_rng([47, r0m])
    for q0m in (0, 1, 7):
        for side in ("above", "left"):
            q0, r0 = 8 + q0m, 64 + r0m
            R = np.zeros((q0 + 200, r0 + 230), np.uint8)
            cells = plant(R, q0, r0, ((1, 1), (1, 2), (2, 1), (1, 2)), rng, n=110)
            plain = ref.dmax_full(R)[2]
            if side == "above":
                R[q0 - 1, r0] = 1
            else:
                R[q0, r0 - 1] = 1
            for setting in ((0.5, 0.5, 2), (0.5, 0.7, 2), (1.0, 0.25, 3)):
                want, wcells, wq = _check_dp(ctx, R, setting, "planted at (%d, %d), a bit %s the start" % (q0, r0, side))
                assert want[1:3] == (q0, r0) and [tuple(c) for c in wcells] == cells and want[4] - want[2] > 3 * C
                assert wq[0] == 2 and (setting != (0.5, 0.5, 2) or np.array_equal(wq, plain + 1))


def _diag(R, end, L):
    for t in range(L):
        R[end[0] - t, end[1] - t] = 1


def test_ties_between_lanes_and_between_strips(ctx):
    """Two diagonals of equal score: the row-major first END wins -- the earlier row even in a higher lane or a later strip, the smaller
    column in the same row.  (A lone diagonal scores its length under Dmax as under Qmax.)"""
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
            want, wcells, _ = _check_dp(ctx, R, setting, "ties %s %s" % (a, b))
            end = (a, b)[winner]
            assert want == (float(L), end[0] - L + 1, end[1] - L + 1, end[0], end[1]), (a, b, setting, want)


def test_ties_among_the_three_predecessors(ctx):
    """Dense plots: ties among c2, c3, c4 with their bonus bits, and among the penalised values in gap cells."""
    rng = np.random.default_rng(53)
    plots = [np.ones((20, 80), np.uint8), np.ones((70, 9), np.uint8)]
    R = np.ones((24, 70), np.uint8)
    R[::3, ::4] = 0
    plots.append(R)
    R = np.ones((30, 100), np.uint8)
    R[5::2] = 0                                          # every second row empty: (2, 1) steps through gap rows
    plots.append(R)
    for _ in range(4):
        plots.append(ref.random_plot(rng, int(rng.integers(10, 40)), int(rng.integers(40, 130)), 0.85))
    for R in plots:
        for setting in SETTINGS + [(0.0, 0.0, 2)]:
            _check_dp(ctx, R, setting, "ties")


@pytest.mark.parametrize("which", ["column 0", "column 1", "the last column", "columns 0 and 1"])
def test_edge_columns_of_ones(ctx, which):
    """R[i][1] is a bonus of column 2's c4 and R[i][N - 1] of nothing inside the matrix when dp_start is 3: the columns the sweep forces to 0
    must stay 0 and their bits must still count as bonus."""
    rng = np.random.default_rng([59, len(which)])
    for M, N in ((9, 40), (40, 9), (30, 70), (12, STRIP + 1), (12, STRIP + 2)):
        R = ref.random_plot(rng, M, N, 0.3)
        if "0" in which:
            R[:, 0] = 1
        if "1" in which:
            R[:, 1] = 1
        if "last" in which:
            R[:, -1] = 1
        for setting in SETTINGS:
            _check_dp(ctx, R, setting, which + " all ones")


def test_empty_plot_capacity_and_bad_input(ctx):
    from acoss_amd import _lib
    for setting in SETTINGS:
        want, cells, _ = _check_dp(ctx, np.zeros((7, 9), np.uint8), setting, "all zero")
        assert want == ref.NO_MATCH and cells.shape == (0, 2)
        for shape in ((2, 5), (5, 2), (1, 1)):
            assert _check_dp(ctx, np.ones(shape, np.uint8), setting, "smaller than 3 x 3")[0] == ref.NO_MATCH
    R = np.eye(12, 20, dtype=np.uint8)
    with pytest.raises(ValueError, match="dmax_path_binary: cap 11 is too small: 12 cells required"):
        ctx.dmax_path_binary(R, cap=11)
    bad = R.copy()
    bad[3, 3] = 2
    with pytest.raises(ValueError, match="non-binary elements found in input"):
        ctx.dmax_path_binary(bad)
    with pytest.raises(ValueError, match="dmax_locate_binary: non-binary"):
        ctx.dmax_locate_binary(bad)
    # params->dmax is ignored
    rec, cells = ctx.dmax_path_binary(R, _lib.serra09_params(dmax=1), cap=12)
    assert _rec(rec[0]) == (10.0, 2, 2, 11, 11) and cells.tolist() == [[t, t] for t in range(2, 12)]
    assert rec.tobytes() == ctx.dmax_path_binary(R, _lib.serra09_params(dmax=0))[0].tobytes()


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
    """dmax_full of a device plot, computed once per (plot, penalties, dp_start)."""
    key = (R.shape, R.tobytes(), float(p.gamma_o), float(p.gamma_e), int(p.dp_start))
    if key not in _REFS:
        _REFS[key] = ref.dmax_full(R, p.gamma_o, p.gamma_e, p.dp_start)
    return _REFS[key]


def _paths_against_plots(ctx, pairs, tag, **kw):
    """chenfusion_align_paths(plane 1) over `pairs` against the reference on the device's own plots (serra09_debug_bits); the records
    against chenfusion_align's bytes and the scores against chenfusion_pairs' Dmax column."""
    from acoss_amd import _lib
    p = _lib.serra09_params(**kw)
    got, off, cells = ctx.chenfusion_align_paths(pairs, p, plane=1)
    assert got.tobytes() == ctx.chenfusion_align(pairs, p, plane=1).tobytes(), tag
    assert np.array_equal(got["score"].view(np.uint32), ctx.chenfusion_pairs(pairs, p)[:, 1].copy().view(np.uint32)), tag
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
    long_rec = each[-1][0][0]                              # the streaming pair: the last 300 cells of a 2100-cell version of the same work
    assert long_rec["r1"] >= STRIP > long_rec["r0"], "the streaming pair's alignment crosses the strip seam: %s" % (long_rec,)
    mixed = _paths_against_plots(ctx, pairs, "mixed list", m=M9)
    assert np.array_equal(mixed[0], np.concatenate([e[0] for e in each])) and np.array_equal(mixed[2], np.concatenate([e[2] for e in each]))
    rev = _paths_against_plots(ctx, pairs[::-1].copy(), "mixed list reversed", m=M9)
    assert np.array_equal(rev[0], mixed[0][::-1]) and np.array_equal(rev[2], np.concatenate([e[2] for e in each[::-1]]))
    _paths_against_plots(ctx, pairs, "mixed list, gammas (1, 0.25), dp_start 3", m=M9, gamma_o=1.0, gamma_e=0.25, dp_start=3)
    # a stack of 17 frames: every pair streams, however short
    short = np.array([[pool["start"][249], pool["end"][505]]], np.int32)
    _paths_against_plots(ctx, short, "m = 17", m=17)
    # the Dmax alignment is not the Qmax alignment of the same plots
    p = ctx_params(m=M9)
    assert ctx.chenfusion_align(pairs, p, plane=1).tobytes() != ctx.chenfusion_align(pairs, p, plane=0).tobytes()


def ctx_params(**kw):
    from acoss_amd import _lib
    return _lib.serra09_params(**kw)


def test_plane_0_is_the_qmax_alignment_byte_for_byte(ctx, pool):
    ctx.upload_pool(pool["frames"], pool["offsets"])
    pairs = pool["pairs"]
    for kw in (dict(m=M9), dict(m=M9, gamma_o=1.0, gamma_e=0.25, dp_start=3), dict(m=M9, dmax=1)):
        p, q = ctx_params(**kw), ctx_params(**dict(kw, dmax=0))
        assert ctx.chenfusion_align(pairs, p, plane=0).tobytes() == ctx.serra09_align(pairs, q).tobytes()
        a, b = ctx.chenfusion_align_paths(pairs, p, plane=0), ctx.serra09_align_paths(pairs, q)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # params->dmax is ignored for plane 1 as well
    assert ctx.chenfusion_align(pairs, ctx_params(m=M9, dmax=1), plane=1).tobytes() == ctx.chenfusion_align(pairs, ctx_params(m=M9), plane=1).tobytes()


def _launches(ctx, call):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        out = call()
        prof = ctx.profile()
    finally:
        ctx.profile_enable(False)
    return out, prof["dmax_locate_kernel"]["launches"], prof["dmax_path_kernel"]["launches"], prof


def test_batches_chunks_and_the_budget(ctx, pool):
    """Two batches under a scratch limit give the paths of one; under a smaller limit the boxes of a batch run in more than one chunk
    of the direction plane (half the limit); a box beyond that budget is ACX_ERR_NOMEM and the next valid call succeeds."""
    from acoss_amd import _lib
    st, en = pool["start"], pool["end"]
    p = _lib.serra09_params(m=M9)
    lens = np.diff(pool["offsets"])
    ctx.upload_pool(pool["frames"], pool["offsets"])
    pairs = np.array([(st[a], en[b]) for a in (249, 300, 505) for b in (249, 300, 505)] + [(en[300], en[LONG]), (st[LONG], st[300])], np.int32)
    limit = 6 << 20
    assert np.all(_lib.serra09_plan(lens, pairs, p)["batch"] == 0)
    assert _lib.serra09_plan(lens, pairs, p, scratch_limit=limit)["batch"].max() >= 1
    one = _paths_against_plots(ctx, pairs, "one batch", m=M9)
    ctx.set_scratch_limit(limit)
    try:
        two = ctx.chenfusion_align_paths(pairs, p, plane=1)
        assert all(np.array_equal(a, b) for a, b in zip(one, two))
        rev = ctx.chenfusion_align_paths(pairs[::-1].copy(), p, plane=1)
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
        got, nloc, npath, prof = _launches(ctx, lambda: ctx.chenfusion_align_paths(pairs, p, plane=1))
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert nloc == plan["batch"].max() + 1 and npath > nloc, "more chunks (%d) than batches (%d)" % (npath, nloc)
        assert prof["dmax_path_kernel"]["ms"] > 0
        assert all(prof[k]["launches"] == 0 for k in ("qmax_bits_kernel", "qmax_locate_kernel", "qmax_path_kernel"))
        ctx.set_scratch_limit(limit - 16)                  # the largest plane no longer fits half the limit
        with pytest.raises(MemoryError, match="dmax_path: .* beyond the path budget"):
            ctx.chenfusion_align_paths(pairs, p, plane=1)
    finally:
        ctx.set_scratch_limit(0)
    assert all(np.array_equal(a, b) for a, b in zip(ctx.chenfusion_align_paths(pairs, p, plane=1), want))


def test_refused_lists_launch_nothing(ctx, pool):
    """The codes of acx_serra09_align_paths, for the whole list before the first launch; the plane; cap below the bound."""
    from acoss_amd import _lib
    ctx.upload_pool(pool["frames"], pool["offsets"])
    n = len(pool["M"])
    p = _lib.serra09_params(m=M9)
    good = pool["pairs"][:2]
    want = ctx.chenfusion_align_paths(good, p, plane=1)

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
        for call in (lambda b=bad: ctx.chenfusion_align_paths(np.concatenate([good, [b]]), p, plane=1),
                     lambda b=bad: ctx.chenfusion_align(np.concatenate([good, [b]]), p, plane=1)):
            launches_nothing(ValueError, "track index out of range in pair 2", call)
    for plane in (2, -1):
        launches_nothing(ValueError, "chenfusion_align: plane must be 0 \\(qmax\\) or 1 \\(dmax\\)", lambda: ctx.chenfusion_align(good, p, plane=plane))
        launches_nothing(ValueError, "chenfusion_align_paths: plane must be 0", lambda: ctx.chenfusion_align_paths(good, p, plane=plane))
    launches_nothing(_lib.AcxError, "shorter than the delay-embedding stack",
                     lambda: ctx.chenfusion_align_paths(good, _lib.serra09_params(m=30, tau=9), plane=1))
    bound = sum(min(int(pool["M"][i]), int(pool["M"][j])) for i, j in good)
    launches_nothing(ValueError, "chenfusion_align_paths: cap %d is too small: %d cells required" % (bound - 1, bound),
                     lambda: ctx.chenfusion_align_paths(good, p, plane=1, cap=bound - 1))
    got = ctx.chenfusion_align_paths(good, p, plane=1, cap=bound)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_profile_names_the_kernels(ctx, pool):
    """The entries, and -- on the same two pairs -- the Dmax kernels' milliseconds beside the Qmax kernels' (printed)."""
    from acoss_amd import _lib
    ctx.upload_pool(pool["frames"], pool["offsets"])
    p = _lib.serra09_params(m=M9)
    _, nloc, npath, prof = _launches(ctx, lambda: ctx.chenfusion_align_paths(pool["pairs"][:2], p, plane=1))
    names = list(prof)
    assert names[-1] == "ef_align_kernel" and names.index("dmax_locate_kernel") + 1 == names.index("dmax_path_kernel")
    assert (nloc, npath) == (1, 1) and prof["dmax_locate_kernel"]["ms"] > 0 and prof["dmax_path_kernel"]["ms"] > 0
    assert prof["dmax_path_kernel"]["cells"] > 0 and prof["dmax_locate_kernel"]["cells"] > 0
    assert all(prof[k]["launches"] == 0 for k in ("qmax_bits_kernel", "qmax_locate_kernel", "qmax_path_kernel"))
    _, _, _, qprof = _launches(ctx, lambda: ctx.chenfusion_align_paths(pool["pairs"][:2], p, plane=0))
    assert qprof["dmax_locate_kernel"]["launches"] == 0 and qprof["dmax_path_kernel"]["launches"] == 0
    assert qprof["qmax_locate_kernel"]["launches"] == 1 and qprof["qmax_path_kernel"]["launches"] == 1
    print("two pairs: dmax_locate_kernel %.3f ms beside qmax_locate_kernel %.3f ms; dmax_path_kernel %.3f ms beside qmax_path_kernel %.3f ms"
          % (prof["dmax_locate_kernel"]["ms"], qprof["qmax_locate_kernel"]["ms"], prof["dmax_path_kernel"]["ms"], qprof["qmax_path_kernel"]["ms"]))


# ---- ChenFusion.align*(similarity_type=) ------------------------------------------------------------------------------------------------------
def _dataset(tmp_path, tag, n):
    path = tmp_path / ("%s.csv" % tag)
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


def _algo(tmp_path, tag, tracks, cls, **kw):
    a = cls(_dataset(tmp_path, tag, len(tracks)), "feat/", shortname=tag, **kw)
    a.set_pooled_features(tracks, ["w%d" % (i // 2) for i in range(len(tracks))])
    return a


def _close(algo):
    algo._ctx.close()
    algo._ctx = None
    algo.cleanup_memmap()


def test_align_paths_on_the_planted_excerpt(tmp_path, monkeypatch):
    """The planted excerpt of tests/test_gpu_qmax_path.py: B's pooled frames [50, 130) are A's [20, 100).  The spans are printed, not asserted."""
    from acoss_amd import synth
    from acoss_amd.algorithms import ChenFusion, Serra09
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(11)
    A = synth._frame_max_normalise(rng.random((150, 12))).astype(np.float32)
    B = synth._frame_max_normalise(rng.random((200, 12))).astype(np.float32)
    B[50:130] = A[20:100]
    idxs = [[1, 0], [0, 1]]
    chen = _algo(tmp_path, "dmaxexcerpt", [A, B], ChenFusion, oti=False, m=9, tau=1)
    try:
        al, paths = chen.align_paths(idxs, similarity_type="dmax")
        plain = chen.align(idxs, similarity_type="dmax")
        assert al.dtype == plain.dtype == chen.ALIGN_DTYPE and al.tobytes() == plain.tobytes()
        for f in chen.ALIGN_DTYPE.names:
            assert np.array_equal(al[f], plain[f]), f
        _, Rs = chen._context().serra09_debug_bits(np.array(idxs, np.int32), chen._params())
        lens = (len(B), len(A))
        for k, R in enumerate(Rs):
            want, wcells, _ = ref.dmax_full(R)
            assert _rec(al[k]) == want and paths[k].dtype == np.int32 and np.array_equal(paths[k], wcells), k
            assert tuple(al[k]["q_span"]) == (want[1], min(want[3] + 8, lens[k] - 1)) and tuple(al[k]["r_span"]) == (want[2], min(want[4] + 8, lens[1 - k] - 1))
            print("pair %d: dmax %.1f, q_span %s r_span %s, %d path cells" % (k, al[k]["score"], al[k]["q_span"].tolist(), al[k]["r_span"].tolist(), len(paths[k])))
        assert chen.align_paths(np.zeros((0, 2), np.int64), similarity_type="dmax")[1] == []
        # the default is still the Qmax result: Serra09's on the same tracks, and the explicit "qmax"
        qal, qpaths = chen.align_paths(idxs)
        eal, epaths = chen.align_paths(idxs, similarity_type="qmax")
        assert qal.tobytes() == eal.tobytes() == chen.align(idxs).tobytes() and qal.tobytes() != al.tobytes()
        sc = chen._context().chenfusion_pairs(np.array(idxs, np.int32), chen._params())
        assert np.array_equal(qal["score"], sc[:, 0]) and np.array_equal(al["score"], sc[:, 1])
    finally:
        _close(chen)
    ser = _algo(tmp_path, "dmaxexcerpt_s", [A, B], Serra09, oti=False, m=9, tau=1)
    try:
        sal, spaths = ser.align_paths(idxs)
        assert sal.tobytes() == qal.tobytes() and all(np.array_equal(a, b) and np.array_equal(a, c) for a, b, c in zip(spaths, qpaths, epaths))
    finally:
        _close(ser)


def test_align_matches_on_identify_output(tmp_path, monkeypatch):
    from acoss_amd import synth
    from acoss_amd.algorithms import ChenFusion
    monkeypatch.chdir(tmp_path)
    d = synth.cover_set(n_works=6, versions=2, seed=5, t_range=(60, 120))
    n = len(d["offsets"]) - 1
    algo = _algo(tmp_path, "dmaxmatches", [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for i in range(n)], ChenFusion)
    try:
        queries = [0, 7, 3, 7]
        idx, _ = algo.identify(queries, k=12)["dmax"]      # eleven candidates: the last slot of every row is empty
        assert idx.shape == (4, 12) and np.all(idx[:, -1] == -1) and np.all(idx[:, :-1] >= 0)
        got, paths = algo.align_match_paths(queries, idx, similarity_type="dmax")
        assert got.tobytes() == algo.align_matches(queries, idx, similarity_type="dmax").tobytes()
        assert got.tobytes() != algo.align_matches(queries, idx).tobytes(), "the default is the Qmax alignment"
        assert len(paths) == 4 and all(len(row) == 12 for row in paths)
        for i, q in enumerate(queries):
            assert got[i, -1]["q0"] == -1 and paths[i][-1].shape == (0, 2) and paths[i][-1].dtype == np.int32, "an empty slot: a no-match row, an empty path"
            row_al, row_paths = algo.align_paths([[q, j] for j in idx[i, :-1]], similarity_type="dmax")
            assert np.array_equal(got[i, :-1], row_al)
            for s in range(11):
                assert np.array_equal(paths[i][s], row_paths[s]), (i, s)
        _, Rs = algo._context().serra09_debug_bits(np.array([[queries[0], j] for j in idx[0, :-1]], np.int32), algo._params())
        for s, R in enumerate(Rs):
            want, wcells, _ = ref.dmax_full(R)
            assert _rec(got[0, s]) == want and np.array_equal(paths[0][s], wcells), s
    finally:
        _close(algo)
