"""
GPU tests (run with -m gpu on a real MI355X): EVERY matched section of a pair -- qmax_sections_kernel<EQG>
(acoss_amd/csrc/serra09_sections_kernels.hpp) through acx_qmax_sections_binary (the DP alone on a given plot) and
acx_serra09_align_sections (the product chain), Serra09.align_sections and Serra09.align_match_sections.

Every comparison is exact: the records, their number, the offsets and every cell against the full-masked-matrix restatement of the
contract (tests/_qmax_sections_ref.py sections_full; tests/test_qmax_sections_ref.py holds it against the sweep per free interval),
and section 0 against the locating sweep's bytes on the same arguments.

The kernel sweeps one free interval of rows at a time from two zero register rows: an interval begins at any row -- either parity
of the unrolled row pair, any phase of the bitmap's skew (row & 7) -- and the strip seam records cover the swept rows only.
"""
import numpy as np
import pytest

from tests import _qmax_sections_ref as ref
from tests import _serra09_shapes as S

pytestmark = pytest.mark.gpu

STRIP = 2048
GAMMAS = ((0.5, 0.5), (1.0, 0.25), (0.25, 1.0))          # gamma_o == gamma_e: qmax_sections_kernel<true>; the others <false>
SETTINGS = [(go, ge, st) for st in (2, 3) for go, ge in GAMMAS]
FIELDS = ("score", "q0", "r0", "q1", "r1")
NO_MATCH = (0.0, -1, -1, -1, -1)


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _rec(a):
    return (float(a["score"]),) + tuple(int(a[f]) for f in FIELDS[1:])


def _opts(**kw):
    from acoss_amd import _lib
    return _lib.section_opts("test", **kw)


def _compare(label, S_, got, n, off, cells, want, wpaths):
    """One pair's device result -- S_ records, their number, S_ + 1 offsets (relative to off[0]) and the cells -- against (a)."""
    recs = [_rec(got[s]) for s in range(S_)]
    assert n == len(want), "%s: %d sections %s, reference %d %s" % (label, n, recs[:n], len(want), want)
    assert recs[:n] == want, "%s: device %s, reference %s" % (label, recs[:n], want)
    assert all(r == NO_MATCH for r in recs[n:]), "%s: the no-match record behind the count: %s" % (label, recs[n:])
    if off is None:
        return
    for s in range(S_):
        mine = cells[off[s]:off[s + 1]]
        if s >= n:
            assert len(mine) == 0, label
        elif not np.array_equal(mine, wpaths[s]):
            raise AssertionError("%s: section %d has %d cells %s ..., reference %d %s ..." % (
                label, s, len(mine), mine[:3].tolist(), len(wpaths[s]), wpaths[s][:3].tolist()))


def _check_dp(ctx, R, setting, tag, **okw):
    """qmax_sections_binary on R against sections_full; section 0 against qmax_locate_binary's bytes.  Returns the reference."""
    from acoss_amd import _lib
    go, ge, st = setting
    p = _lib.serra09_params(gamma_o=go, gamma_e=ge, dp_start=st)
    o = _opts(**okw)
    got, n, off, cells = ctx.qmax_sections_binary(R, p, o)
    S_ = o.max_sections
    assert got.shape == (S_,) and got.dtype == _lib.ALIGNMENT_DTYPE and off.shape == (S_ + 1,) and off[0] == 0
    assert cells.dtype == np.int32 and cells.shape == (off[-1], 2)
    want, wpaths = ref.sections_full(R, go, ge, st, **okw)
    label = "%s, %s plot, gammas (%s, %s), dp_start %d, %s" % (tag, R.shape, go, ge, st, okw)
    _compare(label, S_, got, n, off, cells, want, wpaths)
    first = ctx.qmax_locate_binary(R, p)
    if first[0]["score"] >= o.min_score:
        assert n >= 1 and got[:1].tobytes() == first.tobytes(), label
    else:
        assert n == 0, label
    bare, nb = ctx.qmax_sections_binary(R, p, o, paths=False)
    assert nb == n and bare.tobytes() == got.tobytes(), label
    return want, wpaths


def plant(R, i, j, steps, n):
    """Ones along a path of n cells from (i, j), `steps` taken in turn (cyclically).  Returns the cells."""
    cells = []
    for t in range(n):
        R[i, j] = 1
        cells.append((i, j))
        i, j = i + steps[t % len(steps)][0], j + steps[t % len(steps)][1]
    return cells


MIXED = ((1, 1), (1, 2), (2, 1), (1, 2))


# ---- the DP alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.HAND, ids=[h[0] for h in ref.HAND])
def test_hand_checked_plots(ctx, case):
    name, R, okw, want = case
    got, _ = _check_dp(ctx, R, (0.5, 0.5, 2), name, **okw)
    assert got == want, name
    _check_dp(ctx, R, (1.0, 0.25, 3), name, **okw)


@pytest.mark.parametrize("N", [3, 33, 64, 2047, 2049, 4097])
def test_random_plots(ctx, N):
    """N x M of the issue's grid, every setting (both EQG instantiations, both dp_start).  Per N, max_sections steps with the plot
    and the setting, pad with the plot: every setting meets max_sections 1, 2 and 16 (three of the four M are distinct mod 3), and
    every pad meets both instantiations."""
    rng = np.random.default_rng([28, N])
    total = 0
    for mi, M in enumerate((5, 9, 64, 130)):
        R = (rng.random((M, N)) < (0.05, 0.3, 0.6)[(M + N) % 3]).astype(np.uint8)
        for si, setting in enumerate(SETTINGS):
            want, _ = _check_dp(ctx, R, setting, "random plot", max_sections=(1, 2, 16)[(mi + si // 3 + si) % 3],
                                pad=(0, 1, 5)[(mi + si // 3) % 3], min_score=(1.5, 2.0)[(mi + si) % 2])
            total += len(want)
    print("N = %d: %d sections in 24 calls" % (N, total))


def test_intervals_begin_and_end_on_every_row_phase(ctx):
    """Section 0 planted at rows q0 .. q1 with q0 & 7 and q1 & 7 taking every value (both parities of either): the interval above ends
    at q0 - pad - 1, the one below begins at q1 + pad + 1, and each holds a shorter planted section the sweep has to find."""
    t = 0
    for q0m in range(8):
        for q1m in range(8):
            q0 = 24 + q0m
            L = 24 + (q1m - (q0 + 23)) % 8          # rows q0 .. q0 + L - 1, (q0 + L - 1) & 7 == q1m
            q1 = q0 + L - 1
            assert q1 & 7 == q1m and 24 <= L < 32
            pad = t % 3
            R = np.zeros((q1 + 40, 200), np.uint8)
            plant(R, q0, 100, ((1, 1),), L)
            above = plant(R, 3, 20, MIXED, 12)      # rows 3 .. : ends below q0 - pad
            below = plant(R, q1 + pad + 1, 40, MIXED, 14)
            assert above[-1][0] < q0 - pad and below[-1][0] < R.shape[0]
            want, _ = _check_dp(ctx, R, SETTINGS[t % 6], "phases (%d, %d)" % (q0m, q1m), max_sections=4, pad=pad, min_score=3.0)
            if SETTINGS[t % 6][2] == 2:
                assert len(want) == 3 and want[0][1] == q0 and want[0][3] == q1 and {w[1] for w in want[1:]} == {3, q1 + pad + 1}, want
            t += 1


def test_interval_from_dp_row_2_to_the_last_row(ctx):
    """Section 0 in the middle; the interval above begins at row 0 -- its DP at row 2, where a section starts -- and the one below ends
    at the plot's last row, where a section ends."""
    M = 61
    R = np.zeros((M, 90), np.uint8)
    plant(R, 20, 30, ((1, 1),), 20)                 # rows 20 .. 39
    plant(R, 2, 60, ((1, 1),), 10)                  # rows 2 .. 11 (each diagonal LEFT of the one above it: out of its decaying tail)
    plant(R, M - 12, 5, ((1, 1),), 12)              # rows 49 .. 60
    want, _ = _check_dp(ctx, R, (0.5, 0.5, 2), "row 2 and the last row", max_sections=3)
    assert want == [(20.0, 20, 30, 39, 49), (12.0, 49, 5, 60, 16), (10.0, 2, 60, 11, 69)]
    want, _ = _check_dp(ctx, R, (1.0, 0.25, 3), "row 2 and the last row", max_sections=3)
    assert want == [(20.0, 20, 30, 39, 49), (11.0, 49, 5, 59, 15), (10.0, 2, 60, 11, 69)], "dp_start 3 never reads the last row"


def test_sections_across_the_strip_seam(ctx):
    """A plot of 2300 columns: section 0 lies left of the seam at column 2048; the two intervals it splits each hold a section whose
    alignment crosses the seam, one of them through a missing cell (the penalised values of the seam records)."""
    R = np.zeros((200, 2300), np.uint8)
    plant(R, 60, 100, ((1, 1),), 60)                # rows 60 .. 119
    up = plant(R, 5, 2030, MIXED, 36)
    down = plant(R, 125, 2020, ((1, 1),), 50)
    R[125 + 27, 2047] = 0                           # the cell left of the seam is missing: the diagonal goes on through a gap cell
    assert up[-1][0] < 60 and up[0][1] < STRIP < up[-1][1] and down[-1][0] < 200 and down[-1][1] > STRIP
    for setting in ((0.5, 0.5, 2), (1.0, 0.25, 2), (0.25, 1.0, 3)):
        want, wpaths = _check_dp(ctx, R, setting, "seam", max_sections=3, min_score=5.0)
        assert len(want) == 3 and want[0][1:] == (60, 100, 119, 159)
        for w in want[1:]:
            assert w[2] < STRIP < w[4], "the section crosses the seam: %s" % (w,)
        assert any(R[tuple(c)] == 0 for c in wpaths[1]) or any(R[tuple(c)] == 0 for c in wpaths[2]), "a path runs through the missing cell"


def test_abutting_sections(ctx):
    R = np.zeros((70, 120), np.uint8)
    plant(R, 10, 10, ((1, 1),), 20)                 # rows 10 .. 29
    plant(R, 30, 70, ((1, 1),), 15)                 # rows 30 .. 44: begins in the row behind the first one's end
    for setting in SETTINGS:
        want, _ = _check_dp(ctx, R, setting, "abutting", max_sections=4)
        assert want == [(20.0, 10, 10, 29, 29), (15.0, 30, 70, 44, 84)]
        assert want[1][1] == want[0][3] + 1


def test_ties_between_intervals_in_shuffled_bands(ctx):
    """Six diagonals of 9, 7, 7, 5, 5, 5 cells, one per band of 14 rows, the lengths shuffled over the bands (each diagonal LEFT of
    the ones above it): equal lengths in different free intervals tie, and the slot order of the intervals is whatever the earlier
    splits left.  The reference side counts the rounds in which interval records tie and those won by a slot that is not the lowest
    of the tied ones -- where a rule by slot order would answer differently."""
    rng = np.random.default_rng(41)
    tied, by_row = 0, 0
    for t in range(12):
        lengths = rng.permutation([9, 7, 7, 5, 5, 5])
        R = ref.ones((6 * 14 + 4, 6 * 12 + 4), [(3 + 14 * b, 2 + 12 * (5 - b), int(n)) for b, n in enumerate(lengths)])
        setting = SETTINGS[t % 6]
        want, _ = _check_dp(ctx, R, setting, "shuffled bands %s" % lengths.tolist(), max_sections=6, min_score=3.0)
        assert [w[0] for w in want] == [9.0, 7.0, 7.0, 5.0, 5.0, 5.0] and [w[1] for w in want[1:3]] == sorted(w[1] for w in want[1:3])
        ties = []
        ref.sections_intervals(R, *setting, max_sections=6, min_score=3.0, ties=ties)
        tied += sum(len(slots) > 1 for slots, _ in ties)
        by_row += sum(len(slots) > 1 and pick != min(slots) for slots, pick in ties)
    print("%d rounds with tied interval records, %d of them won by a higher slot" % (tied, by_row))
    assert tied >= 12 and by_row >= 3


def test_sixteen_sections_fill_the_cap_and_a_seventeenth_exists(ctx):
    """17 diagonals of 22, 21, .. 6 cells, each in rows and columns of its own and LEFT of the earlier ones (the values that decay
    behind a diagonal's end spread down and to the right only): max_sections = 16 reports the first 16, and the 17th is a section
    where it may be -- the plot below the 16th holds it."""
    R = np.zeros((17 * 24 + 4, 17 * 24 + 8), np.uint8)
    for k in range(17):
        plant(R, 2 + 24 * k, 4 + 24 * (16 - k), ((1, 1),), 22 - k)
    for setting in ((0.5, 0.5, 2), (0.25, 1.0, 2)):
        want, _ = _check_dp(ctx, R, setting, "17 diagonals", max_sections=16, min_score=3.0)
        assert [w[0] for w in want] == [float(22 - k) for k in range(16)] and [w[1] for w in want] == [2 + 24 * k for k in range(16)]
    assert ref.sections_full(R[24 * 16:], min_score=3.0)[0] == [(6.0, 2, 4, 7, 9)], "the 17th candidate"


def test_score_equal_to_the_threshold(ctx):
    for okw, n in ((dict(min_score=9.0), 2), (dict(min_score=9.5), 1), (dict(min_ratio=0.75), 2), (dict(min_ratio=0.76), 1),
                   (dict(min_score=12.0), 1), (dict(min_score=12.5), 0)):
        want, _ = _check_dp(ctx, ref.THREE, (0.5, 0.5, 2), "threshold", max_sections=4, **okw)
        assert len(want) == n, (okw, want)


def _launches_nothing(ctx, exc, match, call):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        with pytest.raises(exc, match=match):
            call()
        prof = ctx.profile()
    finally:
        ctx.profile_enable(False)
    assert sum(v["launches"] for v in prof.values()) == 0, {k: v["launches"] for k, v in prof.items() if v["launches"]}


def _raw_opts(max_sections=4, pad=0, min_score=2.0, min_ratio=0.0):
    from acoss_amd import _lib
    return _lib.SectionOpts(max_sections, pad, min_score, min_ratio)


BAD_OPTS = [(dict(max_sections=0), "max_sections"), (dict(max_sections=17), "max_sections"), (dict(pad=-1), "pad"),
            (dict(min_score=1.0), "min_score"), (dict(min_score=float("nan")), "min_score"), (dict(min_ratio=-0.5), "min_ratio"),
            (dict(min_ratio=1.25), "min_ratio"), (dict(min_ratio=float("nan")), "min_ratio")]


def test_empty_plot_capacity_and_refused_options(ctx):
    from acoss_amd import _lib
    for setting in SETTINGS:
        assert _check_dp(ctx, np.zeros((7, 9), np.uint8), setting, "all zero", max_sections=3)[0] == []
        for shape in ((2, 5), (5, 2), (1, 1), (3, 3)):
            assert _check_dp(ctx, np.ones(shape, np.uint8), setting, "too small", min_score=1.5)[0] == []
    R = ref.THREE                                    # 60 x 120: min(M, 4 * min(M, N)) = 60, min(M, 1 * 60) = 60
    _launches_nothing(ctx, ValueError, "cap 59 is too small: 60 cells required", lambda: ctx.qmax_sections_binary(R, cap=59))
    got = ctx.qmax_sections_binary(R, cap=60)
    assert got[1] == 3 and got[2].tolist() == [0, 12, 21, 27, 27]
    T = np.ascontiguousarray(R.T)                    # 120 x 60: min(120, 1 * 60) = 60, min(120, 4 * 60) = 120
    _launches_nothing(ctx, ValueError, "cap 119 is too small: 120 cells required", lambda: ctx.qmax_sections_binary(T, cap=119))
    _launches_nothing(ctx, ValueError, "cap 59 is too small: 60 cells required",
                      lambda: ctx.qmax_sections_binary(T, opts=_opts(max_sections=1), cap=59))
    for bad, what in BAD_OPTS:
        _launches_nothing(ctx, ValueError, "qmax_sections_binary: %s" % what, lambda: ctx.qmax_sections_binary(R, opts=_raw_opts(**bad)))
    _launches_nothing(ctx, NotImplementedError, "Qmax alignment only", lambda: ctx.qmax_sections_binary(R, _lib.serra09_params(dmax=1)))
    bad = R.copy()
    bad[3, 3] = 2
    with pytest.raises(ValueError, match="non-binary"):
        ctx.qmax_sections_binary(bad)
    assert ctx.qmax_sections_binary(R)[1] == 3


# ---- the product path -----------------------------------------------------------------------------------------------------------------------
M9 = 9
LONG = 2100                    # cells: beyond the last band class (2041), the streaming kernels
SIDES = S.UPPER + (300, LONG)


@pytest.fixture(scope="module")
def pool():
    """The pool of tests/test_gpu_qmax_path.py: two versions (the start and the end of one work) of a track at the upper edge of every
    band size class, of 300 and of 2100 cells."""
    rng = np.random.default_rng([9, 16])
    tracks, Ms, start, end, _ = S._two_ends(rng, SIDES, M9, 1)
    d = S._pack(tracks, Ms, [(start[a], end[a]) for a in S.UPPER] + [(end[300], end[LONG])], start=start, end=end)
    for c, a in enumerate(S.UPPER):                        # one pair per band class, at the class edge as the plan reports it
        assert S.key(a, a, M9) == (c, c) and S.cls(a + 1, M9) == c + 1
    assert S.key(300, LONG, M9) == (S.NC, S.NC)
    return d


_REFS = {}


def _reference(R, p, okw):
    """sections_full of a device plot, computed once per (plot, penalties, dp_start, options)."""
    key = (R.shape, R.tobytes(), float(p.gamma_o), float(p.gamma_e), int(p.dp_start), tuple(sorted(okw.items())))
    if key not in _REFS:
        _REFS[key] = ref.sections_full(R, p.gamma_o, p.gamma_e, p.dp_start, **okw)
    return _REFS[key]


OKW = dict(max_sections=3, min_score=3.0, pad=2)


def _sections_against_plots(ctx, pairs, tag, okw=OKW, **kw):
    """serra09_align_sections over `pairs` against the reference on the device's own plots (serra09_debug_bits); section 0 against
    serra09_align's bytes; max_sections = 1 against serra09_align; the call without paths against the one with."""
    from acoss_amd import _lib
    p = _lib.serra09_params(**kw)
    o = _opts(**okw)
    S_ = o.max_sections
    got, n, off, cells = ctx.serra09_align_sections(pairs, p, o, paths=True)
    assert got.shape == (len(pairs), S_) and n.shape == (len(pairs),) and off.shape == (len(pairs) * S_ + 1,) and off[0] == 0
    assert cells.shape == (off[-1], 2)
    bare, nb = ctx.serra09_align_sections(pairs, p, o)
    assert bare.tobytes() == got.tobytes() and np.array_equal(nb, n), tag
    al = ctx.serra09_align(pairs, p)
    one, n1 = ctx.serra09_align_sections(pairs, p, _opts(max_sections=1, min_score=okw.get("min_score", 2.0)))
    _, Rs = ctx.serra09_debug_bits(pairs, p)
    for k, R in enumerate(Rs):
        want, wpaths = _reference(R, p, okw)
        label = "%s pair %d %s, %s plot" % (tag, k, tuple(pairs[k]), R.shape)
        o_k = off[k * S_:(k + 1) * S_ + 1]
        _compare(label, S_, got[k], int(n[k]), o_k, cells, want, wpaths)
        if al[k]["score"] >= o.min_score:
            assert n[k] >= 1 and got[k, :1].tobytes() == al[k:k + 1].tobytes() == one[k].tobytes() and n1[k] == 1, label
        else:
            assert n[k] == 0 and n1[k] == 0 and _rec(one[k, 0]) == NO_MATCH, label
    return got, n, off, cells


def test_one_pair_per_class_streaming_and_mixed(ctx, pool):
    ctx.upload_pool(pool["frames"], pool["offsets"])
    pairs = pool["pairs"]
    each = [_sections_against_plots(ctx, pairs[k:k + 1], "class %d alone" % k, m=M9) for k in range(len(pairs))]
    print("sections per pair: %s" % [int(e[1][0]) for e in each])
    assert all(e[1][0] >= 1 for e in each)
    mixed = _sections_against_plots(ctx, pairs, "mixed list", m=M9)
    assert np.array_equal(mixed[0], np.concatenate([e[0] for e in each])) and np.array_equal(mixed[3], np.concatenate([e[3] for e in each]))
    rev = _sections_against_plots(ctx, pairs[::-1].copy(), "mixed list reversed", m=M9)
    assert np.array_equal(rev[0], mixed[0][::-1]) and np.array_equal(rev[1], mixed[1][::-1])
    assert np.array_equal(rev[3], np.concatenate([e[3] for e in each[::-1]]))


def test_other_penalties_and_a_long_stack(ctx, pool):
    ctx.upload_pool(pool["frames"], pool["offsets"])
    pairs = pool["pairs"][[0, 1, 5]]
    _sections_against_plots(ctx, pairs, "gammas (1, 0.25), dp_start 3", m=M9, gamma_o=1.0, gamma_e=0.25, dp_start=3)
    # a stack of 17 frames: every pair streams, however short
    short = np.array([[pool["start"][249], pool["end"][505]]], np.int32)
    _sections_against_plots(ctx, short, "m = 17", m=17)


def _profiled(ctx, call):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        out = call()
        prof = ctx.profile()
    finally:
        ctx.profile_enable(False)
    return out, prof


def test_two_batches_under_a_scratch_limit(ctx, pool):
    from acoss_amd import _lib
    st, en = pool["start"], pool["end"]
    p = _lib.serra09_params(m=M9)
    o = _opts(**OKW)
    lens = np.diff(pool["offsets"])
    ctx.upload_pool(pool["frames"], pool["offsets"])
    pairs = np.array([(st[a], en[b]) for a in (249, 300, 505) for b in (249, 300, 505)] + [(en[300], en[LONG]), (st[LONG], st[300])], np.int32)
    limit = 6 << 20
    assert np.all(_lib.serra09_plan(lens, pairs, p)["batch"] == 0)
    nbatch = int(_lib.serra09_plan(lens, pairs, p, scratch_limit=limit)["batch"].max()) + 1
    assert nbatch >= 2
    one, prof = _profiled(ctx, lambda: _sections_against_plots(ctx, pairs, "one batch", m=M9))
    assert prof["qmax_sections_kernel"]["launches"] == 3 and prof["qmax_sections_kernel"]["ms"] > 0      # (with paths, without, max_sections 1)
    ctx.set_scratch_limit(limit)
    try:
        two, prof = _profiled(ctx, lambda: ctx.serra09_align_sections(pairs, p, o, paths=True))
        assert all(np.array_equal(a, b) for a, b in zip(one, two))
        assert prof["qmax_sections_kernel"]["launches"] == nbatch, "ONE launch per batch"
        assert prof["qmax_locate_kernel"]["launches"] == 0 and prof["qmax_bits_kernel"]["launches"] == 0
        rev = ctx.serra09_align_sections(pairs[::-1].copy(), p, o, paths=True)
        assert np.array_equal(rev[0], one[0][::-1]) and np.array_equal(rev[1], one[1][::-1]) and rev[2][-1] == one[2][-1]
    finally:
        ctx.set_scratch_limit(0)


def test_refused_lists_launch_nothing(ctx, pool):
    from acoss_amd import _lib
    ctx.upload_pool(pool["frames"], pool["offsets"])
    n = len(pool["M"])
    p = _lib.serra09_params(m=M9)
    o = _opts(**OKW)
    good = pool["pairs"][:2]
    want = ctx.serra09_align_sections(good, p, o, paths=True)
    for bad in ([n, 0], [0, -1]):
        _launches_nothing(ctx, ValueError, "track index out of range in pair 2",
                          lambda: ctx.serra09_align_sections(np.concatenate([good, [bad]]), p, o, paths=True))
        _launches_nothing(ctx, ValueError, "track index out of range in pair 2", lambda: ctx.serra09_align_sections(np.concatenate([good, [bad]]), p, o))
    _launches_nothing(ctx, NotImplementedError, "Qmax alignment only", lambda: ctx.serra09_align_sections(good, _lib.serra09_params(m=M9, dmax=1), o))
    _launches_nothing(ctx, _lib.AcxError, "shorter than the delay-embedding stack",
                      lambda: ctx.serra09_align_sections(good, _lib.serra09_params(m=30, tau=9), o))
    for bad, what in BAD_OPTS:
        _launches_nothing(ctx, ValueError, "serra09_align_sections: %s" % what, lambda: ctx.serra09_align_sections(good, p, _raw_opts(**bad)))
    Ms = [(int(pool["M"][i]), int(pool["M"][j])) for i, j in good]
    bound = sum(min(a, 3 * min(a, b)) for a, b in Ms)
    _launches_nothing(ctx, ValueError, "cap %d is too small: %d cells required" % (bound - 1, bound),
                      lambda: ctx.serra09_align_sections(good, p, o, paths=True, cap=bound - 1))
    got = ctx.serra09_align_sections(good, p, o, paths=True, cap=bound)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- Serra09.align_sections / align_match_sections ------------------------------------------------------------------------------------------
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
    if algo._ctx is not None:
        algo._ctx.close()
        algo._ctx = None
    algo.cleanup_memmap()


def _rows_disjoint(sec):
    rows = sorted((int(a["q0"]), int(a["q1"])) for a in sec)
    return all(a[1] < b[0] for a, b in zip(rows, rows[1:]))


def test_align_sections_on_the_planted_recording(tmp_path, monkeypatch):
    """Track B = A[100:180] followed by A[20:100] (pooled frames), m = 9, tau = 1, oti off: for (B, A) the embedded frames 0 .. 71 of B
    are A's 100 .. 171 (diagonal r - q = 100) and B's 80 .. 151 are A's 20 .. 91 (r - q = -60).  Asserted is structure only -- at
    least two sections, disjoint rows, fields and paths against the reference on the device's plot --; the spans and the share of
    path cells on each planted diagonal are printed: what chance recurrences add is not known in advance."""
    from acoss_amd import synth
    from acoss_amd.algorithms import ChenFusion
    monkeypatch.chdir(tmp_path)
    rng = np.random.default_rng(11)
    A = synth._frame_max_normalise(rng.random((200, 12))).astype(np.float32)
    B = np.concatenate([A[100:180], A[20:100]]).astype(np.float32)
    idxs = [[1, 0], [0, 1]]
    algo = _serra09(tmp_path, "secplanted", [A, B], oti=False, m=9, tau=1)
    try:
        sections, paths = algo.align_sections(idxs, max_sections=4, min_score=5.0, pad=2, paths=True)
        plain = algo.align_sections(idxs, max_sections=4, min_score=5.0, pad=2)
        al = algo.align(idxs)
        _, Rs = algo._context().serra09_debug_bits(np.array(idxs, np.int32), algo._params())
        assert len(sections) == len(paths) == len(plain) == 2
        for k, R in enumerate(Rs):
            sec = sections[k]
            assert sec.dtype == algo.ALIGN_DTYPE and sec.tobytes() == plain[k].tobytes() and len(paths[k]) == len(sec)
            assert len(sec) >= 2 and _rows_disjoint(sec), sec
            assert sec[:1].tobytes() == al[k:k + 1].tobytes(), "section 0 is align()'s row"
            want, wpaths = ref.sections_full(R, max_sections=4, min_score=5.0, pad=2)
            assert [_rec(a) for a in sec] == want and all(np.array_equal(a, b) for a, b in zip(paths[k], wpaths))
            T = (len(B), len(A)) if k == 0 else (len(A), len(B))
            for a in sec:
                assert tuple(a["q_span"]) == (a["q0"], min(a["q1"] + 8, T[0] - 1)) and tuple(a["r_span"]) == (a["r0"], min(a["r1"] + 8, T[1] - 1))
            for s, (a, cells) in enumerate(zip(sec, paths[k])):
                d = cells[:, 1] - cells[:, 0] if k == 0 else cells[:, 0] - cells[:, 1]
                print("pair %d section %d: score %.1f, query span %s, reference span %s, %d cells, %d on r - q = 100, %d on r - q = -60" % (
                    k, s, a["score"], a["q_span"].tolist(), a["r_span"].tolist(), len(cells), int(np.sum(d == 100)), int(np.sum(d == -60))))
        assert algo.align_sections(np.zeros((0, 2), np.int64)) == [] and algo.align_sections(np.zeros((0, 2), np.int64), paths=True) == ([], [])
        first = algo.align_sections(idxs, max_sections=1, min_score=5.0)
        assert all(f.tobytes() == al[k:k + 1].tobytes() for k, f in enumerate(first)), "max_sections = 1 is align()"
    finally:
        _close(algo)
    chen = _serra09(tmp_path, "secchen", [A, B], cls=ChenFusion, oti=False, m=9, tau=1)
    try:
        csec, cpaths = chen.align_sections(idxs, max_sections=4, min_score=5.0, pad=2, paths=True, similarity_type="qmax")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(csec, sections))
        assert all(np.array_equal(x, y) for a, b in zip(cpaths, paths) for x, y in zip(a, b))
        with pytest.raises(ValueError, match="align_sections: .*dmax"):
            chen.align_sections(idxs, similarity_type="dmax")
    finally:
        _close(chen)


def test_align_match_sections_on_identify_output_and_in_a_session(tmp_path, monkeypatch):
    from acoss_amd import synth
    monkeypatch.chdir(tmp_path)
    d = synth.cover_set(n_works=4, versions=2, seed=5, t_range=(60, 120))
    n = len(d["offsets"]) - 1
    tracks = [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for i in range(n)]
    algo = _serra09(tmp_path, "secmatches", tracks[:n - 2])
    whole = _serra09(tmp_path, "secwhole", tracks)
    try:
        queries = [0, 5, 3]
        idx, _ = algo.identify(queries, k=7)["main"]       # five candidates: the last two slots of every row are empty
        assert idx.shape == (3, 7) and np.all(idx[:, -2:] == -1) and np.all(idx[:, :-2] >= 0)
        got, paths = algo.align_match_sections(queries, idx, max_sections=3, min_score=3.0, paths=True)
        bare = algo.align_match_sections(queries, idx, max_sections=3, min_score=3.0)
        assert len(got) == len(paths) == 3 and all(len(row) == 7 for row in got) and all(len(row) == 7 for row in paths)
        for i, q in enumerate(queries):
            for s in (5, 6):
                assert got[i][s].shape == (0,) and got[i][s].dtype == algo.ALIGN_DTYPE and paths[i][s] == [], "an empty slot"
            row, row_paths = algo.align_sections([[q, j] for j in idx[i, :5]], max_sections=3, min_score=3.0, paths=True)
            for s in range(5):
                assert got[i][s].tobytes() == row[s].tobytes() == bare[i][s].tobytes() and _rows_disjoint(got[i][s])
                assert len(paths[i][s]) == len(row_paths[s]) and all(np.array_equal(a, b) for a, b in zip(paths[i][s], row_paths[s]))
        # inside appended() the indices run over N + Q: the same sections as on an object that holds all the tracks
        pairs = [[0, n - 2], [n - 1, 1], [n - 2, n - 1]]
        want, wpaths = whole.align_sections(pairs, max_sections=3, min_score=3.0, pad=1, paths=True)
        with pytest.raises(ValueError, match="align_sections: idxs must be track indices in \\[0, %d\\)" % (n - 2)):
            algo.align_sections(pairs)
        with algo.appended(tracks[n - 2:]) as s:
            assert s.total == n
            inside, ipaths = algo.align_sections(pairs, max_sections=3, min_score=3.0, pad=1, paths=True)
            m_in = algo.align_match_sections([n - 1], [[0, -1, n - 2]], max_sections=3, min_score=3.0, pad=1)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(inside, want))
        assert all(np.array_equal(x, y) for a, b in zip(ipaths, wpaths) for x, y in zip(a, b))
        m_want = whole.align_sections([[n - 1, 0], [n - 1, n - 2]], max_sections=3, min_score=3.0, pad=1)
        assert m_in[0][0].tobytes() == m_want[0].tobytes() and len(m_in[0][1]) == 0 and m_in[0][2].tobytes() == m_want[1].tobytes()
    finally:
        _close(algo)
        _close(whole)
