"""
GPU tests (run with -m gpu on a real MI355X) of the product-path tail of the wide band kernel: band_kernel<M, 8, role, false, 0,
FAST> (acoss_amd/csrc/serra09_kernels.hpp), the copy of the row tail in which everything the host knows about a pass is a constant
(serra09_fast_tail, serra09_plan.hpp, decides per launch).  Every case runs the product call through acx_serra09_debug_bits and
compares the recurrence plots its kernels wrote and the scores with the CPU oracle, bit for bit (np.array_equal, no tolerance);
acx_serra09_pairs must return the same scores.  The debug entry point acx_serra09_debug_pair wants eps and D2 and therefore runs the
generic copy: it serves as the "must not take FAST" case that also compares the thresholds.

The wide class depends on the cells per row of a PASS, so a pair needs one long track only: a short track against a long one gives
the wide class in the row pass alone (rows = query frames, Mr cells each), the swapped pair in the column pass alone, and the oracle
stays cheap.  Which launches take the FAST copy is worked out from the plan's predicate and compared with what the launcher did
(acx_serra09_fast_tail_launches counts the FAST launches of the process): a dispatch that never, or always, took the copy fails here.

Forced cold exits: for every such case the test asserts FROM THE REFERENCE ALONE (the oracle's distances) that the condition occurs:
rows whose two order statistics around the percentile position are tied, rows with more than 64 cells tied at that rank (the
selection's candidate list overflows), rows inside the snap's relative gap of 2^-12, and all-zero rows.
"""
import numpy as np
import pytest

from tests import _serra09_shapes as S
from tests._serra09_compare import compare_pair

pytestmark = pytest.mark.gpu

M = 9                       # stack size: a track of T frames has T - 9 embedded frames
KAPPA = 0.095


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _iid(rng, T):
    from acoss_amd import synth
    return synth._frame_max_normalise(rng.random((T, 12)))


def _set(tracks, pairs):
    from acoss_amd import synth
    frames, offsets = synth.pack(tracks)
    return dict(frames=frames, offsets=offsets, pairs=np.ascontiguousarray(pairs, np.int32).reshape(-1, 2),
                M=np.array([S._embed_len(len(t), M) for t in tracks], np.int64))


def _fast(d, k, params=None):
    """(row pass, column pass) of pair k alone: does its launch take the FAST copy?"""
    from acoss_amd import _lib
    i, j = d["pairs"][k]
    return (_lib.serra09_fast_tail(int(d["M"][j]), 0, params), _lib.serra09_fast_tail(int(d["M"][i]), 1, params))


def _fast_runs(flags):
    """FAST launches of one band pass whose pairs, in launch order, qualify as `flags` says (serra09_fast_tail_runs, serra09_plan.hpp):
    one per maximal run of qualifying pairs; more than 2 + B / 32 runs in all: one generic launch."""
    runs = [f for k, f in enumerate(flags) if k == 0 or f != flags[k - 1]]
    return 0 if len(runs) > 2 + len(flags) // 32 else sum(runs)


def _expected_fast_launches(d, pairs, params=None):
    """How many launches of one product call over `pairs` (one batch) must take the FAST copy: the batch is sorted by the key
    5 cr + cq (stable), the row pass runs once per row class cr, the column pass once per key, and each pass is cut into runs of
    neighbouring pairs that all qualify or all do not."""
    keys = [S.key(int(d["M"][i]), int(d["M"][j]), M) for i, j in pairs]
    order = sorted(range(len(pairs)), key=lambda k: 5 * keys[k][0] + keys[k][1])
    flags = [_fast(dict(d, pairs=pairs), k, params) for k in range(len(pairs))]
    rows, cols = {}, {}
    for k in order:
        rows.setdefault(keys[k][0], []).append(flags[k][0])
        cols.setdefault(keys[k], []).append(flags[k][1])
    return sum(_fast_runs(v) for v in rows.values()) + sum(_fast_runs(v) for v in cols.values())


def _observed(ctx, d, pairs, p):
    """acx_serra09_debug_bits over `pairs` and the number of FAST launches it made, which must be the plan's."""
    from acoss_amd import _lib
    n0 = _lib.serra09_fast_tail_launches()
    out = ctx.serra09_debug_bits(pairs, p)
    got, want = _lib.serra09_fast_tail_launches() - n0, _expected_fast_launches(d, pairs, p)
    assert got == want, "FAST launches: %d, the plan says %d (pairs %s)" % (got, want, pairs.tolist())
    return out


def _product_call(ctx, d, tag, want=None, **kw):
    """One product call per pair list AND one per pair (a launch of its own each) against the oracle; returns the oracle's (scores, plots)."""
    from acoss_amd import _lib
    p = _lib.serra09_params(m=M, **kw)
    want = want if want is not None else S.oracle_plots(d, m=M, **kw)
    ctx.upload_pool(d["frames"], d["offsets"])
    scores, Rs = _observed(ctx, d, d["pairs"], p)
    print("%s: %d set bits outside the matrices' columns" % (tag, ctx.outside_bits))
    S.assert_plots_equal(d, M, Rs, want[1], tag)
    S.assert_scores_equal(d, M, scores, want[0], tag)
    assert ctx.outside_bits == 0, tag              # (the FAST copy drops the bitmap's column mask: pads are +inf and stay 0)
    S.assert_scores_equal(d, M, ctx.serra09_pairs(d["pairs"], p), want[0], tag + " serra09_pairs")
    for k in range(len(d["pairs"])):
        one = S.subset(d, d["pairs"][k:k + 1])
        s1, R1 = _observed(ctx, d, one["pairs"], p)
        S.assert_plots_equal(one, M, R1, want[1][k:k + 1], tag + " alone")
        S.assert_scores_equal(one, M, s1, want[0][k:k + 1], tag + " alone")
        assert ctx.outside_bits == 0, tag
    return want


def _wide_rows(d, it, i, j):
    """The rows of the pair's wide passes as the oracle's distances: [(role, rows x cells)]."""
    out = []
    if S.cls(int(d["M"][j]), M) == 4:
        out.append((0, it["d"]))
    if S.cls(int(d["M"][i]), M) == 4:
        out.append((1, it["d"].T))
    return out


def _census(rows):
    """From the oracle's distances of one wide pass (rows x n cells): rows whose order statistics ilo, ihi around the position are
    tied; rows with more than 64 cells equal to the statistic of rank ilo; rows surely inside the snap's relative gap (the kernel
    tests (shi - slo) > shi 2^-12 on SQUARED distances; the oracle's d = sqrtf(d2) squared in f64 is d2 within 2^-22 relative, so
    a margin of 2^-8 of the gap decides whatever the rounding) without being tied; rows that are zero throughout."""
    n = rows.shape[1]
    kf = np.float32(n - 1) * np.float32(KAPPA)
    ilo, ihi = int(np.floor(kf)), int(np.ceil(kf))
    assert ihi == ilo + 1
    s = np.sort(rows.astype(np.float64), axis=1)
    lo, hi = s[:, ilo], s[:, ihi]
    tied = lo == hi
    many = np.sum(rows.astype(np.float64) == lo[:, None], axis=1) > 64
    gap = ~tied & ((hi * hi - lo * lo) <= hi * hi * 2.0 ** -12 * (1 - 2.0 ** -8))
    zero = s[:, -1] == 0.0
    return dict(rows=len(rows), tied=int(tied.sum()), many=int(many.sum()), gap=int(gap.sum()), zero=int(zero.sum()))


def test_smallest_wide_rows(ctx):
    """(60, 1030) and (1030, 60) frames: 1021 cells, 17 tiles -- the wide class in the row pass only and in the column pass only,
    at its lower edge; the waves have two or three tiles, so the generic sweep runs with the FAST tail.  Also the class's very first
    length (1018 cells) and short tracks of 61 and 67 frames: 52 and 58 rows, the last band is partial."""
    rng = np.random.default_rng(701)
    d = _set([_iid(rng, T) for T in (60, 1030, 61, 67, 1027)], [(0, 1), (1, 0), (2, 1), (1, 3), (3, 4), (4, 2)])
    assert [S.key(int(d["M"][i]), int(d["M"][j]), M) for i, j in d["pairs"]] == [(4, 0), (0, 4), (4, 0), (0, 4), (4, 0), (0, 4)]
    for k in range(len(d["pairs"])):
        assert _fast(d, k) == ((True, False) if k % 2 == 0 else (False, True))
    _product_call(ctx, d, "smallest wide rows")


def test_full_waves_and_upper_edge(ctx):
    """1991 + 9 and 2041 + 9 frames against 60 and 67: four tiles per wave (the one-block sweep), the product length and the
    class's upper edge (32 tiles, 2041 cells), rows and columns."""
    rng = np.random.default_rng(702)
    d = _set([_iid(rng, T) for T in (60, 2000, 2050, 67)], [(0, 1), (1, 0), (3, 2), (2, 3), (0, 2)])
    assert [int(x) for x in d["M"]] == [51, 1991, 2041, 58]
    for k in range(len(d["pairs"])):
        assert any(_fast(d, k))
    _product_call(ctx, d, "full waves")


def test_pair_2000_by_2000(ctx):
    """One product-sized pair: both passes wide, FAST and the one-block sweep in both."""
    from acoss_amd import synth
    d0 = synth.rand_set(2, T=2000, seed=1234)
    d = dict(frames=d0["frames"], offsets=d0["offsets"], pairs=np.array([(0, 1)], np.int32), M=np.array([1991, 1991]))
    assert _fast(d, 0) == (True, True)
    _product_call(ctx, d, "2000 x 2000")


def test_mixed_launch_is_cut_into_runs(ctx):
    """2001 cells put the percentile position on an integer (2000 x 0.095 = 190 in f32: ihi == ilo): that pair does not qualify.  It
    shares its passes with pairs that do; the pass is cut into runs, the odd pair runs the generic copy and its neighbours the FAST
    one (the number of FAST launches is checked in _observed).  Thirteen alternating pairs make more runs than a pass is cut into:
    one generic launch."""
    rng = np.random.default_rng(703)
    d = _set([_iid(rng, T) for T in (60, 2010, 1500)], [(0, 1), (0, 2), (1, 0), (2, 0)])
    assert int(d["M"][1]) == 2001
    assert _fast(d, 0) == (False, False) and _fast(d, 2) == (False, False)
    assert _fast(d, 1) == (True, False) and _fast(d, 3) == (False, True)
    assert _expected_fast_launches(d, d["pairs"]) == 2
    want = _product_call(ctx, d, "mixed launch")
    alt = S.subset(d, [(0, 1), (0, 2)] * 6 + [(0, 1)])
    assert _expected_fast_launches(alt, alt["pairs"]) == 0
    from acoss_amd import _lib
    scores, Rs = _observed(ctx, alt, alt["pairs"], _lib.serra09_params(m=M))
    S.assert_plots_equal(alt, M, Rs, [want[1][k % 2] for k in range(13)], "alternating list")
    S.assert_scores_equal(alt, M, scores, np.array([want[0][k % 2] for k in range(13)], np.float32), "alternating list")


def _cold_tracks(rng, T_long=1030, T_short=60):
    from acoss_amd import synth
    protos = synth._frame_max_normalise(rng.random((5, 12)))
    runs = protos[np.repeat(rng.integers(0, 5, T_long // 25 + 1), 25)[:T_long]].astype(np.float32)
    const_long = np.repeat(protos[:1], T_long, axis=0).astype(np.float32)
    const_short = np.repeat(protos[:1], T_short, axis=0).astype(np.float32)
    half = _iid(rng, T_long // 2)
    twins = np.concatenate([half, half * (1.0 + 2e-6 * rng.random((T_long // 2, 12)))]).astype(np.float32)
    return dict(short=_iid(rng, T_short), runs=runs, const_long=const_long, const_short=const_short, twins=twins)


@pytest.mark.parametrize("case", ["runs", "constant", "zero", "twins"])
def test_forced_cold_exits(ctx, case):
    """The data-dependent exits of the FAST path into the generic continuation, rows and columns:
      runs      a long track of 25-frame runs of identical frames: the rows are heavily tied, the candidate list overflows
                (ncand > 64) or the pivot pass gives up, the narrowing selection answers and the closed-form threshold follows;
      constant  a long constant track against a random short one: every row is one value;
      zero      ... against the same constant: every distance is zero (the pivot's range test fails);
      twins     a long track whose second half repeats the first with a relative difference <= 2e-6: every cell has a near twin,
                so the two order statistics of many rows are distinct but closer than the snap's gap -- the selection succeeds
                and the gap test falls through.
    The condition is asserted from the oracle's distances before the device's result is looked at."""
    import oracle
    t = _cold_tracks(np.random.default_rng(704))
    short, long_ = {"runs": ("short", "runs"), "constant": ("short", "const_long"), "zero": ("const_short", "const_long"),
                    "twins": ("short", "twins")}[case]
    d = _set([t[short], t[long_]], [(0, 1), (1, 0)])
    assert _fast(d, 0) == (True, False) and _fast(d, 1) == (False, True)
    p = oracle.serra09_params(m=M)
    res = [oracle.serra09_pair(S.track(d, i), S.track(d, j), p, want_intermediates=True) for i, j in d["pairs"]]
    for (i, j), (_, it) in zip(d["pairs"], res):
        passes = _wide_rows(d, it, i, j)
        assert len(passes) == 1
        c = _census(passes[0][1])
        print("%s pair (%d, %d) role %d: %s" % (case, i, j, passes[0][0], c))
        if case == "runs":
            assert c["tied"] > c["rows"] // 2 and c["many"] > c["rows"] // 2, c
        elif case == "constant":
            assert c["tied"] == c["rows"] and c["many"] == c["rows"] and c["zero"] == 0, c
        elif case == "zero":
            assert c["zero"] == c["rows"], c
        else:
            assert c["gap"] > 0 and c["many"] == 0, c
    want = (np.array([s for s, _ in res], np.float32), [it["R"] for _, it in res])
    _product_call(ctx, d, "cold exit: " + case, want=want)


@pytest.mark.parametrize("kw", [dict(pct_mode=1), dict(pct_mode=2), dict(inclusive=0), dict(kappa=0.4)])
def test_parameter_sets_that_keep_the_generic_tail(ctx, kw):
    """pct_mode 1 and 2, the exclusive comparison and a kappa for which use_pivot fails: the plan refuses FAST, results stay the oracle's."""
    from acoss_amd import _lib
    rng = np.random.default_rng(705)
    d = _set([_iid(rng, T) for T in (60, 1030)], [(0, 1), (1, 0)])
    p = _lib.serra09_params(m=M, **kw)
    assert _fast(d, 0, p) == (False, False) and _fast(d, 1, p) == (False, False)
    _product_call(ctx, d, "generic: %s" % kw, **kw)


def test_eps_returning_debug_call(ctx):
    """acx_serra09_debug_pair wants eps and D2: the generic copy, every intermediate against the oracle (distances, eps, thresholds,
    plot, score) on the shapes of the FAST cases -- the thresholds of the same rows that the product call binarised above."""
    import oracle
    from acoss_amd import _lib
    rng = np.random.default_rng(701)
    d = _set([_iid(rng, T) for T in (60, 1030)], [(0, 1), (1, 0)])
    for role in (0, 1):
        assert _lib.serra09_fast_tail(1021, role, _lib.serra09_params(m=M), debug=True) is False
    ctx.upload_pool(d["frames"], d["offsets"])
    n0 = _lib.serra09_fast_tail_launches()
    for i, j in d["pairs"]:
        compare_pair(ctx, d, int(i), int(j), _lib.serra09_params(m=M), oracle.serra09_params(m=M), "debug pair (%d, %d)" % (i, j))
    assert _lib.serra09_fast_tail_launches() == n0          # the debug call launched the generic copies only
