"""
GPU tests (run with -m gpu on a real MI355X): the Serra09 STREAMING class, cell for cell -- what the product path launches for a pair with a
side of more than 2041 cells or a stack of 17 .. 33 frames (cr = cq = 5 in acoss_amd/csrc/serra09_plan.hpp): csm_long_kernel,
rowsel_long_kernel with wave_select_stream, binarise_long_kernel and the four qmax_bits_long_kernel<EQG, DMAX> instantiations of
acoss_amd/csrc/serra09_long_kernels.hpp.

tests/test_gpu_serra09_shapes.py pins the five band classes and m = 1 .. 16 and stops at rows of 2041 cells.  Here, with the same bars --
the recurrence plot through acx_serra09_debug_bits against the oracle's R with np.array_equal, scores equal, no tolerance, no pair
skipped -- every stack size 17 .. 33 (tree_sum_rt's decomposition of a run-time m, the 32-frame halo to its last frame), stacks of <= 16
frames inside the streaming kernels, a last 64 x 64 tile of 1, 63 and 64 rows and columns, matrices of one to three rows or columns,
every parameter switch the kernels read, the streaming selector on rows full of ties, one, two and three strips of 2048 columns for
dp_start 2 and 3 with alignments and penalised cells across the seams, batches that mix band and streaming pairs, pool neighbours, and the
pair grid.  The shape sets are tests/_serra09_shapes.py; tests/test_serra09_shapes_design.py shows on the CPU what they reach.

Bits outside a matrix's columns: binarise_long_kernel writes none and the sweeps mask them anyway; their count is printed, not asserted.
"""
import numpy as np
import pytest

from tests import _serra09_shapes as S
from tests._serra09_compare import compare_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


_SHARED = {}


def _reference(d, name, m, **kw):
    """(scores, plots) of the oracle for a whole set, left unchanged by its users.  long_set(9) at the defaults serves several tests and is
    computed once; every other reference has one user and is not kept."""
    key = (name, m, tuple(sorted(kw.items())))
    if key in _SHARED:
        return _SHARED[key]
    ref = S.oracle_plots(d, m=m, **kw)
    if key == ("long_set", 9, ()):
        _SHARED[key] = ref
    return ref


def _bits_and_scores(ctx, d, m, want, tag, **kw):
    """One product call over d's pairs through acx_serra09_debug_bits against want = (scores, plots) of the oracle."""
    from acoss_amd import _lib
    scores, Rs = ctx.serra09_debug_bits(d["pairs"], _lib.serra09_params(m=m, **kw))
    print("%s m=%d: %d set bits outside the matrices' columns (masked by the sweeps)" % (tag, m, ctx.outside_bits))
    S.assert_plots_equal(d, m, Rs, want[1], tag)
    S.assert_scores_equal(d, m, scores, want[0], tag)
    return scores, Rs


def _qmax_and_dmax(ctx, d, m, want, tag, **kw):
    """LateFusionChen's entry returns (Qmax, Dmax) of the same plots; acx_serra09_pairs returns its column 0."""
    from acoss_amd import _lib
    p = _lib.serra09_params(m=m, **kw)
    both = ctx.chenfusion_pairs(d["pairs"], p)
    S.assert_scores_equal(d, m, both, np.stack([want[0], S.oracle_sweeps(want[1], dmax=True)], 1), tag + " (Qmax, Dmax)")
    S.assert_scores_equal(d, m, ctx.serra09_pairs(d["pairs"], p), both[:, 0], tag + " serra09_pairs vs chenfusion_pairs")


# ---- (a) every stack size ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(17, 34))
def test_every_stack_size_bits_and_scores(ctx, m):
    """stack_set(m) in ONE call: 121 pairs with sides of 1, 2, 3, 63, 64, 65, 127, 128, 129, 200 and 449 cells both ways.  tree_sum_rt takes
    another path through its highest-bit / lower-bits decomposition for every m (31 = 16 + 8 + 4 + 2 + 1, 32 alone, 33 = 32 + 1 reads the
    halo's last frame); the iok / colok masks and the transposed write of csm_long_kernel see a last tile of 1, 63 and 64 cells."""
    d = S.stack_set(m)
    want = S.oracle_plots(d, m=m)
    ctx.upload_pool(d["frames"], d["offsets"])
    _bits_and_scores(ctx, d, m, want, "stack set")
    _qmax_and_dmax(ctx, d, m, want, "stack set")


# ---- (b) long sides at band-kernel stack sizes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 9, 16, 17, 33])
def test_long_sides_bits_and_scores(ctx, m):
    """long_set(m): a side beyond 2041 cells streams at any m, so the streaming kernels run with m <= 16 too.  Long sides on both sides of
    the class limit, of a tile edge and of one, two and three strips, as rows and as columns, against 1, 2, 3, 40 and 65 cells."""
    d = S.long_set(m)
    want = _reference(d, "long_set", m)
    ctx.upload_pool(d["frames"], d["offsets"])
    _bits_and_scores(ctx, d, m, want, "long set")
    _qmax_and_dmax(ctx, d, m, want, "long set")


def test_long_sides_dense_plots_through_every_sweep(ctx):
    """Dense plots (kappa = 0.4) of long_set(9) through all four qmax_bits_long_kernel<EQG, DMAX> instantiations on every strip count (the
    streaming sweep has no packed default-penalty kernel: (0.5, 0.5) and (1.0, 1.0) both take <true, D>).  Expected: the oracle's DP on
    the oracle's plot."""
    from acoss_amd import _lib
    m = 9
    d = S.long_set(m)
    want = _reference(d, "long_set", m, kappa=0.4)
    ctx.upload_pool(d["frames"], d["offsets"])
    _bits_and_scores(ctx, d, m, want, "long set kappa=0.4", kappa=0.4)
    for go, ge in ((0.5, 0.5), (1.0, 1.0), (1.0, 0.25)):
        for dmax in (0, 1):
            got = ctx.serra09_pairs(d["pairs"], _lib.serra09_params(m=m, kappa=0.4, gamma_o=go, gamma_e=ge, dmax=dmax))
            S.assert_scores_equal(d, m, got, S.oracle_sweeps(want[1], go, ge, bool(dmax)), "gammas (%g, %g) dmax=%d" % (go, ge, dmax))


@pytest.mark.parametrize("kw", [dict(), dict(kappa=0.4, gamma_o=1.0, gamma_e=0.25, dmax=1)], ids=["defaults", "dense-penalised-dmax"])
def test_long_sides_dp_start_3(ctx, kw):
    """dp_start = 3 drops the last row and column: 2049 and 4097 columns become one and two full strips, 2050 and 4099 keep a strip of one
    and two columns.  Expected: the full-chain oracle."""
    from acoss_amd import _lib
    m = 9
    d = S.long_set(m)
    ctx.upload_pool(d["frames"], d["offsets"])
    got = ctx.serra09_pairs(d["pairs"], _lib.serra09_params(m=m, dp_start=3, **kw))
    S.assert_scores_equal(d, m, got, S.oracle_scores(d, m=m, dp_start=3, **kw), "dp_start=3 %s" % (kw,))


# ---- (c) parameter switches inside the streaming kernels ------------------------------------------------------------------------------------
# (the last case: the combined set of test_gpu_serra09.py::test_parameter_switches_bit_exact.  Its m = 1 applies to the long_set(9) tracks,
# whose long sides stay beyond 2041 cells; stack_set(17) streams because of its m, which it keeps)
_SWITCHES = [dict(pct_mode=1), dict(pct_mode=2), dict(pct_mode=3), dict(inclusive=0), dict(kappa=0.0), dict(kappa=0.004), dict(kappa=0.4),
             dict(kappa=1.0), dict(embed_full=1), dict(oti=False), dict(oti_target=1), dict(tau=2),
             dict(dmax=1, gamma_o=1.0, gamma_e=0.5, m=1, kappa=0.3, pct_mode=2, inclusive=0, dp_start=3, oti=False)]


def _switch_sets(kw):
    """(name, m, set, parameters without m) for one switch setting; the sets' M by the oracle's embedded length under that setting."""
    tau = kw.get("tau", 1)
    rest = {k: v for k, v in kw.items() if k != "m"}
    for name, m, d in (("stack_set(17)", 17, S.stack_set(17, tau=tau)),
                       ("long_set(9) 2042 | 2049", kw.get("m", 9), S.long_subset(S.long_set(9, tau=tau)))):
        yield name, m, S.relabel(d, m, tau=tau, embed_full=kw.get("embed_full", 0)), rest


@pytest.mark.parametrize("kw", _SWITCHES, ids=lambda kw: ",".join("%s=%s" % it for it in kw.items()))
def test_parameter_switches_in_the_streaming_kernels(ctx, kw):
    """Each switch on its own, on stack_set(17) (m > 16) and on the twenty long_set(9) pairs with a side of 2042 or 2049 cells (m <= 16 inside
    the streaming kernels): rowsel_long_kernel's percentile modes (2 and 3 do not interpolate, 3 takes another k) and k clamped at both
    ends (kappa 0 and 1), the exclusive comparison, csm_long_kernel's query rotation (oti_target = 1) and no rotation at all, the other
    embedding length, a decimated pool.  Plots and scores per setting."""
    import oracle
    from acoss_amd import _lib
    for name, m, d, rest in _switch_sets(kw):
        p = oracle.serra09_params(m=m, **rest)
        assert [oracle.serra09_embed_len(int(T), p) for T in np.diff(d["offsets"])] == d["M"].tolist()
        rec = _lib.serra09_plan(np.diff(d["offsets"]), d["pairs"], _lib.serra09_params(m=m, **rest))
        assert np.all(rec["cr"] == S.NC) and np.all(rec["cq"] == S.NC) and np.all(rec["batch"] == 0), name
        if kw.get("oti_target") == 1:
            otis = S.pool_map(lambda ij: oracle.serra09_pair(S.track(d, ij[0]), S.track(d, ij[1]), p, want_intermediates=True)[1]["oti"],
                              d["pairs"])
            print("%s: transposition indices %s" % (name, sorted(set(otis))))
            assert len(set(otis)) >= 5, (name, sorted(set(otis)))
        want = S.oracle_plots(d, m=m, **rest)
        ctx.upload_pool(d["frames"], d["offsets"])
        _bits_and_scores(ctx, d, m, want, "%s %s" % (name, kw), **rest)


# ---- (d) the streaming selector on ties -----------------------------------------------------------------------------------------------------
_TIE_SETTINGS = [dict(), dict(pct_mode=1), dict(pct_mode=2), dict(pct_mode=3), dict(inclusive=0), dict(kappa=0.5), dict(kappa=0.0),
                 dict(kappa=1.0)]


@pytest.mark.parametrize("kw", _TIE_SETTINGS, ids=lambda kw: ",".join("%s=%s" % it for it in kw.items()) or "defaults")
@pytest.mark.parametrize("m", [17, 9])
def test_streaming_selector_on_ties(ctx, m, kw):
    """wave_select_stream on rows it cannot settle in one histogram pass: all-equal rows (a constant track), bins of more than 64 equal
    values (piecewise-constant tracks without noise, exact zeros), near-ties (periodic tracks); tests/test_serra09_shapes_design.py counts
    them.  tie_set(17): all 127 pairs stream; tie_set(9): the six pairs with the 2100-cell track.  Every streaming pair through
    acx_serra09_debug_pair: distances, eps_q / eps_r, the d2-domain thresholds, R and the score, bit for bit; the product call over the
    whole list returns the oracle's scores."""
    import oracle
    from acoss_amd import _lib
    d = S.tie_set(m)
    gp, op = _lib.serra09_params(m=m, **kw), oracle.serra09_params(m=m, **kw)
    rec = _lib.serra09_plan(np.diff(d["offsets"]), d["pairs"], gp)
    streams = np.nonzero(rec["cr"] == S.NC)[0]
    Ms = d["M"][d["pairs"]]
    assert np.array_equal(rec["cr"] == S.NC, np.ones(len(rec), bool) if m > 16 else Ms.max(axis=1) == S.TIE_LONG)
    refs = S.pool_map(lambda k: oracle.serra09_pair(S.track(d, d["pairs"][k][0]), S.track(d, d["pairs"][k][1]), op, want_intermediates=True),
                      streams)
    ctx.upload_pool(d["frames"], d["offsets"])
    for k, ref in zip(streams, refs):
        i, j = (int(v) for v in d["pairs"][k])
        compare_pair(ctx, d, i, j, gp, op, "ties %s %s" % (kw, S.describe(d, int(k), m)), ref=ref)
    S.assert_scores_equal(d, m, ctx.serra09_pairs(d["pairs"], gp), S.oracle_scores(d, m=m, **kw), "tie set %s" % (kw,))


# ---- (e) the strip seam, DP alone -----------------------------------------------------------------------------------------------------------
_SEAM_SETTINGS = [(0.5, 0.5, 0), (0.5, 0.5, 1), (1.0, 0.25, 0), (1.0, 0.25, 1)]
_SEAM_SHAPES = [(M, N) for N in (2047, 2048, 2049, 2050, 2051, 4095, 4096, 4097, 4098, 6145) for M in (1, 2, 3, 4, 5, 9, 64)] + \
               [(M, N) for M in (2042, 2500) for N in (1, 2, 3, 30)]


def _check_dp(ctx, R, setting, tag):
    import oracle
    from acoss_amd import _lib
    go, ge, dmax = setting
    got = ctx.qmax_binary(R, _lib.serra09_params(gamma_o=go, gamma_e=ge, dmax=dmax))
    ref = oracle.qmax_binary(R, go, ge, bool(dmax))
    assert got == ref, "%s, %d x %d plot, gammas (%g, %g) dmax=%d: device %r, oracle %r" % (tag, R.shape[0], R.shape[1], go, ge, dmax, got, ref)
    return ref


def test_strip_seam_on_random_and_full_plots(ctx):
    """qmax_bits_long_kernel alone (acx_qmax_binary) on plots of 2047 .. 6145 columns -- both sides of one, two and three strips -- with 1 .. 64
    rows (one to three rows with several strips: the bout[0], bout[1] and bin[i - 1] guards), and of 2042 and 2500 rows with 1 .. 30
    columns.  All ones, and random plots of density 0.3 and 0.8; every shape with every plot kind, the four settings {(0.5, 0.5),
    (1.0, 0.25)} x Qmax | Dmax taken in turn so that every shape and every kind meets each of them: 234 launches.  On such plots the best
    path seldom needs two strips (a build whose lane 0 ignored the records passed them), so the shapes with a seam and two rows or more
    get a fourth plot: density 0.8 within two columns of a diagonal that crosses the last seam in its middle row and nothing elsewhere, 48
    launches; with four rows or more (32 of the 48) a path along that diagonal is cut by the seam, so for at least half of the plots the
    oracle must score either side of the seam alone lower than the whole."""
    import oracle
    rng = np.random.default_rng(2048)
    seen, windows, crossing = set(), 0, 0
    for s, (M, N) in enumerate(_SEAM_SHAPES):
        for kind, dens in enumerate((1.0, 0.3, 0.8)):
            R = np.ones((M, N), np.uint8) if dens == 1.0 else (rng.random((M, N)) < dens).astype(np.uint8)
            t = (s + kind) % 4
            seen.add((kind, t))
            _check_dp(ctx, R, _SEAM_SETTINGS[t], "density %g" % dens)
        seam = (N - 1) // S.STRIP * S.STRIP
        if seam > 0 and M >= 2 and N > 2041:
            i, j = np.nonzero(rng.random((M, N)) < 0.8)
            keep = np.abs(j - (seam - M // 2 + i)) <= 2
            R = np.zeros((M, N), np.uint8)
            R[i[keep], j[keep]] = 1
            go, ge, dmax = _SEAM_SETTINGS[s % 4]
            whole = _check_dp(ctx, R, _SEAM_SETTINGS[s % 4], "density 0.8 along a diagonal across column %d" % seam)
            windows += 1
            crossing += max(oracle.qmax_binary(R[:, :seam], go, ge, bool(dmax)), oracle.qmax_binary(R[:, seam:], go, ge, bool(dmax))) < whole
    print("%d plots around a seam, %d of them score more than either side alone" % (windows, crossing))
    assert len(seen) == 12 and windows == 48 and 2 * crossing >= windows, (len(seen), windows, crossing)


def _diagonal(M, N, shift, missing=()):
    """Ones on j = i + shift but for the cells whose COLUMN is in `missing`."""
    R = np.zeros((M, N), np.uint8)
    for i in range(M):
        j = i + shift
        if 0 <= j < N and j not in missing:
            R[i, j] = 1
    return R


def test_strip_seam_on_planted_diagonals(ctx):
    """A diagonal of 64 ones that crosses column 2048 (4096) at an even and at an odd row: the path's score travels to the next strip
    through the float4 record of the two columns left of the seam.  Whole, with one cell missing at seam column -2, -1, 0, +1 (the
    penalised value crosses: the record's .z / .w halves), and with two adjacent cells missing astride the seam (the detour of
    test_qmax_analytic_known_answers: L - 4.5 with an onset penalty of 0.5, L - 5 with 1.0).  Four settings each: 96 launches."""
    import oracle
    M, L = 64, 64
    for seam, N in ((2048, 4098), (4096, 6145)):
        for row in (30, 31):
            shift = seam - row                                    # the diagonal's cell in row `row` sits in column `seam`
            gaps = [()] + [(seam + o,) for o in (-2, -1, 0, 1)] + [(seam - 1, seam)]
            for missing in gaps:
                R = _diagonal(M, N, shift, missing)
                assert int(R.sum()) == L - len(missing) and R[row, seam] == (seam not in missing)
                tag = "diagonal across column %d at row %d, missing columns %s" % (seam, row, list(missing))
                ref = [_check_dp(ctx, R, setting, tag) for setting in _SEAM_SETTINGS]
                if len(missing) == 2:        # on the oracle alone: the two penalty settings differ, so the record's penalty halves matter
                    assert (ref[0], ref[2]) == (L - 4.5, L - 5.0), (tag, ref)
                    assert oracle.qmax_binary(R[:, :seam]) < ref[0] and oracle.qmax_binary(R[:, seam:]) < ref[0]
                elif len(missing) == 0:
                    assert ref[0] == ref[2] == L - 2, (tag, ref)
                else:
                    assert ref[0] == L - 3.5, (tag, ref)


def _two_diagonals(M, N, ra, ca, di, dj):
    """Ones on the diagonal that ends in (ra, ca) and on the one that starts in (ra + di, ca + dj)."""
    R = np.zeros((M, N), np.uint8)
    t = np.arange(0, min(ra, ca) + 1)
    R[ra - t, ca - t] = 1
    t = np.arange(0, min(M - ra - di, N - ca - dj))
    R[ra + di + t, ca + dj + t] = 1
    return R


def test_strip_seam_on_diagonals_that_jump(ctx):
    """A straight diagonal reaches the next strip through ONE field of the record, Q[i - 1][c - 1] (.x of the row above), and where a
    detour has a mirror image on the other side of the diagonal the other fields stay unobserved (a build that dropped .y passed every
    other plot of this file but the dense long_set ones).  Here the only best path takes one of the other steps into the strip's first
    or second column: a diagonal that jumps by (1, 2) or by (2, 1) lands through Q[i - 1][c - 2] (.y) or Q[i - 2][c - 1] (.x of the
    record two rows up); one that jumps by (2, 4) or (4, 2) has exactly one route, two such steps through one missing cell, which takes
    the PENALISED halves (.w, .z).  The cell in question in column seam and seam + 1, in an even and an odd row.  64 launches."""
    import oracle
    M = 64
    for s, (seam, N) in enumerate(((2048, 4098), (4096, 6145))):
        for (di, dj), (hi, hj) in (((1, 2), (1, 2)), ((2, 1), (2, 1)), ((2, 4), (1, 2)), ((4, 2), (2, 1))):
            for col in (seam, seam + 1):
                row = 30 + (s + col) % 2                            # the landing cell, or the missing cell in the middle of the long jump
                ra, ca = row - hi, col - hj
                R = _two_diagonals(M, N, ra, ca, di, dj)
                L = int(R.sum())
                assert L == ra + 1 + M - ra - di and R[row, col] == ((di, dj) == (hi, hj))
                tag = "diagonal that jumps by (%d, %d) from (%d, %d), seam %d" % (di, dj, ra, ca, seam)
                ref = [_check_dp(ctx, R, setting, tag) for setting in _SEAM_SETTINGS]
                if (di, dj) == (hi, hj):                            # on the oracle alone: every one is on the path ...
                    assert ref[0] == ref[2] == L - 2, (tag, ref)
                else:                                               # ... and the missing cell costs one onset penalty
                    assert (ref[0], ref[2]) == (L - 2.5, L - 3.0), (tag, ref)
                assert oracle.qmax_binary(R[:, :seam]) < ref[0] and oracle.qmax_binary(R[:, seam:]) < ref[0]


# ---- (f) the seam through the whole chain ---------------------------------------------------------------------------------------------------
def test_alignments_across_the_strip_seams(ctx):
    """seam_set(9): two 300-cell queries whose alignments with the 4300-cell reference cross columns 2048 and 4096 (shown on the CPU: the
    plot cut at the seam scores about half), and the swapped order as control.  Plots, Qmax and Dmax, unequal penalties, dp_start 3."""
    from acoss_amd import _lib
    m = 9
    d = S.seam_set(m)
    want = S.oracle_plots(d, m=m)
    ctx.upload_pool(d["frames"], d["offsets"])
    _bits_and_scores(ctx, d, m, want, "seam set")
    _qmax_and_dmax(ctx, d, m, want, "seam set")
    assert min(want[0][:2]) >= 250
    for dmax in (0, 1):
        got = ctx.serra09_pairs(d["pairs"], _lib.serra09_params(m=m, gamma_o=1.0, gamma_e=0.25, dmax=dmax))
        S.assert_scores_equal(d, m, got, S.oracle_sweeps(want[1], 1.0, 0.25, bool(dmax)), "seam set gammas (1, 0.25) dmax=%d" % dmax)
        kw = dict(dp_start=3, dmax=dmax)
        got = ctx.serra09_pairs(d["pairs"], _lib.serra09_params(m=m, **kw))
        S.assert_scores_equal(d, m, got, S.oracle_scores(d, m=m, **kw), "seam set %s" % (kw,))
    both = ctx.chenfusion_pairs(d["pairs"], _lib.serra09_params(m=m, dp_start=3, gamma_o=1.0, gamma_e=0.25))
    ref = np.stack([S.oracle_scores(d, m=m, dp_start=3, gamma_o=1.0, gamma_e=0.25, dmax=x) for x in (0, 1)], 1)
    S.assert_scores_equal(d, m, both, ref, "seam set dp_start=3 gammas (1, 0.25) (Qmax, Dmax)")


# ---- (g) batches ----------------------------------------------------------------------------------------------------------------------------
def mixed_batch_set(m=9):
    """The twenty long_set(9) pairs with a side of 2042 or 2049 cells interleaved with twenty band-class pairs of edge_set(9) (sides of up to
    1017 cells), over ONE pool that holds both track lists."""
    from acoss_amd import synth
    dl, de = S.long_subset(S.long_set(m)), S.edge_set(m)
    nl = len(dl["M"])
    tracks = [S.track(dl, i) for i in range(nl)] + [S.track(de, i) for i in range(len(de["M"]))]
    band = [(i + nl, j + nl) for i, j in de["pairs"] if max(de["M"][i], de["M"][j]) <= 1017][:20]
    assert len(dl["pairs"]) == len(band) == 20
    pairs = np.empty((40, 2), np.int32)
    pairs[0::2], pairs[1::2] = dl["pairs"], band
    frames, offsets = synth.pack(tracks)
    return dict(frames=frames, offsets=offsets, pairs=pairs, M=np.concatenate([dl["M"], de["M"]]))


MIXED_SCRATCH_LIMIT = 4 << 20      # bytes: a streaming pair of 2049 x 65 cells takes 1.6 MB of D2, D2^T and strip records


def test_batches_that_mix_band_and_streaming_pairs(ctx):
    """A batch with a streaming pair keeps its sweeps on the main stream (the strip records live in the shared scratch arena), and so do
    chenfusion_pairs' two sweeps over one set of records.  The mixed list in one batch is the reference (a sample of it against the oracle);
    under a scratch limit that splits it into at least four batches with streaming pairs in consecutive ones, in permuted order and
    through chenfusion_pairs the scores are bit-equal to it.  Each run once."""
    import oracle
    from acoss_amd import _lib
    m = 9
    d = mixed_batch_set(m)
    p = _lib.serra09_params(m=m)
    lens = np.diff(d["offsets"])
    rec = _lib.serra09_plan(lens, d["pairs"], p)
    assert np.all(rec["batch"] == 0) and np.array_equal(rec["cr"] == S.NC, np.arange(40) % 2 == 0)
    rec = _lib.serra09_plan(lens, d["pairs"], p, scratch_limit=MIXED_SCRATCH_LIMIT)
    assert rec["batch"].max() >= 3
    with_stream = sorted({int(r["batch"]) for r in rec if r["cr"] == S.NC})
    assert len(with_stream) >= 4 and any(b + 1 in with_stream for b in with_stream), with_stream
    ctx.upload_pool(d["frames"], d["offsets"])
    one = ctx.serra09_pairs(d["pairs"], p)
    two = ctx.chenfusion_pairs(d["pairs"], p)
    S.assert_scores_equal(d, m, two[:, 0], one, "one batch: chenfusion_pairs vs serra09_pairs")
    sample = np.arange(0, 40, 3)
    ds = S.subset(d, d["pairs"][sample])
    S.assert_scores_equal(ds, m, one[sample], S.oracle_scores(ds, m=m), "one batch vs the oracle")
    S.assert_scores_equal(ds, m, two[sample, 1], S.oracle_scores(ds, m=m, dmax=1), "one batch, Dmax vs the oracle")
    perm = np.random.default_rng(40).permutation(40)
    dp = S.subset(d, d["pairs"][perm])
    S.assert_scores_equal(dp, m, ctx.serra09_pairs(dp["pairs"], p), one[perm], "one batch, permuted")
    ctx.set_scratch_limit(MIXED_SCRATCH_LIMIT)
    try:
        S.assert_scores_equal(d, m, ctx.serra09_pairs(d["pairs"], p), one, "several batches")
        S.assert_scores_equal(d, m, ctx.chenfusion_pairs(d["pairs"], p), two, "several batches (Qmax, Dmax)")
        S.assert_scores_equal(dp, m, ctx.serra09_pairs(dp["pairs"], p), one[perm], "several batches, permuted")
        S.assert_scores_equal(dp, m, ctx.chenfusion_pairs(dp["pairs"], p), two[perm], "several batches, permuted (Qmax, Dmax)")
    finally:
        ctx.set_scratch_limit(0)


# ---- (h) neighbours and the pool's end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,cells", [(9, (2049, 65)), (17, (129, 65))])
def test_pool_neighbours_do_not_leak_into_streaming_pairs(ctx, m, cells):
    """csm_long_kernel reads LST = 96 frames per tile side and zero-fills beyond the track's last frame; inside the pool the frames behind
    a track are its neighbour's.  The same two tracks, paired both ways, between different neighbours and as the last tracks of the
    pool: identical plots and scores, the oracle's (the pattern of test_gpu_serra09_shapes.py::test_pool_neighbours_do_not_leak)."""
    from acoss_amd import synth
    rng = np.random.default_rng([m, 8])
    X, Y = (synth._frame_max_normalise(rng.random((S.frames_for(M, m), 12))) for M in cells)
    nb = {"random": synth._frame_max_normalise(rng.random((120, 12))), "zero": np.zeros((120, 12), np.float32),
          "one": np.ones((120, 12), np.float32), "1e15": np.full((120, 12), 1e15, np.float32)}
    pools = [(kind, [N, X, N, Y, N], (1, 3)) for kind, N in nb.items()]
    pools += [("last: X, Y", [nb["random"], X, Y], (1, 2)), ("last: Y, X", [nb["1e15"], Y, X], (2, 1)), ("alone", [X, Y], (0, 1))]
    want = None
    for kind, tracks, (ix, iy) in pools:
        frames, offsets = synth.pack(tracks)
        d = dict(frames=frames, offsets=offsets, pairs=np.array([(ix, iy), (iy, ix)], np.int32),
                 M=np.array([S._embed_len(len(t), m) for t in tracks]))
        assert S.key(*cells, m) == (S.NC, S.NC)
        if want is None:
            want = S.oracle_plots(d, m=m)
        ctx.upload_pool(frames, offsets)
        _bits_and_scores(ctx, d, m, want, "neighbours: %s" % kind)


# ---- (i) the grid ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,first", [(9, 2049), (17, 300)])
def test_pair_grid_equals_pair_list_with_streaming_pairs(ctx, m, first):
    """acx_pair_grid over a pool of eight tracks, one of them of 2049 cells at m = 9 (its row and column of the grid stream, the other
    tiles do not), and over eight short tracks at m = 17 (every pair streams): the pair list's scores, bit for bit, for both grid
    kinds and two tile sizes (the pattern of test_gpu_grid.py::test_pair_grid_equals_pair_list_serra09)."""
    import oracle
    from acoss_amd import _lib, synth
    rng = np.random.default_rng([m, 9])
    lens = [S.frames_for(first, m), 150, 61, 330, 97, 240, 128 + m, 65 + m]
    tracks = [S._iid(rng, T) for T in lens]
    tracks[3] = S._version(rng, tracks[1].repeat(3, axis=0)[:lens[3]])
    frames, offsets = synth.pack(tracks)
    n = len(lens)
    p = _lib.serra09_params(m=m)
    rec = _lib.serra09_plan(np.diff(offsets), oracle.all_pairs(n, False).astype(np.int32), p)
    assert (rec["cr"] == S.NC).sum() == (14 if m == 9 else 56)
    ctx.upload_pool(frames, offsets)
    for sym in (True, False):
        pairs = oracle.all_pairs(n, sym).astype(np.int32)
        got = ctx.serra09_pairs(pairs, p)
        want = np.zeros((n, n), np.float32)
        want[pairs[:, 0], pairs[:, 1]] = got
        if sym:
            want += want.T
        for tile in (0, 3):
            D = np.zeros((n, n), np.float32)
            ctx.pair_grid(_lib.ALGO_SERRA09, sym, p, [D], mirror=sym, tile=tile)
            assert np.array_equal(D, want), (m, sym, tile, np.argwhere(D != want)[:5])
    pairs = oracle.all_pairs(n, True).astype(np.int32)
    assert np.array_equal(ctx.serra09_pairs(pairs, p), oracle.serra09_pairs(frames, offsets, pairs, oracle.serra09_params(m=m)))
