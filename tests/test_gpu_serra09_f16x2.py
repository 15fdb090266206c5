"""
GPU tests (run with -m gpu on a real MI355X): the nine band kernel instantiations of the opt-in Serra09 arithmetic arith = "f16x2" --
band_kernel<9, 2 | 4 | 8, role 0 | 1, D2 written or not, ARITH = 1> -- cell by cell against f64, at the size-class edges, tile rims and
row residues of tests/_serra09_shapes.py.

This arithmetic is not the f32 spec, so the oracle's plot is no bit-for-bit specification of it.  tests/_serra09_f64.py says which
cells the f64 distances DECIDE when squared distances are known within DELTA_PLOT (from the f64 matrix alone, never from the device's);
on those the device's plot must equal the f64 plot, in every pair, with no allowance.  tests/test_serra09_f64_ref.py proves the
comparator against the CPU oracle and caps the undecided cells.  The squared distances themselves and the thresholds are held through
acx_serra09_debug_pair (the D2-writing instantiations), the sweep by the oracle's sweep of the DEVICE's plots, bit for bit.
"""
import numpy as np
import pytest

from tests import _serra09_f64 as F
from tests import _serra09_shapes as S

pytestmark = pytest.mark.gpu

M = F.M_STACK
SETS = ("edge_set", "tile_edge_set", "row_residue_set")


def _pf(**kw):
    from acoss_amd import _lib
    return _lib.serra09_params(m=M, arith="f16x2", **kw)


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


_RUNS = {}


def _run(ctx, name):
    """One product call (acx_serra09_debug_bits, arith = f16x2) over a whole set: (set, scores, plots, outside_bits), made once and
    left unchanged by its users."""
    if name not in _RUNS:
        tau = 2 if name == "tau2_set" else 1
        d = F.tau2_set(M) if name == "tau2_set" else getattr(S, name)(M)
        ctx.upload_pool(d["frames"], d["offsets"])
        scores, Rs = ctx.serra09_debug_bits(d["pairs"], _pf(tau=tau))
        _RUNS[name] = (d, scores, Rs, ctx.outside_bits, tau)
    return _RUNS[name]


def _assert_plots_decided(d, Rs, tau, tag):
    """On every cell the f64 distances decide within DELTA_PLOT the device's plot is the f64 plot."""
    def one(k):
        i, j = d["pairs"][k]
        q, r = S.track(d, i), S.track(d, j)
        d2 = F.d2_f64(q, r, M, F.oti(q, r), tau)
        if d2.shape != Rs[k].shape:
            return "shape %s, expected %s" % (Rs[k].shape, d2.shape), 0, 0
        c = F.classify(d2, F.KAPPA, F.DELTA_PLOT)
        bad = F.wrong_decided(Rs[k], c)
        und = int(np.sum(~(c["one"] | c["zero"])))
        return ("%d of %d decided cells wrong, first %s" % (len(bad), d2.size - und, F.explain(d2, c, bad[0]))) if len(bad) else "", d2.size, und
    res = S.pool_map(one, range(len(d["pairs"])))
    print("%s: %d pairs, %d cells, %d undecided" % (tag, len(res), sum(r[1] for r in res), sum(r[2] for r in res)))
    wrong = [(k, r[0]) for k, r in enumerate(res) if r[0]]
    assert not wrong, "%s: %d of %d pairs differ from the f64 plot; first: %s: %s" % (
        tag, len(wrong), len(res), F.describe(d, wrong[0][0], tau), wrong[0][1])


@pytest.mark.parametrize("name", SETS)
def test_product_path_plots_cell_by_cell(ctx, name):
    """(a) band_kernel<9, 2 | 4 | 8, role 0 | 1, false, 1> as acx_serra09_pairs launches them, many pairs per launch sorted by class:
    all 25 (cr, cq) keys and both sides of every class edge, of every tile count, every row count mod 8."""
    d, _, Rs, outside, tau = _run(ctx, name)
    print("%s f16x2: %d set bits outside the matrices' columns (masked by the sweeps)" % (name, outside))
    _assert_plots_decided(d, Rs, tau, name)


@pytest.mark.parametrize("name", SETS)
def test_scores_are_exact_given_the_plot(ctx, name):
    """(b) The sweep is the same code in both arithmetics: the scores are the oracle's sweep of the DEVICE's f16x2 plots bit for bit, the
    product entry returns them, LateFusionChen's entry (Qmax, Dmax) of the same plots."""
    d, scores, Rs, _, _ = _run(ctx, name)
    want = S.oracle_sweeps(Rs)
    S.assert_scores_equal(d, M, scores, want, "%s f16x2 debug_bits vs the sweep of its plots" % name)
    ctx.upload_pool(d["frames"], d["offsets"])
    S.assert_scores_equal(d, M, ctx.serra09_pairs(d["pairs"], _pf()), want, "%s f16x2 serra09_pairs" % name)
    S.assert_scores_equal(d, M, ctx.chenfusion_pairs(d["pairs"], _pf()), np.stack([want, S.oracle_sweeps(Rs, dmax=True)], 1),
                          "%s f16x2 (Qmax, Dmax)" % name)


def _ulp4(lo, hi):
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    return lo - 4.0 * np.spacing(lo32).astype(np.float64), hi + 4.0 * np.spacing(hi32).astype(np.float64)


def _f64_of_pair(q, r):
    """What a debug pair is held to: (oti, d2_f64, the thresholds' bounds at DELTA_D2 widened by 4 f32 ulp)."""
    oti = F.oti(q, r)
    d2 = F.d2_f64(q, r, M, oti)
    c = F.classify(d2, F.KAPPA, F.DELTA_D2)
    return oti, d2, {"eps_q": _ulp4(c["q_lo"], c["q_hi"]), "eps_r": _ulp4(c["r_lo"], c["r_hi"])}


def _check_debug_pair(got, ref, tag, scale=1.0):
    """The output of acx_serra09_debug_pair (arith = f16x2) for features uploaded times `scale` against f64: the transposition index,
    every threshold between the percentiles of the distances' bounds, |d2 - d2_f64| <= DELTA_D2 in every cell (in units of the
    unscaled features).  Returns the largest error."""
    oti, want, bounds = ref
    assert got["oti"] == oti, tag
    assert got["d2"].shape == want.shape, tag
    for name, (lo, hi) in bounds.items():
        eps = got[name].astype(np.float64) / float(scale)
        out = np.nonzero((eps < lo) | (eps > hi))[0]
        assert len(out) == 0, "%s: %s outside the f64 bounds at %d of %d entries, first %d: %.9g not in [%.9g, %.9g]" % (
            tag, name, len(out), len(eps), out[0], eps[out[0]], lo[out[0]], hi[out[0]])
    err = np.abs(got["d2"].astype(np.float64) / (float(scale) * float(scale)) - want)
    worst = float(err.max())
    print("%s: max |d2 - d2_f64| = %.3g" % (tag, worst))
    if worst > F.DELTA_D2:
        bad = np.argwhere(err > F.DELTA_D2)
        rows, cols = np.unique(bad[:, 0]), np.unique(bad[:, 1])
        raise AssertionError("%s: |d2 - d2_f64| up to %.3g > %.3g in %d cells of rows %d .. %d (%d of them) and columns %d .. %d (%d), worst at %s" % (
            tag, worst, F.DELTA_D2, len(bad), rows[0], rows[-1], len(rows), cols[0], cols[-1], len(cols),
            np.unravel_index(int(np.argmax(err)), err.shape)))
    return worst


def _debug_pairs(ctx, d, cases):
    """The listed pairs of the uploaded set d through the debug entry, then (on the CPU threads) against f64: {(i, j): worst error}."""
    got = [ctx.serra09_debug_pair(int(i), int(j), _pf()) for i, j in cases]
    def one(k):
        i, j = (int(x) for x in cases[k])
        tag = "Mq=%d Mr=%d (cr, cq)=%s" % (d["M"][i], d["M"][j], S.key(int(d["M"][i]), int(d["M"][j]), M))
        return _check_debug_pair(got[k], _f64_of_pair(S.track(d, i), S.track(d, j)), tag)
    worst = S.pool_map(one, range(len(cases)))
    per_class = {}
    for (i, j), w in zip(cases, worst):
        cr = S.key(int(d["M"][i]), int(d["M"][j]), M)[0]
        per_class[cr] = max(per_class.get(cr, 0.0), w)
    print("worst |d2 - d2_f64| per reference class: %s" % ", ".join("%d: %.3g" % kv for kv in sorted(per_class.items())))
    return per_class


def test_d2_and_thresholds_at_class_edges(ctx):
    """(c) band_kernel<9, V4, 0, true, 1> and <9, V4, 1, false, 1> through the debug entry: the last and the first row length of every
    class, square, and 249 x 2041 / 2041 x 249."""
    d = S.edge_set(M)
    ctx.upload_pool(d["frames"], d["offsets"])
    st, en = d["start"], d["end"]
    cases = [(st[n], en[n]) for n in (249, 250, 505, 506, 761, 762, 1017, 1018, 2041)] + [(st[249], en[2041]), (st[2041], en[249])]
    assert sorted(_debug_pairs(ctx, d, cases)) == list(range(S.NC))


def test_d2_and_thresholds_at_row_residues(ctx):
    """(c) 1, 7, 9 and 17 rows (a partial band, a band and one row, two bands and one row) against one reference per class."""
    d = S.row_residue_set(M)
    ctx.upload_pool(d["frames"], d["offsets"])
    cases = [(int(i), int(j)) for i, j in d["pairs"] if int(d["M"][i]) in (1, 7, 9, 17)]
    assert len(cases) == 20
    assert sorted(_debug_pairs(ctx, d, cases)) == list(range(S.NC))


def test_batches_and_order_do_not_change_the_bits(ctx):
    """(d) The edge set in several batches (a scratch limit the plan splits at) and reversed: the same scores bit for bit."""
    from acoss_amd import _lib
    d, scores, _, _, _ = _run(ctx, "edge_set")
    ctx.upload_pool(d["frames"], d["offsets"])
    limit = 1 << 20
    assert _lib.serra09_plan(np.diff(d["offsets"]), d["pairs"], _pf(), scratch_limit=limit)["batch"].max() >= 2
    ctx.set_scratch_limit(limit)
    try:
        S.assert_scores_equal(d, M, ctx.serra09_pairs(d["pairs"], _pf()), scores, "f16x2 in several batches")
        S.assert_scores_equal(d, M, ctx.serra09_pairs(d["pairs"][::-1], _pf())[::-1], scores, "f16x2 in several batches, reversed")
    finally:
        ctx.set_scratch_limit(0)
    S.assert_scores_equal(d, M, ctx.serra09_pairs(d["pairs"][::-1], _pf())[::-1], scores, "f16x2 reversed")


def test_modes_alternate_on_one_context(ctx):
    """(d) The f32 and the f16 operand pool share the launcher's pointer slot: exact -> f16x2 -> exact -> f16x2 over one list returns each
    mode's own bits again, also around a tau = 2 call of either mode (which drops both pools and rebuilds them from the decimated one)."""
    from acoss_amd import _lib
    d = S.row_residue_set(M)
    ctx.upload_pool(d["frames"], d["offsets"])
    pe = _lib.serra09_params(m=M)
    long_enough = np.array([k for k, (i, j) in enumerate(d["pairs"]) if d["M"][i] >= 14])     # (tau = 2 halves a track: the stack must still fit)
    sub = d["pairs"][long_enough]
    first = {}
    for mode, p in (("exact", pe), ("f16x2", _pf())) * 2:
        got = ctx.serra09_debug_bits(d["pairs"], p)
        if mode in first:
            S.assert_scores_equal(d, M, got[0], first[mode][0], "%s again" % mode)
            S.assert_plots_equal(d, M, got[1], first[mode][1], "%s again" % mode)
        else:
            first[mode] = got
    want = S.oracle_plots(d, m=M)
    S.assert_plots_equal(d, M, first["exact"][1], want[1], "exact between f16x2 calls")
    tau2 = {}
    for mode, p2, p1 in (("exact", _lib.serra09_params(m=M, tau=2), pe), ("f16x2", _pf(tau=2), _pf())):
        tau2[mode] = ctx.serra09_pairs(sub, p2)
        for again, p in (("f16x2", _pf()), ("exact", pe)):
            got = ctx.serra09_debug_bits(d["pairs"], p)
            S.assert_scores_equal(d, M, got[0], first[again][0], "%s after a tau = 2 call of %s" % (again, mode))
            S.assert_plots_equal(d, M, got[1], first[again][1], "%s after a tau = 2 call of %s" % (again, mode))
        assert np.array_equal(ctx.serra09_pairs(sub, p2), tau2[mode]), mode
    assert np.array_equal(tau2["exact"], S.oracle_scores(S.subset(d, sub), m=M, tau=2))


def test_stride_two_plots_cell_by_cell(ctx):
    """(d) One tau = 2 pair per family through (a): the operand pool made from the decimated pool, the embedding at stride 2 in f64."""
    d, scores, Rs, outside, tau = _run(ctx, "tau2_set")
    assert tau == 2 and [R.shape for R in Rs] == [(n, n) for n in F.TAU2_CELLS]
    print("tau2_set f16x2: %d set bits outside the matrices' columns" % outside)
    _assert_plots_decided(d, Rs, tau, "tau2_set")
    assert np.array_equal(scores, S.oracle_sweeps(Rs))


def test_accuracy_over_the_accepted_range(ctx):
    """(e) One 505-cell and one 1017-cell pair uploaded scaled by every fourth power of two from the lower to the upper limit of the range
    arith = f16x2 accepts, the limits included: |d2 - 4^e d2_f64| <= 4^e DELTA_D2 and the thresholds scale with 2^e.  One step beyond
    either limit the pool is refused."""
    from acoss_amd import synth
    d0 = S.edge_set(M)
    tracks = [S.track(d0, d0[side][n]) for n in (505, 1017) for side in ("start", "end")]
    assert all(t.max() == 1.0 for t in tracks)
    frames, offsets = synth.pack(tracks)
    refs = S.pool_map(lambda ij: _f64_of_pair(tracks[ij[0]], tracks[ij[1]]), [(0, 1), (2, 3)])
    lo, hi = F.RANGE_LOG2
    exps = list(range(lo, hi + 1, 2))
    assert exps[0] == lo and exps[-1] == hi
    for e in exps:
        scale = 2.0 ** e
        ctx.upload_pool(frames * np.float32(scale), offsets)
        for (i, j), ref in zip(((0, 1), (2, 3)), refs):
            _check_debug_pair(ctx.serra09_debug_pair(i, j, _pf()), ref, "pool maximum 2^%d, %d x %d cells" % ((e,) + ref[1].shape), scale)
    for e in (lo - 1, hi + 1):
        ctx.upload_pool(frames * np.float32(2.0 ** e), offsets)
        with pytest.raises(NotImplementedError, match=r"f16x2 needs features .*\[2\^%d, 2\^%d\]" % (lo, hi)):
            ctx.serra09_pairs(np.array([[0, 1]], np.int32), _pf())
