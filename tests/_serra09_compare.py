"""
The intermediate-by-intermediate comparison of one Serra09 pair (acx_serra09_debug_pair against the CPU oracle) that
tests/test_gpu_serra09.py and tests/test_gpu_serra09_streaming.py share.
"""
import numpy as np


def _track(d, i):
    return d["frames"][d["offsets"][i]:d["offsets"][i + 1]]


def compare_pair(ctx, d, i, j, gp, op, tag="", ref=None):
    """Pair (i, j) of the uploaded pool d through acx_serra09_debug_pair with the parameters gp against the oracle with op: transposition
    index, distances, eps_q / eps_r, the d2-domain thresholds, the recurrence plot and the score, bit for bit.  ref: the oracle's
    (score, intermediates) of that pair where the caller has computed them already."""
    import oracle
    g = ctx.serra09_debug_pair(i, j, gp)
    s, it = ref if ref is not None else oracle.serra09_pair(_track(d, i), _track(d, j), op, want_intermediates=True)
    assert g["oti"] == it["oti"], "%s oti %d vs %d" % (tag, g["oti"], it["oti"])
    dg = np.sqrt(g["d2"])
    nbad = int(np.sum(dg != it["d"]))
    assert nbad == 0, "%s distances differ in %d / %d cells, max |diff| %g" % (
        tag, nbad, dg.size, float(np.max(np.abs(dg - it["d"]))))
    bq = np.nonzero(g["eps_q"] != it["eps_q"])[0]
    br = np.nonzero(g["eps_r"] != it["eps_r"])[0]
    assert len(bq) == 0, "%s row thresholds differ at %s: %s vs %s" % (tag, bq[:5], g["eps_q"][bq[:5]], it["eps_q"][bq[:5]])
    assert len(br) == 0, "%s col thresholds differ at %s: %s vs %s" % (tag, br[:5], g["eps_r"][br[:5]], it["eps_r"][br[:5]])
    # the device compares SQUARED distances against thresholds moved to the d2 domain: thr = the
    # largest f32 x with sqrt(x) <= eps (inclusive) or sqrt(x) < eps (exclusive), so `d2 <= thr` is the
    # test in both modes; it must reproduce the oracle's comparison of d = sqrt(d2) with eps
    Rg = (g["d2"] <= g["thr_q"][:, None]) & (g["d2"] <= g["thr_r"][None, :])
    if op.inclusive:
        Rd = (dg <= g["eps_q"][:, None]) & (dg <= g["eps_r"][None, :])
    else:
        Rd = (dg < g["eps_q"][:, None]) & (dg < g["eps_r"][None, :])
    assert np.array_equal(Rg, Rd), "%s d2-domain thresholds disagree with d-domain comparison in %d cells" % (
        tag, int(np.sum(Rg != Rd)))
    assert np.array_equal(Rg.astype(np.uint8), it["R"]), "%s recurrence plot differs in %d cells" % (
        tag, int(np.sum(Rg.astype(np.uint8) != it["R"])))
    assert g["score"] == s, "%s score %r vs %r" % (tag, g["score"], s)
    return g, it
