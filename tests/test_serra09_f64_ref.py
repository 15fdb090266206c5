"""
CPU-only: the f64 comparator of tests/_serra09_f64.py is right and sharp enough to hold the opt-in f16x2 Gram cell by cell
(tests/test_gpu_serra09_f16x2.py).

  1. It agrees with the oracle: the exact-f32 plot of the CPU oracle equals `classify`'s verdict on every decided cell of every pair of the
     three m = 9 shape sets -- the oracle's arithmetic lies inside DELTA_PLOT too, so a disagreement would be the comparator's mistake.
  2. The cells it leaves undecided are few: at most CAP_SET of a set's cells and CAP_PAIR of any pair of 10 000 cells or more.  They
     depend on the f64 matrix alone; the caps are conditions on the inputs (a changed seed that breaks one wants other inputs, not another cap).
  3. Under arith = "f16x2" the edge set reaches all 25 (cr, cq) keys and the three band_kernel<M<=9, 2 | 4 | 8> families in both passes,
     and no band2 kernel.
  4. The lower limit of the feature range the f16x2 mode accepts is the smallest power of two at which the two-term fp16 split still
     represents 2 xy within twice its error at a pool maximum of 1.
"""
import numpy as np
import pytest

from tests import _serra09_f64 as F
from tests import _serra09_shapes as S

M = F.M_STACK
SETS = ("edge_set", "tile_edge_set", "row_residue_set")
ALL_SETS = SETS + ("tau2_set",)       # (the stride-2 pairs of F.tau2_set: the same two conditions)
_MEASURED = {}


def _measure(name):
    """Per pair of a set: (cells, undecided cells, wrong decided cells of the oracle's plot, the first of them explained, max |d - sqrt(d2_f64)|,
    max |d^2 - d2_f64|).  Computed once per set and shared."""
    if name in _MEASURED:
        return _MEASURED[name]
    import oracle
    oracle.lib()
    tau = 2 if name == "tau2_set" else 1
    d = F.tau2_set(M) if name == "tau2_set" else getattr(S, name)(M)
    p = oracle.serra09_params(m=M, kappa=F.KAPPA, tau=tau)

    def one(ij):
        q, r = S.track(d, ij[0]), S.track(d, ij[1])
        _, it = oracle.serra09_pair(q, r, p, want_intermediates=True)
        assert F.oti(q, r) == it["oti"]
        d2 = F.d2_f64(q, r, M, it["oti"], tau)
        assert d2.shape == it["R"].shape
        c = F.classify(d2, F.KAPPA, F.DELTA_PLOT)
        assert not np.any(c["one"] & c["zero"])
        bad = F.wrong_decided(it["R"], c)
        d64 = it["d"].astype(np.float64)
        return (d2.size, int(np.sum(~(c["one"] | c["zero"]))), len(bad), F.explain(d2, c, bad[0]) if len(bad) else "",
                float(np.max(np.abs(d64 - np.sqrt(d2)))), float(np.max(np.abs(d64 * d64 - d2))))
    _MEASURED[name] = (d, S.pool_map(one, d["pairs"]), tau)
    return _MEASURED[name]


@pytest.mark.parametrize("name", ALL_SETS)
def test_comparator_agrees_with_the_oracle_on_every_decided_cell(name):
    d, res, tau = _measure(name)
    print("%s: %d pairs, max |d - sqrt(d2_f64)| = %.3g, max |d^2 - d2_f64| = %.3g" % (
        name, len(res), max(r[4] for r in res), max(r[5] for r in res)))
    for k, r in enumerate(res):
        assert r[2] == 0, "%s: the oracle's plot is wrong on %d decided cells, first %s" % (F.describe(d, k, tau), r[2], r[3])
        # the oracle's own f32 distances lie inside the envelope the device's are held to
        assert r[5] <= F.DELTA_D2, (F.describe(d, k, tau), r[5])


@pytest.mark.parametrize("name", ALL_SETS)
def test_undecided_cells_stay_under_the_caps(name):
    d, res, tau = _measure(name)
    cells, und = sum(r[0] for r in res), sum(r[1] for r in res)
    big = [(r[1] / r[0], k) for k, r in enumerate(res) if r[0] >= F.CAP_PAIR_CELLS]
    worst, k = max(big)
    print("%s: %d cells, %d undecided (%.2g); worst pair of >= %d cells: %.2g, %s" % (
        name, cells, und, und / cells, F.CAP_PAIR_CELLS, worst, F.describe(d, k, tau)))
    assert und <= F.CAP_SET * cells, (name, und, cells)
    assert worst <= F.CAP_PAIR, (F.describe(d, k, tau), worst)


def test_a_wrong_reference_is_noticed():
    """The comparator is sharp: a d2_f64 whose last column is made from the frames one stack further (frame M instead of M - 1: what a
    rim that reads one frame too far computes) disagrees with the oracle's plot on decided cells."""
    import oracle
    d = S.edge_set(M)
    i, j = d["start"][250], d["end"][249]
    q, r = S.track(d, i), S.track(d, j)
    _, it = oracle.serra09_pair(q, r, oracle.serra09_params(m=M), want_intermediates=True)
    good = F.d2_f64(q, r, M, it["oti"])
    assert len(F.wrong_decided(it["R"], F.classify(good))) == 0
    shifted = F.d2_f64(q, np.concatenate([r[1:], r[-1:]]), M, it["oti"])
    bad = good.copy()
    bad[:, -1] = shifted[:, -1]
    assert len(F.wrong_decided(it["R"], F.classify(bad))) > 0


def test_edge_set_reaches_every_f16x2_family():
    from acoss_amd import _lib
    d = S.edge_set(M)
    p = _lib.serra09_params(m=M, arith="f16x2")
    rec = _lib.serra09_plan(np.diff(d["offsets"]), d["pairs"], p)
    assert len(rec) == 45 and np.all(rec["batch"] == 0)
    assert {(int(r["cr"]), int(r["cq"])) for r in rec} == {(cr, cq) for cr in range(S.NC) for cq in range(S.NC)}
    want = {"band_kernel<M<=9, 2>", "band_kernel<M<=9, 4>", "band_kernel<M<=9, 8>"}
    rows = {_lib.serra09_family_name(f, M) for f in rec["row_family"]}
    cols = {_lib.serra09_family_name(f, M) for f in rec["col_family"]}
    assert rows == want and cols == want
    assert not any("band2" in f for f in rows | cols)
    # classes 0 and 1 share the two-tile kernel, 2 and 3 the four-tile one (the unpacked middle class), 4 has the eight-tile one
    by_class = {int(r["cr"]): _lib.serra09_family_name(r["row_family"], M) for r in rec}
    assert [by_class[c] for c in range(S.NC)] == ["band_kernel<M<=9, 2>"] * 2 + ["band_kernel<M<=9, 4>"] * 2 + ["band_kernel<M<=9, 8>"]
    for name in SETS[1:]:
        d = getattr(S, name)(M)
        rec = _lib.serra09_plan(np.diff(d["offsets"]), d["pairs"], p)
        assert np.all(rec["batch"] == 0)
        assert {_lib.serra09_family_name(f, M) for f in rec["row_family"]} == want


def test_the_accepted_range_is_where_the_split_is_accurate():
    """F.RANGE_LOG2[0] is the smallest power of two at which split_f16's representation error of 2 xy stays within twice its value at a
    pool maximum of 1, on an i.i.d. and on a chord pair; below it the second term falls into fp16's subnormal step of 2^-24 and the error
    doubles with every halving.  The upper limit keeps h1 finite and is as accurate as 1."""
    te, ed = S.tile_edge_set(M), S.edge_set(M)
    pairs = {"i.i.d.": (S.track(te, 4), S.track(te, 63)), "chord": (S.track(ed, ed["start"][250]), S.track(ed, ed["end"][249]))}
    lo, hi = F.RANGE_LOG2
    ok_below = []
    for name, (q, r) in pairs.items():
        assert q.max() == 1.0 and r.max() == 1.0
        at1 = F.split_error_2xy(q, r, M, 1.0)
        err = {e: F.split_error_2xy(q, r, M, 2.0 ** e) for e in (lo - 1, lo, hi, -4, -8)}
        print("%s pair: error of 2 xy at pool maximum 1: %.3g; %s" % (name, at1, ", ".join("2^%d: %.3g" % (e, err[e]) for e in sorted(err))))
        assert err[lo] <= 2 * at1 and err[hi] <= 2 * at1, (name, at1, err)
        assert err[-8] > 100 * at1, (name, at1, err)          # the former lower limit: two orders worse
        ok_below.append(err[lo - 1] <= 2 * at1)
    assert not all(ok_below)                                  # lo is the smallest
