"""
CPU test of the dispatch predicate of the band kernel's product-path tail (serra09_fast_tail, acoss_amd/csrc/serra09_plan.hpp,
through acx_serra09_fast_tail): which parameter sets and row lengths may run band_row_tail's FAST copy.  The predicate is restated
here in numpy float32 from the conditions the kernel's generic copy tests at run time (band_row_tail: `weights_ok`, `use_pivot`,
the interpolating percentile, the inclusive comparison, no eps) and compared for every row length of the wide class.
"""
import numpy as np
import pytest

WIDE = (1018, 2041)         # cells per row of the wide class (17 .. 32 tiles of 64 columns)


def _expect(n, kappa=0.095, pct_mode=0, inclusive=1, arith=0, debug=False):
    f = np.float32
    kf = f(n - 1) * f(kappa) if n > 1 else f(n) * f(kappa)
    fl, ce = np.floor(kf), np.ceil(kf)
    ilo = min(max(int(fl), 0), n - 1)
    ihi = min(max(int(ce), 0), n - 1)
    weights_ok = ihi == ilo + 1 and fl >= f(1) and f(ce - kf) >= f(2.0 ** -8) and f(kf - fl) >= f(2.0 ** -8)
    use_pivot = (ihi + 2) * 9 <= n
    return bool(WIDE[0] <= n <= WIDE[1] and arith == 0 and pct_mode == 0 and inclusive and not debug and weights_ok and use_pivot)


def test_every_wide_row_length_at_the_default_parameters():
    from acoss_amd import _lib
    p = _lib.serra09_params()
    got = {n: (_lib.serra09_fast_tail(n, 0, p), _lib.serra09_fast_tail(n, 1, p)) for n in range(WIDE[0] - 3, WIDE[1] + 4)}
    for n, (row, col) in got.items():
        assert row == col == _expect(n), n
    # the product configuration's lengths take it; a position (n - 1) kappa that is an integer in f32 does not (ihi == ilo)
    for n in (1021, 1991, 2041, WIDE[0]):
        assert got[n] == (True, True), n
    for n in (1201, 1401, 1801, 2001):
        assert np.float32(n - 1) * np.float32(0.095) == np.floor(np.float32(n - 1) * np.float32(0.095))
        assert got[n] == (False, False), n
    # the classes beside the wide one
    assert got[WIDE[0] - 1] == (False, False) and got[WIDE[1] + 1] == (False, False)
    assert sum(r for r, _ in got.values()) > 0.95 * (WIDE[1] - WIDE[0] + 1)       # almost every length of the class


@pytest.mark.parametrize("kw", [dict(pct_mode=1), dict(pct_mode=2), dict(pct_mode=3), dict(inclusive=0), dict(kappa=0.4),
                                dict(kappa=0.12), dict(kappa=0.0004), dict(kappa=0.0), dict(kappa=1.0), dict(arith="f16x2")])
def test_parameter_sets_that_keep_the_generic_tail(kw):
    from acoss_amd import _lib
    p = _lib.serra09_params(**kw)
    ex = dict(kw)
    ex["arith"] = 1 if kw.get("arith") == "f16x2" else 0
    for n in (1021, 1500, 1991, 2041):
        for role in (0, 1):
            assert _lib.serra09_fast_tail(n, role, p) == _expect(n, **ex) == False, (kw, n, role)


def test_use_pivot_threshold_in_kappa():
    """(ihi + 2) * 9 <= n is the selection's `use_pivot`: at n = 1991 it holds up to ihi = 219, i.e. kappa just below 0.11."""
    from acoss_amd import _lib
    for kappa in (0.05, 0.095, 0.1, 0.109, 0.1095, 0.111, 0.2):
        p = _lib.serra09_params(kappa=kappa)
        for n in (1021, 1991):
            assert _lib.serra09_fast_tail(n, 0, p) == _expect(n, kappa=kappa), (kappa, n)
    assert _lib.serra09_fast_tail(1991, 0, _lib.serra09_params(kappa=0.109)) is True
    assert _lib.serra09_fast_tail(1991, 0, _lib.serra09_params(kappa=0.111)) is False


def test_debug_call_and_other_stack_sizes():
    from acoss_amd import _lib
    p = _lib.serra09_params()
    for role in (0, 1):
        assert _lib.serra09_fast_tail(1991, role, p, debug=True) is False      # eps (and D2 in the row pass) wanted
    for m in (1, 4, 9, 10, 16):
        assert _lib.serra09_fast_tail(1991, 0, _lib.serra09_params(m=m)) is True
    assert _lib.serra09_fast_tail(1991, 0, _lib.serra09_params(m=17)) is False  # the streaming kernels
    with pytest.raises(ValueError):
        _lib.serra09_fast_tail(0, 0, p)
