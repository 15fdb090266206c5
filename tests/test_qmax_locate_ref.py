"""
Host-side checks of the locating Qmax sweep (Serra09.align / align_matches, acx_serra09_align, acx_qmax_locate_binary): the
two restatements of the contract in tests/_qmax_locate_ref.py against each other, against the CPU oracle's score and against
hand-checked answers; the ABI surface; the Python-side argument checks, none of which may touch a GPU.
"""
import os
import re

import numpy as np
import pytest

from . import _qmax_locate_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMAS = ((0.5, 0.5), (1.0, 0.25), (0.25, 1.0))


def _both(R, go=0.5, ge=0.5, dp_start=2):
    a = ref.locate_traceback(R, go, ge, dp_start)
    b = ref.locate_forward(R, go, ge, dp_start)
    assert a == b, "traceback %s vs forward %s for a %s plot, gammas (%s, %s), dp_start %d" % (a, b, np.shape(R), go, ge, dp_start)
    return b


@pytest.mark.parametrize("seed", range(6))
def test_the_two_implementations_agree_and_score_as_the_oracle(seed):
    import oracle
    rng = np.random.default_rng(900 + seed)
    shapes = [(1, 1), (40, 70), (2, 9), (9, 2), (3, 3), (1, 30)]
    for n in range(60):                            # 6 x 60 plots
        M, N = shapes[n] if n < len(shapes) else (int(rng.integers(1, 41)), int(rng.integers(1, 71)))
        R = (rng.random((M, N)) < rng.uniform(0.02, 0.6)).astype(np.uint8)
        for go, ge in GAMMAS:
            got = _both(R, go, ge, 2)
            want = np.float32(oracle.qmax_binary(R, go, ge))
            assert np.float32(got[0]).view(np.uint32) == want.view(np.uint32), (M, N, go, ge, got, want)
            assert (got[0] == 0) == (got[1:] == (-1, -1, -1, -1))
            if got[0] > 0:
                assert R[got[1], got[2]] == 1, "a path starts at a match cell"
                assert 2 <= got[1] <= got[3] < M and 2 <= got[2] <= got[4] < N
            # dp_start 3: the same DP on the plot less its last row and column, in the same (R) frame
            assert _both(R, go, ge, 3) == _both(R[:M - 1, :N - 1], go, ge, 2)


def test_hand_checked_answers():
    assert _both(np.eye(8)) == (6.0, 2, 2, 7, 7)
    assert _both(np.eye(8), dp_start=3) == (5.0, 2, 2, 6, 6)
    # one gap: 3 matches, a gap after a match (-gamma_o), 4 matches
    R = np.eye(10, dtype=np.uint8)
    R[5, 5] = 0
    assert _both(R) == (6.5, 2, 2, 9, 9)
    assert _both(R, 1.0, 0.25) == (6.0, 2, 2, 9, 9)
    # two gaps on the diagonal: ONE gap cell bridges them -- (4, 4) = 3, the gap cell (5, 6) = 3 - gamma_o by its (i-1, j-2)
    # predecessor, (7, 7) = that + 1 by its (i-2, j-1) predecessor, four more matches -- which beats walking the diagonal
    # (3 - gamma_o - gamma_e + 5)
    R = np.eye(12, dtype=np.uint8)
    R[5, 5] = R[6, 6] = 0
    assert _both(R) == (7.5, 2, 2, 11, 11)
    assert _both(R, 1.0, 0.25) == (7.0, 2, 2, 11, 11)
    assert _both(R, 0.25, 1.0) == (7.75, 2, 2, 11, 11)
    # a (2, 1) and a (1, 2) step instead of gaps
    R = np.zeros((12, 12), np.uint8)
    for c in ((2, 2), (3, 3), (5, 4), (6, 5), (7, 7), (8, 8)):
        R[c] = 1
    assert _both(R) == (6.0, 2, 2, 8, 8)
    # two diagonals of equal length: the upper-left one (the row-major first maximum)
    # (far enough apart that the first one's gap cells, 4 - 0.5 per step, have decayed to 0 before the second begins)
    R = np.zeros((40, 40), np.uint8)
    for d in range(4):
        R[2 + d, 2 + d] = R[25 + d, 30 + d] = 1
    assert _both(R) == (4.0, 2, 2, 5, 5)
    R = np.zeros((20, 20), np.uint8)
    for d in range(4):
        R[9 + d, 2 + d] = R[9 + d, 12 + d] = 1     # ... ending in the SAME row: the smaller column
    assert _both(R) == (4.0, 9, 2, 12, 5)
    # c2 and c3 tie at (6, 6): (5, 5) <- (4, 4) and (4, 5) <- (3, 4), both 2; c2's start is inherited
    R = np.zeros((9, 9), np.uint8)
    for c in ((4, 4), (5, 5), (3, 4), (4, 5), (6, 6)):
        R[c] = 1
    assert _both(R) == (3.0, 4, 4, 6, 6)
    assert _both(np.zeros((7, 9))) == ref.NO_MATCH
    for shape in ((2, 5), (5, 2), (1, 1), (2, 2)):
        assert _both(np.ones(shape)) == ref.NO_MATCH
    assert _both(np.ones((3, 3))) == (1.0, 2, 2, 2, 2)
    assert _both(np.ones((3, 3)), dp_start=3) == ref.NO_MATCH


def test_exports_named_in_header_and_shim():
    from acoss_amd import _lib
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    assert re.search(r"typedef struct \{ float score; int32_t q0, r0, q1, r1; \} acx_alignment;", header)
    assert re.search(r"\bint acx_serra09_align\(acx_ctx \*ctx, const int32_t \*pairs, int64_t K, const acx_serra09_params \*params, acx_alignment \*out\);", header)
    assert re.search(r"\bint acx_qmax_locate_binary\(acx_ctx \*ctx, const uint8_t \*R, int32_t M, int32_t N, const acx_serra09_params \*params,\s*acx_alignment \*out\);", header)
    assert re.search(r"#define ACX_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    for name in ("acx_serra09_align", "acx_qmax_locate_binary"):
        assert _lib.EXPORTS.count(name) == 1
    assert _lib.ALIGNMENT_DTYPE.names == ("score", "q0", "r0", "q1", "r1") and _lib.ALIGNMENT_DTYPE.itemsize == 20
    assert callable(_lib.Context.serra09_align) and callable(_lib.Context.qmax_locate_binary)


# ---------------------------------------------------------------------------------------------- argument checks
def _csv(tmp_path, n):
    path = tmp_path / "ds.csv"
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


class _NoDevice(object):
    """Stands where the class's libacx context would be: any use is a test failure."""
    def __getattr__(self, name):
        raise AssertionError("the library was reached (%s) before the arguments were checked" % name)


def _no_device(monkeypatch, tmp_path, n, **kw):
    from acoss_amd.algorithms import Serra09
    algo = Serra09(_csv(tmp_path, n), "feat/", shortname="align", **kw)
    algo._ctx = _NoDevice()
    monkeypatch.setattr(Serra09, "_context", lambda self: (_ for _ in ()).throw(AssertionError("pool upload before the argument checks")))
    return algo


def test_python_side_argument_errors_come_first(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo = _no_device(monkeypatch, tmp_path, 8)
    with pytest.raises(ValueError, match=r"idxs must be \(K, 2\)"):
        algo.align([0, 1, 2])
    with pytest.raises(ValueError, match=r"idxs must be \(K, 2\)"):
        algo.align([[0, 1, 2]])
    with pytest.raises(ValueError, match=r"track indices in \[0, 8\)"):
        algo.align([[0, 8]])
    with pytest.raises(ValueError, match=r"track indices in \[0, 8\)"):
        algo.align([[-1, 3]])
    with pytest.raises(ValueError, match="integers"):
        algo.align([[0.5, 1.0]])
    with pytest.raises(ValueError, match=r"one row per query \(2\)"):
        algo.align_matches([0, 3], [[1, 2], [3, 4], [5, 6]])
    with pytest.raises(ValueError, match=r"one row per query \(2\)"):
        algo.align_matches([0, 3], [1, 2])
    with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 8\)"):
        algo.align_matches([0, 8], [[1, 2], [3, 4]])
    with pytest.raises(ValueError, match=r"track indices in \[0, 8\) or -1"):
        algo.align_matches([0, 3], [[1, 8], [3, 4]])
    with pytest.raises(ValueError, match=r"track indices in \[0, 8\) or -1"):
        algo.align_matches([0, 3], [[1, -2], [3, 4]])
    with pytest.raises(ValueError, match="integers"):
        algo.align_matches([0, 3], [[1.0, 2.0], [3.0, 4.0]])
    # nothing to align: no library call either
    out = algo.align(np.zeros((0, 2), np.int64))
    assert out.shape == (0,) and out.dtype.names == ("score", "q0", "r0", "q1", "r1", "q_span", "r_span")
    out = algo.align_matches([0, 3], [[-1, -1], [-1, -1]])
    assert out.shape == (2, 2) and np.all(out["score"] == 0) and np.all(out["q0"] == -1) and np.all(out["r_span"] == -1)
    # valid arguments get past the checks, to the (absent) library
    with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
        algo.align([[0, 1]])
    with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
        algo.align_matches([0, 3], [[1, -1], [-1, 4]])
    dmax = _no_device(monkeypatch, tmp_path, 8, engine={"dmax": 1})
    with pytest.raises(ValueError, match="Qmax alignment only"):
        dmax.align([[0, 1]])
    with pytest.raises(ValueError, match="Qmax alignment only"):
        dmax.align_matches([0], [[1]])
    for a in (algo, dmax):
        a._ctx = None
        a.cleanup_memmap()
