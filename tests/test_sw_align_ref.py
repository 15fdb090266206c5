"""
Host-side checks of the EarlyFusion alignment (EarlyFusion.align / align_paths / align_matches / align_match_paths, acx_ef_align,
acx_sw_align_binary): the two restatements of the contract in tests/_sw_align_ref.py against each other, against the score of
tests/_ef_backend_ref.py::sw_tenths and of the CPU oracle, and against hand-checked answers; the ABI surface; the Python-side
argument checks, none of which may touch a GPU.
"""
import os
import re

import numpy as np
import pytest

from . import _ef_backend_ref as backend
from . import _sw_align_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSITIES = (0.05, 0.1, 0.5, 0.9)


def _both(B):
    a, ca = ref.align_traceback(B)
    b, cb = ref.align_forward(B)
    assert a == b and np.array_equal(ca, cb), "traceback %s %s vs forward %s %s for a %s plot" % (a, ca.tolist(), b, cb.tolist(), np.shape(B))
    assert ca.dtype == np.int32 and ca.ndim == 2 and ca.shape[1] == 2
    ref.check_path(b, cb, np.shape(B))
    return b, cb


def _tenths(rec):
    return int(round(float(rec[0]) * 10))


@pytest.mark.parametrize("density", DENSITIES)
def test_the_two_statements_agree_and_score_as_the_oracle(density):
    import oracle
    rng = np.random.default_rng(1900 + int(100 * density))
    shapes = [(4, 4), (4, 40), (40, 4), (40, 40), (5, 4), (4, 5)]
    ties = 0
    for n in range(80):                            # 4 x 80 plots
        M, N = shapes[n] if n < len(shapes) else (int(rng.integers(4, 41)), int(rng.integers(4, 41)))
        B = ref.random_plot(rng, M, N, density)
        rec, cells = _both(B)
        want = oracle.sw_constrained_i32(B)
        assert backend.sw_tenths(B) == want == _tenths(rec), (M, N, density, rec)
        assert np.float32(rec[0]).view(np.uint32) == (np.float32(want) / np.float32(10)).view(np.uint32)
        # a 1 anywhere in the counted interior scores at least 10 - 7: every random plot has a match
        assert want >= 3 and rec != ref.NO_MATCH and len(cells) >= 1
        assert B[rec[1], rec[2]] == 1, "a path starts at a 1: a chain that begins at 0 needs + 10"
        ties += len(cells) > 2
    assert ties > 0


def test_hand_checked_answers():
    for name, B, want, cells in ref.hand_checked():
        rec, got = _both(B)
        assert rec == want and np.array_equal(got, cells), (name, rec, got.tolist())
        assert backend.sw_tenths(B) == _tenths(rec), name


def test_no_match_plots():
    for B in ref.no_match_plots():
        rec, cells = _both(B)
        assert rec == ref.NO_MATCH and cells.shape == (0, 2), B.shape
        assert backend.sw_tenths(B) == 0


def test_step_set_and_length_bound_on_dense_plots():
    """Dense plots are where predecessors tie and paths run the whole shorter side."""
    rng = np.random.default_rng(77)
    longest = 0
    for M, N in ((40, 12), (12, 40), (33, 33), (40, 40)):
        for density in (0.5, 0.9, 1.0):
            B = (rng.random((M, N)) < density).astype(np.uint8)
            rec, cells = _both(B)
            assert len(cells) <= min(M, N) - 3            # rows / columns 0, 1 and the last one hold no cell
            longest = max(longest, len(cells))
    assert longest == 37                                   # ones((40, 40)): the diagonal (2, 2) .. (38, 38)


def test_exports_named_in_header_and_shim():
    from acoss_amd import _lib
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert ("int acx_ef_align(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_ef_params *params, int32_t plane , "
            "acx_alignment *out , int64_t *path_off , int32_t *cells , int64_t cap);") in flat
    assert ("int acx_sw_align_binary(acx_ctx *ctx, const uint8_t *B, int32_t M, int32_t N, acx_alignment *out, int32_t *cells, "
            "int64_t cap, int64_t *n_cells);") in flat
    assert re.search(r"#define ACX_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    for name in ("acx_ef_align", "acx_sw_align_binary"):
        assert _lib.EXPORTS.count(name) == 1
    assert callable(_lib.Context.ef_align) and callable(_lib.Context.sw_align_binary)


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
    from acoss_amd.algorithms import EarlyFusion
    algo = EarlyFusion(_csv(tmp_path, n), "feat/", shortname="efalign", **kw)
    algo._ctx = _NoDevice()
    monkeypatch.setattr(EarlyFusion, "_context", lambda self: (_ for _ in ()).throw(AssertionError("pool upload before the argument checks")))
    return algo


FIELDS = ("score", "q0", "r0", "q1", "r1", "q_span", "r_span")


def test_python_side_argument_errors_come_first(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo = _no_device(monkeypatch, tmp_path, 8)
    for fn in (algo.align, algo.align_paths):
        with pytest.raises(ValueError, match=r"idxs must be \(K, 2\)"):
            fn([0, 1, 2])
        with pytest.raises(ValueError, match=r"idxs must be \(K, 2\)"):
            fn([[0, 1, 2]])
        with pytest.raises(ValueError, match=r"track indices in \[0, 8\)"):
            fn([[0, 8]])
        with pytest.raises(ValueError, match=r"track indices in \[0, 8\)"):
            fn([[-1, 3]])
        with pytest.raises(ValueError, match="integers"):
            fn([[0.5, 1.0]])
    for fn in (algo.align_matches, algo.align_match_paths):
        with pytest.raises(ValueError, match=r"one row per query \(2\)"):
            fn([0, 3], [[1, 2], [3, 4], [5, 6]])
        with pytest.raises(ValueError, match=r"one row per query \(2\)"):
            fn([0, 3], [1, 2])
        with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 8\)"):
            fn([0, 8], [[1, 2], [3, 4]])
        with pytest.raises(ValueError, match=r"track indices in \[0, 8\) or -1"):
            fn([0, 3], [[1, 8], [3, 4]])
        with pytest.raises(ValueError, match=r"track indices in \[0, 8\) or -1"):
            fn([0, 3], [[1, -2], [3, 4]])
        with pytest.raises(ValueError, match="integers"):
            fn([0, 3], [[1.0, 2.0], [3.0, 4.0]])
    # similarity_type: the four device planes only (None: the default, 'early'), checked before the indices
    for bad in ("late", "early+late", "nope", 3):
        with pytest.raises(ValueError, match="similarity_type must be one of"):
            algo.align([[0, 99]], similarity_type=bad)
        with pytest.raises(ValueError, match="similarity_type must be one of"):
            algo.align_paths([[0, 1]], similarity_type=bad)
        with pytest.raises(ValueError, match="similarity_type must be one of"):
            algo.align_matches([0], [[1]], similarity_type=bad)
        with pytest.raises(ValueError, match="similarity_type must be one of"):
            algo.align_match_paths([0], [[1]], similarity_type=bad)
    # nothing to align: no library call either
    out = algo.align(np.zeros((0, 2), np.int64))
    assert out.shape == (0,) and out.dtype.names == FIELDS
    al, paths = algo.align_paths(np.zeros((0, 2), np.int64), similarity_type="mfccs")
    assert al.shape == (0,) and al.dtype.names == FIELDS and paths == []
    out = algo.align_matches([0, 3], [[-1, -1], [-1, -1]])
    assert out.shape == (2, 2) and np.all(out["score"] == 0) and np.all(out["q0"] == -1) and np.all(out["r_span"] == -1)
    out, paths = algo.align_match_paths([0, 3], [[-1, -1], [-1, -1]], similarity_type="chromas")
    assert out.shape == (2, 2) and np.all(out["q_span"] == -1)
    assert [[p.shape for p in row] for row in paths] == [[(0, 2)] * 2] * 2
    # valid arguments get past the checks, to the (absent) library
    for plane in ("mfccs", "ssms", "chromas", "early"):
        with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
            algo.align([[0, 1]], similarity_type=plane)
    with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
        algo.align_paths([[0, 1]])
    with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
        algo.align_matches([0, 3], [[1, -1], [-1, 4]])
    with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
        algo.align_match_paths([0, 3], [[1, -1], [-1, 4]])
    algo._ctx = None
    algo.cleanup_memmap()


def test_serra09_keeps_its_checks_through_the_shared_module(tmp_path, monkeypatch):
    """The checks moved to acoss_amd/algorithms/_align.py: Serra09's methods reach them with the same order and messages."""
    from acoss_amd.algorithms import Serra09, _align
    monkeypatch.chdir(tmp_path)
    algo = Serra09(_csv(tmp_path, 8), "feat/", shortname="shared", engine={"dmax": 1})
    with pytest.raises(ValueError, match="Qmax alignment only"):
        algo._check_align_pairs("align", [[0.5, 99]])            # the engine check still comes before dtype and range
    algo._engine = {}
    assert algo._check_align_pairs("align", [[0, 7]]).dtype == np.int32
    idx, rows, slots, pairs = algo._check_align_matches("align_matches", [0, 3], [[1, -1], [-1, 4]])
    assert pairs.tolist() == [[0, 1], [3, 4]] and rows.tolist() == [0, 1] and slots.tolist() == [0, 1]
    assert algo._no_match_rows((2,)).dtype == Serra09.ALIGN_DTYPE and np.all(algo._no_match_rows((2,))["q_span"] == -1)
    assert _align.no_match_rows((1,), Serra09.ALIGN_DTYPE)["score"][0] == 0
    algo.cleanup_memmap()
