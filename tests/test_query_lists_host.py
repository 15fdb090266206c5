"""
Host-side checks of the rerank path (rerank / identify_cascade / rerank_tracks, acx_query_topk_lists): the ABI surface,
the Python-side argument checks -- none of which may touch a GPU --, the ragged-to-padded conversion of shortlists and
the numpy yardstick the GPU tests grade against (tests/_query_lists_ref.py).
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from . import _query_lists_ref as lref
from . import _rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "acx_query_topk_lists"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_symbol_in_header_exports_and_library():
    from acoss_amd import _lib
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    assert re.search(r"\bint %s\(acx_ctx \*ctx, const acx_query_spec \*spec, const void \*params" % NAME, header)
    assert _lib.EXPORTS.count(NAME) == 1
    assert re.search(r"#define ACX_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libacx.so is not built: build() comes before the tests")
    L = ctypes.CDLL(_lib.LIB_PATH)            # (no device is needed to look symbols up)
    assert hasattr(L, NAME)
    L.acx_abi_version.restype = ctypes.c_int
    assert L.acx_abi_version() == 4


def test_signatures():
    from acoss_amd import _lib
    from acoss_amd.algorithms import ChenFusion, Serra09
    from acoss_amd.algorithms.algorithm_template import CoverAlgorithm
    sig = inspect.signature(_lib.Context.query_topk_lists)
    assert list(sig.parameters) == ["self", "algo", "symmetric", "params", "queries", "lists", "k", "col", "col_mode"]
    assert sig.parameters["col"].default is None and sig.parameters["col_mode"].default == 0
    sig = inspect.signature(CoverAlgorithm.rerank)
    assert list(sig.parameters) == ["self", "queries", "shortlists", "k", "similarity_types"]
    assert sig.parameters["k"].default == 10 and sig.parameters["similarity_types"].default is None
    sig = inspect.signature(CoverAlgorithm.identify_cascade)
    assert list(sig.parameters) == ["self", "first", "queries", "k", "shortlist", "first_type", "similarity_types"]
    assert sig.parameters["k"].default == 10 and sig.parameters["shortlist"].default == 200
    assert sig.parameters["first_type"].default is None
    sig = inspect.signature(CoverAlgorithm.rerank_tracks)
    assert list(sig.parameters) == ["self", "tracks", "shortlists", "k", "similarity_types"]
    for cls in (Serra09, ChenFusion):
        sig = inspect.signature(cls.rerank_tracks)
        assert list(sig.parameters) == ["self", "tracks", "shortlists", "k", "similarity_types", "raw"]
        assert sig.parameters["raw"].default is False


# ---------------------------------------------------------------------------------------------- the yardstick
def _tied_matrix(rng, n, levels):
    D = rng.integers(0, levels, size=(n, n)).astype(np.float32)
    D[rng.random((n, n)) < 0.05] = -0.0
    D[rng.random((n, n)) < 0.03] = np.nan
    D[rng.random((n, n)) < 0.03] = -np.inf
    return D


def _random_lists(rng, n, queries, L):
    """Per query: a shuffled subset of the tracks (sometimes with the query itself) with empty slots anywhere."""
    lists = np.full((len(queries), L), -1, np.int64)
    for i in range(len(queries)):
        m = int(rng.integers(0, min(L, n) + 1))
        slots = rng.choice(L, size=m, replace=False)
        lists[i, slots] = rng.choice(n, size=m, replace=False)
    return lists


@pytest.mark.parametrize("seed", range(8))
def test_reference_agrees_with_rank_ref(seed):
    """The restatement against the yardstick of the ranking kernels on rows full of ties, signed zeros, NaN and -inf:
    a row's list is _rank_ref's FULL ordering of the row with everything removed that the row does not list."""
    rng = np.random.default_rng(500 + seed)
    n = int(rng.integers(5, 40))
    D = _tied_matrix(rng, n, levels=int(rng.integers(2, 6)))
    assert np.isnan(D).any() and np.isinf(D).any() and np.signbit(D[D == 0]).any()
    queries = rng.integers(0, n, size=int(rng.integers(1, 9)))
    L = int(rng.integers(1, n + 6))
    lists = _random_lists(rng, n, queries, L)
    full_i, full_s = _rank_ref.topk_rows(D, n - 1, rows=queries)
    for k in (1, 4, L + 5):
        gi, gs = lref.topk_lists(D[queries], queries, lists, k)
        assert gi.shape == (len(queries), k) and gi.dtype == np.int32 and gs.dtype == np.float32
        for r in range(len(queries)):
            keep = np.isin(full_i[r], lists[r][lists[r] >= 0])
            wi, ws = full_i[r][keep][:k], full_s[r][keep][:k]
            assert queries[r] not in gi[r]
            assert np.array_equal(gi[r, :len(wi)], wi) and np.array_equal(_bits(gs[r, :len(wi)]), _bits(ws))
            assert np.all(gi[r, len(wi):] == -1) and np.all(np.isnan(gs[r, len(wi):]))
    # the order within a row and the place of its empty slots mean nothing
    shuffled = np.stack([rng.permutation(row) for row in lists])
    a, b = lref.topk_lists(D[queries], queries, lists, 6), lref.topk_lists(D[queries], queries, shuffled, 6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def test_reference_col_modes_and_edges():
    rows = np.array([[4.0, 0.0, 9.0, 2.5], [1.0, 1.0, -0.0, 0.0]], np.float32)
    col = np.sqrt(np.array([3.0, 5.0, 7.0, 11.0]))
    idx, sc = lref.topk_lists(rows, [2, 0], [[3, -1, 1, 0, 2], [-1, -1, -1, -1, -1]], 4, col=col, col_mode=2)
    assert idx[0].tolist() == [0, 3, 1, -1] and sc[0, 2] == -np.inf and np.isnan(sc[0, 3])
    assert sc[0, 0] == -np.float32(col[0] / 4.0)
    assert np.all(idx[1] == -1) and np.all(np.isnan(sc[1]))
    idx, sc = lref.topk_lists(rows, [2, 0], [[3, 1], [3, 2]], 3)
    assert idx.tolist() == [[3, 1, -1], [2, 3, -1]], "-0.0 and +0.0 tie: ascending track index"
    idx, sc = lref.topk_lists(rows, [2, 0], np.zeros((2, 0), np.int64), 2)
    assert np.all(idx == -1) and np.all(np.isnan(sc))
    with pytest.raises(AssertionError):
        lref.topk_lists(rows, [2, 0], [[3, 3], [1, 2]], 2)


# ---------------------------------------------------------------------------------------------- ragged -> padded
def test_ragged_to_padded():
    from acoss_amd.algorithms.algorithm_template import shortlists_to_array
    a = shortlists_to_array("t", [[5, 2, 9], [], (4,), np.array([7, -1, 3, 1], np.int32)])
    assert a.dtype == np.int64 and a.tolist() == [[5, 2, 9, -1], [-1, -1, -1, -1], [4, -1, -1, -1], [7, -1, 3, 1]]
    assert shortlists_to_array("t", [[], []]).shape == (2, 0)
    assert shortlists_to_array("t", []).shape == (0, 0)
    b = np.array([[1, -1], [0, 2]], np.int16)
    assert np.array_equal(shortlists_to_array("t", b), b) and shortlists_to_array("t", b).dtype == np.int64
    assert shortlists_to_array("t", np.zeros((3, 0))).shape == (3, 0)
    with pytest.raises(ValueError, match=r"\(Q, L\)"):
        shortlists_to_array("t", np.arange(4))
    with pytest.raises(ValueError, match="integer"):
        shortlists_to_array("t", np.array([[0.5, 1.0]]))
    with pytest.raises(ValueError, match="integer"):
        shortlists_to_array("t", [[1, 2], [0.5]])
    with pytest.raises(ValueError, match="flat sequence"):
        shortlists_to_array("t", [[[1, 2]], [3]])
    with pytest.raises(ValueError, match="sequence of sequences"):
        shortlists_to_array("t", 7)


# ---------------------------------------------------------------------------------------------- argument checks
def _csv(tmp_path, n, tag="ds"):
    path = tmp_path / ("%s.csv" % tag)
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


class _NoDevice(object):
    """Stands where a class's libacx context would be: any use is a test failure."""
    def __getattr__(self, name):
        raise AssertionError("the library was reached (%s) before the arguments were checked" % name)


def _no_device(monkeypatch, cls_name, tmp_path, n, tag):
    from acoss_amd import algorithms
    cls = getattr(algorithms, cls_name)
    algo = cls(_csv(tmp_path, n, tag), "feat/", shortname=tag)
    algo._ctx = _NoDevice()                                   # nothing may get as far as a context
    monkeypatch.setattr(cls, "_context", lambda self: (_ for _ in ()).throw(AssertionError("pool upload before the argument checks")))
    return algo


@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion", "Simple", "EarlyFusion", "FTM2D"])
def test_python_side_argument_errors_come_first(tmp_path, monkeypatch, cls_name):
    monkeypatch.chdir(tmp_path)
    algo = _no_device(monkeypatch, cls_name, tmp_path, 8, "args")
    ok = [[1, 2, -1], [5, -1, 0]]
    with pytest.raises(ValueError, match="k must be >= 1"):
        algo.rerank([0, 3], ok, k=0)
    with pytest.raises(ValueError, match=r"one row per query \(2\), got 3"):
        algo.rerank([0, 3], ok + [[4]], k=3)
    with pytest.raises(ValueError, match=r"one row per query \(2\), got 1"):
        algo.rerank([0, 3], np.array([[1, 2]]), k=3)
    with pytest.raises(ValueError, match=r"track indices in \[0, 8\) or -1"):
        algo.rerank([0, 3], [[1, 8], [2]], k=3)
    with pytest.raises(ValueError, match=r"track indices in \[0, 8\) or -1"):
        algo.rerank([0, 3], [[1, -2], [2]], k=3)
    with pytest.raises(ValueError, match="row 1 lists track 5 twice"):
        algo.rerank([0, 3], [[1, 2, 3], [5, -1, 5]], k=3)
    with pytest.raises(ValueError, match="integer"):
        algo.rerank([0, 3], [[1.5], [2.0]], k=3)
    with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 8\)"):
        algo.rerank([0, 8], ok, k=3)
    with pytest.raises(ValueError, match="unknown similarity type"):
        algo.rerank([0, 3], ok, k=3, similarity_types=["nope"])
    for fused in algo._identify_fused:
        with pytest.raises(NotImplementedError, match="whole N x N"):
            algo.rerank([0, 3], ok, k=3, similarity_types=[fused])
    # two empty slots in a row are no duplicate: the call gets past the checks, to the (absent) library
    with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
        algo.rerank([0, 3], [[-1, -1, 2], [-1, -1, -1]], k=3)

    first = _no_device(monkeypatch, "FTM2D", tmp_path, 8, "first")
    other = _no_device(monkeypatch, "FTM2D", tmp_path, 6, "other")
    with pytest.raises(ValueError, match="first holds 6 tracks, this collection 8"):
        algo.identify_cascade(other, [0, 3])
    with pytest.raises(ValueError, match="first holds None tracks"):
        algo.identify_cascade(object(), [0, 3])
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError, match=r"shortlist must be in 1\.\.1024"):
            algo.identify_cascade(first, [0, 3], shortlist=bad)
    with pytest.raises(ValueError, match="k must be >= 1"):
        algo.identify_cascade(first, [0, 3], k=0)
    with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 8\)"):
        algo.identify_cascade(first, [9], shortlist=5)
    with pytest.raises(ValueError, match="unknown similarity type"):
        algo.identify_cascade(first, [0], shortlist=5, first_type="nope")
    with pytest.raises(ValueError, match="unknown similarity type"):
        algo.identify_cascade(first, [0], shortlist=5, similarity_types=["nope"])

    rng = np.random.default_rng(1)
    if cls_name in ("Serra09", "ChenFusion"):
        new = [rng.random((40, 12)).astype(np.float32) for _ in range(2)]
    elif cls_name == "Simple":
        new = [rng.random((12, 40)) for _ in range(2)]
    elif cls_name == "FTM2D":
        new = list(rng.standard_normal((2, 12 * int(algo.WIN))))
    else:
        from acoss_amd import synth
        new = synth.earlyfusion_set(2, seed=2, nb_range=(20, 30))
    with pytest.raises(ValueError, match="k must be >= 1"):
        algo.rerank_tracks(new, ok, k=0)
    with pytest.raises(ValueError, match=r"one row per query \(2\), got 3"):
        algo.rerank_tracks(new, ok + [[1]], k=3)
    with pytest.raises(ValueError, match=r"track indices in \[0, 8\) or -1"):
        algo.rerank_tracks(new, [[1, 8], [2]], k=3)          # (8 would be the first new track itself)
    with pytest.raises(ValueError, match="row 0 lists track 2 twice"):
        algo.rerank_tracks(new, [[2, 1, 2], [3]], k=3)
    with pytest.raises(ValueError, match="at least one track"):
        algo.rerank_tracks([], [], k=3)
    with pytest.raises(ValueError, match="unknown similarity type"):
        algo.rerank_tracks(new, ok, k=3, similarity_types=["nope"])
    if cls_name in ("Serra09", "ChenFusion"):
        with pytest.raises(ValueError, match="row 1 lists track 0 twice"):
            algo.rerank_tracks(new, [[2], [0, 0]], k=3, raw=True)
    for a in (algo, first, other):
        a._ctx = None
        a.cleanup_memmap()
