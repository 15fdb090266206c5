"""
Host-side checks of the query path (identify / query_rows, acx_query_scores / acx_query_topk): the ABI surface, the
Python-side argument checks -- none of which may touch a GPU -- and the numpy yardstick the GPU tests grade against.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from . import _query_ref
from . import _rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("acx_query_scores", "acx_query_topk")


def test_symbols_in_header_exports_and_library():
    from acoss_amd import _lib
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(acx_ctx \*" % name, header), name
        assert _lib.EXPORTS.count(name) == 1
    assert "typedef struct" in header and "} acx_query_spec;" in header
    assert re.search(r"#define ACX_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libacx.so is not built: build() comes before the tests")
    L = ctypes.CDLL(_lib.LIB_PATH)            # (no device is needed to look symbols up)
    for name in NEW:
        assert hasattr(L, name), name
    L.acx_abi_version.restype = ctypes.c_int
    assert L.acx_abi_version() == 4


def test_spec_struct_layout():
    from acoss_amd import _lib
    assert ctypes.sizeof(_lib.QuerySpec) == 16
    assert [f[0] for f in _lib.QuerySpec._fields_] == ["algo", "symmetric", "col_mode", "reserved"]
    assert all(f[1] is ctypes.c_int32 for f in _lib.QuerySpec._fields_)


def test_signatures():
    from acoss_amd import _lib
    from acoss_amd.algorithms.algorithm_template import CoverAlgorithm
    sig = inspect.signature(CoverAlgorithm.identify)
    assert list(sig.parameters) == ["self", "queries", "k", "candidates", "similarity_types"]
    assert sig.parameters["k"].default == 10 and sig.parameters["candidates"].default is None
    assert sig.parameters["similarity_types"].default is None
    sig = inspect.signature(CoverAlgorithm.query_rows)
    assert list(sig.parameters) == ["self", "queries", "similarity_types"] and sig.parameters["similarity_types"].default is None
    sig = inspect.signature(_lib.Context.query_scores)
    assert list(sig.parameters) == ["self", "algo", "symmetric", "params", "queries", "col", "col_mode"]
    assert sig.parameters["col"].default is None and sig.parameters["col_mode"].default == 0
    sig = inspect.signature(_lib.Context.query_topk)
    assert list(sig.parameters) == ["self", "algo", "symmetric", "params", "queries", "k", "candidates", "col", "col_mode"]
    assert sig.parameters["candidates"].default is None and sig.parameters["col_mode"].default == 0


def _csv(tmp_path, n):
    path = tmp_path / "ds.csv"
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


class _NoDevice(object):
    """Stands where a class's libacx context would be: any use is a test failure."""
    def __getattr__(self, name):
        raise AssertionError("the library was reached (%s) before the arguments were checked" % name)


def test_identify_without_grid_raises(tmp_path, monkeypatch):
    from acoss_amd.algorithms.algorithm_template import CoverAlgorithm
    monkeypatch.chdir(tmp_path)

    class Toy(CoverAlgorithm):
        def similarity(self, idxs):
            self.Ds["main"][idxs[:, 0], idxs[:, 1]] = 1.0

    toy = Toy(_csv(tmp_path, 6), name="Toy", datapath="feat/", shortname="t")
    with pytest.raises(NotImplementedError, match="_grid"):
        toy.identify([0, 1], k=2)
    with pytest.raises(NotImplementedError, match="_grid"):
        toy.query_rows([0])
    toy.cleanup_memmap()


@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion", "Simple", "EarlyFusion", "FTM2D"])
def test_python_side_argument_errors_come_first(tmp_path, monkeypatch, cls_name):
    from acoss_amd import algorithms
    monkeypatch.chdir(tmp_path)
    cls = getattr(algorithms, cls_name)
    algo = cls(_csv(tmp_path, 8), "feat/", shortname="args")
    algo._ctx = _NoDevice()                                   # nothing below may get as far as a context
    monkeypatch.setattr(cls, "_context", lambda self: (_ for _ in ()).throw(AssertionError("pool upload before the argument checks")))
    first = algo._identify_planes[0]
    with pytest.raises(ValueError, match="k must be >= 1"):
        algo.identify([0], k=0)
    with pytest.raises(ValueError, match="unknown similarity type"):
        algo.identify([0], k=3, similarity_types=["nope"])
    with pytest.raises(ValueError, match="unknown similarity type"):
        algo.query_rows([0], similarity_types=[first, "nope"])
    with pytest.raises(ValueError, match="strictly ascending"):
        algo.identify([0], k=3, candidates=[1, 3, 3])
    with pytest.raises(ValueError, match="strictly ascending"):
        algo.identify([0], k=3, candidates=[[4, 2], [5, 6]])  # flattened to 4, 2, 5, 6
    with pytest.raises(ValueError, match="candidates must be track indices"):
        algo.identify([0], k=3, candidates=[1, 8])
    with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 8\)"):
        algo.identify([0, 8], k=3)
    with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 8\)"):
        algo.query_rows([-1])
    with pytest.raises(ValueError, match="integer"):
        algo.identify([0.5], k=3)
    for fused in algo._identify_fused:
        with pytest.raises(NotImplementedError, match="whole N x N"):
            algo.identify([0], k=3, similarity_types=[fused])
    algo._ctx = None
    algo.cleanup_memmap()


def test_fused_types_are_named():
    from acoss_amd.algorithms import ChenFusion, EarlyFusion, Serra09, Simple, FTM2D
    assert ChenFusion._identify_fused == ("Late",) and ChenFusion._identify_planes == ("qmax", "dmax")
    assert EarlyFusion._identify_fused == ("late", "early+late")
    assert EarlyFusion._identify_planes == ("mfccs", "ssms", "chromas", "early")
    assert Serra09._identify_planes == Simple._identify_planes == FTM2D._identify_planes == ("main",)
    assert Simple._identify_symmetric is False and Serra09._identify_symmetric and EarlyFusion._identify_symmetric


def _tied_matrix(rng, n, levels):
    D = rng.integers(0, levels, size=(n, n)).astype(np.float32)
    D[rng.random((n, n)) < 0.05] = -0.0
    D[rng.random((n, n)) < 0.03] = np.nan
    D[rng.random((n, n)) < 0.03] = -np.inf
    return D


@pytest.mark.parametrize("seed", range(6))
def test_reference_agrees_with_rank_ref(seed):
    """The yardstick of tests/test_gpu_query.py against the yardstick of the ranking kernels, on matrices full of ties,
    signed zeros, NaN and -inf: without candidates they are the same statement and must give the same lists; with
    candidates the non-candidates are removed from _rank_ref's FULL ordering of the row."""
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(5, 40))
    D = _tied_matrix(rng, n, levels=int(rng.integers(2, 6)))
    queries = rng.integers(0, n, size=int(rng.integers(1, 9)))
    for k in (1, 3, n - 1, n + 4):
        gi, gs = _query_ref.topk(D[queries], queries, k)
        wi, ws = _rank_ref.topk_rows(D, k, rows=queries)
        assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
    cand = np.sort(rng.choice(n, size=max(1, n // 2), replace=False))
    full_i, full_s = _rank_ref.topk_rows(D, n - 1, rows=queries)
    for k in (1, 4, n + 2):
        gi, gs = _query_ref.topk(D[queries], queries, k, candidates=cand)
        for r in range(len(queries)):
            keep = np.isin(full_i[r], cand)
            wi, ws = full_i[r][keep][:k], full_s[r][keep][:k]
            assert np.array_equal(gi[r, :len(wi)], wi) and np.array_equal(gs[r, :len(wi)].view(np.uint32), ws.view(np.uint32))
            assert np.all(gi[r, len(wi):] == -1) and np.all(np.isnan(gs[r, len(wi):]))


def test_reference_col_modes():
    rows = np.array([[4.0, 0.0, 9.0, 2.5]], np.float32)
    col = np.sqrt(np.array([3.0, 5.0, 7.0, 11.0]))
    m1 = _query_ref.finish(rows, col, 1)
    m2 = _query_ref.finish(rows, col, 2)
    assert m1.dtype == np.float32 and m2.dtype == np.float32
    assert np.array_equal(m1, (rows.astype(np.float64) / col).astype(np.float32))
    assert m2[0, 1] == -np.inf and m2[0, 0] == -np.float32(col[0] / 4.0)
    idx, sc = _query_ref.topk(rows, [2], 4, col=col, col_mode=2)
    assert idx[0].tolist() == [0, 3, 1, -1] and sc[0, 2] == -np.inf and np.isnan(sc[0, 3])
    assert np.array_equal(_query_ref.scores(rows, [2], col, 1)[0, [2]], [0.0])
