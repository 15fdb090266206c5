"""
Host-side checks of fused scores for query shortlists (rerank_fused / rerank_tracks_fused / identify_cascade_fused,
acx_query_fused_lists): the ABI surface, the Python-side argument checks -- none of which may touch a GPU --, and the numpy
restatement of the definition (tests/_fused_ref.py) on oracle pair scores, pinned to the stage-by-stage specification of the
fusion kernels (tests/_snf_ref.py).
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from . import _fused_ref as fref
from . import _snf_ref
from .test_query_lists_host import _no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "acx_query_fused_lists"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_symbol_in_header_exports_and_library():
    from acoss_amd import _lib
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    assert re.search(r"\bint %s\(acx_ctx \*ctx, const acx_query_spec \*spec, const void \*params" % NAME, header)
    assert re.search(r"const acx_fused_spec \*fused, int32_t k,\s+int32_t \*out_idx, float \*out_score, uint8_t \*out_flag\);", header)
    assert _lib.EXPORTS.count(NAME) == 1
    assert re.search(r"#define ACX_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4, "additive: the ABI version stays"
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libacx.so is not built: build() comes before the tests")
    L = ctypes.CDLL(_lib.LIB_PATH)            # (no device is needed to look symbols up)
    assert hasattr(L, NAME)
    # the struct as the header lays it out: 15 ints, padding to 8, two doubles
    assert ctypes.sizeof(_lib.FusedSpec) == 80 and _lib.FusedSpec.reg_diag.offset == 64 and _lib.FusedSpec.reserved.offset == 56
    assert (_lib.FUSED_SQRTLEN, _lib.FUSED_INV1P) == (1, 2)
    assert re.search(r"#define ACX_FUSED_SQRTLEN 1\b", header) and re.search(r"#define ACX_FUSED_INV1P 2\b", header)


def test_signatures_and_class_tables():
    from acoss_amd import _lib
    from acoss_amd.algorithms import ChenFusion, EarlyFusion
    from acoss_amd.algorithms.algorithm_template import CoverAlgorithm
    sig = inspect.signature(CoverAlgorithm.rerank_fused)
    assert list(sig.parameters) == ["self", "queries", "shortlists", "k", "similarity_types", "K", "niters"]
    assert [sig.parameters[p].default for p in ("k", "similarity_types", "K", "niters")] == [10, None, 20, 20]
    sig = inspect.signature(CoverAlgorithm.rerank_tracks_fused)
    assert list(sig.parameters) == ["self", "tracks", "shortlists", "k", "similarity_types", "K", "niters"]
    assert list(inspect.signature(ChenFusion.rerank_tracks_fused).parameters)[-1] == "raw"
    sig = inspect.signature(CoverAlgorithm.identify_cascade_fused)
    assert list(sig.parameters) == ["self", "first", "queries", "k", "shortlist", "first_type", "similarity_types", "K", "niters"]
    # the planes and their ORDER are do_late_fusion's
    assert ChenFusion._fused_planes == {"Late": ("qmax", "dmax")} and ChenFusion._fused_transform == _lib.FUSED_SQRTLEN
    assert EarlyFusion._fused_planes == {"late": ("chromas", "ssms", "mfccs"), "early+late": ("chromas", "ssms", "mfccs", "early")}
    assert EarlyFusion._fused_transform == _lib.FUSED_INV1P
    for cls in (ChenFusion, EarlyFusion):
        assert tuple(cls._fused_planes) == cls._identify_fused
        assert all(p in cls._identify_planes for planes in cls._fused_planes.values() for p in planes)
    f = _lib.fused_spec([(2, 1, 0), (2, 1, 0, 3)], _lib.FUSED_INV1P)
    assert (f.n_types, list(f.count), list(f.planes[0]), list(f.planes[1])) == (2, [3, 4], [2, 1, 0, 0], [2, 1, 0, 3])
    assert (f.K, f.niters, f.reserved, f.reg_diag, f.mu) == (20, 20, 0, 1.0, 0.5)
    for bad in ([], [(0, 1)] * 3, [(0,)], [(0, 1, 2, 3, 0)]):
        with pytest.raises(ValueError):
            _lib.fused_spec(bad, _lib.FUSED_INV1P)


def _long_row(n, skip, length):
    return [t for t in range(n) if t != skip][:length]


@pytest.mark.parametrize("cls_name", ["ChenFusion", "EarlyFusion"])
def test_python_side_argument_errors_come_first(tmp_path, monkeypatch, cls_name):
    monkeypatch.chdir(tmp_path)
    n = 30
    algo = _no_device(monkeypatch, cls_name, tmp_path, n, "args")
    fused = algo._identify_fused[0]
    ok = [_long_row(n, 0, 21), _long_row(n, 3, 25)]
    with pytest.raises(ValueError, match="k must be >= 1"):
        algo.rerank_fused([0, 3], ok, k=0)
    with pytest.raises(ValueError, match=r"one row per query \(2\), got 3"):
        algo.rerank_fused([0, 3], ok + [[4]], k=3)
    with pytest.raises(ValueError, match=r"track indices in \[0, 30\) or -1"):
        algo.rerank_fused([0, 3], [ok[0], ok[1] + [30]], k=3)
    with pytest.raises(ValueError, match="row 1 lists track 5 twice"):
        algo.rerank_fused([0, 3], [ok[0], ok[1] + [5]], k=3)
    with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 30\)"):
        algo.rerank_fused([0, 30], ok, k=3)
    with pytest.raises(ValueError, match="unknown similarity type"):
        algo.rerank_fused([0, 3], ok, similarity_types=["nope"])
    with pytest.raises(ValueError, match="is not a fused type"):
        algo.rerank_fused([0, 3], ok, similarity_types=[algo._identify_planes[0]])
    with pytest.raises(ValueError, match="twice"):
        algo.rerank_fused([0, 3], ok, similarity_types=[fused, fused])
    with pytest.raises(ValueError, match="at least one fused type"):
        algo.rerank_fused([0, 3], ok, similarity_types=[])
    # n < K + 2, the row named: 20 other tracks and the query are 21; the query listed in its own row does not count twice
    with pytest.raises(ValueError, match=r"row 1 gives a neighbourhood of 21 tracks .* K \+ 2 = 22"):
        algo.rerank_fused([0, 3], [ok[0], _long_row(n, 3, 20)], k=3)
    with pytest.raises(ValueError, match=r"row 0 gives a neighbourhood of 21 tracks"):
        algo.rerank_fused([0, 3], [_long_row(n, 0, 20) + [0, -1], ok[1]], k=3)
    with pytest.raises(ValueError, match=r"row 0 gives a neighbourhood of 22 tracks .* K \+ 2 = 27"):
        algo.rerank_fused([0, 3], ok, K=25)
    with pytest.raises(ValueError, match="K must be >= 1"):
        algo.rerank_fused([0, 3], ok, K=0)
    with pytest.raises(NotImplementedError, match="64 neighbours"):
        algo.rerank_fused([0, 3], ok, K=65)
    with pytest.raises(ValueError, match="niters must be >= 1"):
        algo.rerank_fused([0, 3], ok, niters=0)
    with pytest.raises(NotImplementedError, match="more than 1024 entries"):
        algo.rerank_fused([0], [_long_row(n, 0, 29) + [-1] * 1000], k=3)
    # the plane methods keep refusing fused types, and say where they are served
    for call in (lambda: algo.rerank([0, 3], ok, similarity_types=[fused]), lambda: algo.identify([0], similarity_types=[fused]),
                 lambda: algo.evaluate(similarity_types=[fused])):
        with pytest.raises(NotImplementedError, match=r"whole N x N.*rerank_fused"):
            call()
    # a call that passes every check gets as far as the (absent) library
    with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
        algo.rerank_fused([0, 3], ok, k=3)
    with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
        algo.rerank_fused([0, 3], [_long_row(n, 0, 3), _long_row(n, 3, 4)], k=3, K=2, niters=1)

    first = _no_device(monkeypatch, "FTM2D", tmp_path, n, "first")
    other = _no_device(monkeypatch, "FTM2D", tmp_path, 6, "other")
    with pytest.raises(ValueError, match="first holds 6 tracks, this collection 30"):
        algo.identify_cascade_fused(other, [0, 3])
    for bad in (0, 1025):
        with pytest.raises(ValueError, match=r"shortlist must be in 1\.\.1024"):
            algo.identify_cascade_fused(first, [0, 3], shortlist=bad)
    with pytest.raises(ValueError, match="k must be >= 1"):
        algo.identify_cascade_fused(first, [0, 3], k=0, shortlist=25)
    with pytest.raises(ValueError, match=r"neighbourhoods below K \+ 2 = 22"):
        algo.identify_cascade_fused(first, [0, 3], shortlist=20)
    with pytest.raises(ValueError, match="is not a fused type"):
        algo.identify_cascade_fused(first, [0, 3], shortlist=25, similarity_types=[algo._identify_planes[0]])
    with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 30\)"):
        algo.identify_cascade_fused(first, [31], shortlist=25)
    with pytest.raises(ValueError, match="unknown similarity type"):
        algo.identify_cascade_fused(first, [0], shortlist=25, first_type="nope")

    rng = np.random.default_rng(1)
    if cls_name == "ChenFusion":
        new = [rng.random((40, 12)).astype(np.float32) for _ in range(2)]
    else:
        from acoss_amd import synth
        new = synth.earlyfusion_set(2, seed=2, nb_range=(20, 30))
    rows = [_long_row(n, -1, 21), _long_row(n, -1, 24)]
    with pytest.raises(ValueError, match="k must be >= 1"):
        algo.rerank_tracks_fused(new, rows, k=0)
    with pytest.raises(ValueError, match=r"one row per query \(2\), got 1"):
        algo.rerank_tracks_fused(new, rows[:1], k=3)
    with pytest.raises(ValueError, match=r"track indices in \[0, 30\) or -1"):
        algo.rerank_tracks_fused(new, [rows[0], rows[1] + [30]], k=3)          # (30 would be the first new track itself)
    with pytest.raises(ValueError, match=r"row 1 gives a neighbourhood of 21 tracks"):
        algo.rerank_tracks_fused(new, [rows[0], rows[1][:20]], k=3)
    with pytest.raises(ValueError, match="at least one track"):
        algo.rerank_tracks_fused([], [], k=3)
    with pytest.raises(NotImplementedError, match="64 neighbours"):
        algo.rerank_tracks_fused(new, rows, K=70)
    if cls_name == "ChenFusion":
        with pytest.raises(ValueError, match="niters must be >= 1"):
            algo.rerank_tracks_fused(new, rows, niters=0, raw=True)
    for a in (algo, first, other):
        a._ctx = None
        a.cleanup_memmap()


@pytest.mark.parametrize("cls_name", ["Serra09", "Simple", "FTM2D"])
def test_classes_without_fused_types_refuse_by_name(tmp_path, monkeypatch, cls_name):
    monkeypatch.chdir(tmp_path)
    algo = _no_device(monkeypatch, cls_name, tmp_path, 30, "plain")
    with pytest.raises(NotImplementedError, match="%s has no fused similarity type" % type(algo).__name__):
        algo.rerank_fused([0], [_long_row(30, 0, 25)])
    with pytest.raises(NotImplementedError, match="has no fused similarity type"):
        algo.rerank_tracks_fused([np.zeros((40, 12), np.float32)], [_long_row(30, -1, 25)])
    with pytest.raises(NotImplementedError, match="has no fused similarity type"):
        algo.identify_cascade_fused(algo, [0], shortlist=25)
    algo._ctx = None
    algo.cleanup_memmap()


# ---------------------------------------------------------------------------------------------- the definition in numpy
@pytest.fixture(scope="module")
def oracle_scores():
    """Qmax and Dmax of every pair of 12 short synthetic tracks on the CPU oracle: (12, 12, 2) f32, upper triangle."""
    import oracle
    from acoss_amd import synth
    d = synth.cover_set(clique_sizes=[2] * 6, seed=5, t_range=(60, 90))
    n = len(d["offsets"]) - 1
    pairs = oracle.all_pairs(n, True).astype(np.int32)
    S = np.zeros((n, n, 2), np.float32)
    for e in (0, 1):
        S[pairs[:, 0], pairs[:, 1], e] = oracle.serra09_pairs(d["frames"], d["offsets"], pairs, oracle.serra09_params(dmax=e))
    return S, np.sqrt(np.diff(d["offsets"]).astype(np.float64))


def _oracle_fuse(Ds, K, niters):
    import oracle
    return oracle.snf_fuse(Ds, K=K, niters=niters, reg_diag=1)[1]


def test_definition_on_oracle_scores_pinned_to_the_kernel_specification(oracle_scores):
    """oracle pair scores -> matrices -> oracle.snf_fuse -> row -> f32 -> stable order, and the same with the fusion of
    tests/_snf_ref.py (one numpy function per kernel) on the same matrices: the fused rows agree to the oracle's own distance
    from that specification (tests/test_snf_ref.py: rtol 1e-10), and where two neighbours' f32 scores differ the order agrees."""
    S, col = oracle_scores
    n = S.shape[0]
    assert np.all(S[np.triu_indices(n, 1)] > 0), "synthetic covers: no empty plot"
    score_pairs = lambda pr: S[pr[:, 0], pr[:, 1]]
    queries = [7, 2, 7, 11]
    lists = np.array([[3, -1, 0, 9, 11, 5, -1, 1], [11, 10, 9, 8, 7, 6, 5, 4], [1, 2, 3, 4, 5, 7, 6, -1], [-1, 0, 2, 4, 6, 8, 10, -1]])
    K, niters, k = 3, 4, 9
    assert [len(fref.neighbourhood(q, r)[0]) for q, r in zip(queries, lists)] == [7, 9, 7, 7]
    rows = {}

    def keep(tag, fuse):
        def f(Ds, K_, niters_):
            F = fuse(Ds, K_, niters_)
            rows.setdefault(tag, []).append(np.array(F))
            return F
        return f
    a = fref.rerank_fused(score_pairs, keep("oracle", _oracle_fuse), queries, lists, k, [(0, 1)], fref.SQRTLEN, col=col, K=K, niters=niters)
    b = fref.rerank_fused(score_pairs, keep("spec", lambda Ds, K_, n_: _snf_ref.fuse(Ds, K_, n_, 1)[1]), queries, lists, k, [(0, 1)],
                          fref.SQRTLEN, col=col, K=K, niters=niters)
    for Fo, Fs in zip(rows["oracle"], rows["spec"]):
        np.testing.assert_allclose(Fs, Fo, rtol=1e-10, atol=1e-14)
    assert not a[2].any() and not b[2].any()
    np.testing.assert_allclose(b[1], a[1], rtol=2e-7, equal_nan=True)          # f32 of values within 1e-10: one ulp at most
    for i in range(len(queries)):
        T, qpos = fref.neighbourhood(queries[i], lists[i])
        m = len(T) - 1
        assert np.all(a[0][i, 0, m:] == -1) and np.all(np.isnan(a[1][i, 0, m:])) and queries[i] not in a[0][i]
        assert sorted(a[0][i, 0, :m]) == sorted(t for t in T if t != queries[i])
        assert np.all(np.diff(a[1][i, 0, :m]) <= 0), "descending"
        if len(np.unique(a[1][i, 0, :m])) == m and np.array_equal(_bits(a[1][i]), _bits(b[1][i])):
            assert np.array_equal(a[0][i], b[0][i])
    # the order of the rows and of the entries means nothing; a duplicate query with another list is its own problem
    perm = [2, 0, 3, 1]
    rng = np.random.default_rng(0)
    c = fref.rerank_fused(score_pairs, _oracle_fuse, [queries[p] for p in perm], np.stack([rng.permutation(lists[p]) for p in perm]), k,
                          [(0, 1)], fref.SQRTLEN, col=col, K=K, niters=niters)
    assert np.array_equal(c[0], a[0][perm]) and np.array_equal(_bits(c[1]), _bits(a[1][perm]))
    assert not np.array_equal(a[0][0], a[0][2])


def test_definition_details():
    T, pos = fref.neighbourhood(5, [9, -1, 5, 2, -1, 7])
    assert T.tolist() == [2, 5, 7, 9] and pos == 1
    assert fref.triangle_pairs(T).tolist() == [[2, 5], [2, 7], [2, 9], [5, 7], [5, 9], [7, 9]]
    sc = np.array([[1, 10], [2, 20], [0, 30], [4, 40], [5, 50], [6, 60]], np.float32)
    col = np.sqrt(np.arange(12.0))
    D = fref.distances(sc, T, (1, 0), fref.SQRTLEN, col)
    assert len(D) == 2 and D[0][0, 1] == np.float64(np.float32(col[5] / 10.0)) and D[0][1, 0] == np.float64(np.float32(col[2] / 10.0))
    assert D[1][0, 3] == np.inf and D[1][3, 0] == np.inf and np.all(np.diag(D[1]) == 0) and fref.nonfinite_flag(D) == 1
    assert fref.nonfinite_flag(D[:1]) == 0
    E = fref.distances(sc, T, (0,), fref.INV1P)
    assert E[0][0, 3] == 1.0 and E[0][2, 3] == 1.0 / 7.0 and np.array_equal(E[0], E[0].T)
    # the order: larger first, -0.0 and +0.0 tie, ties by ascending index, NaN last, the tail -1 / NaN
    row = np.array([0.5, np.nan, -0.0, 9.0, 0.0, 0.5], np.float32)
    idx, s = fref.stable_topk(row, 3, np.array([10, 11, 12, 13, 14, 15]), 7)
    assert idx.tolist() == [10, 15, 12, 14, 11, -1, -1] and np.isnan(s[4:]).all() and s[0] == 0.5
