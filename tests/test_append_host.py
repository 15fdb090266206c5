"""
Host-side checks of the append path (acx_pool_append & co., identify_tracks / score_tracks): the ABI surface and the
Python-side argument checks, none of which may create a context or touch a GPU.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("acx_pool_append", "acx_pool_append_raw", "acx_pool_append_f64", "acx_ef_pool_append", "acx_ftm2d_append_shingles",
       "acx_pool_truncate")


def test_symbols_in_header_exports_and_library():
    from acoss_amd import _lib
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(acx_ctx \*" % name, header), name
        assert _lib.EXPORTS.count(name) == 1
    assert re.search(r"#define ACX_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libacx.so is not built: build() comes before the tests")
    L = ctypes.CDLL(_lib.LIB_PATH)            # (no device is needed to look symbols up)
    for name in NEW:
        assert hasattr(L, name), name


def test_ctypes_prototypes():
    from acoss_amd import _lib
    L = _lib.load()
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    vp, fp, dp, lp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)
    want = {"acx_pool_append": [vp, fp, lp, i32, i32],
            "acx_pool_append_raw": [vp, fp, lp, i32, i32, i32, lp],
            "acx_pool_append_f64": [vp, dp, lp, i32, i32],
            "acx_ef_pool_append": [vp, fp, fp, fp, dp, lp, i32],
            "acx_ftm2d_append_shingles": [vp, dp, i32, i32],
            "acx_pool_truncate": [vp, i32, i32]}
    assert sorted(want) == sorted(NEW)
    for name, argtypes in want.items():
        assert list(getattr(L, name).argtypes) == argtypes, name


def test_signatures():
    from acoss_amd import _lib
    from acoss_amd.algorithms.algorithm_template import CoverAlgorithm
    sig = inspect.signature(CoverAlgorithm.identify_tracks)
    assert list(sig.parameters) == ["self", "tracks", "k", "candidates", "similarity_types"]
    assert sig.parameters["k"].default == 10 and sig.parameters["candidates"].default is None
    sig = inspect.signature(CoverAlgorithm.score_tracks)
    assert list(sig.parameters) == ["self", "tracks", "similarity_types"]
    for name, params in (("pool_append", ["self", "frames", "offsets"]), ("pool_append_raw", ["self", "raw", "raw_offsets", "fac"]),
                         ("pool_append_f64", ["self", "frames", "offsets"]), ("ef_pool_append", ["self", "tracks"]),
                         ("ftm2d_append_shingles", ["self", "shingles"]), ("pool_truncate", ["self", "algo", "n_tracks"])):
        assert list(inspect.signature(getattr(_lib.Context, name)).parameters) == params, name


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


def _good_and_bad(cls_name):
    """-> (a well-formed track, [(bad track list, message pattern)])"""
    rng = np.random.default_rng(5)
    if cls_name in ("Serra09", "ChenFusion"):
        good = rng.random((40, 12)).astype(np.float32)
        return good, [([rng.random((40, 11)).astype(np.float32)], r"\(T, 12\)"), ([rng.random(12).astype(np.float32)], r"\(T, 12\)"),
                      ([good, np.ones((40, 12), np.int32)], "track 1 must be floating-point")]
    if cls_name == "Simple":
        good = rng.random((12, 40))
        return good, [([rng.random((40, 12))], r"\(12, n\)"), ([good, np.ones((12, 40), np.int64)], "track 1 must be floating-point")]
    if cls_name == "EarlyFusion":
        good = dict(mfccs=np.zeros((5, 650), np.float32), ssms=np.zeros((5, 1225), np.float32), chromas=np.zeros((5, 480), np.float32),
                    chroma_med=np.zeros(12))
        return good, [([dict(good, ssms=np.zeros((4, 1225), np.float32))], "same number of blocks"),
                      ([{k: v for k, v in good.items() if k != "chroma_med"}], "dict of block features"),
                      ([good, dict(good, mfccs=np.zeros((5, 600), np.float32))], "track 1: block-feature widths"),
                      ([dict(good, chroma_med=np.zeros(11))], "12 values"), ([dict(good, chromas=np.zeros((5, 480), np.int32))], "floating-point")]
    good = rng.standard_normal(36)
    return good, [([rng.standard_normal(24)], r"\(36,\) shingle"), ([rng.standard_normal((1, 36))], r"\(36,\) shingle"),
                  ([good, np.ones(36, np.int64)], "track 1 must be a floating-point")]


@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion", "Simple", "EarlyFusion", "FTM2D"])
def test_python_side_argument_errors_come_first(tmp_path, monkeypatch, cls_name):
    from acoss_amd import _lib, algorithms
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a context was created before the argument checks")))
    cls = getattr(algorithms, cls_name)
    kw = dict(WIN=3) if cls_name == "FTM2D" else {}
    algo = cls(_csv(tmp_path, 8), "feat/", shortname="args", **kw)
    algo._ctx = _NoDevice()
    monkeypatch.setattr(cls, "_context", lambda self: (_ for _ in ()).throw(AssertionError("pool upload before the argument checks")))
    good, bad = _good_and_bad(cls_name)
    for fn in (algo.identify_tracks, algo.score_tracks):
        with pytest.raises(ValueError, match="at least one track"):
            fn([])
        with pytest.raises(ValueError, match="unknown similarity type"):
            fn([good], similarity_types=["nope"])
        for tracks, pattern in bad:
            with pytest.raises(ValueError, match=pattern):
                fn(tracks)
        for fused in algo._identify_fused:
            with pytest.raises(NotImplementedError, match="whole N x N"):
                fn([good], similarity_types=[fused])
    with pytest.raises(ValueError, match="k must be >= 1"):
        algo.identify_tracks([good], k=0)
    with pytest.raises(ValueError, match="strictly ascending"):
        algo.identify_tracks([good], candidates=[1, 3, 3])
    with pytest.raises(ValueError, match=r"candidates must be tracks of the collection, indices in \[0, 8\)"):
        algo.identify_tracks([good], candidates=[1, 8])          # 8 would be the new track itself
    with pytest.raises(ValueError, match="integer"):
        algo.identify_tracks([good], candidates=[0.5])
    assert algo.N == 8
    algo._ctx = None
    algo.cleanup_memmap()


def test_tracks_without_grid_raise(tmp_path, monkeypatch):
    from acoss_amd.algorithms.algorithm_template import CoverAlgorithm
    monkeypatch.chdir(tmp_path)

    class Toy(CoverAlgorithm):
        def similarity(self, idxs):
            self.Ds["main"][idxs[:, 0], idxs[:, 1]] = 1.0

    toy = Toy(_csv(tmp_path, 6), name="Toy", datapath="feat/", shortname="t")
    with pytest.raises(NotImplementedError, match="_grid"):
        toy.identify_tracks([np.zeros((20, 12), np.float32)], k=2)
    with pytest.raises(NotImplementedError, match="_grid"):
        toy.score_tracks([np.zeros((20, 12), np.float32)])
    toy.cleanup_memmap()
