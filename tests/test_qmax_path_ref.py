"""
CPU tests of the Qmax alignment PATH's yardstick (tests/_qmax_path_ref.py) and of the BOX PROPERTY that licenses the design of
qmax_path_kernel: the DP on the cells of the reported box alone, with 0 for every Q outside it, gives the
cells of the full matrix's traceback and the same Q on every one of them.

The last tests hold the library's surface against the yardstick's: they fail where the exports and methods are missing.
"""
import numpy as np
import pytest

from tests import _qmax_locate_ref as loc
from tests import _qmax_path_ref as ref

GAMMAS = ((0.5, 0.5), (0.5, 0.7), (1.0, 0.25))
DENSITIES = (0.2, 0.5, 0.8)
STEP_SET = {(1, 1), (2, 1), (1, 2)}


def _check_plot(R, go, ge, st):
    """Every property the issue lists, on one plot; returns whether the plot has a match."""
    rec, cells, q = ref.path_full(R, go, ge, st)
    assert rec == loc.locate_forward(R, go, ge, st), "the endpoints are locate_forward's"
    if rec == ref.NO_MATCH:
        assert len(cells) == 0 and len(q) == 0
        assert ref.path_box(R, rec, go, ge, st)[0] == ref.NO_MATCH
        return False
    brec, bcells, bq = ref.path_box(R, rec, go, ge, st)
    assert np.array_equal(cells, bcells), "the box path is the full matrix's path"
    assert np.array_equal(q.view(np.uint32), bq.view(np.uint32)), "Q is identical on the path cells"
    assert brec == rec
    assert tuple(cells[0]) == rec[1:3] and tuple(cells[-1]) == rec[3:5]
    assert {tuple(d) for d in np.diff(cells, axis=0)} <= STEP_SET
    assert len(cells) <= min(rec[3] - rec[1], rec[4] - rec[2]) + 1
    assert q[0] == 1 and q[-1] == np.float32(rec[0])
    return True


@pytest.mark.parametrize("st", (2, 3))
@pytest.mark.parametrize("gammas", GAMMAS)
def test_box_property_on_random_plots(gammas, st):
    """60 plots per (gammas, dp_start): 360 in all, sides 3 .. 40, three densities."""
    rng = np.random.default_rng([17, st, int(8 * gammas[0]), int(100 * gammas[1])])
    matched = 0
    for t in range(60):
        M, N = (int(v) for v in rng.integers(3, 41, 2))
        R = (rng.random((M, N)) < DENSITIES[t % 3]).astype(np.uint8)
        matched += _check_plot(R, gammas[0], gammas[1], st)
    assert matched >= 50, "nearly every plot has a match: %d of 60" % matched


def test_no_match_gives_an_empty_path():
    for st in (2, 3):
        assert not _check_plot(np.zeros((7, 9), np.uint8), 0.5, 0.5, st)
        for shape in ((2, 5), (5, 2), (1, 1), (2, 2)):
            assert not _check_plot(np.ones(shape, np.uint8), 1.0, 0.25, st)


def test_hand_checked_plots():
    for name, R, (go, ge, st), rec, cells in ref.HAND:
        got = ref.path_full(R, go, ge, st)
        assert got[0] == rec and [tuple(c) for c in got[1]] == cells, (name, got)
        assert _check_plot(R, go, ge, st), name


def test_tie_between_c2_and_c3_takes_c2():
    name, R, (go, ge, st), rec, cells = ref.HAND[3]
    Q = ref.full_matrix(R, go, ge, st)
    assert Q[4, 4] == Q[3, 4] == 1 and Q[5, 5] == Q[4, 5] == 2, "the ties the plot was built for"
    assert [tuple(c) for c in ref.path_full(R, go, ge, st)[1]] == [(4, 4), (5, 5), (6, 6)]


# ---- the library's surface (no device needed) ---------------------------------------------------------------------------------------------
def test_exports_and_header_name_the_path_calls():
    import os
    from acoss_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "acx.h")).read()
    for name in ("acx_serra09_align_paths", "acx_qmax_path_binary"):
        assert name in _lib.EXPORTS and ("int %s(" % name) in header
    L = _lib.load()
    assert hasattr(L, "acx_serra09_align_paths") and hasattr(L, "acx_qmax_path_binary")
    assert _lib.ABI_VERSION == 4


def test_python_methods_exist_and_check_their_arguments_first(tmp_path, monkeypatch):
    """align_paths / align_match_paths refuse bad arguments with _check_align's wording before any library call (no device here)."""
    from acoss_amd import _lib
    from acoss_amd.algorithms import ChenFusion, Serra09
    for cls in (Serra09, ChenFusion):
        assert callable(cls.align_paths) and callable(cls.align_match_paths)
    assert callable(_lib.Context.serra09_align_paths) and callable(_lib.Context.qmax_path_binary)
    monkeypatch.chdir(tmp_path)
    csv = tmp_path / "d.csv"
    csv.write_text("work_id,track_id\nw0,t0\nw0,t1\n")
    tracks = [np.random.default_rng(k).random((40, 12)).astype(np.float32) for k in range(2)]
    algo = Serra09(str(csv), "feat/", shortname="pathargs")
    try:
        algo.set_pooled_features(tracks, ["w0", "w0"])
        with pytest.raises(ValueError, match="align_paths: idxs must be \\(K, 2\\)"):
            algo.align_paths([0, 1, 0])
        with pytest.raises(ValueError, match="align_paths: idxs must be track indices in \\[0, 2\\)"):
            algo.align_paths([[0, 2]])
        with pytest.raises(ValueError, match="align_paths: track indices must be integers"):
            algo.align_paths([[0.0, 1.0]])
        with pytest.raises(ValueError, match="align_match_paths: indices must be \\(Q, k\\)"):
            algo.align_match_paths([0, 1], [[1]])
        with pytest.raises(ValueError, match="align_match_paths: indices must be track indices in \\[0, 2\\) or -1"):
            algo.align_match_paths([0], [[-2]])
        assert algo._ctx is None, "no library call was made"
    finally:
        algo.cleanup_memmap()
    algo = Serra09(str(csv), "feat/", shortname="pathargs2", engine={"dmax": 1})
    try:
        algo.set_pooled_features(tracks, ["w0", "w0"])
        with pytest.raises(ValueError, match="align_paths: the Qmax alignment only"):
            algo.align_paths([[0, 1]])
        with pytest.raises(ValueError, match="align_match_paths: the Qmax alignment only"):
            algo.align_match_paths([0], [[1]])
    finally:
        algo.cleanup_memmap()
