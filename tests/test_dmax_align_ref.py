"""
CPU tests of the Dmax alignment's yardstick (tests/_dmax_align_ref.py) and of the BOX PROPERTY that licenses dmax_path_kernel (DESIGN.md
section 22): the Dmax DP on the cells of the reported box alone, with 0 for every Q outside it and R read AS IT IS outside it, gives the
cells of the full matrix's traceback and the same Q on every one of them.

The last tests hold the library's surface against the yardstick's: they fail where the exports, methods and the keyword are missing.
"""
import numpy as np
import pytest

import oracle
from tests import _dmax_align_ref as ref
from tests import _qmax_locate_ref as qloc
from tests import _qmax_path_ref as qpath

DENSITIES = (0.1, 0.3, 0.6)
STEP_SET = {(1, 1), (2, 1), (1, 2)}


def _check_plot(R, go, ge, st):
    """Every property on one plot; returns (has a match, the Dmax record differs from the Qmax record, the start is a gap cell,
    the start's Q is not 1)."""
    rec, cells, q = ref.dmax_full(R, go, ge, st)
    assert rec == ref.dmax_forward(R, go, ge, st), "(a) and (b) agree on the record"
    Rd = R[:-1, :-1] if st == 3 else R          # (the oracle's DP on a given plot starts at 2: dp_start 3 is the plot less its last row / column)
    want = oracle.qmax_binary(Rd, go, ge, dmax=True) if min(Rd.shape) > 0 else 0.0
    assert np.float32(rec[0]).view(np.uint32) == np.float32(want).view(np.uint32), "the score is the oracle's Dmax, bit for bit"
    qrec = qloc.locate_traceback(R, go, ge, st)
    # the bonus switched off: both references are the Qmax references
    off_rec, off_cells, off_q = ref.dmax_full(R, go, ge, st, bonus=False)
    assert off_rec == qrec == ref.dmax_forward(R, go, ge, st, bonus=False)
    pf = qpath.path_full(R, go, ge, st)
    assert np.array_equal(off_cells, pf[1]) and np.array_equal(off_q.view(np.uint32), pf[2].view(np.uint32))
    bo = ref.dmax_box(R, off_rec, go, ge, bonus=False)
    pb = qpath.path_box(R, pf[0], go, ge, st)
    assert bo[0] == pb[0] and np.array_equal(bo[1], pb[1]) and np.array_equal(bo[2].view(np.uint32), pb[2].view(np.uint32))
    if rec == ref.NO_MATCH:
        assert len(cells) == 0 and len(q) == 0
        assert ref.dmax_box(R, rec, go, ge)[0] == ref.NO_MATCH
        return False, rec != qrec, False, False
    brec, bcells, bq = ref.dmax_box(R, rec, go, ge)
    assert np.array_equal(cells, bcells), "the box path is the full matrix's path"
    assert np.array_equal(q.view(np.uint32), bq.view(np.uint32)), "Q is identical on the path cells"
    assert brec == rec
    assert tuple(cells[0]) == rec[1:3] and tuple(cells[-1]) == rec[3:5]
    assert {tuple(d) for d in np.diff(cells, axis=0)} <= STEP_SET
    assert len(cells) <= min(rec[3] - rec[1], rec[4] - rec[2]) + 1
    assert q[-1] == np.float32(rec[0]) and q[0] > 0
    return True, rec != qrec, R[rec[1], rec[2]] == 0, q[0] != 1


def test_box_property_on_random_plots():
    """60 plots per (gammas, dp_start): 360 in all, sides 3 .. 40, three densities."""
    total = matched = differ = gaps = not1 = 0
    for gammas in ref.GAMMAS:
        for st in (2, 3):
            rng = np.random.default_rng([23, st, int(8 * gammas[0]), int(100 * gammas[1])])
            for t in range(60):
                M, N = (int(v) for v in rng.integers(3, 41, 2))
                hit, d, g, n1 = _check_plot(ref.random_plot(rng, M, N, DENSITIES[t % 3]), gammas[0], gammas[1], st)
                total += 1; matched += hit; differ += d; gaps += g; not1 += n1
    print("%d of %d plots matched; %d Dmax records differ from the Qmax record; gap starts %.1f %%, starts with Q != 1 %.1f %% of the matched"
          % (matched, total, differ, 100.0 * gaps / matched, 100.0 * not1 / matched))
    assert matched >= 300, "nearly every plot has a match: %d of %d" % (matched, total)
    assert 4 * differ >= 3 * total, "a device run that silently took Qmax cannot pass: only %d of %d records differ" % (differ, total)


def test_no_match_gives_an_empty_path():
    for st in (2, 3):
        assert not _check_plot(np.zeros((7, 9), np.uint8), 0.5, 0.5, st)[0]
        for shape in ((2, 5), (5, 2), (1, 1), (2, 2)):
            assert not _check_plot(np.ones(shape, np.uint8), 1.0, 0.25, st)[0]


def test_hand_checked_plots():
    for name, R, (go, ge, st), rec, cells, qs in ref.HAND:
        got = ref.dmax_full(R, go, ge, st)
        assert got[0] == rec and [tuple(c) for c in got[1]] == cells and got[2].tolist() == [float(v) for v in qs], (name, got)
        assert _check_plot(R, go, ge, st)[0], name


def test_hand_checked_plots_cover_what_qmax_cannot_do():
    by = {h[0]: h for h in ref.HAND}
    # the start holds 2, and the Qmax alignment of the same plot is another one
    name, R, (go, ge, st), rec, cells, qs = by["a start with Q = 2"]
    assert qs[0] == 2 and qloc.locate_traceback(R, go, ge, st) != rec
    # a gap start: R is 0 at the start, 1 at its bonus neighbour (q0 - 1, r0) resp. (q0, r0 - 1)
    for key, nb in (("a gap start: a bonus from row 1 into DP row 2", (-1, 0)), ("a gap start: a bonus from column 1 into DP column 2", (0, -1))):
        name, R, (go, ge, st), rec, cells, qs = by[key]
        assert R[rec[1], rec[2]] == 0 and R[rec[1] + nb[0], rec[2] + nb[1]] == 1 and qs[0] == 0.5
    # the set bonus cell changes the values, not the cells
    for step in ("(2, 1)", "(1, 2)"):
        unset, isset = by["a %s step, bonus cell (4, 4) unset" % step], by["a %s step, bonus cell (4, 4) set" % step]
        assert unset[4] == isset[4] and isset[3][0] == unset[3][0] + 1 and (4, 4) not in isset[4]
    # the ties the plot was built for
    name, R, (go, ge, st), rec, cells, qs = by["c2 and c3 tie, c2 wins"]
    Q = ref.full_matrix(R, go, ge, st)
    assert Q[4, 4] == 2 and Q[3, 4] + R[4, 5] == 2 and Q[5, 5] == 3


# ---- the library's surface (no device needed) ---------------------------------------------------------------------------------------------
def test_exports_and_header_name_the_dmax_calls():
    import os
    from acoss_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "acx.h")).read()
    L = _lib.load()
    for name in ("acx_chenfusion_align", "acx_chenfusion_align_paths", "acx_dmax_locate_binary", "acx_dmax_path_binary"):
        assert name in _lib.EXPORTS and ("int %s(" % name) in header and hasattr(L, name)
    assert _lib.ABI_VERSION == 4 and "#define ACX_ABI_VERSION 4" in header


def test_python_methods_exist_and_check_their_arguments_first(tmp_path, monkeypatch):
    """ChenFusion.align*(..., similarity_type=) refuse bad arguments before any library call (no device here)."""
    from acoss_amd import _lib
    from acoss_amd.algorithms import ChenFusion, Serra09
    for name in ("chenfusion_align", "chenfusion_align_paths", "dmax_locate_binary", "dmax_path_binary"):
        assert callable(getattr(_lib.Context, name))
    monkeypatch.chdir(tmp_path)
    csv = tmp_path / "d.csv"
    csv.write_text("work_id,track_id\nw0,t0\nw0,t1\n")
    tracks = [np.random.default_rng(k).random((40, 12)).astype(np.float32) for k in range(2)]
    algo = ChenFusion(str(csv), "feat/", shortname="dmaxargs")
    try:
        algo.set_pooled_features(tracks, ["w0", "w0"])
        for call in (lambda t: algo.align([[0, 1]], similarity_type=t), lambda t: algo.align_paths([[0, 1]], similarity_type=t),
                     lambda t: algo.align_matches([0], [[1]], similarity_type=t), lambda t: algo.align_match_paths([0], [[1]], similarity_type=t)):
            with pytest.raises(ValueError, match="'Late' is fused from whole score matrices and has no alignment of its own"):
                call("Late")
            with pytest.raises(ValueError, match="unknown similarity type 'main'"):
                call("main")
        for t in ("qmax", "dmax"):
            with pytest.raises(ValueError, match="align: idxs must be \\(K, 2\\)"):
                algo.align([0, 1, 0], similarity_type=t)
            with pytest.raises(ValueError, match="align_paths: idxs must be track indices in \\[0, 2\\)"):
                algo.align_paths([[0, 2]], similarity_type=t)
            with pytest.raises(ValueError, match="align_matches: indices must be \\(Q, k\\)"):
                algo.align_matches([0, 1], [[1]], similarity_type=t)
            with pytest.raises(ValueError, match="align_match_paths: indices must be track indices in \\[0, 2\\) or -1"):
                algo.align_match_paths([0], [[-2]], similarity_type=t)
        assert algo._ctx is None, "no library call was made"
    finally:
        algo.cleanup_memmap()
    # Serra09 has one type, 'main' (None: the default; ChenFusion's types are unknown to it), and keeps its refusal
    import inspect
    assert inspect.signature(Serra09.align).parameters["similarity_type"].default is None
    algo = Serra09(str(csv), "feat/", shortname="dmaxargs2", engine={"dmax": 1})
    try:
        algo.set_pooled_features(tracks, ["w0", "w0"])
        for t in ("qmax", "dmax"):
            with pytest.raises(ValueError, match="align: unknown similarity type '%s'" % t):
                algo.align([[0, 1]], similarity_type=t)
        with pytest.raises(ValueError, match="align: the Qmax alignment only"):
            algo.align([[0, 1]])
        with pytest.raises(ValueError, match="align: the Qmax alignment only"):
            algo.align([[0, 1]], similarity_type="main")
        assert algo._ctx is None, "no library call was made"
    finally:
        algo.cleanup_memmap()
