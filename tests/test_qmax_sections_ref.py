"""
CPU tests of the Qmax SECTIONS' yardstick (tests/_qmax_sections_ref.py): its two statements of the contract
against each other, the consequences the contract promises, the box property that lets qmax_path_kernel serve every section, and
hand-checked plots.

The last tests hold the library's surface against the yardstick's: they fail where the exports and methods are missing.
"""
import numpy as np
import pytest

from tests import _qmax_locate_ref as loc
from tests import _qmax_path_ref as pref
from tests import _qmax_sections_ref as ref

GAMMAS = ((0.5, 0.5), (0.5, 0.7), (1.0, 0.25))
DENSITIES = (0.2, 0.5, 0.8)
STEP_SET = {(1, 1), (2, 1), (1, 2)}


def check_sections(R, go, ge, st, recs, paths, opts):
    """The consequences of the contract on one plot's sections (a list of records and, where known, their paths)."""
    S, ms, mr = opts.get("max_sections", 4), opts.get("min_score", 2.0), opts.get("min_ratio", 0.0)
    assert len(recs) <= S
    first = loc.locate_forward(R, go, ge, st)
    if first[0] >= ms:
        assert recs and recs[0] == first, "section 0 is the alignment of section 16"
    else:
        assert not recs
    scores = [np.float32(r[0]) for r in recs]
    assert all(a >= b for a, b in zip(scores, scores[1:])), "scores do not increase"
    assert all(s >= ref.threshold(k, scores[0], ms, mr) for k, s in enumerate(scores))
    rows = sorted((r[1], r[3]) for r in recs)
    assert all(q1 > q0 for q0, q1 in rows) and all(a[1] < b[0] for a, b in zip(rows, rows[1:])), "row ranges are disjoint"
    for rec, cells in zip(recs, paths or ()):
        # the DP on the section's box alone, on the UNMASKED plot, makes the same choices
        brec, bcells, _ = pref.path_box(R, rec, go, ge, st)
        assert brec == rec and np.array_equal(bcells, cells), "path_box reproduces the section's cells and score"
        assert tuple(cells[0]) == rec[1:3] and tuple(cells[-1]) == rec[3:5]
        assert {tuple(d) for d in np.diff(cells, axis=0)} <= STEP_SET
        assert len(cells) <= rec[3] - rec[1] + 1


@pytest.mark.parametrize("st", (2, 3))
@pytest.mark.parametrize("gammas", GAMMAS)
def test_both_statements_agree_on_random_plots(gammas, st):
    """64 plots per (gammas, dp_start): 384 in all, sides 3 .. 40, three densities, pad 0 .. 3, max_sections 1 .. 16."""
    rng = np.random.default_rng([28, st, int(8 * gammas[0]), int(100 * gammas[1])])
    n_sections, n_multi = 0, 0
    for t in range(64):
        M, N = (int(v) for v in rng.integers(3, 41, 2))
        R = (rng.random((M, N)) < DENSITIES[t % 3]).astype(np.uint8)
        opts = dict(max_sections=(1, 2, 4, 16)[(t // 3) % 4], pad=t % 4, min_score=(1.5, 2.0, 3.0)[(t // 12) % 3],
                    min_ratio=(0.0, 0.5)[(t // 36) % 2])
        recs, paths = ref.sections_full(R, gammas[0], gammas[1], st, **opts)
        assert recs == ref.sections_intervals(R, gammas[0], gammas[1], st, **opts), (t, opts)
        check_sections(R, gammas[0], gammas[1], st, recs, paths, opts)
        n_sections += len(recs)
        n_multi += len(recs) > 1
    print("%d sections on 64 plots, %d plots with more than one" % (n_sections, n_multi))
    assert n_multi >= 8, "the plots hold sections behind the first to compare: %d plots with more than one" % n_multi


def test_max_sections_one_is_the_alignment():
    rng = np.random.default_rng(5)
    for t in range(20):
        R = (rng.random((30, 37)) < 0.4).astype(np.uint8)
        for st in (2, 3):
            recs, paths = ref.sections_full(R, 0.5, 0.7, st, max_sections=1, min_score=1.5)
            rec, cells, _ = pref.path_full(R, 0.5, 0.7, st)
            assert recs == [rec] and np.array_equal(paths[0], cells)


@pytest.mark.parametrize("case", ref.HAND, ids=[h[0] for h in ref.HAND])
def test_hand_checked_plots(case):
    name, R, opts, want = case
    recs, paths = ref.sections_full(R, **opts)
    assert recs == want, (name, recs)
    assert ref.sections_intervals(R, **opts) == want
    check_sections(R, 0.5, 0.5, 2, recs, paths, opts)


def test_cleared_rows_would_bridge_the_excluded_stretch():
    """Why Q is forced to 0 instead of clearing rows of R: with rows 40..79 cleared the next alignment runs through them."""
    R = ref.BRIDGE.copy()
    R[40:80] = 0
    assert loc.locate_forward(R) == (32.5, 10, 10, 95, 95)
    assert ref.sections_full(ref.BRIDGE)[0][1] == (30.0, 10, 10, 39, 39)


def test_the_tie_plots_tie_between_intervals():
    """The hand plots named for it really make two INTERVAL records share the largest value, in the round they say, and the record
    with the smaller end cell is picked -- in TIE3 the one in the higher slot, where a rule by slot order would pick the other."""
    ties = []
    ref.sections_intervals(ref.TIE2, max_sections=4, ties=ties)
    assert ties[1] == ([0, 1], 0), ties
    ties = []
    ref.sections_intervals(ref.TIE3, max_sections=4, ties=ties)
    assert ties[2] == ([1, 2], 2), ties


def test_a_round_sweeps_only_the_split_intervals():
    swept = []
    recs = ref.sections_intervals(ref.THREE, max_sections=3, swept=swept)
    assert len(recs) == 3
    assert swept == [(0, 59), (0, 3), (16, 59), (16, 19), (29, 59)]


def test_empty_and_tiny_plots_have_no_sections():
    for st in (2, 3):
        # (3 x 3 ones: the one DP cell holds 1, below every admissible min_score)
        for R in [np.zeros((7, 9), np.uint8)] + [np.ones(shape, np.uint8) for shape in ((2, 5), (5, 2), (1, 1), (3, 3))]:
            assert ref.sections_full(R, 0.5, 0.5, st, min_score=1.5) == ([], [])
            assert ref.sections_intervals(R, 0.5, 0.5, st, min_score=1.5) == []


# ---- the library's surface (no device needed) ---------------------------------------------------------------------------------------------
def test_exports_and_header_name_the_section_calls():
    import os
    from acoss_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "acx.h")).read()
    for name in ("acx_serra09_align_sections", "acx_qmax_sections_binary"):
        assert name in _lib.EXPORTS and ("int %s(" % name) in header
        assert hasattr(_lib.load(), name)
    assert "acx_section_opts" in header
    assert _lib.ABI_VERSION == 4


def _algo(cls, tmp_path, shortname, **kw):
    csv = tmp_path / "d.csv"
    csv.write_text("work_id,track_id\nw0,t0\nw0,t1\n")
    algo = cls(str(csv), "feat/", shortname=shortname, **kw)
    algo.set_pooled_features([np.random.default_rng(k).random((40, 12)).astype(np.float32) for k in range(2)], ["w0", "w0"])
    return algo


def test_python_methods_check_their_arguments_first(tmp_path, monkeypatch):
    """align_sections / align_match_sections refuse bad arguments before any library call (no device here)."""
    from acoss_amd import _lib
    from acoss_amd.algorithms import ChenFusion, Serra09
    assert callable(_lib.Context.serra09_align_sections) and callable(_lib.Context.qmax_sections_binary)
    monkeypatch.chdir(tmp_path)
    algo = _algo(Serra09, tmp_path, "secargs")
    try:
        with pytest.raises(ValueError, match="align_sections: idxs must be \\(K, 2\\)"):
            algo.align_sections([0, 1, 0])
        with pytest.raises(ValueError, match="align_sections: idxs must be track indices in \\[0, 2\\)"):
            algo.align_sections([[0, 2]])
        with pytest.raises(ValueError, match="align_sections: track indices must be integers"):
            algo.align_sections([[0.0, 1.0]])
        with pytest.raises(ValueError, match="align_match_sections: indices must be \\(Q, k\\)"):
            algo.align_match_sections([0, 1], [[1]])
        with pytest.raises(ValueError, match="align_match_sections: indices must be track indices in \\[0, 2\\) or -1"):
            algo.align_match_sections([0], [[-2]])
        for bad, what in ((dict(max_sections=0), "max_sections"), (dict(max_sections=17), "max_sections"), (dict(min_score=1.0), "min_score"),
                          (dict(min_score=float("nan")), "min_score"), (dict(min_ratio=-0.1), "min_ratio"), (dict(min_ratio=1.5), "min_ratio"),
                          (dict(pad=-1), "pad"), (dict(pad=1.5), "pad"), (dict(max_sections=2.0), "max_sections")):
            with pytest.raises(ValueError, match="align_sections: %s" % what):
                algo.align_sections([[0, 1]], **bad)
            with pytest.raises(ValueError, match="align_match_sections: %s" % what):
                algo.align_match_sections([0], [[1]], **bad)
        assert algo._ctx is None, "no library call was made"
    finally:
        algo.cleanup_memmap()
    algo = _algo(Serra09, tmp_path, "secargs2", engine={"dmax": 1})
    try:
        with pytest.raises(ValueError, match="align_sections: the Qmax alignment only"):
            algo.align_sections([[0, 1]])
        with pytest.raises(ValueError, match="align_match_sections: the Qmax alignment only"):
            algo.align_match_sections([0], [[1]])
    finally:
        algo.cleanup_memmap()
    algo = _algo(ChenFusion, tmp_path, "secargs3")
    try:
        for st in ("dmax", "Late"):
            with pytest.raises(ValueError, match="align_sections: .*%s" % st):
                algo.align_sections([[0, 1]], similarity_type=st)
            with pytest.raises(ValueError, match="align_match_sections: .*%s" % st):
                algo.align_match_sections([0], [[1]], similarity_type=st)
        with pytest.raises(ValueError, match="align_sections: unknown similarity type"):
            algo.align_sections([[0, 1]], similarity_type="main")
        with pytest.raises(ValueError, match="align_sections: min_score"):
            algo.align_sections([[0, 1]], min_score=0.5, similarity_type="qmax")
        assert algo._ctx is None, "no library call was made"
    finally:
        algo.cleanup_memmap()
