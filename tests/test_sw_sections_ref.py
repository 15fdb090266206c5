"""
CPU tests of the EarlyFusion SECTIONS' yardstick (tests/_sw_sections_ref.py): its two statements of the contract
against each other, the consequences the contract promises, and hand-checked plots.

The last tests hold the library's surface against the yardstick's: they fail where the exports and methods are missing.
"""
import os
import re

import numpy as np
import pytest

from . import _sw_align_ref as aref
from . import _sw_sections_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def check_sections(B, recs, paths, opts):
    """The consequences of the contract on one plot's sections."""
    S, ms, mr = opts.get("max_sections", 4), opts.get("min_score", 2.0), opts.get("min_ratio", 0.0)
    assert len(recs) <= S and len(paths) == len(recs)
    first, cells = aref.align_traceback(B)
    if F(first[0]) >= F(ms):
        assert recs and recs[0] == first and np.array_equal(paths[0], cells), "section 0 is the alignment of section 19"
    else:
        assert not recs
    scores = [F(r[0]) for r in recs]
    assert all(a >= b for a, b in zip(scores, scores[1:])), "scores do not increase"
    assert all(s >= ref.threshold(k, scores[0], ms, mr) for k, s in enumerate(scores))
    rows = sorted((r[1], r[3]) for r in recs)
    assert all(q1 > q0 for q0, q1 in rows) and all(a[1] < b[0] for a, b in zip(rows, rows[1:])), "row ranges are disjoint"
    ref.check_sections(recs, paths, B.shape)                     # start, end, step set {(1, 1), (2, 1), (1, 2)}, counted rectangle
    for rec, cells in zip(recs, paths):
        assert len(cells) <= rec[3] - rec[1] + 1


def _same(a, b):
    return a[0] == b[0] and len(a[1]) == len(b[1]) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_both_statements_agree_on_random_plots():
    """600 plots: sides 3 .. 40, five densities, pad 0 .. 3, max_sections in {1, 2, 4, 16}, three min_score, two min_ratio."""
    rng = np.random.default_rng(29)
    n2 = n3 = 0
    for t in range(600):
        B, opts = ref.random_case(rng)
        full = ref.sections_full(B, **opts)
        assert _same(full, ref.sections_intervals(B, **opts)), (t, opts)
        check_sections(B, full[0], full[1], opts)
        n2 += len(full[0]) >= 2
        n3 += len(full[0]) >= 3
    print("600 plots: %d with two or more sections, %d with three or more" % (n2, n3))
    assert n2 >= 60 and n3 >= 15, "the plots hold sections behind the first to compare: %d with two or more, %d with three or more" % (n2, n3)


def test_max_sections_one_is_the_alignment():
    rng = np.random.default_rng(5)
    for t in range(20):
        B = (rng.random((30, 37)) < (0.1, 0.4)[t % 2]).astype(np.uint8)
        recs, paths = ref.sections_full(B, max_sections=1, min_score=1.1)
        rec, cells = aref.align_traceback(B)
        assert recs == [rec] and np.array_equal(paths[0], cells)


@pytest.mark.parametrize("case", ref.HAND, ids=[h[0] for h in ref.HAND])
def test_hand_checked_plots(case):
    name, B, opts, want = case
    recs, paths = ref.sections_full(B, **opts)
    assert recs == ref.hand_records(want), (name, recs)
    assert _same((recs, paths), ref.sections_intervals(B, **opts))
    check_sections(B, recs, paths, opts)


def test_cleared_rows_would_bridge_the_excluded_stretch():
    """Why T' is forced to 0 instead of clearing rows of the plot: a cleared row still carries `predecessor - 17`, and with rows
    40..59 cleared the next alignment runs through them on (2, 1) steps -- 183 tenths at (39, 39), ten cleared cells (-10, then nine
    times -17) leave 20 at (59, 49), and the 18 ones from (60, 50) add 10 - 7 + 170: 193 at (77, 67)."""
    recs, paths = ref.sections_cleared(ref.BRIDGE)
    assert recs == ref.hand_records([(19.3, 40, 200, 59, 219), (19.3, 21, 21, 77, 67)])
    assert len(set(range(40, 60)) & set(paths[1][:, 0].tolist())) == 10, "the second answer crosses the excluded rows"
    assert ref.sections_full(ref.BRIDGE)[0][1] == ref.hand_records([(18.3, 21, 21, 39, 39)])[0]


def test_the_tie_plot_ties_between_intervals():
    """TIE2 really makes two INTERVAL records share the largest value in round 1, and the one with the smaller end cell is picked."""
    ties = []
    ref.sections_intervals(ref.TIE2, max_sections=4, ties=ties)
    assert ties[1] == ([0, 1], 0), ties


def test_a_round_sweeps_only_the_split_intervals():
    swept = []
    recs, _ = ref.sections_intervals(ref.THREE, max_sections=3, swept=swept)
    assert len(recs) == 3
    assert swept == [(0, 59), (0, 3), (16, 59), (16, 19), (29, 59)]
    # an interval of one counted row ([8, 8]) and one without a counted row ([0, 1]) are left unswept
    swept = []
    ref.sections_intervals(ref.ONE_ROW, max_sections=4, min_score=1.01, swept=swept)
    assert swept == [(0, 19), (8, 19), (15, 19)]


def test_an_excluded_row_keeps_its_bits_as_rows_0_and_1_do():
    """U' = (B ? 0 : -7) on an excluded row: RATIO's second diagonal scores 10 n below the 1 at (9, 29), not 10 n - 7."""
    recs, _ = ref.sections_full(ref.RATIO, max_sections=2)
    assert recs[1] == ref.hand_records([(4.0, 10, 30, 13, 33)])[0]
    B = ref.RATIO.copy()
    B[9, 29] = 0
    assert ref.sections_full(B, max_sections=2)[0][1] == ref.hand_records([(3.3, 10, 30, 13, 33)])[0]


def test_empty_and_tiny_plots_have_no_sections():
    for B in aref.no_match_plots():
        assert ref.sections_full(B, min_score=1.1) == ([], [])
        assert ref.sections_intervals(B, min_score=1.1) == ([], [])
    # 4 x 4 ones: the one counted cell holds 1.0, below every admissible min_score
    assert ref.sections_full(np.ones((4, 4), np.uint8), min_score=1.01) == ([], [])


# ---- the library's surface (no device needed) ---------------------------------------------------------------------------------------------
def test_exports_header_and_integration_name_the_section_calls():
    from acoss_amd import _lib
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    flat = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert ("int acx_ef_align_sections(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_ef_params *params, int32_t plane , "
            "const acx_section_opts *opts, acx_alignment *out , int32_t *n_sections , int64_t *path_off , int32_t *cells , int64_t cap);") in flat
    assert ("int acx_sw_sections_binary(acx_ctx *ctx, const uint8_t *B, int32_t M, int32_t N, const acx_section_opts *opts, "
            "acx_alignment *out, int32_t *n_sections, int64_t *path_off, int32_t *cells, int64_t cap);") in flat
    assert re.search(r"#define ACX_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("acx_ef_align_sections", "acx_sw_sections_binary"):
        assert _lib.EXPORTS.count(name) == 1 and hasattr(_lib.load(), name)
        assert ("`%s(" % name) in integration
    assert callable(_lib.Context.ef_align_sections) and callable(_lib.Context.sw_sections_binary)


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


def test_python_methods_check_their_arguments_first(tmp_path, monkeypatch):
    """align_sections / align_match_sections refuse bad arguments before any library call (no device here)."""
    from acoss_amd.algorithms import EarlyFusion
    monkeypatch.chdir(tmp_path)
    algo = EarlyFusion(_csv(tmp_path, 8), "feat/", shortname="efsections")
    algo._ctx = _NoDevice()
    monkeypatch.setattr(EarlyFusion, "_context", lambda self: (_ for _ in ()).throw(AssertionError("pool upload before the argument checks")))
    with pytest.raises(ValueError, match=r"align_sections: idxs must be \(K, 2\)"):
        algo.align_sections([0, 1, 0])
    with pytest.raises(ValueError, match=r"align_sections: idxs must be track indices in \[0, 8\)"):
        algo.align_sections([[0, 8]])
    with pytest.raises(ValueError, match="align_sections: track indices must be integers"):
        algo.align_sections([[0.0, 1.0]])
    with pytest.raises(ValueError, match=r"align_match_sections: indices must be \(Q, k\)"):
        algo.align_match_sections([0, 1], [[1]])
    with pytest.raises(ValueError, match=r"align_match_sections: indices must be track indices in \[0, 8\) or -1"):
        algo.align_match_sections([0], [[-2]])
    for bad, what in ((dict(max_sections=0), "max_sections"), (dict(max_sections=17), "max_sections"), (dict(min_score=1.0), "min_score"),
                      (dict(min_score=float("nan")), "min_score"), (dict(min_ratio=-0.1), "min_ratio"), (dict(min_ratio=1.5), "min_ratio"),
                      (dict(pad=-1), "pad"), (dict(pad=1.5), "pad"), (dict(max_sections=2.0), "max_sections")):
        with pytest.raises(ValueError, match="align_sections: %s" % what):
            algo.align_sections([[0, 1]], **bad)
        with pytest.raises(ValueError, match="align_match_sections: %s" % what):
            algo.align_match_sections([0], [[1]], **bad)
    # similarity_type: the four device planes only (None: the default, 'early'), checked before the options and the indices
    for bad in ("late", "early+late", "nope", 3):
        with pytest.raises(ValueError, match="align_sections: .*similarity_type must be one of"):
            algo.align_sections([[0, 99]], similarity_type=bad, min_score=0.0)
        with pytest.raises(ValueError, match="align_match_sections: .*similarity_type must be one of"):
            algo.align_match_sections([0], [[1]], similarity_type=bad)
    # nothing to align: no library call either
    assert algo.align_sections(np.zeros((0, 2), np.int64)) == []
    assert algo.align_sections(np.zeros((0, 2), np.int64), similarity_type="mfccs", paths=True) == ([], [])
    out, paths = algo.align_match_sections([0, 3], [[-1, -1], [-1, -1]], paths=True)
    assert [[a.shape for a in row] for row in out] == [[(0,)] * 2] * 2 and out[0][0].dtype == EarlyFusion.ALIGN_DTYPE
    assert paths == [[[], []], [[], []]]
    # valid arguments get past the checks, to the (absent) library
    for plane in ("mfccs", "ssms", "chromas", "early"):
        with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
            algo.align_sections([[0, 1]], similarity_type=plane)
    with pytest.raises(AssertionError, match="pool upload before|the library was reached"):
        algo.align_match_sections([0, 3], [[1, -1], [-1, 4]])
    algo._ctx = None
    algo.cleanup_memmap()


def test_a_list_with_a_long_track_is_refused_by_name_before_the_library(tmp_path, monkeypatch):
    """Tracks beyond 1024 blocks: the class asks the context's block counts (ef_has_long_track) and refuses the whole list."""
    from acoss_amd import _lib
    from acoss_amd.algorithms import EarlyFusion

    class _Blocks(object):
        ef_blocks = np.array([40, 1025, 50], np.int64)
        ef_has_long_track = _lib.Context.ef_has_long_track

        def __getattr__(self, name):
            raise AssertionError("the library was reached (%s)" % name)
    monkeypatch.chdir(tmp_path)
    algo = EarlyFusion(_csv(tmp_path, 3), "feat/", shortname="efsectionslong")
    monkeypatch.setattr(EarlyFusion, "_context", lambda self: _Blocks())
    with pytest.raises(NotImplementedError, match="align_sections: sections need the bit path: tracks of at most 1024 blocks"):
        algo.align_sections([[0, 2], [1, 2]])
    with pytest.raises(NotImplementedError, match="align_match_sections: sections need the bit path"):
        algo.align_match_sections([0], [[2, 1]])
    with pytest.raises(AssertionError, match="the library was reached \\(ef_align_sections\\)"):
        algo.align_sections([[0, 2]])
    algo.cleanup_memmap()
