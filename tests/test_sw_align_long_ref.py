"""
Host-side checks of the EarlyFusion alignment beyond 1024 blocks (acx_ef_align_long, acx_sw_align_long_binary):
the strip-wise restatement of tests/_sw_align_strips.py equals tests/_sw_align_ref.py::align_forward on every plot that
tests/test_gpu_sw_align_long.py hands the kernel, and each of its mutants changes the record or the cells of at least one of them --
the proof that those plots can see what they are for; the ABI surface; the class's choice between the two exports.
"""
import os
import re

import numpy as np
import pytest

from . import _sw_align_ref as ref
from . import _sw_align_strips as strips

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def forward():
    """align_forward of every plot of section a, once."""
    return {name: ref.align_forward(B) for name, B in strips.all_plots()}


def test_restatement_equals_align_forward_on_every_plot(forward):
    plots = strips.all_plots()
    assert len({name for name, _ in plots}) == len(plots)
    for name, B in plots:
        rec, cells, _ = strips.align_strips(B)
        want = forward[name]
        assert rec == want[0] and np.array_equal(cells, want[1]), (name, rec, want[0])
        ref.check_path(rec, cells, B.shape)


def test_planted_answers(forward):
    """What the plots were built to show is what the reference answers on them."""
    n = 0
    for name, B, cells in strips.planted_plots():
        n += 1
        if cells is not None:
            assert np.array_equal(forward[name][1], cells), name
    assert n == 66
    for name, B, end in strips.tie_plots() + strips.tall_plots():
        if end is not None:
            assert forward[name][0][3:5] == end, (name, forward[name][0])
    assert forward["tie_late_strip0_early_strip1"][0] == (float(np.float32(9.3)), 3, 1500, 12, 1509)
    for name, B, cells in strips.seam_pred_tie_plots():
        assert forward[name][1].tolist() == [list(c) for c in cells], name
    rec, cells = forward["eye_3400"]
    assert rec == (3397.0, 2, 2, 3398, 3398) and len(cells) == 3397


def _seen(mutant, plots, forward):
    """The plots of `plots` on which the mutant's record or cells differ from the reference's."""
    out = []
    for name, B in plots:
        rec, cells, _ = strips.align_strips(B, mutant)
        if not _same((rec, cells), forward[name]):
            out.append(name)
    return out


RECORD_MUTANTS = ("swap", "drop2", "row", "ring")


@pytest.mark.parametrize("mutant", RECORD_MUTANTS)
def test_record_mutants_are_seen_by_the_planted_paths(mutant, forward):
    planted = [(n, B) for n, B, _ in strips.planted_plots()]
    seen = _seen(mutant, planted, forward)
    assert seen, mutant
    if mutant == "ring":
        assert all(n.startswith("seam2048") or n.startswith("seam3072") for n in seen)      # strip 1 reads strip 0 either way
    else:
        assert {n[:8] for n in seen} == {"seam1024", "seam2048", "seam3072"}, (mutant, seen)


def test_best_mutants_are_seen(forward):
    ties = [(n, B) for n, B, _ in strips.tie_plots()]
    assert "tie_same_lane_late_then_early" in _seen("tie_row", ties, forward)
    assert _seen("reduce_col", ties, forward), "no tie plot tells the reduction's column rule"
    tall = [(n, B) for n, B, _ in strips.tall_plots()]
    assert "tall_maximum_row_2400" in _seen("row10", tall, forward)
    assert _seen("t16", [strips.big_value_plots()[0]], forward) == ["eye_3400"]


def test_stale_plane_is_seen():
    ones, sparse = strips.stale_pair()
    want = ref.align_forward(sparse)
    _, _, plane = strips.align_strips(ones)
    rec, cells, _ = strips.align_strips(sparse, None, plane.copy())
    assert _same((rec, cells), want)
    rec, cells, _ = strips.align_strips(sparse, "stale", plane.copy())
    assert not _same((rec, cells), want)


def test_exports_named_in_header_and_shim():
    from acoss_amd import _lib
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    assert ("int acx_ef_align_long(acx_ctx *ctx, const int32_t *pairs, int64_t K, const acx_ef_params *params, int32_t plane , "
            "acx_alignment *out , int64_t *path_off , int32_t *cells , int64_t cap);") in flat
    assert ("int acx_sw_align_long_binary(acx_ctx *ctx, const uint8_t *B, int32_t M, int32_t N, acx_alignment *out, int32_t *cells, "
            "int64_t cap, int64_t *n_cells);") in flat
    assert re.search(r"#define ACX_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    for name in ("acx_ef_align_long", "acx_sw_align_long_binary"):
        assert _lib.EXPORTS.count(name) == 1
    assert callable(_lib.Context.ef_align_long) and callable(_lib.Context.sw_align_long_binary)
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "| `acx_ef_align_long(" in table and "`acx_sw_align_long_binary(" in table


# ---------------------------------------------------------------------------------------------- the class's dispatch
class _StandIn(object):
    """Stands where the class's libacx context would be and records which export a call would take."""
    def __init__(self, blocks):
        self.ef_blocks = np.asarray(blocks, np.int64)
        self.calls = []

    def _answer(self, name, pairs, paths):
        from acoss_amd import _lib
        self.calls.append((name, np.asarray(pairs).tolist(), paths))
        al = np.zeros(len(pairs), _lib.ALIGNMENT_DTYPE)
        al["score"], al["q0"], al["r0"], al["q1"], al["r1"] = 2.3, 4, 5, 6, 7
        if not paths:
            return al
        return al, np.arange(len(pairs) + 1, dtype=np.int64), np.tile(np.array([[4, 5]], np.int32), (len(pairs), 1))

    def ef_has_long_track(self, pairs):
        from acoss_amd import _lib
        return _lib.Context.ef_has_long_track(self, pairs)

    def ef_align(self, pairs, kappa, K, plane, paths=False, cap=None):
        return self._answer("ef_align", pairs, paths)

    def ef_align_long(self, pairs, kappa, K, plane, paths=False, cap=None):
        return self._answer("ef_align_long", pairs, paths)


def _stand_in(monkeypatch, tmp_path, blocks):
    from acoss_amd.algorithms import EarlyFusion
    path = tmp_path / "ds.csv"
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(len(blocks)):
            f.write("w%d,t%d\n" % (i // 2, i))
    algo = EarlyFusion(str(path), "feat/", shortname="efalignlong")
    ctx = _StandIn(blocks)
    monkeypatch.setattr(EarlyFusion, "_context", lambda self: ctx)
    return algo, ctx


def test_a_long_track_routes_to_ef_align_long(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    algo, ctx = _stand_in(monkeypatch, tmp_path, [300, 1024, 1025, 17])
    al = algo.align([[0, 1], [3, 1]])
    assert [c[0] for c in ctx.calls] == ["ef_align"] and al["q0"].tolist() == [4, 4]
    assert al["q_span"].tolist() == [[4, 6 + algo.blocksize - 1]] * 2
    algo.align([[0, 1], [3, 2]])
    algo.align([[2, 0]])
    al, paths = algo.align_paths([[1, 2], [0, 3]])
    assert [c[0] for c in ctx.calls[1:]] == ["ef_align_long"] * 3 and ctx.calls[-1][2] is True
    assert len(paths) == 2 and paths[0].tolist() == [[4, 5]]
    al, paths = algo.align_paths([[1, 0], [0, 3]])
    assert ctx.calls[-1][0] == "ef_align" and ctx.calls[-1][2] is True
    # the hits of an identification: the empty slot is not a listed track
    algo.align_matches([2], [[0, -1]])
    assert ctx.calls[-1][0] == "ef_align_long" and ctx.calls[-1][1] == [[2, 0]]
    algo.align_matches([1], [[0, -1]])
    assert ctx.calls[-1][0] == "ef_align"


def test_ef_align_long_needs_cap_for_a_pool_it_did_not_see(monkeypatch):
    from acoss_amd import _lib

    class _Lib(object):
        def __getattr__(self, name):
            raise AssertionError("the library was reached (%s)" % name)
    ctx = object.__new__(_lib.Context)
    ctx._L, ctx._h = _Lib(), None
    with pytest.raises(ValueError, match="cap must be given"):
        ctx.ef_align_long([[0, 1]], paths=True)
    # ... and without block counts every list goes to ef_align_long, which serves short lists as ef_align does
    assert ctx.ef_has_long_track([[0, 1]]) is True
    ctx.ef_blocks = np.array([5, 1024, 1025])
    assert ctx.ef_has_long_track([[0, 1]]) is False and ctx.ef_has_long_track([[1, 2]]) is True
    assert ctx.ef_has_long_track([[0, 7]]) is False and ctx.ef_has_long_track(np.zeros((0, 2), np.int32)) is False
