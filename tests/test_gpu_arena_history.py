"""
GPU tests (run with -m gpu on a real MI355X): HISTORY INDEPENDENCE -- no result may depend on what device memory held before a call.

A context keeps its device arenas from call to call (DeviceBuffer::grow is grow-only and never clears), many kernels read arena
words they did not write, and the entry points that allocate per call get recycled memory from hipMalloc.  The rest of the suite
meets that only by accident of test order.  Here, for every probe of tests/_history_cases.py and every fill word of its WORDS:

    a new context with the allocation fill on  ->  the case's uploads  ->  the probe's DIRTYING call (the same export on a larger,
    denser problem)  ->  acx_debug_fill_arenas(word): every scratch block of the context, to capacity  ->  the probe

  (a) the probe's outputs are the same bits under all five words;
  (b) they are the CPU reference's, under the checker of the family's own test (imported from it, no bound restated here).

A probe whose bits move with the word has found a read of memory nobody wrote.  The Serra09 bits outside a matrix's columns are a
documented dependence the sweeps mask: their count is printed, and what the API returns is asserted.
tests/test_history_cases_design.py shows on the CPU that the references are the reference modules' and that the dirtying calls cover
the probes' arenas.
"""
import numpy as np
import pytest

from . import _history_cases as H
from . import _serra09_shapes as S

pytestmark = pytest.mark.gpu


def _under_every_word(case, probe):
    """The schedule above; returns the outputs per word.  The allocation fill is process-wide: off again whatever happens."""
    from acoss_amd import _lib
    outs = []
    for word in H.WORDS:
        try:
            _lib.set_alloc_fill(True, word)
            ctx = _lib.Context(0)
            try:
                case.prepare(ctx)
                probe.dirty(ctx)
                ctx.debug_fill_arenas(word)
                outs.append(probe.run(ctx))
            finally:
                ctx.close()
        finally:
            _lib.set_alloc_fill(False, 0)
    return outs


def _same_bits(probe, outs):
    first = H.flat(outs[0])
    for word, out in zip(H.WORDS[1:], outs[1:]):
        mine = H.flat(out)
        assert sorted(mine) == sorted(first), (probe.name, hex(word))
        for key in first:
            assert mine[key][1:] == first[key][1:], (probe.name, key, "shape / dtype under 0x%08X" % word, mine[key][1:], first[key][1:])
            if mine[key][0] != first[key][0]:
                a, b = (np.ascontiguousarray(x[key]).reshape(-1) for x in (outs[0], out))
                bad = np.nonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))[0]
                raise AssertionError("%s: output `%s` under fill word 0x%08X differs from the one under 0x%08X in %d of %d elements, first "
                                     "at %s: a read of memory nobody wrote" % (probe.name, key, word, H.WORDS[0], len(bad), len(a), bad[:5].tolist()))


# ---- (b): the checkers of the families' own tests ---------------------------------------------------------------------------------------------
def _serra09_set(probe):
    return S.subset(S.relabel(H.serra09_pool(), probe.info.get("m", H.M9)), probe.info["pairs"])


def _check_scores(probe, out):
    S.assert_scores_equal(_serra09_set(probe), probe.info.get("m", H.M9), out["scores"], probe.want["scores"], probe.name)


def _check_debug_bits(probe, out):
    d, m = _serra09_set(probe), probe.info["m"]
    S.assert_plots_equal(d, m, [out["plot0"]], probe.want["plots"], probe.name)
    S.assert_scores_equal(d, m, out["scores"], probe.want["scores"], probe.name)


def _check_record(rec_of):
    def check(probe, out):
        got = out["records"]
        assert got.shape == (1,), probe.name
        assert rec_of(got[0]) == probe.want["record"], "%s: device %s, reference %s" % (probe.name, rec_of(got[0]), probe.want["record"])
        if "cells" in probe.want:
            cells = out["cells"]
            if "offsets" in out:
                assert out["offsets"].tolist() == [0, len(cells)], probe.name
            assert cells.dtype == np.int32 and np.array_equal(cells, probe.want["cells"]), "%s: %d cells %s ..., reference %d %s ..." % (
                probe.name, len(cells), cells[:3].tolist(), len(probe.want["cells"]), probe.want["cells"][:3].tolist())
    return check


def _check_sections(probe, out):
    from .test_gpu_qmax_sections import _compare
    recs = out["records"].reshape(-1)
    S_ = len(recs)
    off = np.asarray(out["offsets"])
    assert off.shape == (S_ + 1,) and off[0] == 0 and out["cells"].shape == (off[-1], 2), probe.name
    _compare(probe.name, S_, recs, int(np.asarray(out["counts"]).reshape(-1)[0]), off, out["cells"], probe.want["records"], probe.want["paths"])


def _check_qmax_binary(probe, out):
    from .test_gpu_qmax_locate import _bits
    assert _bits(out["score"]) == _bits(probe.want["score"]), (probe.name, out["score"], probe.want["score"])


def _qmax_rec(a):
    from .test_gpu_qmax_locate import _rec
    return _rec(a)


def _dmax_rec(a):
    from .test_gpu_dmax_align import _rec
    return _rec(a)


CHECK = {
    "serra09_debug_bits": _check_debug_bits, "serra09_pairs": _check_scores, "chenfusion_pairs": _check_scores,
    "serra09_align": _check_record(_qmax_rec), "serra09_align_paths": _check_record(_qmax_rec), "serra09_align_sections": _check_sections,
    "chenfusion_align": _check_record(_dmax_rec), "chenfusion_align_paths": _check_record(_dmax_rec),
    "qmax_binary": _check_qmax_binary, "qmax_locate_binary": _check_record(_qmax_rec), "qmax_path_binary": _check_record(_qmax_rec),
    "qmax_sections_binary": _check_sections, "dmax_locate_binary": _check_record(_dmax_rec), "dmax_path_binary": _check_record(_dmax_rec),
}


# ---- EarlyFusion, stand-alone -------------------------------------------------------------------------------------------------------------
def _tenths_are(probe, out):
    from .test_gpu_ef_backend import _sw, _tenths
    assert _tenths(out["score"]) == probe.want["tenths"], (probe.name, out["score"], probe.want["tenths"])
    if "plot" in probe.want and max(probe.want["plot"].shape) <= 1024:
        assert _sw(probe.want["plot"]) == probe.want["tenths"], probe.name


def _check_csm_debug_bits(probe, out):
    from .test_gpu_ef_backend import _check_slot, _mean_ratio
    C, w = probe.info["matrix"], probe.want
    assert ("bits" in out) == (w["bits"] is not None), probe.name
    B = _check_slot(C, w["kb"], out["t"], out["jcut"], out.get("bits"), (probe.name,))
    assert np.array_equal(B, w["plot"]) and np.array_equal(out["jcut"], w["jcut"]), probe.name
    if w["bits"] is not None:
        assert np.array_equal(out["bits"], w["bits"]), probe.name
    print("%s: worst r error / bound %.3f" % (probe.name, _mean_ratio(out["r"], C, H.EF_K, 1, (probe.name,))))
    _tenths_are(probe, out)


def _check_sw_score(probe, out):
    from .test_gpu_ef_backend import _sw, _tenths
    assert _tenths(out["score"]) == probe.want["tenths"] == _sw(probe.info["plot"]()), (probe.name, out["score"])


def _check_sw_align(probe, out):
    from . import _sw_align_ref
    from .test_gpu_sw_align import _rec, _same
    rec, cells = _rec(out["records"][0]), out["cells"]
    assert _same(rec, probe.want["record"]) and np.array_equal(cells, probe.want["cells"]), (probe.name, rec, probe.want["record"])
    assert cells.dtype == np.int32 and cells.shape == (len(probe.want["cells"]), 2)
    _sw_align_ref.check_path(tuple(probe.want["record"]), cells, probe.info["plot"]().shape)


def _check_sw_sections(probe, out):
    from .test_gpu_sw_sections import _compare
    recs = out["records"].reshape(-1)
    off = np.asarray(out["offsets"])
    assert off.shape == (len(recs) + 1,) and off[0] == 0 and out["cells"].shape == (off[-1], 2), probe.name
    _compare(probe.name, len(recs), recs, int(np.asarray(out["counts"]).reshape(-1)[0]), off, out["cells"], probe.want["records"], probe.want["paths"])


def _check_xsel(probe, out):
    from .test_gpu_crossfusion import _score_eq
    w = probe.want
    assert np.array_equal(out["bits"], w["bits"]), (probe.name, np.argwhere(out["bits"] != w["bits"])[:5])
    assert _score_eq(out["score"], w["score"]), (probe.name, out["score"], w["score"])


# ---- rank, query, SiMPle, per-call buffers -----------------------------------------------------------------------------------------------------
class _Replay(object):
    """A context that returns a recorded result for the methods named and hands every other call to a context nobody filled: the
    checkers of the families' tests make the call under test themselves."""

    def __init__(self, clean, **recorded):
        self._clean, self._recorded = clean, recorded

    def __getattr__(self, name):
        if name in self._recorded:
            return lambda *a, **kw: self._recorded[name]
        return getattr(self._clean, name)


def _check_rank(probe, out):
    from . import test_gpu_rank as T
    D, rows, moff, mates, posn = H.rank_input(H.RANK_SMALL)
    if probe.kind == "rank_columns":
        T._check_rank(_Replay(None, rank_columns=(out["pos"], out["flag"])), D, rows, moff, mates, posn, expect_flags=[])
        assert np.array_equal(out["pos"], probe.want["pos"])
    else:
        T._check_topk(_Replay(None, topk_rows=(out["idx"], out["score"])), D, 10, rows=rows, posn=posn)
        assert np.array_equal(out["idx"], probe.want["idx"])


def _check_query(probe, out):
    from .test_gpu_query import _same
    w = probe.want
    if probe.kind == "query_ranks":
        assert out["pos"].shape == w["pos"].shape and np.array_equal(out["pos"], w["pos"]) and not out["flag"].any(), probe.name
        return
    assert np.array_equal(out["idx"][:, 0], w["idx"]) and _same(out["score"][:, 0], w["score"]), probe.name


def _check_simple_pairs(probe, out):
    from .test_gpu_simple_shapes import _check
    print("%s: worst error / bound %.3f" % (probe.name, _check(out["scores"], probe.want["scores"], probe.want["tol"], probe.name)))


def _check_simple_profile(probe, out):
    from .test_gpu_simple_profile import _check_continuous
    off = out["offsets"]
    K = len(probe.info["pairs"])
    got = (out["records"], [out["mp"][off[k]:off[k + 1]] for k in range(K)], [out["mpi"][off[k]:off[k + 1]] for k in range(K)])
    print("%s: worst error / bound %.3f, smallest gap / bound %.3g" % ((probe.name,) + _check_continuous(got, probe.want["refs"], H.SIMPLE_L, probe.name)))


def _check_ftm2d_track(probe, out):
    from .test_gpu_ftm2d import _check_stages
    _check_stages(out, *probe.info["args"])


def _check_snf(probe, out):
    from .test_gpu_snf import _check_fused
    _check_fused(probe.want["Ws"], probe.want["fused"], [out["W%d" % k] for k in range(len(probe.want["Ws"]))], out["fused"])


def _check_crossfusion(probe, out):
    from acoss_amd import _lib
    from .test_gpu_crossfusion import _check_stages
    clean = _lib.Context(0)
    try:
        a = H.XF_ARGS
        got = dict(out, score=float(out["score"]))
        _check_stages(_Replay(clean, crossfusion_matrices=got), *H.xf_triple(*H.XF_SMALL), a["K"], a["niters"], a["kappa"], probe.name)
    finally:
        clean.close()


def _check_grid(probe, out):
    from .test_gpu_ftm2d import _ulps
    D, want = out["D"], probe.want["D"]
    assert D.shape == want.shape and np.array_equal(D, D.T) and np.all(np.diag(D) == 0), probe.name
    if probe.kind == "pair_grid_serra09":
        np.testing.assert_array_equal(D, want)
    else:
        assert _ulps(D, want).max() <= 1, probe.name


CHECK.update({
    "csm_debug_bits": _check_csm_debug_bits, "csm_binary_sw": _tenths_are, "sw_binary": _check_sw_score, "sw_bits_binary": _check_sw_score,
    "sw_align_binary": _check_sw_align, "sw_sections_binary": _check_sw_sections, "xsel_binary_sw": _check_xsel,
    "rank_columns": _check_rank, "topk_rows": _check_rank, "query_topk": _check_query, "query_ranks": _check_query,
    "query_topk_lists": _check_query, "simple_pairs": _check_simple_pairs, "simple_profile": _check_simple_profile,
    "ftm2d_debug_track": _check_ftm2d_track, "snf_fuse_dists": _check_snf, "crossfusion_matrices": _check_crossfusion,
    "pair_grid_ftm2d": _check_grid, "pair_grid_serra09": _check_grid,
})


# ---- EarlyFusion, the product path: the specification on the device's own matrices ---------------------------------------------------------------
_YARDSTICK = {}


def _ef_yardstick(probe):
    """Per (list, K): the listed scores, and per pair its four matrices, from a context nobody filled; computed once, left unchanged."""
    from acoss_amd import _lib
    key = (probe.info["pairs"].tobytes(), probe.info["K"])
    if key not in _YARDSTICK:
        clean = _lib.Context(0)
        try:
            clean.ef_upload_pool(H.ef_pool())
            pairs, K = probe.info["pairs"], probe.info["K"]
            listed = clean.earlyfusion_pairs(pairs, H.EF_KAPPA, K)
            mats = []
            for k in range(len(pairs)):
                dm = clean.ef_debug_pairs(pairs, k, H.EF_KAPPA, K)
                assert np.array_equal(dm["scores"], listed)
                mats.append([dm["csm"][0], dm["csm"][1], dm["csm"][2], dm["fused"]])
            _YARDSTICK[key] = (listed, mats)
        finally:
            clean.close()
    return _YARDSTICK[key]


def _check_ef(probe, out):
    from . import _sw_align_ref
    from .test_gpu_ef_backend import _check_slot, _mean_ratio, _sw, _tenths
    from .test_gpu_sw_align import _rec, _same
    from .test_gpu_sw_sections import _compare
    listed, mats = _ef_yardstick(probe)
    k, K, plane = probe.info["which"], probe.info["K"], probe.info["plane"]
    plots = H.ef_plots(mats[k])
    assert mats[k][0].shape == probe.info["shape"], probe.name
    if probe.kind == "earlyfusion_pairs":
        assert np.array_equal(out["scores"].view(np.uint32), listed.view(np.uint32)), probe.name
        for kk in range(len(listed)):
            for s, (_, _, B) in enumerate(H.ef_plots(mats[kk])):
                assert _tenths(out["scores"][kk, s]) == _sw(B), (probe.name, kk, s)
        return
    if probe.kind == "ef_debug_bits":
        import oracle
        assert np.array_equal(out["scores"].view(np.uint32), listed.view(np.uint32)), probe.name
        assert ("bits" in out) == (max(H.EF_BLOCKS[t] for t in probe.info["pairs"].ravel()) <= 1024), probe.name
        worst = dict(r=0.0, c=0.0)
        for s in range(4):
            where = (probe.name, "slot %d" % s)
            C = mats[k][s]
            _check_slot(C, oracle.binary_k(H.EF_KAPPA, C.shape[1]), out["t"][s], out["jcut"][s], out["bits"][s] if "bits" in out else None, where)
            if s < 3:
                worst["r"] = max(worst["r"], _mean_ratio(out["r"][s], C, K, 1, where + ("r",)))
                worst["c"] = max(worst["c"], _mean_ratio(out["c"][s], C, K, 0, where + ("c",)))
        print("%s: worst error / bound r %.3f, c %.3f" % (probe.name, worst["r"], worst["c"]))
        return
    B = plots[plane][2]
    want = H.ef_want(probe.kind, B)
    n = len(listed)
    if probe.kind == "ef_align_sections":
        S_ = out["records"].shape[1]
        off = out["offsets"]
        assert out["records"].shape == (n, S_) and off.shape == (n * S_ + 1,) and off[0] == 0 and out["cells"].shape == (off[-1], 2), probe.name
        _compare(probe.name, S_, out["records"][k], int(out["counts"][k]), off[k * S_:(k + 1) * S_ + 1], out["cells"], want["records"], want["paths"])
        return
    al, off, cells = out["records"], out["offsets"], out["cells"]
    assert al.shape == (n,) and off.shape == (n + 1,) and off[0] == 0 and off[-1] == len(cells), probe.name
    got = cells[off[k]:off[k + 1]]
    assert _same(_rec(al[k]), want["record"]) and np.array_equal(got, want["cells"]), (probe.name, _rec(al[k]), want["record"])
    assert al["score"][k].view(np.uint32) == listed[k, plane].view(np.uint32), (probe.name, "earlyfusion_pairs")
    _sw_align_ref.check_path(tuple(want["record"]), got, B.shape)


CHECK.update({e: _check_ef for e in ("earlyfusion_pairs", "ef_debug_bits", "ef_align", "ef_align_long", "ef_align_sections")})


def _check_fused_lists(probe, out):
    from .test_gpu_fused import _Pool, _same
    q, lists, kw, k = probe.info["args"]()
    pool = _Pool("chen")
    try:
        _same((out["idx"], out["score"], out["flag"]), pool.want(q, lists, k, **kw), probe.name)
    finally:
        pool.ctx.close()
    assert not out["flag"].any(), probe.name


CHECK["query_fused_lists"] = _check_fused_lists


def _params(case):
    return [pytest.param(case, p, id=p.name.replace(" ", "_")) for p in case.probes]


def _hold(case, probe):
    outs = _under_every_word(case, probe)
    _same_bits(probe, outs)
    CHECK[probe.kind](probe, outs[0])


@pytest.mark.parametrize("case,probe", _params(H.serra09_product_case()))
def test_serra09_product_path(case, probe):
    """serra09_debug_bits, serra09_pairs and chenfusion_pairs at m = 9 behind a dense call (kappa 0.4 on 1017 x 1017 and 2041 x 505):
    ragged row bands and column tiles, both sides of the first class edge, the streaming class (D2^T and the strip records in
    d_scratch) and a 63 x 65 pair at m = 17.  Plots and scores."""
    _hold(case, probe)


@pytest.mark.parametrize("case,probe", _params(H.serra09_one_list_case()))
def test_serra09_probes_in_a_later_batch_of_one_list(case, probe):
    """The same probes behind the dense pairs inside ONE list, under a scratch limit that sends them to a later batch: the arenas
    they run in were written by an earlier batch of the same call (and filled before it)."""
    _hold(case, probe)


@pytest.mark.parametrize("case,probe", _params(H.serra09_align_case()))
def test_serra09_alignments(case, probe):
    """serra09_align, _align_paths, _align_sections, chenfusion_align and _align_paths (plane 1) on the same probes and on a 40 x 2049
    pair (seam records), each behind the same export on the dense pairs."""
    _hold(case, probe)


@pytest.mark.parametrize("case,probe", _params(H.serra09_plots_case()))
def test_serra09_stand_alone_plots(case, probe):
    """qmax_binary, qmax_locate / _path / _sections_binary, dmax_locate / _path_binary: an all-ones 64 x 2112 plot first, then a
    5 %-dense random 40 x 2049 plot and a 33 x 65 plot."""
    _hold(case, probe)


@pytest.mark.parametrize("case,probe", _params(H.ef_stand_alone_case()))
def test_earlyfusion_stand_alone(case, probe):
    """csm_debug_bits / csm_binary_sw behind 9 x 1088 matrices of -1e30 and +1e30 (9 x 1025: the long kernels; 12 x 513, 12 x 65: the
    register classes); sw_binary, sw_bits_binary, sw_align_binary and sw_sections_binary on sparse 33 x 65 and 5 x 1023 plots behind
    64 x 1024 ones; xsel_binary_sw on crafted rows of 65 and 5 columns behind rows of 1.0 at 1024."""
    _hold(case, probe)


@pytest.mark.parametrize("case,probe", _params(H.ef_product_case()))
def test_earlyfusion_product_path(case, probe):
    """A pool of 5 .. 1025 blocks; dirtied by (513, 513) and (140, 513) at K = 17 (which keeps C^T).  Bit-path probes at K = 10 and 17,
    float-path probes in a list with the 1025-block track: earlyfusion_pairs, ef_debug_bits, ef_align with paths, ef_align_sections
    and ef_align_long, against the specification on the matrices a context nobody filled returns for the same list."""
    _hold(case, probe)


@pytest.mark.parametrize("case,probe", _params(H.rank_case()) + _params(H.query_case()) + _params(H.fused_case()) + _params(H.simple_case()))
def test_rank_query_and_simple(case, probe):
    """rank_columns and topk_rows at n = 63 behind n = 4097; query_topk, query_ranks and query_topk_lists (Serra09, 22 tracks) behind
    the same export over 20 000 FTM2D shingles; query_fused_lists (LateFusionChen, K = 2, neighbourhoods of 4 and 5 tracks) behind
    neighbourhoods of every size up to 257; simple_pairs and simple_profile at L = 10 on tracks of 11, 12 and 25 frames behind
    all pairs of four 400-frame tracks."""
    _hold(case, probe)


@pytest.mark.parametrize("case,probe", _params(H.per_call_case()))
def test_entry_points_that_allocate_per_call(case, probe):
    """The allocation fill does the work: ftm2d_debug_track at (win 16, 17 beats) and (2, 2) behind (75, 160); snf_fuse_dists at n = 65
    behind 257; crossfusion_matrices at 12 x 30 behind 64 x 65; the symmetric pair_grid of FTM2D at n = 129 behind 257 and of Serra09
    at 5 tracks behind 12 -- the WHOLE returned matrix, the cells no pair writes included."""
    _hold(case, probe)
