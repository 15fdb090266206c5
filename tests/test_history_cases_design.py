"""
CPU suite: what the cases of tests/_history_cases.py (tests/test_gpu_arena_history.py runs them on the GPU) are made of.

  * the reference of every probe is what the suite's reference modules give for the probe's input, derived here a second time
    straight from the input (no helper of the case module in between);
  * wherever a plan report exists, the dirtying call covers the probe: from the report's `need` fields (acx_ef_plan), and for
    Serra09 -- whose report has no such field -- from its Mq, Mr, class and batch fields.  The code under test is not asked.
"""
import numpy as np
import pytest

from . import _history_cases as H
from . import _serra09_shapes as S


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_fill_words():
    assert H.WORDS == (0x00000000, 0xFFFFFFFF, 0x7F800000, 0x00000001, 0x55555555)
    f = np.array(H.WORDS, np.uint32).view(np.float32)
    assert np.isnan(f[1]) and np.isposinf(f[2]) and 0 < f[3] < np.finfo(np.float32).tiny
    assert np.isnan(np.array([0xFFFFFFFF, 0xFFFFFFFF], np.uint32).view(np.float64)[0])
    assert all((H.WORDS[4] >> (2 * e)) & 3 == 1 for e in range(16)) and all((H.WORDS[1] >> (2 * e)) & 3 == 3 for e in range(16))


# ---- Serra09 --------------------------------------------------------------------------------------------------------------------------------------
def _oracle_pair(i, j, m, kappa=0.095, oti=True):
    import oracle
    oracle.lib()
    d = H.serra09_pool()
    s, it = oracle.serra09_pair(S.track(d, i), S.track(d, j), oracle.serra09_params(m=m, kappa=kappa, oti=oti), want_intermediates=True)
    return np.float32(s), it["R"]


def _plot_references(R):
    """What the reference modules say of a plot, by the export that returns it."""
    import oracle
    from . import _dmax_align_ref, _qmax_locate_ref, _qmax_path_ref, _qmax_sections_ref
    prec, pcells, _ = _qmax_path_ref.path_full(R, 0.5, 0.5, 2)
    drec, dcells, _ = _dmax_align_ref.dmax_full(R, 0.5, 0.5, 2)
    srecs, spaths = _qmax_sections_ref.sections_full(R, 0.5, 0.5, 2)
    loc = dict(record=_qmax_locate_ref.locate_forward(R, 0.5, 0.5, 2))
    assert loc["record"] == prec
    return {"qmax": np.float32(oracle.qmax_binary(R, 0.5, 0.5, False)), "dmax": np.float32(oracle.qmax_binary(R, 0.5, 0.5, True)),
            "locate": loc, "path": dict(record=prec, cells=pcells), "sections": dict(records=srecs, paths=spaths),
            "dlocate": dict(record=drec), "dpath": dict(record=drec, cells=dcells)}


_BY_EXPORT = {"serra09_align": "locate", "serra09_align_paths": "path", "serra09_align_sections": "sections", "chenfusion_align": "dlocate",
              "chenfusion_align_paths": "dpath", "qmax_locate_binary": "locate", "qmax_path_binary": "path", "qmax_sections_binary": "sections",
              "dmax_locate_binary": "dlocate", "dmax_path_binary": "dpath"}


@pytest.mark.parametrize("case", [H.serra09_product_case(), H.serra09_align_case()], ids=lambda c: c.name.replace(" ", "_"))
def test_serra09_probe_references(case):
    refs = {}
    for probe in case.probes:
        shape, m = probe.info["shape"], probe.info["m"]
        (i, j), = probe.info["pairs"]
        if (shape, m) not in refs:
            score, R = _oracle_pair(int(i), int(j), m, oti=shape != H.SEAM_PROBE)
            assert R.shape == shape, (probe.name, R.shape)
            refs[(shape, m)] = (score, R, _plot_references(R))
        score, R, by = refs[(shape, m)]
        assert score.view(np.uint32) == by["qmax"].view(np.uint32), probe.name           # the chain's score is the sweep's on its plot
        if probe.kind == "serra09_debug_bits":
            want = dict(scores=np.array([score]), plots=[R])
        elif probe.kind == "serra09_pairs":
            want = dict(scores=np.array([score]))
        elif probe.kind == "chenfusion_pairs":
            want = dict(scores=np.array([[score, by["dmax"]]]))
        else:
            want = by[_BY_EXPORT[probe.kind]]
        assert _same(probe.want, want), probe.name


def test_serra09_probes_meet_alignments():
    """The probes are no empty plots: every shape with four rows and columns or more has a Qmax alignment, and the seam probe's
    crosses column 2048."""
    by = {p.info["shape"]: p.want["record"] for p in H.serra09_align_case().probes if p.kind == "serra09_align"}
    assert all(rec[0] > 0 for shape, rec in by.items() if min(shape) >= 4), by
    assert by[H.SEAM_PROBE][2] < 2048 <= by[H.SEAM_PROBE][4], by[H.SEAM_PROBE]


def test_serra09_dirtying_call_covers_the_probes():
    """From the plan's report: the dense pairs and every band-class probe run in ONE batch each (what debug_bits needs), in band
    classes -- their arenas are the bitmap and threshold arenas, which grow with the cells and the sides of a batch --, and no band
    probe has more cells or a longer side than a dense pair; the streaming probes are of class 5 and take scratch the dense call
    never allocated: they run in blocks that grow inside the probe, whose contents the allocation fill decides."""
    from acoss_amd import _lib
    lens = np.diff(H.serra09_pool()["offsets"])
    dense = _lib.serra09_plan(lens, H.serra09_pairs(H.DENSE), H._params(kappa=H.DENSE_KAPPA))
    assert [(int(r["Mq"]), int(r["Mr"])) for r in dense] == list(H.DENSE) and np.all(dense["batch"] == 0) and np.all(dense["cr"] < S.NC)
    cells = int(np.sum(dense["Mq"].astype(np.int64) * dense["Mr"]))
    for shape in H.BAND_PROBES:
        rec, = _lib.serra09_plan(lens, H.serra09_pairs([shape]), H._params())
        assert (int(rec["Mq"]), int(rec["Mr"])) == shape and rec["cr"] < S.NC and rec["cq"] < S.NC
        assert shape[0] * shape[1] <= cells and shape[0] <= dense["Mq"].max() and shape[1] <= dense["Mr"].max(), shape
    for shape in H.STREAM_PROBES + (H.SEAM_PROBE,):
        rec, = _lib.serra09_plan(lens, H.serra09_pairs([shape]), H._params())
        assert (int(rec["Mq"]), int(rec["Mr"]), int(rec["cr"])) == shape + (S.NC,)
    rec, = _lib.serra09_plan(lens, H.serra09_pairs([H.STACK17], H.M17), H._params(H.M17))
    assert (int(rec["Mq"]), int(rec["Mr"]), int(rec["cr"])) == H.STACK17 + (S.NC,)
    # both sides of the first class edge, ragged bands (rows mod 8) and ragged tiles (columns mod 64)
    assert {S.cls(249), S.cls(250)} == {0, 1} and {a % 8 for a, _ in H.BAND_PROBES} >= {1, 2, 3} and all(b % 64 for _, b in H.BAND_PROBES)


def test_serra09_one_list_runs_the_probes_in_a_later_batch():
    from acoss_amd import _lib
    lens = np.diff(H.serra09_pool()["offsets"])
    for probe in H.serra09_one_list_case().probes:
        shapes = probe.info["shapes"]
        limit = H.one_list_limit(shapes)
        plan = _lib.serra09_plan(lens, probe.info["pairs"], H._params(kappa=H.DENSE_KAPPA), scratch_limit=limit)
        nd = len(H.DENSE)
        assert plan["batch"][0] == 0 and plan["batch"][nd:].min() >= 1, (probe.name, limit, plan["batch"].tolist())
        assert np.array_equal(probe.info["pairs"][:nd], probe.info["dense"])
        want_scores, Rs = [], []
        for i, j in probe.info["pairs"]:
            s, R = _oracle_pair(int(i), int(j), H.M9, H.DENSE_KAPPA)
            want_scores.append(s)
            Rs.append(R)
        want = np.array(want_scores, np.float32)
        if probe.kind == "chenfusion_pairs":
            import oracle
            want = np.stack([want, np.array([oracle.qmax_binary(R, 0.5, 0.5, True) for R in Rs], np.float32)], 1)
        assert _same(probe.want, dict(scores=want)), probe.name


def test_serra09_plot_references():
    ones = np.ones(H.ONES_PLOT, np.uint8)
    for probe in H.serra09_plots_case().probes:
        R = probe.info["plot"]()
        assert R.shape[0] <= ones.shape[0] and R.shape[1] <= ones.shape[1] and 0.03 < R.mean() < 0.07, (probe.name, R.shape, R.mean())
        by = _plot_references(R)
        want = dict(score=by["qmax"]) if probe.kind == "qmax_binary" else by[_BY_EXPORT[probe.kind]]
        assert _same(probe.want, want), probe.name
    # the dirtying plot spans two strips of the locating sweep and of the path pass, as the 40 x 2049 probe does
    assert H.ONES_PLOT[1] > 2048 and any(p.info["plot"]().shape[1] > 2048 for p in H.serra09_plots_case().probes)


# ---- EarlyFusion ------------------------------------------------------------------------------------------------------------------------------------
def test_earlyfusion_stand_alone_references():
    import oracle
    from . import _crossfusion_ref, _ef_backend_ref, _sw_align_ref, _sw_sections_ref
    seen = set()
    for probe in H.ef_stand_alone_case().probes:
        seen.add(probe.kind)
        if probe.kind in ("csm_debug_bits", "csm_binary_sw"):
            C = probe.info["matrix"]
            # (rows of the matrix arena are a multiple of 64 floats apart: the probe takes no more of it than the dirtying matrices)
            assert C.shape in H.CSM_PROBES and C.shape[0] * ((C.shape[1] + 63) // 64 * 64) <= H.CSM_DIRT[0] * H.CSM_DIRT[1]
            kb = oracle.binary_k(H.EF_KAPPA, C.shape[1])
            t, jcut = _ef_backend_ref.thresholds(C, kb)
            B = _ef_backend_ref.binarise(C, t, jcut)
            assert 0 < kb < C.shape[1] and np.all(B.sum(1) == kb)
            want = dict(kb=kb, t=t, jcut=jcut, plot=B, tenths=_ef_backend_ref.sw_tenths(B),
                        bits=_ef_backend_ref.pack_bits(B) if max(C.shape) <= 1024 else None)
            assert sorted(want) == sorted(probe.want) and all(_same(probe.want[k], want[k]) for k in want if want[k] is not None), probe.name
            assert (probe.want["bits"] is None) == (max(C.shape) > 1024)
        elif probe.kind == "xsel_binary_sw":
            X, kappa = probe.info["rows"], probe.info["kappa"]
            assert X.shape[1] <= H.XSEL_DIRT[1] and X.shape[0] <= H.XSEL_DIRT[0]
            B = _crossfusion_ref.select(X, _crossfusion_ref.binary_k(kappa, X.shape[1]))
            assert B.any()
            assert _same(probe.want, dict(bits=_crossfusion_ref.pack_bits(B), plot=B, score=oracle.sw_constrained(B))), probe.name
        else:
            B = probe.info["plot"]()
            assert B.shape in H.SW_PROBES and B.shape[0] <= H.SW_ONES[0] and B.shape[1] <= H.SW_ONES[1] and 0 < B.mean() < 0.1
            if probe.kind in ("sw_binary", "sw_bits_binary"):
                want = dict(tenths=_ef_backend_ref.sw_tenths(B))
                assert want["tenths"] == oracle.sw_constrained_i32(B) > 0
            elif probe.kind == "sw_align_binary":
                rec, cells = _sw_align_ref.align_forward(B)
                want = dict(record=rec, cells=cells)
                assert len(cells) >= 1
            else:
                recs, paths = _sw_sections_ref.sections_full(B)
                want = dict(records=recs, paths=paths)
            assert _same(probe.want, want), probe.name
    assert seen == {"csm_debug_bits", "csm_binary_sw", "xsel_binary_sw"} | set(H.SW_EXPORTS)


def test_earlyfusion_product_dirtying_call_covers_the_probes():
    """From acx_ef_plan's `need` (floats of the scratch arena a pair takes): the dirtying list takes more than any probe list, runs in
    one batch on the bit path and keeps C^T (K > 16: the column statistics are the row pass on the transposed matrices); the bit
    probes run on the bit path, the list with the 1025-block track on the float path."""
    from acoss_amd import _lib
    blocks = np.array(H.EF_BLOCKS)
    dense = np.array(sorted(H.EF_DIRTY), np.int32)
    dirty = _lib.ef_plan(blocks, dense, H.EF_KAPPA, H.EF_DIRTY_K)
    assert sorted((int(r["M"]), int(r["N"])) for r in dirty) == [(140, 513), (513, 513)]
    assert np.all(dirty["batch"] == 0) and np.all(dirty["path"] == 0) and np.all(dirty["col_kernel"] == 0)      # ACX_EF_COL_ROWPASS
    lists = {}
    for probe in H.ef_product_case().probes:
        lists[(probe.info["pairs"].tobytes(), probe.info["K"])] = probe
        assert np.array_equal(probe.info["dense"], dense)
    assert len(lists) == len(H.EF_KS) * (len(H.EF_BIT_PROBES) + 1)
    for probe in lists.values():
        pairs, K = probe.info["pairs"], probe.info["K"]
        plan = _lib.ef_plan(blocks, pairs, H.EF_KAPPA, K)
        shapes = sorted((int(r["M"]), int(r["N"])) for r in plan)
        long_list = len(pairs) > 1
        assert shapes == sorted(H.EF_FLOAT_LIST if long_list else [probe.info["shape"]]), probe.name
        assert np.all(plan["batch"] == 0) and np.all(plan["path"] == (1 if long_list else 0)), probe.name
        assert int(dirty["need"].sum()) >= int(plan["need"].sum()) > 0, (probe.name, dirty["need"].tolist(), plan["need"].tolist())
        assert np.array_equal(pairs, pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]), "ef_debug_bits wants a sorted list"
    assert {K > 16 for K in H.EF_KS} == {False, True}


def test_earlyfusion_product_references_are_the_modules():
    """ef_plots / ef_want on matrices of a probe's shape: thresholds, binarise, align_forward and sections_full, nothing else."""
    import oracle
    from . import _ef_backend_ref, _sw_align_ref, _sw_sections_ref
    rng = np.random.default_rng(5)
    mats = [rng.random((64, 65)).astype(np.float32) for _ in range(4)]
    for C, (t, jcut, B) in zip(mats, H.ef_plots(mats)):
        wt, wj = _ef_backend_ref.thresholds(C, oracle.binary_k(H.EF_KAPPA, 65))
        assert _same(t, wt) and _same(jcut, wj) and _same(B, _ef_backend_ref.binarise(C, wt, wj))
        rec, cells = _sw_align_ref.align_forward(B)
        assert _same(H.ef_want("ef_align", B), dict(record=rec, cells=cells)) and _same(H.ef_want("ef_align_long", B), dict(record=rec, cells=cells))
        recs, paths = _sw_sections_ref.sections_full(B)
        assert _same(H.ef_want("ef_align_sections", B), dict(records=recs, paths=paths))


# ---- rank, query, SiMPle, per-call buffers ---------------------------------------------------------------------------------------------------------
def test_rank_references():
    from . import _rank_ref
    D, rows, moff, mates, posn = H.rank_input(H.RANK_SMALL)
    big = H.rank_input(H.RANK_LARGE)
    assert D.shape == (24, 63) and big[0].shape == (24, 4097) and len(np.unique(D)) <= 9          # heavy ties
    by = {p.kind: p for p in H.rank_case().probes}
    pos, flag = _rank_ref.rank_columns(D, rows, moff, mates, posn)
    assert _same(by["rank_columns"].want, dict(pos=pos, flag=flag)) and not flag.any()
    idx, score = _rank_ref.topk_rows(D, 10, rows=rows, posn=posn)
    assert _same(by["topk_rows"].want, dict(idx=idx, score=score))


def test_query_references():
    import oracle
    from . import _query_lists_ref, _query_ref
    d, a, q = H.query_pool(), H.query_args(), list(H.QUERIES)
    rows = H.query_rows()
    n = a["n"]
    assert rows.shape == (len(q), n) and np.all(rows[np.arange(len(q)), q] == 0)
    for i, qq in enumerate(q):                      # cell (q, c): the oracle's score of the pair (min, max)
        for c in (0, n // 2, n - 1):
            if c != qq:
                want = oracle.serra09_pairs(d["frames"], d["offsets"], np.array([[min(qq, c), max(qq, c)]], np.int32))[0]
                assert rows[i, c].view(np.uint32) == np.float32(want).view(np.uint32)
    by = {p.kind: p for p in H.query_case().probes}
    idx, score = _query_ref.topk(rows, q, H.QUERY_K, col=a["col"], col_mode=1)
    assert _same(by["query_topk"].want, dict(idx=idx, score=score))
    idx, score = _query_lists_ref.topk_lists(rows, q, a["lists"], 4, col=a["col"], col_mode=1)
    assert _same(by["query_topk_lists"].want, dict(idx=idx, score=score))
    fin = _query_ref.scores(rows, q, a["col"], 1)
    for i in range(len(q)):                         # a position: 1 + the columns that rank before the mate (no ties in these rows)
        for m, pos in zip(a["mates"][a["moff"][i]:a["moff"][i + 1]], by["query_ranks"].want["pos"][0][a["moff"][i]:a["moff"][i + 1]]):
            others = np.delete(fin[i], q[i])
            assert pos == 1 + int(np.sum(others > fin[i, m])), (i, m)


def test_simple_references():
    from . import _simple_profile_ref, _simple_ref
    T = H.simple_tracks()
    assert tuple(len(t) for t in T) == H.SIMPLE_SMALL + H.SIMPLE_LARGE and min(H.SIMPLE_SMALL) == H.SIMPLE_L + 1
    by = {p.kind: p for p in H.simple_case().probes}
    pairs = by["simple_pairs"].info["pairs"]
    assert len(pairs) == 6 and pairs.max() == 2
    for k, (i, j) in enumerate(pairs):
        ref = _simple_ref.score_exact(T[i], T[j], H.SIMPLE_L, True)[0]
        assert by["simple_pairs"].want["scores"][k] == ref and by["simple_pairs"].want["tol"][k] == _simple_ref.score_tol(T[i], T[j], H.SIMPLE_L, ref)
        mp, mpi, gap, s, bound = _simple_profile_ref.reference(T[i], T[j], H.SIMPLE_L, True)
        assert _same(by["simple_profile"].want["refs"][k][:3], (mp, mpi, gap)) and by["simple_profile"].want["refs"][k][3] == s
        assert np.all(gap > 2.0 * bound), "every row of the probes' profiles is decided"


def test_per_call_references():
    import oracle
    from . import _crossfusion_ref, _ftm2d_ref, _snf_ref
    by = {p.name: p for p in H.per_call_case().probes}
    for win, nbeats in H.FTM_PROBES:
        p = by["ftm2d_debug_track win=%d beats=%d" % (win, nbeats)]
        X, on, pwr, w, C, nb = p.info["args"]
        assert (w, nb) == (win, nbeats) and win <= H.FTM_DIRT[0] and nbeats <= H.FTM_DIRT[1]
        assert _same(p.want, _ftm2d_ref.stages(X, on, pwr, win, C))
    p = by["snf_fuse_dists n=%d" % H.SNF_SMALL]
    Ds = H.snf_dists(H.SNF_SMALL)
    Ws, fused = oracle.snf_fuse(Ds, K=20, niters=5, reg_diag=1)
    assert _same(p.want, dict(Ws=Ws, fused=fused))
    Ws2, fused2 = _snf_ref.fuse(Ds, 20, 5, 1.0)                   # the per-stage restatement agrees with the oracle
    np.testing.assert_allclose(np.asarray(fused2, np.float64), fused, rtol=1e-10, atol=1e-14)
    p = by["crossfusion_matrices %dx%d" % H.XF_SMALL]
    a = H.XF_ARGS
    assert _same(p.want, _crossfusion_ref.chain(*H.xf_triple(*H.XF_SMALL), a["K"], a["niters"], a["reg_diag"], a["kappa"]))
    n = H.GRID_FTM[0]
    D = by["pair_grid ftm2d n=%d" % n].want["D"]
    i, j = np.triu_indices(n, 1)
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0)
    assert np.array_equal(D[i, j], _ftm2d_ref.pair_scores(H.grid_shingles(n), np.stack([i, j], 1)).astype(np.float32))
    n = H.GRID_SERRA09[0]
    D = by["pair_grid serra09 n=%d" % n].want["D"]
    d = H.grid_serra09_pool()
    i, j = np.triu_indices(n, 1)
    assert np.array_equal(D, D.T) and np.all(np.diag(D) == 0) and len(d["offsets"]) - 1 == H.GRID_SERRA09[1]
    assert np.array_equal(D[i, j], oracle.serra09_pairs(d["frames"][:d["offsets"][n]], d["offsets"][:n + 1], np.stack([i, j], 1).astype(np.int32)))


def test_every_case_is_held():
    """Every probe of every case has a checker in the GPU test, and the CPU cases have references."""
    from . import test_gpu_arena_history as G
    cases = H.cpu_cases() + [H.ef_product_case(), H.fused_case()]
    kinds = {p.kind for c in cases for p in c.probes}
    assert kinds == set(G.CHECK), (kinds ^ set(G.CHECK))
    names = [p.name for c in cases for p in c.probes]
    assert len(names) == len(set(names))


def test_fused_lists_case():
    """The probe is test_gpu_fused.py's smallest call (K = 2: n = K + 2 and one more), the dirtying call its largest (n up to 257)."""
    from . import _fused_ref
    probe, = H.fused_case().probes
    q, lists, kw, k = probe.info["args"]()
    assert kw == dict(K=2, niters=2) and sorted(len(_fused_ref.neighbourhood(a, r)[0]) for a, r in zip(q, lists)) == [4, 4, 5, 5]
    assert len(H.fused_pool()[1]) - 1 == 262
