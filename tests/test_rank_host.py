"""
CPU suite: the host side of the device evaluation path (acx_rank_columns / acx_topk_rows, eval_statistics_device,
getEvalStatistics(engine=...)).  No GPU needed: the device's answer is replaced by a numpy model of it
(tests/_rank_ref.py), so what is checked here is the plan the host sends and the code that turns the returned integer
positions into MR / MRR / MDR / MAP / Top-k -- the tail it shares with eval_statistics' counting branch.
"""
import os
import re

import numpy as np
import pytest

import oracle
from acoss_amd import _lib
from acoss_amd.algorithms import algorithm_template as at
from acoss_amd.algorithms.algorithm_template import CoverAlgorithm, eval_statistics
from acoss_amd.featurestore import save_track

from . import _rank_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_carries_the_ranking_calls():
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    L = _lib.load()
    for sym in ("acx_rank_columns", "acx_topk_rows"):
        assert re.search(r"\bint %s\(acx_ctx \*ctx" % sym, header), sym
        assert sym in _lib.EXPORTS
        assert hasattr(L, sym)
    assert _lib.ABI_VERSION == 4 and L.acx_abi_version() == 4
    assert "#define ACX_ABI_VERSION 4" in header


def _plan_by_hand(cliques, N):
    """rank_plan restated with loops."""
    order = sorted(range(len(cliques)), key=lambda i: -len(cliques[i]))         # (sorted is stable)
    layout = [t for i in order for t in cliques[i]]
    posn = [0] * N
    for p, t in enumerate(layout):
        posn[t] = p
    clique_of = {}
    for i in order:
        for t in cliques[i]:
            clique_of[t] = cliques[i]
    evaluated = sorted(t for t in range(N) if len(clique_of[t]) >= 2)
    rows = evaluated
    if evaluated and 2 * len(evaluated) >= evaluated[-1] - evaluated[0] + 1:
        rows = list(range(evaluated[0], evaluated[-1] + 1))
    moff, mates = [0], []
    for t in rows:
        if len(clique_of[t]) >= 2:
            mates += [m for m in clique_of[t] if m != t]
        moff.append(len(mates))
    return layout, posn, rows, moff, mates


@pytest.mark.parametrize("cliques, N", [
    ([[0, 5], [3], [1, 2, 7], [4], [6, 8]], 9),                   # singletons inside the span: the whole span is sent
    ([[2], [0, 19], [1], [3], [4], [5], [6], [7], [8], [9], [10], [11], [12], [13], [14], [15], [16], [17], [18]], 20),   # sparse: two rows only
    ([[0], [1], [2]], 3),                                         # nothing to evaluate
])
def test_rank_plan_against_a_literal_restatement(cliques, N):
    plan = at.rank_plan(cliques, N)
    layout, posn, rows, moff, mates = _plan_by_hand(cliques, N)
    assert plan["idx"].tolist() == layout
    assert plan["posn"].tolist() == posn and plan["posn"].dtype == np.int32
    assert plan["rows"].tolist() == rows and plan["rows"].dtype == np.int32
    assert plan["moff"].tolist() == moff and plan["moff"].dtype == np.int64
    assert plan["mates"].tolist() == mates and plan["mates"].dtype == np.int32
    assert plan["n_eval"] == sum(len(c) for c in cliques if len(c) >= 2)
    for e in range(plan["n_eval"]):          # where: the mates of the e-th track of the layout
        a, cnt = plan["where"][e]
        t = layout[e]
        assert sorted(plan["mates"][a:a + cnt].tolist()) == sorted(m for c in cliques if t in c for m in c if m != t)
    if N == 20:
        assert rows == [0, 19]
    if N == 9:
        assert rows == list(range(9)) and moff[4] - moff[3] == 0 and moff[5] - moff[4] == 0


def test_rank_plan_wants_every_track_once():
    with pytest.raises(ValueError, match="every track"):
        at.rank_plan([[0, 1], [1, 2]], 3)
    with pytest.raises(ValueError, match="every track"):
        at.rank_plan([[0, 1]], 3)


def _device_model(D, cliques, topsidx, row_block=1024, info=None):
    """eval_statistics_device with the numpy model in the device's place."""
    plan = at.rank_plan(cliques, D.shape[0])
    pos, flag = ref.rank_columns(D, plan["rows"], plan["moff"], plan["mates"], plan["posn"])
    return at._statistics_from_positions(D, plan, pos, flag, topsidx, row_block, info)


def _random_collection(rng, n_cliques, max_size, levels):
    sizes = list(rng.integers(1, max_size + 1, size=n_cliques))
    n = int(sum(sizes))
    perm = rng.permutation(n)
    cl, p = [], 0
    for s in sizes:
        cl.append(sorted(perm[p:p + s].tolist()))
        p += s
    D = rng.random((n, n)).astype(np.float32)
    if levels:
        D = (np.round(D * levels) / levels).astype(np.float32)
    return D, cl


def test_shared_tail_reproduces_the_counting_branch_exactly():
    rng = np.random.default_rng(12)
    for trial in range(12):
        D, cl = _random_collection(rng, int(rng.integers(4, 14)), [5, 13, 30][trial % 3], [0, 3, 8, 10 ** 6][trial % 4])
        for rb in (7, 1024):
            info = {}
            got = _device_model(D, cl, (1, 3, 10), row_block=rb, info=info)
            want = eval_statistics(D, cl, topsidx=(1, 3, 10), row_block=rb, count_max_clique=10 ** 9)
            assert got[:4] == want[:4], (trial, rb, got, want)              # bit for bit, MAP included
            assert np.array_equal(got[4], want[4])
            assert info == {"device_rows": sum(len(c) for c in cl if len(c) >= 2), "host_rows": 0}
        for other in (eval_statistics(D, cl, topsidx=(1, 3, 10)), oracle.eval_statistics(D, cl, topsidx=(1, 3, 10), stable=True)):
            np.testing.assert_allclose(np.array(got[:4]), np.array(other[:4]), rtol=1e-12)
            assert np.array_equal(got[4], other[4])


def test_shared_tail_on_the_reference_goldens(golden):
    g = golden("harness")
    cl = ref.cliques_of(g["labels"])
    for tag in ("sym", "asym"):
        res = _device_model(g["D_" + tag], cl, (1, 2, 5))
        got = np.array(list(res[:4]) + list(res[4]))
        np.testing.assert_allclose(got, g["stats_" + tag], rtol=1e-12)
        want = eval_statistics(g["D_" + tag], cl, topsidx=(1, 2, 5), count_max_clique=10 ** 9)
        assert res[:4] == want[:4] and np.array_equal(res[4], want[4])


def test_flagged_rows_take_the_sorting_branch():
    rng = np.random.default_rng(4)
    D, cl = _random_collection(rng, 12, 6, 8)
    n = D.shape[0]
    evaluated = [t for c in cl if len(c) >= 2 for t in c]
    planted = evaluated[::5]
    for k, t in enumerate(planted):
        D[t, (t + 1 + k) % n if (t + 1 + k) % n != t else (t + 2 + k) % n] = [np.nan, -np.inf][k % 2]
    info = {}
    got = _device_model(D, cl, (1, 3, 10), row_block=5, info=info)
    assert info["host_rows"] == len(planted) and info["device_rows"] == len(evaluated) - len(planted)
    want = eval_statistics(D, cl, topsidx=(1, 3, 10), count_max_clique=0)
    assert (got[0], got[1], got[2]) == (want[0], want[1], want[2]) and np.array_equal(got[4], want[4])
    np.testing.assert_allclose(got[3], want[3], rtol=1e-12)


def _toy(tmp_path, labels, S):
    csv = tmp_path / "toy.csv"
    with open(csv, "w") as f:
        f.write("work_id,track_id\n")
        for k, l in enumerate(labels):
            f.write("%s,t%d\n" % (l, k))
    root = str(tmp_path) + "/"
    for k, l in enumerate(labels):
        save_track(root + "%s/t%d.h5" % (l, k), {"label": l, "track_id": "t%d" % k, "hpcp": np.zeros((3, 12), np.float32)})

    class Toy(CoverAlgorithm):
        def __init__(self):
            CoverAlgorithm.__init__(self, str(csv), name="Toy", datapath=root, shortname="toy")

        def similarity(self, idxs):
            for i, j in zip(idxs[:, 0], idxs[:, 1]):
                self.Ds["main"][i, j] = S[i, j]

    toy = Toy()
    for k in range(toy.N):
        toy.load_features(k)
    toy.all_pairwise(parallel=0, symmetric=False)
    return toy


def test_engine_switch_of_getEvalStatistics(golden, tmp_path, monkeypatch):
    g = golden("harness")
    monkeypatch.chdir(tmp_path)
    toy = _toy(tmp_path, [str(l) for l in g["labels"]], g["Strue"])
    assert CoverAlgorithm.eval_engine == "host"
    a = toy.getEvalStatistics("main", topsidx=[1, 2, 5])
    b = toy.getEvalStatistics("main", topsidx=[1, 2, 5], engine="host")
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4])
    np.testing.assert_allclose(np.array(list(a[:4]) + list(a[4])), g["stats_asym"], rtol=1e-12)
    lines = open("results_toy_Toy.csv").read().splitlines()
    ref_lines = str(g["results_csv"]).splitlines()
    assert lines[0] == ref_lines[0] == "name, MR, MRR, MDR, MAP,Top-1,Top-2,Top-5"
    assert lines[1] == lines[2] == ref_lines[-1]                      # the same CSV row as before, from both spellings
    with pytest.raises(ValueError, match="engine"):
        toy.getEvalStatistics("main", engine="gpu")
    try:
        probe = _lib.Context(0)
    except _lib.AcxError:
        probe = None
    if probe is None:
        # no GPU: the device engine raises what _lib.Context raises -- never a silent host result
        with pytest.raises(_lib.AcxError):
            toy.getEvalStatistics("main", topsidx=[1, 2, 5], engine="device")
        with pytest.raises(_lib.AcxError):
            toy.top_matches("main", k=3)
        assert len(open("results_toy_Toy.csv").read().splitlines()) == 3      # and writes no row
    else:
        probe.close()
        c = toy.getEvalStatistics("main", topsidx=[1, 2, 5], engine="device")
        assert c[:4] == a[:4] and np.array_equal(c[4], a[4])
    toy.cleanup_memmap()
