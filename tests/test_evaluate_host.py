"""
Host-side checks of the evaluation of a query set (CoverAlgorithm.evaluate, acx_query_ranks): the numpy yardstick the
GPU tests grade against (tests/_evalq_ref.py) proved against eval_statistics, the ABI surface, the Python-side argument
checks -- none of which may touch a GPU -- and the planning of a query subset, which is pure numpy.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from . import _evalq_ref
from . import _rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tied_matrix(rng, n, levels):
    D = rng.integers(0, levels, size=(n, n)).astype(np.float32)
    D[rng.random((n, n)) < 0.05] = -0.0
    return D


@pytest.mark.parametrize("seed", range(6))
def test_reference_agrees_with_eval_statistics(seed):
    """queries=None on finite matrices full of ties and signed zeros: the integer statistics exactly, MAP and MRR to
    1e-12 relative -- the agreement DESIGN.md section 11 states between the host branches (counting and sorting)."""
    from acoss_amd.algorithms.algorithm_template import eval_statistics
    rng = np.random.default_rng(300 + seed)
    cliques, n = _rank_ref.datacos_cliques(int(rng.integers(3, 9)), int(rng.integers(2, 5)), int(rng.integers(0, 6)), seed)
    D = _tied_matrix(rng, n, levels=int(rng.integers(2, 7)))
    tops = (1, 3, 10)
    for count_max in (24, 0):                     # the counting branch and the sorting branch
        MR, MRR, MDR, MAP, top = eval_statistics(D, cliques, tops, count_max_clique=count_max)
        rMR, rMRR, rMDR, rMAP, rtop = _evalq_ref.statistics(D, cliques, None, tops)
        assert np.array_equal(top, rtop) and MDR == rMDR and MR == rMR       # (a sum of integers is exact in any order)
        assert MRR == pytest.approx(rMRR, rel=1e-12) and MAP == pytest.approx(rMAP, rel=1e-12)


def test_reference_by_hand():
    """Four tracks, one clique of two plus two singletons, positions worked out by hand."""
    cliques = [[3], [0, 2], [1]]                  # layout: 0 2 3 1
    D = np.array([[0, 5, 5, 5],
                  [1, 0, 1, 1],
                  [7, 9, 0, 7],
                  [2, 2, 2, 0]], np.float32)
    # row 0: columns in layout order without 0: 2, 3, 1 -- all 5: the mate 2 comes first.  row 2: 0, 3, 1 -> 7, 7, 9: 1 first,
    # then 0 (before 3 in the layout): position 2
    assert _evalq_ref.mate_positions(D, cliques) == [(0, [1]), (2, [2])]
    MR, MRR, MDR, MAP, tops = _evalq_ref.statistics(D, cliques, None, (1, 2))
    assert (MR, MDR, MAP) == (1.5, 1.5, 0.75) and MRR == (1.0 + 0.5) / 4 and tops.tolist() == [1, 2]
    MR, MRR, MDR, MAP, tops = _evalq_ref.statistics(D, cliques, [1, 2], (1, 2))
    assert (MR, MDR, MAP) == (2.0, 2.0, 0.5) and MRR == 0.5 / 2 and tops.tolist() == [0, 1]
    assert _evalq_ref.flagged_rows(D, cliques) == 0
    D[2, 3] = -np.inf
    D[1, 0] = np.nan                              # (track 1 is a singleton: not evaluated, not counted)
    assert _evalq_ref.flagged_rows(D, cliques) == 1 and _evalq_ref.flagged_rows(D, cliques, [0, 1]) == 0


def test_symbol_in_header_exports_and_library():
    from acoss_amd import _lib
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    assert re.search(r"\bint acx_query_ranks\(acx_ctx \*", header)
    assert _lib.EXPORTS.count("acx_query_ranks") == 1
    assert re.search(r"#define ACX_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libacx.so is not built: build() comes before the tests")
    L = ctypes.CDLL(_lib.LIB_PATH)                # (no device is needed to look symbols up)
    assert hasattr(L, "acx_query_ranks")


def test_signatures():
    from acoss_amd import _lib
    from acoss_amd.algorithms.algorithm_template import CoverAlgorithm
    sig = inspect.signature(CoverAlgorithm.evaluate)
    assert list(sig.parameters)[:5] == ["self", "queries", "similarity_types", "topsidx", "report"]
    assert sig.parameters["queries"].default is None and sig.parameters["similarity_types"].default is None
    assert sig.parameters["topsidx"].default == [1, 10, 100, 1000] and sig.parameters["report"].default is False
    sig = inspect.signature(_lib.Context.query_ranks)
    assert list(sig.parameters) == ["self", "algo", "symmetric", "params", "queries", "moff", "mates", "posn", "col", "col_mode"]
    assert sig.parameters["posn"].default is None and sig.parameters["col"].default is None and sig.parameters["col_mode"].default == 0


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


def test_evaluate_without_grid_raises(tmp_path, monkeypatch):
    from acoss_amd.algorithms.algorithm_template import CoverAlgorithm
    monkeypatch.chdir(tmp_path)

    class Toy(CoverAlgorithm):
        def similarity(self, idxs):
            self.Ds["main"][idxs[:, 0], idxs[:, 1]] = 1.0

    toy = Toy(_csv(tmp_path, 6), name="Toy", datapath="feat/", shortname="t")
    with pytest.raises(NotImplementedError, match="_grid"):
        toy.evaluate()
    with pytest.raises(NotImplementedError, match="_grid"):
        toy.evaluate(queries=[0, 1])
    toy.cleanup_memmap()


@pytest.mark.parametrize("cls_name", ["Serra09", "ChenFusion", "Simple", "EarlyFusion", "FTM2D"])
def test_python_side_argument_errors_come_first(tmp_path, monkeypatch, cls_name):
    from acoss_amd import algorithms
    monkeypatch.chdir(tmp_path)
    cls = getattr(algorithms, cls_name)
    algo = cls(_csv(tmp_path, 8), "feat/", shortname="args")
    for i in range(8):
        algo._register_label(i, "w%d" % (i // 2))
    algo._ctx = _NoDevice()                                   # nothing below may get as far as a context
    monkeypatch.setattr(cls, "_context", lambda self: (_ for _ in ()).throw(AssertionError("pool upload before the argument checks")))
    first = algo._identify_planes[0]
    with pytest.raises(ValueError, match="unknown similarity type"):
        algo.evaluate(similarity_types=["nope"])
    with pytest.raises(ValueError, match="unknown similarity type"):
        algo.evaluate(queries=[0], similarity_types=[first, "nope"])
    for fused in algo._identify_fused:
        with pytest.raises(NotImplementedError, match="whole N x N"):
            algo.evaluate(similarity_types=[fused])
    with pytest.raises(ValueError, match="distinct"):
        algo.evaluate(queries=[3, 1, 3])
    with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 8\)"):
        algo.evaluate(queries=[0, 8])
    with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 8\)"):
        algo.evaluate(queries=[-1])
    with pytest.raises(ValueError, match="integer"):
        algo.evaluate(queries=[0.5])
    # a track without a label: the cliques must hold every track, as for getEvalStatistics(engine="device")
    algo.cliques["w3"].discard(7)
    with pytest.raises(ValueError, match="every track"):
        algo.evaluate()
    assert not any(np.any(np.asarray(algo.Ds[t])) for t in algo.Ds)
    algo._ctx = None
    algo.cleanup_memmap()


@pytest.mark.parametrize("seed", range(4))
def test_evaluate_plan_full_equals_rank_plan(seed):
    """queries=None: the rows with mates in clique order, and per row exactly the mates rank_plan lists, in its order."""
    from acoss_amd.algorithms.algorithm_template import evaluate_plan, rank_plan
    cliques, n = _rank_ref.datacos_cliques(5 + seed, 2 + seed % 3, 4, seed)
    full, plan = rank_plan(cliques, n), evaluate_plan(cliques, n)
    assert np.array_equal(plan["idx"], full["idx"]) and np.array_equal(plan["posn"], full["posn"]) and plan["n_eval"] == full["n_eval"]
    assert np.array_equal(plan["ev"], np.arange(full["n_eval"])) and plan["n_mrr"] == n
    assert np.array_equal(plan["rows"], full["idx"][:full["n_eval"]])
    assert plan["rows"].dtype == np.int32 and plan["mates"].dtype == np.int32 and plan["moff"].dtype == np.int64
    of_full = {int(t): full["mates"][full["moff"][i]:full["moff"][i + 1]].tolist() for i, t in enumerate(full["rows"])}
    for i, t in enumerate(plan["rows"]):
        mine = plan["mates"][plan["moff"][i]:plan["moff"][i + 1]].tolist()
        assert mine == of_full[int(t)] and int(t) not in mine
        p = int(plan["posn"][t])
        assert plan["where"][p].tolist() == [plan["moff"][i], len(mine)]


def test_evaluate_plan_subset():
    from acoss_amd.algorithms.algorithm_template import evaluate_plan
    cliques = [[5], [0, 3], [1, 2, 6], [4]]                       # layout: 1 2 6 0 3 5 4
    plan = evaluate_plan(cliques, 7, [4, 3, 6, 5, 1])
    assert plan["idx"].tolist() == [1, 2, 6, 0, 3, 5, 4] and plan["n_eval"] == 5 and plan["n_mrr"] == 5
    assert plan["ev"].tolist() == [0, 2, 4] and plan["rows"].tolist() == [1, 6, 3]         # clique order; singletons 4, 5 left out
    assert plan["moff"].tolist() == [0, 2, 4, 5] and plan["mates"].tolist() == [2, 6, 1, 2, 0]
    assert plan["where"].tolist() == [[0, 2], [0, 0], [2, 2], [0, 0], [4, 1]]
    none = evaluate_plan(cliques, 7, [5, 4])
    assert len(none["rows"]) == 0 and none["moff"].tolist() == [0] and len(none["mates"]) == 0 and none["n_mrr"] == 2
    with pytest.raises(ValueError, match="distinct"):
        evaluate_plan(cliques, 7, [1, 1])
    with pytest.raises(ValueError, match="every track"):
        evaluate_plan([[0, 1], [3]], 4, [0])


@pytest.mark.parametrize("seed", range(4))
def test_statistics_tail_on_a_subset(seed):
    """The host tail on exact positions (tests/_rank_ref.py standing in for the device) gives the yardstick's tuple for a
    shuffled subset with singletons; flagged rows come through the callable, never through a matrix."""
    from acoss_amd.algorithms.algorithm_template import _statistics_from_positions, evaluate_plan
    rng = np.random.default_rng(40 + seed)
    cliques, n = _rank_ref.datacos_cliques(6, 2 + seed % 3, 5, seed)
    D = _tied_matrix(rng, n, levels=4)
    if seed >= 2:                                 # a -inf in a non-mate cell of some rows
        single = [c[0] for c in cliques if len(c) == 1][0]
        D[rng.choice(n, size=5, replace=False), single] = -np.inf
    for queries in (None, rng.permutation(n)[:n // 2]):
        plan = evaluate_plan(cliques, n, queries)
        pos, flag = _rank_ref.rank_columns(D, plan["rows"], plan["moff"], plan["mates"], posn=plan["posn"])
        asked = []

        def rows_of(tracks):
            asked.append(len(tracks))
            return D[tracks]
        info = {}
        got = _statistics_from_positions(None, plan, pos, flag, (1, 5, 10), 4, info, rows_of=rows_of)
        want = _evalq_ref.statistics(D, cliques, queries, (1, 5, 10))
        assert np.array_equal(got[4], want[4]) and got[2] == want[2] and got[0] == want[0]
        assert got[1] == pytest.approx(want[1], rel=1e-12) and got[3] == pytest.approx(want[3], rel=1e-12)
        assert info["host_rows"] == _evalq_ref.flagged_rows(D, cliques, queries) == int(flag.sum()) == sum(asked)
        assert info["device_rows"] + info["host_rows"] == len(plan["rows"])
        assert all(k <= 4 for k in asked)


def test_getevalstatistics_report_bytes(tmp_path, monkeypatch):
    """The report tail is shared with evaluate(report=True): the CSV bytes of getEvalStatistics are the reference's."""
    from acoss_amd.algorithms.algorithm_template import CoverAlgorithm
    monkeypatch.chdir(tmp_path)
    a = CoverAlgorithm(_csv(tmp_path, 4), name="Base", datapath="feat/", shortname="rep")
    for i in range(4):
        a._register_label(i, "w%d" % (i // 2))
    a.Ds["main"][:] = np.array([[0, 3, 1, 2], [3, 0, 2, 1], [1, 0.25, 0, 0.5], [0.25, 1, 0.5, 0]], np.float32)
    out = a.getEvalStatistics("main", topsidx=[1, 10])
    assert out[0] == 1.5 and out[4].tolist() == [2, 4]
    a._report_statistics("again", [1, 10], *out)
    text = open("results_rep_Base.csv").read()
    assert text == ("name, MR, MRR, MDR, MAP,Top-1,Top-10\n"
                    "Base_main,1.5, 0.75, 1.5, 0.75, 2, 4\n"
                    "Base_again,1.5, 0.75, 1.5, 0.75, 2, 4\n")
    a.cleanup_memmap()
