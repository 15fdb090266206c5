"""
numpy restatement of CoverAlgorithm.evaluate for the tests: written from the definition, row by row, sharing nothing
with the code under test.  The input is a FINISHED (N, N) score matrix (row t = the scores of track t against every
track, from whatever existing path produced it), the cliques and a query list.
"""
import numpy as np


def clique_layout(cliques):
    """The tracks in the clique-contiguous order of the evaluation: cliques largest first, equal sizes in the order
    given (a stable sort), members in the order given."""
    order = sorted(range(len(cliques)), key=lambda i: -len(cliques[i]))          # sorted() is stable
    return [int(t) for i in order for t in cliques[i]]


def mate_positions(D, cliques, queries=None):
    """[(query, sorted 1-based positions of its clique mates)] for every query that has a mate, in the order of the
    clique layout.  A row is laid out in clique order with the query's own cell removed and ranked by
    np.argsort(-row, kind="stable"): larger first, ties keep the layout's order, NaN after every number."""
    D = np.asarray(D, dtype=np.float32)
    n = D.shape[0]
    layout = clique_layout(cliques)
    assert sorted(layout) == list(range(n)), "every track in exactly one clique"
    mates_of = {}
    for c in cliques:
        for t in c:
            mates_of[int(t)] = [int(u) for u in c if int(u) != int(t)]
    wanted = set(range(n)) if queries is None else set(int(q) for q in queries)
    out = []
    for t in layout:
        if t not in wanted or not mates_of[t]:
            continue
        cols = [c for c in layout if c != t]
        with np.errstate(invalid="ignore"):
            order = np.argsort(-D[t, cols], kind="stable")
        ranked = [cols[j] for j in order]
        out.append((t, sorted(ranked.index(m) + 1 for m in mates_of[t])))
    return out


def flagged_rows(D, cliques, queries=None):
    """How many of the evaluated queries hold a NaN or a -inf outside their own cell."""
    D = np.asarray(D, dtype=np.float32)
    n = D.shape[0]
    k = 0
    for t, _ in mate_positions(D, cliques, queries):
        other = np.arange(n) != t
        k += int(np.isnan(D[t, other]).any() or (D[t, other] == -np.inf).any())
    return k


def statistics(D, cliques, queries=None, topsidx=(1, 10, 100, 1000)):
    """(MR, MRR, MDR, MAP, tops): over the queries that have a clique mate, rank = the position of the first mate,
    AP = mean over the mates (by ascending position) of j / position_j; MR / MDR / MAP the mean / median / mean over
    those queries, Top-t the number of them with rank <= t; MRR = sum(1 / rank) / the number of queries given (every
    track for None), singletons included."""
    n = np.asarray(D).shape[0]
    mp = mate_positions(D, cliques, queries)
    n_given = n if queries is None else len(list(queries))
    ranks = np.array([p[0] for _, p in mp], dtype=np.float64)
    aps = np.array([np.mean([(j + 1) / p for j, p in enumerate(ps)]) for _, ps in mp], dtype=np.float64)
    if len(mp) == 0:
        return float("nan"), 0.0, float("nan"), float("nan"), np.zeros(len(topsidx))
    MR = float(np.mean(ranks))
    MRR = float(np.sum(1.0 / ranks) / n_given)
    MDR = float(np.median(ranks))
    MAP = float(np.mean(aps))
    tops = np.array([np.sum(ranks <= t) for t in topsidx], dtype=np.float64)
    return MR, MRR, MDR, MAP, tops
