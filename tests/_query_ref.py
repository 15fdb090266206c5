"""
numpy restatement of the query contract of libacx (acx_query_scores / acx_query_topk, include/acx.h) for the tests:
written from the definition, sharing nothing with the code under test.  The input is always a set of RAW score rows --
row i = the scores of track queries[i] against every track, from whatever existing path produced them.
"""
import numpy as np


def finish(rows, col=None, col_mode=0):
    """The col_mode of acx_query_spec on raw (Q, N) float32 rows: 0 the score s, 1 s / col[c], 2 -(col[c] / s); one f64
    division, one rounding to float32 (what normalize_by_length of Serra09 / ChenFusion does to a matrix)."""
    rows = np.asarray(rows, dtype=np.float32)
    if col_mode == 0:
        return rows.copy()
    col = np.asarray(col, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if col_mode == 1:
            return (rows.astype(np.float64) / col[None, :]).astype(np.float32)
        if col_mode == 2:
            return -((col[None, :] / rows.astype(np.float64)).astype(np.float32))
    raise ValueError("col_mode must be 0, 1 or 2")


def scores(rows, queries, col=None, col_mode=0):
    """acx_query_scores: the finished rows, a query's own cell 0."""
    out = finish(rows, col, col_mode)
    out[np.arange(len(queries)), np.asarray(queries)] = 0.0
    return out


def topk(rows, queries, k, candidates=None, col=None, col_mode=0):
    """acx_query_topk: (idx (Q, k) int32, score (Q, k) float32).  Per row: finish, drop the query's own column and every
    non-candidate, stable descending sort of what is left (ties keep ascending track order, -0.0 == +0.0, NaN last:
    np.argsort(-v, kind="stable")), first k; tail -1 / NaN."""
    fin = finish(rows, col, col_mode)
    n = fin.shape[1]
    cand = np.arange(n) if candidates is None else np.asarray(candidates, dtype=np.int64)
    idx = np.full((len(queries), k), -1, np.int32)
    sc = np.full((len(queries), k), np.nan, np.float32)
    for i, q in enumerate(queries):
        cols = cand[cand != q]
        v = fin[i, cols]
        best = cols[np.argsort(-v, kind="stable")[:k]]
        idx[i, :len(best)] = best
        sc[i, :len(best)] = fin[i, best]
    return idx, sc
