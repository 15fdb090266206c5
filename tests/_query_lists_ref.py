"""
numpy restatement of the list contract of libacx (acx_query_topk_lists, include/acx.h) for the tests: row i of the result
is what acx_query_topk returns for the single query queries[i] and the candidates "the valid entries of lists[i],
sorted" -- stated through tests/_query_ref.topk, sharing nothing with the code under test.  The input is always a set of
RAW score rows: row i = the scores of track queries[i] against every track, from whatever existing path produced them.
"""
import numpy as np

from . import _query_ref


def topk_lists(rows, queries, lists, k, col=None, col_mode=0):
    """acx_query_topk_lists: (idx (Q, k) int32, score (Q, k) float32).  lists: (Q, L) integers, -1 = an empty slot."""
    rows = np.asarray(rows, dtype=np.float32)
    lists = np.asarray(lists, dtype=np.int64).reshape(len(queries), -1)
    idx = np.full((len(queries), k), -1, np.int32)
    sc = np.full((len(queries), k), np.nan, np.float32)
    for i, q in enumerate(queries):
        cand = np.sort(lists[i][lists[i] >= 0])
        assert len(np.unique(cand)) == len(cand), "a track twice in one row is outside the contract"
        idx[i], sc[i] = (a[0] for a in _query_ref.topk(rows[i:i + 1], [q], k, candidates=cand, col=col, col_mode=col_mode))
    return idx, sc
