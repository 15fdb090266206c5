"""
numpy restatements of libacx's row ranking (acx_rank_columns / acx_topk_rows, include/acx.h) for the tests: written
from the definition, loop by loop, sharing nothing with the code under test.
"""
import numpy as np


def rank_columns(D, rows, moff, mates, posn=None):
    """(pos int32, flag uint8): for rows[i] = track t, the 1-based position of every column m of
    mates[moff[i]:moff[i + 1]] in the order "higher score first, ties by posn", the cell D[t, t] taking no part; a row
    with NaN or -inf in another cell is flagged and its positions are -1."""
    D = np.asarray(D)
    n = D.shape[1]
    posn = np.arange(n) if posn is None else np.asarray(posn)
    pos = np.full(len(mates), -1, np.int32)
    flag = np.zeros(len(rows), np.uint8)
    with np.errstate(invalid="ignore"):
        for i, t in enumerate(rows):
            s = np.asarray(D[t], dtype=np.float32)
            other = np.arange(n) != t
            if np.isnan(s[other]).any() or (s[other] == -np.inf).any():
                flag[i] = 1
                continue
            for j in range(int(moff[i]), int(moff[i + 1])):
                m = int(mates[j])
                pos[j] = 1 + np.count_nonzero(other & (s > s[m])) + np.count_nonzero(other & (s == s[m]) & (posn < posn[m]))
    return pos, flag


def topk_rows(D, k, rows=None, posn=None):
    """(idx (R, k) int32, score (R, k) float32): np.argsort(-row_without_self, kind="stable")[:k] mapped back to column
    indices (the columns laid out by posn first, so that "stable" means "ties by posn"); tail: -1 / NaN."""
    D = np.asarray(D)
    n = D.shape[1]
    rows = np.arange(D.shape[0]) if rows is None else np.asarray(rows)
    idx = np.full((len(rows), k), -1, np.int32)
    score = np.full((len(rows), k), np.nan, np.float32)
    for i, t in enumerate(rows):
        s = np.asarray(D[t], dtype=np.float32)
        cols = np.arange(n) if posn is None else np.argsort(np.asarray(posn), kind="stable")
        cols = cols[cols != t]
        best = cols[np.argsort(-s[cols], kind="stable")[:k]]
        idx[i, :len(best)] = best
        score[i, :len(best)] = s[best]
    return idx, score


def cliques_of(labels):
    """Cliques as CoverAlgorithm holds them: label -> sorted members, labels in order of first appearance."""
    cl = {}
    for i, l in enumerate(labels):
        cl.setdefault(str(l), []).append(i)
    return [sorted(v) for v in cl.values()]


def datacos_cliques(n_cliques, size, n_single, seed):
    """A shuffled collection of `n_cliques` cliques of `size` tracks plus `n_single` singletons."""
    rng = np.random.default_rng(seed)
    n = n_cliques * size + n_single
    perm = rng.permutation(n)
    cl = [sorted(perm[c * size:(c + 1) * size].tolist()) for c in range(n_cliques)]
    cl += [[int(t)] for t in perm[n_cliques * size:]]
    order = rng.permutation(len(cl))
    return [cl[i] for i in order], n
