"""
The argument checks and the no-match rows that the alignment methods of Serra09 and EarlyFusion share (align / align_paths /
align_matches / align_match_paths): every check runs before the first library call.
"""
import numpy as np

NO_MATCH_FIELDS = ("q0", "r0", "q1", "r1", "q_span", "r_span")


def check_indices(who, idxs):
    a = np.asarray(idxs)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s: track indices must be integers, got dtype %s" % (who, a.dtype))
    return a


def check_pairs(who, a, n):
    """align() / align_paths(): checked indices -> (K, 2) int32 pairs over a collection of n tracks."""
    if a.size == 0:
        a = a.reshape(0, 2)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError("%s: idxs must be (K, 2) (query, reference) track indices, got shape %s" % (who, a.shape))
    if a.size and (a.min() < 0 or a.max() >= n):
        raise ValueError("%s: idxs must be track indices in [0, %d)" % (who, n))
    return np.ascontiguousarray(a, dtype=np.int32)


def check_matches(who, q, idx, n):
    """align_matches() / align_match_paths(): checked queries and indices -> (the (Q, k) index array, rows and slots of its filled
    slots, their (P, 2) pairs)."""
    q = q.reshape(-1)
    if idx.ndim != 2 or idx.shape[0] != len(q):
        raise ValueError("%s: indices must be (Q, k) with one row per query (%d), got shape %s" % (who, len(q), idx.shape))
    if q.size and (q.min() < 0 or q.max() >= n):
        raise ValueError("%s: queries must be track indices in [0, %d)" % (who, n))
    if idx.size and (idx.min() < -1 or idx.max() >= n):
        raise ValueError("%s: indices must be track indices in [0, %d) or -1" % (who, n))
    rows, slots = np.nonzero(idx >= 0)
    pairs = np.stack([q[rows], idx[rows, slots]], axis=1).astype(np.int32).reshape(-1, 2)
    return idx, rows, slots, np.ascontiguousarray(pairs)


def no_match_rows(shape, dtype):
    out = np.zeros(shape, dtype)
    for f in NO_MATCH_FIELDS:
        out[f] = -1
    return out


def scatter_paths(idx, rows, slots, got):
    """The (Q, k) lists of paths of align_match_paths: `got` are the paths of the filled slots, an empty slot has an empty path."""
    paths = [[np.zeros((0, 2), np.int32) for _ in range(idx.shape[1])] for _ in range(idx.shape[0])]
    for r, s, p in zip(rows, slots, got):
        paths[r][s] = p
    return paths
