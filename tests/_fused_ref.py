"""
The definition of acx_query_fused_lists (include/acx.h) restated in numpy: for every query its neighbourhood T, the pair
scores of T's upper triangle -> mirrored distance matrices -> a fusion -> the query's row -> f32 -> a stable order -> collection
indices.  Where the scores, the fusion and the ranking come from is the caller's choice: the CPU tests hand in the oracle
(oracle pair scores, oracle.snf_fuse, the argsort below), the GPU tests the library's existing exports (acx_*_pairs,
acx_snf_fuse_dists, acx_topk_rows) -- the composition that the batched export must reproduce bit for bit.
"""
import numpy as np

SQRTLEN, INV1P = 1, 2            # acx.h ACX_FUSED_*


def neighbourhood(q, row):
    """T = sorted({q} U valid(row)) as int64, and the position of q in it."""
    row = np.asarray(row).reshape(-1)
    T = np.unique(np.concatenate([[int(q)], row[row >= 0]])).astype(np.int64)
    return T, int(np.searchsorted(T, int(q)))


def triangle_pairs(T):
    """The unordered pairs of T as (min, max) track pairs, upper triangle row by row: (n (n - 1) / 2, 2) int32."""
    a, b = np.triu_indices(len(T), 1)
    return np.stack([T[a], T[b]], axis=1).astype(np.int32)


def distances(scores, T, planes, transform, col=None):
    """scores: (pairs, W) f32 for triangle_pairs(T).  -> one n x n f64 distance matrix per plane of `planes`, in that order:
    mirrored raw scores, then SQRTLEN: (float)(col[c] / (double)s) per column c, widened (ChenFusion.normalize_by_length as
    do_late_fusion reads it); INV1P: 1 / (1 + (double)s) (EarlyFusion.do_late_fusion).  The diagonal is 0 (the fusion zeroes it)."""
    n = len(T)
    a, b = np.triu_indices(n, 1)
    out = []
    for e in planes:
        S = np.zeros((n, n), np.float32)
        S[a, b] = scores[:, e]
        S[b, a] = scores[:, e]
        with np.errstate(divide="ignore", invalid="ignore"):
            if transform == SQRTLEN:
                D = (np.asarray(col, np.float64)[T][None, :] / S.astype(np.float64)).astype(np.float32).astype(np.float64)
            else:
                D = 1.0 / (1.0 + S.astype(np.float64))
        np.fill_diagonal(D, 0.0)
        out.append(D)
    return out


def nonfinite_flag(Ds):
    off = ~np.eye(Ds[0].shape[0], dtype=bool)
    return int(any((~np.isfinite(D[off])).any() for D in Ds))


def stable_topk(row32, qpos, T, k):
    """The order of acx_topk_rows on one f32 row without its own column: larger first (-0.0 and +0.0 tie), ties by ascending
    index, NaN last, a tail of -1 / NaN.  -> (idx (k,) int32 collection indices, score (k,) f32)."""
    cols = np.array([c for c in range(len(T)) if c != qpos], np.int64)
    order = cols[np.argsort(-row32[cols], kind="stable")][:k]
    idx = np.full(k, -1, np.int32)
    sc = np.full(k, np.nan, np.float32)
    idx[:len(order)] = T[order]
    sc[:len(order)] = row32[order]
    return idx, sc


def rerank_fused(score_pairs, fuse, queries, lists, k, type_planes, transform, col=None, K=20, niters=20, rank=stable_topk):
    """score_pairs(pairs (P, 2) int32) -> (P, W) f32;  fuse(Ds, K, niters) -> the fused n x n f64 matrix;
    type_planes: one plane sequence per fused type.  -> (idx (Q, types, k) int32, score (Q, types, k) f32, flag (Q, types) uint8)."""
    Q, nt = len(queries), len(type_planes)
    idx = np.full((Q, nt, k), -1, np.int32)
    sc = np.full((Q, nt, k), np.nan, np.float32)
    flag = np.zeros((Q, nt), np.uint8)
    for i, q in enumerate(queries):
        T, qpos = neighbourhood(q, lists[i])
        assert len(T) >= K + 2, "a neighbourhood below K + 2 tracks is refused, not computed"
        scores = np.asarray(score_pairs(triangle_pairs(T)), np.float32).reshape(len(T) * (len(T) - 1) // 2, -1)
        for t, planes in enumerate(type_planes):
            Ds = distances(scores, T, planes, transform, col)
            flag[i, t] = nonfinite_flag(Ds)
            with np.errstate(all="ignore"):
                F = np.asarray(fuse(Ds, K, niters), np.float64)
                row32 = F[qpos].astype(np.float32)                # ONE rounding
            idx[i, t], sc[i, t] = rank(row32, qpos, T, k)
    return idx, sc, flag
