"""
The yardstick of the Qmax SECTIONS (acx_serra09_align_sections / acx_qmax_sections_binary): two independent
restatements, in f32, of the contract

  section 0      the alignment of tests/_qmax_locate_ref.py / _qmax_path_ref.py, reported iff its score >= min_score
  free rows      the rows of R start as one free interval [0, M - 1]; a section with start row q0 and end row q1 in the free interval
                 [a, b] EXCLUDES rows [max(a, q0 - pad), min(b, q1 + pad)]; [a, b] is replaced by what is left above and below
  section k + 1  the same alignment of Q', the recursion with Q' = 0 on every DP cell whose row of R is excluded; reported iff its
                 score >= max(min_score, min_ratio * score_0) (one f32 multiply, equality counts); the search ends at the first
                 section that fails, or after max_sections

  sections_full        (a) the full masked matrix, a row at a time, and an explicit traceback from its row-major first maximum,
                           every round from scratch
  sections_intervals   (b) per free interval a forward sweep over its rows alone from two zero rows, two rolling rows with the start
                           of the path through every cell, one best record per interval; a round sweeps only the two intervals the
                           last section split, and the next section is the best record by (value, then smaller end cell)

(a) returns (records, paths): records a list of (score, q0, r0, q1, r1), paths the (L, 2) int32 cells of each from start to end.
(b) returns the records.  Coordinates are rows / columns of R, as in the two yardsticks above.
"""
import numpy as np

F = np.float32


def _plot(R):
    R = np.ascontiguousarray(R, dtype=np.uint8)
    assert R.ndim == 2 and R.max(initial=0) <= 1
    return R


def check_opts(max_sections, min_score, min_ratio, pad):
    assert 1 <= max_sections <= 16 and pad >= 0 and F(min_score) > 1 and 0 <= F(min_ratio) <= 1


def threshold(k, score0, min_score, min_ratio):
    return F(min_score) if k == 0 else max(F(min_score), F(F(min_ratio) * F(score0)))


def masked_matrix(R, excluded, gamma_o, gamma_e, dp_start):
    """Q' in DP coordinates, (M, N) f32: Q with 0 on every DP row whose row of R is excluded."""
    M, N = R.shape
    st, o = int(dp_start), (1 if dp_start == 3 else 0)
    Q = np.zeros((M, N), F)
    if M <= st or N <= st:
        return Q
    go, ge = F(gamma_o), F(gamma_e)
    js = np.arange(st, N)
    rj = js - o
    for i in range(st, M):
        ri = i - o
        if excluded[ri]:
            continue
        c2, c3, c4 = Q[i - 1, js - 1], Q[i - 2, js - 1], Q[i - 1, js - 2]
        mx = np.maximum(np.maximum(c2, c3), c4)
        a2 = (c2 - np.where(R[ri - 1, rj - 1] != 0, go, ge)).astype(F)
        a3 = (c3 - np.where(R[ri - 2, rj - 1] != 0, go, ge)).astype(F)
        a4 = (c4 - np.where(R[ri - 1, rj - 2] != 0, go, ge)).astype(F)
        ax = np.maximum(np.maximum(np.maximum(a2, a3), a4), F(0))
        Q[i, st:] = np.where(R[ri, rj] != 0, (mx + F(1)).astype(F), ax)
    return Q


def _traceback(R, Q, gamma_o, gamma_e, dp_start):
    """From the row-major first maximum of Q along the predecessors: (record, cells), or None when Q is 0 everywhere."""
    o = 1 if dp_start == 3 else 0
    go, ge = F(gamma_o), F(gamma_e)
    best = Q.max(initial=F(0))
    if not best > 0:
        return None
    i, j = (int(v) for v in np.unravel_index(int(np.argmax(Q)), Q.shape))
    cells = []
    while True:
        assert Q[i, j] > 0
        cells.append((i - o, j - o))
        pred = ((i - 1, j - 1), (i - 2, j - 1), (i - 1, j - 2))
        if R[i - o, j - o]:
            vals = [Q[c] for c in pred]
        else:
            vals = [F(Q[c] - (go if R[c[0] - o, c[1] - o] else ge)) for c in pred]
        pick = 0
        for k in (1, 2):
            if vals[k] > vals[pick]:
                pick = k
        if R[i - o, j - o] and vals[pick] == 0:
            break
        assert vals[pick] > 0
        i, j = pred[pick]
    cells.reverse()
    rec = (float(best), cells[0][0], cells[0][1], cells[-1][0], cells[-1][1])
    return rec, np.array(cells, np.int32).reshape(-1, 2)


def sections_full(R, gamma_o=0.5, gamma_e=0.5, dp_start=2, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0):
    """(a)."""
    R = _plot(R)
    check_opts(max_sections, min_score, min_ratio, pad)
    M = R.shape[0]
    excluded = np.zeros(M, bool)
    free = [(0, M - 1)]
    recs, paths = [], []
    for k in range(max_sections):
        got = _traceback(R, masked_matrix(R, excluded, gamma_o, gamma_e, dp_start), gamma_o, gamma_e, dp_start)
        if got is None:
            break
        rec, cells = got
        if not F(rec[0]) >= threshold(k, recs[0][0] if recs else 0.0, min_score, min_ratio):
            break
        recs.append(rec)
        paths.append(cells)
        q0, q1 = rec[1], rec[3]
        (a, b), = [iv for iv in free if iv[0] <= q0 and q1 <= iv[1]]          # a section lies in ONE free interval
        x0, x1 = max(a, q0 - pad), min(b, q1 + pad)
        excluded[x0:x1 + 1] = True
        free.remove((a, b))
        free += [(a, x0 - 1), (x1 + 1, b)]
    return recs, paths


def sweep_interval(R, a, b, gamma_o, gamma_e, dp_start):
    """The best record of the free interval [a, b] of R's rows: (value, end, start) with cells as (row of R) * N + (column of R);
    (0, -1, -1) when the interval holds fewer than 2 rows of the DP or nothing matches."""
    M, N = R.shape
    st, o = int(dp_start), (1 if dp_start == 3 else 0)
    lo, hi = max(a, 2), min(b, M - 1 - o)
    if hi - lo < 1 or N <= st:
        return (F(0), -1, -1)
    go, ge = F(gamma_o), F(gamma_e)
    gam = lambda bits: np.where(bits != 0, go, ge).astype(F)
    js = np.arange(st, N)
    rj = js - o
    q1, q2 = np.zeros(N, F), np.zeros(N, F)
    s1, s2 = np.full(N, -1, np.int64), np.full(N, -1, np.int64)
    best, end, start = F(0), -1, -1
    for ri in range(lo, hi + 1):
        c = (q1[js - 1], q2[js - 1], q1[js - 2])
        s = (s1[js - 1], s2[js - 1], s1[js - 2])
        match = R[ri, rj] != 0
        mx, sm = c[0], s[0]
        for k in (1, 2):
            up = c[k] > mx
            mx, sm = np.where(up, c[k], mx), np.where(up, s[k], sm)
        sm = np.where(mx == 0, ri * N + rj, sm)
        a_ = ((c[0] - gam(R[ri - 1, rj - 1])).astype(F), (c[1] - gam(R[ri - 2, rj - 1])).astype(F), (c[2] - gam(R[ri - 1, rj - 2])).astype(F))
        ax, sa = np.zeros(len(js), F), np.full(len(js), -1, np.int64)
        for k in (0, 1, 2):
            up = a_[k] > ax
            ax, sa = np.where(up, a_[k], ax), np.where(up, s[k], sa)
        q = np.zeros(N, F)
        sn = np.full(N, -1, np.int64)
        q[st:] = np.where(match, (mx + F(1)).astype(F), ax)
        sn[st:] = np.where(match, sm, sa)
        jm = int(np.argmax(q))
        if q[jm] > best:
            best, end, start = q[jm], ri * N + (jm - o), int(sn[jm])
        q2, s2 = q1, s1
        q1, s1 = q, sn
    return (best, end, start)


def sections_intervals(R, gamma_o=0.5, gamma_e=0.5, dp_start=2, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0, swept=None, ties=None):
    """(b).  swept: a list that receives the (a, b) of every interval swept, in order.  ties: a list that receives, per round that
    has a candidate, (the slots of the interval records that share the largest value, the slot picked)."""
    R = _plot(R)
    check_opts(max_sections, min_score, min_ratio, pad)
    M, N = R.shape
    ivs = [(0, M - 1)]
    pending = [0]
    best = {}
    recs = []
    while True:
        for t in pending:
            best[t] = sweep_interval(R, ivs[t][0], ivs[t][1], gamma_o, gamma_e, dp_start)
            if swept is not None:
                swept.append(ivs[t])
        pick = -1
        for t in range(len(ivs)):
            v, e, _ = best[t]
            if v > 0 and (pick < 0 or v > best[pick][0] or (v == best[pick][0] and e < best[pick][1])):
                pick = t
        if pick < 0:
            break
        v, e, s = best[pick]
        if ties is not None:
            ties.append(([t for t in range(len(ivs)) if best[t][0] == v], pick))
        if not v >= threshold(len(recs), recs[0][0] if recs else 0.0, min_score, min_ratio):
            break
        recs.append((float(v), s // N, s % N, e // N, e % N))
        if len(recs) == max_sections:
            break
        a, b = ivs[pick]
        q0, q1 = s // N, e // N
        ivs[pick] = (a, max(a, q0 - pad) - 1)
        ivs.append((min(b, q1 + pad) + 1, b))
        pending = [pick, len(ivs) - 1]
    return recs


def ones(shape, diagonals):
    """A plot with diagonals of ones: (row, column, cells) each, R[row + k][column + k] = 1."""
    R = np.zeros(shape, np.uint8)
    for r, c, n in diagonals:
        for k in range(n):
            R[r + k, c + k] = 1
    return R


# Hand-checked plots: (name, R, options, records)
BRIDGE = ones((120, 260), [(10, 10, 30), (40, 200, 40), (80, 80, 16)])
THREE = ones((60, 120), [(4, 4, 12), (20, 50, 9), (40, 90, 6)])
CUT = ones((40, 90), [(10, 10, 12), (16, 60, 15)])
# (every diagonal lies LEFT of the ones above it: the values that decay behind a diagonal's end spread down and to the right only)
TIE2 = ones((60, 60), [(20, 20, 10), (2, 40, 6), (40, 2, 6)])
TIE3 = ones((80, 80), [(10, 60, 10), (30, 45, 6), (50, 20, 12), (66, 2, 6)])
HAND = [
    # three diagonals; with rows 40..79 of R cleared instead of Q forced to 0 the second answer would bridge them: (32.5; 10,10 -> 95,95)
    ("no bridge over an excluded stretch", BRIDGE, dict(max_sections=4),
     [(40.0, 40, 200, 79, 239), (30.0, 10, 10, 39, 39), (16.0, 80, 80, 95, 95)]),
    ("three diagonals", THREE, dict(max_sections=4), [(12.0, 4, 4, 15, 15), (9.0, 20, 50, 28, 58), (6.0, 40, 90, 45, 95)]),
    ("min_score 7", THREE, dict(max_sections=4, min_score=7.0), [(12.0, 4, 4, 15, 15), (9.0, 20, 50, 28, 58)]),
    ("min_ratio 0.75: threshold 9.0, equality reported", THREE, dict(max_sections=4, min_ratio=0.75), [(12.0, 4, 4, 15, 15), (9.0, 20, 50, 28, 58)]),
    ("min_ratio 0.8", THREE, dict(max_sections=4, min_ratio=0.8), [(12.0, 4, 4, 15, 15)]),
    ("max_sections 2", THREE, dict(max_sections=2), [(12.0, 4, 4, 15, 15), (9.0, 20, 50, 28, 58)]),
    # the 15-cell diagonal takes rows 16..30; the 12-cell one from (10, 10) keeps rows 10..15
    ("the second section cut by the first's rows", CUT, dict(max_sections=4), [(15.0, 16, 60, 30, 74), (6.0, 10, 10, 15, 15)]),
    # three diagonals of 8 in ONE interval: the row-major first maximum of a sweep, three times
    ("a tie inside one interval: the smaller row wins", ones((50, 50), [(30, 5, 8), (6, 30, 8), (18, 18, 8)]), dict(max_sections=3),
     [(8.0, 6, 30, 13, 37), (8.0, 18, 18, 25, 25), (8.0, 30, 5, 37, 12)]),
    # section 0 (10 cells, rows 20..29) splits the rows into [0, 19] and [30, 59]; each holds a diagonal of 6: the two intervals'
    # records tie, and the one with the smaller end cell -- rows 2..7 -- is section 1
    ("a tie between two intervals: the smaller row wins", TIE2, dict(max_sections=4),
     [(10.0, 20, 20, 29, 29), (6.0, 2, 40, 7, 45), (6.0, 40, 2, 45, 7)]),
    # section 0 (12 cells, rows 50..61) leaves [0, 49] in slot 0 and [62, 79] in slot 1; section 1 (10 cells, rows 10..19) splits slot 0
    # into [0, 9] and [20, 49], the latter in slot 2.  The diagonals of 6 in rows 30..35 (slot 2) and 66..71 (slot 1) tie: the smaller
    # row wins although its interval holds the HIGHER slot -- the slots are not in row order after two splits
    ("a tie after two splits: the smaller row in the higher slot wins", TIE3, dict(max_sections=4),
     [(12.0, 50, 20, 61, 31), (10.0, 10, 60, 19, 69), (6.0, 30, 45, 35, 50), (6.0, 66, 2, 71, 7)]),
    # pad 3 at row 0: section 0 has rows 2..9, rows 0..12 are excluded; of the diagonal from (11, 20) rows 13..16 are left (4 cells),
    # the one from (13, 30) keeps its 5
    ("pad clipped at row 0", ones((40, 40), [(2, 2, 8), (11, 20, 6), (13, 30, 5)]), dict(max_sections=3, pad=3),
     [(8.0, 2, 2, 9, 9), (5.0, 13, 30, 17, 34)]),
    ("pad clipped at the last row", ones((40, 40), [(30, 30, 10), (20, 5, 9)]), dict(max_sections=3, pad=3),
     [(10.0, 30, 30, 39, 39), (7.0, 20, 5, 26, 11)]),
    # section 0 has rows 20..29, pad 2: rows 18..31 are excluded.  The two diagonals of 8 tie, the one in rows 2..9 is section 1 and
    # excludes rows 0..11; of the other, rows 12..17 are left: section 2 lies in the free interval [12, 17] and its pad stops at 12 and
    # at 17 -- not across section 1 or section 0
    ("pad clipped at an earlier section", ones((50, 60), [(20, 20, 10), (10, 40, 8), (2, 20, 8), (34, 2, 4)]), dict(max_sections=4, pad=2),
     [(10.0, 20, 20, 29, 29), (8.0, 2, 20, 9, 27), (6.0, 12, 42, 17, 47), (4.0, 34, 2, 37, 5)]),
]
