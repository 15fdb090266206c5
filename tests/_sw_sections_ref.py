"""
The yardstick of the EarlyFusion SECTIONS (acx_ef_align_sections / acx_sw_sections_binary): two independent
restatements, in integer tenths, of the contract

  section 0      the alignment of tests/_sw_align_ref.py, reported iff its score >= min_score
  free rows      the rows of B start as one free interval [0, M - 1]; a section with start row q0 and end row q1 in the free interval
                 [a, b] EXCLUDES rows [max(a, q0 - pad), min(b, q1 + pad)]; [a, b] is replaced by what is left above and below
  section k + 1  the same alignment of T', the recursion with T' = 0 -- and so U' = (B ? 0 : -7), what rows 0 and 1 hold -- on every
                 cell of an excluded row; reported iff its f32 score >= max(min_score, min_ratio * score_0) (one f32 multiply,
                 equality counts); the search ends at the first section that fails, or after max_sections

  sections_full        (a) the full masked matrix, a row at a time, with the table of chosen predecessors, and an explicit traceback
                           from its row-major first maximum; every round from scratch
  sections_intervals   (b) per free interval [a, b] _sw_align_ref.align_forward on the CROPPED plot B[lo - 2 .. hi + 1] (lo = max(a, 2),
                           hi = min(b, M - 2); rows shifted back by lo - 2), one best record per interval; a round evaluates only the
                           two intervals the last section split, and the next section is the best record by (value, then smaller
                           end cell in row-major order).  An interval with fewer than two counted rows is not swept.
  sections_cleared     NOT the contract: the plain alignment of the plot whose excluded rows are cleared, round by round -- what
                           test_cleared_rows_would_bridge_the_excluded_stretch shows to differ

All return (records, paths): records a list of (score, q0, r0, q1, r1), paths the (L, 2) int32 cells of each from start to end.
"""
import numpy as np

from tests import _sw_align_ref as R

F = np.float32


def _plot(B):
    B = np.ascontiguousarray(B, dtype=np.uint8)
    assert B.ndim == 2 and B.max(initial=0) <= 1
    return B


def check_opts(max_sections, min_score, min_ratio, pad):
    assert 1 <= max_sections <= 16 and pad >= 0 and F(min_score) > 1 and 0 <= F(min_ratio) <= 1


def threshold(k, score0, min_score, min_ratio):
    return F(min_score) if k == 0 else max(F(min_score), F(F(min_ratio) * F(score0)))


def score_of(tenths):
    return float(F(tenths) / F(10))


def masked_matrix(B, excluded):
    """T' (M, N) int64 and the chosen predecessor of every cell (1, 2, 3: (i-1, j-1), (i-2, j-1), (i-1, j-2))."""
    M, N = B.shape
    T = np.zeros((M, N), np.int64)
    D = np.zeros((M, N), np.int8)
    if M < 4 or N < 4:
        return T, D
    gap = np.where(B != 0, 0, -7).astype(np.int64)
    U = gap.copy()                                             # T = 0 wherever nothing is written below
    js = np.arange(2, N - 1)
    for i in range(2, M - 1):
        if excluded[i]:
            continue
        c = (U[i - 1, js - 1], U[i - 2, js - 1], U[i - 1, js - 2])
        mx, d = c[0], np.ones(len(js), np.int8)
        for k in (1, 2):
            up = c[k] > mx
            mx, d = np.where(up, c[k], mx), np.where(up, k + 1, d).astype(np.int8)
        t = np.maximum(0, np.where(B[i, js] != 0, 10, -10) + mx)
        T[i, js] = t
        D[i, js] = d
        U[i, js] = t + gap[i, js]
    return T, D


def _traceback(T, D):
    """From the row-major first maximum of T along the chosen predecessors: (record, cells), or None when T is 0 everywhere."""
    best = int(T.max(initial=0))
    if best == 0:
        return None
    y, x = (int(v) for v in np.unravel_index(int(np.argmax(T)), T.shape))
    end = (y, x)
    cells = [end]
    while True:
        d = int(D[y, x])
        py, px = y - (2 if d == 2 else 1), x - (2 if d == 3 else 1)
        if T[py, px] == 0:
            break
        y, x = py, px
        cells.append((y, x))
    cells.reverse()
    return (score_of(best), y, x, end[0], end[1]), np.array(cells, np.int32).reshape(-1, 2)


def _rounds(B, max_sections, min_score, min_ratio, pad, matrix):
    B = _plot(B)
    check_opts(max_sections, min_score, min_ratio, pad)
    M = B.shape[0]
    excluded = np.zeros(M, bool)
    free = [(0, M - 1)]
    recs, paths = [], []
    for k in range(max_sections):
        got = _traceback(*matrix(B, excluded))
        if got is None:
            break
        rec, cells = got
        if not F(rec[0]) >= threshold(k, recs[0][0] if recs else 0.0, min_score, min_ratio):
            break
        recs.append(rec)
        paths.append(cells)
        q0, q1 = rec[1], rec[3]
        inside = [iv for iv in free if iv[0] <= q0 and q1 <= iv[1]]
        if len(inside) != 1:                                   # (sections_cleared only: the answer bridges an excluded stretch)
            break
        a, b = inside[0]
        x0, x1 = max(a, q0 - pad), min(b, q1 + pad)
        excluded[x0:x1 + 1] = True
        free.remove((a, b))
        free += [(a, x0 - 1), (x1 + 1, b)]
    return recs, paths


def sections_full(B, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0):
    """(a)."""
    return _rounds(B, max_sections, min_score, min_ratio, pad, masked_matrix)


def sections_cleared(B, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0):
    """Not the contract: excluded rows cleared in the plot, the recursion left as it is."""
    def matrix(B, excluded):
        C = B.copy()
        C[excluded] = 0
        return masked_matrix(C, np.zeros(len(excluded), bool))
    return _rounds(B, max_sections, min_score, min_ratio, pad, matrix)


def sweep_interval(B, a, b):
    """The best record of the free interval [a, b]: (tenths, end cell as row * N + column, record, cells), or None when the interval
    holds fewer than two counted rows (not swept) or nothing matches."""
    M, N = B.shape
    lo, hi = max(a, 2), min(b, M - 2)
    if hi - lo < 1 or N < 4:
        return None
    rec, cells = R.align_forward(B[lo - 2:hi + 2])
    if rec == R.NO_MATCH:
        return None
    sh = lo - 2
    cells = cells + np.array([sh, 0], np.int32)
    rec = (rec[0], rec[1] + sh, rec[2], rec[3] + sh, rec[4])
    return (int(round(rec[0] * 10)), rec[3] * N + rec[4], rec, cells)


def sections_intervals(B, max_sections=4, min_score=2.0, min_ratio=0.0, pad=0, swept=None, ties=None):
    """(b).  swept: a list that receives the (a, b) of every interval evaluated by a sweep, in order.  ties: a list that receives,
    per round that has a candidate, (the slots of the interval records that share the largest value, the slot picked)."""
    B = _plot(B)
    check_opts(max_sections, min_score, min_ratio, pad)
    M, N = B.shape
    ivs = [(0, M - 1)]
    pending = [0]
    best = {}
    recs, paths = [], []
    while True:
        for t in pending:
            a, b = ivs[t]
            if min(b, M - 2) - max(a, 2) >= 1 and swept is not None:
                swept.append(ivs[t])
            best[t] = sweep_interval(B, a, b)
        pick = -1
        for t in range(len(ivs)):
            if best[t] is not None and (pick < 0 or best[t][0] > best[pick][0] or (best[t][0] == best[pick][0] and best[t][1] < best[pick][1])):
                pick = t
        if pick < 0:
            break
        v, _, rec, cells = best[pick]
        if ties is not None:
            ties.append(([t for t in range(len(ivs)) if best[t] is not None and best[t][0] == v], pick))
        if not F(rec[0]) >= threshold(len(recs), recs[0][0] if recs else 0.0, min_score, min_ratio):
            break
        recs.append(rec)
        paths.append(cells)
        if len(recs) == max_sections:
            break
        a, b = ivs[pick]
        q0, q1 = rec[1], rec[3]
        ivs[pick] = (a, max(a, q0 - pad) - 1)
        ivs.append((min(b, q1 + pad) + 1, b))
        pending = [pick, len(ivs) - 1]
    return recs, paths


def check_sections(recs, paths, shape):
    """What every answer obeys: each section is a path of _sw_align_ref's kind, scores do not increase, row ranges are disjoint."""
    for rec, cells in zip(recs, paths):
        R.check_path(tuple([F(rec[0])] + list(rec[1:])), cells, shape)
    for k in range(1, len(recs)):
        assert recs[k][0] <= recs[k - 1][0]
        for t in range(k):
            assert recs[k][3] < recs[t][1] or recs[t][3] < recs[k][1], (recs[t], recs[k])


def ones(shape, diagonals, extra=()):
    """A plot with diagonals of ones: (row, column, cells) each, B[row + k][column + k] = 1; and single ones at `extra`."""
    B = np.zeros(shape, np.uint8)
    for r, c, n in diagonals:
        for k in range(n):
            B[r + k, c + k] = 1
    for c in extra:
        B[c] = 1
    return B


def random_case(rng):
    """One random plot and its options, drawn as the issue's check drew them."""
    M, N = int(rng.integers(3, 41)), int(rng.integers(3, 41))
    dens = (0.05, 0.1, 0.3, 0.5, 0.9)[int(rng.integers(5))]
    B = (rng.random((M, N)) < dens).astype(np.uint8)
    opts = dict(max_sections=(1, 2, 4, 16)[int(rng.integers(4))], min_score=(1.1, 2.0, 3.0)[int(rng.integers(3))],
                min_ratio=(0.0, 0.5)[int(rng.integers(2))], pad=int(rng.integers(0, 4)))
    return B, opts


# Hand-checked plots: (name, B, options, records).  A diagonal of n ones whose first cell has no 1 diagonally above it scores
# 10 n - 7 tenths (its first cell 10 - 7); one that starts diagonally below a 1 of a border row OR of an excluded row -- U' = 0 there,
# T' = 0 -- scores 10 n.
BRIDGE = ones((120, 260), [(21, 21, 19), (40, 200, 20), (60, 50, 18)])
THREE = ones((60, 120), [(4, 4, 12), (20, 50, 9), (40, 90, 6)])
CUT = ones((40, 90), [(10, 10, 12), (16, 60, 15)])
TIE2 = ones((60, 60), [(20, 20, 10), (2, 40, 6), (40, 2, 6)])
# ones at (1, 1) .. (9, 9): the counted cells (2, 2) .. (9, 9) score 10 .. 80; (9, 29) is a 1 of the row section 0 excludes, so the
# diagonal (10, 30) .. (13, 33) below it scores 10 .. 40 in round 1: 4.0 == 0.5 * 8.0
RATIO = ones((30, 40), [(1, 1, 9), (9, 29, 5)])
ONE_ROW = ones((20, 30), [(2, 2, 6), (9, 2, 6)], extra=[(7, 19), (8, 20)])
HAND = [
    # with rows 40..59 CLEARED instead of T' forced to 0 the second answer would run from (21, 21) through them to (77, 67)
    ("no bridge over an excluded stretch", BRIDGE, dict(max_sections=4),
     [(19.3, 40, 200, 59, 219), (18.3, 21, 21, 39, 39), (17.3, 60, 50, 77, 67)]),
    ("three diagonals", THREE, dict(max_sections=4), [(11.3, 4, 4, 15, 15), (8.3, 20, 50, 28, 58), (5.3, 40, 90, 45, 95)]),
    ("min_score 8.3: equality reported", THREE, dict(max_sections=4, min_score=8.3), [(11.3, 4, 4, 15, 15), (8.3, 20, 50, 28, 58)]),
    ("min_score 8.4", THREE, dict(max_sections=4, min_score=8.4), [(11.3, 4, 4, 15, 15)]),
    ("max_sections 2", THREE, dict(max_sections=2), [(11.3, 4, 4, 15, 15), (8.3, 20, 50, 28, 58)]),
    ("min_ratio 0.5: threshold 4.0, equality reported", RATIO, dict(max_sections=4, min_ratio=0.5), [(8.0, 2, 2, 9, 9), (4.0, 10, 30, 13, 33)]),
    ("min_ratio 0.51", RATIO, dict(max_sections=4, min_ratio=0.51), [(8.0, 2, 2, 9, 9)]),
    # the 15-cell diagonal takes rows 16..30; the 12-cell one from (10, 10) keeps rows 10..15
    ("a long diagonal cuts a shorter one", CUT, dict(max_sections=4), [(14.3, 16, 60, 30, 74), (5.3, 10, 10, 15, 15)]),
    # three diagonals of 8 in ONE interval (each left of the ones above it: what decays behind a diagonal's end spreads down and right)
    ("a tie inside one interval: the smaller row wins", ones((50, 50), [(30, 5, 8), (6, 30, 8), (18, 18, 8)]), dict(max_sections=3),
     [(7.3, 6, 30, 13, 37), (7.3, 18, 18, 25, 25), (7.3, 30, 5, 37, 12)]),
    # section 0 (rows 20..29) splits the rows into [0, 19] and [30, 59]; each holds a diagonal of 6: the two intervals' records tie,
    # and the one with the smaller end cell -- rows 2..7 -- is section 1
    ("a tie between two intervals: the smaller end cell wins", TIE2, dict(max_sections=4),
     [(9.3, 20, 20, 29, 29), (5.3, 2, 40, 7, 45), (5.3, 40, 2, 45, 7)]),
    # pad 3 at row 0: section 0 has rows 2..9, rows 0..12 are excluded; of the diagonal from (11, 20) rows 13..16 are left -- 4 cells
    # below the 1 at (12, 21) of an excluded row: 4.0 --, the one from (13, 30) scores 4.3 and its pad takes rows 13..20
    ("pad clipped at row 0", ones((40, 40), [(2, 2, 8), (11, 20, 6), (13, 30, 5)]), dict(max_sections=3, pad=3),
     [(7.3, 2, 2, 9, 9), (4.3, 13, 30, 17, 34)]),
    # row 39 does not count: 9 cells; rows 27..39 are excluded, of the diagonal from (20, 5) rows 20..26 are left
    ("pad clipped at the last row", ones((40, 40), [(30, 30, 10), (20, 5, 8)]), dict(max_sections=3, pad=3),
     [(8.3, 30, 30, 38, 38), (6.3, 20, 5, 26, 11)]),
    # section 0 has rows 20..29, pad 2: rows 18..31 are excluded.  The two diagonals of 8 tie, the one in rows 2..9 is section 1 and
    # excludes rows 0..11; of the other, rows 12..17 are left below the 1 at (11, 41): 6.0.  Section 2 lies in the free interval
    # [12, 17] and its pad stops at 12 and at 17 -- not across section 1 or section 0
    ("pad clipped at an earlier section", ones((50, 60), [(20, 20, 10), (10, 40, 8), (2, 20, 8), (34, 2, 4)]), dict(max_sections=4, pad=2),
     [(9.3, 20, 20, 29, 29), (7.3, 2, 20, 9, 27), (6.0, 12, 42, 17, 47), (3.3, 34, 2, 37, 5)]),
    # the two diagonals of 6 tie; rows 2..7 and 9..14 leave [8, 8]: ONE counted row, not swept -- the 1 at (8, 20) below the 1 at
    # (7, 19) of an excluded row scores 1.0 there, which no min_score admits
    ("an interval of one counted row", ONE_ROW, dict(max_sections=4, min_score=1.01), [(5.3, 2, 2, 7, 7), (5.3, 9, 2, 14, 7)]),
]


def hand_records(recs):
    return [tuple([float(F(r[0]))] + list(r[1:])) for r in recs]
