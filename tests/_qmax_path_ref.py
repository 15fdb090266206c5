"""
The yardstick of the Qmax alignment PATH (acx_serra09_align_paths / acx_qmax_path_binary): two independent
restatements, in f32, of the path of tests/_qmax_locate_ref.py's contract -- the same Q, end, predecessor and start, the same
orientation and tie rules -- as the sequence of cells from the start (q0, r0) to the end (q1, r1), both included, that the
predecessor chain from the end visits.  Coordinates are rows / columns of R (with dp_start == 3 the DP cell (i, j) reads
R[i-1][j-1]; listed is the R index).  No match: score 0, -1 four times, no cells.

  path_full   (a) the full Q matrix (a row at a time, vectorised over its columns), then an explicit traceback from the row-major
                  first maximum that recomputes every visited cell's three candidates and records the cells
  path_box    (b) the DP on the cells of a given box [q0, q1] x [r0, r1] only, cell by cell, reading 0 for every Q outside it (R is
                  read as it is, outside the box as well) and storing one 2-bit code per cell -- 0 none, 1 / 2 / 3 for
                  (i-1, j-1) / (i-2, j-1) / (i-1, j-2) -- then a traceback over the codes from the box's last cell

Both return (record, cells, q): record = (score, q0, r0, q1, r1), cells an (L, 2) int32 array from start to end, q the (L,) f32
values of Q on them.  The BOX PROPERTY (tests/test_qmax_path_ref.py): (b) on the box (a) reports gives (a)'s cells and values.
"""
import numpy as np

F = np.float32
NO_MATCH = (0.0, -1, -1, -1, -1)
STEPS = {1: (1, 1), 2: (2, 1), 3: (1, 2)}          # code -> how far the predecessor lies back (rows, columns)


def _plot(R):
    R = np.ascontiguousarray(R, dtype=np.uint8)
    assert R.ndim == 2 and R.max(initial=0) <= 1
    return R


def _empty():
    return NO_MATCH, np.zeros((0, 2), np.int32), np.zeros(0, F)


def full_matrix(R, gamma_o=0.5, gamma_e=0.5, dp_start=2):
    """Q in DP coordinates, (M, N) f32."""
    R = _plot(R)
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
        c2, c3, c4 = Q[i - 1, js - 1], Q[i - 2, js - 1], Q[i - 1, js - 2]
        mx = np.maximum(np.maximum(c2, c3), c4)
        a2 = (c2 - np.where(R[ri - 1, rj - 1] != 0, go, ge)).astype(F)
        a3 = (c3 - np.where(R[ri - 2, rj - 1] != 0, go, ge)).astype(F)
        a4 = (c4 - np.where(R[ri - 1, rj - 2] != 0, go, ge)).astype(F)
        ax = np.maximum(np.maximum(np.maximum(a2, a3), a4), F(0))
        Q[i, st:] = np.where(R[ri, rj] != 0, (mx + F(1)).astype(F), ax)
    return Q


def path_full(R, gamma_o=0.5, gamma_e=0.5, dp_start=2):
    """(a)."""
    R = _plot(R)
    o = 1 if dp_start == 3 else 0
    go, ge = F(gamma_o), F(gamma_e)
    Q = full_matrix(R, gamma_o, gamma_e, dp_start)
    best = Q.max(initial=F(0))
    if not best > 0:
        return _empty()
    end = np.unravel_index(int(np.argmax(Q)), Q.shape)          # the first maximum in row-major order
    i, j = int(end[0]), int(end[1])
    cells, qs = [], []
    while True:
        assert Q[i, j] > 0
        cells.append((i - o, j - o))
        qs.append(Q[i, j])
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
            break                                               # a path starts here
        assert vals[pick] > 0                                   # (a gap cell with Q > 0 has a penalised predecessor > 0)
        i, j = pred[pick]
    cells.reverse()
    qs.reverse()
    rec = (float(best), cells[0][0], cells[0][1], cells[-1][0], cells[-1][1])
    return rec, np.array(cells, np.int32).reshape(-1, 2), np.array(qs, F)


def path_box(R, record, gamma_o=0.5, gamma_e=0.5, dp_start=2):
    """(b): the path inside the box of `record` (score, q0, r0, q1, r1), in R coordinates throughout.  dp_start does not enter: the
    box lies where the DP runs, and Q is 0 outside the box whatever the reason."""
    R = _plot(R)
    score, q0, r0, q1, r1 = record
    if q0 < 0:
        return _empty()
    go, ge = F(gamma_o), F(gamma_e)
    h, w = q1 - q0 + 1, r1 - r0 + 1
    Qb = np.zeros((h, w), F)
    code = np.zeros((h, w), np.uint8)

    def q_at(y, x):                                             # Q of plot cell (y, x): 0 outside the box
        return Qb[y - q0, x - r0] if (q0 <= y <= q1 and r0 <= x <= r1) else F(0)

    for y in range(q0, q1 + 1):
        for x in range(r0, r1 + 1):
            pred = ((y - 1, x - 1), (y - 2, x - 1), (y - 1, x - 2))
            if R[y, x]:
                vals = [q_at(*c) for c in pred]
            else:
                vals = [F(q_at(*c) - (go if R[c] else ge)) for c in pred]
            k = 0
            if vals[1] > vals[0]:
                k = 1
            if vals[2] > vals[k]:
                k = 2
            if R[y, x]:
                Qb[y - q0, x - r0] = F(vals[k] + F(1))
                code[y - q0, x - r0] = 0 if vals[k] == 0 else k + 1
            elif vals[k] > 0:
                Qb[y - q0, x - r0] = vals[k]
                code[y - q0, x - r0] = k + 1
    y, x = q1, r1
    cells, qs = [], []
    while True:
        assert q0 <= y <= q1 and r0 <= x <= r1, "the traceback left the box"
        cells.append((y, x))
        qs.append(Qb[y - q0, x - r0])
        k = int(code[y - q0, x - r0])
        if k == 0:
            break
        y, x = y - STEPS[k][0], x - STEPS[k][1]
    cells.reverse()
    qs.reverse()
    rec = (float(Qb[h - 1, w - 1]), cells[0][0], cells[0][1], q1, r1)
    return rec, np.array(cells, np.int32).reshape(-1, 2), np.array(qs, F)


def _ones(shape, cells):
    R = np.zeros(shape, np.uint8)
    for c in cells:
        R[c] = 1
    return R


# Hand-checked plots: (name, R, (gamma_o, gamma_e, dp_start), record, cells)
HAND = [
    # a pure diagonal: Q = 1 .. 6 on (2, 2) .. (7, 7); rows and columns 0 and 1 stay 0
    ("eye(8)", np.eye(8, dtype=np.uint8), (0.5, 0.5, 2), (6.0, 2, 2, 7, 7), [(t, t) for t in range(2, 8)]),
    # (3, 3) = 2; (4, 4) is missing, (5, 4) takes c3 = Q[3][3] = 2 over c2 = Q[4][3] = 0.5 (a gap cell behind (2, 2)): a (2, 1) step
    ("a (2, 1) step over a missing cell", _ones((9, 9), [(2, 2), (3, 3), (5, 4), (6, 5)]), (0.5, 0.5, 2), (4.0, 2, 2, 6, 5),
     [(2, 2), (3, 3), (5, 4), (6, 5)]),
    # the transpose: (4, 5) takes c4 = Q[3][3]
    ("a (1, 2) step over a missing cell", _ones((9, 9), [(2, 2), (3, 3), (4, 5), (5, 6)]), (0.5, 0.5, 2), (4.0, 2, 2, 5, 6),
     [(2, 2), (3, 3), (4, 5), (5, 6)]),
    # (3, 4) = (4, 4) = 1, (4, 5) = 2; (5, 5): c2 = Q[4][4] = 1 ties c3 = Q[3][4] = 1; (6, 6): c2 = Q[5][5] = 2 ties c3 = Q[4][5] = 2:
    # c2 wins both times, the path is the diagonal from (4, 4)
    ("c2 and c3 tie, c2 wins", _ones((9, 9), [(4, 4), (5, 5), (3, 4), (4, 5), (6, 6)]), (0.5, 0.5, 2), (3.0, 4, 4, 6, 6),
     [(4, 4), (5, 5), (6, 6)]),
    # one missing cell ON the diagonal: (5, 5) is a gap cell, 3 - 0.5, its predecessor the first of the penalised a2, a3, a4
    ("one gap on the diagonal", _ones((10, 10), [(t, t) for t in range(10) if t != 5]), (0.5, 0.5, 2), (6.5, 2, 2, 9, 9),
     [(t, t) for t in range(2, 10)]),
    # dp_start 3: DP cell (i, j) reads R[i-1][j-1], the last row and column of the plot are never read; listed is the R index
    ("eye(8), dp_start 3", np.eye(8, dtype=np.uint8), (0.5, 0.5, 3), (5.0, 2, 2, 6, 6), [(t, t) for t in range(2, 7)]),
]
