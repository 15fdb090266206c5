"""
The yardstick of the Dmax alignment and its path (acx_chenfusion_align* plane 1, acx_dmax_locate_binary / acx_dmax_path_binary,
DESIGN.md section 22): two independent restatements, in f32, of

  Q       the matrix of oracle/acx_oracle.c step 6 with dmax = 1 (acx_o_qmax_binary(..., dmax=1) for a given plot):
          c2 = Q[i-1][j-1], c3 = Q[i-2][j-1] + R[i-1][j], c4 = Q[i-1][j-2] + R[i][j-1];
          match: max(c2, c3, c4) + 1; gap: max(0, c2 - g(R[i-1][j-1]), c3 - g(R[i-2][j-1]), c4 - g(R[i-1][j-2]))
  score   max Q
  end     the first cell in row-major order at which Q attains it
  chosen  match cell: the first of c2, c3, c4 (bonus included) equal to their maximum; gap cell with Q > 0: the first of the three
          penalised values equal to their maximum
  pred    the chosen candidate's cell; none -- a path starts here -- when Q of THAT cell, without its bonus, is 0
  path    the cells the predecessor chain from the end visits, listed from the start to the end

Coordinates are rows / columns of R (with dp_start == 3 the DP cell (i, j) reads R[i-1][j-1]; listed is the R index).  No match: score 0,
-1 four times, no cells.  `bonus=False` switches the two added bits off: the contract is then that of tests/_qmax_locate_ref.py and
tests/_qmax_path_ref.py.

  dmax_full      (a) the full Q matrix in DP coordinates (a row at a time), then an explicit traceback from the row-major first maximum that
                     recomputes every visited cell's three candidates
  dmax_forward   (b1) forward propagation of S[i][j] = the start of the path through (i, j) beside Q and the chosen candidate's own Q,
                     two rolling rows, on the plot less its last row / column for dp_start == 3: the record alone
  dmax_box       (b2) the DP on the cells of a given box only, cell by cell, 0 for every Q outside it, R read AS IT IS outside it as
                     well (bonus bits and penalties), one 2-bit code per cell, then a traceback over the codes

(a) and (b2) return (record, cells, q): record = (score, q0, r0, q1, r1), cells (L, 2) int32 from start to end, q the (L,) f32 values of Q
on them.  The BOX PROPERTY (tests/test_dmax_align_ref.py): (b2) on the box (a) reports gives (a)'s cells and values.
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


def full_matrix(R, gamma_o=0.5, gamma_e=0.5, dp_start=2, bonus=True):
    """Q in DP coordinates, (M, N) f32."""
    R = _plot(R)
    M, N = R.shape
    st, o = int(dp_start), (1 if dp_start == 3 else 0)
    Q = np.zeros((M, N), F)
    if M <= st or N <= st:
        return Q
    go, ge = F(gamma_o), F(gamma_e)
    b = F(1 if bonus else 0)
    js = np.arange(st, N)
    rj = js - o
    for i in range(st, M):
        ri = i - o
        c2 = Q[i - 1, js - 1]
        c3 = (Q[i - 2, js - 1] + b * R[ri - 1, rj].astype(F)).astype(F)
        c4 = (Q[i - 1, js - 2] + b * R[ri, rj - 1].astype(F)).astype(F)
        mx = np.maximum(np.maximum(c2, c3), c4)
        a2 = (c2 - np.where(R[ri - 1, rj - 1] != 0, go, ge)).astype(F)
        a3 = (c3 - np.where(R[ri - 2, rj - 1] != 0, go, ge)).astype(F)
        a4 = (c4 - np.where(R[ri - 1, rj - 2] != 0, go, ge)).astype(F)
        ax = np.maximum(np.maximum(np.maximum(a2, a3), a4), F(0))
        Q[i, st:] = np.where(R[ri, rj] != 0, (mx + F(1)).astype(F), ax)
    return Q


def dmax_full(R, gamma_o=0.5, gamma_e=0.5, dp_start=2, bonus=True):
    """(a)."""
    R = _plot(R)
    o = 1 if dp_start == 3 else 0
    go, ge = F(gamma_o), F(gamma_e)
    Q = full_matrix(R, gamma_o, gamma_e, dp_start, bonus)
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
        ri, rj = i - o, j - o
        pred = ((i - 1, j - 1), (i - 2, j - 1), (i - 1, j - 2))
        add = (F(0), F(R[ri - 1, rj]) if bonus else F(0), F(R[ri, rj - 1]) if bonus else F(0))
        vals = [F(Q[c] + x) for c, x in zip(pred, add)]
        if not R[ri, rj]:
            vals = [F(v - (go if R[c[0] - o, c[1] - o] else ge)) for v, c in zip(vals, pred)]
        pick = 0
        for k in (1, 2):
            if vals[k] > vals[pick]:
                pick = k
        assert Q[i, j] == (F(vals[pick] + F(1)) if R[ri, rj] else vals[pick])
        if Q[pred[pick]] == 0:
            break                                               # the chosen candidate's own Q is 0: a path starts here
        i, j = pred[pick]
    cells.reverse()
    qs.reverse()
    rec = (float(best), cells[0][0], cells[0][1], cells[-1][0], cells[-1][1])
    return rec, np.array(cells, np.int32).reshape(-1, 2), np.array(qs, F)


def dmax_forward(R, gamma_o=0.5, gamma_e=0.5, dp_start=2, bonus=True):
    """(b1): (score, q0, r0, q1, r1).  dp_start == 3 is the same DP on the plot less its last row and column, in R coordinates."""
    R = _plot(R)
    N0 = R.shape[1]
    if dp_start == 3:
        R = R[:-1, :-1]
    M, N = R.shape
    if M <= 2 or N <= 2:
        return NO_MATCH
    go, ge = F(gamma_o), F(gamma_e)
    gam = lambda bits: np.where(bits != 0, go, ge).astype(F)
    js = np.arange(2, N)
    q1, q2 = np.zeros(N, F), np.zeros(N, F)                     # rows i - 1, i - 2 of Q
    s1, s2 = np.full(N, -1, np.int64), np.full(N, -1, np.int64)      # ... of S, as (row) * N0 + (column) of the whole plot
    best, end, start = F(0), -1, -1
    for i in range(2, M):
        x3 = R[i - 1, js].astype(F) if bonus else np.zeros(len(js), F)
        x4 = R[i, js - 1].astype(F) if bonus else np.zeros(len(js), F)
        own = (q1[js - 1], q2[js - 1], q1[js - 2])              # the candidates' own Q
        c = (own[0], (own[1] + x3).astype(F), (own[2] + x4).astype(F))
        s = (s1[js - 1], s2[js - 1], s1[js - 2])
        match = R[i, js] != 0
        # match: the strict `>` chain over c2, c3, c4, carrying the chosen one's S and own Q
        mx, sm, om = c[0], s[0], own[0]
        for k in (1, 2):
            up = c[k] > mx
            mx, sm, om = np.where(up, c[k], mx), np.where(up, s[k], sm), np.where(up, own[k], om)
        # gap: the same chain over the penalised values
        a = ((c[0] - gam(R[i - 1, js - 1])).astype(F), (c[1] - gam(R[i - 2, js - 1])).astype(F), (c[2] - gam(R[i - 1, js - 2])).astype(F))
        ax, sa, oa = a[0], s[0], own[0]
        for k in (1, 2):
            up = a[k] > ax
            ax, sa, oa = np.where(up, a[k], ax), np.where(up, s[k], sa), np.where(up, own[k], oa)
        q = np.zeros(N, F)
        sn = np.full(N, -1, np.int64)
        q[2:] = np.where(match, (mx + F(1)).astype(F), np.maximum(ax, F(0)))
        chosen_s, chosen_q = np.where(match, sm, sa), np.where(match, om, oa)
        sn[2:] = np.where(q[2:] > 0, np.where(chosen_q == 0, i * N0 + js, chosen_s), -1)
        jm = int(np.argmax(q))                                  # (the first maximum of the row)
        if q[jm] > best:
            best, end, start = q[jm], i * N0 + jm, int(sn[jm])
        q2, s2 = q1, s1
        q1, s1 = q, sn
    if end < 0:
        return NO_MATCH
    return (float(best), start // N0, start % N0, end // N0, end % N0)


def dmax_box(R, record, gamma_o=0.5, gamma_e=0.5, bonus=True):
    """(b2): the path inside the box of `record` (score, q0, r0, q1, r1), in R coordinates throughout.  dp_start does not enter: the box
    lies where the DP runs, Q is 0 outside the box whatever the reason, and R is read as it is."""
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
            own = [q_at(*c) for c in pred]
            vals = [own[0], F(own[1] + (F(R[y - 1, x]) if bonus else F(0))), F(own[2] + (F(R[y, x - 1]) if bonus else F(0)))]
            if not R[y, x]:
                vals = [F(v - (go if R[c] else ge)) for v, c in zip(vals, pred)]
            k = 0
            if vals[1] > vals[0]:
                k = 1
            if vals[2] > vals[k]:
                k = 2
            if R[y, x]:
                Qb[y - q0, x - r0] = F(vals[k] + F(1))
                code[y - q0, x - r0] = 0 if own[k] == 0 else k + 1
            elif vals[k] > 0:
                Qb[y - q0, x - r0] = vals[k]
                code[y - q0, x - r0] = 0 if own[k] == 0 else k + 1
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


def random_plot(rng, M, N, density):
    return (rng.random((M, N)) < density).astype(np.uint8)


GAMMAS = [(0.5, 0.5), (0.5, 0.7), (1.0, 0.25)]

# Hand-checked plots: (name, R, (gamma_o, gamma_e, dp_start), record, cells, Q on the cells).  Below, "gap x" is a gap cell holding x.
HAND = [
    # a pure diagonal: the bonus bits of a diagonal cell, R[i-1][i] and R[i][i-1], are 0, and its neighbours (i, i+1) / (i+1, i) are gap
    # cells holding Q[i-1][i-1] + 1 - 0.5 < Q[i][i]: Dmax is Qmax, 1 .. 6 on (2, 2) .. (7, 7)
    ("eye(8): Dmax equals Qmax", np.eye(8, dtype=np.uint8), (0.5, 0.5, 2), (6.0, 2, 2, 7, 7), [(t, t) for t in range(2, 8)],
     [1, 2, 3, 4, 5, 6]),
    # (5, 4): c2 = Q[4][3] = 1.5 (gap: Q[2][2] + R[3][3] - 0.5), c3 = Q[3][3] + R[4][4] = 2 + 0, c4 = 0: a (2, 1) step, 3; (6, 5) = 4
    ("a (2, 1) step, bonus cell (4, 4) unset", _ones((9, 9), [(2, 2), (3, 3), (5, 4), (6, 5)]), (0.5, 0.5, 2), (4.0, 2, 2, 6, 5),
     [(2, 2), (3, 3), (5, 4), (6, 5)], [1, 2, 3, 4]),
    # the same with (4, 4) set: c3 = Q[3][3] + R[4][4] = 3 beats c2 = 1.5; (5, 4) = 4, (6, 5) = 5 (c3 = Q[4][4] + R[5][5] = 3 loses).
    # The path steps OVER (4, 4), which only lends its bit
    ("a (2, 1) step, bonus cell (4, 4) set", _ones((9, 9), [(2, 2), (3, 3), (4, 4), (5, 4), (6, 5)]), (0.5, 0.5, 2), (5.0, 2, 2, 6, 5),
     [(2, 2), (3, 3), (5, 4), (6, 5)], [1, 2, 4, 5]),
    # the transposes: (4, 5) takes c4 = Q[3][3] + R[4][4]
    ("a (1, 2) step, bonus cell (4, 4) unset", _ones((9, 9), [(2, 2), (3, 3), (4, 5), (5, 6)]), (0.5, 0.5, 2), (4.0, 2, 2, 5, 6),
     [(2, 2), (3, 3), (4, 5), (5, 6)], [1, 2, 3, 4]),
    ("a (1, 2) step, bonus cell (4, 4) set", _ones((9, 9), [(2, 2), (3, 3), (4, 4), (4, 5), (5, 6)]), (0.5, 0.5, 2), (5.0, 2, 2, 5, 6),
     [(2, 2), (3, 3), (4, 5), (5, 6)], [1, 2, 4, 5]),
    # (4, 4): c2 = Q[3][3] = 0, c3 = Q[2][3] + R[3][4] = 0 + 1, c4 = 0: Q = 2, chosen c3 whose own Q is 0 -- the path starts at a cell
    # holding 2.  ((3, 4) itself holds 1.)
    ("a start with Q = 2", _ones((8, 8), [(3, 4), (4, 4)]), (0.5, 0.5, 2), (2.0, 4, 4, 4, 4), [(4, 4)], [2]),
    # (2, 2) is a GAP cell: c3 = Q[0][1] + R[1][2] = 1, less 0.5: it holds 0.5 and its chosen candidate (0, 1) holds 0: a gap start, fed by a
    # bonus from row 1 into DP row 2.  (3, 3) = 1.5, (4, 4) = 2.5
    ("a gap start: a bonus from row 1 into DP row 2", _ones((8, 8), [(1, 2), (3, 3), (4, 4)]), (0.5, 0.5, 2), (2.5, 2, 2, 4, 4),
     [(2, 2), (3, 3), (4, 4)], [0.5, 1.5, 2.5]),
    # the transpose: c4 = Q[1][0] + R[2][1]
    ("a gap start: a bonus from column 1 into DP column 2", _ones((8, 8), [(2, 1), (3, 3), (4, 4)]), (0.5, 0.5, 2), (2.5, 2, 2, 4, 4),
     [(2, 2), (3, 3), (4, 4)], [0.5, 1.5, 2.5]),
    # (3, 4) = 1; (4, 4) = 2 from c3 = Q[2][3] + R[3][4] (a start); (4, 5): c2 = Q[3][4] = 1 ties c4 = Q[3][3] + R[4][4] = 1, c2 wins, 2;
    # (5, 5): c2 = Q[4][4] = 2 ties c3 = Q[3][4] + R[4][5] = 2: c2 wins, 3; (6, 6): c2 = 3 beats c3 = Q[4][5] + R[5][6] = 2: 4
    ("c2 and c3 tie, c2 wins", _ones((9, 9), [(4, 4), (5, 5), (3, 4), (4, 5), (6, 6)]), (0.5, 0.5, 2), (4.0, 4, 4, 6, 6),
     [(4, 4), (5, 5), (6, 6)], [2, 3, 4]),
    # dp_start 3: DP cell (i, j) reads R[i-1][j-1], the last row and column of the plot are never read; listed is the R index
    ("eye(8), dp_start 3", np.eye(8, dtype=np.uint8), (0.5, 0.5, 3), (5.0, 2, 2, 6, 6), [(t, t) for t in range(2, 7)], [1, 2, 3, 4, 5]),
    # dp_start 3 and the gap start: the bonus comes from R row 1 all the same (the plot less its last row / column, same DP)
    ("a gap start, dp_start 3", _ones((8, 8), [(1, 2), (3, 3), (4, 4), (7, 7)]), (0.5, 0.5, 3), (2.5, 2, 2, 4, 4),
     [(2, 2), (3, 3), (4, 4)], [0.5, 1.5, 2.5]),
]
