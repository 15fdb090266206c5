"""
The contract of the EarlyFusion alignment (acx_ef_align / acx_sw_align_binary), stated twice and independently
for the tests.  For a binary (M, N) plot B, in integer tenths (tests/_ef_backend_ref.py::sw_tenths, the oracle's
acx_o_sw_constrained_i32):

  T[i][j] = max(0, (B[i][j] ? 10 : -10) + max(U[i-1][j-1], U[i-2][j-1], U[i-1][j-2])),  U = T + (B ? 0 : -7),
  T = 0 in rows and columns 0 and 1; only the cells 2 <= i <= M-2, 2 <= j <= N-2 count.

  score   max T / 10 as f32
  end     (q1, r1): the counted cell, first in row-major order, at which T attains the maximum
  pred    of a cell with T > 0: the first of (i-1, j-1), (i-2, j-1), (i-1, j-2) whose U equals the maximum of the three
  start   (q0, r0): the last cell with T > 0 on the chain of predecessors from the end
  path    the cells from start to end, both included, start first
  no match (score 0, or M < 4 or N < 4): NO_MATCH and an empty path

Both functions return ((score, q0, r0, q1, r1), cells (L, 2) int32).

  align_traceback  the whole T matrix by plain loops and an explicit traceback that records the cells (small plots)
  align_forward    one pass, vectorised over a row's columns, that carries beside every value the START of its chain and the chain's
                   LENGTH (a row needs only the two rows before it: fast enough for 1024 x 1024).  The end, the start and the
                   number of cells come from what was carried; the cells between them are read off the chosen-predecessor table
                   and must arrive at the carried start after the carried number of steps.
"""
import numpy as np

NO_MATCH = (0.0, -1, -1, -1, -1)
STEPS = {(1, 1), (2, 1), (1, 2)}
_EMPTY = np.zeros((0, 2), np.int32)


def align_traceback(B):
    B = np.asarray(B).astype(bool)
    M, N = B.shape
    if M < 4 or N < 4:
        return NO_MATCH, _EMPTY.copy()
    T = [[0] * N for _ in range(M)]
    U = [[0 if B[i, j] else -7 for j in range(N)] for i in range(M)]      # rows / columns 0, 1: T = 0, U = delta(B)
    D = [[0] * N for _ in range(M)]
    best, end = 0, None
    for i in range(2, M - 1):
        for j in range(2, N - 1):
            mx, d = U[i - 1][j - 1], 1
            if U[i - 2][j - 1] > mx:
                mx, d = U[i - 2][j - 1], 2
            if U[i - 1][j - 2] > mx:
                mx, d = U[i - 1][j - 2], 3
            t = max(0, (10 if B[i, j] else -10) + mx)
            T[i][j] = t
            U[i][j] = t + (0 if B[i, j] else -7)
            D[i][j] = d
            if t > best:
                best, end = t, (i, j)
    if best == 0:
        return NO_MATCH, _EMPTY.copy()
    cells = [end]
    y, x = end
    while True:
        d = D[y][x]
        py, px = y - (2 if d == 2 else 1), x - (2 if d == 3 else 1)
        if T[py][px] == 0:
            break
        y, x = py, px
        cells.append((y, x))
    cells.reverse()
    return (float(np.float32(best) / np.float32(10)), y, x, end[0], end[1]), np.array(cells, np.int32).reshape(-1, 2)


def align_forward(B):
    B = np.asarray(B).astype(bool)
    M, N = B.shape
    if M < 4 or N < 4:
        return NO_MATCH, _EMPTY.copy()
    gap = np.where(B, 0, -7).astype(np.int64)
    hit = np.where(B, 10, -10).astype(np.int64)
    js = np.arange(2, N - 1)                                   # the counted columns
    zeros = np.zeros(N, np.int64)
    # rows i-1 and i-2: T, U, and beside every value the start of its chain and the chain's length
    T1, T2, U1, U2 = zeros.copy(), zeros.copy(), gap[1].copy(), gap[0].copy()
    Q1, Q2, R1, R2, L1, L2 = (zeros.copy() for _ in range(6))
    parent = np.full((M, N), -1, np.int64)                     # flat index of the chosen predecessor where that has T > 0
    best, rec = 0, None
    for i in range(2, M - 1):
        mx, d = U1[js - 1], np.ones(len(js), np.int64)
        m = U2[js - 1] > mx
        mx, d = np.where(m, U2[js - 1], mx), np.where(m, 2, d)
        m = U1[js - 2] > mx
        mx, d = np.where(m, U1[js - 2], mx), np.where(m, 3, d)
        t = np.maximum(0, hit[i, js] + mx)

        def of_pred(a1, a2):
            return np.where(d == 1, a1[js - 1], np.where(d == 2, a2[js - 1], a1[js - 2]))
        fresh = of_pred(T1, T2) == 0                           # the chosen predecessor has T == 0: the chain starts here
        q = np.where(fresh, i, of_pred(Q1, Q2))
        r = np.where(fresh, js, of_pred(R1, R2))
        ln = np.where(fresh, 1, of_pred(L1, L2) + 1)
        pflat = (i - np.where(d == 2, 2, 1)) * N + (js - np.where(d == 3, 2, 1))
        parent[i, js] = np.where((t > 0) & ~fresh, pflat, -1)
        if int(t.max()) > best:                                # strictly larger: an earlier row keeps a tie; argmax: the first column
            k = int(np.argmax(t))
            best, rec = int(t[k]), (int(q[k]), int(r[k]), i, int(js[k]), int(ln[k]))
        T2, U2, Q2, R2, L2 = T1, U1, Q1, R1, L1
        T1, U1, Q1, R1, L1 = zeros.copy(), gap[i].copy(), zeros.copy(), zeros.copy(), zeros.copy()
        T1[js], Q1[js], R1[js], L1[js] = t, q, r, ln
        U1[js] = t + gap[i, js]
    if best == 0:
        return NO_MATCH, _EMPTY.copy()
    q0, r0, q1, r1, ln = rec
    cells = np.zeros((ln, 2), np.int32)
    at = q1 * N + r1
    for k in range(ln - 1, -1, -1):
        assert at >= 0, "the chain is shorter than the carried length"
        cells[k] = divmod(at, N)
        at = int(parent[cells[k, 0], cells[k, 1]])
    assert at == -1 and tuple(cells[0]) == (q0, r0), "the chain does not start where the carried start says"
    return (float(np.float32(best) / np.float32(10)), q0, r0, q1, r1), cells


def check_path(rec, cells, shape):
    """What every answer obeys: start and end of the path are the record's, the step set, the length bound, the counted rectangle."""
    M, N = shape
    if rec == NO_MATCH:
        assert len(cells) == 0
        return
    assert rec[0] > 0 and len(cells) >= 1
    assert tuple(cells[0]) == rec[1:3] and tuple(cells[-1]) == rec[3:5]
    assert len(cells) <= min(M, N)
    assert cells[:, 0].min() >= 2 and cells[:, 0].max() <= M - 2 and cells[:, 1].min() >= 2 and cells[:, 1].max() <= N - 2
    assert {tuple(s) for s in np.diff(cells, axis=0)} <= STEPS


def _plot(shape, ones):
    B = np.zeros(shape, np.uint8)
    for c in ones:
        B[c] = 1
    return B


def hand_checked():
    """(name, plot, record, cells): answers worked out by hand.  A chain that starts from border cells without a 1 begins at
    10 - 7 = 3 tenths, one that starts diagonally below a border 1 at 10."""
    diag = lambda a, b, n: [(a + d, b + d) for d in range(n)]
    out = []
    # a pure diagonal: (1, 1) is a border 1 (U = 0), so (2, 2) scores 10 and (8, 8) 70; row and column 9 do not count
    out.append(("diagonal", np.eye(10, dtype=np.uint8), (7.0, 2, 2, 8, 8), diag(2, 2, 7)))
    # a (2, 1) and a (1, 2) step: 3, 13, then (5, 4) takes (3, 3) by its second predecessor, (7, 7) takes (6, 5) by its third
    path = [(2, 2), (3, 3), (5, 4), (6, 5), (7, 7), (8, 8)]
    out.append(("steps", _plot((12, 12), path), (5.3, 2, 2, 8, 8), path))
    # (6, 6): U[5][5] = U[4][5] = 13, the first predecessor wins; so it does at (5, 5), where U[4][4] = U[3][4] = 3
    out.append(("tie_first_two", _plot((9, 9), [(4, 4), (5, 5), (3, 4), (4, 5), (6, 6)]), (2.3, 4, 4, 6, 6), [(4, 4), (5, 5), (6, 6)]))
    # (3, 3): the interior cell (2, 2) (T = 0, no 1: U = -7) ties with the border cells (1, 2) and (2, 1) (U = -7); the first, (2, 2),
    # is chosen, its T is 0, and the path starts at (3, 3) with 3
    out.append(("tie_border_interior", _plot((8, 8), [(3, 3), (4, 4)]), (1.3, 3, 3, 4, 4), [(3, 3), (4, 4)]))
    # the chain is on U, and a border cell has T = 0 whatever its U: at (3, 3) the border 1 at (1, 2) (U = 0) beats the empty interior
    # cell (2, 2) (U = -7), so (3, 3) scores 10 and -- its predecessor being a border cell -- starts the path; with a 1 at (2, 2) as
    # well (T = U = 3) the interior cell wins and the path starts there
    out.append(("border_one_wins", _plot((8, 8), [(1, 2), (3, 3), (4, 4)]), (2.0, 3, 3, 4, 4), [(3, 3), (4, 4)]))
    out.append(("interior_beats_border_one", _plot((8, 8), [(1, 2), (2, 2), (3, 3), (4, 4)]), (2.3, 2, 2, 4, 4), [(2, 2), (3, 3), (4, 4)]))
    # two equal maxima (3, 13, 23, 33 each): the row-major first one is reported
    out.append(("equal_maxima_rows", _plot((40, 40), diag(2, 2, 4) + diag(25, 30, 4)), (3.3, 2, 2, 5, 5), diag(2, 2, 4)))
    out.append(("equal_maxima_same_row", _plot((20, 20), diag(9, 2, 4) + diag(9, 12, 4)), (3.3, 9, 2, 12, 5), diag(9, 2, 4)))
    # the smallest plot with a counted cell: (2, 2) alone, below the border 1 at (1, 1)
    out.append(("ones_4x4", np.ones((4, 4), np.uint8), (1.0, 2, 2, 2, 2), [(2, 2)]))
    return [(name, B, tuple(np.float32(v) if k == 0 else v for k, v in enumerate(rec)), np.array(cells, np.int32).reshape(-1, 2))
            for name, B, rec, cells in out]


def no_match_plots():
    """The designated empty and too-small plots."""
    return [np.zeros((7, 9), np.uint8), np.zeros((4, 4), np.uint8), np.ones((3, 9), np.uint8), np.ones((9, 3), np.uint8),
            np.ones((1, 1), np.uint8), np.ones((3, 3), np.uint8), np.ones((1, 30), np.uint8)]


def random_plot(rng, M, N, density):
    """A random plot with a 1 planted at a random counted cell (M, N >= 4): it has a match, T >= 3 there."""
    B = (rng.random((M, N)) < density).astype(np.uint8)
    B[int(rng.integers(2, M - 1)), int(rng.integers(2, N - 1))] = 1
    return B
