"""
The yardstick of the locating Qmax sweep (acx_serra09_align / acx_qmax_locate_binary): two independent
numpy / Python restatements, in f32, of

  Q       the matrix of oracle/acx_oracle.c step 6 (acx_o_qmax_binary for a given plot) with dp_start, gamma_o, gamma_e
  score   max Q
  end     the first cell in row-major order at which Q attains it (the oracle's strict `v > best`)
  pred    match cell: the first of c2 = Q[i-1][j-1], c3 = Q[i-2][j-1], c4 = Q[i-1][j-2] equal to their maximum (the
          oracle's strict `>` chain), none when that maximum is 0; gap cell with Q > 0: the first of the penalised
          a2, a3, a4 equal to their maximum
  start   follow predecessors from the end until a cell has none

Coordinates are rows / columns of R (with dp_start == 3 the DP cell (i, j) reads R[i-1][j-1]; reported is the R index).
No match: score 0 and -1 four times.

  locate_traceback   (a) the full Q matrix, cell by cell, then an explicit traceback from the row-major first maximum
  locate_forward     (b) forward propagation of S[i][j] = the start of the path through (i, j), two rolling rows, a row at a time
"""
import numpy as np

F = np.float32
NO_MATCH = (0.0, -1, -1, -1, -1)


def _plot(R):
    R = np.ascontiguousarray(R, dtype=np.uint8)
    assert R.ndim == 2 and R.max(initial=0) <= 1
    return R


def locate_traceback(R, gamma_o=0.5, gamma_e=0.5, dp_start=2):
    """(a): (score, q0, r0, q1, r1)."""
    R = _plot(R)
    M, N = R.shape
    st, o = int(dp_start), (1 if dp_start == 3 else 0)
    go, ge = F(gamma_o), F(gamma_e)
    Q = np.zeros((M, N), F)

    def candidates(i, j):
        """The three predecessors of DP cell (i, j): ((cell, value as the cell's branch sees it), ...)."""
        ri, rj = i - o, j - o
        cells = ((i - 1, j - 1), (i - 2, j - 1), (i - 1, j - 2))
        if R[ri, rj]:
            return [(c, Q[c]) for c in cells]
        bits = (R[ri - 1, rj - 1], R[ri - 2, rj - 1], R[ri - 1, rj - 2])
        return [(c, F(Q[c] - (go if b else ge))) for c, b in zip(cells, bits)]

    best, end = F(0), None
    for i in range(st, M):
        for j in range(st, N):
            vals = [v for _, v in candidates(i, j)]
            if R[i - o, j - o]:
                mx = vals[0]
                for v in vals[1:]:
                    if v > mx:
                        mx = v
                q = F(mx + F(1))
            else:
                q = F(0)
                for v in vals:
                    if v > q:
                        q = v
            Q[i, j] = q
            if q > best:
                best, end = q, (i, j)
    if end is None:
        return NO_MATCH
    i, j = end
    while True:
        assert Q[i, j] > 0
        cand = candidates(i, j)
        pick = 0
        for k in (1, 2):
            if cand[k][1] > cand[pick][1]:
                pick = k
        if R[i - o, j - o] and cand[pick][1] == 0:
            break                                  # a path starts here
        assert cand[pick][1] > 0                   # (a gap cell with Q > 0 has a penalised predecessor > 0)
        i, j = cand[pick][0]
    return (float(best), i - o, j - o, end[0] - o, end[1] - o)


def locate_forward(R, gamma_o=0.5, gamma_e=0.5, dp_start=2):
    """(b): (score, q0, r0, q1, r1); vectorised over the columns of a row (cell (i, j) reads rows i - 1 and i - 2 only)."""
    R = _plot(R)
    M, N = R.shape
    st, o = int(dp_start), (1 if dp_start == 3 else 0)
    if M <= st or N <= st:
        return NO_MATCH
    go, ge = F(gamma_o), F(gamma_e)
    gam = lambda bits: np.where(bits != 0, go, ge).astype(F)
    js = np.arange(st, N)
    rj = js - o
    q1, q2 = np.zeros(N, F), np.zeros(N, F)        # rows i - 1, i - 2 of Q
    s1, s2 = np.full(N, -1, np.int64), np.full(N, -1, np.int64)      # ... of S, as (R row) * N + (R column)
    best, end, start = F(0), -1, -1
    for i in range(st, M):
        ri = i - o
        c = (q1[js - 1], q2[js - 1], q1[js - 2])
        s = (s1[js - 1], s2[js - 1], s1[js - 2])
        match = R[ri, rj] != 0
        # match: the strict `>` chain over c2, c3, c4
        mx, sm = c[0], s[0]
        for k in (1, 2):
            up = c[k] > mx
            mx, sm = np.where(up, c[k], mx), np.where(up, s[k], sm)
        sm = np.where(mx == 0, ri * N + rj, sm)
        # gap: the same chain over the penalised values, from 0
        a = ((c[0] - gam(R[ri - 1, rj - 1])).astype(F), (c[1] - gam(R[ri - 2, rj - 1])).astype(F), (c[2] - gam(R[ri - 1, rj - 2])).astype(F))
        ax, sa = np.zeros(len(js), F), np.full(len(js), -1, np.int64)
        for k in (0, 1, 2):
            up = a[k] > ax
            ax, sa = np.where(up, a[k], ax), np.where(up, s[k], sa)
        q = np.zeros(N, F)
        sn = np.full(N, -1, np.int64)
        q[st:] = np.where(match, (mx + F(1)).astype(F), ax)
        sn[st:] = np.where(match, sm, sa)
        jm = int(np.argmax(q))                     # (the first maximum of the row)
        if q[jm] > best:
            best, end, start = q[jm], ri * N + (jm - o), int(sn[jm])
        q2, s2 = q1, s1
        q1, s1 = q, sn
    if end < 0:
        return NO_MATCH
    return (float(best), start // N, start % N, end // N, end % N)
