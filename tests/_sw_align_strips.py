"""
The EarlyFusion alignment (tests/_sw_align_ref.py states the contract) restated AS ef_align_long_kernel COMPUTES IT (DESIGN.md section
26), open to mutation, and the plots that tests/test_gpu_sw_align_long.py hands the kernel.  Importable without a GPU;
tests/test_sw_align_long_ref.py shows on the CPU that the restatement equals align_forward on every one of those plots and that each
mutant -- each way the kernel's strips, records, running best, reduction and code plane can go wrong -- changes the record or the
cells of at least one of them.

  strips        1024 columns (64 lanes x 16); every strip but the last leaves (U[i][c-1], U[i][c-2]) per row in a ring of two record
                buffers, and the next strip's first column reads l1a = U[i-1][c-1], l1b = U[i-1][c-2], l2a = U[i-2][c-1] from them
  codes         two bits per cell (0: T == 0, 1 / 2 / 3: the predecessor), 16 cells a word, a row of 64 words per strip; every word of
                rows 2 .. M-2 is written
  running best  per lane (T, row, column): replaced by a larger T, or by an equal T in an earlier row; within a row the smaller column
  reduction     the xor butterfly over 32 .. 1, comparing T, then row, then column; lane 0's triple is the end
  traceback     from the end along the codes while they are not 0, inside the counted rectangle, at most min(M, N) cells
"""
import numpy as np

from . import _ef_streaming_cases as cases
from . import _sw_align_ref as ref

STRIP, LANES, CPL = 1024, 64, 16
MUTANTS = ("swap", "drop2", "row", "ring", "tie_row", "reduce_col", "row10", "t16", "stale")


def plane_shape(M, N):
    return (M, LANES * ((N + STRIP - 1) // STRIP))


def align_strips(B, mutant=None, plane=None):
    """((score, q0, r0, q1, r1), cells (L, 2) int32, code plane (M, 64 * strips) uint32).  plane: the code plane as an earlier call
    left it (the kernel's buffer is reused); None: zeros.  mutant: None, or
      swap        the two fields of a record swapped
      drop2       the c-2 field of a record is 0
      row         l2a taken from row i-1's record
      ring        strip s >= 2 reads the records of strip s - 2 (a ring of two that does not alternate)
      tie_row     a lane keeps its record against an equal T in an earlier row
      reduce_col  the reduction compares T and row alone
      row10       the row of the running best kept in 10 bits
      t16         the value of the running best kept as 4 T in 16 bits
      stale       a code word that is 0 is not written"""
    assert mutant is None or mutant in MUTANTS
    B = np.asarray(B).astype(bool)
    M, N = B.shape
    if M < 4 or N < 4:
        return ref.NO_MATCH, np.zeros((0, 2), np.int32), plane
    nstrips = (N + STRIP - 1) // STRIP
    if plane is None:
        plane = np.zeros(plane_shape(M, N), np.uint32)
    assert plane.shape == plane_shape(M, N) and plane.dtype == np.uint32
    gap = np.where(B, 0, -7).astype(np.int64)
    hit = np.where(B, 10, -10).astype(np.int64)
    shifts = (2 * np.arange(CPL)).astype(np.uint32)
    bT, bRow, bCol = (np.zeros(LANES, np.int64) for _ in range(3))
    recs = []
    for st in range(nstrips):
        s0, s1 = st * STRIP, min(N, (st + 1) * STRIP)
        w = s1 - s0
        rin = None
        if st > 0:
            rin = recs[st - 2 if (mutant == "ring" and st >= 2) else st - 1]
            if mutant == "swap":
                rin = rin[:, ::-1]
        U = gap[:, s0:s1].copy()
        cols = s0 + np.arange(w)
        dead = (cols < 2) | (cols > N - 2)
        for i in range(2, M - 1):
            l1a = l1b = l2a = 0
            if rin is not None:
                l1a, l1b, l2a = rin[i - 1, 0], rin[i - 1, 1], rin[i - 2, 0]
                if mutant == "row":
                    l2a = rin[i - 1, 0]
                if mutant == "drop2":
                    l1b = 0
            c2 = np.concatenate([[l1a], U[i - 1, :-1]])
            c3 = np.concatenate([[l2a], U[i - 2, :-1]])
            c4 = np.concatenate([[l1b, l1a], U[i - 1, :-2]])[:w]
            mx, d = c2, np.ones(w, np.int64)
            m = c3 > mx
            mx, d = np.where(m, c3, mx), np.where(m, 2, d)
            m = c4 > mx
            mx, d = np.where(m, c4, mx), np.where(m, 3, d)
            T = np.maximum(0, hit[i, s0:s1] + mx)
            T[dead] = 0
            U[i] = T + gap[i, s0:s1]
            # the row's code words: one per lane, lanes right of the plot included
            code = np.zeros(STRIP, np.uint32)
            code[:w] = np.where(T > 0, d, 0)
            words = np.bitwise_or.reduce(code.reshape(LANES, CPL) << shifts, axis=1).astype(np.uint32)
            dst = plane[i, LANES * st:LANES * (st + 1)]
            if mutant == "stale":
                dst[words != 0] = words[words != 0]
            else:
                dst[:] = words
            # the lanes' running bests
            Tp = np.zeros(STRIP, np.int64)
            Tp[:w] = (4 * T) & 0xffff if mutant == "t16" else T
            Tp = Tp.reshape(LANES, CPL)
            rE = np.argmax(Tp, axis=1)                         # the first of equal values: the smaller column
            rT = Tp[np.arange(LANES), rE]
            take = rT > bT
            if mutant != "tie_row":
                take |= (rT == bT) & (rT > 0) & (i < bRow)
            bT = np.where(take, rT, bT)
            bRow = np.where(take, i & 1023 if mutant == "row10" else i, bRow)
            bCol = np.where(take, s0 + CPL * np.arange(LANES) + rE, bCol)
        if s1 < N:
            recs.append(np.stack([U[:, w - 1], U[:, w - 2]], 1))
    lanes = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        oT, oR, oC = bT[lanes ^ o], bRow[lanes ^ o], bCol[lanes ^ o]
        better = oR < bRow
        if mutant != "reduce_col":
            better |= (oR == bRow) & (oC < bCol)
        take = (oT > bT) | ((oT == bT) & better)
        bT, bRow, bCol = np.where(take, oT, bT), np.where(take, oR, bRow), np.where(take, oC, bCol)
    best, y, x = int(bT[0]), int(bRow[0]), int(bCol[0])
    if mutant == "t16":
        best //= 4
    if best <= 0:
        return ref.NO_MATCH, np.zeros((0, 2), np.int32), plane

    def code_at(yy, xx):
        return (int(plane[yy, xx >> 4]) >> (2 * (xx & 15))) & 3
    out = []
    end = (y, x)
    if 2 <= y <= M - 2 and 2 <= x <= N - 2:
        code = code_at(y, x)
        while code != 0 and len(out) < min(M, N):
            out.append((y, x))
            py, px = y - (2 if code == 2 else 1), x - (2 if code == 3 else 1)
            if py < 2 or px < 2:
                break
            code = code_at(py, px)
            if code != 0:
                y, x = py, px
    score = float(np.float32(best) / np.float32(10))
    if not out:
        return (score, -1, -1, -1, -1), np.zeros((0, 2), np.int32), plane
    return (score, y, x, end[0], end[1]), np.array(out[::-1], np.int32).reshape(-1, 2), plane


# ------------------------------------------------------------------------------------------------------------------
# the plots of tests/test_gpu_sw_align_long.py section a
# ------------------------------------------------------------------------------------------------------------------
def _plot(shape, ones):
    B = np.zeros(shape, np.uint8)
    for c in ones:
        B[c] = 1
    return B


def _diag(a, b, n=10):
    return [(a + k, b + k) for k in range(n)]


def small_plots():
    return [(name, B) for name, B, _, _ in ref.hand_checked()] + [("no_match_%dx%d_%d" % (B.shape + (int(B[0, 0]),)), B) for B in ref.no_match_plots()]


def planted_plots():
    """(name, plot, the planted cells where the path has no hole, else None)"""
    return [(name, B, None if "hole" in name else np.array(cells, np.int32)) for name, B, cells, _ in cases.planted_cases()]


def rim_plots():
    return [("rim_%s_%dx%d" % (kind, m, n), cases.rim_plot(kind, m, n)) for n in cases.RIM_N for m in cases.RIM_M for kind in cases.RIM_PLOTS]


def tie_plots():
    """(name, plot, the end that must be reported): two equal diagonals of ten ones (3, 13 .. 93 tenths) on zeros in 64 x 2100.
    `same_lane`: the second diagonal's end in the lane of the first one's, a strip further right -- the lane's own record decides."""
    shape = (64, 2100)
    return [("tie_late_strip0_early_strip1", _plot(shape, _diag(30, 100) + _diag(3, 1500)), (12, 1509)),
            ("tie_early_strip0_late_strip1", _plot(shape, _diag(3, 100) + _diag(30, 1500)), (12, 109)),
            ("tie_same_rows_two_strips", _plot(shape, _diag(20, 100) + _diag(20, 1500)), (29, 109)),
            ("tie_same_rows_lane_edge", _plot(shape, _diag(20, 100) + _diag(20, 120)), (29, 109)),
            ("tie_same_lane_late_then_early", _plot(shape, _diag(30, 100) + _diag(3, 1124)), (12, 1133)),
            ("tie_same_lane_early_then_late", _plot(shape, _diag(3, 100) + _diag(30, 1124)), (12, 109))]


def seam_pred_tie_plots():
    """(name, plot, cells): a cell in a strip's first column whose best predecessors are equal and all read from the seam record:
    (i-1, c-1) against (i-2, c-1), and (i-1, c-1) against (i-1, c-2); the first in order wins."""
    c = STRIP
    first_second = [(3, c - 2), (4, c - 1), (4, c - 2), (5, c - 1), (6, c)]                # U[5][c-1] = U[4][c-1] = 13
    first_third = [(3, c - 3), (4, c - 2), (3, c - 2), (4, c - 1), (5, c)]                 # U[4][c-1] = U[4][c-2] = 13
    return [("seam_pred_tie_1_2", _plot((12, c + 40), first_second), [(4, c - 2), (5, c - 1), (6, c)]),
            ("seam_pred_tie_1_3", _plot((12, c + 40), first_third), [(3, c - 2), (4, c - 1), (5, c)])]


def tall_plots():
    """(name, plot, end): rows beyond 1023."""
    rng = np.random.default_rng(1025)
    return [("tall_1025x8_ones", np.ones((1025, 8), np.uint8), None),
            ("tall_1025x8_random", (rng.random((1025, 8)) < 0.5).astype(np.uint8), None),
            ("tall_equal_maxima_rows_5_1030", _plot((2500, 30), _diag(2, 2, 4) + _diag(1027, 10, 4)), (5, 5)),
            ("tall_maximum_row_2400", _plot((2500, 30), _diag(2391, 5)), (2400, 14))]


def big_value_plots():
    """Values whose 4 T passes 16 bits (np.eye(3400): 33 970 tenths), and many strips of full rows."""
    return [("eye_3400", np.eye(3400, dtype=np.uint8)), ("ones_40x4100", np.ones((40, 4100), np.uint8))]


def stale_pair():
    """An all-ones plot and a sparse plot of the same shape: the second call's plane holds the first one's codes wherever the
    second does not write."""
    shape = (40, 1100)
    return np.ones(shape, np.uint8), _plot(shape, _diag(20, 500, 6) + _diag(10, 1060, 8))


def all_plots():
    """Every plot of section a as (name, plot)."""
    out = small_plots() + [(n, B) for n, B, _ in planted_plots()] + rim_plots() + [(n, B) for n, B, _ in tie_plots()]
    out += [(n, B) for n, B, _ in seam_pred_tie_plots()] + [(n, B) for n, B, _ in tall_plots()] + big_value_plots()
    return out + [("stale_%d" % k, B) for k, B in enumerate(stale_pair())]
