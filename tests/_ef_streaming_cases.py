"""
Case builders for tests/test_gpu_ef_streaming.py: the inputs that hold EarlyFusion's streaming kernels (tracks of more than 1024
blocks: ef_rowstat_long_kernel, sw_long_kernel) per cell.  Importable without a GPU; tests/test_ef_streaming_design.py shows on the
CPU that the inputs can see what they are built for -- the hand-over between the 1024-column strips of sw_long_kernel (strip-wise
restatements of ref.sw_tenths with a broken record), the tie search's group edges, and the two summation orders of the
neighbourhood mean.
"""
import numpy as np

from . import _ef_backend_ref as ref
from .test_gpu_ef_backend import SHORT, WIDE, _pool, _product_probes

STRIP = 1024                               # columns of one strip of sw_long_kernel (64 lanes x 16)
SEAMS = (1024, 2048, 3072)
STEPS = {"diag": (1, 1), "wide": (1, 2), "tall": (2, 1)}        # (rows, columns) of the step INTO the target column
FIELD_OF_STEP = {"diag": "l1a", "wide": "l1b", "tall": "l2a"}   # what lane 0 reads for a step into a strip's first column
PRE, POST = 22, 22                         # cells of a planted path in front of / from the target column on


# ------------------------------------------------------------------------------------------------------------------
# A. sw_long_kernel: ref.sw_tenths in strips, the record between two strips open to mutation
# ------------------------------------------------------------------------------------------------------------------
MUTANTS = ("edge", "swap", "row", "drop2", "ring")             # (a) .. (e) of the design test
FIELDS = ("l1a", "l1b", "l2a")


def sw_strips(B, mutant=None, width=STRIP, records=None):
    """ref.sw_tenths computed as sw_long_kernel does: strips of `width` columns, every strip but the last leaving
    (U[i][c-1], U[i][c-2]) per row (c: the next strip's first column); the next strip's first column reads l1a = U[i-1][c-1],
    l1b = U[i-1][c-2] and l2a = U[i-2][c-1] from them, its second column l1a.  mutant: None, or
      edge   every strip's first two columns are the matrix edge (T = 0)
      swap   the two fields of a record swapped
      row    l2a taken from row i-1's record
      drop2  the c-2 field is 0
      ring   strip s >= 2 reads the records of strip s - 2 (a ring of two that does not alternate)
      l1a / l1b / l2a   that one value lost (the floor, -7)
    records: a list that receives every strip's (M, 2) record array."""
    B = np.asarray(B).astype(bool)
    M, N = B.shape
    if M < 4 or N < 4:
        return 0
    gap = np.where(B, 0, -7).astype(np.int64)
    hit = np.where(B, 10, -10).astype(np.int64)
    recs, best = [], 0
    for st in range((N + width - 1) // width):
        s0, s1 = st * width, min(N, (st + 1) * width)
        w = s1 - s0
        rin = None
        if st > 0:
            rin = recs[st - 2 if (mutant == "ring" and st >= 2) else st - 1]
            if mutant == "swap":
                rin = rin[:, ::-1]
        U = gap[:, s0:s1].copy()
        cols = s0 + np.arange(w)
        for i in range(2, M - 1):
            l1a = l1b = l2a = 0
            if rin is not None:
                l1a, l1b, l2a = rin[i - 1, 0], rin[i - 1, 1], rin[i - 2, 0]
                if mutant == "row":
                    l2a = rin[i - 1, 0]
                if mutant == "drop2":
                    l1b = 0
                if mutant == "l1a":
                    l1a = -7
                if mutant == "l1b":
                    l1b = -7
                if mutant == "l2a":
                    l2a = -7
            c2 = np.concatenate([[l1a], U[i - 1, :-1]])
            c3 = np.concatenate([[l2a], U[i - 2, :-1]])
            c4 = np.concatenate([[l1b, l1a], U[i - 1, :-2]])[:w]
            T = np.maximum(0, hit[i, s0:s1] + np.maximum(np.maximum(c2, c3), c4))
            T[cols < 2] = 0
            if mutant == "edge" and st > 0:
                T[:2] = 0
            seen = T[cols <= N - 2]
            if seen.size:
                best = max(best, int(seen.max()))
            U[i] = T + gap[i, s0:s1]
        if s1 < N:
            recs.append(np.stack([U[:, w - 1], U[:, w - 2]], 1))
    if records is not None:
        records.extend(recs)
    return best


def planted_path(seam, into, step, odd, gaps=(), rows=64):
    """A path of ones on zeros whose only best continuation enters column seam + into by `step` (STEPS), the entering cell in an
    even / odd row: PRE cells on a diagonal up to the step, POST cells on a diagonal from it.  gaps: columns whose path cell is
    taken out again (the alignment runs on through the hole, penalised).  Returns (B, cells of the intact path)."""
    ct = seam + into
    ie = 26 + (1 if odd else 0)
    di, dj = STEPS[step]
    B = np.zeros((rows, seam + 40), np.uint8)
    cells = [(ie - di - k, ct - dj - k) for k in range(PRE - 1, -1, -1)] + [(ie + k, ct + k) for k in range(POST)]
    for (i, j) in cells:
        assert 2 <= i <= rows - 2 and 2 <= j <= B.shape[1] - 2
        if j not in gaps:
            B[i, j] = 1
    return B, cells


def planted_cases():
    """(name, B, intact cells, field): every seam, both first columns of a strip, the three steps, both row parities -- `field`
    names the record value the step reads (a step into the strip's second column reads the record only when it is two columns
    wide: l1a) -- and the diagonal with holes at and astride the seam."""
    out = []
    for seam in SEAMS:
        for odd in (0, 1):
            for into in (0, 1):
                for step in STEPS:
                    field = FIELD_OF_STEP[step] if into == 0 else ("l1a" if step == "wide" else None)
                    B, cells = planted_path(seam, into, step, odd)
                    out.append(("seam%d_col%d_%s_%s" % (seam, into, step, "odd" if odd else "even"), B, cells, field))
            for gaps in ((seam - 2,), (seam - 1,), (seam,), (seam + 1,), (seam - 1, seam)):
                B, cells = planted_path(seam, 0, "diag", odd, gaps)
                out.append(("seam%d_hole%s_%s" % (seam, "_".join(str(g - seam) for g in gaps), "odd" if odd else "even"), B, cells, None))
    return out


RIM_N = (1025, 1026, 1027, 2047, 2048, 2049, 2050, 3073, 4097, 5121)
RIM_M = (4, 5, 6, 64)
RIM_PLOTS = ("ones", "zeros", "random30", "random80")


def rim_plot(kind, m, n):
    if kind == "ones":
        return np.ones((m, n), np.uint8)
    if kind == "zeros":
        return np.zeros((m, n), np.uint8)
    rng = np.random.default_rng([m, n, int(kind[6:])])
    return (rng.random((m, n)) < int(kind[6:]) / 100.0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------
# B. ef_rowstat_long_kernel: rows whose threshold has surplus ties, the tie column at the edges of the 64-column groups
# ------------------------------------------------------------------------------------------------------------------
LONG_N = (1025, 1087, 1088, 1089, 2047, 2048, 2049, 2500)
LONG_M = (1, 2, 5, 9)
TALL_M = 1025
TALL_N = (1, 4, 5, 64, 105, 106, 257, 512, 513, 1024)
LONG_K = (1, 10, 16)
TIE_N = (1025, 1087, 2500)
TIE_KB = (40, 0.1)                         # kappa: a count, and a share of the row
TIE_VALUE = np.float32(0.5)


def tie_placements(n):
    """(label, tie column, surplus ties behind it) of the rows of tie_matrix.  The kernel counts ties per group of 64 columns; the
    tie column -- the budget-th cell equal to t in column order -- stands at lane 0 and at lane 63 of the first and of a middle
    group and at lane 0 of the partial last group; in the last column that can hold one (N - 2: the one surplus tie behind it in
    N - 1); `exact_*`: no surplus at all (eq == budget, the last tie in column N - 1 / in mid row): jcut = JCUT_ALL."""
    last = (n - 1) // 64
    mid = last // 2
    rows = [("first_lane0", 0, 3), ("first_lane63", 63, 70), ("mid_lane0", 64 * mid, 1), ("mid_lane63", 64 * mid + 63, 5)]
    if 64 * last < n - 1:
        rows.append(("last_lane0", 64 * last, 1))
    rows += [("before_last_column", n - 2, 1), ("exact_last_column", n - 1, 0), ("exact_mid", 64 * mid + 17, 0)]
    return rows


def tie_matrix(n, kb, seed=5):
    """(C, labels, tie columns): one row per placement of tie_placements and an all-equal row.  A row holds kb - budget distinct
    cells below TIE_VALUE, budget + surplus cells equal to it -- budget - 1 of them at most 100 columns in front of the tie column,
    so that the tie column's group and the one before it hold several -- and distinct larger cells."""
    rng = np.random.default_rng([n, kb, seed])
    places = tie_placements(n)
    C = np.empty((len(places) + 1, n), np.float32)
    want = []
    for k, (label, col, surplus) in enumerate(places):
        budget = min(kb, col + 1, 2 + (7 * k) % 23)
        before = rng.choice(np.arange(max(0, col - 100), col), budget - 1, replace=False) if budget > 1 else np.zeros(0, np.int64)
        behind = rng.choice(np.arange(col + 1, n), surplus, replace=False) if surplus else np.zeros(0, np.int64)
        ties = np.concatenate([before, [col], behind]).astype(np.int64)
        rest = np.setdiff1d(np.arange(n), ties)
        rest = rest[rng.permutation(len(rest))]
        nlt = kb - budget
        row = np.empty(n, np.float32)
        row[ties] = TIE_VALUE
        row[rest[:nlt]] = (0.01 + 0.4 * (1 + np.arange(nlt)) / (nlt + 1)).astype(np.float32)
        row[rest[nlt:]] = (0.6 + (1 + np.arange(len(rest) - nlt)) / float(n)).astype(np.float32)
        C[k] = row
        want.append(col if surplus else ref.JCUT_ALL)
    C[-1] = TIE_VALUE
    want.append(kb - 1)
    return C, [p[0] for p in places] + ["all_equal"], np.array(want, np.int64)


# ------------------------------------------------------------------------------------------------------------------
# C. the product path with tracks of more than 1024 blocks
# ------------------------------------------------------------------------------------------------------------------
LONG_BLOCKS = [3, 17, 257, 512, 1024, 1025, 1100]
LONG_PROBES = [(1025, 1100), (1100, 1025), (1100, 17), (17, 1100), (3, 1025), (1025, 3), (1024, 1025), (1025, 1024), (512, 1025),
               (1025, 512)]
# (into track, its blocks) <- (from track, its blocks): as the SECOND track of its pair the section crosses block 1024
PLANTS = [((1025, 985, 1025), (1100, 200, 240)), ((1100, 1000, 1050), (1025, 930, 980))]
LONG_CONFIGS = [("fast", "default", 10), ("exact", "default", 10), ("fast", "bf16x3", 10), ("exact", "bf16x3", 10),
                ("fast", "default", 16), ("fast", "default", 17), ("fast", "default", 25)]


def long_pool(seed=91):
    """Tracks of LONG_BLOCKS; the pair of 1025 and 1100 blocks shares a section in each orientation (PLANTS)."""
    tracks = _pool(LONG_BLOCKS, seed)
    for k, ((into, a0, a1), (frm, b0, b1)) in enumerate(PLANTS):
        rng = np.random.default_rng([seed, k])
        dst, src = tracks[LONG_BLOCKS.index(into)], tracks[LONG_BLOCKS.index(frm)]
        for key in ("mfccs", "ssms", "chromas"):
            dst[key][a0:a1] = src[key][b0:b1] + 0.02 * rng.standard_normal((a1 - a0, src[key].shape[1])).astype(np.float32)
    return tracks


def long_probe_list():
    """The probe pairs as one sorted list of track indices, and every probe's place in it."""
    pairs = sorted((LONG_BLOCKS.index(m), LONG_BLOCKS.index(n)) for (m, n) in LONG_PROBES)
    return np.array(pairs, np.int32), {(LONG_BLOCKS[a], LONG_BLOCKS[b]): k for k, (a, b) in enumerate(pairs)}


# ------------------------------------------------------------------------------------------------------------------
# D. batch composition
# ------------------------------------------------------------------------------------------------------------------
BATCH_N = (60, 300, 513, 1000)
BATCH_M = 64
BATCH_K = (10, 16)
MIXED_BLOCKS = SHORT + WIDE + [1025]


def batch_matrix(n):
    """The caller's matrix of D: BATCH_M uniform rows."""
    return np.random.default_rng([n, 41]).random((BATCH_M, n)).astype(np.float32)


def tall_matrix(C):
    """C as the first rows of a matrix of 1025 rows: ef_rowstat_long_kernel runs on every row of it."""
    rest = np.random.default_rng([C.shape[1], 42]).random((TALL_M - C.shape[0], C.shape[1])).astype(np.float32)
    return np.concatenate([C, rest])


def _below(X, vk):
    X = np.asarray(X, np.float32)
    return np.where(X < np.asarray(vk, np.float32)[:, None], X, np.float32(0.0)).astype(np.float32)


def kth_smallest(X, K):
    kk = min(int(K), X.shape[1])
    return np.partition(np.asarray(X, np.float32), kk - 1, axis=1)[:, kk - 1]


def sum_register_order(X, vk):
    """Sum of the cells below vk per row, in f32, in the order of the register kernels (mean_k_smallest + ef_wave_sum_f): lane l
    adds columns 256 q + 4 l + e (q, then e); lanes 1, 2, 4 and 8 apart (the last two as mirrored half rows / rows of 16 lanes),
    then (r0 + r1) + (r2 + r3)."""
    Z = _below(X, vk)
    rows, n = Z.shape
    nq = (n + 255) // 256
    P = np.zeros((rows, nq * 256), np.float32)
    P[:, :n] = Z
    P = P.reshape(rows, nq, 64, 4)
    acc = np.zeros((rows, 64), np.float32)
    for q in range(nq):
        for e in range(4):
            acc = acc + P[:, q, :, e]
    lanes = np.arange(64)
    for partner in (lanes ^ 1, lanes ^ 2, (lanes & ~7) | (7 - (lanes & 7)), (lanes & ~15) | (15 - (lanes & 15))):
        acc = acc + acc[:, partner]
    assert acc.dtype == np.float32
    return (acc[:, 0] + acc[:, 16]) + (acc[:, 32] + acc[:, 48])


def sum_stream_order(X, vk):
    """The same sum in the order ef_rowstat_long_kernel had: lane l adds columns l, l + 64, ...; an xor butterfly over 32 .. 1."""
    Z = _below(X, vk)
    rows, n = Z.shape
    ng = (n + 63) // 64
    P = np.zeros((rows, ng * 64), np.float32)
    P[:, :n] = Z
    P = P.reshape(rows, ng, 64)
    acc = np.zeros((rows, 64), np.float32)
    for g in range(ng):
        acc = acc + P[:, g, :]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ o]
    assert acc.dtype == np.float32
    return acc[:, 0]


def mixed_lists():
    """The probe pairs of the SHORT + WIDE pool (i) alone, (ii) with a pair (1025, 257) -- long rows only -- and (iii) with a pair
    (257, 1025) -- long columns too -- as sorted lists over the pool of MIXED_BLOCKS, and the probes' places in each."""
    blocks = SHORT + WIDE
    probes = _product_probes(blocks, lambda m, n: True)
    L, s = len(blocks), blocks.index(257)
    out = {}
    for name, extra in (("alone", []), ("long_rows", [(L, s)]), ("long_cols", [(s, L)])):
        pairs = sorted(probes + extra)
        out[name] = (np.array(pairs, np.int32), [pairs.index(p) for p in probes])
    return probes, out
