"""
The f64 reference of the opt-in Serra09 arithmetic arith = "f16x2" (tests/test_gpu_serra09_f16x2.py; its own proof on the CPU is
tests/test_serra09_f64_ref.py).  Importable without a GPU: numpy alone; the transposition index comes from the CPU oracle, through
the caller.

The f16x2 Gram is NOT the f32 arithmetic of the spec, so the oracle's plot cannot be its specification bit for bit.  What can be is
the plot of the f64 distances wherever a cell is DECIDED: where its distance, known within +-delta, lies on one side of every threshold
it meets, each of them known within the same +-delta.  `classify` finds those cells from the f64 matrix alone -- never from a
device's output -- so a device error cannot excuse itself by making a cell undecided.

DELTA_D2 is the envelope tests/test_gpu_serra09.py pins for this arithmetic on squared distances (profiles/r04_f16x2.md measured 1.83e-5
against f64); DELTA_PLOT doubles it: the second half covers the f32 root, the f32 interpolation weights and the squaring of the thresholds.
Both are in units of frame-max-normalised chroma (largest bin of a frame = 1), as all the shape sets are.
"""
import numpy as np

DELTA_D2 = 3e-5
DELTA_PLOT = 2 * DELTA_D2
KAPPA = 0.095
M_STACK = 9

# the undecided cells depend on the reference alone; these caps are conditions on the INPUTS (tests/test_serra09_f64_ref.py)
CAP_SET = 2e-4                  # of a whole shape set's cells
CAP_PAIR = 1e-3                 # of any pair of CAP_PAIR_CELLS cells or more
CAP_PAIR_CELLS = 10000

# log2 of the limits of the largest feature magnitude a pool may have under arith = "f16x2" (ensure_f16pool, acoss_amd/csrc/acx.hip);
# tests/test_serra09_f64_ref.py derives the lower one from split_f16, tests/test_gpu_serra09_f16x2.py holds the device to DELTA_D2 over it
RANGE_LOG2 = (-1, 15)


def embed(x, m, tau=1):
    """The delay embedding of a (T, 12) track: (M, 12 m) f64, stack i = frames (i + k) tau, k = 0 .. m - 1; M = ceil((T - m tau) / tau)
    (embed_full = 0, the default)."""
    x = np.asarray(x, np.float64)
    L = x.shape[0] - m * tau
    M = (L + tau - 1) // tau if L > 0 else 0
    assert M > 0, "track shorter than the stack"
    return np.concatenate([x[k * tau:k * tau + (M - 1) * tau + 1:tau] for k in range(m)], axis=1)


def d2_f64(query, reference, m, oti, tau=1):
    """(Mq, Mr) squared Euclidean distances of the two tracks' delay embeddings in f64, the reference rolled by the transposition
    index, clamped at 0."""
    X = embed(query, m, tau)
    Y = embed(np.roll(np.asarray(reference, np.float64), int(oti), axis=1), m, tau)
    d2 = (X * X).sum(1)[:, None] + (Y * Y).sum(1)[None, :] - 2.0 * (X @ Y.T)
    return np.maximum(d2, 0.0)


def percentiles(d, kappa):
    """(per row, per column) kappa-percentiles of a matrix of distances, linear interpolation (pct_mode 0), kappa as the f32 the
    parameter block carries."""
    q = 100.0 * float(np.float32(kappa))
    return np.percentile(d, q, axis=1), np.percentile(d, q, axis=0)


def classify(d2, kappa=KAPPA, delta=DELTA_PLOT):
    """Which cells of the plot are decided by the f64 matrix when squared distances are known within +-delta.

    lo = sqrt(max(d2 - delta, 0)) and hi = sqrt(d2 + delta) bound every distance; pct_mode 0 is a convex combination of two order
    statistics, which are monotone in every entry, so a threshold lies between the percentile of lo and the percentile of hi.
    A cell is surely 1 when hi <= the lo-percentile of its row AND of its column (inclusive comparison), surely 0 when lo > the
    hi-percentile of its row OR of its column; every other cell is undecided.

    Returns dict(one, zero: bool (Mq, Mr); q_lo, q_hi: (Mq,) row thresholds' bounds; r_lo, r_hi: (Mr,) column thresholds' bounds)."""
    d2 = np.asarray(d2, np.float64)
    lo = np.sqrt(np.maximum(d2 - delta, 0.0))
    hi = np.sqrt(d2 + delta)
    q_lo, r_lo = percentiles(lo, kappa)
    q_hi, r_hi = percentiles(hi, kappa)
    one = (hi <= q_lo[:, None]) & (hi <= r_lo[None, :])
    zero = (lo > q_hi[:, None]) | (lo > r_hi[None, :])
    return dict(one=one, zero=zero, q_lo=q_lo, q_hi=q_hi, r_lo=r_lo, r_hi=r_hi)


def split_f16(x):
    """The two-term split of the f16 operand pool (rotpool_f16_kernel): h1 = f16(x), h2 = f16(x - h1) with x in f32; returned as
    h1 + h2 in f64.  numpy's float16 rounds to nearest even and has subnormals, as the device's conversion and matrix pipe do."""
    x = np.asarray(x, np.float32)
    h1 = x.astype(np.float16)
    h2 = (x - h1.astype(np.float32)).astype(np.float16)
    return h1.astype(np.float64) + h2.astype(np.float64)


def split_error_2xy(query, reference, m, scale):
    """Largest representation error of 2 xy over a pair's cells when both tracks go through split_f16 scaled by `scale` (a power of
    two), in units of the unscaled features: max |2 X.Y - 2 X'.Y'| / scale^2, products and sums in f64."""
    s = np.float32(scale)
    X, Y = embed(query, m), embed(reference, m)
    Xs = embed(split_f16(np.asarray(query, np.float32) * s), m)
    Ys = embed(split_f16(np.asarray(reference, np.float32) * s), m)
    return float(np.max(np.abs(2.0 * (X @ Y.T) - 2.0 * (Xs @ Ys.T) / (float(s) * float(s)))))


def oti(query, reference):
    """The oracle's transposition index of a pair (oti_target 0: the reference is rolled by it), from the f32 global chroma of the two
    complete tracks -- the device takes it the same way (tests/test_gpu_serra09.py asserts that they agree)."""
    import ctypes
    import oracle
    L = oracle.lib()
    g = []
    for x in (query, reference):
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty(12, np.float32)
        L.acx_o_global_chroma(x.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), x.shape[0], out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        g.append(out)
    return int(L.acx_o_oti(g[0].ctypes.data_as(ctypes.POINTER(ctypes.c_float)), g[1].ctypes.data_as(ctypes.POINTER(ctypes.c_float))))


TAU2_CELLS = (505, 761, 2041)       # one row length per f16x2 family: band_kernel<M<=9, 2>, <M<=9, 4> (the unpacked middle class), <M<=9, 8>


def tau2_set(m=M_STACK, seed=0):
    """For the stack stride tau = 2 (the f16 operand pool is rebuilt from the decimated pool): per family one pair of the last row length
    of a class, versions of the START and the END of one chord work, T = frames_for(M, m, 2) frames each."""
    from tests import _serra09_shapes as S
    rng = np.random.default_rng([seed, m, 8])
    tracks, Ms, start, end, _ = S._two_ends(rng, TAU2_CELLS, m, 2)
    return S._pack(tracks, Ms, [(start[M], end[M]) for M in TAU2_CELLS], start=start, end=end)


def describe(d, k, tau=1):
    """The label of pair k of a shape set in failure messages, with the band kernel families arith = "f16x2" launches for it (the
    library's own plan, no device needed)."""
    from acoss_amd import _lib
    i, j = (int(x) for x in d["pairs"][k])
    T = np.diff(d["offsets"])
    rec = _lib.serra09_plan([T[i], T[j]], [[0, 1]], _lib.serra09_params(m=M_STACK, tau=tau, arith="f16x2"))[0]
    return "f16x2 m=%d tau=%d pair %d (tracks %d, %d) Mq=%d Mr=%d (cr, cq)=(%d, %d) row pass %s, column pass %s" % (
        M_STACK, tau, k, i, j, rec["Mq"], rec["Mr"], rec["cr"], rec["cq"], _lib.serra09_family_name(rec["row_family"], M_STACK),
        _lib.serra09_family_name(rec["col_family"], M_STACK))


def wrong_decided(R, c):
    """Coordinates (n, 2) of the decided cells of classification c on which the plot R falls on the wrong side."""
    R = np.asarray(R).astype(bool)
    return np.argwhere((c["one"] & ~R) | (c["zero"] & R))


def explain(d2, c, cell):
    """One wrong cell for a failure message: its d2, the bounds of its two thresholds and the side it fell on."""
    i, j = int(cell[0]), int(cell[1])
    return ("(row %d, column %d): d2 = %.9g (d = %.9g), row threshold in [%.9g, %.9g], column threshold in [%.9g, %.9g], the reference says %d, "
            "the plot says %d" % (i, j, d2[i, j], np.sqrt(d2[i, j]), c["q_lo"][i], c["q_hi"][i], c["r_lo"][j], c["r_hi"][j],
                                  int(c["one"][i, j]), int(not c["one"][i, j])))
