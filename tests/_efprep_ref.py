"""
An independent reference of the EarlyFusion block features (EarlyFusion.load_features with
resize_block, earlyfusion_traile.py:100-140, 214-247), numpy only, in np.longdouble.

It is NOT the device's loop (nor oracle.ef_resize's padding and convolution): the resize is written
as two explicit linear operators and a clip,

    resize(x, rows) = clip(L @ G @ x)

  G  (n x n)     the Toeplitz matrix of scipy.ndimage.gaussian_filter1d's documented weights:
                 sigma = max(0, (n / rows - 1) / 2), radius = int(4 sigma + 0.5),
                 G[t, j] = exp(-(j - t)^2 / (2 sigma^2)) / sum over ALL 2 radius + 1 taps for |j - t| <= radius,
                 0 elsewhere (mode='constant': what falls outside the block is dropped, the weights are not
                 renormalised).  No cap on the radius.
  L  (rows x n)  linear interpolation at (o + 0.5) n / rows - 0.5 with zero fill: the weight of a sample
                 outside [0, n) is dropped.
  clip           to [min, max] of the input block over all its columns (after NaN -> 0); results that are
                 exactly 0 stay 0 when 0 lies outside that range (skimage's preserved fill value);
                 non-finite results become 0.  (Along time alone the preserved fill value cannot show: every
                 output row puts a positive weight on at least one frame of the block, so a result is exactly 0
                 only when 0 lies in the block's range.  It is skimage's rule and is kept as that.)

Only the rows of G that L touches are ever materialised (two per output row), as dense vectors over the
band where they are non-zero; L @ G is the (rows x n) matrix the block is multiplied with.

On top: NaN -> 0 for the MFCCs, zero-mean columns, unit rows (zero norm: unscaled), the SSM as direct
differences sqrt(sum((x_r - x_c)^2)) for c < r in row-major order, the chroma block, np.median of the f32
chroma, and the pool's unit-norm chroma rows and squared row norms.  An empty block (i2 <= i1 after
numpy's clipping of the slice to the track) is all zeros: the device's and the oracle's convention.

Everything is returned UNROUNDED (np.longdouble); the tests round or bound as they need.
"""
import numpy as np

LD = np.longdouble


def radius(n, rows):
    """(sigma, radius) of the anti-aliasing filter for n frames -> rows rows; sigma as skimage computes it (f64)."""
    sigma = max(0.0, (float(n) / float(rows) - 1.0) / 2.0)
    return sigma, int(4.0 * sigma + 0.5)


def gaussian_weights(n, rows):
    """The 2 radius + 1 normalised taps (longdouble) of G's rows, and the radius."""
    sigma, r = radius(n, rows)
    if r == 0:
        return np.ones(1, LD), 0
    k = np.arange(-r, r + 1).astype(LD)
    w = np.exp(-(k * k) / (LD(2) * LD(sigma) * LD(sigma)))
    return w / w.sum(), r


def gaussian_row(t, n, w, r):
    """Row t of G as a dense n-vector: zero when t is no sample of the block."""
    g = np.zeros(n, LD)
    if 0 <= t < n:
        j0, j1 = max(0, t - r), min(n - 1, t + r)
        g[j0:j1 + 1] = w[j0 - t + r:j1 - t + r + 1]
    return g


def interpolation_matrix(n, rows):
    """L (rows x n) and, per output row, the (t0, f) it was built from."""
    L = np.zeros((rows, n), LD)
    taps = []
    for o in range(rows):
        pos = (LD(o) + LD(0.5)) * LD(n) / LD(rows) - LD(0.5)
        t0 = int(np.floor(pos))
        f = pos - LD(t0)
        taps.append((t0, f))
        if 0 <= t0 < n:
            L[o, t0] += LD(1) - f
        if 0 <= t0 + 1 < n:
            L[o, t0 + 1] += f
    return L, taps


def resize_operator(n, rows):
    """L @ G, (rows x n) longdouble."""
    w, r = gaussian_weights(n, rows)
    _, taps = interpolation_matrix(n, rows)
    M = np.zeros((rows, n), LD)
    for o, (t0, f) in enumerate(taps):
        M[o] = (LD(1) - f) * gaussian_row(t0, n, w, r) + f * gaussian_row(t0 + 1, n, w, r)
    return M


def _matmul(M, x):
    # longdouble has no BLAS: row by row over the band where the operator is non-zero
    out = np.zeros((M.shape[0], x.shape[1]), LD)
    for o in range(M.shape[0]):
        nz = np.nonzero(M[o])[0]
        if len(nz):
            a, b = nz[0], nz[-1] + 1
            out[o] = (M[o, a:b, None] * x[a:b]).sum(axis=0)
    return out


def resize(x, rows):
    """clip(L @ G @ x) of a block x (n, d) -> (rows, d), longdouble."""
    x = np.array(x, dtype=LD)
    x[np.isnan(x)] = 0
    n, d = x.shape
    if n == 0:
        return np.zeros((rows, d), LD)
    out = _matmul(resize_operator(n, rows), x)
    mn, mx = x.min(), x.max()
    zero = out == 0
    out = np.minimum(np.maximum(out, mn), mx)
    if not (mn <= 0 <= mx):
        out[zero] = 0
    out[~np.isfinite(out)] = 0
    return out


def spans(onsets, T, b, last):
    """Frames [i1, i2) of x[onsets[b]:onsets[last]] for a track of T frames, as numpy clips the slice; i2 <= i1: empty."""
    i1, i2 = int(onsets[b]), int(onsets[last])
    if i1 < 0 or i2 < 0:
        raise ValueError("negative onset")
    i1, i2 = min(i1, T), min(i2, T)
    return i1, max(i1, i2)


NOISE = LD(2.0) ** -40         # a centred row this far below the block's largest value is f64 rounding noise (2^-53 x 8192)


def mfcc_chain(blk, noise=None):
    """zero-mean columns, unit rows (zero norm unscaled), direct-difference SSM of a resized block (R, C).
    `noise` (a list) receives the rows that are mathematically 0 but not exactly: 0 < norm < NOISE x the block's largest
    value.  Scaling such a row to unit length scales rounding noise -- in f64 as here -- so it has no value to compare."""
    R = blk.shape[0]
    top = np.abs(blk).max()
    blk = blk - blk.sum(axis=0, keepdims=True) / LD(R)
    nrm = np.sqrt((blk * blk).sum(axis=1, keepdims=True))
    if noise is not None:
        noise.extend(int(r) for r in np.nonzero((nrm[:, 0] > 0) & (nrm[:, 0] < NOISE * top))[0])
    blk = blk / np.where(nrm == 0, LD(1), nrm)
    dlt = blk[:, None, :] - blk[None, :, :]
    rr, cc = np.tril_indices(R, -1)                  # (r, c) with c < r, row-major over r
    return blk, np.sqrt((dlt * dlt).sum(axis=2))[rr, cc]


def block_features(chroma, mfcc, onsets, blocksize=20, mfccs_per_block=50, chromas_per_block=40):
    """chroma (T, 12) f32, mfcc (T', ncoef) f32 time-major, onsets: dict of mfccs, ssms, chromas (longdouble,
    unrounded, one row per block), chroma_med (np.median of the f32 columns, as f64; NaN for a track of no frames) and
    noise_rows."""
    chroma = np.asarray(chroma, np.float32).reshape(-1, 12)
    mfcc = np.asarray(mfcc, np.float32)
    onsets = np.asarray(onsets, np.int64)
    C, R, Rc = mfcc.shape[1], int(mfccs_per_block), int(chromas_per_block)
    nb = max(0, len(onsets) - int(blocksize))
    out = dict(mfccs=np.zeros((nb, R * C), LD), ssms=np.zeros((nb, R * (R - 1) // 2), LD), chromas=np.zeros((nb, Rc * 12), LD),
               noise_rows=[])                    # (block, row) of the MFCC rows that are rounding noise (mfcc_chain)
    out["chroma_med"] = (np.median(chroma, axis=0) if len(chroma) else np.full(12, np.nan, np.float32)).astype(np.float64)
    for b in range(nb):
        i1, i2 = spans(onsets, len(mfcc), b, b + blocksize - 1)
        noise = []
        blk, ssm = mfcc_chain(resize(mfcc[i1:i2], R), noise)
        out["noise_rows"] += [(b, r) for r in noise]
        out["mfccs"][b], out["ssms"][b] = blk.ravel(), ssm
        i1, i2 = spans(onsets, len(chroma), b, b + blocksize)
        out["chromas"][b] = resize(chroma[i1:i2], Rc).ravel()
    return out


def pool_rows(feats):
    """What the pool holds of block features as the device returns them (f32): the unit-norm chroma rows
    (zero norm: the row stays 0) and the squared norms of the mfcc and ssm rows, all longdouble."""
    ch = np.asarray(feats["chromas"], np.float32).astype(LD)
    nrm = np.sqrt((ch * ch).sum(axis=1, keepdims=True))
    unit = ch / np.where(nrm == 0, LD(1), nrm)
    sq = [(np.asarray(feats[k], np.float32).astype(LD) ** 2).sum(axis=1) for k in ("mfccs", "ssms")]
    return unit, sq[0], sq[1]


# ---- the shapes where a resize can go wrong ----

MAXRAD = 512          # the widest Gaussian the device evaluates (EFP_MAXRAD)


def first_blurred(rows):
    """The first n with n / rows >= 1.25: the first block length at which the Gaussian has a radius."""
    return (5 * rows + 3) // 4


def rounded_up(rows):
    """The first n above 2 rows at which the + 0.5 decides the radius (4 sigma = 2 n / rows - 2 has a fraction >= 0.5), or
    None where there is none (one or two rows: 4 sigma is an integer).  At first_blurred the + 0.5 decides too, but the
    taps it adds weigh exp(-32): nothing an f32 result shows."""
    for n in range(2 * rows + 1, 4 * rows + 4):
        if 2 * ((2 * n) % rows) >= rows:
            return n
    return None


def edge_lengths(rows):
    """Block lengths for a resize to `rows` rows: degenerate blocks, around factor 1, the first radius, a radius that the
    + 0.5 rounds up, the largest radius the device holds (257 rows: r = 512), an ordinary 20-beat block of 1100 frames."""
    ns = [0, 1, 2, rows - 1, rows, rows + 1, first_blurred(rows) - 1, first_blurred(rows), rounded_up(rows), 257 * rows, 1100]
    return sorted(set(n for n in ns if n is not None and n >= 0))


FAMILIES = ("positive", "negative", "with_zero", "straddling")


def family(rng, name, n, d):
    """(n, d) f32 data: all-positive (the fill rule is active), all-negative, non-negative with an exact 0, straddling 0."""
    x = (rng.random((n, d)) * 0.9 + 0.05).astype(np.float32)
    if name == "negative":
        x = -x
    elif name == "with_zero" and n:
        x[rng.integers(n), rng.integers(d)] = 0.0
    elif name == "straddling":
        x = (x - np.float32(0.5)).astype(np.float32)
    return x


# ---- bounds (f32 results of f64-or-better arithmetic rounded once) ----

def ulp32(want):
    """The f32 ulp at max(|want|, 2^-126), elementwise, as longdouble."""
    a = np.maximum(np.abs(np.asarray(want, LD)), LD(2.0) ** -126)
    e = np.floor(np.log2(a))
    e = np.where(LD(2.0) ** e > a, e - 1, e)          # (log2 of a longdouble may round up at a power of two)
    e = np.where(LD(2.0) ** (e + 1) <= a, e + 1, e)
    return LD(2.0) ** (np.maximum(e, -126) - 23)


F64_ORDER = LD(1e-12)          # the allowance for another f64 summation order (measured reference against reference)


def bound_rounded(want):
    """|got - want| for a value computed in f64 or better and rounded once to f32."""
    return ulp32(want) / 2 + F64_ORDER


def bound_ssm(want, ncoef):
    """The device takes the Gram form |x_r|^2 + |x_c|^2 - 2 x_r.x_c on unit rows and clamps it at 0: its f64
    rounding error in d^2 is at most e = 4 (2 ncoef + 4) 2^-53, which is min(sqrt(e), e / (2 want)) in d."""
    want = np.asarray(want, LD)
    e = LD(4 * (2 * ncoef + 4)) * LD(2.0) ** -53
    with np.errstate(divide="ignore"):
        gram = np.minimum(np.sqrt(e), e / (2 * want))
    return ulp32(want) / 2 + gram + F64_ORDER
