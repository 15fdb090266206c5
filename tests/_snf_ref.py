"""
The specification of the similarity-network-fusion kernels (acoss_amd/csrc/snf_kernels.hpp): one numpy function per kernel,
in the operation order the kernel states, sums in np.longdouble (64-bit mantissa on x86).  tests/test_snf_ref.py pins these
functions to the oracle on the CPU and shows that the crafted inputs below tell them from seven wrong variants;
tests/test_gpu_snf_stages.py holds the device's stages against them.

Where a kernel's result is exact (S, the argument of the exponential, J) the function returns f64; where the kernel sums in
an order of its own the function returns longdouble and a `*_bound` beside it says how far an f64 sum may lie from it.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53                      # unit roundoff of f64
TIE_COLUMNS = list(range(60, 71)) + list(range(124, 133))       # across the 64-column ballot groups of snf_knn_kernel


# ------------------------------------------------------------------ one function per kernel

def sym(D):
    """snf_sym_kernel: 0.5 (D + D^T), zero diagonal.  One addition and an exact halving per cell: bit-identical."""
    S = 0.5 * (D + D.T)
    np.fill_diagonal(S, 0.0)
    return S


def take_of(n, K):
    return min(K + 1, n)


def localscale(S, K, skip_diagonal=False, drop_factor=False):
    """snf_localscale_kernel: the mean of the take = min(K + 1, n) smallest cells of a row (the zero diagonal is one of the
    cells) times (K + 1) / K.  Returns (md longdouble (n,), bound (n,)): an f64 evaluation in any order lies within
    (take + 3) 2^-53 (K + 1) / K mean(|the take cells|) -- take - 1 additions, the (take - below) t term, two divisions, one product.
    skip_diagonal / drop_factor: two of the wrong variants of tests/test_snf_ref.py."""
    n = S.shape[0]
    take = take_of(n, K)
    M = S
    if skip_diagonal and n > 1:
        M = S[~np.eye(n, dtype=bool)].reshape(n, n - 1)
        take = min(take, n - 1)
    cells = np.sort(M, 1)[:, :take]
    f = LD(1) if drop_factor else LD(K + 1) / LD(K)
    md = cells.astype(LD).sum(1) / LD(take) * f
    bound = (take + 3) * U * (K + 1) / K * np.abs(cells).mean(1)
    return md, bound


def affinity_arg(S, md, mu=0.5):
    """The argument of the exponential of snf_affinity_kernel, operation for operation (-ffp-contract=off: the same f64
    operations as numpy's): eps = (md_i + md_j + d) / 3, den = 2 (mu eps) (mu eps) with 0 -> 1, -(d d) / den."""
    md = np.asarray(md, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        eps = (md[:, None] + md[None, :] + S) / 3.0
        me = mu * eps
        den = 2.0 * me * me
        den[den == 0.0] = 1.0
        return -(S * S) / den


def affinity(S, md, mu=0.5):
    """snf_affinity_kernel with libm's exp."""
    with np.errstate(invalid="ignore", under="ignore"):
        return np.exp(affinity_arg(S, md, mu))


def knn(W, K, tie_last=False, shift=0):
    """snf_knn_kernel: J = stable descending argsort of the row cut at K; V = v / sum (sum 0 -> 1).  Returns (J int32 (n, K),
    V longdouble (n, K), rel (n,)): an f64 V lies within rel * |V|, rel = (K + 1) 2^-53 sum|v| / |sum v| -- K - 1 additions in
    any order and a division; (K + 1) 2^-53 where all terms are >= 0.
    tie_last: among equal values the LAST column ranks first; shift: the cut `shift` ranks up (wrong variants)."""
    n = W.shape[0]
    if tie_last:
        order = (n - 1 - np.argsort(-W[:, ::-1], 1, kind="stable"))
    else:
        order = np.argsort(-W, 1, kind="stable")
    J = order[:, shift:shift + K]
    v = np.take_along_axis(W, J, 1)
    s = v.astype(LD).sum(1)
    sa = np.abs(v).astype(LD).sum(1)
    rel = np.where(s == 0, 1.0, (sa / np.where(s == 0, LD(1), np.abs(s))).astype(np.float64)) * (K + 1) * U
    s[s == 0] = 1
    return J.astype(np.int32), v / s[:, None], rel


def rownorm(W):
    """snf_rownorm_kernel: P = W / rowsum (0 -> 1).  Returns (P longdouble, rel (n,)): an f64 P lies within rel * |P|,
    rel = (n + 1) 2^-53 sum|row| / |rowsum| -- n - 1 additions in the kernel's tree order and a division."""
    n = W.shape[0]
    s = W.astype(LD).sum(1)
    sa = np.abs(W).astype(LD).sum(1)
    rel = np.where(s == 0, 1.0, (sa / np.where(s == 0, LD(1), np.abs(s))).astype(np.float64)) * (n + 1) * U
    s[s == 0] = 1
    return W / s[:, None], rel


def mean(srcs, scale):
    """snf_mean_kernel: (sum over k in order) * scale.  Returns (acc longdouble, bound): (m + 1) 2^-53 sum|src_k| |scale|."""
    acc = np.zeros(srcs[0].shape, LD)
    ab = np.zeros(srcs[0].shape)
    for A in srcs:
        acc += A
        ab += np.abs(A)
    return acc * LD(scale), (len(srcs) + 1) * U * ab * abs(scale)


def ast(A, J, V):
    """snf_ast_kernel: UT[j][i] = sum_k V[i][k] A[j][J[i][k]] for the rows j of A given.  Returns (UT longdouble, bound):
    (K + 2) 2^-53 sum_k |V a| -- a product and at most K - 1 additions per term, two roundings to spare."""
    K = J.shape[1]
    ut = np.zeros((A.shape[0], J.shape[0]), LD)
    ab = np.zeros((A.shape[0], J.shape[0]))
    for k in range(K):
        a = A[:, J[:, k]]
        ut += V[:, k].astype(LD)[None, :] * a
        ab += np.abs(V[:, k])[None, :] * np.abs(a)
    return ut, (K + 2) * U * ab


def sut(UT, J, V, reg_diag=0.0, rows=None):
    """snf_sut_kernel: P[i][c] = sum_k V[i][k] UT[J[i][k]][c] (+ reg_diag at c == i) for the rows i asked for (default all).
    Returns (P longdouble, bound): (K + 2) 2^-53 sum_k |V ut|, plus one rounding of the result on the diagonal when reg_diag != 0."""
    n, K = J.shape
    rows = np.arange(n) if rows is None else np.asarray(rows)
    p = np.zeros((len(rows), n), LD)
    ab = np.zeros((len(rows), n))
    for k in range(K):
        u = UT[J[rows, k], :]
        p += V[rows, k].astype(LD)[:, None] * u
        ab += np.abs(V[rows, k])[:, None] * np.abs(u)
    bound = (K + 2) * U * ab
    if reg_diag != 0:
        p[np.arange(len(rows)), rows] += LD(reg_diag)
        bound[np.arange(len(rows)), rows] += U * np.abs(p[np.arange(len(rows)), rows]).astype(np.float64)
    return p, bound


def update_cells(A, J, V, reg_diag, rows, cols=None):
    """One update on a few rows straight from A = the mean (n, n), without the n x n UT: P[i][c] = sum_k V[i][k] sum_k' V[c][k']
    A[J[i][k]][J[c][k']] -- K^2 gathers per cell.  Returns (P longdouble (len(rows), n), bound).  The device rounds UT to f64
    in between: |UT_dev - UT| <= (K + 2) u sum|V a|, and the second product adds (K + 2) u sum|V UT_dev|, together
    (2 K + 5) 2^-53 sum_k sum_k' |V V a| (the 5th rounding covers the second-order term), plus the diagonal's rounding."""
    n, K = J.shape
    rows = np.asarray(rows)
    p = np.zeros((len(rows), n), LD)
    ab = np.zeros((len(rows), n))
    for k in range(K):
        a_rows = A[J[rows, k], :]                                  # (R, n): row J[i][k] of A
        for k2 in range(K):
            a = a_rows[:, J[:, k2]]                                # (R, n): A[J[i][k]][J[c][k2]]
            w = V[rows, k].astype(LD)[:, None] * V[:, k2].astype(LD)[None, :]
            p += w * a
            ab += np.abs(w.astype(np.float64) * a)
    bound = (2 * K + 5) * U * ab
    if reg_diag != 0:
        p[np.arange(len(rows)), rows] += LD(reg_diag)
        bound[np.arange(len(rows)), rows] += U * np.abs(p[np.arange(len(rows)), rows]).astype(np.float64)
    return p, bound


# ------------------------------------------------------------------ the stages composed: doSimilarityFusion

def f64(x):
    return np.asarray(x, dtype=np.float64)


def fuse(Ds, K, niters, reg_diag, mu=0.5, wrong=None):
    """acx_snf_fuse_dists from the stage functions, every stage rounded to f64 as the device stores it, the two work lists
    aliasing from the second sweep on as in snf_loop.  Defined for K = n - 1 and K = n, where oracle.snf_getW raises.
    Returns (Ws, fused).  wrong: None or one of WRONG_VARIANTS."""
    m = len(Ds)
    Ws, Js, Vs, cur = [], [], [], []
    for D in Ds:
        S = sym(f64(D))
        md = f64(localscale(S, K, skip_diagonal=wrong == "diagonal_excluded", drop_factor=wrong == "factor_dropped")[0])
        W = affinity(S, md, mu)
        J, V, _ = knn(W, K, tie_last=wrong == "tie_last", shift=1 if wrong == "cut_one_up" and K < W.shape[0] else 0)
        Ws.append(W); Js.append(J); Vs.append(f64(V)); cur.append(f64(rownorm(W)[0]))
    nxt = [None] * m
    for it in range(niters):
        src = cur if it == 0 else nxt
        for i in range(m):
            others = [src[k] for k in range(m) if k != i or wrong == "mean_over_all"]
            scale = 1.0 / (m if wrong == "mean_over_all" else m - 1)
            nxt[i] = update(others, scale, Js[i], Vs[i], reg_diag, wrong)
    return Ws, f64(mean(nxt, 1.0 / m)[0])


def update(srcs, scale, J, V, reg_diag, wrong=None):
    """One update as acx_snf_debug_update runs it, every stage rounded to f64: the new P (n, n)."""
    n = J.shape[0]
    acc = f64(mean(srcs, scale)[0])
    ut = f64(ast(acc, J, V)[0])
    if wrong == "transposed_S":                 # S^T for S in the second product
        Sd = np.zeros((n, n), LD)
        np.add.at(Sd, (np.repeat(np.arange(n), J.shape[1]), J.ravel()), V.ravel().astype(LD))
        p = f64(Sd.T.dot(ut.astype(LD)))
        p[np.arange(n), np.arange(n)] += reg_diag
        return p
    if wrong == "reg_off_diagonal":             # reg_diag on the diagonal of the TRANSPOSED matrix: it ends up as reg * S, off the diagonal
        ut = ut.copy()
        ut[np.arange(n), np.arange(n)] += reg_diag
        return f64(sut(ut, J, V, 0.0)[0])
    return f64(sut(ut, J, V, reg_diag)[0])


WRONG_VARIANTS = ("tie_last", "cut_one_up", "diagonal_excluded", "factor_dropped", "mean_over_all", "transposed_S", "reg_off_diagonal")


# ------------------------------------------------------------------ crafted inputs

def crafted_distances(n, seed=0):
    """A non-symmetric (n, n) distance matrix with a non-zero diagonal whose SYMMETRISED rows are: random; duplicates (distance 0
    to several columns, few distinct values: ties at the cut); negative entries with -0.0 beside +0.0; all equal.  The crafted rows
    hold multiples of 2^-6 split as p + a, p - a with a a multiple of 2^-6 too, so that 0.5 (D + D^T) gives p exactly."""
    rng = np.random.default_rng(1000 * n + seed)
    D = rng.random((n, n)) * 3 + 0.01
    q = 1.0 / 64

    def put(i, pattern):
        a = rng.integers(-32, 33, n) * q
        zero = pattern == 0
        D[i, :] = np.where(zero, pattern, pattern + a)          # a signed zero on both sides: -0.0 + -0.0 stays -0.0
        D[:, i] = np.where(zero, pattern, pattern - a)
        D[i, i] = 1.0 + i                        # the kernel zeroes it

    for i in range(n):
        f = i % 8
        if f == 1:
            put(i, rng.integers(0, 3, n) * (16 * q))
        elif f == 3:
            p = rng.integers(-128, 129, n) * q
            p[rng.random(n) < 0.2] = -0.0
            p[rng.random(n) < 0.2] = 0.0
            put(i, p)
        elif f == 5:
            put(i, np.full(n, 48 * q))
        elif f == 7:
            p = rng.integers(0, 2, n) * (8 * q)                 # distance 0 to about half of the columns
            put(i, p)
    return D


NEQ_TARGETS = (2, 4, 5, 13, 15, 16)       # neq_left runs out mid-group, at a group's last column, at the next group's first: both tie runs


def crafted_affinity(n, K, seed=0):
    """An (n, n) matrix of affinity rows for from_stage = 1, one family per way the selection of snf_knn_kernel can exit; row r
    holds family r mod len(families) with its own random part.  Returns (W, names): names[r] is the family of row r."""
    rng = np.random.default_rng(7919 * n + 31 * K + seed)
    tie_cols = np.array([c for c in TIE_COLUMNS if c < n])
    free = np.setdiff1d(np.arange(n), tie_cols)
    last0 = ((n - 1) // 64) * 64                  # first column of the last ballot group

    def ties(target):
        # `ngt` cells above the tie value, the tie value in TIE_COLUMNS, the rest below: neq_left = K - ngt = target (where K allows)
        row = rng.random(n) * 0.25
        row[tie_cols] = 0.5
        ngt = min(max(K - target, 0), len(free))
        row[rng.choice(free, ngt, replace=False)] = 0.5 + rng.random(ngt) * 0.5 + 1e-3
        return row

    def exact_k_above():
        row = np.full(n, 0.125)
        kk = min(K, n)
        row[rng.choice(n, kk, replace=False)] = 0.5 + rng.random(kk)
        return row

    def last_group():
        row = rng.random(n) * 0.25
        cols = np.arange(n - 1, -1, -1)[:K]       # the last group first, spilling into the columns before it when K is larger
        row[cols] = 0.5 + rng.random(len(cols))
        return row

    def denormals():
        return rng.integers(0, 40, n) * 5e-324

    def last_bit():
        row = rng.permutation(n) / float(n) + 0.25          # distinct
        order = np.argsort(-row, kind="stable")
        if K < n:
            row[order[K]] = np.nextafter(row[order[K - 1]], 0.0)
        return row

    fams = [("ties%d" % t, (lambda t=t: ties(t))) for t in NEQ_TARGETS] + [
        ("all_equal", lambda: np.full(n, 0.375)),
        ("exact_k_above", exact_k_above),
        ("last_group", last_group),
        ("zeros", lambda: np.zeros(n)),
        ("denormals", denormals),
        ("last_bit", last_bit),
        ("signed", lambda: rng.integers(-6, 7, n) / 8.0 + (rng.random(n) < 0.5) * rng.standard_normal(n)),
        ("random", lambda: rng.random(n)),
    ]
    W = np.empty((n, n))
    names = []
    for r in range(n):
        name, make = fams[r % len(fams)]
        W[r] = make()
        names.append(name)
    assert last0 <= n - 1
    return W, names


def crafted_update(n, m_src, K, signed, seed=0):
    """Sources, neighbour lists and weights for one update: m_src (n, n) matrices (signed or >= 0), J K distinct columns per row in random order
    (not by weight, as acx_snf_fuse accepts them), V rows that sum to 1."""
    rng = np.random.default_rng(104729 * n + 1009 * m_src + K + seed)
    srcs = [rng.standard_normal((n, n)) if signed else rng.random((n, n)) for _ in range(m_src)]
    J = np.stack([rng.permutation(n)[:K] for _ in range(n)]).astype(np.int32)
    V = rng.random((n, K)) + 1e-3
    V /= V.sum(1)[:, None]
    return srcs, J, V
