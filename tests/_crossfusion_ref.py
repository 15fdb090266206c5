"""
The specification of the full cross-diffusion early fusion (acoss_amd/csrc/ef_crossfusion_kernels.hpp):
one numpy function per new kernel in the kernel's operation order, sums in np.longdouble; the SNF stages that the chain
reuses come from tests/_snf_ref.py.  tests/test_crossfusion_ref.py pins W and D to the reference's own getWCSMSSM and
doSimilarityFusionWs (tests/golden/crossfusion.npz) and shows that the golden inputs tell the chain from four wrong variants;
tests/test_gpu_crossfusion.py holds the device's stages against these functions.
"""
import numpy as np

from . import _snf_ref as snf

LD = np.longdouble
U = 2.0 ** -53
MU = 0.5
WRONG_VARIANTS = ("k_swapped", "lower_not_transposed", "upper_block_only", "k_smallest")


def split(M, N, K):
    """similarity_fusion.py:93-94."""
    k1 = int(K * float(M) / (M + N))
    return k1, K - k1


def refused(M, N, K):
    """What acx_ef_crossfusion_pairs refuses: np.partition has no room (raises) or a mean is taken over no cell (NaN)."""
    k1, k2 = split(M, N, K)
    return k1 < 1 or k2 < 1 or k1 + 1 >= M or k2 + 1 >= N


def binary_k(kappa, ncols):
    """cross_recurrence.py:149-154 (numpy rounds half to even)."""
    if kappa == 0:
        return ncols
    if kappa < 1:
        return int(np.round(kappa * ncols))
    return int(kappa)


def means(C, k_row, k_col):
    """xf_means_kernel: r_i = mean of the k_row smallest cells of row i, c_j = mean of the k_col smallest of column j of the
    f32 matrix C, widened exactly.  Returns (r, c longdouble, r_bound, c_bound): an f64 evaluation in any order lies within
    (k + 1) 2^-53 mean(|the taken cells|) -- k - 1 additions and a division."""
    C = np.asarray(C, dtype=np.float64)
    rows = np.sort(C, 1)[:, :k_row]
    cols = np.sort(C, 0)[:k_col, :]
    r = rows.astype(LD).sum(1) / LD(k_row)
    c = cols.astype(LD).sum(0) / LD(k_col)
    return r, c, (k_row + 1) * U * np.abs(rows).mean(1), (k_col + 1) * U * np.abs(cols).mean(0)


def cross_arg(C, r, c, mu=MU):
    """The argument of the exponential of xf_cross_affinity_kernel, operation for operation (similarity_fusion.py:52-54; the
    library is built with -ffp-contract=off): Eps = ((r_i + c_j) + C) / 3, -(C C) / (2 ((mu Eps) (mu Eps)))."""
    C = np.asarray(C, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        eps = r[:, None] + c[None, :] + C
        eps = eps / 3.0
        me = mu * eps
        return -(C * C) / (2.0 * (me * me))


def cross_affinity(C, r, c, mu=MU):
    with np.errstate(invalid="ignore", under="ignore"):
        return np.exp(cross_arg(C, r, c, mu))


def getw(S, K, mu=MU):
    """A diagonal block: xf_widen_kernel (exact), then snf_sym_kernel, snf_localscale_kernel, snf_affinity_kernel with K = k1 or k2."""
    Sy = snf.sym(np.asarray(S, dtype=np.float64))
    md = snf.f64(snf.localscale(Sy, K)[0])
    return snf.affinity(Sy, md, mu)


def assemble(WA, WB, WC):
    """xf_place_kernel and the two stores of xf_cross_affinity_kernel (setupWCSMSSM, similarity_fusion.py:56-74)."""
    M, N = WC.shape
    W = np.zeros((M + N, M + N))
    W[:M, :M] = WA
    W[:M, M:] = WC
    W[M:, :M] = WC.T
    W[M:, M:] = WB
    return W


def wcsmssm(SA, SB, C, K, mu=MU, wrong=None):
    """getWCSMSSM (similarity_fusion.py:76-99) from the stage functions, every stage rounded to f64 as the device stores it."""
    M, N = C.shape
    k1, k2 = split(M, N, K)
    ka, kb = (k2, k1) if wrong == "k_swapped" else (k1, k2)       # getWCSM(C, k1, k2): rows take k2, columns k1
    r, c, _, _ = means(C, kb, ka)
    WC = cross_affinity(C, snf.f64(r), snf.f64(c), mu)
    return assemble(getw(SA, k1, mu), getw(SB, k2, mu), WC)


def fuse_ws(Ws, K, niters, reg_diag):
    """doSimilarityFusionWs (similarity_fusion.py:146-186) on snf_knn_kernel, snf_rownorm_kernel and the loop of snf_loop, the
    two work lists aliasing from the second sweep on."""
    m = len(Ws)
    Js, Vs, cur = [], [], []
    for W in Ws:
        J, V, _ = snf.knn(W, K)
        Js.append(J); Vs.append(snf.f64(V)); cur.append(snf.f64(snf.rownorm(W)[0]))
    nxt = [None] * m
    for it in range(niters):
        src = cur if it == 0 else nxt
        for i in range(m):
            nxt[i] = snf.update([src[k] for k in range(m) if k != i], 1.0 / (m - 1), Js[i], Vs[i], reg_diag)
    return snf.f64(snf.mean(nxt, 1.0 / m)[0])


def x_of(D, M, wrong=None):
    """xf_x_kernel: X = D[0:M, M:] + D[M:, 0:M]^T, one addition per cell (bit-identical)."""
    N = D.shape[0] - M
    up = D[:M, M:]
    if wrong == "upper_block_only":
        return up.copy()
    if wrong == "lower_not_transposed":
        return up + np.ascontiguousarray(D[M:, :M]).reshape(M, N)
    return up + D[M:, :M].T


def select(X, k, wrong=None):
    """xf_select_kernel: the first k of the stable descending argsort of every row (-0.0 ranks with +0.0, as numpy compares)."""
    M, N = X.shape
    B = np.zeros((M, N), np.uint8)
    k = min(max(int(k), 0), N)
    if k == 0:
        return B
    order = np.argsort(X if wrong == "k_smallest" else -X, 1, kind="stable")[:, :k]
    B[np.arange(M)[:, None], order] = 1
    return B


def cut_gap(X, k):
    """Per row the distance between the k-th and the (k + 1)-th largest value: what a selection on other roundings of X may
    flip when it is small (inf where the cut takes no or every cell)."""
    M, N = X.shape
    if k <= 0 or k >= N:
        return np.full(M, np.inf)
    s = -np.sort(-X, 1)
    return s[:, k - 1] - s[:, k]


def pack_bits(B):
    """The bitmap layout of d_efbits: bit j % 32 of word j / 32, pitch = N rounded up to 64, pad bits zero."""
    M, N = B.shape
    words = (N + 63) // 64 * 2
    P = np.zeros((M, words * 32), np.uint8)
    P[:, :N] = B
    w = P.reshape(M, words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)[None, None, :]
    return w.sum(2).astype(np.uint32)


def unpack_bits(bits, N):
    M, words = bits.shape
    b = (bits[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1
    return b.reshape(M, words * 32)[:, :N].astype(np.uint8), b.reshape(M, words * 32)[:, N:]


def chain(SA, SB, C, K, niters, reg_diag, kappa, wrong=None):
    """The whole definition for one pair: SA (3, M, M), SB (3, N, N), C (3, M, N) f32.  -> dict(W, D, X, B)."""
    M, N = C.shape[1:]
    Ws = [wcsmssm(SA[f], SB[f], C[f], K, MU, wrong) for f in range(3)]
    D = fuse_ws(Ws, K, niters, reg_diag)
    X = x_of(D, M, wrong)
    return dict(W=np.stack(Ws), D=D, X=X, B=select(X, binary_k(kappa, N), wrong))
