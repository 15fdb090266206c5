"""
The specification of the EarlyFusion back end in plain numpy: what the selection kernels (ef_rowstat2_kernel,
ef_rowstat_kernel, ef_rowstat_long_kernel, ef_colstat_kernel) and the bit Smith-Waterman (sw_bits_h16_kernel) must leave
behind for one f32 matrix C (M x N).  tests/test_ef_backend_ref.py pins it to the oracle on the CPU;
tests/test_gpu_ef_backend.py holds the kernels against it.

  kb   = oracle.binary_k(kappa, N), kk = min(K, N)
  t_i  = -inf if kb <= 0, +inf if kb >= N, else the kb-th smallest value of row i (an element of the row)
  jcut_i = JCUT_ALL if #(C_i <= t_i) == kb or t_i is infinite, else the column of the (kb - #(C_i < t_i))-th cell
           equal to t_i, in column order
  B_ij = C_ij < t_i, or (C_ij == t_i and j <= jcut_i); pad bits (N <= j < pitch) are 0
  r_i  = mean of the kk smallest of row i, c_j = mean of the min(K, M) smallest of column j, in f64
"""
import numpy as np

JCUT_ALL = 0x7fffffff


def thresholds(C, kb):
    """(t, jcut): f32 (M,), int32 (M,)."""
    C = np.asarray(C, np.float32)
    M, N = C.shape
    jcut = np.full(M, JCUT_ALL, np.int32)
    if kb <= 0:
        return np.full(M, -np.inf, np.float32), jcut
    if kb >= N:
        return np.full(M, np.inf, np.float32), jcut
    t = np.sort(C, axis=1)[:, kb - 1].copy()
    lt = np.sum(C < t[:, None], axis=1)
    le = np.sum(C <= t[:, None], axis=1)
    for i in np.nonzero(le != kb)[0]:
        ties = np.nonzero(C[i] == t[i])[0]
        jcut[i] = ties[kb - lt[i] - 1]
    return t, jcut


def binarise(C, t, jcut):
    """B (M, N) uint8 from the thresholds and tie columns."""
    C = np.asarray(C, np.float32)
    j = np.arange(C.shape[1])[None, :]
    return ((C < t[:, None]) | ((C == t[:, None]) & (j <= jcut[:, None]))).astype(np.uint8)


def pitch_words(N):
    return (N + 63) // 64 * 2


def pack_bits(B):
    """(M, pitch / 32) uint32 words of the device layout: bit j % 32 of word j / 32, pitch = N rounded up to 64, pads 0."""
    B = np.asarray(B, np.uint8)
    M, N = B.shape
    full = np.zeros((M, 32 * pitch_words(N)), np.uint8)
    full[:, :N] = B
    return np.packbits(full, axis=1, bitorder="little").view(np.uint32).reshape(M, pitch_words(N))


def unpack_bits(words, N):
    """The (M, N) matrix and the number of set pad bits of device words."""
    words = np.ascontiguousarray(words, np.uint32)
    full = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")
    return full[:, :N].copy(), int(full[:, N:].sum())


def mean_smallest(C, K, axis):
    """Mean of the min(K, n) smallest along `axis` in f64 (axis 1: r_i of the rows; axis 0: c_j of the columns), and the mean
    of their absolute values (the scale of the rounding bound)."""
    C64 = np.asarray(C, np.float32).astype(np.float64)
    kk = min(int(K), C64.shape[axis])
    S = np.take(np.partition(C64, kk - 1, axis=axis), np.arange(kk), axis=axis)
    return S.mean(axis=axis), np.abs(S).mean(axis=axis)


def mean_bound(K, n, scale):
    """|device f32 mean - f64 mean| <= (kk + 2) 2^-24 mean(|the kk summed cells|): kk - 1 f32 additions in any order, the
    (kk - tot) vk term and the division, half an ulp each on partial sums no larger than the sum of the magnitudes."""
    kk = min(int(K), int(n))
    return (kk + 2) * 2.0 ** -24 * scale


def sw_tenths(B):
    """smith_waterman_constrained (alignment_tools.py:26-46) in integer tenths, row by row: T_ij = max(0, +-10 + max(U[i-1][j-1],
    U[i-2][j-1], U[i-1][j-2])), U = T + (B ? 0 : -7), T = 0 in rows and columns 0, 1.  The reference's score matrix is one
    cell ahead of B: the last row and the last column of B are never read."""
    B = np.asarray(B).astype(bool)
    M, N = B.shape
    if M < 4 or N < 4:
        return 0
    last_i, last_j = M - 2, N - 2
    gap = np.where(B, 0, -7).astype(np.int32)
    hit = np.where(B, 10, -10).astype(np.int32)
    U = gap.copy()
    best = 0
    for i in range(2, last_i + 1):
        mx = np.maximum(np.maximum(U[i - 1, 1:last_j], U[i - 2, 1:last_j]), U[i - 1, 0:last_j - 1])
        T = np.maximum(0, hit[i, 2:last_j + 1] + mx)
        U[i, 2:last_j + 1] = T + gap[i, 2:last_j + 1]
        best = max(best, int(T.max()))
    return best
