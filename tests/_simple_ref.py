"""
Exact SiMPle reference, its error bound, mutant references and the SiMPle shape cases of
tests/test_gpu_simple_shapes.py (built here so that tests/test_simple_ref.py can check them on the CPU).

Layout: a track is (n, 12) f64, time-major (the layout of upload_pool_f64).  A pair (A, B) at
subsequence length L has ma = na - L + 1 profile rows and mb = nb - L + 1 columns.

profile_exact evaluates every distance as a sum of SQUARED DIFFERENCES (no cancellation):
    F[t, u]  = sum_c (A[t, c] - B'[u, c])^2                  12 non-negative terms
    D[a, b]  = sum_{k < L} F[a + k, b + k]                     L non-negative terms
so every D[a, b] is within (12 + L) u of itself (u = 2^-53), and since min and median are monotone,
the score -median(min_b D) is within (12 + L + 1) u |score| of the true score.
"""
import math

import numpy as np

U = 2.0 ** -53                     # unit roundoff of f64
F32_U = 2.0 ** -24                 # unit roundoff of f32 (pair_grid stores float32)
BLOCK = 512                        # rows of the distance matrix per block


def stride(L):
    return 64 - L


def rounds(L):
    """Steps per unrolled round of simple_kernel<L> (UN)."""
    return L if L % 2 == 0 else 2 * L


def tail_start(L, mb):
    """First column of the guarded tail of a sweep (simple_kernel: FULL rounds while b0 + UN + 1 < mb)."""
    un, b0 = rounds(L), 1
    while b0 + un + 1 < mb:
        b0 += un
    return b0


def oti(A, B):
    """oracle.simple_oti on time-major tracks: (shift, gap between the best and second best OTI value, scale)."""
    pa, pb = A.sum(0), B.sum(0)
    v = np.array([np.dot(pa, np.roll(pb, s)) for s in range(12)])
    # ties: the highest index, the kernel's `acc >= bestv`.  That is argsort(v)[-1] of a STABLE sort; numpy's default
    # argsort is not stable on every CPU (its SIMD sorts pick another of the tied indices), so the kind is explicit here
    s = int(np.argsort(v, kind="stable")[-1])
    srt = np.sort(v)
    return s, float(srt[-1] - srt[-2]), float(np.dot(np.abs(pa), np.abs(pb)) + 1e-300)


def winnorms(X, L):
    m = X.shape[0] - L + 1
    e = np.sum(X * X, 1)
    return np.array([np.sum(e[t:t + L]) for t in range(m)]) if m > 0 else np.zeros(0)


def _frame_dist(A, B, t0, t1):
    """F[t, u] = sum_c (A[t, c] - B[u, c])^2 for t in [t0, t1): direct differences."""
    F = np.zeros((t1 - t0, B.shape[0]))
    for c in range(12):
        d = A[t0:t1, c][:, None] - B[None, :, c]
        F += d * d
    return F


def _rows(A, B, L, a0, a1):
    """D[a, b] for rows a in [a0, a1), all columns."""
    mb = B.shape[0] - L + 1
    F = _frame_dist(A, B, a0, a1 + L - 1)
    D = np.zeros((a1 - a0, mb))
    for k in range(L):
        D += F[k:k + a1 - a0, k:k + mb]
    return D


def profile_exact(A, B, L, shift):
    """MP[a] = min_b sum_{c, k} (A[a + k, c] - B'[b + k, c])^2 with B' = roll(B, shift) over the chroma axis."""
    B = np.roll(B, shift, axis=1)
    ma = A.shape[0] - L + 1
    out = np.empty(ma)
    for a0 in range(0, ma, BLOCK):
        a1 = min(ma, a0 + BLOCK)
        out[a0:a1] = _rows(A, B, L, a0, a1).min(1)
    return out


def score_exact(A, B, L, do_oti=True):
    """-median(profile_exact) with the OTI shift of oracle.simple_oti (0 without OTI); also the OTI gap and scale."""
    s, gap, scale = oti(A, B) if do_oti else (0, math.inf, 1.0)
    return -float(np.median(profile_exact(A, B, L, s))), s, gap, scale


def score_bound(A, B, L):
    """Absolute bound on |kernel score - score_exact|.

    Write E = max window energy |x_t|^2 + ... + |x_{t+L-1}|^2 over both tracks and d = min(ma, mb) - 1, the
    longest run of diagonal steps behind any cell.  simple_kernel computes dist = (a2 + w) - 2 dot:
      * a2, w: sums of 12L squares (simple_winnorm_kernel): error <= 12L u E each, i.e. 24L u E together;
      * dot at the origin of its diagonal (row 0 or column 0, evaluated in full): the 12-term products and
        their L-term sum, error <= (12 + L) u E (Cauchy-Schwarz: sum |a_i b_i| <= sqrt(a2 w) <= E);
      * every step down the diagonal: dot = (prev - gold) + gnew, where gold is bit for bit the product that
        entered L steps before (the products' own rounding leaves with them), so a step adds only the
        rounding of two additions whose results are bounded by E (first order): 2 u E per step, 2 d u E;
      * the fma (a2 + w) - 2 dot: the rounding of a2 + w (2 u E) and of the result (4 u E at most).
    |error(dist)| <= 24L u E + 2 (12 + L + 2d) u E + 6 u E = (26L + 4d + 30) u E.  min over b and the median
    are 1-Lipschitz in the sup norm, so this bounds the profile and the score; the median of an even count
    rounds once more (u |score|), and the reference itself is within (12 + L + 1) u |score| (module doc).
    Second-order terms (products of two u) are covered by rounding the constant 30 up to 32."""
    ea, eb = winnorms(A, L), winnorms(B, L)
    E = max(float(ea.max(initial=0.0)), float(eb.max(initial=0.0)))
    d = min(len(ea), len(eb)) - 1
    return U * E * (26 * L + 4 * max(d, 0) + 32)


def score_tol(A, B, L, ref, f32=False):
    """score_bound plus the reference's and the median's own rounding; f32: the float32 store of pair_grid."""
    t = score_bound(A, B, L) + U * (14 + L) * abs(ref)
    if f32:
        t += F32_U * (abs(ref) + t)
    return t


# ---------------------------------------------------------------- mutant references
MUTANTS = ("last_column_dropped", "row0_dropped", "handover_first", "handover_last", "L_plus_1", "L_minus_1",
           "wrong_oti_shift", "next_column_winnorm")


def _median(x):
    return float(np.median(x)) if len(x) else math.nan


def mutant_scores(A, B, L, do_oti=True):
    """The score of each mutant of the kernel (None where the mutant does not exist for this shape):
      last_column_dropped  the sweep stops one column short
      row0_dropped         row 0's value never reaches the profile
      handover_first       the first row of group 0 (row 1) takes its neighbour's (row 0's) value
      handover_last        the first row of the last row group takes its neighbour's value
      L_plus_1, L_minus_1  the instantiation of a neighbouring L
      wrong_oti_shift      B rolled by shift + 1 (with OTI off: rolled by 1)
      next_column_winnorm  the window norm of column b + 1 used at column b (the slot behind the last column: 0)"""
    s = oti(A, B)[0] if do_oti else 0
    Bs = np.roll(B, s, axis=1)
    ma, mb = A.shape[0] - L + 1, B.shape[0] - L + 1
    wb = winnorms(Bs, L)
    wnext = np.append(wb[1:], 0.0) - wb
    mp = np.empty(ma)
    mp_last = np.empty(ma)
    mp_wn = np.empty(ma)
    for a0 in range(0, ma, BLOCK):
        a1 = min(ma, a0 + BLOCK)
        D = _rows(A, Bs, L, a0, a1)
        mp[a0:a1] = D.min(1)
        mp_last[a0:a1] = D[:, :-1].min(1) if mb > 1 else math.inf
        mp_wn[a0:a1] = (D + wnext[None, :]).min(1)
    out = {"last_column_dropped": -_median(mp_last), "row0_dropped": -_median(mp[1:]) if ma > 1 else math.nan,
           "next_column_winnorm": -_median(mp_wn)}
    for name, g in (("handover_first", 0), ("handover_last", (ma - 2) // stride(L) if ma >= 2 else -1)):
        r = stride(L) * g + 1
        if g < 0 or r > ma - 1:
            out[name] = None
            continue
        m2 = mp.copy()
        m2[r] = mp[r - 1]
        out[name] = -_median(m2)
    for name, L2 in (("L_plus_1", L + 1), ("L_minus_1", L - 1)):
        out[name] = (-_median(profile_exact(A, Bs, L2, 0)) if L2 >= 1 and min(A.shape[0], B.shape[0]) >= L2 else
                     (None if L2 < 1 else math.nan))
    out["wrong_oti_shift"] = -_median(profile_exact(A, B, L, (s + 1) % 12))
    return out


# ---------------------------------------------------------------- data
def frames(rng, n, peak=0.0):
    """n i.i.d. L2-normalised non-negative chroma frames; peak: added to bin 0 (a key the OTI shift locks on)."""
    X = rng.random((n, 12)) + 0.05
    X[:, 0] += peak
    return X / np.linalg.norm(X, axis=1, keepdims=True)


def n_lose(ma):
    """Near-zero rows for which LOSING one moves the median by O(1): k + 1 of 2k + 1, k of 2k."""
    return ma // 2 + 1 if ma % 2 else ma // 2


def n_gain(ma):
    """Near-zero rows for which GAINING one moves the median by O(1): k of 2k + 1, k of 2k."""
    return ma // 2


def _embed(rng, A, L, s0, n, nb, at, shift):
    """B of nb frames holding A[s0 : s0 + n + L - 1] (rolled by -shift) from frame `at`: rows s0 .. s0 + n - 1
    of the profile are exact zeros, at columns at .. at + n - 1; everything else is random."""
    B = frames(rng, nb)
    B[at:at + n + L - 1] = np.roll(A[s0:s0 + n + L - 1], -shift, axis=1)
    return B


def _fixpoint(rng_seed, A, L, s0, n, nb, at, do_oti):
    """_embed with the roll that OTI will undo: the first shift that is its own OTI shift (unambiguous)."""
    for tries in range(8):
        for s in (range(12) if do_oti else (0,)):
            rng = np.random.default_rng(rng_seed + 1000 * tries)
            B = _embed(rng, A, L, s0, n, nb, at, s)
            if not do_oti:
                return B
            s2, gap, scale = oti(A, B)
            if s2 == s and gap > 1e-9 * scale:
                return B
    raise RuntimeError("no OTI fixpoint")


def row_probe(seed, L, ma, r, positive=True, nb=None, at_end=False, do_oti=False):
    """(A, B): the score is ~0 / O(1) depending on row r alone.  positive: n_lose(ma) exact-zero rows that contain r
    (a wrong row r lifts the median to O(1)); else n_gain(ma) zero rows next to r but not r (a row r wrongly near
    zero drops it to ~0).  at_end: the zero run's matches end at the last column."""
    rng = np.random.default_rng(seed)
    na = ma + L - 1
    A = frames(rng, na, peak=1.5)
    if positive:
        n = n_lose(ma)
        s0 = r if at_end and r + n <= ma else min(max(0, r - n // 2), ma - n)
    else:
        n = n_gain(ma)
        s0 = r + 1 if r + 1 + n <= ma else r - n
        assert s0 >= 0
    return run_probe(seed, L, A, s0, n, nb, at_end, do_oti)


def run_probe(seed, L, A, s0, n, nb=None, at_end=False, do_oti=False):
    """(A, B): rows s0 .. s0 + n - 1 of A's profile are exact zeros, everything else O(1)."""
    nb = nb or n + L - 1 + 7
    at = nb - (n + L - 1) if at_end else 3
    return A, _fixpoint(seed + 7, A, L, s0, n, nb, at, do_oti)


def handover_probe(seed, L, ma, r, nb=None, do_oti=False):
    """(A, B) whose score flips if row r (a group's first row) took row r - 1's value: n_lose(ma) zero rows from r when
    they fit (r loses its zero), else n_gain(ma) zero rows ending at r - 1 (r gains one)."""
    A = frames(np.random.default_rng(seed), ma + L - 1, peak=1.5)
    if r + n_lose(ma) <= ma:
        return run_probe(seed, L, A, r, n_lose(ma), nb, do_oti=do_oti)
    assert r - n_gain(ma) >= 0
    return run_probe(seed, L, A, r - n_gain(ma), n_gain(ma), nb, do_oti=do_oti)


def col_probe(seed, L, mb, c, ma=9):
    """(A, B), OTI off: A holds the frames of B's columns c .. c + n - 1 (n = n_lose(ma)) from row 1, or ending at column c when
    they do not fit: column c is the only match of one of the n zero rows of the median."""
    rng = np.random.default_rng(seed)
    nb = mb + L - 1
    B = frames(rng, nb)
    n = n_lose(ma)
    c0 = c if c + n <= mb else c - n + 1
    assert c0 >= 0
    A = frames(rng, ma + L - 1)
    A[1:1 + n + L - 1] = B[c0:c0 + n + L - 1]
    return A, B


# ---------------------------------------------------------------- cases of the GPU tests
def boundary_lengths(L):
    """(ma values, mb values) at simple_kernel<L>'s boundaries."""
    S, un = stride(L), rounds(L)
    mas = {1, 2, 3}
    for g in (1, 2, 3):                                  # ma - 1 == 0, 1, S - 1 (mod S) around 1, 2, 3 full groups
        for e in (0, 1, S - 1):
            mas.add(S * g + 1 + e if e != S - 1 else S * (g - 1) + 1 + e)
        mas.add(S * g + 2)
    mas = sorted(m for m in mas if m >= 1)
    # mb <= UN + 2: no FULL round, the whole sweep is the guarded tail (mb - 1 = 0, 1, 2 .. steps).  The first FULL round
    # runs from mb = UN + 3 (b0 + UN + 1 < mb); after k FULL rounds the tail has 2 .. UN + 1 steps (a FULL round needs the
    # frame two steps behind its last step, so a tail of 0 or 1 step follows no FULL round): both ends and UN - 1, UN.
    mbs = {1, 2, 3, un + 1, un + 2}
    for k in (1, 2):
        for tail in (2, 3, un - 1, un, un + 1):
            mbs.add(1 + k * un + tail)
    return mas, sorted(m for m in mbs if m >= 1)


def every_L_case(L, do_oti, seed=0):
    """One call per (L, oti) for simple_pairs: (tracks, pairs).  Random pairs at every boundary (ma, mb) shape, even
    and odd ma, plus planted pairs: the last column (run of zero rows ending at column mb - 1) and the hand-over rows of
    the first and the last group."""
    rng = np.random.default_rng(1000 * L + 17 * do_oti + seed)
    mas, mbs = boundary_lengths(L)
    tracks, pairs = [], []

    def add(A, B):
        tracks.extend([A, B])
        pairs.append((len(tracks) - 2, len(tracks) - 1))
    # every ma against a few mb, every mb against a few ma (not the full product: the call stays small)
    for i, ma in enumerate(mas):
        add(frames(rng, ma + L - 1), frames(rng, mbs[(3 * i) % len(mbs)] + L - 1))
    for i, mb in enumerate(mbs):
        add(frames(rng, mas[(5 * i + 2) % len(mas)] + L - 1), frames(rng, mb + L - 1))
    for ma in sorted({mas[-1], mas[-2], 2 * stride(L) + 2, 7}):
        G = (ma - 2) // stride(L) if ma >= 2 else 0
        add(*row_probe(seed + 31 * ma, L, ma, 1 if ma > 1 else 0, positive=True, at_end=True, do_oti=do_oti))
        r = stride(L) * G + 1
        if ma > 2 and r <= ma - 1:
            add(*handover_probe(seed + 37 * ma, L, ma, r, do_oti=do_oti))
    add(frames(rng, L), frames(rng, L))                  # ma = mb = 1: track length == L
    return tracks, np.array(pairs, np.int32)


def probe_rows(L, ma):
    S = stride(L)
    rows = {1, ma - 1}
    g = 0
    while S * g + 1 <= ma - 1:
        rows.add(S * g + 1)                              # first row of group g (lane 0: the DPP hand-over)
        rows.add(min(ma - 1, S * (g + 1)))               # last row of group g (vl == 63: the E writer)
        for k in range(L):                               # the rows the feeders of group g + 1 repeat
            if g == 0 or k in (0, L - 1):
                rows.add(max(1, S * (g + 1) - k))
        g += 1
    return sorted(r for r in rows if 0 <= r < ma)


def probe_cols(L, mb):
    un, t = rounds(L), tail_start(L, mb)
    cols = {0, 1, mb - 1, t, t - 1}
    cols.update(range(1, min(mb, 1 + 2 * un)))           # every column of the first two rounds
    return sorted(c for c in cols if 0 <= c < mb)


PROBE_LS = (1, 2, 3, 9, 10, 11, 16)


def probe_case(L, seed=0):
    """Row and column probes of simple_kernel<L>, OTI off: (tracks, pairs)."""
    S, un = stride(L), rounds(L)
    ma = 2 * S + S // 2 + 1                              # two full groups and half a third one, odd
    mb_row = n_lose(ma) + L + 8
    mb = 3 * un + 5                                      # FULL rounds then a tail
    tracks, pairs = [], []
    for r in probe_rows(L, ma):
        for pos in (True, False):
            if not pos and r + 1 + n_gain(ma) > ma and r - n_gain(ma) < 0:
                continue
            A, B = row_probe(seed + 101 * r + pos, L, ma, r, positive=pos, nb=mb_row + L - 1)
            tracks.extend([A, B])
            pairs.append((len(tracks) - 2, len(tracks) - 1))
    for c in probe_cols(L, mb):
        A, B = col_probe(seed + 211 * c, L, mb, c)
        tracks.extend([A, B])
        pairs.append((len(tracks) - 2, len(tracks) - 1))
    return tracks, np.array(pairs, np.int32)


def undetected(tracks, pairs, L, do_oti, factor=100.0):
    """The mutants that move no score of this call by more than factor x its bound (score_tol).  A mutant that does not
    exist for any pair of the call (handover_* where ma < 2, L_minus_1 at L = 1) counts as detected."""
    left = set(MUTANTS)
    for i, j in pairs:
        if not left:
            break
        A, B = tracks[i], tracks[j]
        ref = score_exact(A, B, L, do_oti)[0]
        tol = score_tol(A, B, L, ref)
        for m, v in mutant_scores(A, B, L, do_oti).items():
            if v is None or not np.isfinite(v) or abs(v - ref) > factor * tol:
                left.discard(m)
    return sorted(left)


def pool_of(tracks):
    offs = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
    return np.ascontiguousarray(np.concatenate(tracks)), offs


# ---------------------------------------------------------------- the vectorised reference of length-L tracks
def short_table(T, L, do_oti=True):
    """T: (N, L, 12) tracks of exactly L frames (ma = mb = 1).  (N, N) exact scores, OTI shifts, OTI gaps / scale."""
    N = T.shape[0]
    P = T.sum(1)
    V = np.stack([P @ np.roll(P, s, axis=1).T for s in range(12)], -1)          # V[i, j, s] = <pa_i, roll(pb_j, s)>
    sh = 11 - np.argmax(V[:, :, ::-1], axis=-1) if do_oti else np.zeros((N, N), np.int64)
    Vs = np.sort(V, -1)
    gap = (Vs[..., -1] - Vs[..., -2]) / (np.abs(P) @ np.abs(P).T + 1e-300)
    out = np.empty((N, N))
    for s in range(12):
        i, j = np.nonzero(sh == s)
        if len(i) == 0:
            continue
        Br = np.roll(T, s, axis=2)
        acc = np.zeros(len(i))
        for k in range(L):
            d = T[i, k, :] - Br[j, k, :]
            acc += np.sum(d * d, 1)
        out[i, j] = -acc
    E = np.max(np.sum(T * T, axis=(1, 2)))
    bound = U * E * (26 * L + 32) + U * (14 + L) * np.abs(out)
    return out, sh, gap if do_oti else np.full((N, N), np.inf), bound


def long_case(maxn, L, seed=0, long_pair=False):
    """One simple_pairs call whose longest track has maxn frames (the LDS limit of launch_simple picks 4 / 3 / 2 / 1 waves
    per workgroup from it): long x short, short x long, short x short, a planted long x half-long pair (zero rows of the
    median ending at the last column), and, with long_pair, long x long.  7 or 8 pairs (not a multiple of the waves)."""
    rng = np.random.default_rng(7919 * maxn + L + seed)
    ma = maxn - L + 1
    A, B = row_probe(seed + maxn, L, ma, 1, positive=True, at_end=True, nb=n_lose(ma) + L - 1 + 5, do_oti=True)
    r = stride(L) * ((ma - 2) // stride(L)) + 1                       # the first row of the last group
    C, D = handover_probe(seed + maxn + 1, L, ma, r, nb=n_lose(ma) + L + 9, do_oti=True)
    tracks = [A, B, frames(rng, 40 + L), frames(rng, 61 + L), frames(rng, maxn), C, D]
    pairs = [(4, 2), (2, 4), (2, 3), (3, 2), (0, 1), (1, 0), (4, 3), (5, 6)]
    pairs.append((4, 0) if long_pair else (3, 0))
    return tracks, np.array(pairs, np.int32)


def silence_tracks(seed, L):
    """oracle.simple_smooth'ed tracks with runs of all-zero frames (left unscaled) and whole zero windows, a planted
    pair, and (last) one track that is silent throughout."""
    import oracle
    rng = np.random.default_rng(seed)
    out = []
    for n, runs in ((90, ((0, 30),)), (150, ((40, 75), (120, 150))), (70, ((20, 50),)), (L + 3, ())):
        raw = rng.random((12, n))
        for r0, r1 in runs:
            raw[:, r0:r1] = 0.0
        out.append(np.ascontiguousarray(oracle.simple_smooth(raw).T))
    out.extend(row_probe(seed, L, 33, 1, positive=True, at_end=True, do_oti=True))   # zero rows ending at the last column
    out.append(np.zeros((L + 20, 12)))
    return out


def tie_case(seed=5, L=4):
    """Integer tracks whose OTI values tie exactly (every product and sum exact in f64): (tracks, pairs, tied shift sets).
    Ties at shifts {0, 11}, at two interior shifts {4, 7}, and at all 12 (a flat profile of B); the last pair (ties None) is
    a planted random one."""
    rng = np.random.default_rng(seed)
    A = rng.integers(0, 4, (24, 12)).astype(np.float64)
    pa = A.sum(0)
    tracks, pairs, ties = [A], [], []
    for want in ((0, 11), (4, 7), tuple(range(12))):
        if len(want) == 12:
            pb = np.full(12, 30.0)
        else:
            cand = rng.integers(0, 40, (400000, 12)).astype(np.float64)
            V = np.stack([cand @ np.roll(pa, -s) for s in range(12)], 1)         # <pa, roll(pb, s)> = <roll(pa, -s), pb>
            mx = V.max(1, keepdims=True)
            ok = np.all((V == mx) == np.isin(np.arange(12), want)[None, :], 1)
            pb = cand[np.nonzero(ok)[0][0]]
        B = rng.integers(0, 4, (30, 12)).astype(np.float64)
        B[-1] = pb - B[:-1].sum(0)
        tracks.append(B)
        pairs.append((0, len(tracks) - 1))
        ties.append(want)
    C, D = row_probe(seed, L, 21, 1, positive=True, at_end=True, do_oti=True)   # not integer: its zero rows end at the last column
    tracks.extend([C, D])
    pairs.append((len(tracks) - 2, len(tracks) - 1))
    ties.append(None)
    return tracks, np.array(pairs, np.int32), ties


def every_L_grid_tracks(L, do_oti, seed=0):
    """A 9-track pool for pair_grid at simple_kernel<L>'s boundaries: every ordered pair of it is one grid cell."""
    rng = np.random.default_rng(3000 * L + 17 * do_oti + seed)
    S, un = stride(L), rounds(L)
    lens = sorted({1, 2, S + 1, S + 2, 2 * S + 1, un + 2, 1 + un + (un - 1)})
    tracks = [frames(rng, m + L - 1) for m in lens]
    # a planted pair: its median rests on zero rows that end at the last column
    A, B = row_probe(seed + 5 * L, L, 2 * S + 3, 1, positive=True, at_end=True, do_oti=do_oti)
    return tracks + [A, B]


def long_grid_tracks(seed=0):
    """A 6000-frame track among short ones (L = 10): one grid call at a single wave per workgroup."""
    rng = np.random.default_rng(seed + 6000)
    A, B = row_probe(seed + 6001, 10, 5991, 1, positive=True, at_end=True, nb=n_lose(5991) + 9 + 5, do_oti=True)
    return [A, B] + [frames(rng, n) for n in (10, 47, 64, 130)]


def chunk_pairs_case(seed=0, L=5, M=64, extra=37):
    """(T (M, L, 12), pairs, L): 2^22 + extra random ordered pairs of tracks of exactly L frames (ma = mb = 1, each score
    one distance), drawn among the pairs with an unambiguous OTI shift."""
    rng = np.random.default_rng(seed + 22)
    T = frames(rng, M * L).reshape(M, L, 12)
    _, _, gap, _ = short_table(T, L)
    ok = np.argwhere(gap > 1e-9)
    pairs = ok[rng.integers(0, len(ok), (1 << 22) + extra)].astype(np.int32)
    return T, pairs, L


def chunk_grid_tracks(seed=0, L=2, N=2100):
    """(T (N, L, 12), L): N tracks of exactly L frames, N (N - 1) > 2^22 ordered pairs in one pair_grid call."""
    rng = np.random.default_rng(seed + 2100)
    return frames(rng, N * L, peak=0.0).reshape(N, L, 12), L


def winnorm_cache_pools(seed=0):
    """Two pools of the same shape (track lengths) with different frames."""
    lens = (25, 40, 63, 90)
    return [[frames(np.random.default_rng(seed + 100 * p + k), n) for k, n in enumerate(lens)] for p in range(2)]
