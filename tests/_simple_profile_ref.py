"""
Exact reference of the SiMPle matrix profile, its index and the matched section (acx_simple_profile),
the decision rule for continuous data, the exact integer cases and the mutant references.  Built on tests/_simple_ref.py
(_rows, oti, score_bound); tests/test_simple_profile_ref.py checks on the CPU what tests/test_gpu_simple_profile.py relies on.

    MP[a]   = min_b D[a, b]                 D from _simple_ref._rows (sums of squared differences)
    MPI[a]  = the smallest b with D[a, b] == MP[a]        (np.argmin: the first occurrence)
    summary = score, shift, best_q / best_r / best_dist and the longest run of MPI[a + 1] == MPI[a] + 1 (the first of several)

A row of continuous data is DECIDED when the gap between its two smallest exact distances exceeds 2 * score_bound: the
kernel's distances are within score_bound of the exact ones, so no other column can come out smaller on the device.
"""
import math

import numpy as np

from tests import _simple_ref as R

FIELDS = ("shift", "best_q", "best_r", "q0", "r0", "q1", "r1", "run_len")      # the integer fields of a record (+ the two spans)
EXACT_LS = (1, 2, 10, 11, 16)


# ---------------------------------------------------------------- the exact reference
def distances(A, B, L, shift):
    """The whole exact distance matrix D (ma, mb) of A against B rolled by `shift`."""
    Bs = np.roll(B, shift, axis=1)
    ma = A.shape[0] - L + 1
    return np.concatenate([R._rows(A, Bs, L, a0, min(ma, a0 + R.BLOCK)) for a0 in range(0, ma, R.BLOCK)], axis=0)


def profile_index(A, B, L, shift):
    """(MP, MPI, gap): gap[a] = second smallest - smallest distance of row a (inf with a single column), block by block."""
    Bs = np.roll(B, shift, axis=1)
    ma, mb = A.shape[0] - L + 1, B.shape[0] - L + 1
    mp, mpi, gap = np.empty(ma), np.empty(ma, np.int32), np.full(ma, math.inf)
    for a0 in range(0, ma, R.BLOCK):
        a1 = min(ma, a0 + R.BLOCK)
        D = R._rows(A, Bs, L, a0, a1)
        mpi[a0:a1] = np.argmin(D, axis=1)
        mp[a0:a1] = D[np.arange(a1 - a0), mpi[a0:a1]]
        if mb > 1:
            two = np.partition(D, 1, axis=1)[:, :2]
            gap[a0:a1] = two[:, 1] - two[:, 0]
    return mp, mpi, gap


def longest_run(mpi):
    """(a0, n): the longest maximal run of rows with mpi[a + 1] == mpi[a] + 1; of several longest the smallest a0."""
    mpi = np.asarray(mpi, np.int64)
    brk = np.concatenate([[0], np.nonzero(mpi[1:] != mpi[:-1] + 1)[0] + 1, [len(mpi)]])
    lens = np.diff(brk)
    k = int(np.argmax(lens))                               # the first of equal lengths
    return int(brk[k]), int(lens[k])


def summary(mp, mpi, L, shift):
    """The record of a pair from its profile and index (every field of acx_simple_alignment)."""
    a0, n = longest_run(mpi)
    bq = int(np.argmin(mp))
    r0 = int(mpi[a0])
    return dict(score=-float(np.median(mp)), best_dist=float(mp[bq]), shift=int(shift), best_q=bq, best_r=int(mpi[bq]),
                q0=a0, r0=r0, q1=a0 + n - 1, r1=r0 + n - 1, q_span=(a0, a0 + n - 1 + L - 1), r_span=(r0, r0 + n - 1 + L - 1),
                run_len=n)


def reference(A, B, L, do_oti):
    """(MP, MPI, gap, summary, bound) of the ordered pair (A, B); the median of MP is _simple_ref.score_exact's."""
    shift = R.oti(A, B)[0] if do_oti else 0
    mp, mpi, gap = profile_index(A, B, L, shift)
    return mp, mpi, gap, summary(mp, mpi, L, shift), R.score_bound(A, B, L)


def undecided_rows(A, B, L, do_oti):
    """(rows that are not decided, rows, exact-zero rows, smallest gap / bound)."""
    mp, _, gap, _, bound = reference(A, B, L, do_oti)
    return int(np.sum(~(gap > 2.0 * bound))), len(mp), int(np.sum(mp == 0.0)), float(gap.min() / bound)


def record_of(rec):
    """A row of the structured array a call returned -> the dict summary() builds."""
    d = {f: int(rec[f]) for f in FIELDS}
    d.update(score=float(rec["score"]), best_dist=float(rec["best_dist"]), q_span=tuple(int(x) for x in rec["q_span"]),
             r_span=tuple(int(x) for x in rec["r_span"]))
    return d


def same_record(a, b):
    """Two summaries agree in every field, the two f64 values bit for bit."""
    return all(a[f] == b[f] for f in FIELDS + ("q_span", "r_span")) and all(
        np.float64(a[f]).tobytes() == np.float64(b[f]).tobytes() for f in ("score", "best_dist"))


# ---------------------------------------------------------------- exact integer cases: entries in {0, 1, 2}
def _ints(rng, n):
    return rng.integers(0, 3, (n, 12)).astype(np.float64)


def dot_form(A, B, L):
    """D as the kernel forms it, |a|^2 + |b|^2 - 2 <a, b>, in f64: exact for integer tracks."""
    ma, mb = A.shape[0] - L + 1, B.shape[0] - L + 1
    G = A @ B.T
    dot = np.zeros((ma, mb))
    for k in range(L):
        dot += G[k:k + ma, k:k + mb]
    return (R.winnorms(A, L)[:, None] + R.winnorms(B, L)[None, :]) - 2.0 * dot


def period_case(L, seed=0, period=70, ma=151):
    """B = `period` frames repeated three times: columns b and b + period tie in every row.  Row 0 is an exact copy of the
    window at column 62: its zeros sit at columns 62 and 132 (and 202 where that is a column) -- lanes 62, 4 and 10 of three
    different 64-strides; a reduction that orders by the value alone hands lane 0 column 132."""
    rng = np.random.default_rng(700 + 31 * L + seed)
    P = _ints(rng, period)
    B = np.tile(P, (3, 1))
    A = _ints(rng, ma + L - 1)
    A[0:L] = B[62:62 + L]
    return A, B


def col0_tie_case(L, seed=0):
    """The window at column 0 of B stands again at column c = L + 9; A holds it at row 0, at row 5 + L and at the first row
    of the second row group: those rows are zero at columns 0 and c, and the first wins."""
    rng = np.random.default_rng(710 + 31 * L + seed)
    S = R.stride(L)
    B = _ints(rng, 60 + L)
    c = L + 9
    B[c:c + L] = B[0:L]
    A = _ints(rng, S + 12 + L - 1)
    for r in (0, 5 + L, S + 1):                       # (rows L apart at least: the copies do not overlap)
        A[r:r + L] = B[0:L]
    return A, B


def silent_case(L, seed=0):
    """B silent throughout: every distance of a row is |a|^2, MPI is 0 everywhere and the longest run has one row."""
    rng = np.random.default_rng(720 + 31 * L + seed)
    return _ints(rng, 80 + L), np.zeros((50 + L, 12))


def _runs(mpi):
    mpi = np.asarray(mpi, np.int64)
    brk = np.concatenate([[0], np.nonzero(mpi[1:] != mpi[:-1] + 1)[0] + 1, [len(mpi)]])
    return brk[:-1], np.diff(brk)


def two_runs_case(L, seed=0):
    """Two sections of A copied from two places of B, a few frames of noise between them: the first seed (counted from `seed`)
    for which the two longest runs have EQUAL length.  The first must win."""
    for s in range(seed, seed + 2000):
        rng = np.random.default_rng(730 + 31 * L + 1009 * s)
        n = 12 + L - 1
        B = _ints(rng, 90 + L)
        A = np.concatenate([_ints(rng, 4), B[7:7 + n], _ints(rng, 3), B[50:50 + n], _ints(rng, 4)])
        _, mpi, _ = profile_index(A, B, L, 0)
        lens = _runs(mpi)[1]
        if np.sum(lens == lens.max()) >= 2 and lens.max() >= 8:
            return A, B
    raise RuntimeError("no seed with two longest runs of equal length")


def planted_run_case(L, first, last, nb_extra=40, seed=0):
    """A whose rows first .. last are copied from B (one run across them), random elsewhere."""
    rng = np.random.default_rng(740 + 31 * L + 7 * first + seed)
    n = last - first + 1
    B = _ints(rng, n + L - 1 + nb_extra)
    A = _ints(rng, last + 9 + L - 1)
    A[first:first + n + L - 1] = B[11:11 + n + L - 1]
    return A, B


def handover_run_case(L, seed=0):
    """A run across the hand-over from row group 0 to row group 1 (rows STRIDE and STRIDE + 1)."""
    S = R.stride(L)
    return planted_run_case(L, S - 5, S + 6, seed=seed)


def chunk_run_case(L, seed=0):
    """A run across rows 63 and 64: the boundary of the run scan's 64-row chunks."""
    return planted_run_case(L, 57, 71, seed=seed)


def contained_case(L, seed=0, ma=140):
    """A wholly contained in B: every row is an exact zero on one diagonal, run_len == ma (across two row-group hand-overs
    and two chunk boundaries)."""
    rng = np.random.default_rng(750 + 31 * L + seed)
    B = _ints(rng, ma + L - 1 + 37)
    return B[20:20 + ma + L - 1].copy(), B


EXACT_CASES = (("period", period_case), ("col0_tie", col0_tie_case), ("silent", silent_case), ("two_runs", two_runs_case),
               ("handover_run", handover_run_case), ("chunk_run", chunk_run_case), ("contained", contained_case))


def exact_case_set(L):
    """[(name, A, B)] of the exact cases at subsequence length L."""
    return [(name, *make(L)) for name, make in EXACT_CASES]


def exact_pool(L):
    """The exact cases of one L as one call: (tracks, pairs, names)."""
    tracks, pairs, names = [], [], []
    for name, A, B in exact_case_set(L):
        tracks.extend([A, B])
        pairs.append((len(tracks) - 2, len(tracks) - 1))
        names.append(name)
    return tracks, np.array(pairs, np.int32), names


# ---------------------------------------------------------------- mutant references
MUTANTS = ("last_minimum", "index_off_by_one", "row0_without_column_order", "column0_index_lost", "group_first_row_neighbour",
           "last_run_preferred", "run_broken_at_group", "run_broken_at_chunk")


def _row0_butterfly(d0):
    """Row 0's index as a reduction that orders by VALUE alone: lane l keeps the first of its columns l, l + 64, ...; the xor
    butterfly replaces a lane's pair only by a strictly smaller value; lane 0 writes."""
    val = np.full(64, math.inf)
    col = np.full(64, np.iinfo(np.int32).max, np.int64)
    for b, v in enumerate(d0):
        if v < val[b % 64]:
            val[b % 64], col[b % 64] = v, b
    o = 32
    while o:
        other = np.arange(64) ^ o
        ov, oc = val[other], col[other]
        take = ov < val
        val, col = np.where(take, ov, val), np.where(take, oc, col)
        o >>= 1
    return int(col[0])


def _longest_run_with(mpi, extra_breaks=(), last=False):
    mpi = np.asarray(mpi, np.int64)
    brk = set(np.nonzero(mpi[1:] != mpi[:-1] + 1)[0] + 1) | {0} | {int(b) for b in extra_breaks if 0 < b < len(mpi)}
    brk = np.array(sorted(brk) + [len(mpi)])
    lens = np.diff(brk)
    k = int(len(lens) - 1 - np.argmax(lens[::-1])) if last else int(np.argmax(lens))
    return int(brk[k]), int(lens[k])


def _summary_run(mp, mpi, L, shift, a0, n):
    s = summary(mp, mpi, L, shift)
    r0 = int(mpi[a0])
    s.update(q0=a0, r0=r0, q1=a0 + n - 1, r1=r0 + n - 1, q_span=(a0, a0 + n - 1 + L - 1), r_span=(r0, r0 + n - 1 + L - 1), run_len=n)
    return s


def mutants(A, B, L, do_oti):
    """{name: (MPI, summary)} of the mutant kernels:
      last_minimum               the LAST column of equal distances (a `<=` in the sweep)
      index_off_by_one           the column counter one ahead
      row0_without_column_order  row 0's cross-lane reduction ordered by the value alone
      column0_index_lost         a row whose minimum stands in column 0 keeps no index (-1)
      group_first_row_neighbour  the first row of every row group takes the index of the row before it
      last_run_preferred         of several longest runs the last
      run_broken_at_group        every run ends at a row-group hand-over
      run_broken_at_chunk        every run ends at a multiple of 64 rows"""
    shift = R.oti(A, B)[0] if do_oti else 0
    D = distances(A, B, L, shift)
    ma, mb = D.shape
    mp = D.min(1)
    mpi = np.argmin(D, 1).astype(np.int32)
    S = R.stride(L)
    out = {}

    def put(name, idx):
        out[name] = (idx, summary(mp, idx, L, shift))
    put("last_minimum", (mb - 1 - np.argmin(D[:, ::-1], 1)).astype(np.int32))
    put("index_off_by_one", mpi + 1)
    m = mpi.copy()
    m[0] = _row0_butterfly(D[0])
    put("row0_without_column_order", m)
    m = mpi.copy()
    m[1:][mpi[1:] == 0] = -1
    put("column0_index_lost", m)
    m = mpi.copy()
    for r in range(1, ma, S):
        m[r] = mpi[r - 1]
    put("group_first_row_neighbour", m)
    out["last_run_preferred"] = (mpi, _summary_run(mp, mpi, L, shift, *_longest_run_with(mpi, last=True)))
    out["run_broken_at_group"] = (mpi, _summary_run(mp, mpi, L, shift, *_longest_run_with(mpi, range(S + 1, ma, S))))
    out["run_broken_at_chunk"] = (mpi, _summary_run(mp, mpi, L, shift, *_longest_run_with(mpi, range(64, ma, 64))))
    return out


def undetected(cases, L, do_oti=False):
    """The mutants that change neither the index nor the record of any case of the set."""
    left = set(MUTANTS)
    for _, A, B in cases:
        _, mpi, _, s, _ = reference(A, B, L, do_oti)
        for name, (m_idx, m_sum) in mutants(A, B, L, do_oti).items():
            if not np.array_equal(m_idx, mpi) or not same_record(m_sum, s):
                left.discard(name)
    return sorted(left)


# ---------------------------------------------------------------- long tracks: where the LDS steps down
def profile_smem(maxn):
    """simple_profile_smem of the driver: simple_kernel's LDS per wave + 4 bytes per row, rounded up to 16."""
    return 64 + 8 * (2 * maxn + maxn // 48 + 4) + (4 * maxn + 15) // 16 * 16


def waves_per_workgroup(maxn):
    w = 4
    while w > 1 and profile_smem(maxn) * w > 160 * 1024:
        w -= 1
    return w


def step_lengths():
    """The smallest maxn at which the launch takes 3, 2 and 1 waves per workgroup."""
    out, w = [], 4
    for n in range(1, 6001):
        if waves_per_workgroup(n) < w:
            w = waves_per_workgroup(n)
            out.append(n)
    return out
