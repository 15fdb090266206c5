"""
SiMPle at every compiled shape: simple_kernel<L> for L = 1..16 through both entry points, against the exact
reference of tests/_simple_ref.py (sums of squared differences) within its derived bound (score_bound).  Every
test records the largest |kernel - exact| / bound it saw (printed, and in simple_shapes.json through
test_gpu_parity_sets' _record); the assertion is that it stays <= 1.  tests/test_simple_ref.py shows on the
CPU that every call below moves by more than 100 bounds under each mutant of _simple_ref.MUTANTS, so these
assertions would fail on those bugs.

What runs where:
  simple_kernel<1..16>, oti on / off, simple_pairs ....... test_every_L_simple_pairs
  simple_kernel<1..16>, oti on / off, pair_grid ........... test_every_L_pair_grid
  ma = 1, mb = 1 (track length == L); ma - 1 = 0, 1, S - 1 (mod S = 64 - L) around 1, 2, 3 groups; mb without a
    FULL round (tail of 0, 1, 2 steps, UN + 1) and after 1 and 2 FULL rounds (UN = L, 2L for odd L) with tails of
    2, 3, UN - 1, UN, UN + 1 steps (the shortest and longest possible); even and odd ma .. test_every_L_simple_pairs
  the f64 kernel scores are checked against the bound; pair_grid's cells also equal float32(simple_pairs) bit for bit,
    and their recorded ratio includes the float32 store (up to half an ulp of the score)
  row probes (row 1, first / last row of every group, the feeder rows below a boundary, the last row) and column
    probes (0, 1, every column of the first two rounds, both sides of FULL -> tail, mb - 1), L in PROBE_LS
    ......................................................................................... test_row_and_column_probes
  4 / 3 / 2 / 1 waves per workgroup (longest track 2528 | 2529, 3372 | 3373, 5061 | 5062, 6000), 7 or 8 pairs per
    call, short pairs next to a long track, long x short and short x long, L = 16 at 6000 x 6000 .. test_long_tracks
  the same through pair_grid on a small grid with one 6000-frame track ................ test_long_track_grid
  the 2^22-pair chunks of simple_pairs (sort / un-sort across the boundary) ............. test_chunk_boundary_pairs
  the 2^22-pair chunks of pair_grid (run_simple_tiles) over 2100 tracks, every cell ....... test_chunk_boundary_grid
  exact OTI ties at shifts {0, 11}, {4, 7} and all 12: the highest shift wins .......... test_oti_exact_ties
  silent frames, zero windows, all-zero tracks, self-pairs without OTI ................. test_silence_and_self_pairs
  the window-norm cache keyed on (pool, L) ................................................ test_winnorm_cache
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _simple_ref as R          # noqa: E402

LONG = ((2528, 10), (2529, 1), (3372, 3), (3373, 11), (5061, 9), (5062, 2), (6000, 16))


def _record(key, value):
    from tests.test_gpu_parity_sets import _record as record_json     # the suite's JSON records
    print("simple_shapes %s: %s" % (key, value))
    record_json("simple_shapes.json", key, value)


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _ref_job(job):
    import sys as _s
    _s.path.insert(0, job[0])
    from tests import _simple_ref as r
    A, B, L, do_oti = job[1:]
    ref, shift, gap, scale = r.score_exact(A, B, L, do_oti)
    return ref, r.score_tol(A, B, L, ref), r.score_tol(A, B, L, ref, f32=True), gap / scale


@pytest.fixture(scope="module")
def refpool():
    import multiprocessing as mp
    from acoss_amd.utils import effective_cpus
    with mp.get_context("spawn").Pool(max(1, min(16, effective_cpus()))) as pool:
        yield pool


def _refs(pool, tracks, pairs, L, do_oti):
    """(exact score, f64 tolerance, f32 tolerance) per pair; asserts every OTI shift is unambiguous (a silent track's
    profile is exactly zero: its twelve OTI values tie exactly, 0 both sides, and the highest shift wins both sides)."""
    jobs = [(ROOT, tracks[i], tracks[j], L, bool(do_oti)) for i, j in pairs]
    out = np.array(pool.map(_ref_job, jobs, chunksize=1), np.float64).reshape(-1, 4)
    if do_oti:
        silent = np.array([not np.any(tracks[i]) or not np.any(tracks[j]) for i, j in pairs], bool)
        assert np.all((out[:, 3] > 1e-9) | silent), "ambiguous OTI shift in a random case"
    return out[:, 0], out[:, 1], out[:, 2]


def _check(got, ref, tol, what):
    ratio = np.abs(got - ref) / np.maximum(tol, 1e-300)
    ratio[(got == ref)] = 0.0
    bad = np.nonzero(~(ratio <= 1.0))[0]
    assert len(bad) == 0, "%s: %d pairs outside the bound, first %s: got %r exact %r bound %r" % (
        what, len(bad), bad[:5], got[bad[:3]], ref[bad[:3]], tol[bad[:3]])
    return float(ratio.max(initial=0.0))


def _run_pairs(ctx, pool, tracks, pairs, L, do_oti, what):
    fr, offs = R.pool_of(tracks)
    ctx.upload_pool_f64(fr, offs)
    got = ctx.simple_pairs(pairs, L, oti=bool(do_oti))
    ref, tol, _ = _refs(pool, tracks, pairs, L, do_oti)
    return _check(got, ref, tol, what), got


def _run_grid(ctx, pool, tracks, L, do_oti, what):
    from acoss_amd import _lib
    import oracle
    fr, offs = R.pool_of(tracks)
    ctx.upload_pool_f64(fr, offs)
    n = len(tracks)
    D = np.zeros((n, n), np.float32)
    ctx.pair_grid(_lib.ALGO_SIMPLE, False, _lib.SimpleParams(L, int(bool(do_oti))), [D], mirror=False)
    pairs = oracle.all_pairs(n, False).astype(np.int32)
    got = D[pairs[:, 0], pairs[:, 1]]
    # the grid runs the same kernel as simple_pairs: the f32 store of the same f64 score
    assert np.array_equal(got, ctx.simple_pairs(pairs, L, oti=bool(do_oti)).astype(np.float32)), what
    ref, _, tol32 = _refs(pool, tracks, pairs, L, do_oti)
    return _check(got.astype(np.float64), ref, tol32, what)


def test_every_L_simple_pairs(ctx, refpool):
    worst = {}
    for L in range(1, 17):
        for do_oti in (1, 0):
            tracks, pairs = R.every_L_case(L, do_oti)
            worst["L%d_oti%d" % (L, do_oti)] = _run_pairs(ctx, refpool, tracks, pairs, L, do_oti, "L=%d oti=%d" % (L, do_oti))[0]
    _record("every_L_simple_pairs", {"max_ratio": max(worst.values()), "per_call": worst})


def test_every_L_pair_grid(ctx, refpool):
    worst = {}
    for L in range(1, 17):
        for do_oti in (1, 0):
            tracks = R.every_L_grid_tracks(L, do_oti)
            worst["L%d_oti%d" % (L, do_oti)] = _run_grid(ctx, refpool, tracks, L, do_oti, "grid L=%d oti=%d" % (L, do_oti))
    _record("every_L_pair_grid", {"max_ratio": max(worst.values()), "per_call": worst})


def test_row_and_column_probes(ctx, refpool):
    worst = {}
    for L in R.PROBE_LS:
        tracks, pairs = R.probe_case(L)
        worst["L%d" % L] = _run_pairs(ctx, refpool, tracks, pairs, L, 0, "probes L=%d" % L)[0]
    _record("row_and_column_probes", {"max_ratio": max(worst.values()), "per_call": worst})


def test_long_tracks(ctx, refpool):
    worst = {}
    for maxn, L in LONG:
        tracks, pairs = R.long_case(maxn, L, long_pair=(maxn == 6000))
        assert max(len(t) for t in tracks) == maxn
        worst["n%d_L%d" % (maxn, L)] = _run_pairs(ctx, refpool, tracks, pairs, L, 1, "long n=%d L=%d" % (maxn, L))[0]
    _record("long_tracks", {"max_ratio": max(worst.values()), "per_call": worst})


def test_long_track_grid(ctx, refpool):
    tracks = R.long_grid_tracks()
    r = _run_grid(ctx, refpool, tracks, 10, 1, "grid with a 6000-frame track")
    _record("long_track_grid", {"max_ratio": r})


def test_chunk_boundary_pairs(ctx):
    T, pairs, L = R.chunk_pairs_case()
    fr, offs = R.pool_of(list(T))
    ctx.upload_pool_f64(fr, offs)
    got = ctx.simple_pairs(pairs, L)
    assert len(pairs) > (1 << 22)
    ref, _, _, bound = R.short_table(T, L)
    i, j = pairs[:, 0], pairs[:, 1]
    # one value per unique pair, whichever chunk and place in the sorted order it came from
    uniq = np.full(ref.shape, np.nan)
    uniq[i[::-1], j[::-1]] = got[::-1]                     # the first occurrence of every pair
    assert np.array_equal(got, uniq[i, j])
    r = _check(got, ref[i, j], bound[i, j], "simple_pairs across 2^22-pair chunks")
    _record("chunk_boundary_pairs", {"pairs": int(len(pairs)), "max_ratio": r})


def test_chunk_boundary_grid(ctx):
    from acoss_amd import _lib
    T, L = R.chunk_grid_tracks()
    n = len(T)
    assert n * (n - 1) > (1 << 22)
    fr, offs = R.pool_of(list(T))
    ctx.upload_pool_f64(fr, offs)
    D = np.zeros((n, n), np.float32)
    ctx.pair_grid(_lib.ALGO_SIMPLE, False, _lib.SimpleParams(L, 1), [D], mirror=False)
    ref, _, _, bound = R.short_table(T, L)
    off = ~np.eye(n, dtype=bool)
    assert np.all(D[~off] == 0)
    r = _check(D[off].astype(np.float64), ref[off], bound[off] + R.F32_U * (np.abs(ref[off]) + bound[off]),
               "pair_grid across 2^22-pair chunks")
    _record("chunk_boundary_grid", {"tracks": n, "pairs": int(n * (n - 1)), "max_ratio": r})


def test_oti_exact_ties(ctx):
    tracks, pairs, ties = R.tie_case()
    fr, offs = R.pool_of(tracks)
    ctx.upload_pool_f64(fr, offs)
    got = ctx.simple_pairs(pairs, 4)
    for k, ((i, j), tie) in enumerate(zip(pairs[:-1], ties[:-1])):
        # integer frames: every product and sum is exact, so is the kernel's score
        want = -float(np.median(R.profile_exact(tracks[i], tracks[j], 4, max(tie))))
        assert got[k] == want, (tie, got[k], want)
        for s in {tie[0], tie[-2]}:
            assert want != -float(np.median(R.profile_exact(tracks[i], tracks[j], 4, s)))
    i, j = pairs[-1]
    ref = R.score_exact(tracks[i], tracks[j], 4)[0]
    r = _check(got[-1:], np.array([ref]), np.array([R.score_tol(tracks[i], tracks[j], 4, ref)]), "planted pair of the tie call")
    _record("oti_exact_ties", {"max_ratio": r, "ties": [list(t) for t in ties[:-1]]})


def test_silence_and_self_pairs(ctx, refpool):
    worst = {}
    for L in (1, 10, 16):
        tracks = R.silence_tracks(3, L)
        n = len(tracks)
        pairs = np.array([(i, j) for i in range(n) for j in range(n)], np.int32)
        for do_oti in (1, 0):
            r, got = _run_pairs(ctx, refpool, tracks, pairs if do_oti == 0 else pairs[pairs[:, 0] != pairs[:, 1]], L, do_oti,
                                "silence L=%d oti=%d" % (L, do_oti))
            worst["L%d_oti%d" % (L, do_oti)] = r
        self_scores = ctx.simple_pairs(np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32), L, oti=False)
        assert self_scores[-1] == 0.0                                         # the all-zero track: exactly 0
    _record("silence_and_self_pairs", {"max_ratio": max(worst.values()), "per_call": worst})


def test_winnorm_cache(ctx, refpool):
    worst = []
    pools = R.winnorm_cache_pools()
    for k, (pool_id, L) in enumerate(((0, 10), (0, 3), (0, 10), (1, 10), (1, 3))):
        tracks = pools[pool_id]
        pairs = np.array([(i, j) for i in range(len(tracks)) for j in range(len(tracks)) if i != j], np.int32)
        worst.append(_run_pairs(ctx, refpool, tracks, pairs, L, 1, "winnorm cache step %d" % k)[0])
    _record("winnorm_cache", {"max_ratio": max(worst)})
