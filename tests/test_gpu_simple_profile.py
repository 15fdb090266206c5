"""
The SiMPle matrix profile, its index and the matched section on the device: simple_profile_kernel<L> through acx_simple_profile
and Simple.align / profile / align_matches, against tests/_simple_profile_ref.py.

  continuous data (every_L_case for L = 1..16 with and without OTI, probe_case for PROBE_LS, the long tracks): score == the f64
    bits of acx_simple_pairs, shift == the reference's, |MP - exact| <= score_bound in every row, MPI == the exact first
    minimum in every row (every row is decided: tests/test_simple_profile_ref.py, and asserted again here from the gaps),
    the record == the summary of the device's own MP and MPI, its run == the reference's
  integer data (tests/_simple_profile_ref.py EXACT_CASES at L = 1, 2, 10, 11, 16): MP, MPI and every field of the record equal
    the reference bit for bit, tie order included
  long tracks: the first maxn with 3, 2 and 1 waves per workgroup and 6000; a mixed list in the caller's order and reversed;
    two chunks under a lowered scratch limit == one chunk
  summary-only calls == the records of profile calls; cap one short, and every other refusal, launch nothing
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _simple_ref as R                  # noqa: E402
from tests import _simple_profile_ref as P          # noqa: E402


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _ref_job(job):
    import sys as _s
    _s.path.insert(0, job[0])
    from tests import _simple_profile_ref as p
    return p.reference(*job[1:])


@pytest.fixture(scope="module")
def refpool():
    import multiprocessing as mp
    from acoss_amd.utils import effective_cpus
    with mp.get_context("spawn").Pool(max(1, min(16, effective_cpus()))) as pool:
        yield pool


def _refs(pool, tracks, pairs, L, do_oti):
    return pool.map(_ref_job, [(ROOT, tracks[i], tracks[j], L, bool(do_oti)) for i, j in pairs], chunksize=1)


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _call(ctx, tracks, pairs, L, do_oti, upload=True):
    """One profile call and its summary-only twin: (records, [MP_k], [MPI_k]); the twin's records, the offsets and the scores
    of acx_simple_pairs are checked here."""
    if upload:
        ctx.upload_pool_f64(*R.pool_of(tracks))
    al, off, mp, mpi = ctx.simple_profile(pairs, L, oti=bool(do_oti), profiles=True)
    assert al.tobytes() == ctx.simple_profile(pairs, L, oti=bool(do_oti)).tobytes(), "summary-only records differ"
    ma = np.array([len(tracks[i]) - L + 1 for i, _ in pairs], np.int64)
    assert off[0] == 0 and np.array_equal(np.diff(off), ma) and len(mp) == len(mpi) == off[-1]
    assert mp.dtype == np.float64 and mpi.dtype == np.int32
    assert np.array_equal(_bits(al["score"]), _bits(ctx.simple_pairs(pairs, L, oti=bool(do_oti)))), "score bits differ from acx_simple_pairs"
    K = len(pairs)
    return al, [mp[off[k]:off[k + 1]] for k in range(K)], [mpi[off[k]:off[k + 1]] for k in range(K)]


def _check_continuous(got, refs, L, what):
    """Returns the largest |MP - exact| / bound and the smallest gap / bound seen."""
    al, mps, mpis = got
    worst, tightest = 0.0, np.inf
    for k, (mp, mpi, gap, s, bound) in enumerate(refs):
        w = "%s pair %d" % (what, k)
        assert al["shift"][k] == s["shift"], w
        err = np.abs(mps[k] - mp)
        assert np.all(err <= bound), (w, float(err.max()), bound)
        assert np.all(gap > 2.0 * bound), (w, "undecided rows", int(np.sum(~(gap > 2.0 * bound))))
        assert np.array_equal(mpis[k], mpi), (w, np.nonzero(mpis[k] != mpi)[0][:5])
        rec = P.record_of(al[k])
        own = P.summary(mps[k], mpis[k], L, s["shift"])
        assert P.same_record(rec, own), (w, rec, own)
        for f in ("q0", "r0", "q1", "r1", "run_len", "q_span", "r_span"):
            assert rec[f] == s[f], (w, f, rec[f], s[f])
        worst, tightest = max(worst, float(err.max()) / bound), min(tightest, float(gap.min()) / bound)
    return worst, tightest


def _check_exact(got, refs, names, what):
    al, mps, mpis = got
    for k, (mp, mpi, _, s, _) in enumerate(refs):
        w = "%s %s" % (what, names[k])
        assert np.array_equal(_bits(mps[k]), _bits(mp)), (w, np.nonzero(mps[k] != mp)[0][:5])
        assert np.array_equal(mpis[k], mpi), (w, np.nonzero(mpis[k] != mpi)[0][:5], mpis[k][:8], mpi[:8])
        assert P.same_record(P.record_of(al[k]), s), (w, P.record_of(al[k]), s)


@pytest.mark.parametrize("L", range(1, 17))
def test_every_L(ctx, refpool, L):
    for do_oti in (1, 0):
        tracks, pairs = R.every_L_case(L, do_oti)
        worst, tight = _check_continuous(_call(ctx, tracks, pairs, L, do_oti), _refs(refpool, tracks, pairs, L, do_oti), L,
                                         "L=%d oti=%d" % (L, do_oti))
        print("simple_profile every_L L=%d oti=%d: %d pairs, max |MP - exact| / bound %.3g, smallest gap %.3g bounds" % (L, do_oti, len(pairs), worst, tight))


@pytest.mark.parametrize("L", R.PROBE_LS)
def test_row_and_column_probes(ctx, refpool, L):
    tracks, pairs = R.probe_case(L)
    worst, tight = _check_continuous(_call(ctx, tracks, pairs, L, 0), _refs(refpool, tracks, pairs, L, 0), L, "probes L=%d" % L)
    print("simple_profile probes L=%d: %d pairs, max |MP - exact| / bound %.3g, smallest gap %.3g bounds" % (L, len(pairs), worst, tight))


@pytest.mark.parametrize("L", P.EXACT_LS)
def test_exact_integer_cases(ctx, refpool, L):
    tracks, pairs, names = P.exact_pool(L)
    for do_oti in (0, 1):
        _check_exact(_call(ctx, tracks, pairs, L, do_oti), _refs(refpool, tracks, pairs, L, do_oti), names, "exact L=%d oti=%d" % (L, do_oti))


LONG_LS = (10, 3, 11)


def _long_cases():
    steps = P.step_lengths()
    assert [P.waves_per_workgroup(n) for n in steps] == [3, 2, 1]
    return list(zip(steps, LONG_LS)) + [(6000, 16)]


@pytest.mark.parametrize("which", range(4))
def test_long_tracks(ctx, refpool, which):
    maxn, L = _long_cases()[which]
    tracks, pairs = R.long_case(maxn, L, long_pair=(maxn == 6000))
    assert max(len(t) for t in tracks) == maxn
    worst, tight = _check_continuous(_call(ctx, tracks, pairs, L, 1), _refs(refpool, tracks, pairs, L, 1), L, "long n=%d L=%d" % (maxn, L))
    print("simple_profile long n=%d L=%d (%d waves per workgroup): max |MP - exact| / bound %.3g, smallest gap %.3g bounds" % (
        maxn, L, P.waves_per_workgroup(maxn), worst, tight))


def _mixed():
    """Short pairs of every_L_case next to one long track (2 waves per workgroup), the second tracks in no order."""
    L = 10
    tracks, pairs = R.every_L_case(L, 1)
    tracks = list(tracks) + [R.frames(np.random.default_rng(77), P.step_lengths()[1] + 3)]
    n = len(tracks) - 1
    pairs = np.concatenate([pairs[::-1][:9], [[n, 0], [3, n], [n, 5]], pairs[:7]]).astype(np.int32)
    return tracks, pairs, L


def test_mixed_list_in_order_and_reversed(ctx, refpool):
    tracks, pairs, L = _mixed()
    fwd = _call(ctx, tracks, pairs, L, 1)
    _check_continuous(fwd, _refs(refpool, tracks, pairs, L, 1), L, "mixed")
    rev = _call(ctx, tracks, pairs[::-1].copy(), L, 1, upload=False)
    assert fwd[0].tobytes() == rev[0][::-1].tobytes()
    for k in range(len(pairs)):
        assert np.array_equal(_bits(fwd[1][k]), _bits(rev[1][len(pairs) - 1 - k])) and np.array_equal(fwd[2][k], rev[2][len(pairs) - 1 - k])


def _launches(ctx, name="simple_profile_kernel"):
    return ctx.profile()[name]["launches"]


def test_two_chunks_equal_one(ctx):
    tracks, pairs, L = _mixed()
    ctx.upload_pool_f64(*R.pool_of(tracks))
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        one = ctx.simple_profile(pairs, L, profiles=True)
        assert _launches(ctx) == 1
        rows = np.array([len(tracks[i]) - L + 1 for i, _ in pairs], np.int64)
        # 12 bytes per row on the device: a limit that holds all but the last few pairs
        ctx.set_scratch_limit(int(12 * (rows.sum() - rows[-3:].sum())))
        ctx.profile_reset()
        two = ctx.simple_profile(pairs, L, profiles=True)
        assert _launches(ctx) == 2
        for a, b in zip(one, two):
            assert a.tobytes() == b.tobytes()
        # summary-only calls hold no profiles on the device: one launch under the same limit
        ctx.profile_reset()
        assert ctx.simple_profile(pairs, L).tobytes() == one[0].tobytes() and _launches(ctx) == 1
        # a single pair beyond the limit: refused before the first launch
        ctx.set_scratch_limit(int(12 * (rows.max() - 1)))
        ctx.profile_reset()
        with pytest.raises(MemoryError, match="scratch limit"):
            ctx.simple_profile(pairs, L, profiles=True)
        assert all(v["launches"] == 0 for v in ctx.profile().values())
    finally:
        ctx.set_scratch_limit(0)
        ctx.profile_enable(False)


def _raw(ctx, pairs, L, oti, out, off, mp, mpi, cap):
    pairs = np.ascontiguousarray(pairs, np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data          # noqa: E731
    rc = ctx._L.acx_simple_profile(ctx._h, pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(pairs), L, oti, ptr(out), ptr(off),
                                   ptr(mp), ptr(mpi), cap)
    return rc, (ctx._L.acx_last_error(ctx._h) or b"").decode()


def test_refusals_launch_nothing(ctx):
    from acoss_amd import _lib
    rng = np.random.default_rng(5)
    tracks = [R.frames(rng, n) for n in (9, 40, 57, 6001, 33)]
    ctx.upload_pool_f64(*R.pool_of(tracks))
    L = 10
    pairs = np.array([[1, 2], [2, 4], [4, 1]], np.int32)
    need = sum(len(tracks[i]) - L + 1 for i, _ in pairs)
    out = np.zeros(3, _lib.SIMPLE_ALIGNMENT_DTYPE)
    off, mp, mpi = np.zeros(4, np.int64), np.zeros(need, np.float64), np.zeros(need, np.int32)
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        rc, msg = _raw(ctx, pairs, L, 1, out, off, mp, mpi, need - 1)          # cap one element short
        assert rc == _lib.ACX_ERR_INVALID and str(need) in msg and "cap" in msg, (rc, msg)
        for a in ((None, mp, mpi), (off, None, mpi), (off, mp, None), (off, None, None)):   # some but not all of the three
            rc, msg = _raw(ctx, pairs, L, 1, out, *a, need)
            assert rc == _lib.ACX_ERR_INVALID and "all" in msg, (rc, msg)
        assert _raw(ctx, pairs, L, 1, None, None, None, None, 0)[0] == _lib.ACX_ERR_INVALID
        assert _raw(ctx, pairs, L, 1, out, off, mp, mpi, -1)[0] == _lib.ACX_ERR_INVALID
        rc, msg = _raw(ctx, np.array([[1, 2], [2, 5]], np.int32), L, 1, out, off, mp, mpi, need)
        assert rc == _lib.ACX_ERR_INVALID and "out of range in pair 1" in msg, (rc, msg)
        assert _raw(ctx, np.array([[-1, 2]], np.int32), L, 1, out, None, None, None, 0)[0] == _lib.ACX_ERR_INVALID
        rc, msg = _raw(ctx, np.array([[1, 2], [0, 1]], np.int32), L, 1, out, off, mp, mpi, need)
        assert rc == _lib.ACX_ERR_SHORT and "shorter than SSLEN (pair 1)" in msg, (rc, msg)
        rc, msg = _raw(ctx, np.array([[1, 3]], np.int32), L, 1, out, None, None, None, 0)
        assert rc == _lib.ACX_ERR_UNSUPPORTED and "6000" in msg, (rc, msg)
        for bad in (0, 17, -3):
            rc, msg = _raw(ctx, pairs, bad, 1, out, None, None, None, 0)
            assert rc == _lib.ACX_ERR_UNSUPPORTED and "1..16" in msg, (bad, rc, msg)
        assert all(v["launches"] == 0 for v in ctx.profile().values()), ctx.profile()
        # K = 0 is an empty answer; a valid call after the refusals succeeds, with its own profile entry
        assert _raw(ctx, np.zeros((0, 2), np.int32), L, 1, None, off, mp, mpi, need)[0] == 0 and off[0] == 0
        rc, msg = _raw(ctx, pairs, L, 1, out, off, mp, mpi, need)
        assert rc == 0 and off[-1] == need, (rc, msg)
        prof = ctx.profile()
        assert prof["simple_profile_kernel"]["launches"] == 1 and prof["simple_profile_kernel"]["cells"] == 3 and prof["simple_profile_kernel"]["ms"] > 0
        assert prof["simple_kernel"]["launches"] == 0
        assert np.array_equal(_bits(out["score"]), _bits(ctx.simple_pairs(pairs, L)))
    finally:
        ctx.profile_enable(False)
    # no pool uploaded: a fresh context
    c2 = _lib.Context(0)
    try:
        rc, msg = _raw(c2, pairs, L, 1, out, None, None, None, 0)
        assert rc == _lib.ACX_ERR_STATE and "not uploaded" in msg, (rc, msg)
    finally:
        c2.close()


def test_class_methods(tmp_path, monkeypatch):
    """Simple.align / profile / align_matches on a small synthetic cover set, empty slots included."""
    import oracle
    from acoss_amd import synth
    from acoss_amd.algorithms import Simple
    monkeypatch.chdir(tmp_path)
    d = synth.cover_set(n_works=3, versions=2, seed=21, t_range=(2600, 5200))
    n = len(d["offsets"]) - 1
    feats = [oracle.simple_features(d["frames"][d["offsets"][i]:d["offsets"][i + 1]]) for i in range(n)]
    with open(tmp_path / "ds.csv", "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("%s,t%d\n" % (d["labels"][i], i))
    a = Simple(str(tmp_path / "ds.csv"), "feat/", shortname="prof")
    try:
        a.set_features(feats, list(d["labels"]))
        L = a.SSLEN
        pairs = np.array([(i, j) for i in range(n) for j in range(n) if i != j][:14], np.int32)
        al = a.align(pairs)
        al2, mps, mpis = a.profile(pairs)
        assert al.dtype == a.ALIGN_DTYPE and al.shape == (len(pairs),) and al.tobytes() == al2.tobytes()
        ctx = a._context()
        assert np.array_equal(_bits(al["score"]), _bits(ctx.simple_pairs(pairs, L)))
        tracks = [np.ascontiguousarray(f.T) for f in feats]
        for k, (i, j) in enumerate(pairs):
            mp, mpi, gap, s, bound = P.reference(tracks[i], tracks[j], L, True)
            assert mps[k].shape == mpis[k].shape == (len(tracks[i]) - L + 1,) and mpis[k].dtype == np.int32
            assert np.all(np.abs(mps[k] - mp) <= bound) and al["shift"][k] == s["shift"]
            dec = gap > 2.0 * bound
            assert np.array_equal(mpis[k][dec], mpi[dec])
            assert P.same_record(P.record_of(al[k]), P.summary(mps[k], mpis[k], L, s["shift"]))
            assert al["run_len"][k] >= 1 and al["q_span"][k][1] == al["q1"][k] + L - 1 < len(tracks[i])
            assert al["r_span"][k][1] == al["r1"][k] + L - 1 < len(tracks[j])
        # the hits of identify(), a slot emptied by hand, and a row with fewer candidates than k
        queries = np.array([4, 0, 2])
        idx = a.identify(queries, k=3)["main"][0]
        idx[1, 2] = -1
        got = a.align_matches(queries, idx)
        assert got.shape == idx.shape and got.dtype == a.ALIGN_DTYPE
        for r in range(len(queries)):
            for s_ in range(idx.shape[1]):
                g = got[r, s_]
                if idx[r, s_] < 0:
                    assert g["run_len"] == 0 and np.isnan(g["score"]) and np.isnan(g["best_dist"])
                    assert all(g[f] == -1 for f in ("best_q", "best_r", "q0", "r0", "q1", "r1")) and np.all(g["q_span"] == -1) and np.all(g["r_span"] == -1)
                else:
                    assert g.tobytes() == a.align(np.array([[queries[r], idx[r, s_]]]))[0].tobytes()
        few = a.identify([1], k=n + 2)["main"][0]
        assert np.sum(few < 0) == 3 and np.sum(a.align_matches([1], few)["run_len"] == 0) == 3
        assert a.align(np.zeros((0, 2), np.int64)).shape == (0,) and a.profile([])[1:] == ([], [])
    finally:
        a.cleanup_memmap()
