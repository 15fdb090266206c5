"""
CPU checks of tests/_simple_ref.py, the exact SiMPle reference of tests/test_gpu_simple_shapes.py: it agrees with
oracle.simple_sim and with the reference's own outputs (tests/golden/simple.npz), and every call the GPU tests make
would fail under each mutant of the kernel (_simple_ref.MUTANTS moves a score of the call by > 100 bounds).
"""
import numpy as np
import pytest

from tests import _simple_ref as R


def test_profile_exact_matches_oracle_within_bound():
    import oracle
    rng = np.random.default_rng(11)
    for k in range(24):
        L = int(rng.integers(1, 17))
        na, nb = int(rng.integers(L, 200)), int(rng.integers(L, 200))
        A, B = R.frames(rng, na), R.frames(rng, nb)
        s = int(rng.integers(0, 12))
        ref = -float(np.median(R.profile_exact(A, B, L, s)))
        want = -oracle.simple_sim(A.T, np.roll(B, s, axis=1).T, L)
        assert abs(ref - want) <= R.score_tol(A, B, L, ref), (k, L, na, nb, ref, want)
        got, shift, gap, scale = R.score_exact(A, B, L)
        assert shift == oracle.simple_oti(A.T, B.T)[1] or gap <= 1e-12 * scale
        assert abs(got + oracle.simple_sim(A.T, np.roll(B, shift, axis=1).T, L)) <= R.score_tol(A, B, L, got)


def test_profile_exact_reproduces_reference_goldens(golden):
    g = golden("simple")
    for k in range(6):
        A, B = g["sim_A_%d" % k].T, g["sim_B_%d" % k].T
        got, shift, gap, scale = R.score_exact(A, B, 10)
        want = -float(g["sim_out_%d" % k])
        assert gap > 1e-9 * scale
        assert abs(got - want) <= R.score_tol(A, B, 10, want), (k, got, want)
        # OTI off on the reference's own rolled B
        got2 = R.score_exact(A, g["oti_B_%d" % k].T, 10, do_oti=False)[0]
        assert abs(got2 - want) <= R.score_tol(A, B, 10, want)


def test_oti_ties_take_the_highest_shift():
    tracks, pairs, ties = R.tie_case()
    for (i, j), tie in zip(pairs[:-1], ties[:-1]):
        pa, pb = tracks[i].sum(0), tracks[j].sum(0)
        v = np.array([pa @ np.roll(pb, s) for s in range(12)])
        assert set(np.nonzero(v == v.max())[0]) == set(tie)
        assert R.oti(tracks[i], tracks[j])[0] == max(tie)
        want = -float(np.median(R.profile_exact(tracks[i], tracks[j], 4, max(tie))))
        for s in {tie[0], tie[-2]}:    # the tie matters: the lowest and the next highest tied shift give other scores
            assert -float(np.median(R.profile_exact(tracks[i], tracks[j], 4, s))) != want


def test_boundary_lengths_cover_the_kernel_edges():
    for L in range(1, 17):
        S, un = R.stride(L), R.rounds(L)
        mas, mbs = R.boundary_lengths(L)
        assert 1 in mas and 1 in mbs
        for g in (1, 2, 3):
            for e in (0, 1, S - 1):
                assert any((m - 1) % S == e and (m - 1) // S in (g - 1, g) for m in mas), (L, g, e)
        assert {m % 2 for m in mas} == {0, 1}
        # the guarded tail's length (mb - its first column): 0 and 1 without a FULL round, its least and most after one
        for tail in (0, 1):
            assert any(R.tail_start(L, mb) == 1 and mb - 1 == tail for mb in mbs), (L, tail)
        for k in (1, 2):
            for tail in {2, max(2, un - 1), un + 1}:
                assert any(R.tail_start(L, mb) == 1 + k * un and mb - R.tail_start(L, mb) == tail for mb in mbs), (L, k, tail)
        assert max(mbs) - R.tail_start(L, max(mbs)) == un + 1


@pytest.mark.parametrize("L", range(1, 17))
def test_every_L_calls_catch_every_mutant(L):
    for do_oti in (1, 0):
        tracks, pairs = R.every_L_case(L, do_oti)
        assert R.undetected(tracks, pairs, L, do_oti) == [], (L, do_oti)
        grid = R.every_L_grid_tracks(L, do_oti)
        n = len(grid)
        gp = [(i, j) for i in range(n) for j in range(n) if i != j][::-1]     # the planted pair first
        assert R.undetected(grid, gp, L, do_oti) == [], ("grid", L, do_oti)


@pytest.mark.parametrize("L", R.PROBE_LS)
def test_probe_calls_catch_every_mutant(L):
    tracks, pairs = R.probe_case(L)
    assert R.undetected(tracks, pairs, L, 0) == []
    assert set(R.probe_rows(L, 2 * R.stride(L) + R.stride(L) // 2 + 1)) >= {1}


def test_probes_hinge_on_their_row_and_column():
    """A row probe's score is ~0 or O(1) and flips if its row alone is wrong; a column probe's if its column alone is."""
    for L in R.PROBE_LS:
        S = R.stride(L)
        ma = 2 * S + S // 2 + 1
        for r in R.probe_rows(L, ma)[:6]:
            A, B = R.row_probe(5 + r, L, ma, r, positive=True)
            mp = R.profile_exact(A, B, L, 0)
            ref = -np.median(mp)
            mp[r] += 1.0
            assert abs(-np.median(mp) - ref) > 1e6 * R.score_tol(A, B, L, ref)
        mb = 3 * R.rounds(L) + 5
        for c in R.probe_cols(L, mb)[-4:]:
            A, B = R.col_probe(9 + c, L, mb, c)
            full = R.profile_exact(A, B, L, 0)
            ref = -np.median(full)
            Bc = B.copy()
            Bc[c] += 0.5                                   # column c's window changes (and its neighbours' to the left)
            bad = -np.median(R.profile_exact(A, Bc, L, 0))
            assert abs(bad - ref) > 1e6 * R.score_tol(A, B, L, ref), (L, c)


def test_long_calls_catch_every_mutant():
    from tests.test_gpu_simple_shapes import LONG
    for maxn, L in LONG:
        tracks, pairs = R.long_case(maxn, L, long_pair=(maxn == 6000))
        assert R.undetected(tracks, pairs, L, 1) == [], (maxn, L)
    assert R.undetected(R.long_grid_tracks(), [(0, 1), (1, 0), (2, 3), (3, 2)], 10, 1) == []


def test_chunk_calls_catch_every_mutant():
    T, pairs, L = R.chunk_pairs_case()
    assert len(pairs) > (1 << 22)
    assert R.undetected(list(T), pairs[:64], L, 1) == []
    T, L = R.chunk_grid_tracks()
    assert len(T) * (len(T) - 1) > (1 << 22)
    assert R.undetected(list(T[:8]), [(i, j) for i in range(8) for j in range(8) if i != j], L, 1) == []
    ref, sh, gap, bound = R.short_table(T[:50], L)
    for i, j in [(0, 1), (3, 7), (49, 2)]:
        got, s, _, _ = R.score_exact(T[i], T[j], L)
        assert s == sh[i, j] and abs(got - ref[i, j]) <= bound[i, j]


def test_other_calls_catch_every_mutant():
    tracks, pairs, _ = R.tie_case()
    assert R.undetected(tracks, pairs, 4, 1) == []
    for L in (1, 10, 16):
        tracks = R.silence_tracks(3, L)
        n = len(tracks)
        for do_oti in (1, 0):
            pairs = [(i, j) for i in range(n) for j in range(n) if do_oti == 0 or i != j]
            assert R.undetected(tracks, pairs, L, do_oti) == [], (L, do_oti)
    pools = R.winnorm_cache_pools()
    for p in pools:
        for L in (10, 3):
            assert R.undetected(p, [(i, j) for i in range(4) for j in range(4) if i != j], L, 1) == []
