"""CPU suite: the numpy specification of the EarlyFusion back end (tests/_ef_backend_ref.py) is the oracle's csm_to_binary,
the neighbourhood means inside the oracle's get_wcsm and the oracle's Smith-Waterman -- and the wrong variants a kernel could
compute instead (tie column excluded, threshold one rank up, pad bits set, a mean over one cell more, column means taken
over rows, an alignment that reads the last column) all differ from it on these inputs, so the GPU tests that compare
against it can tell them apart."""
import numpy as np

import oracle

from . import _ef_backend_ref as ref

KAPPAS = (0.1, 0.05, 0.5, 0.0, 3)


def _matrices():
    rng = np.random.default_rng(5)
    out = []
    for n in list(range(1, 41)):
        m = int(rng.integers(1, 20))
        kind = n % 5
        if kind == 0:
            C = rng.integers(0, 4, (m, n)).astype(np.float32)                   # few distinct values
        elif kind == 1:
            C = np.tile(rng.random((m, 1)).astype(np.float32), (1, n))          # constant rows
        elif kind == 2:
            C = np.ones((m, n), np.float32)                                     # saturated: most cells exactly 1.0f
            hits = rng.random((m, n)) < 0.1
            C[hits] = rng.random(int(hits.sum())).astype(np.float32)
        elif kind == 3:
            C = (np.round(rng.random((m, n)) * 8) / 8).astype(np.float32)
        else:
            C = rng.random((m, n)).astype(np.float32)
        out.append(C)
    out.append(rng.integers(0, 3, (12, 12)).astype(np.float32))               # square: the axes of r and c can be told apart
    out.append(rng.random((25, 25)).astype(np.float32))
    return out


def test_half_to_even_and_empty_rows_occur():
    ks = {n: oracle.binary_k(0.1, n) for n in range(1, 41)}
    assert ks[4] == 0 and ks[5] == 0 and ks[15] == 2 and ks[25] == 2 and ks[35] == 4       # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    assert oracle.binary_k(0.5, 5) == 2 and oracle.binary_k(0.0, 7) == 7 and oracle.binary_k(3, 2) == 3


def test_bitmap_is_the_oracles_csm_to_binary():
    seen_ties = seen_empty = seen_full = 0
    for C in _matrices():
        M, N = C.shape
        for kappa in KAPPAS:
            kb = oracle.binary_k(kappa, N)
            t, jcut = ref.thresholds(C, kb)
            B = ref.binarise(C, t, jcut)
            assert np.array_equal(B, oracle.csm_to_binary(C, kappa)), (C.shape, kappa)
            assert np.all(B.sum(1) == min(max(kb, 0), N))
            if 0 < kb < N:
                assert np.all(np.any(C == t[:, None], axis=1))                      # an element of the row
                assert np.all(np.sum(C <= t[:, None], 1) >= kb) and np.all(np.sum(C < t[:, None], 1) < kb)
            seen_ties += int(np.sum(jcut != ref.JCUT_ALL))
            seen_empty += kb <= 0
            seen_full += kb >= N
            W = ref.pack_bits(B)
            back, pad = ref.unpack_bits(W, N)
            assert W.shape == (M, ref.pitch_words(N)) and np.array_equal(back, B) and pad == 0
    assert seen_ties > 100 and seen_empty > 5 and seen_full > 40


def test_means_are_the_neighbourhood_means_of_get_wcsm():
    for C in _matrices():
        M, N = C.shape
        for K in (1, 3, 10):
            r, rs = ref.mean_smallest(C, K, 1)
            c, cs = ref.mean_smallest(C, K, 0)
            assert r.shape == (M,) and c.shape == (N,) and np.all(rs >= np.abs(r) - 1e-12) and np.all(cs >= np.abs(c) - 1e-12)
            if K < N and K < M:                                      # (np.partition inside get_wcsm needs K < both sides)
                m1 = np.mean(np.partition(C, K, 1)[:, 0:K], 1)        # similarity_fusion.py:42-45, as the oracle has them
                m2 = np.mean(np.partition(C, K, 0)[0:K, :], 0)
                np.testing.assert_allclose(r, m1, rtol=2e-6, atol=1e-7)
                np.testing.assert_allclose(c, m2, rtol=2e-6, atol=1e-7)
                C64 = C.astype(np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    eps = (r[:, None] + c[None, :] + C64) / 3
                    W = np.exp(-C64 ** 2 / (2 * (0.5 * eps) ** 2))
                    Wo = oracle.get_wcsm(C, K, K)
                ok = np.isfinite(W) & np.isfinite(Wo)
                np.testing.assert_allclose(W[ok], Wo[ok], rtol=1e-3, atol=1e-6)


def test_sw_tenths_is_the_oracles_alignment():
    rng = np.random.default_rng(3)
    for (m, n) in [(1, 9), (3, 3), (4, 4), (4, 5), (5, 4), (7, 9), (16, 33), (40, 12), (65, 70)]:
        for dens in (0.05, 0.3, 0.8, 1.0):
            B = (rng.random((m, n)) < dens).astype(np.uint8)
            assert ref.sw_tenths(B) == oracle.sw_constrained_i32(B) == round(oracle.sw_constrained(B) * 10), (m, n, dens)
    assert ref.sw_tenths(np.eye(50, dtype=np.uint8)) == 10 * 47


def test_the_wrong_variants_differ_on_these_inputs():
    differs = dict(tie_column_excluded=0, threshold_one_rank_up=0, pad_bits_set=0, mean_of_one_more=0, c_over_rows=0, last_column_counts=0)
    j_ = lambda C: np.arange(C.shape[1])[None, :]
    for C in _matrices():
        M, N = C.shape
        for kappa in KAPPAS:
            kb = oracle.binary_k(kappa, N)
            t, jcut = ref.thresholds(C, kb)
            B = ref.binarise(C, t, jcut)
            wrong = ((C < t[:, None]) | ((C == t[:, None]) & (j_(C) < jcut[:, None]))).astype(np.uint8)
            differs["tie_column_excluded"] += not np.array_equal(wrong, B)
            if 0 < kb < N - 1:
                t2 = np.sort(C, axis=1)[:, kb]
                differs["threshold_one_rank_up"] += not np.array_equal(t2.view(np.uint32), t.view(np.uint32))
            full = np.ones((M, 32 * ref.pitch_words(N)), np.uint8)
            full[:, :N] = B
            padded = np.packbits(full, axis=1, bitorder="little").view(np.uint32).reshape(M, -1)
            differs["pad_bits_set"] += not np.array_equal(padded, ref.pack_bits(B))
            if M >= 4 and N >= 4:
                differs["last_column_counts"] += ref.sw_tenths(np.pad(B, ((0, 0), (0, 1)))) != ref.sw_tenths(B)
        for K in (1, 10):
            r, rs = ref.mean_smallest(C, K, 1)
            r1, _ = ref.mean_smallest(C, K + 1, 1)
            differs["mean_of_one_more"] += bool(np.any(np.abs(r1 - r) > ref.mean_bound(K, N, rs)))
            if M == N:
                c, cs = ref.mean_smallest(C, K, 0)
                differs["c_over_rows"] += bool(np.any(np.abs(r - c) > ref.mean_bound(K, M, cs)))
    assert all(v > 0 for v in differs.values()), differs
