"""CPU suite: the numpy specification of the SNF kernels (tests/_snf_ref.py) is the oracle's snf_getW, snf_knn_lists and
snf_fuse -- on the reference's golden and on random inputs, stage by stage and composed into a whole fusion -- and each wrong
variant a kernel could compute instead (the tie taken from the last column, the cut one rank up, the diagonal excluded from the
K + 1 smallest, the (K + 1) / K factor dropped, a mean over all m matrices, S^T for S in the second product, reg_diag off the
diagonal) differs from it on at least one of the crafted inputs the GPU tests use, so those tests can tell them apart."""
import numpy as np
import pytest

import oracle

from . import _snf_ref as ref


def _random_scores(rng, n, m):
    out = []
    for _ in range(m):
        D = rng.random((n, n)) * 3
        lab = rng.integers(0, max(2, n // 5), n)
        D[lab[:, None] == lab[None, :]] *= 0.3
        out.append(D)
    return out


def _cases(golden):
    rng = np.random.default_rng(11)
    yield list(golden("snf")["Ds"]), 5, 4
    yield _random_scores(rng, 23, 2), 3, 2
    yield _random_scores(rng, 41, 3), 20, 3
    yield [ref.crafted_distances(37, s) for s in range(3)], 7, 2


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).nmant >= 63


def test_stages_are_the_oracle(golden):
    for Ds, K, _ in _cases(golden):
        for D in Ds:
            n = D.shape[0]
            S = ref.sym(D)
            md, bound = ref.localscale(S, K)
            Neighbs = np.partition(S, K + 1, 1)[:, 0:K + 1]                      # snf_getW's own lines
            want_md = np.mean(Neighbs, 1) * float(K + 1) / float(K)
            assert np.all(np.abs(ref.f64(md) - want_md) <= bound + 1e-300)
            # with the oracle's MeanDist the argument and W are the oracle's, bit for bit
            W = ref.affinity(S, want_md)
            assert np.array_equal(W, oracle.snf_getW(np.array(D), K))
            J, V, rel = ref.knn(W, K)
            Jo, Vo = oracle.snf_knn_lists(W, K)
            assert np.array_equal(J, Jo)
            assert np.all(np.abs(ref.f64(V) - Vo) <= rel[:, None] * Vo)
            P, relp = ref.rownorm(W)
            assert np.all(np.abs(ref.f64(P) - W / W.sum(1)[:, None]) <= relp[:, None] * np.abs(ref.f64(P)))
            assert n == W.shape[0]


def test_golden_affinities(golden):
    g = golden("snf")
    Ws, F = ref.fuse(list(g["Ds"]), 5, 4, 1)
    np.testing.assert_allclose(np.stack(Ws), g["Ws"], rtol=1e-12)
    np.testing.assert_allclose(F, g["F"], rtol=1e-10, atol=1e-12)


def test_composed_fusion_is_the_oracle(golden):
    for Ds, K, niters in _cases(golden):
        for reg in (1, 0):
            Ws_o, want = oracle.snf_fuse(Ds, K=K, niters=niters, reg_diag=reg)
            Ws, got = ref.fuse(Ds, K, niters, reg)
            for a, b in zip(Ws_o, Ws):
                np.testing.assert_allclose(b, a, rtol=1e-12, atol=1e-300)
            np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-14)


def test_one_update_is_the_oracles_dense_product():
    for n, m_src, K, signed in ((9, 1, 3, True), (33, 3, 20, False), (65, 7, 65, True)):
        srcs, J, V = ref.crafted_update(n, m_src, K, signed)
        S = np.zeros((n, n))
        np.add.at(S, (np.repeat(np.arange(n), K), J.ravel()), V.ravel())
        A = sum(srcs) * 0.25
        want = S.dot(S.dot(A.T).T) + np.eye(n)                                   # oracle.snf_fuse's line
        np.testing.assert_allclose(ref.update(srcs, 0.25, J, V, 1.0), want, rtol=1e-10, atol=1e-12)
        rows = np.array([0, n // 2, n - 1])
        p, bound = ref.update_cells(ref.f64(ref.mean(srcs, 0.25)[0]), J, V, 1.0, rows)
        assert np.all(np.abs(ref.f64(p) - ref.update(srcs, 0.25, J, V, 1.0)[rows]) <= bound)


def test_the_spec_is_defined_where_the_oracle_raises():
    D = ref.crafted_distances(33)
    for K in (32, 33):
        with pytest.raises(ValueError):
            oracle.snf_getW(np.array(D), K)
        md, _ = ref.localscale(ref.sym(D), K)
        assert np.all(np.isfinite(ref.f64(md)))
        assert np.all(np.isfinite(ref.fuse([D, D.T * 0.5], K, 2, 1)[1]))


def _crafted_runs():
    """The crafted inputs of tests/test_gpu_snf_stages.py at sizes the CPU handles in a moment: (name, callable(wrong) -> arrays)."""
    runs = []
    for n, K in ((65, 20), (33, 2), (5, 1)):
        D = ref.crafted_distances(n)
        runs.append(("md n=%d K=%d" % (n, K), lambda w, D=D, K=K: [ref.f64(ref.localscale(
            ref.sym(D), K, skip_diagonal=w == "diagonal_excluded", drop_factor=w == "factor_dropped")[0])]))
    for n, K in ((200, 20), (200, 2), (133, 64)):
        W, _ = ref.crafted_affinity(n, K)
        runs.append(("knn n=%d K=%d" % (n, K), lambda w, W=W, K=K: [ref.knn(
            W, K, tie_last=w == "tie_last", shift=1 if w == "cut_one_up" else 0)[0]]))
    for n, m_src, K, signed in ((33, 2, 20, True), (65, 3, 1, False)):
        srcs, J, V = ref.crafted_update(n, m_src, K, signed)
        runs.append(("update n=%d" % n, lambda w, a=(srcs, 0.5, J, V, 1.0): [ref.update(*a, wrong=w)]))
    Ds = [ref.crafted_distances(17, s) for s in range(3)]
    runs.append(("fuse n=17 m=3", lambda w: [ref.fuse(Ds, 4, 2, 1, wrong=w)[1]]))
    return runs


def test_every_wrong_variant_differs_on_a_crafted_input():
    runs = _crafted_runs()
    right = {name: f(None) for name, f in runs}
    caught = {w: [name for name, f in runs if any(not np.array_equal(a, b) for a, b in zip(f(w), right[name]))]
              for w in ref.WRONG_VARIANTS}
    assert all(caught.values()), caught
    # ... and no crafted input is idle: each one rejects a wrong variant
    for name, _ in runs:
        assert any(name in names for names in caught.values()), (name, caught)


def test_crafted_affinity_rows_exit_where_they_say():
    """The tie rows do put the end of neq_left where their name says: inside a 64-column group, on its last column, on the next
    group's first."""
    n, K = 200, 20
    W, names = ref.crafted_affinity(n, K)
    J, _, _ = ref.knn(W, K)
    last_tie = {}
    for r, name in enumerate(names):
        if name.startswith("ties"):
            t = int(name[4:])
            taken = sorted(c for c in J[r] if c in ref.TIE_COLUMNS)
            assert len(taken) == t and taken == ref.TIE_COLUMNS[:t], (name, taken)
            last_tie[t] = taken[-1]
    assert [last_tie[t] for t in ref.NEQ_TARGETS] == [61, 63, 64, 125, 127, 128]
    assert {"all_equal", "exact_k_above", "last_group", "zeros", "denormals", "last_bit", "signed"} <= set(names)
    r = names.index("last_group")
    assert J[r].min() >= n - K and n - K > 128
    r = names.index("last_bit")
    v = np.sort(W[r])[::-1]
    assert v[K] == np.nextafter(v[K - 1], 0.0)
    D = ref.crafted_distances(65)
    S = ref.sym(D)
    assert np.any(np.signbit(S) & (S == 0)) and np.any(S < 0) and np.any(D != D.T) and np.all(np.diag(D) != 0)
    assert np.array_equal(S, S.T)
