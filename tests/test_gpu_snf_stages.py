"""
GPU suite: every kernel of snf_kernels.hpp per stage, and both gather variants of the update.

acx_snf_debug_stages / acx_snf_debug_update launch the kernels through the host functions the product launches them with and
hand back what each one wrote.  Every stage is compared with the specification (tests/_snf_ref.py, pinned to the oracle by
tests/test_snf_ref.py) evaluated on the DEVICE'S OWN previous stage, so that an error cannot hide behind twenty sweeps of
averaging, and each bound is the rounding budget of that one kernel:

  S    bit-identical
  md   (take + 3) 2^-53 (K + 1) / K mean(|the take cells|)
  W    the argument of the exponential is bit-identical by construction; device exp against libm: rtol 1e-12, and
       4 x 2^-1074 absolute for denormal results (each exp within one ulp of the true value, one more rounding where the
       device scales the result into the denormal range, rounded up to a power of two; a relative bound means nothing there)
  J    identical to the stable descending argsort of the device's W
  V    (K + 1) 2^-53 sum|v| / |sum v| relative ((K + 1) 2^-53 where all weights are >= 0)
  P    (n + 1) 2^-53 sum|row| / |rowsum| relative
  acc  (m_src + 1) 2^-53 sum|terms|;  UT, P of the update: (K + 2) 2^-53 sum_k |V a| (+ one rounding on the diagonal)

Every hold prints the worst ratio of the error to its bound (pytest -s); DESIGN.md section 23 records them.
"""
import ctypes

import numpy as np
import pytest

from . import _snf_ref as ref

pytestmark = pytest.mark.gpu

NS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
LD = np.longdouble
DENORMAL_ATOL = 4 * 2.0 ** -1074


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _ks(n):
    return sorted({min(max(k, 1), min(n, 64)) for k in (1, 2, 20, 63, 64, n - 2, n - 1, n)})


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _hold(name, got, want, bound):
    """|got - want| <= bound per cell (want in longdouble); prints the worst ratio before it asserts."""
    err = np.abs(np.asarray(got, LD) - want).astype(np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    exact_ok = bool(np.all(err[~pos] == 0))
    print("SNF-HOLD %-28s worst error / bound = %.3f" % (name, ratio))
    assert np.all(np.isfinite(err)), name
    assert exact_ok, "%s: cells with a zero bound differ" % name
    assert ratio <= 1.0, "%s: error %.3f of its bound" % (name, ratio)
    return ratio


def _ulps(got, want):
    """Largest distance in units of the last place between positive normal values of two arrays."""
    sel = (want >= 2.0 ** -1022) & np.isfinite(want) & np.isfinite(got) & (got >= 2.0 ** -1022)
    if not sel.any():
        return 0
    return int(np.abs(_bits(got[sel]).astype(np.int64) - _bits(want[sel]).astype(np.int64)).max())


def _check_lists(tag, out, W, K):
    """J, V, P of the device against the specification on the device's own W."""
    n = W.shape[0]
    J, V, rel = ref.knn(W, K)
    assert np.array_equal(out["J"], J), "%s: J differs in rows %s" % (tag, np.nonzero((out["J"] != J).any(1))[0][:8])
    _hold(tag + " V", out["V"], V, rel[:, None] * np.abs(ref.f64(V)))
    P, relp = ref.rownorm(W)
    _hold(tag + " P", out["P"], P, relp[:, None] * np.abs(ref.f64(P)))
    assert out["V"].shape == (n, K)


@pytest.mark.parametrize("n", NS)
def test_stages_from_distances(ctx, n):
    """All five kernels on a non-symmetric matrix with a non-zero diagonal whose symmetrised rows are random, duplicates (distance
    0 to several columns, ties at the cut), negative with -0.0 beside +0.0, and all equal: each stage from the device's previous one."""
    worst = 0
    for K in _ks(n):
        tag = "n=%d K=%d" % (n, K)
        D = ref.crafted_distances(n, K)
        out = ctx.snf_debug_stages(D, K)
        assert _same_bits(out["S"], ref.sym(D)), tag
        md, bound = ref.localscale(out["S"], K)
        _hold(tag + " md", out["md"], md, bound)
        W = ref.affinity(out["S"], out["md"])
        worst = max(worst, _ulps(out["W"], W))
        np.testing.assert_allclose(out["W"], W, rtol=1e-12, atol=DENORMAL_ATOL, err_msg=tag)
        _check_lists(tag, out, out["W"], K)
    print("SNF-ULPS n=%d worst distance of W from libm's exp: %d ulps" % (n, worst))


@pytest.mark.parametrize("mu", (0.5, 0.05))
def test_affinity_at_the_ends_of_exp(ctx, mu):
    """Identical tracks (md_i = md_j = d = 0: the zero denominator becomes 1 and W = 1) beside arguments down to
    -4.5 / mu^2 = -1800: results through the denormal range to 0."""
    n, K = 257, 3
    rng = np.random.default_rng(3)
    D = rng.random((n, n)) * 3 + 0.01
    for g in range(0, 64, 4):                     # sixteen cliques of K + 1 identical tracks: md = 0
        D[g:g + 4, g:g + 4] = 0
    out = ctx.snf_debug_stages(D, K, mu=mu)
    assert _same_bits(out["S"], ref.sym(D)) and np.all(out["md"][:64] == 0) and np.all(out["md"][64:] > 0)
    arg = ref.affinity_arg(out["S"], out["md"], mu)
    W = np.exp(arg)
    for g in range(0, 64, 4):
        assert np.all(out["W"][g:g + 4, g:g + 4] == 1.0)
    if mu < 0.1:
        assert np.sum(arg < -700) > 100 and np.sum((W > 0) & (W < 2.0 ** -1022)) >= 8 and np.sum(W == 0) > 100
    tiny = (W < 2.0 ** -1022) | (out["W"] < 2.0 ** -1022)
    print("SNF-ULPS mu=%g worst distance of W from libm's exp: %d ulps; denormal cells %d, worst %g x 2^-1074" % (
        mu, _ulps(out["W"], W), np.sum((W > 0) & (W < 2.0 ** -1022)),
        float(np.abs(out["W"] - W)[tiny].max() / 2.0 ** -1074) if tiny.any() else 0.0))
    np.testing.assert_allclose(out["W"], W, rtol=1e-12, atol=DENORMAL_ATOL)
    _check_lists("ends mu=%g" % mu, out, out["W"], K)


@pytest.mark.parametrize("n", (133, 200, 257))
def test_crafted_affinity_rows(ctx, n):
    """from_stage = 1: rows made for every exit of the selection -- ties in columns 60..70 and 124..132 with neq_left running out
    inside a 64-column group, on its last column and on the next group's first; all cells equal (ngt = 0); exactly K above a crowd
    of ties (neq_left = 0); the K largest in the last, partial group; zeros; denormals; a last-bit difference at the cut; signed."""
    for K in (1, 2, 5, 20, 63, 64):
        tag = "crafted n=%d K=%d" % (n, K)
        W, names = ref.crafted_affinity(n, K)
        out = ctx.snf_debug_stages(W, K, from_stage=1)
        assert out["S"] is None and out["md"] is None and _same_bits(out["W"], W)
        J = ref.knn(W, K)[0]
        bad = sorted({names[r] for r in np.nonzero((out["J"] != J).any(1))[0]})
        assert not bad, "%s: J differs in the families %s" % (tag, bad)
        _check_lists(tag, out, W, K)
        zero = names.index("zeros")
        assert np.all(out["V"][zero] == 0) and np.all(out["P"][zero] == 0)


def _update_ks(n):
    return sorted({min(k, n) for k in (1, 20, 64, 65, min(n, 200))})


def _some_rows(n, rng):
    """All rows up to n = 129; beyond, the rows at the ends and around the 256-row marks plus 32 random ones (every row is a
    workgroup of its own; the variants are still compared on all rows)."""
    if n <= 129:
        return np.arange(n)
    fixed = [r for r in (0, 1, 2, 3, 63, 64, 255, 256, 257, 511, 512, n - 2, n - 1) if r < n]
    return np.unique(np.concatenate([fixed, rng.integers(0, n, 32)]))


@pytest.mark.parametrize("m_src", (1, 2, 3, 7, 8))
@pytest.mark.parametrize("n", NS)
def test_one_update(ctx, n, m_src):
    """acc, UT and P of one update against the longdouble specification, each from the device's previous stage; both gather
    variants give the same bits (the same terms in the same order)."""
    rng = np.random.default_rng(n * 10 + m_src)
    rows = _some_rows(n, rng)
    for idx, K in enumerate(_update_ks(n)):
        reg, signed = float((idx + m_src) & 1), bool(((idx + m_src) >> 1) & 1)
        tag = "update n=%d m=%d K=%d reg=%g %s" % (n, m_src, K, reg, "signed" if signed else "nonneg")
        srcs, J, V = ref.crafted_update(n, m_src, K, signed)
        scale = 1.0 / 3.0
        acc, ut, p = ctx.snf_debug_update(srcs, scale, J, V, reg, variant=1)
        acc2, ut2, p2 = ctx.snf_debug_update(srcs, scale, J, V, reg, variant=2)
        assert _same_bits(acc, acc2) and _same_bits(ut, ut2) and _same_bits(p, p2), tag
        acc0, ut0, p0 = ctx.snf_debug_update(srcs, scale, J, V, reg, variant=0, rows=rows)
        assert _same_bits(acc0, acc[rows]) and _same_bits(ut0, ut[rows]) and _same_bits(p0, p[rows]), tag
        want, bound = ref.mean(srcs, scale)
        _hold(tag + " acc", acc, want, bound)
        want, bound = ref.ast(acc[rows], J, V)
        _hold(tag + " UT", ut[rows], want, bound)
        want, bound = ref.sut(ut, J, V, reg, rows)
        _hold(tag + " P", p[rows], want, bound)


def test_both_regs_and_signs_occur():
    seen = {(float((idx + m) & 1), bool(((idx + m) >> 1) & 1)) for m in (1, 2, 3, 7, 8) for idx in range(5)}
    assert seen == {(0.0, False), (0.0, True), (1.0, False), (1.0, True)}


def test_row_beyond_64_kib_of_lds(ctx):
    """n = 8193: the first row that needs the opt-in dynamic LDS size.  The product's choice (the row in LDS) and the gathers
    from global memory give the same bits, and the requested rows are the specification's (K^2 gathers per cell on the host)."""
    n, K = 8193, 3
    rng = np.random.default_rng(8193)
    A = rng.random((n, n))
    J = rng.integers(0, n, (n, K)).astype(np.int32)
    J[:, 0] = np.arange(n)[::-1]                                  # every column is gathered, the last one by row 0
    V = rng.random((n, K)) + 1e-3
    V /= V.sum(1)[:, None]
    rows = np.unique(np.concatenate([[0, 1, 255, 256, 4096, 8191, 8192], rng.integers(0, n, 25)])).astype(np.int32)
    acc, ut, p = ctx.snf_debug_update([A], 0.5, J, V, 1.0, variant=0, rows=rows)
    acc2, ut2, p2 = ctx.snf_debug_update([A], 0.5, J, V, 1.0, variant=2, rows=rows)
    assert _same_bits(acc, acc2) and _same_bits(ut, ut2) and _same_bits(p, p2)
    mean = A[rows] * 0.5
    assert _same_bits(acc, mean)                                  # one source: 0 + a, then the exact halving
    want, bound = ref.ast(mean, J, V)
    _hold("n=8193 UT", ut, want, bound)
    A *= 0.5
    want, bound = ref.update_cells(A, J, V, 1.0, rows)
    _hold("n=8193 P", p, want, bound)


def _scores(rng, n, m):
    out = []
    for _ in range(m):
        D = rng.random((n, n)) * 3
        lab = rng.integers(0, max(2, n // 5), n)
        D[lab[:, None] == lab[None, :]] *= 0.3
        out.append(D)
    return out


def test_eight_matrices(ctx):
    """m = 8 fills SnfSrc: seven sources in a sweep, eight in the final mean."""
    import oracle
    Scores = _scores(np.random.default_rng(8), 65, 8)
    Ws_o, want = oracle.snf_fuse(Scores, K=20, niters=3, reg_diag=1)
    np.testing.assert_allclose(ctx.snf_fuse_dists(Scores, K=20, niters=3, reg_diag=1.0)[1], want, rtol=1e-10, atol=1e-14)
    lists = [oracle.snf_knn_lists(W, 20) for W in Ws_o]
    got = ctx.snf_fuse(Ws_o, [l[0] for l in lists], [l[1] for l in lists], 3, 1.0)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("K", (65, 200))
def test_more_than_64_neighbours_from_the_caller(ctx, K):
    import oracle
    Scores = _scores(np.random.default_rng(K), 257, 2)
    Ws_o, want = oracle.snf_fuse(Scores, K=K, niters=2, reg_diag=1)
    lists = [oracle.snf_knn_lists(W, K) for W in Ws_o]
    got = ctx.snf_fuse(Ws_o, [l[0] for l in lists], [l[1] for l in lists], 2, 1.0)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-14)


@pytest.mark.parametrize("K", (32, 33))
def test_every_column_a_neighbour(ctx, K):
    """K = n - 1 and K = n at n = 33: take = min(K + 1, n) = n.  The oracle raises there (np.partition out of bounds), so the
    composed specification says what the device returns.  Random distances: a whole run can only be compared where no two
    affinities of a row lie within a rounding of each other at the cut (the device's exp and libm's differ in the last bits)."""
    Ds = _scores(np.random.default_rng(K), 33, 3)
    Ws, want = ref.fuse(Ds, K, 3, 1)
    Ws_d, got = ctx.snf_fuse_dists(Ds, K=K, niters=3, reg_diag=1.0, want_ws=True)
    for a, b in zip(Ws, Ws_d):
        np.testing.assert_allclose(b, a, rtol=1e-12, atol=DENORMAL_ATOL)
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-14)


def test_errors(ctx):
    from acoss_amd import _lib
    rng = np.random.default_rng(0)
    D = rng.random((70, 70))
    with pytest.raises(NotImplementedError):
        ctx.snf_fuse_dists([D, D], K=65)                                       # one candidate per lane
    with pytest.raises(NotImplementedError):
        ctx.snf_debug_stages(D, 65)
    with pytest.raises(NotImplementedError):
        ctx.snf_debug_stages(D, 65, from_stage=1)
    with pytest.raises(ValueError):
        ctx.snf_fuse_dists([D] * 9, K=5)                                       # SnfSrc holds 8 pointers
    with pytest.raises(ValueError):
        ctx.snf_fuse_dists([D[:8, :8]] * 2, K=9)                               # K = n + 1
    with pytest.raises(ValueError):
        ctx.snf_debug_stages(D[:8, :8], 9)
    J = np.zeros((8, 3), np.int32)
    V = np.ones((8, 3))
    with pytest.raises(ValueError):
        ctx.snf_debug_update([D[:8, :8]] * 9, 1.0, J, V)
    with pytest.raises(ValueError):
        ctx.snf_debug_update([D[:8, :8]], 1.0, J + 8, V)                       # neighbour index out of range
    with pytest.raises(ValueError):
        ctx.snf_debug_update([D[:8, :8]], 1.0, J, V, rows=[8])
    with pytest.raises(ValueError):
        ctx.snf_debug_update([D[:8, :8]], 1.0, J, V, variant=3)
    # variant 1 where a row no longer fits the LDS (n = 20 353): refused at the argument check, before any array of that size is
    # read -- so the call can be made with n alone and small arrays behind the pointers
    small = np.zeros(16)
    ptrs = (ctypes.c_void_p * 1)(small.ctypes.data)
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    assert ctx._L.acx_snf_debug_update(ctx._h, ptrs, 1, 20353, 1, 1.0, J.ctypes.data_as(ip), V.ctypes.data_as(dp), 0.0, 1,
                                       None, 0, None, None, None) == _lib.ACX_ERR_UNSUPPORTED


def test_one_infinite_distance(ctx):
    """ChenFusion.normalize_by_length writes +inf where a score is 0.  One off-diagonal +inf: W is NaN in that cell and its mirror
    -- the oracle's cells -- and the oracle's W everywhere else.  Nothing is asserted about the fused matrix of such input (the
    reference's is NaN throughout)."""
    import oracle
    n, K = 65, 20
    D = np.random.default_rng(6).random((n, n)) * 3
    D[7, 40] = np.inf
    with np.errstate(invalid="ignore"):
        want = oracle.snf_getW(np.array(D), K)
    assert int(np.isnan(want).sum()) == 2 and np.isnan(want[7, 40]) and np.isnan(want[40, 7])
    out = ctx.snf_debug_stages(D, K)
    assert np.array_equal(np.isnan(out["W"]), np.isnan(want))
    ok = ~np.isnan(want)
    np.testing.assert_allclose(out["W"][ok], want[ok], rtol=1e-12, atol=DENORMAL_ATOL)
    # The lists of the two rows that hold a NaN: K distinct columns in range, every slot written (the export fills the lists
    # with -1 first).  snf_key ranks a NaN by its sign bit: first of the row (above +inf) or last (below every value, not listed).
    # Ranked as doubles, the NaN and the row's largest value both took slot 0 and slot K - 1 kept whatever the block held:
    # a column index that snf_ast_kernel would gather from.
    J = out["J"]
    assert J.min() >= 0 and J.max() < n and all(len(set(r)) == K for r in J)
    for i, j in ((7, 40), (40, 7)):
        assert J[i, 0] == j or j not in J[i], (i, J[i])
        keep = [c for c in J[i] if c != j]
        rest = out["W"][i].copy()
        rest[j] = -1.0
        assert keep == list(np.argsort(-rest, kind="stable")[:len(keep)])
    rows = np.setdiff1d(np.arange(n), [7, 40])
    assert np.array_equal(J[rows], ref.knn(out["W"], K)[0][rows])
