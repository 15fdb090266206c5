"""
GPU: the full cross-diffusion early fusion (acoss_amd/csrc/ef_crossfusion_kernels.hpp), every stage
held on the DEVICE'S OWN previous stage against tests/_crossfusion_ref.py, as section 23 holds the SNF kernels.

  r, c     (k + 1) 2^-53 mean(|the taken cells|) of the specification: k - 1 additions in any order and a division
  W        cross blocks: the argument of the exponential is bit-identical by construction (numpy's operations under
           -ffp-contract=off, evaluated here on the device's r and c); device exp against libm: rtol 1e-12; the two cross
           blocks each other's transpose bit for bit.  Diagonal blocks: bit-identical to what acx_snf_debug_stages leaves for
           the same f64 matrix and K = k1 / k2 -- the same three kernels, which tests/test_gpu_snf_stages.py holds
  D        rtol 1e-10, atol 1e-14 against the specification run on the device's W
  X        bit-identical to the one addition on the device's D
  bits     identical to the first k of the stable descending argsort of the device's X, pad bits zero
  score    the oracle's Smith-Waterman on the device's bits, and acx_sw_bits_binary on them
"""
import os

import numpy as np
import pytest

from . import _crossfusion_ref as ref
from . import _snf_ref as snf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(5, 40), (12, 30), (30, 12), (40, 33), (63, 66), (64, 65), (127, 130), (120, 1024)]
K, KAPPA, REG = 10, 0.1, 1.0
DENORMAL_ATOL = 4 * 2.0 ** -1074


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _walk(rng, n, width):
    return np.cumsum(rng.standard_normal((n, width)) * 0.3, axis=0) + rng.standard_normal(width)


def _triple(M, N, seed=0):
    """Three feature spaces, two smooth tracks with a shared stretch: SA (3, M, M), SB (3, N, N), C (3, M, N) f32."""
    import oracle
    rng = np.random.default_rng(7000 * M + N + seed)
    SA, SB, C = [], [], []
    for f, width in enumerate((20, 30, 24)):
        A, B = _walk(rng, M, width), _walk(rng, N, width)
        L = max(2, min(M, N) // 2)
        B[:L] = A[M - L:] + rng.standard_normal((L, width)) * 0.05
        if f == 2:
            A, B = np.abs(A), np.abs(B)
        A, B = A.astype(np.float32), B.astype(np.float32)
        dist = oracle.get_csm_cosine if f == 2 else oracle.get_csm
        SA.append(dist(A, A)); SB.append(dist(B, B)); C.append(dist(A, B))
    return np.stack(SA).astype(np.float32), np.stack(SB).astype(np.float32), np.stack(C).astype(np.float32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _score_eq(got, want):
    return round(float(got) * 10) == round(float(want) * 10)


def _check_stages(ctx, SA, SB, C, Kn, niters, kappa, tag):
    import oracle
    M, N = C.shape[1:]
    k1, k2 = ref.split(M, N, Kn)
    out = ctx.crossfusion_matrices(SA, SB, C, kappa=kappa, K=Kn, niters=niters, reg_diag=REG)
    worst = dict(r=0.0, c=0.0, W=0.0)
    for f in range(3):
        r, c, rb, cb = ref.means(C[f], k2, k1)
        er = np.abs(out["r"][f] - r).astype(np.float64)
        ec = np.abs(out["c"][f] - c).astype(np.float64)
        worst["r"] = max(worst["r"], float(np.max(er / np.maximum(rb, 5e-324))))
        worst["c"] = max(worst["c"], float(np.max(ec / np.maximum(cb, 5e-324))))
        assert np.all(er <= rb), (tag, f, "r")
        assert np.all(ec <= cb), (tag, f, "c")
        W = out["W"][f]
        want = np.exp(ref.cross_arg(C[f], out["r"][f], out["c"][f]))
        up = W[:M, M:]
        ok = want > 0
        if ok.any():
            worst["W"] = max(worst["W"], float(np.max(np.abs(up[ok] - want[ok]) / want[ok])) / 1e-12)
        np.testing.assert_allclose(up, want, rtol=1e-12, atol=DENORMAL_ATOL, err_msg="%s W cross %d" % (tag, f))
        assert _same_bits(np.ascontiguousarray(W[M:, :M]), np.ascontiguousarray(up.T)), (tag, f, "the cross blocks are not transposes")
        for S, kk, at, m in ((SA[f], k1, 0, M), (SB[f], k2, M, N)):
            stage = ctx.snf_debug_stages(S.astype(np.float64), kk, mu=0.5)
            assert _same_bits(np.ascontiguousarray(W[at:at + m, at:at + m]), stage["W"]), (tag, f, at, "diagonal block")
    Dw = ref.fuse_ws([out["W"][f] for f in range(3)], Kn, niters, REG)
    eD = float(np.max(np.abs(out["D"] - Dw) / (1e-10 * np.abs(Dw) + 1e-14)))
    np.testing.assert_allclose(out["D"], Dw, rtol=1e-10, atol=1e-14, err_msg=tag + " D")
    assert _same_bits(out["X"], ref.x_of(out["D"], M)), (tag, "X")
    k = ref.binary_k(kappa, N)
    B = ref.select(out["X"], k)
    assert np.array_equal(out["bits"], ref.pack_bits(B)), (tag, "bits")
    assert _score_eq(out["score"], oracle.sw_constrained(B)), (tag, out["score"], oracle.sw_constrained(B))
    assert _score_eq(out["score"], ctx.sw_bits_binary(B)), tag
    print("%s: k1 = %d, k2 = %d, k = %d; worst error over bound: r %.3g, c %.3g, W(cross) %.3g, D %.3g; score %g"
          % (tag, k1, k2, k, worst["r"], worst["c"], worst["W"], eD, out["score"]))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_stages_on_random_triples(ctx, shape):
    M, N = shape
    SA, SB, C = _triple(M, N)
    # (120, 1024): two sweeps -- the second is the one whose work lists alias -- keep the numpy specification at n = 1144 quick
    _check_stages(ctx, SA, SB, C, K, 5 if M + N <= 300 else 2, KAPPA, "random %dx%d" % shape)


def test_stages_with_k1_k2_at_their_limit(ctx):
    """K = 20 at (12, 12): k1 = k2 = 10 = M - 2, the largest the rule admits (np.partition's K + 1 = M - 1 is the last index)."""
    SA, SB, C = _triple(12, 12, seed=3)
    assert ref.split(12, 12, 20) == (10, 10)
    _check_stages(ctx, SA, SB, C, 20, 5, KAPPA, "random 12x12 K=20")


@pytest.fixture(scope="module")
def golden_xf():
    g = np.load(os.path.join(ROOT, "tests", "golden", "crossfusion.npz"))
    return {k: g[k] for k in g.files}


@pytest.mark.parametrize("shape", [(12, 30), (40, 33), (64, 65)], ids=["12x30", "40x33", "64x65"])
def test_golden_inputs_stage_by_stage_and_end_to_end(ctx, golden_xf, shape):
    """The reference's own W and D within section 23's figures, its plot and score exactly: every row's gap at the cut of X is at
    least 1e-6 (re-asserted), far above what rtol 1e-10 moves."""
    g = golden_xf
    tag = "%dx%d_" % shape
    out = _check_stages(ctx, g[tag + "SA"], g[tag + "SB"], g[tag + "C"], int(g["K"]), int(g["niters"]), float(g["kappa"]), "golden %dx%d" % shape)
    np.testing.assert_allclose(out["W"], g[tag + "W"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(out["D"], g[tag + "D"], rtol=1e-10, atol=1e-14)
    assert ref.cut_gap(g[tag + "X"], ref.binary_k(float(g["kappa"]), shape[1])).min() >= 1e-6
    B, pad = ref.unpack_bits(out["bits"], shape[1])
    assert np.array_equal(B, g[tag + "B"]) and not pad.any()
    assert _score_eq(out["score"], float(g[tag + "score"]))


# ------------------------------------------------------------------ the selection alone on crafted rows

def _crafted_rows(N, k, rng):
    """One row per way the selection can exit; names for the messages."""
    rows, names = [], []
    edge = [c for c in (0, 31, 32, 62, 63, 64, 65, 127, 128, N - 1) if 0 <= c < N]

    def put(name, row):
        rows.append(np.asarray(row, np.float64)); names.append(name)

    for ngt in sorted({0, max(k - 2, 0), max(k - 1, 0)}):
        row = rng.random(N) * 0.25                                   # the tie value across the slot edge at column 63 / 64 and at the rims
        row[edge] = 0.5
        free = np.setdiff1d(np.arange(N), edge)
        take = min(ngt, len(free))
        row[rng.choice(free, take, replace=False)] = 0.75 + rng.random(take)
        put("ties_with_%d_above" % take, row)
    row = np.full(N, 0.125)                                          # exactly k cells above a crowd of ties
    row[rng.choice(N, min(k, N), replace=False)] = 1.0 + rng.random(min(k, N))
    put("exactly_k_above", row)
    put("all_equal", np.full(N, 0.375))
    row = rng.permutation(N) / float(N) + 0.25                       # the k-th and the (k + 1)-th value one bit apart
    order = np.argsort(-row, kind="stable")
    if 0 < k < N:
        row[order[k]] = np.nextafter(row[order[k - 1]], 0.0)
    put("one_bit_apart", row)
    row = -rng.random(N) - 0.5                                       # negative values, -0.0 beside +0.0 at the cut
    z = rng.choice(N, min(N, max(k + 2, 3)), replace=False)
    row[z] = np.where(np.arange(len(z)) % 2 == 0, -0.0, 0.0)
    if k >= 2:
        row[z[0]] = 2.0
    put("signed_zeros", row)
    put("random", rng.standard_normal(N))
    return np.stack(rows), names


@pytest.mark.parametrize("N", [4, 5, 63, 64, 65, 1023, 1024])
def test_selection_on_crafted_rows(ctx, N):
    import oracle
    rng = np.random.default_rng(100 + N)
    for kappa in ((0.5, 0.1) if N < 10 else (0.1, 0.02, 0.0)):
        k = ref.binary_k(kappa, N)
        X, names = _crafted_rows(N, k, rng)
        bits, score = ctx.xsel_binary_sw(X, kappa=kappa)
        B = ref.select(X, k)
        want = ref.pack_bits(B)
        for i, name in enumerate(names):
            assert np.array_equal(bits[i], want[i]), (N, kappa, k, name)
        assert B.sum(1).tolist() == [min(k, N)] * len(X)
        assert _score_eq(score, oracle.sw_constrained(B)), (N, kappa)
        if k == 0:
            assert not bits.any() and score == 0.0               # an empty plot
    assert ref.binary_k(0.1, 4) == 0 and ref.binary_k(0.0, 1024) == 1024


# ------------------------------------------------------------------ the product path

BLOCKS = [5, 12, 30, 64, 65, 1024, 4, 40, 1025]
WIDTHS = (40, 100, 96)
VALID = np.array([[1, 2], [2, 1], [3, 4], [0, 7], [5, 5], [2, 3], [4, 3], [7, 2]], np.int32)


@pytest.fixture(scope="module")
def pool(ctx):
    rng = np.random.default_rng(77)
    tracks = []
    for nb in BLOCKS:
        ch = np.abs(_walk(rng, nb, WIDTHS[2])).astype(np.float32)
        tracks.append(dict(mfccs=_walk(rng, nb, WIDTHS[0]).astype(np.float32), ssms=np.abs(_walk(rng, nb, WIDTHS[1])).astype(np.float32),
                           chromas=ch, chroma_med=rng.random(12) ** 2))
    # a planted excerpt: track 4 carries a stretch of track 3
    for key in ("mfccs", "ssms", "chromas"):
        tracks[4][key][10:50] = tracks[3][key][5:45] + (rng.standard_normal(tracks[3][key][5:45].shape) * 0.02).astype(np.float32)
    tracks[4]["chromas"] = np.abs(tracks[4]["chromas"])
    ctx.ef_upload_pool(tracks)
    return tracks


def test_product_path_matrices_are_the_gemm_paths(ctx, pool):
    """csm / ssm_a / ssm_b are the matrices acx_ef_debug_pair returns for (i, j), (i, i), (j, j), bit for bit; the self pairs within
    the bound tests/test_gpu_earlyfusion.py holds every pair to (its _check_pair, imported: the bound is not copied)."""
    from .test_gpu_earlyfusion import _check_pair
    for i, j in ((1, 2), (3, 4), (0, 7)):
        d = ctx.ef_crossfusion_debug(i, j, kappa=KAPPA, K=K, niters=5)
        assert np.array_equal(d["csm"], ctx.ef_debug_pair(i, j)["csm"]), (i, j)
        for t, key in ((i, "ssm_a"), (j, "ssm_b")):
            # (_check_pair runs the oracle's getWCSM with K = 10, which np.partition refuses for a track of 5 blocks)
            one = _check_pair(ctx, t, t, pool[t], pool[t]) if BLOCKS[t] > 10 else ctx.ef_debug_pair(t, t)
            assert one["oti"] == 0
            assert np.array_equal(d[key], one["csm"]), (i, j, key)
        M, N = BLOCKS[i], BLOCKS[j]
        # the chain behind the GEMMs is the one the matrices entry runs: the same intermediates from the same matrices
        m = ctx.crossfusion_matrices(d["ssm_a"], d["ssm_b"], d["csm"], kappa=KAPPA, K=K, niters=5)
        for key in ("W", "D", "X"):
            assert _same_bits(d[key], m[key]), (i, j, key)
        assert np.array_equal(d["bits"], m["bits"]) and d["score"] == m["score"]
        assert d["X"].shape == (M, N)


def test_product_path_lists(ctx, pool):
    got = ctx.ef_crossfusion(VALID, kappa=KAPPA, K=K, niters=5)
    assert got.shape == (len(VALID),) and got.dtype == np.float32
    back = ctx.ef_crossfusion(VALID[::-1], kappa=KAPPA, K=K, niters=5)
    assert np.array_equal(back[::-1], got)
    for k_, (i, j) in enumerate(VALID[:4]):
        assert ctx.ef_crossfusion([[i, j]], kappa=KAPPA, K=K, niters=5)[0] == got[k_], (i, j)       # whatever shares its list
        assert ctx.ef_crossfusion_debug(int(i), int(j), kappa=KAPPA, K=K, niters=5)["score"] == got[k_], (i, j)
    assert ctx.ef_crossfusion(np.zeros((0, 2), np.int32)).shape == (0,)
    early = ctx.earlyfusion_pairs(np.array([[3, 4], [2, 3]], np.int32), kappa=KAPPA, K=K)[:, 3]
    print("planted excerpt (3, 4): full fusion %g beside early %g; unrelated (2, 3): full fusion %g beside early %g"
          % (got[2], early[0], got[5], early[1]))


def test_refusals_launch_nothing(ctx, pool):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        with pytest.raises(NotImplementedError, match=r"pair 2: 4 x 40 blocks with K = 10 give k1 = 0, k2 = 10"):
            ctx.ef_crossfusion([[1, 2], [3, 4], [6, 7], [2, 3]], kappa=KAPPA, K=K, niters=5)
        with pytest.raises(NotImplementedError, match=r"at most 1024 blocks \(pair 1: 30 x 1025\)"):
            ctx.ef_crossfusion([[1, 2], [2, 8]], kappa=KAPPA, K=K, niters=5)
        with pytest.raises(NotImplementedError, match="more than 64 neighbours"):
            ctx.ef_crossfusion(VALID, kappa=KAPPA, K=65, niters=5)
        with pytest.raises(ValueError, match="niters must be >= 1"):
            ctx.ef_crossfusion(VALID, kappa=KAPPA, K=K, niters=0)
        with pytest.raises(ValueError, match="track index out of range in pair 1"):
            ctx.ef_crossfusion([[1, 2], [2, 9]], kappa=KAPPA, K=K, niters=5)
        with pytest.raises(NotImplementedError, match="k1 = 0"):
            ctx.ef_crossfusion_debug(6, 7, kappa=KAPPA, K=K, niters=5)
        SA, SB, C = np.zeros((3, 4, 4), np.float32), np.zeros((3, 40, 40), np.float32), np.zeros((3, 4, 40), np.float32)
        with pytest.raises(NotImplementedError, match="k1 = 0"):
            ctx.crossfusion_matrices(SA, SB, C, K=K)
        with pytest.raises(NotImplementedError, match="more than 1024 rows or columns"):
            ctx.xsel_binary_sw(np.zeros((4, 1025)))
        # none of these refusals launched anything: no call has run since the reset
        assert all(v["launches"] == 0 for v in ctx.profile().values()), ctx.profile()
        # a valid call afterwards succeeds, and the profile names the new kernels
        got = ctx.ef_crossfusion(VALID[:2], kappa=KAPPA, K=K, niters=5)
        assert np.isfinite(got).all()
        prof = ctx.profile()
        for name in ("xf_means_kernel", "xf_affinity_kernels", "xf_snf_kernels", "xf_x_kernel", "xf_select_kernel"):
            assert prof[name]["launches"] >= 2 and prof[name]["ms"] > 0, (name, prof[name])
        assert list(prof)[-1] == "ef_align_kernel"
    finally:
        ctx.profile_enable(False)


def test_without_a_pool():
    from acoss_amd import _lib
    c = _lib.Context(0)
    try:
        with pytest.raises(_lib.AcxError, match="pool not uploaded"):
            c.ef_crossfusion([[0, 1]])
    finally:
        c.close()


# ------------------------------------------------------------------ Python

def test_full_fusion_and_rerank_full(tmp_path, monkeypatch):
    from acoss_amd import synth
    from acoss_amd.algorithms.earlyfusion_traile import EarlyFusion
    tracks = synth.earlyfusion_set(6, seed=31, nb_range=(40, 90))
    monkeypatch.chdir(tmp_path)
    with open("ds.csv", "w") as f:
        f.write("work_id,track_id\n")
        for i in range(6):
            f.write("w%d,t%d\n" % (i // 2, i))
    ef = EarlyFusion("ds.csv", "feat/", shortname="toy")
    ef.set_block_features(tracks)
    pairs = np.array([[0, 1], [2, 5], [5, 2], [3, 4]])
    got = ef.full_fusion(pairs)
    assert got.shape == (4,) and got.dtype == np.float32
    c = ef._context()
    for k_, (i, j) in enumerate(pairs):
        assert c.ef_crossfusion_debug(int(i), int(j), kappa=ef.kappa, K=ef.K, niters=ef.niters)["score"] == got[k_]
    before = {s: ef.Ds[s].copy() for s in ef.Ds}
    q = np.array([0, 3, 5])
    lists = ef.identify(q, k=4, similarity_types=["early"])["early"][0]
    lists[1, 3] = -1                                                  # an empty slot
    lists[2, 0] = 5                                                   # the query's own track: skipped
    idx, score = ef.rerank_full(q, lists, k=4)
    assert idx.shape == (3, 4) and idx.dtype == np.int32 and score.shape == (3, 4) and score.dtype == np.float32
    for r in range(3):
        cand = [int(v) for v in lists[r] if v >= 0 and v != q[r]]
        sc = ef.full_fusion([[min(q[r], v), max(q[r], v)] for v in cand])               # the cell (min, max)
        order = sorted(range(len(cand)), key=lambda t: (-float(sc[t]), cand[t]))[:4]       # score descending, then smaller index
        assert idx[r, :len(order)].tolist() == [cand[t] for t in order], r
        assert np.array_equal(score[r, :len(order)], sc[order]), r
        assert (idx[r, len(order):] == -1).all() and np.isnan(score[r, len(order):]).all(), r
    assert len([v for v in lists[1] if v >= 0]) == 3 and idx[1, 3] == -1
    assert all(np.array_equal(ef.Ds[s], before[s], equal_nan=True) for s in before)     # Ds is not written
