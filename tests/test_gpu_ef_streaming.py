"""
EarlyFusion beyond 1024 blocks: the streaming kernels (ef_rowstat_long_kernel modes 0 / 1 / 2, sw_long_kernel, and ef_colstat_kernel /
ef_fuse_kernel on more than 1024 rows) held per row and per cell against tests/_ef_backend_ref.py, on the inputs of
tests/_ef_streaming_cases.py (tests/test_ef_streaming_design.py shows on the CPU what those inputs can see):

  A  sw_long_kernel on caller bitmaps (sw_binary): paths planted into the first two columns of every strip, penalised values
     across the seam, one to six strips, last strips of one to three columns, scores beyond 16 bits.  Exact.
  B  ef_rowstat_long_kernel mode 0 on crafted matrices (csm_debug_bits): the families of test_gpu_ef_backend.py as long rows and
     as short rows of a tall matrix, a tie family at the edges of the 64-column groups, stale pad columns.
  C  the product path on a pool with tracks of 1025 and 1100 blocks, every configuration.
  D  a pair's statistics and scores do not depend on what shares its batch, across the 1024-block limit too.

Bars as in test_gpu_ef_backend.py: t (bit patterns), jcut and scores exact; r and c within ref.mean_bound of the f64 mean.
"""
import numpy as np
import pytest

from . import _ef_backend_ref as ref
from . import _ef_streaming_cases as S
from .test_gpu_ef_backend import (FAMILIES, KAPPAS, _all_ordered_pairs, _check_product_pair, _check_slot, _mean_ratio, _pool, _sw,
                                  _tenths)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------------------------
# A. sw_long_kernel on caller bitmaps
# ------------------------------------------------------------------------------------------------------------------
def test_planted_paths_into_the_first_columns_of_every_strip(ctx):
    """The only best alignment enters column c and c + 1 of the seams c = 1024, 2048, 3072 by a (1,1), a (1,2) and a (2,1) step, at
    an even and an odd row -- lane 0's three values of the record, U[i-1][c-1], U[i-1][c-2], U[i-2][c-1] -- and runs through one
    hole at c - 2 .. c + 1 and two astride the seam (a U that includes the -7 in the record)."""
    cases = S.planted_cases()
    for name, B, cells, field in cases:
        want = ref.sw_tenths(B)
        assert want > 300
        assert _tenths(ctx.sw_binary(B)) == want, (name, field)
        assert _tenths(ctx.sw_binary(np.ascontiguousarray(B[:, :B.shape[1] - 17]))) == ref.sw_tenths(B[:, :B.shape[1] - 17]), name
    print("%d planted plots" % len(cases))


@pytest.mark.parametrize("m", S.RIM_M)
def test_strip_counts_and_last_strips(ctx, m):
    """One to six strips (the ring of two records reused up to five times) and last strips of one, two and three columns, on all
    ones, all zeros and random plots; m = 4: the row loop runs once, on the records of rows 0 and 1."""
    for n in S.RIM_N:
        for kind in S.RIM_PLOTS:
            B = S.rim_plot(kind, m, n)
            assert _tenths(ctx.sw_binary(B)) == ref.sw_tenths(B), (kind, m, n)


def test_scores_beyond_16_bits_and_the_dispatch_rim(ctx):
    """np.eye(3400) scores 33 970 tenths; all ones at 40 x 4100; and beyond 1024 rows with few columns the caller's plot takes
    sw_kernel<8>: the rim of the dispatch from its other side."""
    eye = np.eye(3400, dtype=np.uint8)
    assert _tenths(ctx.sw_binary(eye)) == ref.sw_tenths(eye) == 33970
    ones = np.ones((40, 4100), np.uint8)
    assert _tenths(ctx.sw_binary(ones)) == ref.sw_tenths(ones)
    rng = np.random.default_rng(17)
    for (m, n) in [(1025, 8), (2500, 30)]:
        for dens in (0.3, 0.8):
            B = (rng.random((m, n)) < dens).astype(np.uint8)
            assert _tenths(ctx.sw_binary(B)) == _sw(B), (m, n, dens)


# ------------------------------------------------------------------------------------------------------------------
# B. ef_rowstat_long_kernel, mode 0, on crafted matrices
# ------------------------------------------------------------------------------------------------------------------
def _check_matrix(ctx, C, kappa, kb, Ks, where, want_score=None):
    """t, jcut, r and the score of one caller's matrix beyond 1024 rows or columns; returns the worst r error / bound."""
    wt, wj = ref.thresholds(C, kb)
    if want_score is None:
        want_score = ref.sw_tenths(ref.binarise(C, wt, wj))
    worst = 0.0
    for K in Ks:
        d = ctx.csm_debug_bits(C, kappa, K)
        assert d["bits"] is None
        _check_slot(C, kb, d["t"], d["jcut"], None, where + (K,))
        worst = max(worst, _mean_ratio(d["r"], C, K, 1, where + (K,)))
        assert _tenths(d["score"]) == want_score, (where, K, d["score"], want_score)
    return worst


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__[5:])
def test_crafted_long_rows(ctx, family):
    """Rows of 1025 .. 2500 cells (1088: the pitch changes; four one-wave rows to a workgroup): every data-dependent exit of the
    selection the families force, kb = 0 (kappa 1e-4), kb = N and a count included; the score is sw_long_kernel on float
    thresholds and tie columns."""
    import oracle
    rng = np.random.default_rng(4321)
    worst = 0.0
    for n in S.LONG_N:
        for m in S.LONG_M:
            for kappa in KAPPAS + (1e-4,):
                kb = oracle.binary_k(kappa, n)
                C = family(m, n, kb, rng)
                worst = max(worst, _check_matrix(ctx, C, kappa, kb, S.LONG_K, (family.__name__, m, n, kappa)))
    print("worst r error / bound, long rows, %s: %.3f" % (family.__name__[5:], worst))


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__[5:])
def test_crafted_short_rows_of_a_tall_matrix(ctx, family):
    """1025 rows of 1 .. 1024 cells: the long kernel on rows the register kernels normally take (kb = 0 and kk = N among them)."""
    import oracle
    rng = np.random.default_rng(8765)
    worst = 0.0
    for n in S.TALL_N:
        for kappa in KAPPAS:
            kb = oracle.binary_k(kappa, n)
            C = family(S.TALL_M, n, kb, rng)
            worst = max(worst, _check_matrix(ctx, C, kappa, kb, S.LONG_K, (family.__name__, S.TALL_M, n, kappa)))
    print("worst r error / bound, tall matrix, %s: %.3f" % (family.__name__[5:], worst))


def test_tie_columns_at_the_edges_of_the_column_groups(ctx):
    """The tie search of ef_rowstat_long_kernel (`seen` over 64-column groups, the (budget - seen)-th set bit, eq > budget): the
    tie column at lane 0 and lane 63 of the first, a middle and the last group, in column N - 2, no surplus (JCUT_ALL), all equal."""
    import oracle
    worst = 0.0
    for n in S.TIE_N:
        for kappa in S.TIE_KB:
            kb = oracle.binary_k(kappa, n)
            C, labels, want = S.tie_matrix(n, kb)
            d = ctx.csm_debug_bits(C, kappa, 10)
            assert np.array_equal(d["jcut"], want), (n, kb, [(labels[k], int(d["jcut"][k]), int(want[k])) for k in np.nonzero(d["jcut"] != want)[0]])
            worst = max(worst, _check_matrix(ctx, C, kappa, kb, S.LONG_K, ("ties", n, kappa)))
    print("worst r error / bound, tie rows: %.3f" % worst)


def test_stale_pad_columns_are_not_read(ctx):
    """A matrix of 1088 columns of -1e30, then one of 1025 columns and as many rows: columns 1025 .. 1087 of the scratch hold the
    earlier values (smaller than every cell).  The long kernels guard by j < n: the results are those of a fresh context."""
    import oracle
    from acoss_amd import _lib
    m = 9
    C = np.random.default_rng(6).random((m, 1025)).astype(np.float32)
    fresh = _lib.Context(0)
    try:
        want = [fresh.csm_debug_bits(C, kappa, 10) for kappa in (0.1, 3)]
    finally:
        fresh.close()
    for k, kappa in enumerate((0.1, 3)):
        ctx.csm_debug_bits(np.full((m, 1088), -1e30, np.float32), kappa, 10)
        got = ctx.csm_debug_bits(C, kappa, 10)
        for key in ("t", "jcut", "r"):
            assert np.array_equal(got[key].view(np.uint32), want[k][key].view(np.uint32)), (kappa, key)
        assert got["score"] == want[k]["score"]
        _check_matrix(ctx, C, kappa, oracle.binary_k(kappa, 1025), (10,), ("stale pad", kappa))


# ------------------------------------------------------------------------------------------------------------------
# C. the product path with tracks of more than 1024 blocks
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def long_tracks():
    return S.long_pool()


@pytest.mark.parametrize("fuse,gemm,K", S.LONG_CONFIGS, ids=lambda v: str(v))
def test_product_path_with_long_tracks(ctx, long_tracks, fuse, gemm, K):
    """Pairs with a track of 1025 / 1100 blocks as rows, as columns and as both (the shared section across block 1024 of the
    second track), beside short tracks down to 3 blocks: all four slots -- t, jcut, r, c and scores against the specification on
    the device's own matrices.  K = 17 / 25: mode 1 of ef_rowstat_long_kernel on C^T; K = 16: ef_colstat_kernel<16> over 1100
    rows; both fuse modes of ef_fuse_kernel; both 16-bit arithmetics of the GEMMs."""
    pairs, index = S.long_probe_list()
    worst = dict(r=0.0, c=0.0)
    ctx.ef_upload_pool(long_tracks)
    ctx.set_ef_fuse(fuse)
    ctx.set_ef_gemm(gemm)
    try:
        listed = ctx.earlyfusion_pairs(pairs, 0.1, K)
        assert ctx.ef_debug_bits(pairs, 0, 0.1, K)["bits"] is None
        for shape in S.LONG_PROBES:
            _check_product_pair(ctx, pairs, index[shape], 0.1, K, listed, worst)
    finally:
        ctx.set_ef_fuse("fast")
        ctx.set_ef_gemm("default")
    planted = [float(listed[index[s], 3]) for s in S.LONG_PROBES[:2]]
    print("worst error / bound, long tracks, %s, %s, K = %d: r %.3f, c %.3f; early scores of the planted pairs %s"
          % (fuse, gemm, K, worst["r"], worst["c"], planted))


# ------------------------------------------------------------------------------------------------------------------
# D. batch composition is invisible
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", S.BATCH_N)
def test_rows_of_a_tall_matrix_equal_the_matrix_alone(ctx, n):
    """The same 64 rows alone (ef_rowstat2_kernel up to 512 cells, ef_rowstat_kernel<4, false> beyond) and as the first rows of a
    matrix of 1025 rows (ef_rowstat_long_kernel): t, jcut and r bit for bit.  With the long kernel's earlier summation order
    (columns lane + 64 k, xor butterfly) r differed on 19, 14, 11 and 17 of the 64 rows of these four matrices at K = 10."""
    C = S.batch_matrix(n)
    T = S.tall_matrix(C)
    m = len(C)
    for K in S.BATCH_K:
        a, b = ctx.csm_debug_bits(C, 0.1, K), ctx.csm_debug_bits(T, 0.1, K)
        assert b["bits"] is None
        differ = {key: int(np.sum(a[key].view(np.uint32) != b[key][:m].view(np.uint32))) for key in ("t", "jcut", "r")}
        print("n = %d, K = %d: rows that differ between the matrix alone and in the tall matrix: %s" % (n, K, differ))
        assert differ == dict(t=0, jcut=0, r=0), (n, K, differ)


def _list_statistics(ctx, pairs, where):
    out = {}
    for k in where:
        d = ctx.ef_debug_bits(pairs, k)
        for key in ("t", "jcut", "r", "c"):
            out["%d_%d_%s" % (pairs[k, 0], pairs[k, 1], key)] = d[key].view(np.uint32)
    out["scores"] = d["scores"][where].view(np.uint32)
    return out


@pytest.fixture(scope="module")
def mixed_tracks():
    return _pool(S.MIXED_BLOCKS)


@pytest.mark.parametrize("fuse", ["fast", "exact"])
def test_short_pairs_beside_a_long_pair_in_one_batch(ctx, mixed_tracks, fuse):
    """Pairs of two tracks of at most 1024 blocks (i) in a list of their own (the bit path), (ii) in one batch with a pair
    (1025, 257) -- every pair runs ef_rowstat_long_kernel -- and (iii) with a pair (257, 1025) -- sw_long_kernel as a single strip
    too: t, jcut, r, c of all four slots and the four scores, bit for bit."""
    probes, lists = S.mixed_lists()
    ctx.ef_upload_pool(mixed_tracks)
    ctx.set_ef_fuse(fuse)
    got = {}
    try:
        for name, (pairs, where) in lists.items():
            ctx.profile_enable(True)
            ctx.profile_reset()
            try:
                scores = ctx.earlyfusion_pairs(pairs)
                launched = ctx.profile()["ef_gemm_kernel"]["launches"]          # one timed GEMM scope per batch
            finally:
                ctx.profile_enable(False)
            assert launched == 1, (name, launched)
            assert (ctx.ef_debug_bits(pairs, 0)["bits"] is None) == (name != "alone")
            got[name] = _list_statistics(ctx, pairs, where)
            assert np.array_equal(got[name]["scores"], scores[where].view(np.uint32))
    finally:
        ctx.set_ef_fuse("fast")
    assert len(got["alone"]) == 4 * len(probes) + 1
    for name in ("long_rows", "long_cols"):
        bad = [key for key in got["alone"] if not np.array_equal(got["alone"][key], got[name][key])]
        print("%s, %s: %d of %d arrays differ from the list alone %s" % (fuse, name, len(bad), len(got["alone"]), bad[:8]))
        assert not bad, (fuse, name, bad[:8])


def test_scores_across_batch_boundaries_and_in_the_pair_grid(ctx, mixed_tracks):
    """earlyfusion_pairs alone: the list of (iii) under scratch limits that cut it into batches at two different sets of
    boundaries (batches with the long pair stream, the others do not), and the pair grid over the pool at two tile sizes (tiles
    without the track of 1025 blocks take the bit path): the scores of the list alone / of the pair list, bit for bit."""
    from acoss_amd import _lib
    probes, lists = S.mixed_lists()
    ctx.ef_upload_pool(mixed_tracks)
    want = ctx.earlyfusion_pairs(lists["alone"][0])
    pairs, where = lists["long_cols"]
    one_pair = 4 * 4 * 1024 * 1088
    for limit in (one_pair, 3 * one_pair + 4096):
        ctx.set_scratch_limit(limit)
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            got = ctx.earlyfusion_pairs(pairs)
            launched = ctx.profile()["ef_gemm_kernel"]["launches"]
        finally:
            ctx.profile_enable(False)
            ctx.set_scratch_limit(0)
        assert launched > 1, (limit, launched)
        diff = np.nonzero(np.any(got[where].view(np.uint32) != want.view(np.uint32), axis=1))[0]
        assert diff.size == 0, (limit, launched, [(probes[k], got[where][k], want[k]) for k in diff[:5]])
    n = len(S.MIXED_BLOCKS)
    every = _all_ordered_pairs(n)
    listed = ctx.earlyfusion_pairs(every)
    index = {(int(a), int(b)): k for k, (a, b) in enumerate(every)}
    sel = [index[p] for p in probes]
    assert np.array_equal(listed[sel].view(np.uint32), want.view(np.uint32))
    for tile in (0, 4):
        planes = [np.zeros((n, n), np.float32) for _ in range(4)]
        ctx.pair_grid(_lib.ALGO_EARLYFUSION, False, _lib.EfParams(0.1, 10), planes, mirror=False, tile=tile)
        for e in range(4):
            got = planes[e][every[:, 0], every[:, 1]]
            assert np.array_equal(got.view(np.uint32), listed[:, e].view(np.uint32)), (tile, e, every[np.nonzero(got != listed[:, e])[0][:5]])
