"""
The EarlyFusion back end behind the GEMMs, held per row and per cell against tests/_ef_backend_ref.py (pinned to the oracle
by tests/test_ef_backend_ref.py): the selection kernels' thresholds, tie columns, neighbourhood means and bitmaps, and the
packed 16-bit Smith-Waterman on arbitrary bitmaps -- through the debug entries acx_sw_bits_binary, acx_csm_debug_bits and
acx_ef_debug_bits, which launch the kernels of the product call.

Bars: t (bit patterns), jcut, bitmap words (pad bits included) and scores are exact.  r and c:
|got - f64 mean| <= (kk + 2) 2^-24 mean(|the kk summed cells|) -- kk - 1 f32 additions in any order, the (kk - tot) vk term and
the division (ref.mean_bound; derived, not measured).  Every test prints the worst ratio to that bound it saw.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from . import _ef_backend_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = (40, 100, 96)                       # feature dims of test_short_k_loops_of_small_feature_dims: the GEMMs cost nothing
SHORT = [1, 3, 7, 8, 9, 17, 64, 105, 106, 129, 257, 511, 512]
WIDE = [513, 769, 1023, 1024]
KAPPAS = (0.1, 0.05, 0.5, 0.0, 3)


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _sw(B):
    """Tenths: the oracle's alignment, which the numpy statement of it must equal."""
    import oracle
    want = oracle.sw_constrained_i32(B)
    assert ref.sw_tenths(B) == want, B.shape
    return want


def _tenths(score):
    v = float(score) * 10
    assert abs(v - round(v)) < 1e-3, score
    return int(round(v))


# ------------------------------------------------------------------------------------------------------------------
# a. sw_bits_h16_kernel<8 | 16> on arbitrary bitmaps
# ------------------------------------------------------------------------------------------------------------------
def test_sw_bits_goldens_bit_exact(ctx, golden):
    g = golden("ef_kernels")
    names = [k for k in g.files if (k.startswith("sw_B_") or k.startswith("swk_B_")) and max(g[k].shape) <= 1024]
    assert len(names) >= 30
    for name in names:
        B = g[name]
        want = float(g[name.replace("_B_", "_out_")])
        got = ctx.sw_bits_binary(B)
        assert abs(got - want) < 1e-5 and round(got * 10) == round(want * 10), (name, got, want)


@pytest.mark.parametrize("m", [4, 5, 1024])
def test_sw_bits_column_rims(ctx, m):
    """Every column count at which a lane, a word or the kernel variant changes (8 / 16 columns per lane, 32-bit words, <8> up
    to 512 and <16> up to 1024 columns), with the fewest rows that align at all, one more, and the most."""
    rng = np.random.default_rng(100 + m)
    for n in (4, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024):
        for dens in (0.05, 0.3, 0.8):
            B = (rng.random((m, n)) < dens).astype(np.uint8)
            assert _tenths(ctx.sw_bits_binary(B)) == _sw(B), (m, n, dens)


def test_sw_bits_random_shapes_vs_oracle(ctx):
    """The shapes of test_smith_waterman_random_shapes_vs_oracle that fit the bit kernels."""
    rng = np.random.default_rng(9)
    for (m, n) in [(4, 4), (5, 64), (64, 5), (65, 65), (300, 511), (512, 512), (129, 8), (8, 500),
                   (513, 513), (700, 40), (40, 700), (1024, 1024), (600, 1023)]:
        for dens in (0.05, 0.3, 0.8):
            B = (rng.random((m, n)) < dens).astype(np.uint8)
            assert _tenths(ctx.sw_bits_binary(B)) == _sw(B), (m, n, dens)


def test_sw_bits_extremes_of_the_16_bit_range(ctx):
    """What the packed 16-bit claim rests on: the longest diagonal (score 10 (1024 - 3) tenths, the ceiling), all ones (every
    cell at its maximum), all zeros (every U at its floor -7), and diagonals with a one-cell gap every 3rd / 4th step (U at
    its floor between matches, the score still climbing)."""
    eye = np.eye(1024, dtype=np.uint8)
    assert _tenths(ctx.sw_bits_binary(eye)) == _sw(eye) == 10 * (1024 - 3)
    for n in (1024, 512):
        for B in (np.ones((n, n), np.uint8), np.zeros((n, n), np.uint8)):
            assert _tenths(ctx.sw_bits_binary(B)) == _sw(B), (n, int(B[0, 0]))
    assert ctx.sw_bits_binary(np.zeros((1024, 1024), np.uint8)) == 0.0
    for step in (3, 4):
        B = np.eye(1024, dtype=np.uint8)
        B[np.arange(0, 1024, step), np.arange(0, 1024, step)] = 0
        want = _sw(B)
        assert want > 1000 and _tenths(ctx.sw_bits_binary(B)) == want, step
        assert _tenths(ctx.sw_bits_binary(B[:, :700])) == _sw(B[:, :700]) and _tenths(ctx.sw_bits_binary(B[:300])) == _sw(B[:300])
    for (m, n) in [(1, 1), (3, 3), (3, 900), (900, 3), (1, 1024), (1024, 2)]:
        assert ctx.sw_bits_binary(np.ones((m, n), np.uint8)) == 0.0
    with pytest.raises(IOError):
        ctx.sw_bits_binary(2 * np.ones((8, 8), np.uint8))
    for shape in [(1025, 8), (8, 1025)]:
        with pytest.raises(ValueError):
            ctx.sw_bits_binary(np.zeros(shape, np.uint8))


# ------------------------------------------------------------------------------------------------------------------
# b. crafted matrices through mode 0 of ef_rowstat2_kernel (N <= 512) / ef_rowstat_kernel<4, false> (513..1024)
# ------------------------------------------------------------------------------------------------------------------
CRAFT_N = [1, 4, 5, 15, 33, 64, 105, 106, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512, 513, 767, 768, 769, 1023, 1024]
CRAFT_M = [1, 2, 7, 8, 9, 17]              # every row count mod 8 of the 8-row workgroup that matters, an unpaired last row included
CRAFT_K = [1, 10, 16]


def _fam_uniform(m, n, kb, rng):
    """The ordinary road: the pivot estimate is accepted, both ranks come out of one histogram as the smallest / largest cell
    of their bin (two-row pass, or ef_select_pivot2 of the one-row kernel); short rows ((kb + 1) 6 > N) take kth()."""
    return rng.random((m, n)).astype(np.float32)


def _fam_few_values(m, n, kb, rng):
    """Four distinct values: more cells equal the threshold than the row may take (le > kb) -- the two-row pass hands the row
    to ef_row_finish, whose tie scan must find jcut; bins of far more than 64 equal cells refuse wave_select_pivot too."""
    return rng.integers(0, 4, (m, n)).astype(np.float32)


def _fam_constant_rows(m, n, kb, rng):
    """range < 1e-30: the pivot estimate is refused (`good` false) in both kernels; wave_select_fast sees one bin; every cell
    ties: jcut = kb - 1."""
    return np.tile(rng.random((m, 1)).astype(np.float32), (1, n))


def _fam_offset_noise(m, n, kb, rng):
    """1000 + 1e-4 noise: minimum > 2048 range -- the estimate is refused because mn * scale would lose the bins; at an ulp of
    6e-5 the row holds a handful of distinct values, so ties too."""
    return (1000.0 + 1e-4 * rng.random((m, n))).astype(np.float32)


def _fam_crowded_bin(m, n, kb, rng):
    """Up to 100 cells one ulp apart around the wanted rank, the rest spread over [0, 1]: the target bin holds more than 32
    (two-row pass: no gather, fallback) and more than 64 cells (one-row: wave_select_pivot / ef_select_pivot2 give up,
    wave_select_fast / wave_select_regs narrow it); all values distinct, so t must be exactly the right member."""
    C = np.empty((m, n), np.float32)
    k = min(max(kb, 1), n)
    q = np.float32(0.05 + 0.9 * k / n)
    for i in range(m):
        nbelow = max(0, k - 50)
        ncl = min(100, n - nbelow)
        cl = (np.float32(q).view(np.uint32) + np.arange(ncl, dtype=np.uint32) - np.uint32(ncl // 2)).astype(np.uint32).view(np.float32)
        below = (rng.random(nbelow) * 0.9 * q).astype(np.float32)
        above = (q * 1.1 + 0.01 + rng.random(n - nbelow - ncl)).astype(np.float32)
        row = np.concatenate([below, cl, above])
        C[i] = row[rng.permutation(n)]
    return C


def _fam_few_small(m, n, kb, rng):
    """Too few cells below the pivot.  Even rows: a small cell in every lane's first slot (every 4th column of the first 128,
    or 256 for wide rows), everything else in [0.9, 1): every group minimum is small, the pivot (largest group minimum + 15 %)
    lets in the 32 / 64 small cells only, fewer than kb + 1 for long rows -- the rank is not in the histogram (L2 < 0).  Odd
    rows: three small cells, the pivot lands among the large ones and their bins crowd."""
    C = (0.9 + 0.1 * rng.random((m, n))).astype(np.float32)
    for i in range(m):
        cols = np.arange(0, min(n, 256 if n > 512 else 128), 4) if i % 2 == 0 else rng.choice(n, min(3, n), replace=False)
        C[i, cols] = (1e-3 * rng.random(len(cols))).astype(np.float32)
    return C


def _fam_saturated(m, n, kb, rng):
    """The saturated fused matrix: most cells exactly 1.0f, 3 % neighbours.  Fewer neighbours than kb: the threshold is 1.0
    with hundreds of ties, jcut deep in the row."""
    C = np.ones((m, n), np.float32)
    hits = rng.random((m, n)) < 0.03
    C[hits] = rng.random(int(hits.sum())).astype(np.float32)
    return C


def _fam_zeros_denormals(m, n, kb, rng):
    """Rows with exact zeros and denormals among ordinary cells: mn = 0, bit patterns below 2^23 in the unsigned minimum /
    maximum reductions, a threshold that is 0.0 or a denormal for small kb (ties between the zeros).  At most two zeros and
    three denormals per row, so that the mean of 10 or 16 cells stays in the normal range the bound of r is stated for."""
    C = (0.01 + rng.random((m, n))).astype(np.float32)
    for i in range(m):
        nz, nd = (2, 3) if n >= 8 else ((1, 1) if n >= 2 else (1, 0))
        cols = rng.choice(n, nz + nd, replace=False)
        C[i, cols[:nz]] = 0.0
        C[i, cols[nz:]] = rng.integers(1, 1 << 22, nd).astype(np.uint32).view(np.float32)
    return C


FAMILIES = [_fam_uniform, _fam_few_values, _fam_constant_rows, _fam_offset_noise, _fam_crowded_bin, _fam_few_small,
            _fam_saturated, _fam_zeros_denormals]


def _check_slot(C, kb, t, jcut, words, where):
    """Thresholds, tie columns and (when there are any) bitmap words of one matrix against the specification; returns B."""
    wt, wj = ref.thresholds(C, kb)
    assert np.array_equal(t.view(np.uint32), wt.view(np.uint32)), (where, "t", np.nonzero(t.view(np.uint32) != wt.view(np.uint32))[0][:5])
    assert np.array_equal(jcut, wj), (where, "jcut", np.nonzero(jcut != wj)[0][:5])
    B = ref.binarise(C, wt, wj)
    if words is not None:
        assert words.shape == (C.shape[0], ref.pitch_words(C.shape[1])), where
        got, pad = ref.unpack_bits(words, C.shape[1])
        assert np.array_equal(got, B), (where, "bitmap", np.argwhere(got != B)[:5])
        assert pad == 0 and np.array_equal(words, ref.pack_bits(B)), (where, "pad bits", pad)
    return B


def _mean_ratio(got, C, K, axis, where):
    """Worst |got - f64 mean| / bound; asserts it is <= 1."""
    want, scale = ref.mean_smallest(C, K, axis)
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bound = ref.mean_bound(K, C.shape[axis], scale)
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), (where, "mean", float(np.max(err - bound)), int(np.argmax(err - bound)))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, 0.0)
    return float(ratio.max()) if ratio.size else 0.0


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f.__name__[5:])
def test_crafted_matrices_through_the_row_statistics(ctx, family):
    """Mode 0 of the kernels the product launches, on matrices built to force each data-dependent exit of the selection (see
    the family's docstring), at every row-length class and workgroup rim: t, jcut, r, bitmap, pad bits and score."""
    import oracle
    rng = np.random.default_rng(1234)
    worst = 0.0
    for n in CRAFT_N:
        for m in CRAFT_M:
            for kappa in KAPPAS:
                kb = oracle.binary_k(kappa, n)
                C = family(m, n, kb, rng)
                wt, wj = ref.thresholds(C, kb)
                want_score = _sw(ref.binarise(C, wt, wj))
                for K in CRAFT_K:
                    where = (family.__name__, m, n, kappa, K)
                    d = ctx.csm_debug_bits(C, kappa, K)
                    _check_slot(C, kb, d["t"], d["jcut"], d["bits"], where)
                    worst = max(worst, _mean_ratio(d["r"], C, K, 1, where))
                    assert _tenths(d["score"]) == want_score, (where, d["score"], want_score)
    print("worst r error / bound, %s: %.3f" % (family.__name__[5:], worst))


# ------------------------------------------------------------------------------------------------------------------
# c. the product path: ef_rowstat2 / <4, false>, ef_colstat / C^T, the fused selection, sw_bits_h16
# ------------------------------------------------------------------------------------------------------------------
def _track(nb, seed):
    rng = np.random.default_rng(seed)
    return dict(mfccs=rng.standard_normal((nb, DIMS[0])).astype(np.float32), ssms=(2 * rng.random((nb, DIMS[1]))).astype(np.float32),
                chromas=(rng.random((nb, DIMS[2])).astype(np.float32) ** 3 + 1e-3), chroma_med=rng.random(12) ** 2)


def _pool(blocks, seed=77):
    """Track k depends on (seed, k) alone, and so does what is planted into it: a prefix of a pool is the pool of the prefix."""
    tracks = [_track(nb, 1000 * seed + k) for k, nb in enumerate(blocks)]
    m = 40                                                      # shared structure: alignments longer than noise gives
    for a, b in ((6, 9), (10, 12), (8, 7), (11, 14), (13, 16)):
        if b < len(tracks):
            rng = np.random.default_rng(1000 * seed + 100 * a + b)
            for key in ("mfccs", "ssms", "chromas"):
                tracks[b][key][10:10 + m] = tracks[a][key][15:15 + m] + 0.02 * rng.standard_normal((m, tracks[a][key].shape[1])).astype(np.float32)
    return tracks


def _all_ordered_pairs(n):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    keep = i != j
    return np.ascontiguousarray(np.stack([i[keep], j[keep]], 1), np.int32)            # sorted by (first, second)


def _n_class(n):
    return (n > 128) + (n > 256) + (n > 384) + (n > 512) + (n > 768)


def _probes(blocks):
    """One pair per (M mod 8, N class) the pool offers, and its transpose: which track stands for a combination rotates, so that
    the probes spread over the pool."""
    seen, out = {}, []
    n = len(blocks)
    for shift in range(1, n):
        for i in range(n):
            j = (i + shift) % n
            key = (blocks[i] % 8, _n_class(blocks[j]))
            if key not in seen:
                seen[key] = (i, j)
                out += [(i, j), (j, i)]
    return sorted(set(out))


def _check_product_pair(ctx, pairs, k, kappa, K, listed, worst):
    """Pair k of the list: matrices from ef_debug_pairs (which stores the fused matrix), statistics and bitmaps from
    ef_debug_bits (which does not), everything against the specification applied to those matrices."""
    import oracle
    dm = ctx.ef_debug_pairs(pairs, k, kappa, K)
    db = ctx.ef_debug_bits(pairs, k, kappa, K)
    assert np.array_equal(db["scores"], listed) and np.array_equal(dm["scores"], listed), k
    mats = [dm["csm"][0], dm["csm"][1], dm["csm"][2], dm["fused"]]
    M, N = mats[0].shape
    kb = oracle.binary_k(kappa, N)
    for s in range(4):
        where = (tuple(int(v) for v in pairs[k]), (M, N), "slot %d" % s, K)
        B = _check_slot(mats[s], kb, db["t"][s], db["jcut"][s], None if db["bits"] is None else db["bits"][s], where)
        assert _tenths(listed[k, s]) == _sw(B), (where, "score")
        if s < 3:
            worst["r"] = max(worst["r"], _mean_ratio(db["r"][s], mats[s], K, 1, where + ("r",)))
            worst["c"] = max(worst["c"], _mean_ratio(db["c"][s], mats[s], K, 0, where + ("c",)))


@pytest.fixture(scope="module")
def pools():
    wide = _pool(SHORT + WIDE)
    return dict(short=(SHORT, wide[:len(SHORT)]), wide=(SHORT + WIDE, wide))


# pairs at the rims of the kernels' row-length classes and with no more rows than neighbours, on top of _probes: every case runs them
RIM_PAIRS = [(511, 512), (512, 511), (257, 512), (512, 257), (512, 129), (9, 17), (17, 8), (3, 1), (1, 512), (512, 1),
             (1023, 1024), (1024, 1023), (513, 1024), (1024, 513), (769, 1023), (1023, 769), (512, 1024), (1024, 512), (17, 1024),
             (1024, 17), (1, 1024), (1024, 1)]
PARTS = {                                                    # which list, and which of its probe pairs one case checks
    "list512": ("short", lambda m, n: True),
    "list1024_short_pairs": ("wide", lambda m, n: max(m, n) <= 512),
    "list1024_wide_pairs_even": ("wide", lambda m, n: max(m, n) > 512 and (m + n) % 2 == 0),
    "list1024_wide_pairs_odd": ("wide", lambda m, n: max(m, n) > 512 and (m + n) % 2 == 1),
}
CONFIGS = [("fast", "default", 10), ("exact", "default", 10), ("fast", "bf16x3", 10), ("exact", "bf16x3", 10),
           ("fast", "default", 11), ("fast", "default", 16), ("fast", "default", 17), ("fast", "default", 25)]


def _product_probes(blocks, keep):
    """Every (M mod 8, N class) the pool offers in both orientations, and the rim pairs: the ones `keep` selects, as track indices."""
    rims = [q for (m, n) in RIM_PAIRS if m in blocks and n in blocks for q in ((m, n), (n, m))]
    probes = set(_probes(blocks)) | {(blocks.index(m), blocks.index(n)) for (m, n) in rims}
    return sorted(p for p in probes if keep(blocks[p[0]], blocks[p[1]]))


@pytest.mark.parametrize("fuse,gemm,K", CONFIGS, ids=lambda v: str(v))
@pytest.mark.parametrize("part", list(PARTS))
def test_product_path(ctx, pools, part, fuse, gemm, K):
    """The product call on two lists: longest track 512 blocks (ef_rowstat2_kernel, ef_rowstat_kernel<2, true>,
    sw_bits_h16_kernel<8>) and one with tracks of 513..1024 (ef_rowstat_kernel<4, false>, <4, true> and sw_bits_h16_kernel<16> for
    ALL its pairs, the short ones included; its probes in three cases).  Every configuration -- both fuse modes (<NQ, true, EXACT>),
    both 16-bit arithmetics of the GEMMs, K = 10 / 11 / 16 (ef_colstat_kernel<10>, <16>) and 17 / 25 (the transposed matrices and
    mode 1 of ef_rowstat_kernel<2 | 4, false>) -- checks the SAME probe pairs: every (M mod 8, N class) the pool offers in both
    orientations and the rim pairs, tracks of 1..17 blocks (M <= K) among them; all four slots of each."""
    which, keep = PARTS[part]
    blocks, tracks = pools[which]
    pairs = _all_ordered_pairs(len(blocks))
    index = {(int(a), int(b)): k for k, (a, b) in enumerate(pairs)}
    worst = dict(r=0.0, c=0.0)
    ctx.ef_upload_pool(tracks)
    ctx.set_ef_fuse(fuse)
    ctx.set_ef_gemm(gemm)
    try:
        listed = ctx.earlyfusion_pairs(pairs, 0.1, K)
        probes = _product_probes(blocks, keep)
        assert len(probes) >= 12
        for p in probes:
            _check_product_pair(ctx, pairs, index[p], 0.1, K, listed, worst)
    finally:
        ctx.set_ef_fuse("fast")
        ctx.set_ef_gemm("default")
    print("worst error / bound, %s, %s, %s, K = %d, %d probes: r %.3f, c %.3f" % (part, fuse, gemm, K, len(probes), worst["r"], worst["c"]))


def test_probe_pairs_cover_every_row_count_and_row_length_class():
    """What test_product_path's docstring says of its probes, held: every (M mod 8, N class) of the pools in both orientations,
    the 512- and 1024-cell rims as N and as M, and rows of no more than 10 / 17 blocks."""
    for blocks in (SHORT, SHORT + WIDE):
        got = [p for part, (which, keep) in PARTS.items() if (which == "short") == (blocks == SHORT) for p in _product_probes(blocks, keep)]
        assert len(got) == len(set(got))
        shapes = {(blocks[a], blocks[b]) for (a, b) in got}
        keys = {(m % 8, _n_class(n)) for (m, n) in shapes}
        assert keys == {(m % 8, _n_class(n)) for m in blocks for n in blocks}
        assert all((n, m) in shapes for (m, n) in shapes)
        for rim in ((512, 1024) if blocks != SHORT else (512,)):
            assert any(n == rim for (_, n) in shapes) and any(m == rim for (m, _) in shapes)
        assert any(m <= 10 for (m, _) in shapes) and any(10 < m <= 17 for (m, _) in shapes)


# ------------------------------------------------------------------------------------------------------------------
# d. which kernel a batch takes is invisible, bit for bit
# ------------------------------------------------------------------------------------------------------------------
def _short_pair_statistics(ctx, tracks, nshort):
    """The statistics of a fixed set of short pairs in the list of all ordered pairs of `tracks`."""
    ctx.ef_upload_pool(tracks)
    pairs = _all_ordered_pairs(len(tracks))
    index = {(int(a), int(b)): k for k, (a, b) in enumerate(pairs)}
    probes = _product_probes(SHORT, lambda m, n: True)
    out = {}
    for (a, b) in probes:
        d = ctx.ef_debug_bits(pairs, index[(a, b)], 0.1, 10)
        for key in ("bits", "t", "jcut", "r", "c"):
            out["%d_%d_%s" % (a, b, key)] = d[key].view(np.uint32) if d[key].dtype == np.float32 else d[key]
    short = (pairs[:, 0] < nshort) & (pairs[:, 1] < nshort)
    out["scores"] = d["scores"][short]
    return out


def _child_main(out_path):
    from acoss_amd import _lib
    c = _lib.Context(0)
    np.savez(out_path, **_short_pair_statistics(c, _pool(SHORT), len(SHORT)))
    c.close()


@pytest.mark.timeout(600)
def test_kernel_choice_is_invisible_bit_for_bit(ctx, pools, tmp_path):
    """ef_rowstat2_kernels.hpp: "bit-identical statistics whichever kernel a batch takes".  The same short pairs in the list of
    short tracks (two-row kernel, narrow fused selection, <8>), in a list that shares its batch with tracks of 513+ blocks
    (<4, false>, <4, true>, <16>) and in a fresh process with ACX_EF_ROWSTAT2=0 (<2, false>): t, jcut, r, c, bitmaps, scores."""
    alone = _short_pair_statistics(ctx, pools["short"][1], len(SHORT))
    mixed = _short_pair_statistics(ctx, pools["wide"][1], len(SHORT))
    assert len(alone) > 40 and sorted(alone) == sorted(mixed)
    for key in alone:
        assert np.array_equal(alone[key], mixed[key]), ("batch with a 513+ track", key)
    out = str(tmp_path / "one_row.npz")
    env = dict(os.environ, ACX_EF_ROWSTAT2="0")
    code = "import sys; sys.path.insert(0, %r); from tests import test_gpu_ef_backend as T; T._child_main(%r)" % (ROOT, out)
    subprocess.check_call([sys.executable, "-c", code], env=env, timeout=300)
    child = np.load(out)
    assert sorted(child.files) == sorted(alone)
    for key in alone:
        assert np.array_equal(alone[key], child[key]), ("ACX_EF_ROWSTAT2=0", key)


# ------------------------------------------------------------------------------------------------------------------
# e. the float path: short batches of a list that holds a track of more than 1024 blocks
# ------------------------------------------------------------------------------------------------------------------
def test_float_path_on_short_batches_equals_the_bit_path(ctx, pools):
    """A list with one track of 1025 blocks takes the float-matrix path for ALL its batches: its short pairs run
    ef_rowstat2_kernel -> sw_kernel<8> -> ef_fuse_kernel -> ef_rowstat_kernel<2, false> mode 2 -> sw_kernel<8>.  Their scores
    must be those of the bit path (ef_rowstat_kernel's comment: the fused arithmetic is ef_fuse_kernel's "to the operation").
    The scratch limit is one long pair's need, so each long pair is a batch of its own and no short pair shares one."""
    short = pools["short"][1]
    tracks = short + [_track(1025, 78)]
    L = len(short)
    A = _all_ordered_pairs(L)
    Bl = np.concatenate([A, np.array([[L, 11], [L, 12]], np.int32)])              # (1025 x 511), (1025 x 512): the end of the sorted list
    ctx.ef_upload_pool(tracks)
    # The batching rule of run_ef (prepare): the float path keeps four matrices of M x pitch(N) floats per pair; a batch takes
    # pairs in list order while they fit the limit.  A long pair needs the whole limit, so it opens a batch of its own.  Held
    # here: the rule replayed on the list gives long pairs alone in their batches, and the library ran that many batches.
    nb = SHORT + [1025]
    limit_floats = 4 * 1025 * 512
    batches, used = [], limit_floats + 1
    for (q, r) in Bl:
        need = 4 * nb[q] * ((nb[r] + 63) // 64 * 64)
        assert need <= limit_floats
        if used + need > limit_floats:
            batches.append([])
            used = 0
        batches[-1].append((int(q), int(r)))
        used += need
    assert all(len(bt) == 1 for bt in batches if any(L in pr for pr in bt)) and sum(L in pr for bt in batches for pr in bt) == 2
    assert len(batches) >= 4
    # ... and the library's own report of its plan (acx_ef_plan: no device) gives the same batches
    from acoss_amd import _lib
    plan = _lib.ef_plan(nb, Bl, scratch_limit=4 * limit_floats)
    assert np.all(plan["path"] == 1) and plan["run_pos"].tolist() == list(range(len(Bl)))
    assert [[(int(q), int(r)) for (q, r) in Bl[plan["batch"] == b]] for b in range(int(plan["batch"].max()) + 1)] == batches
    for fuse in ("fast", "exact"):
        ctx.set_ef_fuse(fuse)
        try:
            a = ctx.earlyfusion_pairs(A)
            ctx.set_scratch_limit(4 * limit_floats)
            ctx.profile_enable(True)
            ctx.profile_reset()
            try:
                b = ctx.earlyfusion_pairs(Bl)
                launched = ctx.profile()["ef_gemm_kernel"]["launches"]          # one timed GEMM scope per batch
            finally:
                ctx.profile_enable(False)
                ctx.set_scratch_limit(0)
            assert launched == len(batches), (launched, len(batches))
        finally:
            ctx.set_ef_fuse("fast")
        diff = np.nonzero(np.any(a != b[:len(A)], axis=1))[0]
        assert diff.size == 0, (fuse, [(tuple(A[k]), a[k], b[k]) for k in diff[:5]])
        for k in (len(A), len(A) + 1):                               # the long pairs alone take the same kernels
            assert np.array_equal(ctx.earlyfusion_pairs(Bl[k:k + 1])[0], b[k]), k


@pytest.mark.parametrize("orient", ["1025_rows", "1025_columns"])
def test_float_path_long_pair_statistics(ctx, pools, orient):
    """ef_rowstat_long_kernel (modes 0 and 2) and ef_colstat_kernel on a pair with a track of 1025 blocks: t, jcut, r, c against
    the specification on the device's matrices, the scores against the oracle on the reference bitmaps.  No bitmaps exist."""
    short = pools["short"][1]
    tracks = short + [_track(1025, 78)]
    L = len(short)
    ctx.ef_upload_pool(tracks)
    pairs = np.array([[L, 10]] if orient == "1025_rows" else [[10, L]], np.int32)
    listed = ctx.earlyfusion_pairs(pairs)
    worst = dict(r=0.0, c=0.0)
    assert ctx.ef_debug_bits(pairs, 0)["bits"] is None
    _check_product_pair(ctx, pairs, 0, 0.1, 10, listed, worst)
    print("worst error / bound, long pair %s: r %.3f, c %.3f" % (orient, worst["r"], worst["c"]))


def test_debug_entries_refuse_what_they_cannot_show(ctx, pools):
    """A list that needs more than one batch (ACX_ERR_UNSUPPORTED, as ef_debug_pairs), an unsorted list, and bitmaps asked of
    the float path (ACX_ERR_INVALID): errors, and the context works afterwards."""
    import ctypes
    from acoss_amd import _lib
    short = pools["short"][1]
    L = len(short)
    ctx.ef_upload_pool(short + [_track(1025, 78)])
    A = _all_ordered_pairs(L)
    want = ctx.earlyfusion_pairs(A)
    ctx.set_scratch_limit(4 * 4 * 512 * 512)
    try:
        with pytest.raises(NotImplementedError):
            ctx.ef_debug_bits(A, 3)
    finally:
        ctx.set_scratch_limit(0)
    with pytest.raises(ValueError):
        ctx.ef_debug_bits(A[::-1], 0)
    long_pair = np.array([[L, 3]], np.int32)
    bits = np.zeros((4, 1025, 2), np.uint32)
    p = _lib.EfParams(0.1, 10)
    rc = ctx._L.acx_ef_debug_bits(ctx._h, long_pair.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1, ctypes.byref(p), 0,
                                  bits.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), None, None, None, None, None)
    assert rc == _lib.ACX_ERR_INVALID
    with pytest.raises(ValueError):
        ctx.csm_debug_bits(np.zeros((4, 4), np.float32), kappa=-1.0)
    assert ctx.csm_debug_bits(np.zeros((3, 1025), np.float32), 0.1, 10)["bits"] is None
    assert np.array_equal(ctx.ef_debug_bits(A, 3)["scores"], want)
