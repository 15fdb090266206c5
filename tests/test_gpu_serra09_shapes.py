"""
GPU tests (run with -m gpu on a real MI355X): every band and sweep kernel the Serra09 PRODUCT path launches, cell for cell.

tests/test_gpu_serra09.py compares intermediates through acx_serra09_debug_pair, which runs the D2-writing instantiations of the band
kernels, one pair per batch on one stream.  acx_serra09_pairs launches other instantiations (no D2, no d-domain thresholds), many
pairs per launch sorted by size class, its sweeps on a second stream -- and was checked through the final score only, a maximum over
alignment paths that a wrong cell in an edge tile rarely moves.  Here acx_serra09_debug_bits runs exactly the product call and hands
back the recurrence bitmap its kernels wrote; the oracle's plot R is the specification, bit for bit (np.array_equal, no tolerance),
for every compiled stack size m = 1 .. 16, every (reference class, query class) key of the batch sort, both sides of every class edge
and of every tile count, every row count mod 8, and the kernels kept behind environment switches.  The shape sets are
tests/_serra09_shapes.py; tests/test_serra09_shapes_design.py shows on the CPU what they reach.

Bits outside a matrix's columns: the sweep kernels mask them (qmax_bits*_kernel build a column mask of their own), so their count is
printed, not asserted.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _serra09_shapes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


_SHARED = {}


def _reference(name, m, kappa):
    """(scores, plots) of the oracle for a whole shape set, left unchanged by its users.  The edge sets of m = 4 and m = 9 serve several
    tests and are computed once; every other reference has one user and is not kept (27 MB of plots each)."""
    key = (name, m, kappa)
    if key in _SHARED:
        return _SHARED[key]
    ref = S.oracle_plots(getattr(S, name)(m), m=m, kappa=kappa)
    if name == "edge_set" and m in (4, 9):
        _SHARED[key] = ref
    return ref


def _bits_and_scores(ctx, d, m, want, tag, **kw):
    """One product call over d's pairs through acx_serra09_debug_bits against want = (scores, plots) of the oracle."""
    from acoss_amd import _lib
    scores, Rs = ctx.serra09_debug_bits(d["pairs"], _lib.serra09_params(m=m, **kw))
    print("%s m=%d: %d set bits outside the matrices' columns (masked by the sweeps)" % (tag, m, ctx.outside_bits))
    S.assert_plots_equal(d, m, Rs, want[1], tag)
    S.assert_scores_equal(d, m, scores, want[0], tag)
    return scores, Rs


@pytest.mark.parametrize("m", range(1, 17))
def test_every_m_every_class_bits_and_scores(ctx, m):
    """The edge set in ONE call: every band_kernel<M, 2 | 4 | 8, role, false> and every band2 class x m <= 9, on all 25 (cr, cq) keys
    and both sides of every class edge.  Plots and Qmax against the oracle; LateFusionChen's entry returns (Qmax, Dmax) of the same
    plots; acx_serra09_pairs returns its column 0."""
    from acoss_amd import _lib
    d = S.edge_set(m)
    want = _reference("edge_set", m, 0.095)
    ctx.upload_pool(d["frames"], d["offsets"])
    _bits_and_scores(ctx, d, m, want, "edge set")
    p = _lib.serra09_params(m=m)
    both = ctx.chenfusion_pairs(d["pairs"], p)
    S.assert_scores_equal(d, m, both, np.stack([want[0], S.oracle_sweeps(want[1], dmax=True)], 1), "edge set (Qmax, Dmax)")
    S.assert_scores_equal(d, m, ctx.serra09_pairs(d["pairs"], p), both[:, 0], "edge set serra09_pairs vs chenfusion_pairs")


@pytest.mark.parametrize("m", [9, 12])
def test_every_tile_count(ctx, m):
    """Both sides of every tile count (57 + 64 k | 58 + 64 k cells) as rows and as columns, all in one batch: short pairs sit in
    launches sized for the longest pair of their class."""
    d = S.tile_edge_set(m)
    ctx.upload_pool(d["frames"], d["offsets"])
    _bits_and_scores(ctx, d, m, _reference("tile_edge_set", m, 0.095), "tile-edge set")


@pytest.mark.parametrize("m", [4, 9, 13])
def test_row_residues(ctx, m):
    """1 .. 17 and 248 .. 251 rows (every count mod 8: bands of 8 rows, four and two rows per wave) against one reference per class."""
    d = S.row_residue_set(m)
    ctx.upload_pool(d["frames"], d["offsets"])
    _bits_and_scores(ctx, d, m, _reference("row_residue_set", m, 0.095), "row-residue set")


@pytest.mark.parametrize("m", [4, 9, 12])
def test_sweeps_on_product_shapes(ctx, m):
    """Dense plots (kappa = 0.4) of the edge set -- tall-narrow, wide-short and square, in every class -- through the sweeps as the
    product path picks them (by Mr alone, packed two or four pairs to a wave for the default penalties): qmax_bits_h16_multi_kernel
    <16 | 32, D>, qmax_bits_h16_kernel<16 | 32, D> and qmax_bits_kernel<true | false, D, 8 | 16 | 32>.  Expected: the oracle's DP on
    the oracle's plot; dp_start = 3: the full-chain oracle."""
    from acoss_amd import _lib
    d = S.edge_set(m)
    want = _reference("edge_set", m, 0.4)
    ctx.upload_pool(d["frames"], d["offsets"])
    _bits_and_scores(ctx, d, m, want, "edge set kappa=0.4", kappa=0.4)
    for go, ge in ((0.5, 0.5), (1.0, 1.0), (1.0, 0.25)):
        for dmax in (0, 1):
            got = ctx.serra09_pairs(d["pairs"], _lib.serra09_params(m=m, kappa=0.4, gamma_o=go, gamma_e=ge, dmax=dmax))
            S.assert_scores_equal(d, m, got, S.oracle_sweeps(want[1], go, ge, bool(dmax)), "gammas (%g, %g) dmax=%d" % (go, ge, dmax))
    got = ctx.serra09_pairs(d["pairs"], _lib.serra09_params(m=m, kappa=0.4, dp_start=3))
    S.assert_scores_equal(d, m, got, S.oracle_scores(d, m=m, kappa=0.4, dp_start=3), "dp_start=3")


# heights (Mq) of the lists, in list order; the batch sort orders a class by the query's class, so 3, 40 and 249 rows share a wave
# with each other and with 1017 or 2041 rows, and the last wave is partly empty
_CLASS0_LISTS = ([249], [3, 2041], [40, 1017, 2041], [3, 40, 249, 1017, 2041], [3, 40, 249, 1017, 2041, 2041, 3, 1017, 40])
_CLASS1_LISTS = ([40], [3, 2041, 249], [3, 40, 1017, 2041, 2041])


def test_pairs_per_wave_tails(ctx):
    """qmax_bits_h16_multi_kernel packs four pairs (rows of <= 249 cells) or two (<= 505) into a wave: lists that leave the last wave
    partly empty, with members of 3 to 2041 rows side by side (a short member idles while its neighbour works).  Qmax and Dmax,
    dp_start 2 and 3, dense plots."""
    from acoss_amd import _lib
    m = 9
    d0 = S.edge_set(m)
    ctx.upload_pool(d0["frames"], d0["offsets"])
    st, en = d0["start"], d0["end"]
    for refs, lists in (((en[249], st[40]), _CLASS0_LISTS), ((en[505], en[250]), _CLASS1_LISTS)):
        for heights in lists:
            d = S.subset(d0, [(st[h], refs[k % 2]) for k, h in enumerate(heights)])
            assert len({S.key(int(d0["M"][i]), int(d0["M"][j]))[0] for i, j in d["pairs"]}) == 1
            tag = "list of %d pairs, Mq %s" % (len(heights), heights)
            want = S.oracle_plots(d, m=m, kappa=0.4)
            _bits_and_scores(ctx, d, m, want, tag, kappa=0.4)
            for dp_start in (2, 3):
                ref = np.stack([S.oracle_scores(d, m=m, kappa=0.4, dp_start=dp_start, dmax=x) for x in (0, 1)], 1)
                for dmax in (0, 1):
                    got = ctx.serra09_pairs(d["pairs"], _lib.serra09_params(m=m, kappa=0.4, dp_start=dp_start, dmax=dmax))
                    S.assert_scores_equal(d, m, got, ref[:, dmax], "%s dp_start=%d dmax=%d" % (tag, dp_start, dmax))
                both = ctx.chenfusion_pairs(d["pairs"], _lib.serra09_params(m=m, kappa=0.4, dp_start=dp_start))
                S.assert_scores_equal(d, m, both, ref, "%s dp_start=%d (Qmax, Dmax)" % (tag, dp_start))


@pytest.mark.parametrize("m", [9, 12])
def test_pool_neighbours_do_not_leak(ctx, m):
    """The band kernels' edge tiles read frames and norms before and behind a track without clamping the index -- inside the pool
    that is the neighbouring track -- and mask the cells they feed.  The same two tracks (249 and 505 cells, paired in both orders:
    Mr = 505 and Mr = 249) between different neighbours, and as the last tracks of the pool: identical plots and scores, the
    oracle's.  The neighbours are finite with finite squares and dot products (a neighbour near 3e38 is a known limit)."""
    from acoss_amd import synth
    rng = np.random.default_rng([m, 6])
    X, Y = (synth._frame_max_normalise(rng.random((S.frames_for(M, m), 12))) for M in (249, 505))
    nb = {"random": synth._frame_max_normalise(rng.random((120, 12))), "zero": np.zeros((120, 12), np.float32),
          "one": np.ones((120, 12), np.float32), "1e15": np.full((120, 12), 1e15, np.float32)}
    pools = [(kind, [N, X, N, Y, N], (1, 3)) for kind, N in nb.items()]
    pools += [("last: X, Y", [nb["random"], X, Y], (1, 2)), ("last: Y, X", [nb["1e15"], Y, X], (2, 1)), ("alone", [X, Y], (0, 1))]
    want = None
    for kind, tracks, (ix, iy) in pools:
        frames, offsets = synth.pack(tracks)
        d = dict(frames=frames, offsets=offsets, pairs=np.array([(ix, iy), (iy, ix)], np.int32),
                 M=np.array([S._embed_len(len(t), m) for t in tracks]))
        if want is None:
            want = S.oracle_plots(d, m=m)
        ctx.upload_pool(frames, offsets)
        _bits_and_scores(ctx, d, m, want, "neighbours: %s" % kind)


def test_debug_bits_wants_one_batch(ctx):
    """A list the product path would split into batches is refused (ACX_ERR_UNSUPPORTED) before anything runs: slot 0's
    descriptors describe one batch only.  The product entry takes the same list in several batches and returns the same scores."""
    from acoss_amd import _lib
    m = 9
    d = S.row_residue_set(m)
    ctx.upload_pool(d["frames"], d["offsets"])
    p = _lib.serra09_params(m=m)
    scores, _ = ctx.serra09_debug_bits(d["pairs"], p)
    ctx.set_scratch_limit(1 << 18)            # 65536 floats; a bitmap word counts as two: the 105 pairs need 140422, the largest 12048
    try:
        with pytest.raises(NotImplementedError, match="one batch"):
            ctx.serra09_debug_bits(d["pairs"], p)
        assert np.array_equal(ctx.serra09_pairs(d["pairs"], p), scores)
    finally:
        ctx.set_scratch_limit(0)
    assert np.array_equal(ctx.serra09_debug_bits(d["pairs"], p)[0], scores)


_VARIANTS = ({}, {"ACX_BAND2": "0"}, {"ACX_BAND2": "1"}, {"ACX_BAND2": "2"}, {"ACX_QMAX_MULTI": "0"}, {"ACX_QMAX_STREAM": "0"})
_VARIANT_CASES = [(m, kappa) for m in (4, 9) for kappa in (0.095, 0.4)]

_VARIANT_SNIPPET = r'''
import sys, numpy as np
sys.path.insert(0, %(root)r)
from acoss_amd import _lib
from tests import _serra09_shapes as S
ctx = _lib.Context(0)
out = {}
for m, kappa in %(cases)r:
    d = S.edge_set(m)
    ctx.upload_pool(d["frames"], d["offsets"])
    p = _lib.serra09_params(m=m, kappa=kappa)
    scores, Rs = ctx.serra09_debug_bits(d["pairs"], p)
    key = "m%%d_k%%g" %% (m, kappa)
    out[key + "_bits"] = np.packbits(np.concatenate([R.ravel() for R in Rs]))
    out[key + "_scores"] = scores
    out[key + "_both"] = ctx.chenfusion_pairs(d["pairs"], p)
np.savez(%(out)r, **out)
ctx.close()
'''


@pytest.mark.timeout(900)
def test_environment_variants_give_the_same_bits(tmp_path):
    """The kernels kept behind per-process switches as A/B aids -- band_kernel<M <= 9, 2 | 4> (ACX_BAND2=0 | 1 | 2 peel the band2 classes
    off one by one), qmax_bits_h16_kernel<8, D> (ACX_QMAX_MULTI=0: one wave per pair) and the one-stream path (ACX_QMAX_STREAM=0) --
    must write the default's plots and return its (Qmax, Dmax) bit for bit, and the default the oracle's.  The switches are read
    once per process: one fresh child per setting, one after the other; a failing child raises and no further child starts."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    results = []
    for k, extra in enumerate(_VARIANTS):
        out = str(tmp_path / ("variant_%d.npz" % k))
        env = dict(os.environ)
        for name in ("ACX_BAND2", "ACX_QMAX_MULTI", "ACX_QMAX_STREAM"):
            env.pop(name, None)
        env.update(extra)
        subprocess.check_call([sys.executable, "-c", _VARIANT_SNIPPET % {"root": root, "cases": _VARIANT_CASES, "out": out}],
                              env=env, timeout=300)
        with np.load(out) as z:
            results.append({name: z[name] for name in z.files})
    for extra, res in zip(_VARIANTS[1:], results[1:]):
        assert sorted(res) == sorted(results[0])
        for name in sorted(res):
            assert np.array_equal(res[name], results[0][name]), (extra, name, int(np.sum(res[name] != results[0][name])))
    for m, kappa in _VARIANT_CASES:
        d = S.edge_set(m)
        scores, Rs = _reference("edge_set", m, kappa)
        key = "m%d_k%g" % (m, kappa)
        n = sum(R.size for R in Rs)
        flat = np.unpackbits(results[0][key + "_bits"])[:n]
        off = np.concatenate([[0], np.cumsum([R.size for R in Rs])])
        S.assert_plots_equal(d, m, [flat[off[k]:off[k + 1]].reshape(Rs[k].shape) for k in range(len(Rs))], Rs, "default, kappa=%g" % kappa)
        S.assert_scores_equal(d, m, results[0][key + "_scores"], scores, "default, kappa=%g" % kappa)
        S.assert_scores_equal(d, m, results[0][key + "_both"], np.stack([scores, S.oracle_sweeps(Rs, dmax=True)], 1),
                              "default (Qmax, Dmax), kappa=%g" % kappa)
