"""
CPU: the specification of the full cross-diffusion early fusion (tests/_crossfusion_ref.py) against the reference's own
getWCSMSSM and doSimilarityFusionWs (tests/golden/crossfusion.npz, made by tests/golden/make_crossfusion_goldens.py), the
refusal rule against what the reference does on such shapes, four wrong variants, the export list and the argument checks
of EarlyFusion.full_fusion / rerank_full, which run without a device.

  W, D     rtol 1e-10, atol 1e-14 (DESIGN.md section 23's figures: other summation orders of the same f64 operations)
  B, score exact; every row's gap at the cut of X is at least 1e-6, far above what rtol 1e-10 moves
"""
import os
import re

import numpy as np
import pytest

from . import _crossfusion_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("acx_ef_crossfusion_pairs", "acx_ef_crossfusion_debug", "acx_crossfusion_matrices", "acx_xsel_binary_sw")
MIN_GAP = 1e-6


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "crossfusion.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def chains(golden):
    """The specification run once per golden shape."""
    out = {}
    for M, N in golden["shapes"]:
        tag = "%dx%d_" % (M, N)
        out[(int(M), int(N))] = ref.chain(golden[tag + "SA"], golden[tag + "SB"], golden[tag + "C"], int(golden["K"]), int(golden["niters"]),
                                          float(golden["reg_diag"]), float(golden["kappa"]))
    return out


def test_golden_shapes(golden):
    assert [tuple(s) for s in golden["shapes"]] == [(12, 30), (40, 33), (64, 65)]
    assert int(golden["K"]) == 10 and int(golden["niters"]) == 5
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "crossfusion.npz")) < 1000000


@pytest.mark.parametrize("shape", [(12, 30), (40, 33), (64, 65)])
def test_specification_against_the_reference(golden, chains, shape):
    import oracle
    tag = "%dx%d_" % shape
    got = chains[shape]
    k = ref.binary_k(float(golden["kappa"]), shape[1])
    errW = np.max(np.abs(got["W"] - golden[tag + "W"]) / (1e-10 * np.abs(golden[tag + "W"]) + 1e-14))
    errD = np.max(np.abs(got["D"] - golden[tag + "D"]) / (1e-10 * np.abs(golden[tag + "D"]) + 1e-14))
    print("%s: W %.3g of its bound, D %.3g of its bound" % (shape, errW, errD))
    np.testing.assert_allclose(got["W"], golden[tag + "W"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(got["D"], golden[tag + "D"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(got["X"], golden[tag + "X"], rtol=1e-10, atol=1e-14)
    assert ref.cut_gap(golden[tag + "X"], k).min() >= MIN_GAP
    assert ref.cut_gap(got["X"], k).min() >= MIN_GAP / 2
    assert np.array_equal(got["B"], golden[tag + "B"])
    assert got["B"].sum(1).tolist() == [k] * shape[0]
    assert oracle.sw_constrained(got["B"]) == float(golden[tag + "score"])
    # the plot is csm_to_binary(exp(-X), kappa): stated without the exponential
    assert np.array_equal(got["B"], oracle.csm_to_binary(np.exp(-got["X"]), float(golden["kappa"])))


def test_w_is_symmetric_and_d_is_not(chains):
    for (M, N), got in chains.items():
        for W in got["W"]:
            assert np.array_equal(W[:M, M:], W[M:, :M].T)
        assert not np.array_equal(got["D"][:M, M:], got["D"][M:, :M].T)


@pytest.mark.parametrize("wrong", ref.WRONG_VARIANTS)
def test_wrong_variants_differ(golden, chains, wrong):
    """Each wrong variant leaves the bounds the device is held to on EVERY golden input: X (bit-identical on the device's D, D
    within rtol 1e-10) moves by far more, or -- the selection variant, which leaves X alone -- the plot itself changes.  Whether the
    PLOT changes too is printed: the upper block alone picks the same cells as both blocks on these three inputs."""
    plots = 0
    for M, N in golden["shapes"]:
        tag = "%dx%d_" % (M, N)
        if wrong == "k_swapped" and len(set(ref.split(M, N, int(golden["K"])))) == 1:      # (40, 33): k1 = k2 = 5, nothing to swap
            continue
        bad = ref.chain(golden[tag + "SA"], golden[tag + "SB"], golden[tag + "C"], int(golden["K"]), int(golden["niters"]),
                        float(golden["reg_diag"]), float(golden["kappa"]), wrong=wrong)
        good = chains[(int(M), int(N))]
        if wrong == "k_smallest":
            assert np.array_equal(bad["X"], good["X"]) and not np.array_equal(bad["B"], good["B"]), (wrong, M, N)
        else:
            rel = np.max(np.abs(bad["X"] - good["X"]) / np.abs(good["X"]))
            assert rel > 1e-6, (wrong, M, N, rel)
        plots += not np.array_equal(bad["B"], good["B"])
    print("%s: the plot changes on %d of 3 golden inputs" % (wrong, plots))


def _reference_getwcsm(C, k1, k2):
    import warnings
    import oracle
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (numpy: "Mean of empty slice" at k1 = 0)
        return oracle.get_wcsm(C, k1, k2)


def test_refusal_rule_against_the_reference():
    """(4, 40): k1 = 0, the mean over no cell -> NaN; (3, 5): k1 + 1 = M, np.partition of getW raises.  Both are refused; the golden
    shapes and the GPU tests' shapes are not."""
    import oracle
    rng = np.random.default_rng(5)
    assert ref.split(4, 40, 10) == (0, 10) and ref.refused(4, 40, 10)
    W = _reference_getwcsm(rng.random((4, 40)), 0, 10)
    assert np.isnan(W).all()
    k1, k2 = ref.split(3, 5, 10)
    assert (k1, k2) == (3, 7) and ref.refused(3, 5, 10)
    with pytest.raises(ValueError):
        oracle.snf_getW(rng.random((3, 3)), k1)
    with pytest.raises(ValueError):
        _reference_getwcsm(rng.random((3, 5)), k1, k2)
    for M, N, K in [(5, 40, 10), (12, 30, 10), (30, 12, 10), (40, 33, 10), (63, 66, 10), (64, 65, 10), (127, 130, 10), (120, 1024, 10), (12, 12, 20)]:
        assert not ref.refused(M, N, K), (M, N, K)
    assert ref.split(5, 40, 10) == (1, 9) and ref.split(12, 12, 20) == (10, 10)
    assert ref.refused(12, 12, 22) and ref.refused(40, 2, 10) and ref.refused(30, 30, 1)


def test_pack_and_unpack():
    rng = np.random.default_rng(9)
    for N in (4, 63, 64, 65, 130):
        B = (rng.random((5, N)) < 0.3).astype(np.uint8)
        bits = ref.pack_bits(B)
        assert bits.shape == (5, (N + 63) // 64 * 2) and bits.dtype == np.uint32
        back, pad = ref.unpack_bits(bits, N)
        assert np.array_equal(back, B) and not pad.any()
        assert all(((int(bits[0, j // 32]) >> (j % 32)) & 1) == B[0, j] for j in range(N))


def test_select_ties_in_column_order():
    X = np.array([[1.0, 3.0, 3.0, 3.0, 0.0, -0.0, 5.0]])
    assert ref.select(X, 3).tolist() == [[0, 1, 1, 0, 0, 0, 1]]
    assert ref.select(X, 6).tolist() == [[1, 1, 1, 1, 1, 0, 1]]            # +0.0 and -0.0 tie: the first column wins
    assert ref.select(X, 0).sum() == 0 and ref.select(X, 9).sum() == 7
    assert ref.select(X, 3, wrong="k_smallest").tolist() == [[1, 0, 0, 0, 1, 1, 0]]


def test_header_and_exports_carry_the_names():
    from acoss_amd import _lib
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert name in _lib.EXPORTS, name
        assert re.search(r"\bint %s\(acx_ctx \*ctx" % name, header), name
        assert name in integration, name
    assert os.path.exists(os.path.join(ROOT, "acoss_amd", "csrc", "ef_crossfusion_kernels.hpp"))


class _NoDevice(object):
    """An EarlyFusion whose context must not be asked for: the argument checks come before the first library call."""

    def __init__(self, N=6, K=10, niters=5):
        from acoss_amd.algorithms.earlyfusion_traile import EarlyFusion
        self.ef = EarlyFusion.__new__(EarlyFusion)
        self.ef.N, self.ef.K, self.ef.niters, self.ef.kappa = N, K, niters, 0.1

        def no_context():
            raise AssertionError("the library was called")
        self.ef._context = no_context


def test_full_fusion_argument_checks_need_no_device():
    ef = _NoDevice().ef
    with pytest.raises(ValueError, match=r"idxs must be \(K, 2\)"):
        ef.full_fusion([1, 2, 3])
    with pytest.raises(ValueError, match=r"track indices in \[0, 6\)"):
        ef.full_fusion([[0, 6]])
    with pytest.raises(ValueError, match="must be integers"):
        ef.full_fusion([[0.5, 1.0]])
    out = ef.full_fusion(np.zeros((0, 2), np.int64))
    assert out.shape == (0,) and out.dtype == np.float32
    with pytest.raises(ValueError, match="niters must be >= 1"):
        _NoDevice(niters=0).ef.full_fusion([[0, 1]])
    with pytest.raises(NotImplementedError, match="more than 64 neighbours"):
        _NoDevice(K=65).ef.full_fusion([[0, 1]])
    with pytest.raises(ValueError, match="K must be >= 1"):
        _NoDevice(K=0).ef.full_fusion([[0, 1]])


def test_rerank_full_argument_checks_need_no_device():
    ef = _NoDevice().ef
    with pytest.raises(ValueError, match=r"queries must be track indices in \[0, 6\)"):
        ef.rerank_full([6], [[1]])
    with pytest.raises(ValueError, match="k must be >= 1"):
        ef.rerank_full([0], [[1]], k=0)
    with pytest.raises(ValueError, match="one row per query"):
        ef.rerank_full([0, 1], [[1]])
    with pytest.raises(ValueError, match="lists track 2 twice"):
        ef.rerank_full([0], [[2, 3, 2]])
    with pytest.raises(ValueError, match=r"in \[0, 6\) or -1"):
        ef.rerank_full([0], [[7]])
    with pytest.raises(ValueError, match="niters must be >= 1"):
        _NoDevice(niters=0).ef.rerank_full([0], [[1]])
    # nothing to compute: the query's own track and empty slots alone
    idx, score = ef.rerank_full([0, 1], [[0, -1], [-1, 1]], k=3)
    assert idx.shape == (2, 3) and idx.dtype == np.int32 and (idx == -1).all()
    assert score.shape == (2, 3) and score.dtype == np.float32 and np.isnan(score).all()
