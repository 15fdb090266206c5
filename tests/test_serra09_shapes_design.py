"""
CPU-only: the shape sets of tests/_serra09_shapes.py reach what tests/test_gpu_serra09_shapes.py says they reach -- every (cr, cq) class
key of the product path's batch sort, both sides of every inner class edge as rows AND as columns, every band kernel family in both
roles -- and the recurrence plots they give the kernels are neither empty nor full.  S.cls / S.key / S.family are the library's own
answers (acx_serra09_plan: the table of acoss_amd/csrc/serra09_plan.hpp, no device needed), so the literals below pin that table.
"""
import numpy as np
import pytest

from tests import _serra09_shapes as S


def _dims(d):
    return [(int(d["M"][i]), int(d["M"][j])) for i, j in d["pairs"]]


@pytest.mark.parametrize("m", [1, 9, 10, 16])
def test_edge_set_hits_every_key_and_both_sides_of_every_edge(m):
    import oracle
    d = S.edge_set(m)
    p = oracle.serra09_params(m=m)
    lens = np.diff(d["offsets"])
    assert [oracle.serra09_embed_len(int(T), p) for T in lens] == d["M"].tolist()
    dims = _dims(d)
    assert len(dims) == 45 and sum(a * b for a, b in dims) == 26_822_817
    assert {S.key(a, b) for a, b in dims} == {(cr, cq) for cr in range(S.NC) for cq in range(S.NC)}
    Mqs, Mrs = {a for a, _ in dims}, {b for _, b in dims}
    for lo, up in zip(S.LOWER, S.UPPER):
        assert lo == up + 1 and S.cls(lo) == S.cls(up) + 1
        assert {lo, up} <= Mqs and {lo, up} <= Mrs, (lo, up)
    assert S.cls(2041) == 4 and S.cls(2042) == 5 and S.cls(1) == 0
    # two versions per length, from the two ends of the work
    assert sorted(d["M"].tolist()) == sorted(2 * (list(S.UPPER) + list(S.LOWER) + [3, 40]))


def test_every_band_family_is_named_in_both_roles():
    # the row pass of a pair runs the kernel of class cr (role 0), its column pass that of class cq (role 1); the edge set holds every key
    seen = {(S.family(m, c), role) for m in range(1, 17) for c in range(S.NC) for role in (0, 1)}
    assert {f for f, _ in seen} == set(S.FAMILIES) and len(S.FAMILIES) == 8
    assert seen == {(f, role) for f in S.FAMILIES for role in (0, 1)}
    assert [S.family(9, c) for c in range(5)] == ["band2_kernel<M, B2_NV, 16>", "band2_kernel<M, B2_NV, 32>", "band2_kernel<M, B2_NV_MID, 32>",
                                                  "band_kernel<M<=9, 4>", "band_kernel<M<=9, 8>"]
    assert [S.family(10, c) for c in range(5)] == ["band_kernel<M>=10, 2>"] * 2 + ["band_kernel<M>=10, 4>"] * 2 + ["band_kernel<M>=10, 8>"]
    # per m, the keys of the edge set put every class on both passes
    for m in (1, 9, 10, 16):
        dims = _dims(S.edge_set(m))
        assert {(S.family(m, S.key(a, b)[0]), 0) for a, b in dims} | {(S.family(m, S.key(a, b)[1]), 1) for a, b in dims} == \
            {(S.family(m, c), role) for c in range(S.NC) for role in (0, 1)}


def test_tile_edge_and_row_residue_sets():
    for m in (9, 12):
        d = S.tile_edge_set(m)
        dims = _dims(d)
        assert len(dims) == 126
        tiles = lambda M: (M + S.BAND - 1 + 63) // 64
        for side in (0, 1):         # every tile count 1 .. 32 from its last length, 2 .. 32 from its first, as Mq and as Mr
            other = [x[1 - side] for x in dims if x[side] != 300]
            assert set(other) == {300}
            Ms = sorted(x[side] for x in dims if x[side] != 300)
            assert Ms == sorted([57 + 64 * k for k in range(32)] + [58 + 64 * k for k in range(31)])
            assert {tiles(M) for M in Ms if M % 64 == 57} == set(range(1, 33))
            assert {tiles(M) for M in Ms if M % 64 == 58} == set(range(2, 33))
    for m in (4, 9, 13):
        dims = _dims(S.row_residue_set(m))
        assert len(dims) == 105
        assert {a for a, _ in dims} == set(range(1, 18)) | {248, 249, 250, 251}
        assert {a % 8 for a, _ in dims} == set(range(8))
        assert sorted({S.cls(b) for _, b in dims}) == [0, 1, 2, 3, 4]


@pytest.mark.parametrize("kappa", [0.095, 0.4])
def test_plots_are_neither_empty_nor_full(kappa):
    for d in (S.edge_set(9), S.tile_edge_set(9)):
        scores, Rs = S.oracle_plots(d, m=9, kappa=kappa)
        dens = np.array([R.mean() for R in Rs])
        print("kappa %g: densities %.4f .. %.4f, scores %g .. %g" % (kappa, dens.min(), dens.max(), scores.min(), scores.max()))
        for k, R in enumerate(Rs):
            assert 0 < int(R.sum()) < R.size, S.describe(d, k, 9)
            assert 0.01 <= dens[k] <= 0.6, (S.describe(d, k, 9), dens[k])
