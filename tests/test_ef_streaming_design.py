"""
The inputs of tests/test_gpu_ef_streaming.py can see what they are built for -- shown on the CPU, on the specification alone
(tests/_ef_backend_ref.py) and on restatements of it that are broken on purpose (tests/_ef_streaming_cases.py).
"""
import numpy as np

from . import _ef_backend_ref as ref
from . import _ef_streaming_cases as S


def test_strip_restatement_equals_the_specification():
    """sw_strips without a mutant is ref.sw_tenths, on planted, rim and random plots and at strip widths that put seams everywhere."""
    for name, B, cells, field in S.planted_cases():
        assert S.sw_strips(B) == ref.sw_tenths(B), name
    for n in S.RIM_N[:7]:
        for m in (4, 6):
            for kind in S.RIM_PLOTS:
                B = S.rim_plot(kind, m, n)
                assert S.sw_strips(B) == ref.sw_tenths(B), (kind, m, n)
    rng = np.random.default_rng(3)
    for width in (2, 3, 5, 16):
        for dens in (0.3, 0.8):
            B = (rng.random((23, 37)) < dens).astype(np.uint8)
            assert S.sw_strips(B, width=width) == ref.sw_tenths(B), (width, dens)


def test_planted_paths_score_their_length_and_cross_their_seam():
    cases = S.planted_cases()
    assert len(cases) == 3 * 2 * (2 * 3 + 5)
    for name, B, cells, field in cases:
        assert len(cells) >= 40 and B.shape[0] <= 64
        holes = len(cells) - int(B.sum())
        want = ref.sw_tenths(B)
        if holes == 0:
            assert want == 10 * len(cells) - 7, name             # the path and nothing else: + 10 a cell, from the floor (-7) in front of it
        else:
            # one hole costs the match (+10), the mismatch (-10) and the gap (-7): the path runs on through it.  Two holes side by
            # side cost both matches and ONE penalised cell: a (2,1) step onto a zero in column seam - 1, a (1,2) step back
            assert want == 10 * len(cells) - 7 - (27 if holes == 1 else 37), (name, want)
            recs = []
            S.sw_strips(B, records=recs)
            seam = int(name[4:8])
            carried = recs[seam // S.STRIP - 1]
            assert np.any((carried > 0) & (carried % 10 != 0)), name        # a U that includes the -7 crosses the seam


def test_every_mutant_of_the_hand_over_changes_a_planted_score():
    cases = S.planted_cases()
    want = {name: ref.sw_tenths(B) for name, B, _, _ in cases}
    for mutant in S.MUTANTS:
        caught = [name for name, B, _, _ in cases if S.sw_strips(B, mutant) != want[name]]
        assert caught, mutant
        if mutant == "ring":                                     # only where the ring is reused: a path that crosses the third seam
            assert any(name.startswith("seam3072") for name in caught)
            assert not any(name.startswith("seam1024") for name in caught)
        print("%s: %d of %d planted cases" % (mutant, len(caught), len(cases)))
    # penalised values: the holes are seen too
    for name, B, _, _ in cases:
        if "hole" in name:
            assert S.sw_strips(B, "edge") != want[name], name


def test_every_record_field_is_decisive_where_its_step_enters_the_strip():
    """The case built for a field changes its score when that field alone is lost, at every seam and row parity; the other two
    fields leave a (1,1) / (1,2) / (2,1) entry alone only where the case does not name them."""
    cases = S.planted_cases()
    named = {f: 0 for f in S.FIELDS}
    for name, B, _, field in cases:
        if field is None:
            continue
        want = ref.sw_tenths(B)
        assert S.sw_strips(B, field) != want, (name, field)
        named[field] += 1
    assert all(v >= 6 for v in named.values()), named


def test_rim_plots_have_the_strip_counts_and_last_strips_the_kernel_can_get_wrong():
    strips = {(n + S.STRIP - 1) // S.STRIP for n in S.RIM_N}
    assert strips == {2, 3, 4, 5, 6}
    assert {n % S.STRIP for n in S.RIM_N} >= {1, 2, 3, 0, 1023}
    assert min(S.RIM_M) == 4 and max(S.RIM_M) <= 64
    # the 32-bit claim: a diagonal of 3400 scores more than 16 bits hold
    assert 10 * (3400 - 3) > 32767


def test_tie_rows_put_the_tie_column_where_the_group_search_turns():
    import oracle
    seen = set()
    for n in S.TIE_N:
        for kappa in S.TIE_KB:
            kb = oracle.binary_k(kappa, n)
            C, labels, want = S.tie_matrix(n, kb)
            t, jcut = ref.thresholds(C, kb)
            assert np.all(t == S.TIE_VALUE), (n, kb)
            assert np.array_equal(jcut, want), (n, kb, jcut, want)
            eq = np.sum(C == t[:, None], axis=1)
            budget = kb - np.sum(C < t[:, None], axis=1)
            need = 0
            for k, label in enumerate(labels):
                if jcut[k] != ref.JCUT_ALL:
                    need += 1
                    assert eq[k] > budget[k]
                    group = jcut[k] // 64
                    where = "first" if group == 0 else ("last" if group == (n - 1) // 64 else "middle")
                    seen.add((where, int(jcut[k] % 64)))
                    if jcut[k] == n - 2:
                        seen.add("before_last_column")
                else:
                    assert eq[k] == budget[k] and label.startswith("exact"), (n, kb, label)
                    seen.add("exact")
                    if C[k, n - 1] == t[k]:
                        seen.add("exact_last_column")
                if label == "all_equal":
                    assert eq[k] == n and jcut[k] == kb - 1
                    seen.add("all_equal")
            assert need >= 6, (n, kb, need)                      # rows of the case that need a tie column
            # ties in the tie column's own group in front of it, and in groups before: the set-bit walk and `seen` both count
            k = labels.index("mid_lane63")
            cols = np.nonzero(C[k] == t[k])[0]
            assert np.sum((cols // 64 == jcut[k] // 64) & (cols < jcut[k])) >= 1 and np.sum(cols // 64 < jcut[k] // 64) >= 1
    for placement in [("first", 0), ("first", 63), ("middle", 0), ("middle", 63), ("last", 0), "before_last_column", "exact",
                      "exact_last_column", "all_equal"]:
        assert placement in seen, (placement, sorted(map(str, seen)))


def test_long_pool_plants_its_sections_across_block_1024_of_the_second_track():
    for ((into, a0, a1), (frm, b0, b1)) in S.PLANTS:
        assert into > 1024 and a0 < 1024 < a1 and a1 - a0 == b1 - b0 >= 40 and b1 <= frm
        assert (frm, into) in S.LONG_PROBES
    pairs, index = S.long_probe_list()
    assert len(pairs) == len(S.LONG_PROBES) == len(index) == 10
    assert all(tuple(pairs[k - 1]) <= tuple(pairs[k]) for k in range(1, len(pairs)))
    tracks = S.long_pool()
    assert [len(t["mfccs"]) for t in tracks] == S.LONG_BLOCKS
    (into, a0, a1), (frm, b0, b1) = S.PLANTS[1]
    d = tracks[S.LONG_BLOCKS.index(into)]["mfccs"][a0:a1] - tracks[S.LONG_BLOCKS.index(frm)]["mfccs"][b0:b1]
    assert 0 < np.abs(d).max() < 0.2


def test_the_two_summation_orders_differ_on_the_batch_matrices():
    """The register kernels' order and the order ef_rowstat_long_kernel had give different f32 sums on at least a tenth of the rows
    of every matrix of D (uniform rows: about a quarter) -- and both stay inside ref.mean_bound."""
    for n in S.BATCH_N:
        C = S.batch_matrix(n)
        assert C.shape == (S.BATCH_M, n) and S.BATCH_M <= 64
        for K in S.BATCH_K:
            kk = min(K, n)
            vk = S.kth_smallest(C, K)
            a, b = S.sum_register_order(C, vk), S.sum_stream_order(C, vk)
            differ = int(np.sum(a.view(np.uint32) != b.view(np.uint32)))
            print("n = %d, K = %d: the orders differ on %d of %d rows" % (n, K, differ, len(C)))
            assert differ * 10 >= len(C), (n, K, differ)
            tot = np.sum(C < vk[:, None], axis=1)
            want, scale = ref.mean_smallest(C, K, 1)
            for s in (a, b):
                m = (s + (kk - tot).astype(np.float32) * vk) / np.float32(kk)
                assert m.dtype == np.float32 and np.all(np.abs(m.astype(np.float64) - want) <= ref.mean_bound(K, n, scale))


def test_mixed_lists_are_sorted_and_hold_one_long_pair():
    probes, lists = S.mixed_lists()
    assert len(probes) >= 30 and all(max(S.MIXED_BLOCKS[a], S.MIXED_BLOCKS[b]) <= 1024 for (a, b) in probes)
    for name, (pairs, where) in lists.items():
        assert all(tuple(pairs[k - 1]) < tuple(pairs[k]) for k in range(1, len(pairs)))
        assert [tuple(pairs[k]) for k in where] == probes
        shapes = [(S.MIXED_BLOCKS[a], S.MIXED_BLOCKS[b]) for (a, b) in pairs]
        assert len(pairs) == len(probes) + (name != "alone")
        assert max(m for m, _ in shapes) == (1024 if name != "long_rows" else 1025)
        assert max(n for _, n in shapes) == (1025 if name == "long_cols" else 1024)
