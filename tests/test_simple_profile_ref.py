"""
CPU checks of tests/_simple_profile_ref.py, the reference tests/test_gpu_simple_profile.py holds acx_simple_profile to:

  * its median is _simple_ref.score_exact, its index the first minimum, its record follows the definitions;
  * every row of every continuous case the GPU test hands to the device is DECIDED (the gap between the two smallest exact
    distances exceeds 2 * score_bound), so the device must return the exact index there;
  * the integer cases are exact in f64 in both forms of the distance, and hold what they are built for (ties in every row of
    the periodic B, a tie with column 0, a tie at the first row of the second row group, a silent B, two longest runs, runs
    across the row-group hand-over and the 64-row chunk boundary, A contained in B);
  * every mutant reference changes an index or a record of the exact case set at every L the GPU test runs it at.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _simple_ref as R                  # noqa: E402
from tests import _simple_profile_ref as P          # noqa: E402

DECIDED_LS = tuple(range(1, 17))              # every L the GPU test runs every_L_case at (probe_case: PROBE_LS)


def test_reference_is_score_exact_and_first_minimum():
    rng = np.random.default_rng(3)
    for L, do_oti in ((1, True), (4, False), (10, True), (16, True)):
        A, B = R.frames(rng, 90 + L), R.frames(rng, 75 + L)
        mp, mpi, gap, s, bound = P.reference(A, B, L, do_oti)
        ref, shift, _, _ = R.score_exact(A, B, L, do_oti)
        assert s["score"] == ref and s["shift"] == shift
        assert np.array_equal(mp, R.profile_exact(A, B, L, shift))
        D = P.distances(A, B, L, shift)
        for a in range(len(mp)):
            assert D[a, mpi[a]] == mp[a] and np.all(D[a, :mpi[a]] > mp[a])
        assert np.all(gap >= 0) and bound > 0


def test_summary_definitions():
    mp = np.array([3.0, 1.0, 2.0, 1.0, 5.0, 4.0, 6.0, 7.0])
    mpi = np.array([4, 5, 6, 0, 1, 2, 9, 3], np.int32)
    s = P.summary(mp, mpi, 3, 7)
    # runs: rows 0-2 (columns 4-6) and rows 3-5 (columns 0-2), both of three rows: the first wins
    assert (s["q0"], s["r0"], s["q1"], s["r1"], s["run_len"]) == (0, 4, 2, 6, 3)
    assert s["q_span"] == (0, 4) and s["r_span"] == (4, 8)
    # the smallest value stands twice: the first row wins
    assert (s["best_q"], s["best_r"], s["best_dist"]) == (1, 5, 1.0)
    assert s["score"] == -3.5 and s["shift"] == 7
    assert P.longest_run(np.array([5], np.int32)) == (0, 1)
    assert P.longest_run(np.array([0, 0, 0], np.int32)) == (0, 1)
    assert P.longest_run(np.array([2, 7, 8, 9, 1], np.int32)) == (1, 3)


@pytest.mark.parametrize("L", DECIDED_LS)
def test_every_continuous_row_is_decided(L):
    """The cap of the GPU test: no undecided row in every_L_case (with and without OTI) and in probe_case."""
    rows = zeros = 0
    smallest = np.inf
    calls = [R.every_L_case(L, do_oti) + (do_oti,) for do_oti in (1, 0)]
    if L in R.PROBE_LS:
        calls.append(R.probe_case(L) + (0,))
    for tracks, pairs, do_oti in calls:
        for i, j in pairs:
            bad, n, z, g = P.undecided_rows(tracks[i], tracks[j], L, bool(do_oti))
            assert bad == 0, (L, do_oti, i, j, bad, g)
            rows, zeros, smallest = rows + n, zeros + z, min(smallest, g)
    print("L=%d: %d rows, 0 undecided, %d exact zeros, smallest gap %.3g bounds" % (L, rows, zeros, smallest))
    assert smallest > 2.0


@pytest.mark.parametrize("L", P.EXACT_LS)
def test_integer_cases_are_exact_and_hold_their_property(L):
    S = R.stride(L)
    cases = {name: (A, B) for name, A, B in P.exact_case_set(L)}
    for name, (A, B) in cases.items():
        assert set(np.unique(A)) <= {0.0, 1.0, 2.0} and set(np.unique(B)) <= {0.0, 1.0, 2.0}, name
        # both forms of the distance are exact: the same bits
        assert np.array_equal(P.dot_form(A, B, L), P.distances(A, B, L, 0)), name
    ref = {name: P.reference(A, B, L, False) for name, (A, B) in cases.items()}

    def ties(name):
        A, B = cases[name]
        D = P.distances(A, B, L, 0)
        return np.sum(D == D.min(1, keepdims=True), axis=1)

    # the periodic B: columns b and b + 70 tie in every one of the 151 rows; row 0 is zero at 62 and 132 (lanes 62 and 4)
    A, B = cases["period"]
    mp, mpi = ref["period"][:2]
    t = ties("period")
    assert len(mp) == 151 and np.all(t >= 2) and np.all(mpi < 70)
    D0 = P.distances(A[:L], B, L, 0)[0]
    assert mpi[0] == 62 and mp[0] == 0.0 and D0[132] == 0.0
    assert t[S + 1] >= 2                                     # a tie at the first row of the second row group
    # a tie between column 0 and a later column, in row 0, inside group 0 and at the first row of group 1
    mp, mpi = ref["col0_tie"][:2]
    D = P.distances(*cases["col0_tie"], L, 0)
    for r in (0, 5 + L, S + 1):
        assert mpi[r] == 0 and mp[r] == 0.0 and D[r, L + 9] == 0.0, r
    # a silent B
    mp, mpi, _, s, _ = ref["silent"]
    assert np.all(mpi == 0) and s["run_len"] == 1 and (s["q0"], s["r0"]) == (0, 0)
    # two longest runs of equal length: the first wins
    _, mpi, _, s, _ = ref["two_runs"]
    starts, lens = P._runs(mpi)
    assert np.sum(lens == lens.max()) >= 2 and s["q0"] == starts[np.argmax(lens)] < starts[len(lens) - 1 - np.argmax(lens[::-1])]
    # runs across the hand-over of row group 0 and across rows 63 | 64
    s = ref["handover_run"][3]
    assert s["q0"] <= S and s["q1"] >= S + 1
    s = ref["chunk_run"][3]
    assert s["q0"] <= 63 and s["q1"] >= 64
    # A wholly inside B
    mp, mpi, _, s, _ = ref["contained"]
    assert s["run_len"] == len(mp) == 140 and np.all(mp == 0.0) and np.array_equal(mpi, 20 + np.arange(140))


@pytest.mark.parametrize("L", P.EXACT_LS)
def test_every_mutant_is_detected(L):
    assert P.undetected(P.exact_case_set(L), L) == []


def test_lds_steps():
    steps = P.step_lengths()
    assert len(steps) == 3 and [P.waves_per_workgroup(n) for n in steps] == [3, 2, 1]
    assert [P.waves_per_workgroup(n - 1) for n in steps] == [4, 3, 2]
    assert P.profile_smem(6000) <= 160 * 1024                # the 6000-frame limit fits one wave


def test_record_layout_and_export():
    from acoss_amd import _lib
    dt = _lib.SIMPLE_ALIGNMENT_DTYPE
    assert dt.itemsize == 64 and dt.fields["score"][1] == 0 and dt.fields["best_dist"][1] == 8
    assert [dt.fields[f][1] for f in ("shift", "best_q", "best_r", "q0", "r0", "q1", "r1", "q_span", "r_span", "run_len")] == \
        [16, 20, 24, 28, 32, 36, 40, 44, 52, 60]
    header = open(os.path.join(ROOT, "include", "acx.h")).read()
    assert _lib.EXPORTS.count("acx_simple_profile") == 1 and "int acx_simple_profile(" in header
    assert hasattr(_lib.load(), "acx_simple_profile")
