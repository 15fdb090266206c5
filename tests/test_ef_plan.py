"""
CPU-only: the EarlyFusion batch plan as the library reports it without a device (acx_ef_plan -> acoss_amd/csrc/ef_plan.hpp, the
functions run_ef_impl itself calls): where the kernel classes step, which column kernel a neighbourhood size takes, csm_to_binary's
neighbours per row, how a list splits into batches of equal size under a scratch limit, which lists are refused with which code, the
run order, and what the per-process switch ACX_EF_ROWSTAT2 changes.

The expectations are written from the rules, not read off the code under test: a pair of M x N blocks keeps three (the float path or
the debug entry: four) matrices of M x pitch(N) floats, pitch = the next multiple of 64, and for K > 16 three transposed ones of
N x pitch(M); a list beyond the limit runs in batches of min(limit, total / ceil(total / limit) * 1.02 + 2^22) floats, filled greedily
in run order, at most 65535 pairs each.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from acoss_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pitch(n):
    return (np.asarray(n, np.int64) + 63) // 64 * 64


def _need(M, N, mats=3, transposed=False):
    M, N = np.asarray(M, np.int64), np.asarray(N, np.int64)
    return mats * M * _pitch(N) + (3 * N * _pitch(M) if transposed else 0)


def _names(rec):
    return {st: _lib.ef_kernel_name(st, rec[st]) for st in _lib.EF_PLAN_STAGES}


def _self_pair_classes():
    """n -> (path, the four kernel names) of the self pair of a track of n blocks, each in a list of its own."""
    out = {}
    for n in range(1, 1101):
        rec = _lib.ef_plan([n], [[0, 0]])
        assert len(rec) == 1 and (rec["M"][0], rec["N"][0], rec["batch"][0], rec["run_pos"][0]) == (n, n, 0, 0)
        out[n] = (int(rec["path"][0]), _names(rec[0]))
    return out


NARROW = dict(row_kernel="ef_rowstat2_kernel", col_kernel="ef_colstat_kernel<10>", fuse_kernel="ef_rowstat_kernel<2, true>",
              sw_kernel="sw_bits_h16_kernel<8>")
WIDE = dict(row_kernel="ef_rowstat_kernel<4, false>", col_kernel="ef_colstat_kernel<10>", fuse_kernel="ef_rowstat_kernel<4, true>",
            sw_kernel="sw_bits_h16_kernel<16>")
LONG = dict(row_kernel="ef_rowstat_long_kernel", col_kernel="ef_colstat_kernel<10>", fuse_kernel="ef_fuse_kernel",
            sw_kernel="sw_long_kernel")


def _check_classes(classes, narrow):
    for n, (path, names) in classes.items():
        want = narrow if n <= 512 else (WIDE if n <= 1024 else LONG)
        assert names == want, (n, names)
        assert path == (1 if n > 1024 else 0), n


def test_kernel_classes_step_at_513_and_1025():
    classes = _self_pair_classes()
    _check_classes(classes, NARROW)
    steps = [n for n in range(2, 1101) if classes[n] != classes[n - 1]]
    assert steps == [513, 1025]


_SWITCH_SNIPPET = r'''
import json, sys
sys.path.insert(0, %(root)r)
from tests import test_ef_plan as T
print(json.dumps({str(n): v for n, v in T._self_pair_classes().items()}))
'''


def test_rowstat2_switch_removes_the_two_row_class_and_nothing_else():
    """The switch is read once per process: a child (no GPU is opened: the report needs none)."""
    env = dict(os.environ, ACX_EF_ROWSTAT2="0")
    r = subprocess.run([sys.executable, "-c", _SWITCH_SNIPPET % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    classes = {int(n): (v[0], v[1]) for n, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}
    assert sorted(classes) == list(range(1, 1101))
    _check_classes(classes, dict(NARROW, row_kernel="ef_rowstat_kernel<2, false>"))


def test_column_statistics_by_neighbourhood_size():
    blocks, pairs = [100, 300, 513], [[0, 1], [1, 2], [2, 0]]
    M, N = np.array([100, 300, 513]), np.array([300, 513, 100])
    for K, want in ((1, "ef_colstat_kernel<10>"), (10, "ef_colstat_kernel<10>"), (11, "ef_colstat_kernel<16>"),
                    (16, "ef_colstat_kernel<16>"), (17, "ef_rowstat_kernel on C^T"), (40, "ef_rowstat_kernel on C^T")):
        rec = _lib.ef_plan(blocks, pairs, K=K)
        assert {_lib.ef_kernel_name("col_kernel", k) for k in rec["col_kernel"]} == {want}, K
        assert rec["need"].tolist() == _need(M, N, transposed=K > 16).tolist(), K           # K > 16: ctN = N, three matrices of N x pitch(M)
        # the row kernels go by the batch's longest side: a 513-block track anywhere in it
        assert {_lib.ef_kernel_name("row_kernel", k) for k in rec["row_kernel"]} == {"ef_rowstat_kernel<4, false>"}


def test_kbin_is_numpys_round():
    Ns = np.arange(1, 201)
    pairs = np.stack([np.arange(200), np.arange(200)], 1)
    for kappa in (0.1, 0.5):
        want = np.round(kappa * Ns.astype(np.float64)).astype(int)              # half to even, in f64
        assert _lib.ef_plan(Ns, pairs, kappa=kappa)["kbin"].tolist() == want.tolist(), kappa
    halves = [int(n) for n in Ns if n % 2 == 1]                                  # 0.5 N = x.5: to the even neighbour
    assert all(int(round(0.5 * n)) % 2 == 0 for n in halves) and len(halves) == 100
    assert int(np.round(0.1 * 5)) == 0 and int(np.round(0.1 * 15)) == 2 and int(np.round(0.1 * 25)) == 2
    assert _lib.ef_plan(Ns, pairs, kappa=0.0)["kbin"].tolist() == Ns.tolist()
    assert _lib.ef_plan(Ns, pairs, kappa=3)["kbin"].tolist() == [3] * 200
    with pytest.raises(_lib.AcxError, match="kappa must be >= 0") as e:
        _lib.ef_plan(Ns, pairs, kappa=-0.1)
    assert e.value.code == _lib.ACX_ERR_INVALID
    with pytest.raises(_lib.AcxError, match="K must be >= 1"):
        _lib.ef_plan(Ns, pairs, K=0)


# 15 tracks of 40 .. 140 blocks, all ordered pairs in sorted order: 225 pairs
BATCH_BLOCKS = [40, 57, 64, 65, 90, 127, 128, 129, 130, 133, 135, 136, 138, 139, 140]


def _batch_pairs():
    n = len(BATCH_BLOCKS)
    return np.array([[i, j] for i in range(n) for j in range(n)], np.int32)


def _want_batch_floats(total, limit_floats):
    if total <= limit_floats:
        return limit_floats
    nb = math.ceil(total / limit_floats)
    return min(limit_floats, int(total / nb * 1.02) + (1 << 22))


@pytest.mark.parametrize("K,limit_floats", [(10, 1 << 20), (10, 3_000_000), (17, 16_000_000), (17, 20_000_000), (17, 14_000_000), (17, 1 << 21)])
def test_batches_are_equalised_greedy_contiguous_and_within_the_limit(K, limit_floats):
    pairs = _batch_pairs()
    nb_ = np.array(BATCH_BLOCKS)
    need = _need(nb_[pairs[:, 0]], nb_[pairs[:, 1]], transposed=K > 16)
    total = int(need.sum())
    assert total > limit_floats > int(need.max())
    rec = _lib.ef_plan(BATCH_BLOCKS, pairs, K=K, scratch_limit=4 * limit_floats)
    assert rec["need"].tolist() == need.tolist() and rec["run_pos"].tolist() == list(range(len(pairs)))
    batch = rec["batch"].astype(int)
    assert batch[0] == 0 and set(np.diff(batch).tolist()) == {0, 1}          # contiguous runs of the list, in run order
    count = int(batch[-1]) + 1
    batch_floats = _want_batch_floats(total, limit_floats)
    for b in range(count):
        used = int(need[batch == b].sum())
        assert used <= batch_floats, (b, used, batch_floats)
        if b + 1 < count:                                                    # greedy: the next pair did not fit
            assert used + int(need[np.nonzero(batch == b + 1)[0][0]]) > batch_floats, (b, used)
    least = math.ceil(total / limit_floats)
    assert count >= least
    if batch_floats < limit_floats:
        # the equal-size rule applies: 2 % and 2^22 floats of slack over total / least hold `least` greedy batches -- each but the last
        # is filled to within one pair of batch_floats, and least * (one pair) stays below the slack
        assert least * int(need.max()) < 0.02 * total / least * least + least * (1 << 22)
        assert count == least, (count, least)
    else:
        # batches of the limit itself: a batch wastes less than one pair's need, so one more batch at the most here
        assert (least + 1) * (limit_floats - int(need.max())) >= total
        assert count in (least, least + 1), (count, least)


def test_the_equal_size_rule_applies_to_two_of_the_cases_above():
    pairs = _batch_pairs()
    nb_ = np.array(BATCH_BLOCKS)
    total = int(_need(nb_[pairs[:, 0]], nb_[pairs[:, 1]], transposed=True).sum())
    assert _want_batch_floats(total, 16_000_000) < 16_000_000 and _want_batch_floats(total, 20_000_000) < 20_000_000
    assert _want_batch_floats(total, 14_000_000) == 14_000_000 and _want_batch_floats(total, 1 << 21) == 1 << 21


def test_no_limit_is_one_batch_and_a_grid_dimension_splits_it():
    pairs = _batch_pairs()
    assert np.all(_lib.ef_plan(BATCH_BLOCKS, pairs)["batch"] == 0)
    rec = _lib.ef_plan([1], np.zeros((70000, 2), np.int32))
    assert np.all(rec["need"] == 3 * 64)
    assert rec["batch"].tolist() == [0] * 65535 + [1] * (70000 - 65535)


def test_refused_lists_return_the_runs_codes():
    blocks = [100, 0, 200]
    with pytest.raises(_lib.AcxError, match="track index out of range in pair 2") as e:
        _lib.ef_plan(blocks, [[0, 2], [2, 0], [0, 3], [3, 3]])
    assert e.value.code == _lib.ACX_ERR_INVALID
    with pytest.raises(_lib.AcxError, match="track index out of range in pair 1") as e:
        _lib.ef_plan(blocks, [[0, 2], [-1, 0]])
    assert e.value.code == _lib.ACX_ERR_INVALID
    with pytest.raises(_lib.AcxError, match=r"track without blocks \(pair 1\)") as e:
        _lib.ef_plan(blocks, [[0, 2], [2, 1], [1, 1]])
    assert e.value.code == _lib.ACX_ERR_SHORT
    # both in one list: the index error comes first, wherever the track without blocks stands
    with pytest.raises(_lib.AcxError, match="track index out of range in pair 2") as e:
        _lib.ef_plan(blocks, [[1, 0], [0, 2], [0, 7]])
    assert e.value.code == _lib.ACX_ERR_INVALID
    # a single pair beyond the limit: 3 x 200 x 128 floats
    assert len(_lib.ef_plan(blocks, [[0, 0], [2, 0]], scratch_limit=4 * 76800)) == 2
    with pytest.raises(_lib.AcxError, match="pair 1 does not fit the scratch limit") as e:
        _lib.ef_plan(blocks, [[0, 0], [2, 0]], scratch_limit=4 * 76799)
    assert e.value.code == _lib.ACX_ERR_NOMEM


def test_an_unsorted_list_is_planned_in_run_order_and_reported_in_the_callers():
    rng = np.random.default_rng(5)
    blocks = rng.integers(40, 141, 12)
    pairs = rng.integers(0, 12, (150, 2)).astype(np.int32)
    pairs[17] = pairs[3]                                                    # (equal pairs keep their order: a stable sort)
    order = np.lexsort((np.arange(150), pairs[:, 1], pairs[:, 0]))
    assert not np.array_equal(order, np.arange(150))
    need = _need(blocks[pairs[:, 0]], blocks[pairs[:, 1]])
    limit_floats = int(need.sum()) // 3
    rec = _lib.ef_plan(blocks, pairs, scratch_limit=4 * limit_floats)
    assert rec["M"].tolist() == blocks[pairs[:, 0]].tolist() and rec["N"].tolist() == blocks[pairs[:, 1]].tolist()
    assert rec["need"].tolist() == need.tolist()
    assert rec["run_pos"][order].tolist() == list(range(150))
    batch = rec["batch"][order].astype(int)                                  # batches are contiguous runs of the RUN order
    assert batch[0] == 0 and set(np.diff(batch).tolist()) == {0, 1} and batch[-1] >= 2
    # the same list sorted by the caller: untouched, and the same plan
    srt = _lib.ef_plan(blocks, pairs[order], scratch_limit=4 * limit_floats)
    assert srt["run_pos"].tolist() == list(range(150))
    for name in rec.dtype.names:
        assert np.array_equal(srt[name], rec[name][order]), name


def test_one_long_track_turns_every_batch_to_the_float_path():
    blocks = [60, 100, 140, 1025]
    pairs = np.array([[i, j] for i in range(3) for j in range(3)] + [[3, 0]], np.int32)
    M, N = np.array(blocks)[pairs[:, 0]], np.array(blocks)[pairs[:, 1]]
    short = _lib.ef_plan(blocks, pairs[:-1])
    assert np.all(short["path"] == 0) and short["need"].tolist() == _need(M[:-1], N[:-1]).tolist()
    limit_floats = 4 * 1025 * 64                                             # the long pair's need: a batch of its own
    rec = _lib.ef_plan(blocks, pairs, scratch_limit=4 * limit_floats)
    assert np.all(rec["path"] == 1) and rec["need"].tolist() == _need(M, N, mats=4).tolist()
    assert rec["batch"][-1] == rec["batch"].max() >= 1 and np.sum(rec["batch"] == rec["batch"][-1]) == 1
    for r in rec[:-1]:                                                       # short batches: the float kernels of their own class
        assert _names(r) == dict(row_kernel="ef_rowstat2_kernel", col_kernel="ef_colstat_kernel<10>", fuse_kernel="ef_fuse_kernel",
                                 sw_kernel="sw_kernel<8>")
    assert _names(rec[-1]) == dict(row_kernel="ef_rowstat_long_kernel", col_kernel="ef_colstat_kernel<10>", fuse_kernel="ef_fuse_kernel",
                                   sw_kernel="sw_kernel<8>")
    # the debug entry that keeps the fused matrix: four matrices on the bit path too
    kept = _lib.ef_plan(blocks, pairs[:-1], keep_fused=True)
    assert np.all(kept["path"] == 0) and kept["need"].tolist() == _need(M[:-1], N[:-1], mats=4).tolist()
