"""
CPU-only: the Serra09 batch plan as the library reports it without a device (acx_serra09_plan -> acoss_amd/csrc/serra09_plan.hpp, the
functions run_serra09_impl itself calls): where the size classes step, how a list splits into batches under a scratch limit, which
pairs are refused with which code, and what the per-process switches ACX_BAND2 / ACX_QMAX_MULTI change.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from acoss_amd import _lib
from tests import _serra09_shapes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _self_pairs(Ms, m):
    """One track per embedded length (tau = 1, embed_full = 0: T = M + m frames), each paired with itself."""
    n = len(Ms)
    return [M + m for M in Ms], np.stack([np.arange(n), np.arange(n)], 1)


@pytest.mark.parametrize("m", [1, 9, 10, 16])
def test_classes_step_at_the_table_limits(m):
    Ms = list(range(1, 2101))
    rec = _lib.serra09_plan(*_self_pairs(Ms, m), _lib.serra09_params(m=m))
    assert rec["Mq"].tolist() == Ms and rec["Mr"].tolist() == Ms
    cr = rec["cr"].astype(int)
    assert np.array_equal(cr, rec["cq"])
    assert cr[0] == 0 and cr[-1] == 5 and np.all(np.diff(cr) >= 0)
    assert [Ms[i + 1] for i in np.nonzero(np.diff(cr))[0]] == [250, 506, 762, 1018, 2042]
    assert np.all(np.diff(cr) <= 1)
    # the sweep of a class: columns per lane and pairs per wave
    assert [(int(rec["sweep_cols"][M - 1]), int(rec["sweep_pack"][M - 1])) for M in S.UPPER + (2042,)] == \
        [(8, 4), (8, 2), (16, 1), (16, 1), (32, 1), (0, 1)]
    assert np.all(rec["row_family"][cr == 5] == 6) and np.all(rec["row_family"][cr < 5] < 6)


def test_a_stack_beyond_the_band_kernels_streams_every_pair():
    Ms = list(range(1, 2101, 7))
    rec = _lib.serra09_plan(*_self_pairs(Ms, 17), _lib.serra09_params(m=17))
    assert rec["Mq"].tolist() == Ms
    for name in ("cr", "cq"):
        assert np.all(rec[name] == 5)
    assert np.all(rec["row_family"] == 6) and np.all(rec["col_family"] == 6) and np.all(rec["sweep_cols"] == 0)
    assert "long" in _lib.serra09_family_name(6, 17)


def _need(rec):
    """Floats a band-class pair of the product path takes of the scratch limit: its bitmap alone (Mq rows of ceil((Mr + 7) / 64) u64
    words), a word counting as two floats."""
    return 2 * rec["Mq"].astype(np.int64) * ((rec["Mr"].astype(np.int64) + 7 + 63) // 64)


def test_batches_are_greedy_contiguous_and_within_the_limit():
    m = 9
    d = S.row_residue_set(m)
    lengths = np.diff(d["offsets"])
    p = _lib.serra09_params(m=m)
    limit = 1 << 18                       # bytes: 65536 floats (tests/test_gpu_serra09_shapes.py::test_debug_bits_wants_one_batch)
    rec = _lib.serra09_plan(lengths, d["pairs"], p, scratch_limit=limit)
    assert [(int(r["Mq"]), int(r["Mr"])) for r in rec] == [(int(d["M"][i]), int(d["M"][j])) for i, j in d["pairs"]]
    need = _need(rec)
    assert int(need.sum()) == 140422 and int(need.max()) == 12048
    batch = rec["batch"].astype(int)
    assert batch[0] == 0 and set(np.diff(batch).tolist()) == {0, 1}          # contiguous runs of the list, in list order
    nb = int(batch[-1]) + 1
    assert nb >= 3                                                          # 140422 floats do not fit two batches of 65536
    for b in range(nb):
        total = int(need[batch == b].sum())
        assert total <= limit // 4, (b, total)
        if b + 1 < nb:
            first_of_next = int(np.nonzero(batch == b + 1)[0][0])
            assert total + int(need[first_of_next]) > limit // 4, (b, total)
    # no limit: one batch
    assert np.all(_lib.serra09_plan(lengths, d["pairs"], p)["batch"] == 0)
    assert np.all(_lib.serra09_plan(lengths, d["pairs"], p, scratch_limit=4 * 140422)["batch"] == 0)
    assert _lib.serra09_plan(lengths, d["pairs"], p, scratch_limit=4 * 140421)["batch"].max() == 1


def test_refused_lists_return_the_runs_codes():
    m = 9
    d = S.row_residue_set(m)
    lengths = np.diff(d["offsets"])
    p = _lib.serra09_params(m=m)
    with pytest.raises(_lib.AcxError, match="does not fit the scratch limit") as e:
        _lib.serra09_plan(lengths, d["pairs"], p, scratch_limit=4 * 12047)       # the largest pair wants 12048 floats
    assert e.value.code == _lib.ACX_ERR_NOMEM
    assert _lib.serra09_plan(lengths, d["pairs"], p, scratch_limit=4 * 12048)["batch"].max() > 0
    with pytest.raises(_lib.AcxError, match="shorter than the delay-embedding stack") as e:
        _lib.serra09_plan([100, m], [[0, 0], [0, 1]], p)
    assert e.value.code == _lib.ACX_ERR_SHORT
    for bad in ([0, 2], [-1, 0]):
        with pytest.raises(_lib.AcxError, match="index out of range") as e:
            _lib.serra09_plan([100, 100], [[0, 1], bad], p)
        assert e.value.code == _lib.ACX_ERR_INVALID


_SWITCH_SNIPPET = r'''
import json, sys
sys.path.insert(0, %(root)r)
from acoss_amd import _lib
from tests import _serra09_shapes as S
out = {}
for m in (9, 10):
    rec = _lib.serra09_plan([M + m for M in S.UPPER], [[i, i] for i in range(5)], _lib.serra09_params(m=m))
    assert rec["cr"].tolist() == [0, 1, 2, 3, 4]
    out["m%%d" %% m] = [_lib.serra09_family_name(f, m) for f in rec["row_family"]]
    out["pack%%d" %% m] = rec["sweep_pack"].tolist()
    out["cols%%d" %% m] = rec["sweep_cols"].tolist()
print(json.dumps(out))
'''


def _plan_under(extra):
    env = dict(os.environ)
    for name in ("ACX_BAND2", "ACX_QMAX_MULTI", "ACX_QMAX_STREAM"):
        env.pop(name, None)
    env.update(extra)
    r = subprocess.run([sys.executable, "-c", _SWITCH_SNIPPET % {"root": ROOT}], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (extra, r.stdout, r.stderr)
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_switches_change_what_they_say_and_nothing_else():
    """The switches are read once per process: one child per setting (no GPU is opened: the report needs none).  ACX_BAND2 peels the band2
    classes off ONE BY ONE, cumulatively: 2 moves the four-row class 0 onto the two-row kernel; 1 also moves the 24-position class 2
    onto band_kernel<M, 4>; 0 also moves classes 0 and 1 onto band_kernel<M, 2> (the families
    tests/test_gpu_serra09_shapes.py::test_environment_variants_give_the_same_bits names).  So ACX_BAND2=1 differs from the default in
    classes {0, 2}, not in {2} alone: the launcher this table replaced read `four_rows` as false for '0', '1' AND '2', and ran class 0
    on band2_kernel<M, B2_NV, 32> with that setting.  The meaning of a switch is not this test's to change."""
    base = _plan_under({})
    assert base["m9"] == ["band2_kernel<M, B2_NV, 16>", "band2_kernel<M, B2_NV, 32>", "band2_kernel<M, B2_NV_MID, 32>",
                          "band_kernel<M<=9, 4>", "band_kernel<M<=9, 8>"]
    assert base["m10"] == ["band_kernel<M>=10, 2>"] * 2 + ["band_kernel<M>=10, 4>"] * 2 + ["band_kernel<M>=10, 8>"]
    assert base["pack9"] == base["pack10"] == [4, 2, 1, 1, 1] and base["cols9"] == base["cols10"] == [8, 8, 16, 16, 32]
    two, four = "band_kernel<M<=9, 2>", "band_kernel<M<=9, 4>"
    want = {"0": {0: two, 1: two, 2: four},
            "1": {0: "band2_kernel<M, B2_NV, 32>", 2: four},
            "2": {0: "band2_kernel<M, B2_NV, 32>"}}
    for value, moved in want.items():
        got = _plan_under({"ACX_BAND2": value})
        assert {c: f for c, f in enumerate(got["m9"]) if f != base["m9"][c]} == moved, value
        assert {k: v for k, v in got.items() if k != "m9"} == {k: v for k, v in base.items() if k != "m9"}, value      # m = 10, the sweeps
    got = _plan_under({"ACX_QMAX_MULTI": "0"})
    assert got["pack9"] == got["pack10"] == [1] * 5
    assert {k: v for k, v in got.items() if not k.startswith("pack")} == {k: v for k, v in base.items() if not k.startswith("pack")}
    assert _plan_under({"ACX_QMAX_STREAM": "0"}) == base          # (where the sweeps run is not part of the report)
