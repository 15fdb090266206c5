"""
GPU test (run with -m gpu on a real MI355X): the EarlyFusion run follows the plan the library reports without a device (acx_ef_plan ->
acoss_amd/csrc/ef_plan.hpp).  Three small lists on one pool of 12 tracks with 3, 64, 65, 140, 512, 513 and 1025 blocks: the bit path
in three batches of equal size, the float path (a list with the 1025-block track), and the transposed row pass (K = 17).  Held: the
run opens one GEMM scope per batch of the plan (what tests/test_gpu_ef_backend.py already relies on), and a pair's four scores in
the list are those of the same pair run alone, bit for bit -- whichever batch, run position and kernel class the list gave it.
"""
import math

import numpy as np
import pytest

from . import test_gpu_ef_backend as B

pytestmark = pytest.mark.gpu

BLOCKS = [3, 64, 65, 140, 512, 513, 1025, 512, 513, 140, 512, 513]
LONG = 6
BIG = [4, 5, 7, 8, 10, 11]                       # the tracks of 512 and 513 blocks


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    c.ef_upload_pool([B._track(nb, 4200 + k) for k, nb in enumerate(BLOCKS)])
    yield c
    c.close()


@pytest.fixture(scope="module")
def alone():
    """(q, r, K) -> the scores of the pair run as a list of its own; computed once per pair, never changed."""
    return {}


def _shuffled(pairs, seed):
    pairs = np.asarray(pairs, np.int32)
    return np.ascontiguousarray(pairs[np.random.default_rng(seed).permutation(len(pairs))])


def _lists():
    bits = [(q, r) for q in BIG for r in BIG] + [(0, 1), (1, 2), (2, 3), (3, 0), (9, 9), (1, 4), (5, 2)]
    flt = [(LONG, 0), (LONG, 3), (1, LONG), (2, 1), (3, 9), (0, 0), (4, 2), (LONG, 5)]
    tr = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 3), (9, 0), (2, 2), (7, 1)]
    return dict(bits=(_shuffled(bits, 1), 10), float=(_shuffled(flt, 2), 10), transposed=(_shuffled(tr, 3), 17))


def _limit_floats(name, plan):
    """The scratch limit of a case, in floats, from the needs the plan reports (which tests/test_ef_plan.py holds against the formula)."""
    total = int(plan["need"].sum())
    if name == "bits":
        # three batches whose size the equal-size rule sets: total / 3 * 1.02 + 2^22 floats, below a limit of just under total / 2
        limit = total // 2 - (1 << 16)
        assert math.ceil(total / limit) == 3 and int(total / 3 * 1.02) + (1 << 22) < limit
        return limit
    return max(int(plan["need"].max()), total // 2)


@pytest.mark.parametrize("name", ["bits", "float", "transposed"])
def test_the_run_follows_the_plan(ctx, alone, name):
    from acoss_amd import _lib
    pairs, K = _lists()[name]
    limit = _limit_floats(name, _lib.ef_plan(BLOCKS, pairs, K=K))
    plan = _lib.ef_plan(BLOCKS, pairs, K=K, scratch_limit=4 * limit)
    nbatch = int(plan["batch"].max()) + 1
    assert np.all(plan["path"] == (1 if name == "float" else 0))
    assert nbatch == 3 if name == "bits" else nbatch >= 2
    assert not np.array_equal(plan["run_pos"], np.arange(len(pairs)))          # (the list is not in run order)
    want_col = "ef_rowstat_kernel on C^T" if K > 16 else "ef_colstat_kernel<10>"
    assert {_lib.ef_kernel_name("col_kernel", k) for k in plan["col_kernel"]} == {want_col}
    ctx.set_scratch_limit(4 * limit)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        got = ctx.earlyfusion_pairs(pairs, K=K)
        launched = ctx.profile()["ef_gemm_kernel"]["launches"]                  # one timed GEMM scope per batch
    finally:
        ctx.profile_enable(False)
        ctx.set_scratch_limit(0)
    assert launched == nbatch, (launched, nbatch)
    for k, (q, r) in enumerate(pairs):
        key = (int(q), int(r), K)
        if key not in alone:
            alone[key] = ctx.earlyfusion_pairs(np.array([[q, r]], np.int32), K=K)[0].copy()
        assert np.array_equal(got[k].view(np.uint32), alone[key].view(np.uint32)), (name, k, key, got[k], alone[key], plan[k])
