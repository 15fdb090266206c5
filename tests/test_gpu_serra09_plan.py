"""
GPU test (run with -m gpu on a real MI355X): the run launches what the device-free report (acx_serra09_plan) says it launches.  The
per-kernel profile counts launches by family; the report of the same list gives the class keys, and from them the count the batch
loop of run_serra09_impl must reach: one column pass per (cr, cq) key, one row pass and one sweep per cr.
"""
import numpy as np
import pytest

from tests import _serra09_shapes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    c.profile_enable(True)
    yield c
    c.profile_enable(False)
    c.close()


def _launches(ctx, call, *args):
    ctx.profile_reset()
    out = call(*args)
    return out, {name: v["launches"] for name, v in ctx.profile().items() if v["launches"]}


@pytest.mark.parametrize("m", [9, 10])
def test_band_and_sweep_launches_are_the_plans(ctx, m):
    from acoss_amd import _lib
    d = S.edge_set(m)
    p = _lib.serra09_params(m=m)
    rec = _lib.serra09_plan(np.diff(d["offsets"]), d["pairs"], p)
    assert np.all(rec["batch"] == 0) and rec["cr"].max() == 4
    keys = {(int(r["cr"]), int(r["cq"])) for r in rec}
    rows = {cr for cr, _ in keys}
    band, sweeps = len(keys) + len(rows), len(rows)
    print("m=%d: %d keys, %d row classes -> %d band launches, %d sweeps" % (m, len(keys), len(rows), band, sweeps))
    assert (band, sweeps) == (30, 5)                        # the figures of the commit before the plan header, measured
    ctx.upload_pool(d["frames"], d["offsets"])
    _, n = _launches(ctx, ctx.serra09_pairs, d["pairs"], p)
    print("serra09_pairs:", n)
    assert n["band_kernel"] == band and n["qmax_bits_kernel"] == sweeps and n["oti_kernel"] == 1
    assert "csm_long_kernel" not in n and "rowsel_long_kernel" not in n
    _, n = _launches(ctx, ctx.chenfusion_pairs, d["pairs"], p)
    print("chenfusion_pairs:", n)
    assert n["band_kernel"] == band and n["qmax_bits_kernel"] == 2 * sweeps == 10
    assert "csm_long_kernel" not in n and "rowsel_long_kernel" not in n


def test_a_stack_of_17_streams_every_pair(ctx):
    """The smallest shape that reaches the streaming kernels: m = 17 (> MAX_M), four i.i.d. tracks of 60 frames, all six pairs."""
    import oracle
    from acoss_amd import _lib, synth
    m = 17
    rng = np.random.default_rng(17)
    frames, offsets = synth.pack([S._iid(rng, 60) for _ in range(4)])
    pairs = oracle.all_pairs(4, True).astype(np.int32)
    p = _lib.serra09_params(m=m)
    rec = _lib.serra09_plan(np.diff(offsets), pairs, p)
    assert len(rec) == 6 and np.all(rec["cr"] == 5) and np.all(rec["cq"] == 5) and np.all(rec["Mq"] == 60 - m)
    assert {_lib.serra09_family_name(f, m) for f in rec["row_family"]} == {_lib.serra09_family_name(6, m)}
    ctx.upload_pool(frames, offsets)
    got, n = _launches(ctx, ctx.serra09_pairs, pairs, p)
    print("m=17:", n)
    assert "band_kernel" not in n
    assert n["csm_long_kernel"] == 1 and n["rowsel_long_kernel"] == 1 and n["qmax_bits_kernel"] == 1
    assert np.array_equal(got, oracle.serra09_pairs(frames, offsets, pairs, oracle.serra09_params(m=m)))


def test_long_sides_stream_in_one_launch_each(ctx):
    """long_set(9): 103 pairs with a side beyond 2041 cells, m = 9.  The report puts them all into class 5 of one batch, and the run
    launches no band kernel: one csm_long_kernel, one rowsel_long_kernel and one sweep per call, two sweeps for chenfusion_pairs."""
    from acoss_amd import _lib
    m = 9
    d = S.long_set(m)
    p = _lib.serra09_params(m=m)
    rec = _lib.serra09_plan(np.diff(d["offsets"]), d["pairs"], p)
    assert len(rec) == 103 and np.all(rec["batch"] == 0) and np.all(rec["cr"] == 5) and np.all(rec["cq"] == 5) and np.all(rec["sweep_cols"] == 0)
    assert {_lib.serra09_family_name(f, m) for f in rec["row_family"]} == {"csm_long_kernel + rowsel_long_kernel"}
    ctx.upload_pool(d["frames"], d["offsets"])
    _, n = _launches(ctx, ctx.serra09_pairs, d["pairs"], p)
    print("serra09_pairs:", n)
    assert "band_kernel" not in n
    assert n["csm_long_kernel"] == 1 and n["rowsel_long_kernel"] == 1 and n["qmax_bits_kernel"] == 1 and n["oti_kernel"] == 1
    _, n = _launches(ctx, ctx.chenfusion_pairs, d["pairs"], p)
    print("chenfusion_pairs:", n)
    assert "band_kernel" not in n
    assert n["csm_long_kernel"] == 1 and n["rowsel_long_kernel"] == 1 and n["qmax_bits_kernel"] == 2
