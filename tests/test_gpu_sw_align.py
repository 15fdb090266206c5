"""
The EarlyFusion alignment on the device (ef_align_kernel through acx_sw_align_binary, acx_ef_align and EarlyFusion.align*),
held against tests/_sw_align_ref.py (pinned to the oracle's score by tests/test_sw_align_ref.py).  Every comparison is exact: the
score's bits, the four coordinates, every cell of the path.
"""
import ctypes

import numpy as np
import pytest

from . import _ef_backend_ref as backend
from . import _sw_align_ref as ref

pytestmark = pytest.mark.gpu

DIMS = (40, 100, 96)                       # small feature widths: the GEMMs cost nothing
SMALL = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65]
# above 65: the diagonal of {511, 512, 513, 1023, 1024} and pairs that mix the classes (lane edges at multiples of 16, the pitch
# at multiples of 64, the score kernels' width class at 512)
LARGE = [(511, 511), (512, 512), (513, 513), (1023, 1023), (1024, 1024), (511, 1024), (1024, 511), (513, 1023), (1023, 513),
         (512, 513), (513, 512), (17, 1024), (1024, 17), (65, 1023), (1023, 65), (4, 1024), (1024, 4), (3, 1024), (1024, 1)]


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _rec(al):
    """A structured row -> (f32 score, q0, r0, q1, r1)."""
    return (np.float32(al["score"]), int(al["q0"]), int(al["r0"]), int(al["q1"]), int(al["r1"]))


def _same(got, want):
    return np.float32(got[0]).view(np.uint32) == np.float32(want[0]).view(np.uint32) and tuple(got[1:]) == tuple(want[1:])


def _check_dp(ctx, B, where, want=None):
    """acx_sw_align_binary on B against statement 2 (and statement 1 up to 64 x 64); the record alone is the same bytes; the score is
    the bit kernel's."""
    al, cells = ctx.sw_align_binary(B)
    rec = _rec(al[0])
    wrec, wcells = want if want is not None else ref.align_forward(B)
    assert _same(rec, wrec) and np.array_equal(cells, wcells), (where, rec, wrec, cells.tolist()[:8], wcells.tolist()[:8])
    if max(B.shape) <= 64:
        trec, tcells = ref.align_traceback(B)
        assert _same(rec, trec) and np.array_equal(cells, tcells), (where, "statement 1", rec, trec)
    assert cells.dtype == np.int32 and cells.shape == (len(wcells), 2)
    ref.check_path(tuple(wrec), cells, B.shape)
    assert ctx.sw_align_binary(B, paths=False).tobytes() == al.tobytes(), (where, "record alone")
    assert np.float32(ctx.sw_bits_binary(B)).view(np.uint32) == np.float32(rec[0]).view(np.uint32), (where, "score")
    return rec, cells


def _random(rng, M, N, density):
    return ref.random_plot(rng, M, N, density) if min(M, N) >= 4 else (rng.random((M, N)) < density).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------
# a. the DP alone
# ------------------------------------------------------------------------------------------------------------------
def test_hand_checked_plots(ctx):
    for name, B, want, cells in ref.hand_checked():
        _check_dp(ctx, B, name, (want, cells))
    for B in ref.no_match_plots():
        rec, cells = _check_dp(ctx, B, B.shape)
        assert tuple(rec) == ref.NO_MATCH and len(cells) == 0


@pytest.mark.parametrize("density", [0.05, 0.1, 0.5, 0.9])
def test_random_small_plots_full_product(ctx, density):
    rng = np.random.default_rng(4100 + int(100 * density))
    matches = 0
    for M in SMALL:
        for N in SMALL:
            rec, cells = _check_dp(ctx, _random(rng, M, N, density), (M, N, density))
            assert (rec[0] > 0) == (min(M, N) >= 4)
            matches += rec[0] > 0
    assert matches == 64


@pytest.mark.parametrize("shape", LARGE, ids=lambda s: "%dx%d" % s)
def test_random_large_plots(ctx, shape):
    M, N = shape
    rng = np.random.default_rng(100 * M + N)
    for density in ((0.08, 0.5) if M * N > 300000 else (0.05, 0.1, 0.5, 0.9)):
        rec, cells = _check_dp(ctx, _random(rng, M, N, density), (M, N, density))
        assert (rec[0] > 0) == (min(M, N) >= 4)


def test_planted_path_across_every_lane_edge(ctx):
    """Mixed steps from (2, 2) to the last counted column of a 1024-column plot, in low-density noise: the path crosses all 63 lane
    edges (multiples of 16) and both halves of every code word."""
    rng = np.random.default_rng(5)
    B = (rng.random((1024, 1024)) < 0.02).astype(np.uint8)
    steps = [(1, 1)] * 4 + [(2, 1)] + [(1, 1)] * 4 + [(1, 2)]
    y, x, k, planted = 2, 2, 0, []
    while y <= 1022 and x <= 1022:
        planted.append((y, x))
        B[y, x] = 1
        y, x, k = y + steps[k % 10][0], x + steps[k % 10][1], k + 1
    rec, cells = _check_dp(ctx, B, "planted")
    assert rec[2] < 16 and rec[4] >= 1008 and len(cells) > 800
    on = len({tuple(c) for c in cells.tolist()} & set(planted))
    assert on >= 0.9 * len(planted), (on, len(planted))
    assert {tuple(s) for s in np.diff(cells, axis=0)} == ref.STEPS


@pytest.mark.parametrize("first,second,winner", [
    ((10, 5), (40, 70), 0), ((40, 5), (10, 70), 1),            # two lanes, the earlier row in the lower / in the higher lane
    ((20, 5), (20, 70), 0), ((20, 70), (20, 5), 1),            # two lanes, the same row: the smaller column
    ((10, 33), (40, 41), 0), ((40, 33), (10, 41), 1),          # one lane (columns 32 .. 47), both row orders
    ((20, 33), (20, 41), 0),                                   # one lane, the same row
    ((10, 15), (40, 16), 0), ((40, 15), (10, 16), 1),          # across a lane edge
])
def test_equal_maxima(ctx, first, second, winner):
    B = np.zeros((64, 128), np.uint8)
    for (a, b) in (first, second):
        for d in range(4):
            B[a + d, b + d] = 1
    rec, cells = _check_dp(ctx, B, (first, second))
    a, b = (first, second)[winner]
    assert tuple(rec) == (np.float32(3.3), a, b, a + 3, b + 3)


def test_refusals_leave_the_context_usable(ctx):
    B = ref.random_plot(np.random.default_rng(9), 40, 30, 0.2)
    with pytest.raises(ValueError, match=r"cap 29 is too small: 30 cells required"):
        ctx.sw_align_binary(B, cap=29)
    ctx.sw_align_binary(B, cap=30)
    with pytest.raises(NotImplementedError, match="alignment needs the bit path: at most 1024 blocks"):
        ctx.sw_align_binary(np.zeros((1025, 8), np.uint8))
    with pytest.raises(NotImplementedError, match="alignment needs the bit path: at most 1024 blocks"):
        ctx.sw_align_binary(np.zeros((8, 1025), np.uint8), paths=False)
    C = B.copy()
    C[7, 7] = 2
    with pytest.raises(ValueError, match="non-binary"):
        ctx.sw_align_binary(C)
    _check_dp(ctx, B, "after the refusals")


# ------------------------------------------------------------------------------------------------------------------
# b. the product path
# ------------------------------------------------------------------------------------------------------------------
BLOCKS = [4, 63, 64, 65, 512, 513, 1024, 1025]
# sorted by (first, second): every track of up to 1024 blocks as rows and as columns, wide and narrow, tall and flat
PAIRS = np.array([(0, 1), (0, 6), (1, 2), (2, 3), (3, 1), (3, 4), (4, 5), (5, 4), (5, 6), (6, 0), (6, 5)], np.int32)
PLANES = ("mfccs", "ssms", "chromas", "early")


def _track(nb, seed):
    rng = np.random.default_rng(seed)
    return dict(mfccs=rng.standard_normal((nb, DIMS[0])).astype(np.float32), ssms=(2 * rng.random((nb, DIMS[1]))).astype(np.float32),
                chromas=(rng.random((nb, DIMS[2])).astype(np.float32) ** 3 + 1e-3), chroma_med=rng.random(12) ** 2)


def _tracks():
    tracks = [_track(nb, 31000 + k) for k, nb in enumerate(BLOCKS)]
    rng = np.random.default_rng(31999)
    for a, b, at_a, at_b, m in ((4, 5, 100, 300, 60), (5, 6, 20, 700, 80), (2, 3, 5, 9, 30), (6, 5, 400, 100, 50)):
        for key in ("mfccs", "ssms", "chromas"):          # shared excerpts: alignments longer than noise gives
            tracks[b][key][at_b:at_b + m] = tracks[a][key][at_a:at_a + m] + 0.02 * rng.standard_normal((m, tracks[a][key].shape[1])).astype(np.float32)
    return tracks


@pytest.fixture(scope="module")
def pool(ctx):
    ctx.ef_upload_pool(_tracks())
    return ctx


@pytest.fixture(scope="module")
def expected(pool):
    """Per pair of PAIRS: the four plots as the selection kernels left them (ef_debug_bits), their answers by statement 2, and the
    listed scores.  Computed once, shared, never changed."""
    listed = pool.earlyfusion_pairs(PAIRS)
    out = []
    for k in range(len(PAIRS)):
        db = pool.ef_debug_bits(PAIRS, k)
        assert np.array_equal(db["scores"], listed)
        N = BLOCKS[PAIRS[k, 1]]
        plots = []
        for s in range(4):
            B, pads = backend.unpack_bits(db["bits"][s], N)
            assert pads == 0 and B.shape == (BLOCKS[PAIRS[k, 0]], N)
            plots.append(B)
        out.append(dict(plots=plots, answers=[ref.align_forward(B) for B in plots]))
    return listed, out


def _profile_launches(c, name):
    return c.profile()[name]["launches"]


@pytest.mark.parametrize("plane", range(4), ids=PLANES)
def test_product_path_every_plane(pool, expected, plane):
    listed, exp = expected
    al, off, cells = pool.ef_align(PAIRS, plane=plane, paths=True)
    alone = pool.ef_align(PAIRS, plane=plane)
    assert alone.tobytes() == al.tobytes(), "the records are the same bytes with and without the paths"
    assert off[0] == 0 and off[-1] == len(cells) and np.all(np.diff(off) >= 0)
    longest = 0
    for k in range(len(PAIRS)):
        wrec, wcells = exp[k]["answers"][plane]
        got = cells[off[k]:off[k + 1]]
        assert _same(_rec(al[k]), wrec) and np.array_equal(got, wcells), (PAIRS[k].tolist(), plane, _rec(al[k]), wrec)
        assert al["score"][k].view(np.uint32) == listed[k, plane].view(np.uint32), (PAIRS[k].tolist(), plane, "earlyfusion_pairs")
        ref.check_path(tuple(wrec), got, exp[k]["plots"][plane].shape)
        longest = max(longest, len(got))
    print("plane %s: longest path %d cells" % (PLANES[plane], longest))
    assert longest >= 2


def test_list_order_does_not_matter(pool, expected):
    listed, exp = expected
    order = np.random.default_rng(3).permutation(len(PAIRS))
    mixed = np.ascontiguousarray(PAIRS[order])
    for lst, idx in ((mixed, order), (np.ascontiguousarray(mixed[::-1]), order[::-1])):
        al, off, cells = pool.ef_align(lst, plane=3, paths=True)
        for k, src in enumerate(idx):
            wrec, wcells = exp[src]["answers"][3]
            assert _same(_rec(al[k]), wrec) and np.array_equal(cells[off[k]:off[k + 1]], wcells), (k, src)
    # a pair listed twice gets its answer twice
    twice = np.ascontiguousarray(np.concatenate([PAIRS[3:5], PAIRS[3:5]]))
    al = pool.ef_align(twice, plane=0)
    assert al[:2].tobytes() == al[2:].tobytes() and _same(_rec(al[0]), exp[3]["answers"][0][0])


# sorted by (first, second), as ef_debug_bits wants its list
SHORT_PAIRS = np.array([(0, 1), (1, 0), (1, 2), (1, 3), (2, 1), (2, 3), (3, 1), (3, 2)], np.int32)


def _short_reference(pool):
    """The list's answer in one batch, which is statement 2's for the plots of that batch."""
    al, off, cells = pool.ef_align(SHORT_PAIRS, plane=3, paths=True)
    for k in range(len(SHORT_PAIRS)):
        B, _ = backend.unpack_bits(pool.ef_debug_bits(SHORT_PAIRS, k)["bits"][3], BLOCKS[SHORT_PAIRS[k, 1]])
        wrec, wcells = ref.align_forward(B)
        assert _same(_rec(al[k]), wrec) and np.array_equal(cells[off[k]:off[k + 1]], wcells), k
    return al, off, cells


def test_batches_and_chunks(pool, monkeypatch):
    """Two batches under a small scratch limit; more chunks than batches when a chunk holds fewer waves.  (Under the scratch limit
    alone a batch is never more than one chunk: a pair's direction plane is 1 / 48 of the float matrices the same pair holds in the
    batch, and a chunk may take half the limit.)"""
    want = _short_reference(pool)
    need = sum(12 * BLOCKS[i] * ((BLOCKS[j] + 63) // 64 * 64) for i, j in SHORT_PAIRS)
    pool.profile_enable(True)
    try:
        pool.set_scratch_limit(int(0.6 * need))
        pool.profile_reset()
        got = pool.ef_align(SHORT_PAIRS, plane=3, paths=True)
        batches, chunks = _profile_launches(pool, "sw_kernel"), _profile_launches(pool, "ef_align_kernel")
        assert batches == 2 and chunks == 2, (batches, chunks)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        monkeypatch.setenv("ACX_EF_ALIGN_WAVES", "3")
        pool.profile_reset()
        got = pool.ef_align(SHORT_PAIRS, plane=3, paths=True)
        batches, chunks = _profile_launches(pool, "sw_kernel"), _profile_launches(pool, "ef_align_kernel")
        assert batches == 2 and chunks > batches and chunks >= (len(SHORT_PAIRS) + 2) // 3, (batches, chunks)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        monkeypatch.delenv("ACX_EF_ALIGN_WAVES")
    finally:
        pool.set_scratch_limit(0)
        pool.profile_enable(False)


def test_refused_lists_launch_nothing(pool, expected):
    from acoss_amd import _lib
    listed, exp = expected
    pool.profile_enable(True)
    try:
        pool.profile_reset()
        bad = np.ascontiguousarray(np.concatenate([PAIRS[:3], [[2, 7]], PAIRS[3:]]).astype(np.int32))      # track 7: 1025 blocks
        with pytest.raises(NotImplementedError, match="alignment needs the bit path: at most 1024 blocks"):
            pool.ef_align(bad, plane=3)
        with pytest.raises(NotImplementedError, match="alignment needs the bit path: at most 1024 blocks"):
            pool.ef_align(bad[::-1].copy(), plane=3, paths=True)
        for plane in (-1, 4):
            with pytest.raises(ValueError, match=r"plane must be 0\.\.3"):
                pool.ef_align(PAIRS, plane=plane)
        with pytest.raises(ValueError, match="track index out of range in pair 2"):
            pool.ef_align(np.array([(6, 5), (0, 1), (0, 8)], np.int32), plane=3)
        bound = int(sum(min(BLOCKS[i], BLOCKS[j]) for i, j in PAIRS))
        with pytest.raises(ValueError, match=r"cap %d is too small: %d cells required" % (bound - 1, bound)):
            pool.ef_align(PAIRS, plane=3, paths=True, cap=bound - 1)
        # none of these refusals launched anything, the 1025-block lists included: no call has run since the reset
        assert all(v["launches"] == 0 for v in pool.profile().values()), pool.profile()
        # exactly one of path_off / cells: refused
        out = np.zeros(len(PAIRS), _lib.ALIGNMENT_DTYPE)
        off = np.zeros(len(PAIRS) + 1, np.int64)
        p = _lib.EfParams(0.1, 10)
        ip = PAIRS.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        assert pool._L.acx_ef_align(pool._h, ip, len(PAIRS), ctypes.byref(p), 3, out.ctypes.data, off.ctypes.data, None, 1 << 20) == -1
        assert pool._L.acx_ef_align(pool._h, ip, len(PAIRS), ctypes.byref(p), 3, out.ctypes.data, None, off.ctypes.data, 1 << 20) == -1
        assert all(v["launches"] == 0 for v in pool.profile().values()), pool.profile()
        # a valid call after the refusals succeeds
        al = pool.ef_align(PAIRS, plane=3)
        assert all(_same(_rec(al[k]), exp[k]["answers"][3][0]) for k in range(len(PAIRS)))
    finally:
        pool.profile_enable(False)


def test_profile_entry(pool):
    pool.profile_enable(True)
    try:
        pool.profile_reset()
        pool.earlyfusion_pairs(PAIRS)
        before = pool.profile()
        assert list(before)[-1] == "ef_align_kernel" and before["ef_align_kernel"] == dict(ms=0.0, launches=0, cells=0)
        pool.profile_reset()
        pool.ef_align(PAIRS, plane=2)
        after = pool.profile()
        assert after["ef_align_kernel"]["launches"] == 1 and after["ef_align_kernel"]["ms"] > 0
        assert after["ef_align_kernel"]["cells"] == sum(BLOCKS[i] * BLOCKS[j] for i, j in PAIRS)
        # the option adds its own launch and nothing else: every other entry counts what the call without it counts
        for name in before:
            if name != "ef_align_kernel":
                assert after[name]["launches"] == before[name]["launches"] and after[name]["cells"] == before[name]["cells"], name
        print("ef_align_kernel %.3f ms beside sw_kernel %.3f ms on the same %d pairs" % (after["ef_align_kernel"]["ms"], after["sw_kernel"]["ms"], len(PAIRS)))
    finally:
        pool.profile_enable(False)


# ------------------------------------------------------------------------------------------------------------------
# c. Python
# ------------------------------------------------------------------------------------------------------------------
def _dataset(tmp_path, n):
    path = tmp_path / "ds.csv"
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


@pytest.fixture()
def algo(tmp_path, monkeypatch):
    from acoss_amd.algorithms import EarlyFusion
    monkeypatch.chdir(tmp_path)
    blocks = [90, 120, 70, 100, 64, 130]
    tracks = [_track(nb, 52000 + k) for k, nb in enumerate(blocks)]
    rng = np.random.default_rng(52999)
    for key in ("mfccs", "ssms", "chromas"):             # the planted excerpt: blocks 20 .. 59 of track 0 are blocks 50 .. 89 of track 1
        tracks[1][key][50:90] = tracks[0][key][20:60] + 0.01 * rng.standard_normal((40, tracks[0][key].shape[1])).astype(np.float32)
    a = EarlyFusion(_dataset(tmp_path, len(blocks)), "feat/", shortname="efalign_gpu")
    a.set_block_features(tracks, ["w%d" % (i // 2) for i in range(len(blocks))])
    yield a
    a.cleanup_memmap()


def test_python_align_and_paths(algo):
    idxs = np.array([(0, 1), (1, 0), (2, 3), (5, 4), (4, 2)])
    for stype in PLANES:
        al = algo.align(idxs, similarity_type=stype)
        al2, paths = algo.align_paths(idxs, similarity_type=stype)
        assert al.dtype == algo.ALIGN_DTYPE and al.tobytes() == al2.tobytes() and len(paths) == len(idxs)
        sc = algo._context().earlyfusion_pairs(idxs.astype(np.int32), kappa=algo.kappa, K=algo.K)
        assert np.array_equal(al["score"].view(np.uint32), sc[:, PLANES.index(stype)].view(np.uint32))
        for k, p in enumerate(paths):
            assert p.dtype == np.int32 and p.ndim == 2 and p.shape[1] == 2
            if al["score"][k] > 0:
                assert tuple(p[0]) == (al["q0"][k], al["r0"][k]) and tuple(p[-1]) == (al["q1"][k], al["r1"][k])
                assert al["q_span"][k].tolist() == [al["q0"][k], al["q1"][k] + algo.blocksize - 1]
                assert al["r_span"][k].tolist() == [al["r0"][k], al["r1"][k] + algo.blocksize - 1]
            else:
                assert len(p) == 0 and al["q_span"][k].tolist() == [-1, -1] and al["q0"][k] == -1
    assert not any(np.any(D) for D in algo.Ds.values()), "Ds is not written"
    # the planted excerpt: prints, does not assert
    al, paths = algo.align_paths([(0, 1)], similarity_type="early")
    p = paths[0]
    share = float(np.mean(p[:, 1] - p[:, 0] == 30)) if len(p) else 0.0
    print("planted excerpt (blocks 20..59 of track 0 = 50..89 of track 1): score %.1f, q_span %s, r_span %s, %d cells, %.0f %% on the copy's diagonal"
          % (al["score"][0], al["q_span"][0].tolist(), al["r_span"][0].tolist(), len(p), 100 * share))


def test_python_align_match_paths_on_identify(algo):
    queries = [0, 3, 5]
    idx, score = algo.identify(queries, k=3)["early"]
    idx = idx.copy()
    idx[1, 2] = -1                                         # an empty slot
    al = algo.align_matches(queries, idx, similarity_type="early")
    al2, paths = algo.align_match_paths(queries, idx, similarity_type="early")
    assert al.shape == idx.shape and al.tobytes() == al2.tobytes()
    assert al["q0"][1, 2] == -1 and al["score"][1, 2] == 0 and al["r_span"][1, 2].tolist() == [-1, -1] and paths[1][2].shape == (0, 2)
    for i, q in enumerate(queries):
        for s in range(idx.shape[1]):
            if idx[i, s] < 0:
                continue
            one, p1 = algo.align_paths([(q, idx[i, s])])
            assert one[0].tobytes() == al[i, s].tobytes() and np.array_equal(p1[0], paths[i][s])
            # identify() of this symmetric class scored the cell (min, max): that pair's alignment has the listed score
            lo, hi = min(q, idx[i, s]), max(q, idx[i, s])
            assert algo.align([(lo, hi)])["score"][0].view(np.uint32) == score[i, s].view(np.uint32)
