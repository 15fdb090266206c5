"""
The EarlyFusion alignment beyond 1024 blocks on the device (ef_align_long_kernel through acx_sw_align_long_binary, acx_ef_align_long
and EarlyFusion.align*), held against tests/_sw_align_ref.py::align_forward.  Every comparison is exact: the
score's bits, the four coordinates, every cell of the path.  tests/test_sw_align_long_ref.py shows on the CPU that the plots of
section a can see the kernel's strips, records, running best, reduction and code plane go wrong.
"""
import ctypes

import numpy as np
import pytest

from . import _ef_streaming_cases as S
from . import _sw_align_ref as ref
from . import _sw_align_strips as strips

pytestmark = pytest.mark.gpu

PLANES = ("mfccs", "ssms", "chromas", "early")


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
    """acx_sw_align_long_binary on B against align_forward; the record alone is the same bytes; the score is sw_binary's."""
    al, cells = ctx.sw_align_long_binary(B)
    rec = _rec(al[0])
    wrec, wcells = want if want is not None else ref.align_forward(B)
    assert _same(rec, wrec) and np.array_equal(cells, wcells), (where, rec, wrec, cells.tolist()[:8], wcells.tolist()[:8])
    assert cells.dtype == np.int32 and cells.shape == (len(wcells), 2)
    ref.check_path(tuple(wrec), cells, B.shape)
    assert ctx.sw_align_long_binary(B, paths=False).tobytes() == al.tobytes(), (where, "record alone")
    assert np.float32(ctx.sw_binary(B)).view(np.uint32) == np.float32(rec[0]).view(np.uint32), (where, "score")
    return rec, cells


# ------------------------------------------------------------------------------------------------------------------
# a. the DP alone
# ------------------------------------------------------------------------------------------------------------------
def test_hand_checked_and_empty_plots(ctx):
    for name, B, want, cells in ref.hand_checked():
        rec, got = _check_dp(ctx, B, name, (want, cells))
        assert tuple(rec) == want
    for B in ref.no_match_plots():
        rec, got = _check_dp(ctx, B, "no match %s" % (B.shape,))
        assert tuple(rec) == ref.NO_MATCH and got.shape == (0, 2)


@pytest.mark.parametrize("seam", S.SEAMS)
def test_planted_paths_across_the_seams(ctx, seam):
    n = 0
    for name, B, planted in strips.planted_plots():
        if not name.startswith("seam%d_" % seam):
            continue
        rec, cells = _check_dp(ctx, B, name)
        if planted is not None:
            assert np.array_equal(cells, planted), name
        assert cells[0, 1] < seam <= cells[-1, 1], (name, "the path crosses the seam")
        n += 1
    assert n == 22


@pytest.mark.parametrize("n", S.RIM_N)
def test_rims(ctx, n):
    for m in S.RIM_M:
        for kind in S.RIM_PLOTS:
            _check_dp(ctx, S.rim_plot(kind, m, n), "rim %s %d x %d" % (kind, m, n))


def test_ties_across_strips_and_lanes(ctx):
    for name, B, end in strips.tie_plots():
        rec, cells = _check_dp(ctx, B, name)
        assert rec[3:5] == end and rec[0] == np.float32(9.3) and len(cells) == 10, (name, rec)
    assert _rec(ctx.sw_align_long_binary(strips.tie_plots()[0][1], paths=False)[0]) == (np.float32(9.3), 3, 1500, 12, 1509)


def test_predecessor_ties_read_from_the_seam_record(ctx):
    for name, B, want in strips.seam_pred_tie_plots():
        rec, cells = _check_dp(ctx, B, name)
        assert cells.tolist() == [list(c) for c in want], (name, cells.tolist())


def test_rows_beyond_1023(ctx):
    for name, B, end in strips.tall_plots():
        rec, cells = _check_dp(ctx, B, name)
        assert end is None or rec[3:5] == end, (name, rec)


def test_values_beyond_16_bits(ctx):
    (_, eye), (_, ones) = strips.big_value_plots()
    rec, cells = _check_dp(ctx, eye, "eye 3400")
    assert tuple(rec) == (np.float32(3397.0), 2, 2, 3398, 3398) and len(cells) == 3397
    _check_dp(ctx, ones, "ones 40 x 4100")


def test_stale_codes():
    """The plane of an all-ones plot under a sparse plot of the same shape: every word is written, zeros included."""
    from acoss_amd import _lib
    ones, sparse = strips.stale_pair()
    fresh, used = _lib.Context(0), _lib.Context(0)
    try:
        want = fresh.sw_align_long_binary(sparse)
        used.sw_align_long_binary(ones)
        got = used.sw_align_long_binary(sparse)
    finally:
        fresh.close()
        used.close()
    assert got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    wrec, wcells = ref.align_forward(sparse)
    assert _same(_rec(got[0][0]), wrec) and np.array_equal(got[1], wcells)


def test_refusals_leave_the_context_usable(ctx):
    B = ref.random_plot(np.random.default_rng(9), 40, 1030, 0.2)
    with pytest.raises(ValueError, match=r"cap 39 is too small: 40 cells required"):
        ctx.sw_align_long_binary(B, cap=39)
    ctx.sw_align_long_binary(B, cap=40)
    C = B.copy()
    C[7, 1027] = 2
    with pytest.raises(ValueError, match="non-binary"):
        ctx.sw_align_long_binary(C)
    _check_dp(ctx, B, "after the refusals")


def test_stand_alone_exports_share_the_decode_and_record_no_profile(ctx):
    """acx_sw_align_binary and acx_sw_align_long_binary are one driver function over the batch path's decode: the records and cells
    are the reference's with and without paths, and no profile entry counts a launch (the batch path's bookkeeping is not shared)."""
    small = np.zeros((6, 7), np.uint8)
    small[np.arange(6), np.arange(6)] = 1                     # counted rows 2..4: (2, 2), (3, 3), (4, 4), 10 tenths a cell
    wide = np.zeros((5, 1030), np.uint8)
    wide[np.arange(5), 1021 + np.arange(5)] = 1               # counted rows 2..3: (2, 1023), (3, 1024), across the two strips
    assert ref.align_forward(small)[0] == (np.float32(3.0), 2, 2, 4, 4) and ref.align_forward(small)[1].tolist() == [[2, 2], [3, 3], [4, 4]]
    assert ref.align_forward(wide)[1].tolist() == [[2, 1023], [3, 1024]]
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        for name, call, B in (("bits 6 x 7", ctx.sw_align_binary, small), ("long 6 x 7", ctx.sw_align_long_binary, small),
                              ("long 5 x 1030", ctx.sw_align_long_binary, wide)):
            wrec, wcells = ref.align_forward(B)
            al, cells = call(B)
            assert _same(_rec(al[0]), wrec) and np.array_equal(cells, wcells), (name, _rec(al[0]), wrec, cells.tolist(), wcells.tolist())
            assert cells.dtype == np.int32 and cells.shape == (len(wcells), 2), name
            alone = call(B, paths=False)
            assert alone.shape == (1,) and alone.tobytes() == al.tobytes(), (name, "record alone")
        prof = ctx.profile()
        assert len(prof) > 0 and all(v["launches"] == 0 for v in prof.values()), prof
    finally:
        ctx.profile_enable(False)


# ------------------------------------------------------------------------------------------------------------------
# b. the product path
# ------------------------------------------------------------------------------------------------------------------
BLOCKS = S.LONG_BLOCKS


@pytest.fixture(scope="module")
def pool(ctx):
    ctx.ef_upload_pool(S.long_pool())
    return ctx


@pytest.fixture(scope="module")
def probes(pool):
    pairs, index = S.long_probe_list()
    return pairs, index, pool.earlyfusion_pairs(pairs)


@pytest.fixture(scope="module")
def aligned(pool, probes):
    """ef_align_long of the probe list, per plane: computed once, shared, never changed."""
    return [pool.ef_align_long(probes[0], plane=plane, paths=True) for plane in range(4)]


def _device_plots(pool, pairs, k):
    """The four plots of pair k as sw_long_kernel::load_b reads them: the device's own matrices, thresholds and tie columns."""
    mats = pool.ef_debug_pairs(pairs, k)
    stats = pool.ef_debug_bits(pairs, k)
    assert stats["bits"] is None
    out = []
    for s in range(4):
        X = mats["csm"][s] if s < 3 else mats["fused"]
        t, jcut = stats["t"][s][:, None], stats["jcut"][s][:, None]
        out.append(((X < t) | ((X == t) & (np.arange(X.shape[1])[None, :] <= jcut))).astype(np.uint8))
    return out


@pytest.mark.parametrize("shape", S.LONG_PROBES, ids=lambda s: "%dx%d" % s)
def test_product_path_every_plane(pool, probes, aligned, shape):
    pairs, index, listed = probes
    k = index[shape]
    for plane, B in enumerate(_device_plots(pool, pairs, k)):
        assert B.shape == shape
        al, off, cells = aligned[plane]
        wrec, wcells = ref.align_forward(B)
        got = cells[off[k]:off[k + 1]]
        assert _same(_rec(al[k]), wrec) and np.array_equal(got, wcells), (shape, plane, _rec(al[k]), wrec)
        assert al["score"][k].view(np.uint32) == listed[k, plane].view(np.uint32), (shape, plane, "earlyfusion_pairs")
        ref.check_path(tuple(wrec), got, shape)


def test_records_alone_and_offsets(pool, probes, aligned):
    pairs = probes[0]
    for plane in (0, 3):
        al, off, cells = aligned[plane]
        assert pool.ef_align_long(pairs, plane=plane).tobytes() == al.tobytes(), "the records are the same bytes with and without the paths"
        assert off[0] == 0 and off[-1] == len(cells) and np.all(np.diff(off) >= 0)


def test_planted_section_crosses_block_1024(pool, probes, aligned):
    """Blocks 930 .. 980 of the track of 1025 blocks are blocks 1000 .. 1050 of the track of 1100: the early alignment of the pair
    (1025, 1100) crosses COLUMN 1024 -- the seam of its two strips --, that of (1100, 1025) crosses ROW 1024."""
    pairs, index, listed = probes
    al, off, cells = aligned[3]
    for shape, axis in zip(S.LONG_PROBES[:2], (1, 0)):
        k = index[shape]
        p = cells[off[k]:off[k + 1]]
        print("pair %d x %d: early score %.1f, rows %d..%d, columns %d..%d, %d cells"
              % (shape + (al["score"][k], p[0, 0], p[-1, 0], p[0, 1], p[-1, 1], len(p))))
        assert p[0, axis] < 1024 <= p[-1, axis], (shape, axis, p[0].tolist(), p[-1].tolist())


def test_list_order_does_not_matter(pool, probes, aligned):
    pairs = probes[0]
    al, off, cells = aligned[3]
    order = np.random.default_rng(3).permutation(len(pairs))
    mixed = np.ascontiguousarray(pairs[order])
    for lst, idx in ((mixed, order), (np.ascontiguousarray(mixed[::-1]), order[::-1])):
        gal, goff, gcells = pool.ef_align_long(lst, plane=3, paths=True)
        for k, src in enumerate(idx):
            assert gal[k].tobytes() == al[src].tobytes() and np.array_equal(gcells[goff[k]:goff[k + 1]], cells[off[src]:off[src + 1]]), (k, src)


SMALL_LIST = np.array(sorted((BLOCKS.index(m), BLOCKS.index(n)) for m, n in ((17, 1100), (1100, 17), (3, 1025), (1025, 3), (512, 1025), (1025, 512))), np.int32)


def test_batches_and_chunks(pool, monkeypatch):
    """Two batches under a small scratch limit; more chunks than batches when a chunk holds fewer waves."""
    want = pool.ef_align_long(SMALL_LIST, plane=3, paths=True)
    need = sum(16 * BLOCKS[i] * ((BLOCKS[j] + 63) // 64 * 64) for i, j in SMALL_LIST)
    pool.profile_enable(True)
    try:
        pool.set_scratch_limit(int(0.6 * need))
        pool.profile_reset()
        got = pool.ef_align_long(SMALL_LIST, plane=3, paths=True)
        prof = pool.profile()
        batches, chunks = prof["ef_gemm_kernel"]["launches"], prof["ef_align_long_kernel"]["launches"]
        assert batches == 2 and chunks == 2 and prof["ef_align_kernel"]["launches"] == 0, (batches, chunks)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        monkeypatch.setenv("ACX_EF_ALIGN_WAVES", "3")
        pool.profile_reset()
        got = pool.ef_align_long(SMALL_LIST, plane=3, paths=True)
        prof = pool.profile()
        batches, chunks = prof["ef_gemm_kernel"]["launches"], prof["ef_align_long_kernel"]["launches"]
        assert batches == 2 and chunks > batches and chunks >= (len(SMALL_LIST) + 2) // 3, (batches, chunks)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        monkeypatch.delenv("ACX_EF_ALIGN_WAVES")
    finally:
        pool.set_scratch_limit(0)
        pool.profile_enable(False)


def test_refused_lists_launch_nothing(pool, probes, aligned):
    from acoss_amd import _lib
    pairs = probes[0]
    pool.profile_enable(True)
    try:
        pool.profile_reset()
        for plane in (-1, 4):
            with pytest.raises(ValueError, match=r"plane must be 0\.\.3"):
                pool.ef_align_long(pairs, plane=plane)
        with pytest.raises(ValueError, match="track index out of range in pair 2"):
            pool.ef_align_long(np.array([(6, 5), (0, 1), (0, 7)], np.int32), plane=3)
        bound = int(sum(min(BLOCKS[i], BLOCKS[j]) for i, j in pairs))
        with pytest.raises(ValueError, match=r"cap %d is too small: %d cells required" % (bound - 1, bound)):
            pool.ef_align_long(pairs, plane=3, paths=True, cap=bound - 1)
        out = np.zeros(len(pairs), _lib.ALIGNMENT_DTYPE)
        off = np.zeros(len(pairs) + 1, np.int64)
        p = _lib.EfParams(0.1, 10)
        ip = pairs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        assert pool._L.acx_ef_align_long(pool._h, ip, len(pairs), ctypes.byref(p), 3, out.ctypes.data, off.ctypes.data, None, 1 << 20) == -1
        assert pool._L.acx_ef_align_long(pool._h, ip, len(pairs), ctypes.byref(p), 3, out.ctypes.data, None, off.ctypes.data, 1 << 20) == -1
        # none of these refusals launched anything: no call has run since the reset
        assert all(v["launches"] == 0 for v in pool.profile().values()), pool.profile()
        # acx_ef_align keeps its refusal of the same list, word for word
        with pytest.raises(NotImplementedError, match="alignment needs the bit path: at most 1024 blocks"):
            pool.ef_align(pairs, plane=3)
        assert all(v["launches"] == 0 for v in pool.profile().values()), pool.profile()
        # a valid call after the refusals succeeds
        assert pool.ef_align_long(pairs, plane=3).tobytes() == aligned[3][0].tobytes()
    finally:
        pool.profile_enable(False)


def test_profile_entry(pool, probes):
    pairs = probes[0]
    pool.profile_enable(True)
    try:
        pool.profile_reset()
        pool.earlyfusion_pairs(pairs)
        before = pool.profile()
        assert before["ef_align_long_kernel"] == dict(ms=0.0, launches=0, cells=0)
        pool.profile_reset()
        pool.ef_align_long(pairs, plane=3)
        after = pool.profile()
        assert after["ef_align_long_kernel"]["launches"] == 1 and after["ef_align_long_kernel"]["ms"] > 0
        assert after["ef_align_long_kernel"]["cells"] == sum(BLOCKS[i] * BLOCKS[j] for i, j in pairs)
        # the option adds its own launch and nothing else: every other entry counts what the call without it counts
        for name in before:
            if name != "ef_align_long_kernel":
                assert after[name]["launches"] == before[name]["launches"] and after[name]["cells"] == before[name]["cells"], name
        print("ef_align_long_kernel %.3f ms (one plane) beside sw_kernel %.3f ms (sw_long_kernel, four planes) on the same %d pairs"
              % (after["ef_align_long_kernel"]["ms"], after["sw_kernel"]["ms"], len(pairs)))
    finally:
        pool.profile_enable(False)


@pytest.fixture(scope="module")
def mixed():
    from acoss_amd import _lib
    from .test_gpu_ef_backend import _pool
    c = _lib.Context(0)
    c.ef_upload_pool(_pool(S.MIXED_BLOCKS))
    yield c
    c.close()


@pytest.mark.parametrize("plane", range(4), ids=PLANES)
def test_short_pairs_beside_a_long_pair(mixed, plane):
    """The short pairs of a list that holds a long pair -- aligned by ef_align_long_kernel off the float matrices -- get bit for bit
    what ef_align_kernel gives them off the bitmaps in a list of their own."""
    probes, lists = S.mixed_lists()
    alone = lists["alone"][0]
    want = mixed.ef_align(alone, plane=plane, paths=True)
    mixed.profile_enable(True)
    try:
        # no long track: the code path of acx_ef_align, launches included
        mixed.profile_reset()
        got = mixed.ef_align_long(alone, plane=plane, paths=True)
        prof = mixed.profile()
        assert prof["ef_align_kernel"]["launches"] == 1 and prof["ef_align_long_kernel"]["launches"] == 0
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        for name in ("long_rows", "long_cols"):
            pairs, where = lists[name]
            mixed.profile_reset()
            al, off, cells = mixed.ef_align_long(pairs, plane=plane, paths=True)
            prof = mixed.profile()
            assert prof["ef_align_kernel"]["launches"] == 0 and prof["ef_align_long_kernel"]["launches"] == 1, name
            for k, src in enumerate(where):
                assert al[src].tobytes() == want[0][k].tobytes(), (name, probes[k], _rec(al[src]), _rec(want[0][k]))
                assert np.array_equal(cells[off[src]:off[src + 1]], want[2][want[1][k]:want[1][k + 1]]), (name, probes[k])
    finally:
        mixed.profile_enable(False)


# ------------------------------------------------------------------------------------------------------------------
# c. Python
# ------------------------------------------------------------------------------------------------------------------
def _dataset(tmp_path, n, name="ds.csv"):
    path = tmp_path / name
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


def _algo(tmp_path, tracks, shortname):
    from acoss_amd.algorithms import EarlyFusion
    a = EarlyFusion(_dataset(tmp_path, len(tracks), shortname + ".csv"), "feat/", shortname=shortname)
    a.set_block_features(tracks, ["w%d" % (i // 2) for i in range(len(tracks))])
    return a


@pytest.fixture()
def algo(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    a = _algo(tmp_path, S.long_pool(), "efalignlong_gpu")
    yield a
    a.cleanup_memmap()


LONGEST = BLOCKS.index(1100)


def test_python_align_and_paths(algo):
    idxs = np.array([(LONGEST, 5), (5, LONGEST), (1, LONGEST), (LONGEST, 0), (3, LONGEST)])
    for stype in ("early", "chromas"):
        plane = PLANES.index(stype)
        al = algo.align(idxs, similarity_type=stype)
        al2, paths = algo.align_paths(idxs, similarity_type=stype)
        assert al.dtype == algo.ALIGN_DTYPE and al.tobytes() == al2.tobytes() and len(paths) == len(idxs)
        want, off, cells = algo._context().ef_align_long(idxs.astype(np.int32), algo.kappa, algo.K, plane, paths=True)
        for f in want.dtype.names:
            assert np.array_equal(al[f], want[f]), f
        for k, p in enumerate(paths):
            assert np.array_equal(p, cells[off[k]:off[k + 1]])
            if al["score"][k] > 0:
                assert al["q_span"][k].tolist() == [al["q0"][k], al["q1"][k] + algo.blocksize - 1]
                assert al["r_span"][k].tolist() == [al["r0"][k], al["r1"][k] + algo.blocksize - 1]
            else:
                assert len(p) == 0 and al["q_span"][k].tolist() == [-1, -1] and al["q0"][k] == -1
    assert al["score"][0] > 0 and al["score"][1] > 0


def test_python_align_match_paths_on_identify(algo):
    queries = [LONGEST, 5, 1]
    idx, score = algo.identify(queries, k=3)["early"]
    idx = idx.copy()
    idx[1, 2] = -1                                         # an empty slot
    al = algo.align_matches(queries, idx, similarity_type="early")
    al2, paths = algo.align_match_paths(queries, idx, similarity_type="early")
    assert al.shape == idx.shape and al.tobytes() == al2.tobytes()
    assert al["q0"][1, 2] == -1 and al["score"][1, 2] == 0 and paths[1][2].shape == (0, 2)
    for i, q in enumerate(queries):
        for s in range(idx.shape[1]):
            if idx[i, s] < 0:
                continue
            one, p1 = algo.align_paths([(q, idx[i, s])])
            assert one[0].tobytes() == al[i, s].tobytes() and np.array_equal(p1[0], paths[i][s])
            lo, hi = min(q, idx[i, s]), max(q, idx[i, s])
            assert algo.align([(lo, hi)])["score"][0].view(np.uint32) == score[i, s].view(np.uint32)


def test_locate_a_long_track_outside_the_collection(tmp_path, monkeypatch):
    """The track of 1100 blocks as a track the collection does not hold: what the object built over all tracks returns."""
    monkeypatch.chdir(tmp_path)
    tracks = S.long_pool()
    A, B = _algo(tmp_path, tracks[:LONGEST], "efalignlong_a"), _algo(tmp_path, tracks, "efalignlong_b")
    try:
        idx, score, al, paths = A.locate_tracks([tracks[LONGEST]], k=3, paths=True)
        widx, wscore = B.identify([LONGEST], k=3, candidates=list(range(LONGEST)))["early"]
        assert np.array_equal(idx, widx) and np.array_equal(score.view(np.uint32), wscore.view(np.uint32))
        pairs = np.stack([idx[0], np.full(3, LONGEST)], axis=1)
        wal, wpaths = B.align_paths(pairs)
        assert al[0].tobytes() == wal.tobytes() and all(np.array_equal(a, b) for a, b in zip(paths[0], wpaths))
        assert np.array_equal(al["score"][0].view(np.uint32), score[0].view(np.uint32))
        idx2, score2, al2 = A.locate_tracks([tracks[LONGEST]], k=3)
        assert np.array_equal(idx2, idx) and al2.tobytes() == al.tobytes()
        assert A._n_tracks() == LONGEST
    finally:
        A.cleanup_memmap()
        B.cleanup_memmap()


def test_short_collections_keep_their_kernel(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    a = _algo(tmp_path, S.long_pool()[:5], "efalignlong_short")            # 3 .. 1024 blocks
    try:
        c = a._context()
        c.profile_enable(True)
        c.profile_reset()
        a.align_paths([(4, 3), (3, 4), (2, 4)])
        prof = c.profile()
        c.profile_enable(False)
        assert prof["ef_align_kernel"]["launches"] == 1 and prof["ef_align_long_kernel"]["launches"] == 0
    finally:
        a.cleanup_memmap()
