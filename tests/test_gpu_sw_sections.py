"""
EVERY matched section of an EarlyFusion pair on the device: ef_sections_kernel through acx_sw_sections_binary
(the DP alone on a given plot), acx_ef_align_sections (the product chain), EarlyFusion.align_sections and align_match_sections.
Every comparison is exact against statement (a) of tests/_sw_sections_ref.py (held against statement (b) by
tests/test_sw_sections_ref.py): records, counts, offsets, every cell.
"""
import ctypes

import numpy as np
import pytest

from . import _ef_backend_ref as backend
from . import _sw_sections_ref as ref

pytestmark = pytest.mark.gpu

FIELDS = ("score", "q0", "r0", "q1", "r1")
NO_MATCH = (0.0, -1, -1, -1, -1)


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _rec(a):
    return (float(a["score"]),) + tuple(int(a[f]) for f in FIELDS[1:])


def _opts(**kw):
    from acoss_amd import _lib
    return _lib.section_opts("test", **kw)


def _compare(label, S_, got, n, off, cells, want, wpaths):
    """One pair's device result -- S_ records, their number, S_ + 1 offsets and the cells -- against (a)."""
    recs = [_rec(got[s]) for s in range(S_)]
    assert n == len(want), "%s: %d sections %s, reference %d %s" % (label, n, recs[:n], len(want), want)
    assert recs[:n] == want, "%s: device %s, reference %s" % (label, recs[:n], want)
    assert all(r == NO_MATCH for r in recs[n:]), "%s: the no-match record behind the count: %s" % (label, recs[n:])
    if off is None:
        return
    for s in range(S_):
        mine = cells[off[s]:off[s + 1]]
        if s >= n:
            assert len(mine) == 0, label
        elif not np.array_equal(mine, wpaths[s]):
            raise AssertionError("%s: section %d has %d cells %s ..., reference %d %s ..." % (
                label, s, len(mine), mine[:3].tolist(), len(wpaths[s]), wpaths[s][:3].tolist()))


def _check_dp(ctx, B, tag, **okw):
    """sw_sections_binary on B against sections_full; section 0 against sw_align_binary's bytes.  Returns the reference."""
    from acoss_amd import _lib
    o = _opts(**okw)
    got, n, off, cells = ctx.sw_sections_binary(B, o)
    S_ = o.max_sections
    assert got.shape == (S_,) and got.dtype == _lib.ALIGNMENT_DTYPE and off.shape == (S_ + 1,) and off[0] == 0
    assert cells.dtype == np.int32 and cells.shape == (off[-1], 2)
    want, wpaths = ref.sections_full(B, **okw)
    label = "%s, %s plot, %s" % (tag, B.shape, okw)
    _compare(label, S_, got, n, off, cells, want, wpaths)
    first, fcells = ctx.sw_align_binary(B)
    if first[0]["score"] >= o.min_score:
        assert n >= 1 and got[:1].tobytes() == first.tobytes() and np.array_equal(cells[:off[1]], fcells), label
    else:
        assert n == 0, label
    bare, nb = ctx.sw_sections_binary(B, o, paths=False)
    assert nb == n and bare.tobytes() == got.tobytes(), label
    return want, wpaths


def plant(B, i, j, steps, n):
    """Ones along a path of n cells from (i, j), `steps` taken in turn (cyclically).  Returns the cells."""
    cells = []
    for t in range(n):
        B[i, j] = 1
        cells.append((i, j))
        i, j = i + steps[t % len(steps)][0], j + steps[t % len(steps)][1]
    return cells


MIXED = ((1, 1), (1, 2), (2, 1), (1, 2))


# ---- the DP alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.HAND, ids=[h[0] for h in ref.HAND])
def test_hand_checked_plots(ctx, case):
    name, B, okw, want = case
    got, _ = _check_dp(ctx, B, name, **okw)
    assert got == ref.hand_records(want), name


@pytest.mark.parametrize("N", [4, 5, 17, 33, 64, 65, 1023, 1024])
def test_random_plots(ctx, N):
    """N x M of the issue's grid at three densities; max_sections and pad step with the plot, so that every N meets max_sections 1, 2
    and 16 and pad 0, 1 and 5.  Where the plot has the room, four short diagonals at random places join the noise: sections behind
    the first to find on the wide plots as well."""
    rng = np.random.default_rng([29, N])
    total = 0
    for mi, M in enumerate((4, 5, 9, 64, 130)):
        for di, dens in enumerate((0.05, 0.3, 0.6)):
            B = (rng.random((M, N)) < dens).astype(np.uint8)
            if M >= 64 and N >= 17:
                for _ in range(4):
                    n = int(rng.integers(4, 13))
                    plant(B, int(rng.integers(2, M - 1 - n)), int(rng.integers(2, N - 1 - n)), ((1, 1),), n)
            want, _ = _check_dp(ctx, B, "random plot, density %s" % dens, max_sections=(1, 2, 16)[(mi + di) % 3], pad=(0, 1, 5)[(mi + 2 * di) % 3],
                                min_score=(1.1, 2.0)[(mi + di) % 2])
            total += len(want)
    print("N = %d: %d sections in 15 calls" % (N, total))


def test_intervals_begin_and_end_on_every_row_phase(ctx):
    """Section 0 planted at rows q0 .. q1 with q0 & 7 and q1 & 7 taking every value (both parities of either): the interval above ends
    at q0 - pad - 1, the one below begins at q1 + pad + 1 -- with pad 0 the sections ABUT --, and each holds a shorter planted section
    that crosses the lane edge between columns 15 and 16."""
    t = 0
    for q0m in range(8):
        for q1m in range(8):
            q0 = 24 + q0m
            L = 24 + (q1m - (q0 + 23)) % 8          # rows q0 .. q0 + L - 1, (q0 + L - 1) & 7 == q1m
            q1 = q0 + L - 1
            assert q1 & 7 == q1m and 24 <= L < 32
            pad = t % 3
            B = np.zeros((q1 + 40, 200), np.uint8)
            plant(B, q0, 100, ((1, 1),), L)
            above = plant(B, 3, 8, MIXED, 12)       # rows 3 .. : ends above q0 - pad
            below = plant(B, q1 + pad + 1, 6, MIXED, 14)
            assert above[-1][0] < q0 - pad and below[-1][0] <= B.shape[0] - 2
            for path in (above, below):
                assert min(c[1] for c in path) <= 15 and max(c[1] for c in path) >= 16
            want, _ = _check_dp(ctx, B, "phases (%d, %d)" % (q0m, q1m), max_sections=4, pad=pad, min_score=3.0)
            assert len(want) == 3 and want[0][1] == q0 and want[0][3] == q1
            assert {(w[1], w[3]) for w in want[1:]} == {(above[0][0], above[-1][0]), (below[0][0], below[-1][0])}
            t += 1


def test_intervals_from_row_2_and_to_the_last_counted_row(ctx):
    """The interval above section 0 begins at DP row 2 and holds a section that starts there; the one below runs to row M - 2 and holds
    a section that ends there.  Then the same with the short sections swapped in as section 0's neighbours at a lane edge."""
    for M, N in ((70, 90), (71, 1024)):
        B = np.zeros((M, N), np.uint8)
        plant(B, 20, N - 40, ((1, 1),), 30)             # section 0: rows 20 .. 49
        top = plant(B, 2, 10, ((1, 1),), 12)            # rows 2 .. 13, columns 10 .. 21
        bottom = plant(B, M - 2 - 11, 4, ((1, 1),), 12)  # ends at (M - 2, 15); the next column is the lane edge
        want, _ = _check_dp(ctx, B, "row 2 and row M - 2", max_sections=4, pad=1, min_score=3.0)
        assert len(want) == 3 and {(w[1], w[3]) for w in want[1:]} == {(2, 13), (M - 13, M - 2)}
        assert bottom[-1] == (M - 2, 15) and top[0] == (2, 10)


def test_sixteen_sections_and_a_seventeenth_candidate(ctx):
    """17 diagonals in row bands of their own, each left of the ones above it: max_sections = 16 reports 16 and leaves one."""
    B = np.zeros((4 + 12 * 17 + 4, 2 + 12 * 17 + 12), np.uint8)
    lengths = [5 + (7 * k) % 6 for k in range(17)]
    for k, n in enumerate(lengths):
        plant(B, 4 + 12 * k, 2 + 12 * (16 - k), ((1, 1),), n)
    want, _ = _check_dp(ctx, B, "17 diagonals", max_sections=16, min_score=2.0)
    assert len(want) == 16
    assert sorted(w[3] - w[1] + 1 for w in want) == sorted(lengths)[1:], "the shortest diagonal (one of them) is the one left over"
    assert [w[0] for w in want] == sorted((w[0] for w in want), reverse=True)
    want, _ = _check_dp(ctx, B, "17 diagonals, pad 3", max_sections=16, min_score=2.0, pad=3)
    assert len(want) == 16


def _launches_nothing(ctx, exc, match, call):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        with pytest.raises(exc, match=match):
            call()
        prof = ctx.profile()
    finally:
        ctx.profile_enable(False)
    assert sum(v["launches"] for v in prof.values()) == 0, {k: v["launches"] for k, v in prof.items() if v["launches"]}


def _raw_opts(max_sections=4, pad=0, min_score=2.0, min_ratio=0.0):
    from acoss_amd import _lib
    return _lib.SectionOpts(max_sections, pad, min_score, min_ratio)


BAD_OPTS = [(dict(max_sections=0), "max_sections"), (dict(max_sections=17), "max_sections"), (dict(pad=-1), "pad"),
            (dict(min_score=1.0), "min_score"), (dict(min_score=float("nan")), "min_score"), (dict(min_ratio=-0.5), "min_ratio"),
            (dict(min_ratio=1.25), "min_ratio"), (dict(min_ratio=float("nan")), "min_ratio")]


def test_empty_plot_capacity_and_refused_options(ctx):
    assert _check_dp(ctx, np.zeros((7, 9), np.uint8), "all zero", max_sections=3)[0] == []
    for shape in ((3, 9), (9, 3), (1, 1), (3, 3), (4, 4)):
        assert _check_dp(ctx, np.ones(shape, np.uint8), "too small", min_score=1.1)[0] == []
    _launches_nothing(ctx, NotImplementedError, "sw_sections_binary: alignment needs the bit path: at most 1024 blocks",
                      lambda: ctx.sw_sections_binary(np.zeros((1025, 8), np.uint8)))
    _launches_nothing(ctx, NotImplementedError, "at most 1024 blocks", lambda: ctx.sw_sections_binary(np.zeros((8, 1025), np.uint8), paths=False))
    B = ref.THREE                                    # 60 x 120: min(M, 4 * min(M, N)) = 60, min(M, 1 * 60) = 60
    _launches_nothing(ctx, ValueError, "cap 59 is too small: 60 cells required", lambda: ctx.sw_sections_binary(B, cap=59))
    got = ctx.sw_sections_binary(B, cap=60)
    assert got[1] == 3 and got[2].tolist() == [0, 12, 21, 27, 27]
    T = np.ascontiguousarray(B.T)                    # 120 x 60: min(120, 1 * 60) = 60, min(120, 4 * 60) = 120
    _launches_nothing(ctx, ValueError, "cap 119 is too small: 120 cells required", lambda: ctx.sw_sections_binary(T, cap=119))
    _launches_nothing(ctx, ValueError, "cap 59 is too small: 60 cells required", lambda: ctx.sw_sections_binary(T, opts=_opts(max_sections=1), cap=59))
    for bad, what in BAD_OPTS:
        _launches_nothing(ctx, ValueError, "sw_sections_binary: %s" % what, lambda: ctx.sw_sections_binary(B, opts=_raw_opts(**bad)))
    bad = B.copy()
    bad[3, 3] = 2
    _launches_nothing(ctx, ValueError, "non-binary", lambda: ctx.sw_sections_binary(bad))
    # exactly one of path_off / cells: refused
    o = _raw_opts()
    out = np.zeros(4, np.dtype([(f, np.float32 if f == "score" else np.int32) for f in FIELDS]))
    n = np.zeros(1, np.int32)
    off = np.zeros(5, np.int64)
    bp = B.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert ctx._L.acx_sw_sections_binary(ctx._h, bp, 60, 120, ctypes.byref(o), out.ctypes.data, n.ctypes.data, off.ctypes.data, None, 1 << 20) == -1
    assert ctx._L.acx_sw_sections_binary(ctx._h, bp, 60, 120, ctypes.byref(o), out.ctypes.data, n.ctypes.data, None, off.ctypes.data, 1 << 20) == -1
    assert ctx.sw_sections_binary(B)[1] == 3


# ---- the product path -----------------------------------------------------------------------------------------------------------------------
DIMS = (40, 100, 96)                       # small feature widths: the GEMMs cost nothing
BLOCKS = [4, 63, 64, 65, 512, 1024, 1025]
# sorted by (first, second), as ef_debug_bits wants its list
PAIRS = np.array([(0, 1), (1, 2), (2, 3), (3, 1), (3, 4), (4, 5), (5, 3), (5, 4)], np.int32)
PLANES = ("mfccs", "ssms", "chromas", "early")
OKW = dict(max_sections=3, min_score=2.0, pad=1)


def _track(nb, seed):
    rng = np.random.default_rng(seed)
    return dict(mfccs=rng.standard_normal((nb, DIMS[0])).astype(np.float32), ssms=(2 * rng.random((nb, DIMS[1]))).astype(np.float32),
                chromas=(rng.random((nb, DIMS[2])).astype(np.float32) ** 3 + 1e-3), chroma_med=rng.random(12) ** 2)


def _copy(tracks, rng, a, b, at_a, at_b, m):
    """Blocks at_a .. at_a + m - 1 of track a, with a little noise, as blocks at_b .. of track b."""
    for key in ("mfccs", "ssms", "chromas"):
        tracks[b][key][at_b:at_b + m] = tracks[a][key][at_a:at_a + m] + 0.02 * rng.standard_normal((m, tracks[a][key].shape[1])).astype(np.float32)


def _tracks():
    tracks = [_track(nb, 29000 + k) for k, nb in enumerate(BLOCKS)]
    rng = np.random.default_rng(29999)
    # two excerpts each, in swapped order: more than one section to find (a track is written before it is copied from)
    for a, b, at_a, at_b, m in ((2, 3, 5, 40, 20), (2, 3, 35, 8, 22), (3, 4, 2, 300, 25), (3, 4, 33, 100, 28), (4, 5, 100, 600, 60), (4, 5, 300, 200, 50)):
        _copy(tracks, rng, a, b, at_a, at_b, m)
    return tracks


@pytest.fixture(scope="module")
def pool(ctx):
    ctx.ef_upload_pool(_tracks())
    return ctx


@pytest.fixture(scope="module")
def expected(pool):
    """Per pair of PAIRS: the four plots as the selection kernels left them (ef_debug_bits) and their sections by statement (a) under
    OKW.  Computed once, shared, never changed."""
    out = []
    for k in range(len(PAIRS)):
        db = pool.ef_debug_bits(PAIRS, k)
        N = BLOCKS[PAIRS[k, 1]]
        plots = []
        for s in range(4):
            B, pads = backend.unpack_bits(db["bits"][s], N)
            assert pads == 0 and B.shape == (BLOCKS[PAIRS[k, 0]], N)
            plots.append(B)
        out.append(dict(plots=plots, answers=[ref.sections_full(B, **OKW) for B in plots]))
    return out


def _against(label, S_, got, n, off, cells, k, answer):
    _compare(label, S_, got[k], int(n[k]), off[k * S_:(k + 1) * S_ + 1], cells, answer[0], answer[1])


@pytest.mark.parametrize("plane", range(4), ids=PLANES)
def test_product_path_every_plane(pool, expected, plane):
    o = _opts(**OKW)
    S_ = o.max_sections
    got, n, off, cells = pool.ef_align_sections(PAIRS, plane=plane, opts=o, paths=True)
    assert got.shape == (len(PAIRS), S_) and n.shape == (len(PAIRS),) and off.shape == (len(PAIRS) * S_ + 1,) and off[0] == 0
    assert cells.shape == (off[-1], 2) and np.all(np.diff(off) >= 0)
    bare, nb = pool.ef_align_sections(PAIRS, plane=plane, opts=o)
    assert bare.tobytes() == got.tobytes() and np.array_equal(nb, n), "the records are the same bytes with and without the paths"
    al, aoff, acells = pool.ef_align(PAIRS, plane=plane, paths=True)
    one, n1 = pool.ef_align_sections(PAIRS, plane=plane, opts=_opts(max_sections=1, min_score=OKW["min_score"]))
    for k in range(len(PAIRS)):
        label = "pair %s plane %s" % (PAIRS[k].tolist(), PLANES[plane])
        _against(label, S_, got, n, off, cells, k, expected[k]["answers"][plane])
        if al[k]["score"] >= o.min_score:
            assert n[k] >= 1 and got[k, :1].tobytes() == al[k:k + 1].tobytes() == one[k].tobytes() and n1[k] == 1, label
            assert np.array_equal(cells[off[k * S_]:off[k * S_ + 1]], acells[aoff[k]:aoff[k + 1]]), label
        else:
            assert n[k] == 0 and n1[k] == 0 and _rec(one[k, 0]) == NO_MATCH, label
    print("plane %s: sections per pair %s" % (PLANES[plane], n.tolist()))
    assert n.max() >= 2


def test_list_order_does_not_matter(pool, expected):
    o = _opts(**OKW)
    order = np.random.default_rng(3).permutation(len(PAIRS))
    mixed = np.ascontiguousarray(PAIRS[order])
    for lst, idx in ((mixed, order), (np.ascontiguousarray(mixed[::-1]), order[::-1])):
        got, n, off, cells = pool.ef_align_sections(lst, plane=3, opts=o, paths=True)
        for k, src in enumerate(idx):
            _against("mixed list position %d" % k, 3, got, n, off, cells, k, expected[src]["answers"][3])


def _profiled(ctx, call):
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        out = call()
        prof = ctx.profile()
    finally:
        ctx.profile_enable(False)
    return out, prof


# sorted by (first, second)
SHORT_PAIRS = np.array([(0, 1), (1, 0), (1, 2), (1, 3), (2, 1), (2, 3), (3, 1), (3, 2)], np.int32)


def test_batches_and_chunks(pool, monkeypatch):
    """Two batches under a small scratch limit: one launch per chunk, a batch being one chunk; more chunks than batches when a chunk
    holds fewer waves."""
    o = _opts(**OKW)
    call = lambda: pool.ef_align_sections(SHORT_PAIRS, plane=3, opts=o, paths=True)
    want, prof = _profiled(pool, call)
    assert prof["sw_kernel"]["launches"] == 1 and prof["ef_sections_kernel"]["launches"] == 1 and prof["ef_align_kernel"]["launches"] == 0
    for k in range(len(SHORT_PAIRS)):
        B, _ = backend.unpack_bits(pool.ef_debug_bits(SHORT_PAIRS, k)["bits"][3], BLOCKS[SHORT_PAIRS[k, 1]])
        _against("short pair %d" % k, 3, want[0], want[1], want[2], want[3], k, ref.sections_full(B, **OKW))
    need = sum(12 * BLOCKS[i] * ((BLOCKS[j] + 63) // 64 * 64) for i, j in SHORT_PAIRS)
    try:
        pool.set_scratch_limit(int(0.6 * need))
        got, prof = _profiled(pool, call)
        assert prof["sw_kernel"]["launches"] == 2 and prof["ef_sections_kernel"]["launches"] == 2, prof
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        monkeypatch.setenv("ACX_EF_ALIGN_WAVES", "3")
        got, prof = _profiled(pool, call)
        batches, chunks = prof["sw_kernel"]["launches"], prof["ef_sections_kernel"]["launches"]
        assert batches == 2 and chunks > batches and chunks >= (len(SHORT_PAIRS) + 2) // 3, (batches, chunks)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        monkeypatch.delenv("ACX_EF_ALIGN_WAVES")
    finally:
        pool.set_scratch_limit(0)


def test_refused_lists_launch_nothing(pool, expected):
    from acoss_amd import _lib
    o = _opts(**OKW)
    bad = np.ascontiguousarray(np.concatenate([PAIRS[:3], [[2, 6]], PAIRS[3:]]).astype(np.int32))      # track 6: 1025 blocks
    _launches_nothing(pool, NotImplementedError, "ef_align_sections: alignment needs the bit path: at most 1024 blocks",
                      lambda: pool.ef_align_sections(bad, plane=3, opts=o))
    _launches_nothing(pool, NotImplementedError, "at most 1024 blocks", lambda: pool.ef_align_sections(bad[::-1].copy(), plane=3, opts=o, paths=True))
    for plane in (-1, 4):
        _launches_nothing(pool, ValueError, r"ef_align_sections: plane must be 0\.\.3", lambda: pool.ef_align_sections(PAIRS, plane=plane, opts=o))
    _launches_nothing(pool, ValueError, "track index out of range in pair 2",
                      lambda: pool.ef_align_sections(np.array([(5, 4), (0, 1), (0, 7)], np.int32), plane=3, opts=o))
    for wrong, what in BAD_OPTS:
        _launches_nothing(pool, ValueError, "ef_align_sections: %s" % what, lambda: pool.ef_align_sections(PAIRS, plane=3, opts=_raw_opts(**wrong)))
    bound = int(sum(min(BLOCKS[i], 3 * min(BLOCKS[i], BLOCKS[j])) for i, j in PAIRS))
    _launches_nothing(pool, ValueError, r"cap %d is too small: %d cells required" % (bound - 1, bound),
                      lambda: pool.ef_align_sections(PAIRS, plane=3, opts=o, paths=True, cap=bound - 1))
    # exactly one of path_off / cells: refused
    out = np.zeros((len(PAIRS), 3), _lib.ALIGNMENT_DTYPE)
    n = np.zeros(len(PAIRS), np.int32)
    off = np.zeros(3 * len(PAIRS) + 1, np.int64)
    p = _lib.EfParams(0.1, 10)
    ip = PAIRS.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    fn = pool._L.acx_ef_align_sections
    assert fn(pool._h, ip, len(PAIRS), ctypes.byref(p), 3, ctypes.byref(o), out.ctypes.data, n.ctypes.data, off.ctypes.data, None, 1 << 20) == -1
    assert fn(pool._h, ip, len(PAIRS), ctypes.byref(p), 3, ctypes.byref(o), out.ctypes.data, n.ctypes.data, None, off.ctypes.data, 1 << 20) == -1
    # a valid call after the refusals succeeds, with cap at the bound
    got, n, off, cells = pool.ef_align_sections(PAIRS, plane=3, opts=o, paths=True, cap=bound)
    for k in range(len(PAIRS)):
        _against("after the refusals, pair %d" % k, 3, got, n, off, cells, k, expected[k]["answers"][3])


def test_profile_entry(pool):
    """ef_sections_kernel stands in ef_align_kernel's place, in front of ef_align_long_kernel in the list; every other entry counts what
    the call without the option counts."""
    _, before = _profiled(pool, lambda: pool.ef_align(PAIRS, plane=2))
    _, after = _profiled(pool, lambda: pool.ef_align_sections(PAIRS, plane=2, opts=_opts(**OKW)))
    names = list(after)
    assert names[-1] == "ef_align_kernel" and names[-2] == "ef_align_long_kernel" and names[-3] == "ef_sections_kernel"
    assert before["ef_sections_kernel"] == dict(ms=0.0, launches=0, cells=0) and before["ef_align_kernel"]["launches"] == 1
    assert after["ef_align_kernel"]["launches"] == 0
    assert after["ef_sections_kernel"]["launches"] == 1 and after["ef_sections_kernel"]["ms"] > 0
    assert after["ef_sections_kernel"]["cells"] == before["ef_align_kernel"]["cells"] == sum(BLOCKS[i] * BLOCKS[j] for i, j in PAIRS)
    for name in before:
        if name not in ("ef_align_kernel", "ef_sections_kernel"):
            assert after[name]["launches"] == before[name]["launches"] and after[name]["cells"] == before[name]["cells"], name
    print("ef_sections_kernel %.3f ms (max_sections 3) beside ef_align_kernel %.3f ms on the same %d pairs" % (
        after["ef_sections_kernel"]["ms"], before["ef_align_kernel"]["ms"], len(PAIRS)))


# ---- EarlyFusion.align_sections / align_match_sections --------------------------------------------------------------------------------------
def _dataset(tmp_path, tag, n):
    path = tmp_path / ("%s.csv" % tag)
    with open(path, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return str(path)


def _earlyfusion(tmp_path, tag, tracks):
    from acoss_amd.algorithms import EarlyFusion
    a = EarlyFusion(_dataset(tmp_path, tag, len(tracks)), "feat/", shortname=tag)
    a.set_block_features(tracks, ["w%d" % (i // 2) for i in range(len(tracks))])
    return a


def _close(algo):
    if getattr(algo, "_ctx", None) is not None:
        algo._ctx.close()
        algo._ctx = None
    algo.cleanup_memmap()


def _rows_disjoint(sec):
    rows = sorted((int(a["q0"]), int(a["q1"])) for a in sec)
    return all(a[1] < b[0] for a, b in zip(rows, rows[1:]))


def _py_tracks():
    blocks = [90, 120, 70, 100, 64, 130, 80, 110]
    tracks = [_track(nb, 53000 + k) for k, nb in enumerate(blocks)]
    rng = np.random.default_rng(53999)
    _copy(tracks, rng, 0, 1, 20, 60, 40)
    _copy(tracks, rng, 0, 1, 65, 5, 20)
    _copy(tracks, rng, 2, 7, 10, 50, 30)
    _copy(tracks, rng, 6, 3, 0, 40, 35)
    return tracks


def test_align_sections_on_the_planted_recording(tmp_path, monkeypatch):
    """Track B = blocks 100 .. 179 of A followed by blocks 20 .. 99 of A (a little noise added): for (B, A) rows 0 .. 79 lie on the
    diagonal r - q = 100 and rows 80 .. 159 on r - q = -60.  Asserted is structure only -- at least two sections, disjoint rows, fields
    and paths against the reference on the device's plot --; the spans and the share of path cells on each planted diagonal are
    printed: what the binarisation and chance matches add is not known in advance."""
    monkeypatch.chdir(tmp_path)
    A = _track(200, 54000)
    rng = np.random.default_rng(54001)
    B = {}
    for key in ("mfccs", "ssms", "chromas"):
        both = np.concatenate([A[key][100:180], A[key][20:100]])
        B[key] = (both + 0.02 * rng.standard_normal(both.shape)).astype(np.float32)
    B["chroma_med"] = A["chroma_med"].copy()
    idxs = [[1, 0], [0, 1]]
    kw = dict(max_sections=4, min_score=5.0, pad=2)
    algo = _earlyfusion(tmp_path, "efsecplanted", [A, B])
    try:
        for stype in ("early", "chromas"):
            plane = PLANES.index(stype)
            sections, paths = algo.align_sections(idxs, similarity_type=stype, paths=True, **kw)
            plain = algo.align_sections(idxs, similarity_type=stype, **kw)
            al = algo.align(idxs, similarity_type=stype)
            assert len(sections) == len(paths) == len(plain) == 2
            for k in range(2):
                sec = sections[k]
                db = algo._context().ef_debug_bits(np.array(idxs, np.int32)[k:k + 1], 0, kappa=algo.kappa, K=algo.K)
                P, _ = backend.unpack_bits(db["bits"][plane], 200 if k == 0 else 160)
                assert sec.dtype == algo.ALIGN_DTYPE and sec.tobytes() == plain[k].tobytes() and len(paths[k]) == len(sec)
                assert len(sec) >= 2 and _rows_disjoint(sec), sec
                assert sec[:1].tobytes() == al[k:k + 1].tobytes(), "section 0 is align()'s row"
                want, wpaths = ref.sections_full(P, **kw)
                assert [_rec(a) for a in sec] == want and all(np.array_equal(a, b) for a, b in zip(paths[k], wpaths))
                for a in sec:
                    assert tuple(a["q_span"]) == (a["q0"], a["q1"] + algo.blocksize - 1) and tuple(a["r_span"]) == (a["r0"], a["r1"] + algo.blocksize - 1)
                for s, (a, cells) in enumerate(zip(sec, paths[k])):
                    d = cells[:, 1] - cells[:, 0] if k == 0 else cells[:, 0] - cells[:, 1]
                    print("%s pair %d section %d: score %.1f, query span %s, reference span %s, %d cells, %d on r - q = 100, %d on r - q = -60" % (
                        stype, k, s, a["score"], a["q_span"].tolist(), a["r_span"].tolist(), len(cells), int(np.sum(d == 100)), int(np.sum(d == -60))))
        assert algo.align_sections(np.zeros((0, 2), np.int64)) == [] and algo.align_sections(np.zeros((0, 2), np.int64), paths=True) == ([], [])
        al = algo.align(idxs)
        first = algo.align_sections(idxs, max_sections=1, min_score=5.0)
        assert all(f.tobytes() == al[k:k + 1].tobytes() for k, f in enumerate(first)), "max_sections = 1 is align()"
        assert not any(np.any(D) for D in algo.Ds.values()), "Ds is not written"
    finally:
        _close(algo)


def test_align_match_sections_on_identify_output_and_in_a_session(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    tracks = _py_tracks()
    n = len(tracks)
    algo = _earlyfusion(tmp_path, "efsecmatches", tracks[:n - 2])
    whole = _earlyfusion(tmp_path, "efsecwhole", tracks)
    kw = dict(max_sections=3, min_score=2.0)
    try:
        queries = [0, 5, 3]
        idx, _ = algo.identify(queries, k=3)["early"]
        idx = idx.copy()
        idx[1, 2] = -1                                         # an empty slot
        got, paths = algo.align_match_sections(queries, idx, paths=True, **kw)
        bare = algo.align_match_sections(queries, idx, **kw)
        assert len(got) == len(paths) == 3 and all(len(row) == 3 for row in got) and all(len(row) == 3 for row in paths)
        assert got[1][2].shape == (0,) and got[1][2].dtype == algo.ALIGN_DTYPE and paths[1][2] == [], "an empty slot"
        for i, q in enumerate(queries):
            filled = [s for s in range(3) if idx[i, s] >= 0]
            row, row_paths = algo.align_sections([[q, idx[i, s]] for s in filled], paths=True, **kw)
            for t, s in enumerate(filled):
                assert got[i][s].tobytes() == row[t].tobytes() == bare[i][s].tobytes() and _rows_disjoint(got[i][s])
                assert len(paths[i][s]) == len(row_paths[t]) and all(np.array_equal(a, b) for a, b in zip(paths[i][s], row_paths[t]))
        # inside appended() the indices run over N + Q: the same sections as on an object that holds all the tracks
        pairs = [[0, n - 2], [n - 1, 2], [n - 2, 3]]
        want, wpaths = whole.align_sections(pairs, pad=1, paths=True, similarity_type="chromas", **kw)
        assert max(len(w) for w in want) >= 1
        with pytest.raises(ValueError, match="align_sections: idxs must be track indices in \\[0, %d\\)" % (n - 2)):
            algo.align_sections(pairs)
        with algo.appended(tracks[n - 2:]) as s:
            assert s.total == n
            inside, ipaths = algo.align_sections(pairs, pad=1, paths=True, similarity_type="chromas", **kw)
            m_in = algo.align_match_sections([n - 1], [[0, -1, n - 2]], pad=1, **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(inside, want))
        assert all(np.array_equal(x, y) for a, b in zip(ipaths, wpaths) for x, y in zip(a, b))
        m_want = whole.align_sections([[n - 1, 0], [n - 1, n - 2]], pad=1, **kw)
        assert m_in[0][0].tobytes() == m_want[0].tobytes() and len(m_in[0][1]) == 0 and m_in[0][2].tobytes() == m_want[1].tobytes()
    finally:
        _close(algo)
        _close(whole)
