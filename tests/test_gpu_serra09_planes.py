"""
The wide class's per-rotation operand planes (planepool_kernel and band_kernel<M, 8, role, WD2, 0, FAST, PLANES>,
acoss_amd/csrc/serra09_kernels.hpp; ensure_planes, acx.hip): for each rotation rot = 0..11 one plane that holds, per frame, the four
triples the lanes lk = 0..3 of a pair of that rotation load, 48 bytes per frame, frames consecutive.  Only addresses differ from the
rotated pool, so everything is compared bit for bit (np.array_equal): scores, thresholds, distances and plots against the CPU oracle,
and the scores of a process that runs with ACX_PLANES=0 (the switch is read once per process, so that run is a child process; one
child serves every list).  acx_serra09_plane_launches counts the launches that read the planes: a dispatch that never took them
fails here.

The layout itself needs no GPU: test_plane_layout_model compares a numpy model of the planes, built from the rotated pool's
definition, with the kernel's addressing formula for every (rot, lk, kb).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _serra09_shapes as S
from tests._serra09_compare import compare_pair

M = 9
NBIN = 12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the layout, without a GPU ------------------------------------------------------------

def _rotated_pool(frames):
    """rotpool_kernel: frot[f][r][cls][kb] = frame[f][cls + 4 ((r + kb) mod 3)]."""
    out = np.empty((len(frames), 3, 4, 3), frames.dtype)
    for r in range(3):
        for cls in range(4):
            for kb in range(3):
                out[:, r, cls, kb] = frames[:, cls + 4 * ((r + kb) % 3)]
    return out.reshape(len(frames), 36)


def _planes(frot):
    """planepool_kernel: plane rot, frame f, float 3 lk + kb = the rotated pool's float (r, cls, kb) of c0 = (lk - rot) mod 12,
    r = c0 / 4, cls = c0 % 4."""
    out = np.empty((NBIN, len(frot), NBIN), frot.dtype)
    for rot in range(NBIN):
        for lk in range(4):
            c0 = (lk - rot) % NBIN
            for kb in range(3):
                out[rot, :, 3 * lk + kb] = frot[:, (c0 // 4) * NBIN + (c0 % 4) * 3 + kb]
    return out


def test_plane_layout_model():
    """Lane (lr, lk) of the 16-frame block at frame b of a pair of rotation rot reads 12 bytes at byte 48 (b + lr) + 12 lk of plane
    rot (the kernel: descriptor at the plane's frame, lane offset 48 lr + 12 lk, scalar tile offset in units of 48).  Those three
    floats must be (a) what the same lane reads from the rotated pool at byte 144 (b + lr) + 4 (12 r + 3 cls) and (b) the rotated
    frame's bins 4 kb + lk, kb = 0, 1, 2: the k-steps of the MFMA chain.  Every (rot, lk, kb), every frame of a 64-frame track."""
    rng = np.random.default_rng(1)
    frames = rng.random((64, NBIN)).astype(np.float32)
    frot = _rotated_pool(frames)
    planes = _planes(frot)
    flat = planes.reshape(NBIN, -1).view(np.uint8)                      # a plane as bytes
    frot_b = frot.reshape(-1).view(np.uint8)
    seen = set()
    for rot in range(NBIN):
        rolled = np.roll(frames, rot, axis=1)                             # rotated bin b = source bin (b - rot) mod 12
        for lk in range(4):
            c0 = (lk - rot) % NBIN
            offB = 4 * ((c0 // 4) * NBIN + (c0 % 4) * 3)                  # the kernel's offB on the rotated pool
            for b in range(0, 64, 16):
                for lr in range(16):
                    got = flat[rot, 48 * (b + lr) + 12 * lk:][:12].view(np.float32)
                    old = frot_b[144 * (b + lr) + offB:][:12].view(np.float32)
                    assert np.array_equal(got, old), (rot, lk, b, lr)
                    for kb in range(3):
                        assert got[kb] == rolled[b + lr, 4 * kb + lk], (rot, lk, kb, b, lr)
                        seen.add((rot, lk, kb))
    assert len(seen) == NBIN * 4 * 3
    # one wave instruction (16 frames x 4 lk x 12 bytes) covers 768 contiguous bytes of the plane
    offs = sorted(48 * lr + 12 * lk + e for lr in range(16) for lk in range(4) for e in range(12))
    assert offs == list(range(768))


# ---- on the GPU ---------------------------------------------------------------------------

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from acoss_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _biased(rng, T, b, weight=3.0):
    """iid frames with bin b raised: the global chroma peaks at b, so the transposition index of a pair follows the two peaks."""
    from acoss_amd import synth
    x = rng.random((T, NBIN))
    x[:, b] += weight
    return synth._frame_max_normalise(x)


def _iid(rng, T):
    from acoss_amd import synth
    return synth._frame_max_normalise(rng.random((T, NBIN)))


def _set(tracks, pairs):
    from acoss_amd import synth
    frames, offsets = synth.pack(tracks)
    return dict(frames=frames, offsets=offsets, pairs=np.ascontiguousarray(pairs, np.int32).reshape(-1, 2),
                M=np.array([S._embed_len(len(t), M) for t in tracks], np.int64))


def _edge_set():
    """Wide tracks of 1018 + 9 (the class's first length), 1999, 2000 (a last tile of 7 and of 8 cells) and 2040 + 9 frames (its last)
    with their chroma peak at bin 0, and twelve short tracks of 60 frames peaking at bins 0..11: short x wide is the wide class in the
    row pass, wide x short in the column pass, and the twelve peaks give the twelve transposition indices.  Two wide x wide pairs
    (both passes wide at once).  The wide tracks are the pool's first and last tracks: their edge tiles read the slack."""
    rng = np.random.default_rng(801)
    wide = [1027, 1999, 2000, 2049]
    tracks = [_biased(rng, wide[0], 0)] + [_biased(rng, 60, b) for b in range(NBIN)] + [_biased(rng, T, 0) for T in wide[1:]]
    w = [0, 13, 14, 15]
    pairs = []
    for b in range(NBIN):
        pairs.append((1 + b, w[b % 4]))          # row pass wide
        pairs.append((w[(b + 1) % 4], 1 + b))    # column pass wide
    pairs += [(0, 15), (14, 13)]
    d = _set(tracks, pairs)
    assert [int(d["M"][t]) for t in w] == [1018, 1990, 1991, 2040]
    assert all(S.cls(int(d["M"][t]), M) == 4 for t in w) and S.cls(int(d["M"][1]), M) == 0
    return d


def _mixed_set():
    """Wide, middle and narrow classes in one batch: tracks of 2000, 1500, 700, 300 and 60 frames, every ordered pair."""
    rng = np.random.default_rng(802)
    tracks = [_iid(rng, T) for T in (2000, 1500, 700, 300, 60)]
    pairs = [(i, j) for i in range(5) for j in range(5) if i != j]
    d = _set(tracks, pairs)
    assert sorted({S.cls(int(m), M) for m in d["M"]}) == [0, 1, 2, 4]
    return d


_SETS = {"edge": _edge_set, "mixed": _mixed_set}


@pytest.fixture(scope="module")
def sets():
    return {k: f() for k, f in _SETS.items()}


@pytest.fixture(scope="module")
def oracle_edge(sets):
    """The oracle over the edge set, once: (score, intermediates) per pair."""
    import oracle
    oracle.lib()
    d = sets["edge"]
    p = oracle.serra09_params(m=M)
    return S.pool_map(lambda ij: oracle.serra09_pair(S.track(d, ij[0]), S.track(d, ij[1]), p, want_intermediates=True), d["pairs"])


def _planes_on(ctx, call):
    """call() must launch kernels that read the planes."""
    from acoss_amd import _lib
    n0 = _lib.serra09_plane_launches()
    out = call()
    assert _lib.serra09_plane_launches() > n0, "no band launch of this call read the operand planes"
    return out


@gpu
def test_all_rotations_at_the_class_edges(ctx, sets, oracle_edge):
    """Scores against the oracle, all twelve transposition indices, the four edge lengths, rows and columns."""
    from acoss_amd import _lib
    d = sets["edge"]
    otis = {(int(it["oti"]), "row" if S.cls(int(d["M"][j]), M) == 4 and S.cls(int(d["M"][i]), M) != 4 else "col")
            for (i, j), (_, it) in zip(d["pairs"][:24], oracle_edge)}
    assert {o for o, r in otis if r == "row"} == set(range(NBIN)), otis
    assert {o for o, r in otis if r == "col"} == set(range(NBIN)), otis
    want = np.array([s for s, _ in oracle_edge], np.float32)
    ctx.upload_pool(d["frames"], d["offsets"])
    got = _planes_on(ctx, lambda: ctx.serra09_pairs(d["pairs"], _lib.serra09_params(m=M)))
    S.assert_scores_equal(d, M, got, want, "edge set")
    scores, Rs = _planes_on(ctx, lambda: ctx.serra09_debug_bits(d["pairs"], _lib.serra09_params(m=M)))
    S.assert_plots_equal(d, M, Rs, [it["R"] for _, it in oracle_edge], "edge set")
    S.assert_scores_equal(d, M, scores, want, "edge set, debug_bits")


@gpu
def test_thresholds_and_distances_through_the_debug_entry(ctx, sets, oracle_edge):
    """acx_serra09_debug_pair (the D2-writing copy of the wide kernel, also on the planes): transposition index, distances, eps, the
    d2-domain thresholds, plot and score of the first pair, of a column-pass pair with another rotation and of a wide x wide pair."""
    import oracle
    from acoss_amd import _lib
    d = sets["edge"]
    ctx.upload_pool(d["frames"], d["offsets"])
    for k in (0, 3, 24):
        i, j = (int(x) for x in d["pairs"][k])
        _planes_on(ctx, lambda: compare_pair(ctx, d, i, j, _lib.serra09_params(m=M), oracle.serra09_params(m=M), "pair %d" % k,
                                             ref=oracle_edge[k]))


_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from acoss_amd import _lib
from tests import test_gpu_serra09_planes as T
ctx = _lib.Context(0)
out = {}
for name, make in T._SETS.items():
    d = make()
    ctx.upload_pool(d["frames"], d["offsets"])
    out[name] = [float(x) for x in ctx.serra09_pairs(d["pairs"], _lib.serra09_params(m=T.M))]
out["plane_launches"] = _lib.serra09_plane_launches()
ctx.close()
print("RESULT " + json.dumps(out))
"""


@gpu
def test_planes_off_gives_the_same_scores(ctx, sets):
    """The same pair lists in a process with ACX_PLANES=0 (which must not launch a plane kernel) and here: identical scores.  The
    lists: the edge set (wide tracks first and last in the pool: the slack) and a batch that mixes wide and narrower classes."""
    from acoss_amd import _lib
    env = dict(os.environ, ACX_PLANES="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    off = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert off["plane_launches"] == 0
    for name, d in sets.items():
        ctx.upload_pool(d["frames"], d["offsets"])
        on = _planes_on(ctx, lambda: ctx.serra09_pairs(d["pairs"], _lib.serra09_params(m=M)))
        S.assert_scores_equal(d, M, on, np.array(off[name], np.float32), name + ": planes on vs off")


@gpu
def test_planes_follow_the_pool(ctx, sets):
    """A stale plane pool fails here: the planes exist (a wide batch ran), then a wide track is appended and pairs with it must match
    the oracle; then the pool is cut back and another track appended in its place; then a second upload replaces everything."""
    from acoss_amd import _lib
    rng = np.random.default_rng(803)
    a, b, s = _biased(rng, 1500, 2), _biased(rng, 1999, 7), _iid(rng, 60)
    d0 = _set([s, a], [(0, 1), (1, 0)])
    p = _lib.serra09_params(m=M)
    ctx.upload_pool(d0["frames"], d0["offsets"])
    S.assert_scores_equal(d0, M, _planes_on(ctx, lambda: ctx.serra09_pairs(d0["pairs"], p)), S.oracle_scores(d0, m=M), "before the append")
    # append a wide track behind the pool's end
    ctx.pool_append(b, np.array([0, len(b)], np.int64))
    d1 = _set([s, a, b], [(0, 2), (2, 0), (1, 2), (0, 1)])
    want1 = S.oracle_scores(d1, m=M)
    S.assert_scores_equal(d1, M, _planes_on(ctx, lambda: ctx.serra09_pairs(d1["pairs"], p)), want1, "after the append")
    # cut it off again and append another one where it was
    ctx.pool_truncate(_lib.ALGO_SERRA09, 2)
    c = _biased(rng, 1100, 5)
    ctx.pool_append(c, np.array([0, len(c)], np.int64))
    d2 = _set([s, a, c], [(0, 2), (2, 0), (1, 2), (0, 1)])
    S.assert_scores_equal(d2, M, _planes_on(ctx, lambda: ctx.serra09_pairs(d2["pairs"], p)), S.oracle_scores(d2, m=M), "after truncate + append")
    # a second upload: the first set's tracks in another order
    d3 = _set([b, s, a], [(1, 0), (0, 1), (2, 0), (1, 2)])
    ctx.upload_pool(d3["frames"], d3["offsets"])
    S.assert_scores_equal(d3, M, _planes_on(ctx, lambda: ctx.serra09_pairs(d3["pairs"], p)), S.oracle_scores(d3, m=M), "after a second upload")
