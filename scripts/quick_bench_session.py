"""locate_tracks() -- which tracks of the collection are the covers of new tracks, and where they match, in ONE append --
against the two other routes to the same answer, for Serra09 on the covers-shaped pool of quick_bench_append.py (sets of
164 tracks / 80 works, T ~ U{150..650} pooled frames) of 15 000 tracks, Q = 128 tracks the collection does not hold, k = 10:

    python scripts/quick_bench_session.py [n_tracks] [--queries 128] [--k 10] [--reps 3] [--out FILE]

  leg (a)   algo.locate_tracks(new, k): one append, one query band, the Q x k alignments, one truncate
  leg (b)   algo.identify_tracks(new, k) followed by algo.align_tracks(new, idx): the same work in two appends
  leg (c)   the only route without sessions: an object over the N + Q tracks whose pool is uploaded again with the new
            tracks behind it, then identify(queries=[N ..], k, candidates=range(N)) and align_matches(queries, idx)

All legs run in one process, alternating, `reps` times each after one warm-up each; every run is reported, legs (b) and (c)
with their steps apart.  The three answers must be equal (indices, score bits and every field of every record): the script
asserts it in every run.  There is no speed gate."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd import synth  # noqa: E402
from acoss_amd.algorithms import Serra09  # noqa: E402


def _opt(name, default=None):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    v = sys.argv[k + 1]
    del sys.argv[k:k + 2]
    return v


Q = int(_opt("--queries", 128))
K = int(_opt("--k", 10))
REPS = int(_opt("--reps", 3))
OUT = _opt("--out")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 15000
OUT = os.path.abspath(OUT or os.path.join(ROOT, "profiles", "session_%d.json" % N))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
os.chdir(tempfile.mkdtemp())


def dataset(name, n):
    with open(name, "w") as f:
        f.write("work_id,track_id\n")
        for i in range(n):
            f.write("w%d,t%d\n" % (i // 2, i))
    return ["w%d" % (i // 2) for i in range(n)]


sets = [synth.covers80_shaped(seed=100 + s, t_range=(150, 650)) for s in range((N + Q + 163) // 164)]
tracks = [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for d in sets for i in range(len(d["offsets"]) - 1)][:N + Q]
new = tracks[N:]
labels_a, labels_b = dataset("a.csv", N), dataset("b.csv", N + Q)
a = Serra09("a.csv", "feat/", shortname="session_a")
a.set_pooled_features(tracks[:N], labels_a)
b = Serra09("b.csv", "feat/", shortname="session_b")
b.set_pooled_features(tracks, labels_b)
ctx_a, ctx_b = a._context(), b._context()
new_q, old_c = np.arange(N, N + Q), np.arange(N)


def clock(ctx, marks):
    ctx.dev_sync()
    marks.append(time.perf_counter())


def leg_a():
    marks = []
    clock(ctx_a, marks)
    idx, score, al = a.locate_tracks(new, k=K)
    clock(ctx_a, marks)
    return {"wall_s": round(marks[1] - marks[0], 4)}, (idx, score, al)


def leg_b():
    marks = []
    clock(ctx_a, marks)
    idx, score = a.identify_tracks(new, k=K)["main"]
    clock(ctx_a, marks)
    al = a.align_tracks(new, idx)
    clock(ctx_a, marks)
    d = np.diff(marks)
    return {"wall_s": round(marks[2] - marks[0], 4), "identify_tracks_s": round(d[0], 4), "align_tracks_s": round(d[1], 4)}, (idx, score, al)


def leg_c():
    b._pool_ready = False                            # the route that exists without appends: the collection goes up again
    marks = []
    clock(ctx_b, marks)
    b._context()
    clock(ctx_b, marks)
    idx, score = b.identify(new_q, k=K, candidates=old_c)["main"]
    clock(ctx_b, marks)
    al = b.align_matches(new_q, idx)
    clock(ctx_b, marks)
    d = np.diff(marks)
    return {"wall_s": round(marks[3] - marks[0], 4), "upload_s": round(d[0], 4), "identify_s": round(d[1], 4), "align_matches_s": round(d[2], 4)}, (idx, score, al)


def same(x, y):
    return all(u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes() for u, v in zip(x, y))


legs = {"locate_tracks": leg_a, "identify_tracks+align_tracks": leg_b, "reupload+identify+align_matches": leg_c}
first = {leg: fn() for leg, fn in legs.items()}
want = first["reupload+identify+align_matches"][1]
for leg in legs:
    assert same(first[leg][1], want), leg
runs = {leg: [] for leg in legs}
for _ in range(REPS):
    for leg, fn in legs.items():
        t, got = fn()
        runs[leg].append(t)
        assert same(got, want), leg
rec = {"n_tracks": N, "new_tracks": Q, "k": K, "reps": REPS, "pool": "covers-shaped, T ~ U{150..650}", "pairs_per_band": int(Q * N),
       "alignments": int(np.count_nonzero(want[0] >= 0)),
       "protocol": "one process, one object for legs (a) and (b), one for leg (c); a warm-up of each leg, then the legs alternating; wall "
                   "seconds with a device synchronise on either side of every step",
       "warm_up": {leg: first[leg][0] for leg in legs}, "runs": runs, "answers_equal": True}
print(json.dumps(rec), flush=True)
a.cleanup_memmap()
b.cleanup_memmap()
ctx_a.close()
ctx_b.close()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
