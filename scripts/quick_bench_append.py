"""identify_tracks() against the only route that answered the same question before it, for Serra09 on a covers-shaped
pool (as quick_bench_identify.py: sets of 164 tracks / 80 works, T ~ U{150..650} pooled frames) of 15 000 tracks,
Q = 128 tracks the collection does not hold, k = 10:

    python scripts/quick_bench_append.py [n_tracks] [--queries 128] [--k 10] [--reps 3] [--out FILE]

  leg (a)   algo.identify_tracks(new, k): append behind the uploaded pool, one query band, truncate
  leg (b)   an object over the N + Q tracks: the whole collection uploaded again with the new tracks behind it, then
            identify(queries=[N ..], k, candidates=range(N))

Both legs run in one process, alternating, `reps` times each after one warm-up each; every run is reported, leg (b) with
its upload and its identify() apart.  One more run of leg (a) takes the three steps one by one (append, band, truncate),
and one more run of each leg with the library's event clocks on gives the per-kernel-family milliseconds
(acx_profile_*).  The lists of the two legs must be equal (indices and score bits): the script asserts it."""
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
OUT = os.path.abspath(OUT or os.path.join(ROOT, "profiles", "append_%d.json" % N))
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
a = Serra09("a.csv", "feat/", shortname="append_a")
a.set_pooled_features(tracks[:N], labels_a)
b = Serra09("b.csv", "feat/", shortname="append_b")
b.set_pooled_features(tracks, labels_b)
ctx_a, ctx_b = a._context(), b._context()
new_q, old_c = np.arange(N, N + Q), np.arange(N)


def leg_a():
    ctx_a.dev_sync()
    t0 = time.perf_counter()
    out = a.identify_tracks(new, k=K)["main"]
    ctx_a.dev_sync()
    return {"wall_s": round(time.perf_counter() - t0, 4)}, out


def leg_b():
    b._pool_ready = False                            # the route that exists without appends: the collection goes up again
    ctx_b.dev_sync()
    t0 = time.perf_counter()
    b._context()
    ctx_b.dev_sync()
    t1 = time.perf_counter()
    out = b.identify(new_q, k=K, candidates=old_c)["main"]
    ctx_b.dev_sync()
    t2 = time.perf_counter()
    return {"wall_s": round(t2 - t0, 4), "upload_s": round(t1 - t0, 4), "identify_s": round(t2 - t1, 4)}, out


def leg_a_steps():
    """identify_tracks' three steps by hand, each between two device synchronisations."""
    _, algo, params, mode, col = a._query_call()
    checked = a._check_tracks("quick_bench_append", new)
    marks = [time.perf_counter()]
    tail = a._append_tracks(ctx_a, checked)
    ctx_a.dev_sync()
    marks.append(time.perf_counter())
    out = ctx_a.query_topk(algo, True, params, new_q.astype(np.int32), K, candidates=old_c.astype(np.int32),
                           col=np.concatenate([col, tail]), col_mode=mode)
    ctx_a.dev_sync()
    marks.append(time.perf_counter())
    ctx_a.pool_truncate(algo, N)
    ctx_a.dev_sync()
    marks.append(time.perf_counter())
    d = np.diff(marks)
    return {"append_s": round(d[0], 4), "band_s": round(d[1], 4), "truncate_s": round(d[2], 4)}, (out[0][:, 0], out[1][:, 0])


def profiled(fn, ctx):
    ctx.profile_enable(True)
    ctx.profile_reset()
    t, _ = fn()
    prof = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in ctx.profile().items() if v["launches"]}
    ctx.profile_enable(False)
    return dict(t, kernels_ms=prof)


def same(x, y):
    return np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32))


legs = {"identify_tracks": leg_a, "reupload_identify": leg_b}
first = {leg: fn() for leg, fn in legs.items()}
want = first["reupload_identify"][1]
assert same(first["identify_tracks"][1], want)
runs = {leg: [] for leg in legs}
for _ in range(REPS):
    for leg, fn in legs.items():
        t, got = fn()
        runs[leg].append(t)
        assert same(got, want), leg
steps = []
for _ in range(REPS):
    t, got = leg_a_steps()
    steps.append(t)
    assert same(got, want), "steps"
rec = {"n_tracks": N, "new_tracks": Q, "k": K, "reps": REPS, "pool": "covers-shaped, T ~ U{150..650}", "pairs_per_leg": int(Q * N),
       "protocol": "one process, one object per leg; a warm-up of each leg, then the legs alternating; wall seconds with a device "
                   "synchronise on either side; kernels_ms: one further run per leg with acx_profile on",
       "warm_up": {leg: first[leg][0] for leg in legs}, "runs": runs, "identify_tracks_steps": steps,
       "with_event_clocks": {"identify_tracks": profiled(leg_a, ctx_a), "reupload_identify": profiled(leg_b, ctx_b)},
       "lists_equal": True}
print(json.dumps(rec), flush=True)
a.cleanup_memmap()
b.cleanup_memmap()
ctx_a.close()
ctx_b.close()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
