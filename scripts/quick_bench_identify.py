"""identify() against the route that answered the same question before it, on a collection of 15 000 tracks, Q = 128
queries, k = 10:

  Serra09   covers-shaped pool (bench_other.py's covers leg: sets of 164 tracks / 80 works, T ~ U{150..650} pooled frames)
  FTM2D     injected random shingles (12 x 75 values)

    python scripts/quick_bench_identify.py [n_tracks] [--queries 128] [--k 10] [--reps 3] [--algos serra09,ftm2d] [--out FILE]

  leg (a)   algo.identify(queries, k)
  leg (b)   the same cells through what existed before: similarity(idxs) over the Q (N - 1) pairs into the N x N float32
            memmap, the mirror of the cells computed as (column, query), normalize_by_length's arithmetic on the Q rows,
            top_matches(type, k, rows=queries)

Both legs run in one process on one object, alternating, `reps` times each after one warm-up each; every run is reported.
One more run of each with the library's event clocks on gives the per-kernel-family milliseconds (acx_profile_*).  The
lists of the two legs must be equal (indices and score bits): the script asserts it."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd import synth  # noqa: E402
from acoss_amd.algorithms import FTM2D, Serra09  # noqa: E402


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
ALGOS = _opt("--algos", "serra09,ftm2d").split(",")
OUT = _opt("--out")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 15000
OUT = os.path.abspath(OUT or os.path.join(ROOT, "profiles", "identify_%d.json" % N))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
os.chdir(tempfile.mkdtemp())
with open("ds.csv", "w") as f:
    f.write("work_id,track_id\n")
    for i in range(N):
        f.write("w%d,t%d\n" % (i // 2, i))
labels = ["w%d" % (i // 2) for i in range(N)]
rng = np.random.default_rng(2025)
queries = np.sort(rng.choice(N, size=Q, replace=False)).astype(np.int64)


def make_serra09():
    sets = [synth.covers80_shaped(seed=100 + s, t_range=(150, 650)) for s in range((N + 163) // 164)]
    tracks = [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for d in sets for i in range(len(d["offsets"]) - 1)][:N]
    a = Serra09("ds.csv", "feat/", shortname="identify")
    a.set_pooled_features(tracks, labels)
    norm = np.sqrt(np.array([len(t) for t in tracks], dtype=np.float64))
    return a, lambda rows: (rows / norm[None, :]).astype(np.float32), "covers-shaped, T ~ U{150..650}"


def make_ftm2d():
    S = rng.standard_normal((N, 900))
    S /= np.linalg.norm(S, axis=1, keepdims=True)
    a = FTM2D("ds.csv", "feat/", shortname="identify")
    a.set_features(list(S), labels)
    return a, None, "injected unit shingles of 900 values"


def old_route(a, normalise):
    """Leg (b): pair list -> memmap -> host normalisation of the rows -> back to the device for the ranking."""
    cols = np.arange(N, dtype=np.int64)
    idxs = np.concatenate([np.stack([np.minimum(q, cols[cols != q]), np.maximum(q, cols[cols != q])], 1) for q in queries])
    a.similarity(idxs)
    D = a.Ds["main"]
    for q in queries:
        D[q, :q] = D[:q, q]                          # the cells computed as (column, query)
    if normalise is not None:
        D[queries] = normalise(np.asarray(D[queries]))
    return a.top_matches("main", K, rows=queries)


def new_route(a, normalise):
    return a.identify(queries, k=K)["main"]


def timed(fn, a, normalise, ctx):
    a.Ds["main"][queries] = 0
    ctx.dev_sync()
    t0 = time.perf_counter()
    out = fn(a, normalise)
    ctx.dev_sync()
    return time.perf_counter() - t0, out


def profiled(fn, a, normalise, ctx):
    ctx.profile_enable(True)
    ctx.profile_reset()
    t, _ = timed(fn, a, normalise, ctx)
    prof = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in ctx.profile().items() if v["launches"]}
    ctx.profile_enable(False)
    return {"wall_s": round(t, 4), "kernels_ms": prof}


rec = {"n_tracks": N, "queries": Q, "k": K, "reps": REPS,
       "protocol": "one process, one object per algorithm; a warm-up of each leg, then the legs alternating; wall seconds around the "
                   "whole call with a device synchronise on either side; kernels_ms: one further run per leg with acx_profile on"}
for name in ALGOS:
    a, normalise, what = make_serra09() if name == "serra09" else make_ftm2d()
    ctx = a._context()
    legs = {"identify": new_route, "pair_list_memmap_topk": old_route}
    first = {leg: timed(fn, a, normalise, ctx) for leg, fn in legs.items()}
    want = first["pair_list_memmap_topk"][1]
    times = {leg: [] for leg in legs}
    for _ in range(REPS):
        for leg, fn in legs.items():
            t, got = timed(fn, a, normalise, ctx)
            times[leg].append(round(t, 4))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (name, leg)
    rec[name] = {"pool": what, "pairs_per_leg": int(Q * (N - 1)),
                 "wall_s": times, "warm_up_s": {leg: round(first[leg][0], 4) for leg in legs},
                 "with_event_clocks": {leg: profiled(fn, a, normalise, ctx) for leg, fn in legs.items()},
                 "lists_equal": True}
    print(json.dumps({name: rec[name]}), flush=True)
    a.cleanup_memmap()
    ctx.close()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
