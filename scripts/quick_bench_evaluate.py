"""evaluate() against the route through the N x N matrix, on a collection of 15 000 tracks:

  Serra09   covers-shaped pool (bench_other.py's covers leg: sets of 164 tracks / 80 works, T ~ U{150..650} pooled frames)
  FTM2D     injected random shingles (12 x 75 values), labelled in cliques of two

    python scripts/quick_bench_evaluate.py [n_tracks] [--subset 1280] [--reps 3] [--algos serra09,ftm2d] [--out FILE]

  leg (a)   algo.evaluate()                          every track a query, no matrix
  leg (b)   algo.all_pairwise(symmetric=True) + normalize_by_length() (where the class has one) +
            getEvalStatistics("main", engine="device")    the route through the (N, N) float32 memmap
  leg (c)   algo.evaluate(queries=<subset>)          1 280 random tracks against the collection

Legs (a) and (b) run in one process on one object, alternating, `reps` times each after one warm-up each; every run is
reported and the two tuples must be equal bit for bit: the script asserts it.  Leg (c) runs `reps` times after them.  One
more run of each leg with the library's event clocks on gives the per-kernel-family milliseconds (acx_profile_*).  A
symmetric class computes every unordered pair twice in leg (a), once in the band of each end: the pair-kernel
milliseconds of the two legs state that ratio."""
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


SUBSET = int(_opt("--subset", 1280))
REPS = int(_opt("--reps", 3))
ALGOS = _opt("--algos", "serra09,ftm2d").split(",")
OUT = _opt("--out")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 15000
OUT = os.path.abspath(OUT or os.path.join(ROOT, "profiles", "evaluate_%d.json" % N))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
os.chdir(tempfile.mkdtemp())
with open("ds.csv", "w") as f:
    f.write("work_id,track_id\n")
    for i in range(N):
        f.write("w%d,t%d\n" % (i // 2, i))
rng = np.random.default_rng(2025)
subset = rng.choice(N, size=min(SUBSET, N), replace=False).astype(np.int64)
TOPS = [1, 10, 100, 1000]


def make_serra09():
    sets = [synth.covers80_shaped(seed=100 + s, t_range=(150, 650)) for s in range((N + 163) // 164)]
    tracks = [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for d in sets for i in range(len(d["offsets"]) - 1)][:N]
    labels = ["s%d_%s" % (s, l) for s, d in enumerate(sets) for l in d["labels"]][:N]
    a = Serra09("ds.csv", "feat/", shortname="evaluate")
    a.set_pooled_features(tracks, labels)
    return a, "covers-shaped, T ~ U{150..650}, the sets' own works as cliques"


def make_ftm2d():
    S = rng.standard_normal((N, 900))
    S /= np.linalg.norm(S, axis=1, keepdims=True)
    a = FTM2D("ds.csv", "feat/", shortname="evaluate")
    a.set_features(list(S), ["w%d" % (i // 2) for i in range(N)])
    return a, "injected unit shingles of 900 values, cliques of two"


def matrix_route(a):
    a.all_pairwise(symmetric=True)
    if hasattr(a, "normalize_by_length"):
        a.normalize_by_length()
    return a.getEvalStatistics("main", topsidx=TOPS, engine="device")


def band_route(a):
    return a.evaluate(topsidx=TOPS)["main"]


def subset_route(a):
    return a.evaluate(queries=subset, topsidx=TOPS)["main"]


def timed(fn, a, ctx):
    ctx.dev_sync()
    t0 = time.perf_counter()
    out = fn(a)
    ctx.dev_sync()
    return time.perf_counter() - t0, out


def profiled(fn, a, ctx):
    ctx.profile_enable(True)
    ctx.profile_reset()
    t, _ = timed(fn, a, ctx)
    prof = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in ctx.profile().items() if v["launches"]}
    ctx.profile_enable(False)
    return {"wall_s": round(t, 4), "kernels_ms": prof}


def same(x, y):
    return all(np.float64(x[i]).tobytes() == np.float64(y[i]).tobytes() for i in range(4)) and np.array_equal(x[4], y[4])


def plain(t):
    return [float(t[0]), float(t[1]), float(t[2]), float(t[3]), [float(v) for v in t[4]]]


rec = {"n_tracks": N, "subset": int(len(subset)), "reps": REPS,
       "protocol": "one process, one object per algorithm; a warm-up of each leg, then legs (a) and (b) alternating, then leg (c); "
                   "wall seconds around the whole call with a device synchronise on either side; kernels_ms: one further run per "
                   "leg with acx_profile on"}
for name in ALGOS:
    a, what = make_serra09() if name == "serra09" else make_ftm2d()
    ctx = a._context()
    legs = {"evaluate": band_route, "matrix_getEvalStatistics_device": matrix_route}
    first = {leg: timed(fn, a, ctx) for leg, fn in legs.items()}
    want = first["matrix_getEvalStatistics_device"][1]
    assert same(first["evaluate"][1], want), (name, first["evaluate"][1], want)
    times = {leg: [] for leg in legs}
    for _ in range(REPS):
        for leg, fn in legs.items():
            t, got = timed(fn, a, ctx)
            times[leg].append(round(t, 4))
            assert same(got, want), (name, leg, got, want)
    sub_first = timed(subset_route, a, ctx)
    times["evaluate_subset"] = [round(timed(subset_route, a, ctx)[0], 4) for _ in range(REPS)]
    legs["evaluate_subset"] = subset_route
    rec[name] = {"pool": what, "unordered_pairs": int(N * (N - 1) // 2),
                 "wall_s": times, "warm_up_s": dict({leg: round(first[leg][0], 4) for leg in first}, evaluate_subset=round(sub_first[0], 4)),
                 "with_event_clocks": {leg: profiled(fn, a, ctx) for leg, fn in legs.items()},
                 "statistics": plain(want), "statistics_subset": plain(sub_first[1]), "tuples_equal": True}
    print(json.dumps({name: rec[name]}), flush=True)
    a.cleanup_memmap()
    ctx.close()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
