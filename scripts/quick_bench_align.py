"""align_matches() on the hits of identify(): where in the two recordings the match lies, for Q = 128 queries and k = 10 hits each
(1 280 pairs) on the covers-shaped pool of quick_bench_identify.py (sets of 164 tracks / 80 works, T ~ U{150..650} pooled frames).

    python scripts/quick_bench_align.py [n_tracks] [--queries 128] [--k 10] [--reps 3] [--out FILE]

identify() runs once and is timed; align_matches(queries, hits) runs `reps` times after one warm-up, wall seconds around the call
with a device synchronise on either side.  One further run with the library's event clocks on (acx_profile_*) gives the locating
sweep's milliseconds (qmax_locate_kernel), and serra09_pairs on the same pairs under the same clocks gives the score sweep's
(qmax_bits_kernel) beside it; the two calls' scores must be the same bits, which the script asserts.  Writes profiles/align_<n>.json."""
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
OUT = os.path.abspath(OUT or os.path.join(ROOT, "profiles", "align_%d.json" % N))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
os.chdir(tempfile.mkdtemp())
with open("ds.csv", "w") as f:
    f.write("work_id,track_id\n")
    for i in range(N):
        f.write("w%d,t%d\n" % (i // 2, i))
labels = ["w%d" % (i // 2) for i in range(N)]
rng = np.random.default_rng(2025)
queries = np.sort(rng.choice(N, size=Q, replace=False)).astype(np.int64)

sets = [synth.covers80_shaped(seed=100 + s, t_range=(150, 650)) for s in range((N + 163) // 164)]
tracks = [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for d in sets for i in range(len(d["offsets"]) - 1)][:N]
a = Serra09("ds.csv", "feat/", shortname="align")
a.set_pooled_features(tracks, labels)
ctx = a._context()


def timed(fn):
    ctx.dev_sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.dev_sync()
    return time.perf_counter() - t0, out


def profiled(fn):
    ctx.profile_enable(True)
    ctx.profile_reset()
    t, out = timed(fn)
    prof = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in ctx.profile().items() if v["launches"]}
    ctx.profile_enable(False)
    return {"wall_s": round(t, 4), "kernels_ms": prof}, out


t_identify, (hits, _) = timed(lambda: a.identify(queries, k=K)["main"])
rows, slots = np.nonzero(hits >= 0)
pairs = np.stack([queries[rows], hits[rows, slots]], axis=1).astype(np.int32)
warm, first = timed(lambda: a.align_matches(queries, hits))
times = []
for _ in range(REPS):
    t, got = timed(lambda: a.align_matches(queries, hits))
    times.append(round(t, 4))
    assert np.array_equal(got, first)
prof_align, got = profiled(lambda: a.align_matches(queries, hits))
prof_score, scores = profiled(lambda: ctx.serra09_pairs(pairs, a._params()))
assert np.array_equal(got[rows, slots]["score"].view(np.uint32), scores.view(np.uint32)), "align's scores are serra09_pairs' bits"
hit = first["q0"] >= 0
rec = {"n_tracks": N, "queries": Q, "k": K, "reps": REPS, "pairs": int(len(pairs)), "pool": "covers-shaped, T ~ U{150..650}",
       "protocol": "one process, one object; identify() once, then align_matches() on its hits: a warm-up, `reps` runs, wall seconds "
                   "around the whole call with a device synchronise on either side; with_event_clocks: one further run of "
                   "align_matches and one of serra09_pairs on the same pairs with acx_profile on",
       "identify_wall_s": round(t_identify, 4), "align_matches_wall_s": times, "align_matches_warm_up_s": round(warm, 4),
       "with_event_clocks": {"align_matches": prof_align, "serra09_pairs": prof_score},
       "locate_sweep_ms": prof_align["kernels_ms"].get("qmax_locate_kernel", {}).get("ms"),
       "score_sweep_ms": prof_score["kernels_ms"].get("qmax_bits_kernel", {}).get("ms"),
       "matches": int(hit.sum()), "no_match": int((~hit & (hits >= 0)).sum()),
       "median_query_span_frames": float(np.median((first["q_span"][hit][:, 1] - first["q_span"][hit][:, 0] + 1))) if hit.any() else None,
       "scores_equal_serra09_pairs": True}
print(json.dumps(rec), flush=True)
a.cleanup_memmap()
ctx.close()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
