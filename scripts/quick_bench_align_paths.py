"""align_match_paths() on the hits of identify(): the PATH of every match, for Q = 128 queries and k = 10 hits each (1 280 pairs) on
the covers-shaped pool of quick_bench_identify.py (sets of 164 tracks / 80 works, T ~ U{150..650} pooled frames).

    python scripts/quick_bench_align_paths.py [n_tracks] [--queries 128] [--k 10] [--reps 3] [--out FILE]

identify() runs once; align_match_paths(queries, hits) runs `reps` times after one warm-up, wall seconds around the call with a
device synchronise on either side, and align_matches on the same hits beside it.  One further run with the library's event clocks
on (acx_profile_*) gives the path pass's milliseconds (qmax_path_kernel: the box DP and the traceback, a chain of at most
min(h, w) dependent loads per pair) beside the locating sweep's (qmax_locate_kernel).  The records must be align_matches' bytes,
which the script asserts.  Writes profiles/align_paths_<n>.json."""
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
OUT = os.path.abspath(OUT or os.path.join(ROOT, "profiles", "align_paths_%d.json" % N))
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
a = Serra09("ds.csv", "feat/", shortname="alignpaths")
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
warm, (first, paths) = timed(lambda: a.align_match_paths(queries, hits))
times, times_plain = [], []
for _ in range(REPS):
    t, (got, got_paths) = timed(lambda: a.align_match_paths(queries, hits))
    times.append(round(t, 4))
    assert np.array_equal(got, first) and all(np.array_equal(x, y) for r, s in zip(got_paths, paths) for x, y in zip(r, s))
    t, plain = timed(lambda: a.align_matches(queries, hits))
    times_plain.append(round(t, 4))
    assert plain.tobytes() == first.tobytes(), "align_match_paths' records are align_matches' bytes"
prof, _ = profiled(lambda: a.align_match_paths(queries, hits))
hit = first["q0"] >= 0
lengths = np.array([len(p) for row in paths for p in row if len(p)])
box = (first["q1"][hit] - first["q0"][hit] + 1).astype(np.int64) * (first["r1"][hit] - first["r0"][hit] + 1)
rec = {"n_tracks": N, "queries": Q, "k": K, "reps": REPS, "pairs": int((hits >= 0).sum()), "pool": "covers-shaped, T ~ U{150..650}",
       "protocol": "one process, one object; identify() once, then align_match_paths() on its hits: a warm-up, `reps` runs, wall "
                   "seconds around the whole call with a device synchronise on either side, align_matches() on the same hits after "
                   "each; with_event_clocks: one further run of align_match_paths with acx_profile on",
       "identify_wall_s": round(t_identify, 4), "align_match_paths_wall_s": times, "align_matches_wall_s": times_plain,
       "align_match_paths_warm_up_s": round(warm, 4), "with_event_clocks": prof,
       "path_pass_ms": prof["kernels_ms"].get("qmax_path_kernel", {}).get("ms"),
       "path_pass_launches": prof["kernels_ms"].get("qmax_path_kernel", {}).get("launches"),
       "locate_sweep_ms": prof["kernels_ms"].get("qmax_locate_kernel", {}).get("ms"),
       "matches": int(hit.sum()), "box_cells": int(box.sum()),
       "median_path_cells": float(np.median(lengths)) if len(lengths) else None, "max_path_cells": int(lengths.max()) if len(lengths) else None,
       "records_equal_align_matches": True}
print(json.dumps(rec), flush=True)
a.cleanup_memmap()
ctx.close()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
