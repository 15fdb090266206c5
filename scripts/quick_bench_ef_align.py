"""EarlyFusion.align_match_paths() on the hits of identify(): where every match lies and its path, for Q queries and k hits each on
a cover-structured block-feature pool (synth.earlyfusion_cover_set: works of `versions` versions, nb ~ U{300..500} blocks).

    python scripts/quick_bench_ef_align.py [n_works] [--versions 4] [--queries 32] [--k 10] [--reps 3] [--type early] [--long]

identify() runs once; align_match_paths(queries, hits) runs `reps` times after one warm-up, wall seconds around the call with a
device synchronise on either side, and align_matches on the same hits beside it.  One further run with the library's event clocks
on (acx_profile_*) gives the alignment pass's milliseconds (ef_align_kernel: the i32 DP with its direction plane and the traceback,
a chain of at most min(M, N) dependent loads per pair) beside the score kernel's on the same pairs (sw_kernel's entry:
sw_bits_h16_kernel, all four planes) and the rest of the chain.  The records must be align_matches' bytes, which the script
asserts.  --long: nb ~ U{900..1300}, so that tracks of more than 1024 blocks stand in the hit lists and align_match_paths takes
acx_ef_align_long (the float path and ef_align_long_kernel beside sw_long_kernel).  Prints one JSON line;
writes nothing."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd import synth  # noqa: E402
from acoss_amd.algorithms import EarlyFusion  # noqa: E402


def _opt(name, default=None):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    v = sys.argv[k + 1]
    del sys.argv[k:k + 2]
    return v


VERSIONS = int(_opt("--versions", 4))
Q = int(_opt("--queries", 32))
K = int(_opt("--k", 10))
REPS = int(_opt("--reps", 3))
TYPE = _opt("--type", "early")
LONG = "--long" in sys.argv
if LONG:
    sys.argv.remove("--long")
NB = (900, 1300) if LONG else (300, 500)
WORKS = int(sys.argv[1]) if len(sys.argv) > 1 else 16
tracks, labels = synth.earlyfusion_cover_set(n_works=WORKS, versions=VERSIONS, seed=2026, nb_range=NB)
N = len(tracks)
os.chdir(tempfile.mkdtemp())
with open("ds.csv", "w") as f:
    f.write("work_id,track_id\n")
    for i in range(N):
        f.write("%s,t%d\n" % (labels[i], i))
rng = np.random.default_rng(2026)
queries = np.sort(rng.choice(N, size=min(Q, N), replace=False)).astype(np.int64)
a = EarlyFusion("ds.csv", "feat/", shortname="efalign")
a.set_block_features(tracks, labels)
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


t_identify, (hits, _) = timed(lambda: a.identify(queries, k=K)[TYPE])
warm, (first, paths) = timed(lambda: a.align_match_paths(queries, hits, similarity_type=TYPE))
times, times_plain = [], []
for _ in range(REPS):
    t, (got, got_paths) = timed(lambda: a.align_match_paths(queries, hits, similarity_type=TYPE))
    times.append(round(t, 4))
    assert got.tobytes() == first.tobytes() and all(np.array_equal(x, y) for r, s in zip(got_paths, paths) for x, y in zip(r, s))
    t, plain = timed(lambda: a.align_matches(queries, hits, similarity_type=TYPE))
    times_plain.append(round(t, 4))
    assert plain.tobytes() == first.tobytes(), "align_match_paths' records are align_matches' bytes"
prof, _ = profiled(lambda: a.align_match_paths(queries, hits, similarity_type=TYPE))
hit = first["q0"] >= 0
lengths = np.array([len(p) for row in paths for p in row if len(p)])
rec = {"n_tracks": N, "queries": len(queries), "k": K, "reps": REPS, "type": TYPE, "pairs": int((hits >= 0).sum()),
       "pool": "earlyfusion_cover_set, %d works x %d versions, nb ~ U{%d..%d}" % ((WORKS, VERSIONS) + NB),
       "identify_wall_s": round(t_identify, 4), "align_match_paths_wall_s": times, "align_matches_wall_s": times_plain,
       "align_match_paths_warm_up_s": round(warm, 4), "with_event_clocks": prof,
       "align_pass_ms": prof["kernels_ms"].get("ef_align_kernel", {}).get("ms"),
       "align_pass_launches": prof["kernels_ms"].get("ef_align_kernel", {}).get("launches"),
       "align_long_pass_ms": prof["kernels_ms"].get("ef_align_long_kernel", {}).get("ms"),
       "align_long_pass_launches": prof["kernels_ms"].get("ef_align_long_kernel", {}).get("launches"),
       "score_kernel_ms": prof["kernels_ms"].get("sw_kernel", {}).get("ms"),
       "matches": int(hit.sum()),
       "median_path_cells": float(np.median(lengths)) if len(lengths) else None, "max_path_cells": int(lengths.max()) if len(lengths) else None,
       "records_equal_align_matches": True}
print(json.dumps(rec), flush=True)
a.cleanup_memmap()
ctx.close()
