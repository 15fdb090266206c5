"""ChenFusion.align_match_paths(similarity_type="dmax") on the hits of identify(): the Dmax alignment and its PATH for Q = 128 queries
and k = 10 hits each (1 280 pairs) on the covers-shaped pool of quick_bench_identify.py (sets of 164 tracks / 80 works, T ~ U{150..650}
pooled frames), beside the Qmax alignment of the same hits.

    python scripts/quick_bench_dmax_align.py [n_tracks] [--queries 128] [--k 10] [--reps 3] [--out FILE]

identify() runs once, on the `dmax` list; align_match_paths(queries, hits, "dmax") runs `reps` times after one warm-up, wall seconds
around the call with a device synchronise on either side, and the same call with "qmax" beside it.  One further run of each with the
library's event clocks on (acx_profile_*) gives dmax_locate_kernel / dmax_path_kernel beside qmax_locate_kernel / qmax_path_kernel.
The Dmax records must be align_matches(..., "dmax")'s bytes and their scores chenfusion_pairs' Dmax column, which the script asserts;
it also counts the gap starts among the first 64 hits, read off the device's own plots.  Writes profiles/dmax_align_<n>.json."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd import synth  # noqa: E402
from acoss_amd.algorithms import ChenFusion  # noqa: E402


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
OUT = os.path.abspath(OUT or os.path.join(ROOT, "profiles", "dmax_align_%d.json" % N))
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
a = ChenFusion("ds.csv", "feat/", shortname="dmaxalign")
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


t_identify, (hits, _) = timed(lambda: a.identify(queries, k=K)["dmax"])
warm, (first, paths) = timed(lambda: a.align_match_paths(queries, hits, similarity_type="dmax"))
times, times_qmax = [], []
for _ in range(REPS):
    t, (got, got_paths) = timed(lambda: a.align_match_paths(queries, hits, similarity_type="dmax"))
    times.append(round(t, 4))
    assert np.array_equal(got, first) and all(np.array_equal(x, y) for r, s in zip(got_paths, paths) for x, y in zip(r, s))
    t, _ = timed(lambda: a.align_match_paths(queries, hits, similarity_type="qmax"))
    times_qmax.append(round(t, 4))
assert a.align_matches(queries, hits, similarity_type="dmax").tobytes() == first.tobytes(), "align_match_paths' records are align_matches' bytes"
rows, slots = np.nonzero(hits >= 0)
pairs = np.stack([queries[rows], hits[rows, slots]], axis=1).astype(np.int32)
assert np.array_equal(first["score"][rows, slots], ctx.chenfusion_pairs(pairs, a._params())[:, 1]), "the scores are chenfusion_pairs' Dmax column"
prof_d, _ = profiled(lambda: a.align_match_paths(queries, hits, similarity_type="dmax"))
prof_q, (qfirst, _) = profiled(lambda: a.align_match_paths(queries, hits, similarity_type="qmax"))
hit = first["q0"] >= 0
_, plots = ctx.serra09_debug_bits(pairs[:64], a._params())       # the starts of the first 64 hits, read off the device's own plots
al64 = first[rows[:64], slots[:64]]
gap_starts = int(sum(1 for r, R in zip(al64, plots) if r["q0"] >= 0 and R[r["q0"], r["r0"]] == 0))
lengths = np.array([len(p) for row in paths for p in row if len(p)])
box = (first["q1"][hit] - first["q0"][hit] + 1).astype(np.int64) * (first["r1"][hit] - first["r0"][hit] + 1)


def ms(prof, name):
    return prof["kernels_ms"].get(name, {}).get("ms")


rec = {"n_tracks": N, "queries": Q, "k": K, "reps": REPS, "pairs": int((hits >= 0).sum()), "pool": "covers-shaped, T ~ U{150..650}",
       "protocol": "one process, one object; identify() once, then align_match_paths(similarity_type='dmax') on its dmax hits: a warm-up, "
                   "`reps` runs, wall seconds around the whole call with a device synchronise on either side, the 'qmax' call on the same "
                   "hits after each; with_event_clocks: one further run of each with acx_profile on",
       "identify_wall_s": round(t_identify, 4), "dmax_align_match_paths_wall_s": times, "qmax_align_match_paths_wall_s": times_qmax,
       "warm_up_s": round(warm, 4), "with_event_clocks": {"dmax": prof_d, "qmax": prof_q},
       "dmax_locate_ms": ms(prof_d, "dmax_locate_kernel"), "qmax_locate_ms": ms(prof_q, "qmax_locate_kernel"),
       "dmax_path_ms": ms(prof_d, "dmax_path_kernel"), "qmax_path_ms": ms(prof_q, "qmax_path_kernel"),
       "matches": int(hit.sum()), "records_that_differ_from_qmax": int(np.sum(first[hit] != qfirst[hit])),
       "gap_starts_among_the_first_64": gap_starts, "box_cells": int(box.sum()),
       "median_path_cells": float(np.median(lengths)) if len(lengths) else None, "max_path_cells": int(lengths.max()) if len(lengths) else None,
       "records_equal_align_matches": True}
print(json.dumps(rec), flush=True)
a.cleanup_memmap()
ctx.close()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
