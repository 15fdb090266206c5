"""What the matrix profile's index costs: acx_simple_profile (records alone, and with the profiles) beside acx_simple_pairs on the
same pair lists, on a pool of bench_other.simple_leg's shape (tracks of 12 x 150..250 pooled frames, Simple.smooth'ed).

    python scripts/quick_bench_simple_profile.py [n_pairs] [--tracks 1536] [--sslen 10] [--reps 5]

The three calls alternate `reps` times after one warm-up each (the same list, ordered pairs drawn at random); a time is wall
seconds around the call with a device synchronise on either side, so it includes the host's sort, the copies of the results and,
with profiles, of 12 bytes per row.  One further run of each with the library's event clocks on (acx_profile_*) gives the
kernels' own milliseconds: simple_kernel beside simple_profile_kernel.  The scores of all three must be the same bits, which the
script asserts.  Prints one JSON line; writes nothing."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd import _lib  # noqa: E402
from acoss_amd.algorithms.simple_silva import Simple  # noqa: E402


def _opt(name, default=None):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    v = sys.argv[k + 1]
    del sys.argv[k:k + 2]
    return v


TRACKS = int(_opt("--tracks", 1536))
SSLEN = int(_opt("--sslen", 10))
REPS = int(_opt("--reps", 5))
K = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
rng = np.random.default_rng(0)
tm = [np.ascontiguousarray(Simple.smooth(None, rng.random((12, int(rng.integers(150, 251))))).T) for _ in range(TRACKS)]
na = np.array([len(t) for t in tm])
offs = np.concatenate([[0], np.cumsum(na)]).astype(np.int64)
pairs = rng.integers(0, TRACKS, (K, 2)).astype(np.int32)
pairs[:, 1] = np.where(pairs[:, 1] == pairs[:, 0], (pairs[:, 1] + 1) % TRACKS, pairs[:, 1])
ctx = _lib.Context(0)
ctx.upload_pool_f64(np.concatenate(tm), offs)


def timed(fn):
    ctx.dev_sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.dev_sync()
    return time.perf_counter() - t0, out


legs = {"simple_pairs": lambda: ctx.simple_pairs(pairs, SSLEN),
        "profile_records": lambda: ctx.simple_profile(pairs, SSLEN),
        "profile_with_profiles": lambda: ctx.simple_profile(pairs, SSLEN, profiles=True)}
ref = None
for name, fn in legs.items():                      # warm-up: code objects, window norms, buffers
    _, out = timed(fn)
    score = out if name == "simple_pairs" else (out["score"] if name == "profile_records" else out[0]["score"])
    ref = score if ref is None else ref
    assert np.array_equal(np.asarray(score).view(np.uint64), np.asarray(ref).view(np.uint64)), "%s: other score bits" % name
wall = {name: [] for name in legs}
for _ in range(REPS):
    for name, fn in legs.items():
        wall[name].append(round(timed(fn)[0], 4))
kern = {}
ctx.profile_enable(True)
for name, fn in legs.items():
    ctx.profile_reset()
    fn()
    kern[name] = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in ctx.profile().items() if v["launches"]}
ctx.profile_enable(False)
med = {name: float(np.median(t)) for name, t in wall.items()}
k_pairs = kern["simple_pairs"]["simple_kernel"]["ms"]
rows = int((na[pairs[:, 0]] - SSLEN + 1).sum())
cells = float(((na[pairs[:, 0]] - SSLEN + 1).astype(np.float64) * (na[pairs[:, 1]] - SSLEN + 1)).sum())
rec = {"pairs": K, "tracks": TRACKS, "sslen": SSLEN, "reps": REPS, "profile_rows": rows, "cells": cells,
       "pool": "Simple.smooth'ed random chroma, 12 x U{150..250} pooled frames per track",
       "wall_s": wall, "wall_median_s": med, "kernels_ms": kern,
       "kernel_ratio_records": round(kern["profile_records"]["simple_profile_kernel"]["ms"] / k_pairs, 3),
       "kernel_ratio_with_profiles": round(kern["profile_with_profiles"]["simple_profile_kernel"]["ms"] / k_pairs, 3),
       "wall_ratio_records": round(med["profile_records"] / med["simple_pairs"], 3),
       "wall_ratio_with_profiles": round(med["profile_with_profiles"] / med["simple_pairs"], 3),
       "gcells_per_s_simple_kernel": round(cells / k_pairs / 1e6, 1),
       "timing": "wall: perf_counter around the call with acx_dev_sync on either side, legs alternating; kernels_ms: one further "
                 "run per leg with acx_profile on", "score_bits_equal": True}
print(json.dumps(rec), flush=True)
ctx.close()
