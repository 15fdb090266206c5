"""identify_cascade() -- an FTM2D shortlist reranked by Serra09 -- against identify() over the whole collection, on one
covers-shaped synthetic collection (bench_other.py's covers leg: sets of 164 tracks / 80 works, T ~ U{150..650} pooled
frames), Q = 128 queries, k = 10:

    python scripts/quick_bench_rerank.py [n_tracks] [--queries 128] [--k 10] [--reps 3] [--shortlists 50,200,1000] [--out FILE]

  leg (a)   serra09.identify(queries, k): Q (N - 1) alignments
  leg (b)   serra09.identify_cascade(ftm2d, queries, k, shortlist=S) for every S: Q N FTM2D cells, then Q S alignments

Both objects hold the same tracks: the FTM2D shingles are computed on the device from the pooled chroma with a beat every
second frame and WIN = 20 (the shortest track has 75 such beats).  Both legs run in one process, alternating, `reps` times
each after one warm-up each; every run is reported.  One more run of each with the library's event clocks on gives the
per-kernel-family milliseconds (acx_profile_*).  overlap_with_full: the mean share of leg (a)'s top-k that leg (b)
returns -- a property of the two ALGORITHMS on this synthetic data, reported, never gated."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd import _lib, synth  # noqa: E402
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
SHORTLISTS = [int(s) for s in _opt("--shortlists", "50,200,1000").split(",")]
OUT = _opt("--out")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 15000
WIN = 20
OUT = os.path.abspath(OUT or os.path.join(ROOT, "profiles", "rerank_%d.json" % N))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
os.chdir(tempfile.mkdtemp())
with open("ds.csv", "w") as f:
    f.write("work_id,track_id\n")
    for i in range(N):
        f.write("w%d,t%d\n" % (i // 2, i))
labels = ["w%d" % (i // 2) for i in range(N)]
rng = np.random.default_rng(2025)
queries = np.sort(rng.choice(N, size=Q, replace=False)).astype(np.int64)
SHORTLISTS = [s for s in SHORTLISTS if s <= min(1024, N - 1)]

sets = [synth.covers80_shaped(seed=100 + s, t_range=(150, 650)) for s in range((N + 163) // 164)]
tracks = [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for d in sets for i in range(len(d["offsets"]) - 1)][:N]
second = Serra09("ds.csv", "feat/", shortname="rerank")
second.set_pooled_features(tracks, labels)
side = _lib.Context(0)
side.ftm2d_upload_raw_pool([dict(chroma=t, onsets=np.arange(0, len(t), 2, dtype=np.int64)) for t in tracks], win=WIN)
shingles = side.ftm2d_download_shingles()
side.close()
first = FTM2D("ds.csv", "feat/", shortname="rerank", WIN=WIN)
first.set_features(list(shingles), labels)
ctxs = [second._context(), first._context()]


def sync():
    for c in ctxs:
        c.dev_sync()


def timed(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return time.perf_counter() - t0, out


def profiled(fn):
    for c in ctxs:
        c.profile_enable(True)
        c.profile_reset()
    t, _ = timed(fn)
    prof = {}
    for c in ctxs:
        for k, v in c.profile().items():
            if v["launches"]:
                prof[k] = {"ms": round(prof.get(k, {}).get("ms", 0.0) + v["ms"], 3), "launches": prof.get(k, {}).get("launches", 0) + v["launches"]}
        c.profile_enable(False)
    return {"wall_s": round(t, 4), "kernels_ms": prof}


legs = {"identify_all": lambda: second.identify(queries, k=K)["main"]}
for S in SHORTLISTS:
    legs["cascade_%d" % S] = lambda S=S: second.identify_cascade(first, queries, k=K, shortlist=S)["main"]
warm = {leg: timed(fn) for leg, fn in legs.items()}
full = warm["identify_all"][1][0]
times = {leg: [] for leg in legs}
for _ in range(REPS):
    for leg, fn in legs.items():
        t, got = timed(fn)
        times[leg].append(round(t, 4))
        assert np.array_equal(got[0], warm[leg][1][0]), leg        # (a leg repeats itself)
overlap = {leg: round(float(np.mean([len(set(full[i]) & set(warm[leg][1][0][i])) / float(K) for i in range(Q)])), 4) for leg in legs}
rec = {"n_tracks": N, "queries": Q, "k": K, "reps": REPS, "ftm2d_win": WIN,
       "pool": "covers-shaped, T ~ U{150..650}; FTM2D shingles of the same tracks, a beat every second frame",
       "protocol": "one process, one Serra09 and one FTM2D object over the same tracks; a warm-up of each leg, then the legs "
                   "alternating; wall seconds around the whole call with a device synchronise on either side; kernels_ms: one "
                   "further run per leg with acx_profile on; overlap_with_full: mean share of identify_all's top-k in the leg's",
       "alignments_per_leg": {leg: int(Q * (N - 1)) if leg == "identify_all" else int(Q * int(leg.split("_")[1])) for leg in legs},
       "wall_s": times, "warm_up_s": {leg: round(warm[leg][0], 4) for leg in legs},
       "with_event_clocks": {leg: profiled(fn) for leg, fn in legs.items()},
       "overlap_with_full": overlap}
print(json.dumps(rec), flush=True)
second.cleanup_memmap()
first.cleanup_memmap()
for c in ctxs:
    c.close()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
