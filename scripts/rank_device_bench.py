"""getEvalStatistics on the host against the device engine, and top_matches against np.argsort, on ONE finished score
matrix in the Da-TACOS shape: N tracks = N / 15 cliques of 13 + 2 N / 15 singletons (15 000: 1 000 + 2 000), one float32
memmap as all_pairwise leaves it (uniform scores rounded to 4 decimals: ties in every row; covers 0.2 higher).

    python scripts/rank_device_bench.py [n_tracks] [--reps 3] [--no-topk] [--out FILE]     (FILE: the JSON record; default
                                                                               rank_device_<n>.json where the script was started)
    python scripts/rank_device_bench.py [n_tracks] --device-only              (one warm-up + one timed device evaluation and
                                                                               one top_matches: the run to put under a tracer)

Both engines run in one process, alternating, `reps` times each after one warm-up each; the device engine's timed
region ends with a device synchronise.  The host engine is eval_statistics as it is (counting branch for cliques of 13)."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd.algorithms.algorithm_template import CoverAlgorithm  # noqa: E402


def _opt(name, default=None, flag=False):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    if flag:
        del sys.argv[k]
        return True
    v = sys.argv[k + 1]
    del sys.argv[k:k + 2]
    return v


REPS = int(_opt("--reps", 3))
TOPK = not _opt("--no-topk", False, flag=True)
DEVICE_ONLY = _opt("--device-only", False, flag=True)
OUT = _opt("--out")
N = int(sys.argv[1]) if len(sys.argv) > 1 else 15000
OUT = os.path.abspath(OUT or "rank_device_%d.json" % N)             # (before the chdir below)
n_cl = N // 15
rng = np.random.default_rng(2024)
perm = rng.permutation(N)
labels = np.empty(N, dtype=object)
for c in range(n_cl):
    labels[perm[13 * c:13 * c + 13]] = "w%d" % c
for t in perm[13 * n_cl:]:
    labels[t] = "s%d" % t
os.makedirs(os.path.dirname(OUT), exist_ok=True)
os.chdir(tempfile.mkdtemp())
with open("ds.csv", "w") as f:
    f.write("work_id,track_id\n")
    for i, l in enumerate(labels):
        f.write("%s,t%d\n" % (l, i))


class Scores(CoverAlgorithm):
    """A user subclass without any device code: the matrix is filled below."""

    def __init__(self):
        CoverAlgorithm.__init__(self, "ds.csv", name="Scores", datapath="feat/", shortname="rank")


alg = Scores()
for i, l in enumerate(labels):
    alg._register_label(i, l)
D = alg.Ds["main"]
work = {l: k for k, l in enumerate(dict.fromkeys(labels))}
wid = np.array([work[l] for l in labels])
for a in range(0, N, 1024):
    b = min(N, a + 1024)
    blk = rng.random((b - a, N), dtype=np.float32)
    blk += 0.2 * (wid[a:b, None] == wid[None, :])
    D[a:b] = np.round(blk, 4)
D.flush()
ctx = alg._rank_context()


def run(engine):
    t0 = time.perf_counter()
    res = alg.getEvalStatistics("main", engine=engine)
    if engine == "device":
        ctx.dev_sync()
    return time.perf_counter() - t0, res


def run_topk():
    t0 = time.perf_counter()
    out = alg.top_matches("main", k=10)
    ctx.dev_sync()
    return time.perf_counter() - t0, out


if DEVICE_ONLY:
    run("device")
    t, res = run("device")
    tk, _ = run_topk()
    print(json.dumps({"n_tracks": N, "device_s": round(t, 4), "top_matches_k10_s": round(tk, 4), "MAP": res[3]}))
    alg.cleanup_memmap()
    ctx.close()
    sys.exit(0)

times = {"host": [], "device": []}
first = {e: run(e) for e in ("host", "device")}                      # warm-up: page cache, pinned slots, code objects
for _ in range(REPS):
    for e in ("host", "device"):
        t, res = run(e)
        times[e].append(t)
        assert tuple(res[:4]) == tuple(first["host"][1][:4]) and np.array_equal(res[4], first["host"][1][4]), (e, res, first["host"][1])
ctx.profile_enable(True)
ctx.profile_reset()
t_prof, _ = run("device")
prof = ctx.profile()
ctx.profile_enable(False)
rec = {"workload": "%d tracks: %d cliques of 13 + %d singletons, one float32 memmap of %d MB; getEvalStatistics('main'), "
                   "engine host against engine device in one process, alternating, %d repetitions each after a warm-up"
                   % (N, n_cl, N - 13 * n_cl, N * N * 4 >> 20, REPS),
       "getEvalStatistics_s": {e: {"runs": [round(t, 4) for t in v], "median": round(float(np.median(v)), 4), "min": round(min(v), 4),
                                   "max": round(max(v), 4)} for e, v in times.items()},
       "warm_up_s": {e: round(first[e][0], 4) for e in first},
       "host_over_device_median": round(float(np.median(times["host"]) / np.median(times["device"])), 2),
       "device_run_with_event_timing": {"wall_s": round(t_prof, 4),
                                        "rank_columns_kernel_ms": round(prof["rank_columns_kernel"]["ms"], 3),
                                        "launches": prof["rank_columns_kernel"]["launches"]},
       "stats": {"MR": first["host"][1][0], "MRR": first["host"][1][1], "MDR": first["host"][1][2], "MAP": first["host"][1][3],
                 "tops": [float(v) for v in first["host"][1][4]]},
       "engines_agree_exactly": True}
if TOPK:
    run_topk()
    tk = [run_topk() for _ in range(REPS)]
    t0 = time.perf_counter()
    Dh = np.array(D)
    np.fill_diagonal(Dh, -np.inf)                                   # (finite scores: the track itself sorts last)
    want = np.argsort(-Dh, axis=1, kind="stable")[:, :10].astype(np.int32)
    t_np = time.perf_counter() - t0
    assert np.array_equal(tk[-1][1][0], want)
    ctx.profile_enable(True)
    ctx.profile_reset()
    run_topk()
    prof = ctx.profile()
    ctx.profile_enable(False)
    rec["top_matches_k10"] = {"device_s": [round(t, 4) for t, _ in tk], "numpy_stable_argsort_s": round(t_np, 3),
                              "topk_rows_kernel_ms": round(prof["topk_rows_kernel"]["ms"], 3), "lists_equal": True}
print(json.dumps(rec))
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
alg.cleanup_memmap()
ctx.close()
