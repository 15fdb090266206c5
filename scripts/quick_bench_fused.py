"""rerank_fused() -- the fused (late-fusion) score within every query's shortlist -- on one covers-shaped synthetic collection
(sets of 164 tracks / 80 works; ChenFusion: T ~ U{150..650} pooled frames, EarlyFusion: 60..100 blocks), Q = 128 queries, k = 10:

    python scripts/quick_bench_fused.py [n_tracks] [--cls ChenFusion|EarlyFusion] [--queries 128] [--k 10] [--reps 3]
                                        [--shortlists 50,100] [--out FILE] [--loop-only 1]

  leg (a)   algo.rerank_fused(queries, shortlists of S, k) for every S: Q (S + 1) S / 2 alignments, then Q fusions of S + 1
            tracks side by side (acx_query_fused_lists)
  leg (b)   the same Q fusions as Q consecutive acx_snf_fuse_dists calls on the host's distance matrices -- the export the
            whole-collection do_late_fusion runs on, one neighbourhood at a time; its pair scores (acx_*_pairs per
            neighbourhood) are computed before the clock starts and are not part of the leg

The shortlists are random tracks of the collection: the cost of either leg does not depend on which tracks a list holds.
Both legs run in one process, alternating, `reps` times each after one warm-up each; every run is reported.  One more run
of leg (a) with the library's event clocks on gives the milliseconds per kernel family (acx_profile_*): the pair kernels,
the staging kernel, the batched SNF stages and the row kernel.  The two legs must agree bit for bit on every fused row
(checked here on the rounded rows' order).  --loop-only 1 runs leg (b) alone: the script then needs nothing of this feature and
times the same fusions on a checkout of an earlier commit (copy it into that checkout's scripts/)."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd import _lib, synth  # noqa: E402
from acoss_amd import algorithms  # noqa: E402


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
CLS = _opt("--cls", "ChenFusion")
SHORTLISTS = [int(s) for s in _opt("--shortlists", "50,100").split(",")]
OUT = _opt("--out")
LOOP_ONLY = bool(int(_opt("--loop-only", 0)))
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
OUT = os.path.abspath(OUT or os.path.join(ROOT, "profiles", "fused_lists.json"))
os.makedirs(os.path.dirname(OUT), exist_ok=True)
os.chdir(tempfile.mkdtemp())
with open("ds.csv", "w") as f:
    f.write("work_id,track_id\n")
    for i in range(N):
        f.write("w%d,t%d\n" % (i // 2, i))
labels = ["w%d" % (i // 2) for i in range(N)]
rng = np.random.default_rng(2025)
queries = np.sort(rng.choice(N, size=Q, replace=False)).astype(np.int32)
SHORTLISTS = [s for s in SHORTLISTS if 21 <= s <= min(1024, N - 1)]

algo = getattr(algorithms, CLS)("ds.csv", "feat/", shortname="fused")
if CLS == "ChenFusion":
    sets = [synth.covers80_shaped(seed=100 + s, t_range=(150, 650)) for s in range((N + 163) // 164)]
    tracks = [d["frames"][d["offsets"][i]:d["offsets"][i + 1]] for d in sets for i in range(len(d["offsets"]) - 1)][:N]
    algo.set_pooled_features(tracks, labels)
else:
    tracks = [t for s in range((N + 163) // 164) for t in synth.earlyfusion_cover_set(clique_sizes=synth.COVERS80_CLIQUES, seed=100 + s)[0]][:N]
    algo.set_block_features(tracks, labels)
ctx, algo_id, params, mode, col = algo._query_call()
planes = list(algo._identify_planes)
types = list(algo._identify_fused)
# do_late_fusion's plane lists (the classes' _fused_planes, restated so that --loop-only runs on a build without them)
FUSED = {"ChenFusion": {"Late": ("qmax", "dmax")},
         "EarlyFusion": {"late": ("chromas", "ssms", "mfccs"), "early+late": ("chromas", "ssms", "mfccs", "early")}}[CLS]
assert LOOP_ONLY or dict(algo._fused_planes) == FUSED
type_planes = [[planes.index(p) for p in FUSED[t]] for t in types]


def timed(fn):
    ctx.dev_sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.dev_sync()
    return time.perf_counter() - t0, out


def lists_of(S):
    r = np.random.default_rng(S)
    return np.stack([r.choice(np.setdiff1d(np.arange(N), [q]), S, replace=False) for q in queries]).astype(np.int32)


def host_matrices(S):
    """Per query and fused type the distance matrices of its neighbourhood, built on the host from acx_*_pairs: what leg (b) fuses."""
    out = []
    for q, row in zip(queries, lists_of(S)):
        T = np.unique(np.concatenate([[q], row])).astype(np.int64)
        a, b = np.triu_indices(len(T), 1)
        pairs = np.stack([T[a], T[b]], axis=1).astype(np.int32)
        sc = ctx.chenfusion_pairs(pairs, params) if CLS == "ChenFusion" else ctx.earlyfusion_pairs(pairs, kappa=params.kappa, K=params.K)
        per_type = []
        for pl in type_planes:
            Ds = []
            for e in pl:
                Sm = np.zeros((len(T), len(T)), np.float32)
                Sm[a, b] = sc[:, e]
                Sm[b, a] = sc[:, e]
                with np.errstate(divide="ignore"):
                    D = (col[T][None, :] / Sm.astype(np.float64)).astype(np.float32).astype(np.float64) if CLS == "ChenFusion" \
                        else 1.0 / (1.0 + Sm.astype(np.float64))
                np.fill_diagonal(D, 0.0)
                Ds.append(D)
            per_type.append(Ds)
        out.append((T, int(np.searchsorted(T, q)), per_type))
    return out


legs, mats = {}, {}
for S in SHORTLISTS:
    mats[S] = host_matrices(S)
    if not LOOP_ONLY:
        legs["rerank_fused_%d" % S] = lambda S=S: algo.rerank_fused(queries, lists_of(S), k=K)
    legs["fuse_dists_loop_%d" % S] = lambda S=S: [[ctx.snf_fuse_dists(Ds, K=20, niters=20, reg_diag=1.0)[1][pos] for Ds in per_type]
                                                  for _, pos, per_type in mats[S]]
warm = {leg: timed(fn) for leg, fn in legs.items()}
for S in ([] if LOOP_ONLY else SHORTLISTS):                # the two legs compute the same rows
    got, rows = warm["rerank_fused_%d" % S][1], warm["fuse_dists_loop_%d" % S][1]
    for i, (T, pos, _) in enumerate(mats[S]):
        for t, name in enumerate(types):
            r32 = rows[i][t].astype(np.float32)
            order = np.array([c for c in np.argsort(-r32, kind="stable") if c != pos][:K])
            assert np.array_equal(got[name][0][i], T[order]) and np.array_equal(got[name][1][i].view(np.uint32), r32[order].view(np.uint32)), (S, i, name)
times = {leg: [] for leg in legs}
for _ in range(REPS):
    for leg, fn in legs.items():
        times[leg].append(round(timed(fn)[0], 4))


def profiled(fn):
    ctx.profile_enable(True)
    ctx.profile_reset()
    t, _ = timed(fn)
    prof = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in ctx.profile().items() if v["launches"]}
    ctx.profile_enable(False)
    snf = sum(v["ms"] for k, v in prof.items() if k.startswith("snf_batch_"))
    own = sum(v["ms"] for k, v in prof.items() if k.startswith("snf_batch_") or k.startswith("fused_"))
    total = sum(v["ms"] for v in prof.values())
    return {"wall_s": round(t, 4), "kernels_ms": prof, "pair_kernels_ms": round(total - own, 3), "snf_stages_ms": round(snf, 3),
            "pair_share_of_kernel_ms": round((total - own) / total, 4) if total else None, "snf_share_of_kernel_ms": round(snf / total, 4) if total else None}


rec = {"class": CLS, "loop_only": LOOP_ONLY, "n_tracks": N, "queries": Q, "k": K, "reps": REPS, "fused_types": types, "snf": {"K": 20, "niters": 20},
       "pool": "covers-shaped; ChenFusion T ~ U{150..650} pooled frames, EarlyFusion 60..100 blocks; random shortlists",
       "protocol": "one process, one object; a warm-up of each leg, then the legs alternating; wall seconds around the whole call with a "
                   "device synchronise on either side; fuse_dists_loop: Q consecutive acx_snf_fuse_dists calls per fused type on host "
                   "matrices prepared before the clock starts (their pair scores are not in the leg); with_event_clocks: one further run "
                   "of rerank_fused with acx_profile on",
       "alignments_per_call": {str(S): int(Q * (S + 1) * S // 2) for S in SHORTLISTS},
       "wall_s": times, "warm_up_s": {leg: round(warm[leg][0], 4) for leg in legs},
       "with_event_clocks": {"rerank_fused_%d" % S: profiled(legs["rerank_fused_%d" % S]) for S in ([] if LOOP_ONLY else SHORTLISTS)}}
print(json.dumps(rec), flush=True)
algo.cleanup_memmap()
with open(OUT, "w") as f:
    json.dump(rec, f, indent=1)
print("wrote", OUT)
