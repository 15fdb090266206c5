"""The full cross-diffusion early fusion (Context.ef_crossfusion) on PAIRS pairs of covers-shaped tracks:
a cover-structured block-feature pool (synth.earlyfusion_cover_set, block counts drawn as bench_other.py's EarlyFusion leg draws
them: nb ~ U{300..500}), every pair two different tracks, half of them two versions of one work.

    python scripts/quick_bench_crossfusion.py [pairs] [--works 16] [--versions 4] [--reps 3] [--niters 5] [--K 10] [--out profiles/crossfusion_256.json]

The list runs `reps` times after one warm-up, wall seconds around the call with a device synchronise on either side; the `early`
plane's rate (Context.earlyfusion_pairs) on the same pairs beside it.  One further run with the library's event clocks on
(acx_profile_*) gives the per-kernel milliseconds: the GEMMs and the statistics of the three pairs (A, B), (A, A), (B, B) a pair
costs, the new kernels (xf_*: means, affinities with the two getW blocks, the SNF lists and loop, X, the selection) and the
Smith-Waterman.  Prints one JSON line and writes it to --out."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acoss_amd import _lib, synth  # noqa: E402


def _opt(name, default=None):
    if name not in sys.argv:
        return default
    k = sys.argv.index(name)
    v = sys.argv[k + 1]
    del sys.argv[k:k + 2]
    return v


WORKS = int(_opt("--works", 16))
VERSIONS = int(_opt("--versions", 4))
REPS = int(_opt("--reps", 3))
NITERS = int(_opt("--niters", 5))
K = int(_opt("--K", 10))
OUT = _opt("--out", os.path.join(ROOT, "profiles", "crossfusion_256.json"))
PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 256
KAPPA = 0.1

tracks, labels = synth.earlyfusion_cover_set(n_works=WORKS, versions=VERSIONS, seed=2026, nb_range=(300, 500))
N = len(tracks)
rng = np.random.default_rng(2026)
pairs = []
while len(pairs) < PAIRS:
    i = int(rng.integers(0, N))
    same = [t for t in range(N) if labels[t] == labels[i] and t != i]
    j = int(rng.choice(same)) if len(pairs) % 2 == 0 and same else int(rng.integers(0, N))
    if i != j:
        pairs.append((i, j))
pairs = np.array(pairs, np.int32)
ctx = _lib.Context(0)
ctx.ef_upload_pool(tracks)
blocks = np.asarray(ctx.ef_blocks)


def timed(fn):
    ctx.dev_sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.dev_sync()
    return time.perf_counter() - t0, out


full = lambda: ctx.ef_crossfusion(pairs, kappa=KAPPA, K=K, niters=NITERS)      # noqa: E731
early = lambda: ctx.earlyfusion_pairs(pairs, kappa=KAPPA, K=K)                  # noqa: E731
warm, first = timed(full)
timed(early)
t_full, t_early = [], []
for _ in range(REPS):
    t, got = timed(full)
    assert np.array_equal(got, first)
    t_full.append(round(t, 4))
    t, e = timed(early)
    t_early.append(round(t, 4))
ctx.profile_enable(True)
ctx.profile_reset()
t_prof, _ = timed(full)
prof = {k: {"ms": round(v["ms"], 3), "launches": v["launches"]} for k, v in ctx.profile().items() if v["launches"]}
ctx.profile_enable(False)
same_work = np.array([labels[i] == labels[j] for i, j in pairs])
rec = {
    "what": "Context.ef_crossfusion on %d pairs of a cover-structured pool (%d tracks, %d-%d blocks), K = %d, niters = %d, kappa = %g"
            % (len(pairs), N, blocks.min(), blocks.max(), K, NITERS, KAPPA),
    "pairs": int(len(pairs)), "mean_n": float(np.mean(blocks[pairs[:, 0]] + blocks[pairs[:, 1]])),
    "warmup_s": round(warm, 4), "full_fusion_s": t_full, "full_fusion_pairs_per_s": round(len(pairs) / float(np.median(t_full)), 1),
    "ms_per_pair": round(1e3 * float(np.median(t_full)) / len(pairs), 3),
    "early_plane_s": t_early, "early_plane_pairs_per_s": round(len(pairs) / float(np.median(t_early)), 1),
    "profiled_run": {"wall_s": round(t_prof, 4), "kernels_ms": prof},
    "mean_score": {"same_work": {"full": float(first[same_work].mean()), "early": float(e[same_work, 3].mean())},
                   "other_work": {"full": float(first[~same_work].mean()), "early": float(e[~same_work, 3].mean())}},
}
ctx.close()
line = json.dumps(rec)
print(line)
if OUT:
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write(line + "\n")
